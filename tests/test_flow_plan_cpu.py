"""The host-only plan of the register-flow block kernel (csrc/ssdk_flow_plan.h): how launch_mbflow cuts a map into 16-lane
column strips and into row segments.  The header is plain C++; this file compiles it into a stand-alone program (its own
main, g++, AddressSanitizer + UBSan), lets it print the plan as numbers and judges those numbers here:

  columns   every column 0 .. W - 1 of a map is stored by exactly one (strip, lane), no stored lane lies outside the map, a
            stored lane 0 is column 0 and a stored lane 15 is column W - 1 (their missing neighbour is the zero padding: the
            DPP row shift hands them 0), every other stored lane has both neighbours in its strip;
  rows      the segments tile rows 0 .. Ho - 1 exactly once, the row loop runs at least the rows a segment needs, and the full
            segments run no surplus row (stride 2: one, the least there is) wherever such a length exists.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ssds.pytorch_amd", "csrc")
WMAX = HMAX = 300
KINDS = {"pair": (1, 1, 4), "s1": (1, 0, 6), "s2": (2, 0, 4)}  # name -> stride, row pairs, rows per trip of the row loop
PER_ROW = (3, 40, 576, 640, 5000)                               # N * groups: forced small maps ... more than any bench map
SIMDS = 1024                                                    # 256 CUs

PROGRAM = r"""
#include <cstdio>
#include "ssdk_flow_plan.h"
using namespace ssdk;
int main() {
  for (int layout = kFlowHalo; layout <= kFlowEdge; ++layout)
    for (int W = 1; W <= %(wmax)d; ++W) {
      const int strips = flow_strips(layout, W);
      std::printf("C %%d %%d %%d", layout, W, strips);
      for (int k = 0; k < strips; ++k) {
        unsigned mask = 0;
        for (int lane = 0; lane < kFlowLanes; ++lane) mask |= flow_lane_stores(layout, k, lane, W) ? 1u << lane : 0u;
        std::printf(" %%d:%%u", flow_strip_col0(layout, k), mask);
      }
      std::printf("\n");
    }
  const int kinds[3][2] = {{1, 1}, {1, 0}, {2, 0}};
  const long per_row[] = {%(per_row)s};
  for (auto& kd : kinds)
    for (long pr : per_row)
      for (int forced = 0; forced < 2; ++forced)
        for (int Ho = 1; Ho <= %(hmax)d; ++Ho) {
          const FlowRows r = flow_plan_rows(pr, Ho, kd[0], kd[1] != 0, forced != 0, %(simds)d);
          std::printf("R %%d %%d %%ld %%d %%d %%d %%d %%ld %%d", kd[0], kd[1], pr, forced, Ho, r.rs, r.segs, r.items,
                      flow_row_step(kd[0], kd[1] != 0));
          for (int s = 0; s < r.segs; ++s) {
            const int n = flow_seg_rows(Ho, r.rs, s);
            std::printf(" %%d:%%d:%%d:%%d", flow_seg_first(r.rs, s), n, flow_rows_needed(kd[0], n), flow_rows_run(kd[0], kd[1] != 0, n));
          }
          std::printf("\n");
        }
  for (long pr : per_row)  // the stem instances: 64 / 32 / 16 (forced: / 8) rows on the stride-1 loop
    for (int forced = 0; forced < 2; ++forced)
      for (int Ho = 1; Ho <= %(hmax)d; ++Ho) {
        const FlowRows r = flow_plan_rows_halving(pr, Ho, forced != 0);
        std::printf("H 1 0 %%ld %%d %%d %%d %%d %%ld 6", pr, forced, Ho, r.rs, r.segs, r.items);
        for (int s = 0; s < r.segs; ++s) {
          const int n = flow_seg_rows(Ho, r.rs, s);
          std::printf(" %%d:%%d:%%d:%%d", flow_seg_first(r.rs, s), n, flow_rows_needed(1, n), flow_rows_run(1, false, n));
        }
        std::printf("\n");
      }
  std::printf("G %%d %%d %%d %%d\n", flow_strips(kFlowParity, 128), flow_groups(19, 2), (int)flow_takes(576, 128), (int)flow_takes(320, 64));
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("flow_plan")
    src, exe = str(d / "flow_plan_dump.cpp"), str(d / "flow_plan_dump")
    with open(src, "w") as f:
        f.write(PROGRAM % dict(wmax=WMAX, hmax=HMAX, simds=SIMDS, per_row=", ".join("%dL" % v for v in PER_ROW)))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    cols, rows, halving, misc = {}, [], [], None
    for line in out.stdout.splitlines():
        t = line.split()
        if t[0] == "C":
            cols[(int(t[1]), int(t[2]))] = (int(t[3]), [tuple(int(v) for v in s.split(":")) for s in t[4:]])
        elif t[0] in "RH":
            (rows if t[0] == "R" else halving).append((tuple(int(v) for v in t[1:10]), [tuple(int(v) for v in s.split(":")) for s in t[10:]]))
        else:
            misc = tuple(int(v) for v in t[1:])
    assert len(cols) == 2 * WMAX and len(rows) == 3 * len(PER_ROW) * 2 * HMAX and len(halving) == len(PER_ROW) * 2 * HMAX
    assert misc is not None
    return cols, rows, misc, halving


HALO, EDGE = 0, 1


@pytest.mark.parametrize("layout", [HALO, EDGE])
def test_every_column_is_stored_exactly_once(plan, layout):
    cols = plan[0]
    for W in range(1, WMAX + 1):
        strips, table = cols[(layout, W)]
        assert strips == len(table) >= 1
        owner = {}
        for k, (col0, mask) in enumerate(table):
            assert col0 == 14 * k - (1 if layout == HALO else 0)
            for lane in range(16):
                if not (mask >> lane) & 1:
                    continue
                col = col0 + lane
                assert 0 <= col < W, "W=%d: strip %d lane %d stores column %d outside the map" % (W, k, lane, col)
                assert col not in owner, "W=%d: column %d stored by %s and by %s" % (W, col, owner[col], (k, lane))
                owner[col] = (k, lane)
                # a lane without a neighbour in its strip may only store where that neighbour is the padding of the map
                assert lane != 0 or col == 0, "W=%d: lane 0 of strip %d stores column %d" % (W, k, col)
                assert lane != 15 or col == W - 1, "W=%d: lane 15 of strip %d stores column %d" % (W, k, col)
                if layout == HALO:
                    assert 1 <= lane <= 14
        assert sorted(owner) == list(range(W)), "W=%d: columns %s are never stored" % (W, sorted(set(range(W)) - set(owner)))
        want = -(-W // 14) if layout == HALO else (1 if W <= 16 else -(-(W - 2) // 14))
        assert strips == want, (W, strips, want)
    assert cols[(EDGE, 128)][0] == 9 and cols[(HALO, 128)][0] == 10 and cols[(HALO, 256)][0] == 19 and cols[(EDGE, 256)][0] == 19


def _tiles(table, Ho, rs, stride, step, what):
    """The segments cover rows 0 .. Ho - 1 once, in order; the row loop runs whole trips and at least the rows a segment needs."""
    nxt = 0
    for first, n, needed, run in table:
        assert first == nxt and n >= 1, what
        nxt = first + n
        assert needed == (n + 2 if stride == 1 else 2 * n + 1), what
        assert run >= needed and run % step == 0 and run - needed < step, (what, first, n, needed, run)
    assert nxt == Ho, "%s: the segments end at row %d" % (what, nxt)
    assert all(n == rs for _, n, _, _ in table[:-1]) and table[-1][1] <= rs, what


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_segments_tile_the_rows_and_full_segments_run_no_surplus(plan, kind):
    stride, pair, step = KINDS[kind]
    least = 0 if stride == 1 else 1  # 2 rs + 1 input rows are odd, the stride-2 loop runs four rows per trip
    seen = 0
    for (st, pr_, per_row, forced, Ho, rs, segs, items, step_), table in plan[1]:
        if (st, pr_) != (stride, pair):
            continue
        seen += 1
        assert step_ == step and segs == len(table) and items == per_row * segs and 1 <= rs <= min(64, Ho)
        _tiles(table, Ho, rs, stride, step, "%s Ho=%d rs=%d" % (kind, Ho, rs))
        # a full segment: one of the planned length.  Lengths with the least surplus exist for every loop (from 16 rows down to
        # 6), so a map cut into several segments must have been cut at one of them; a map that is ONE segment is the "last,
        # shorter" segment of a longer length and runs whatever its height asks for
        if segs >= 2:
            assert (-(rs + 2) % step if stride == 1 else -(2 * rs + 1) % step) == least, (kind, forced, Ho, rs)
            for first, n, needed, run in table:
                if n == rs:
                    assert run - needed == least
        if not forced:
            assert rs >= min(12, Ho)
        elif per_row <= 40 and Ho >= 12:
            assert segs >= 2, "%s Ho=%d: a forced launch on a small map must still run several segments" % (kind, Ho)
    assert seen == len(PER_ROW) * 2 * HMAX


def test_stem_segments_tile_the_rows(plan):
    """The stem instances keep 64 / 32 / 16 rows (forced: down to 8): the same tiling, a surplus of up to five rows."""
    for (st, pr_, per_row, forced, Ho, rs, segs, items, step), table in plan[3]:
        assert segs == len(table) and items == per_row * segs and 1 <= rs <= min(64, Ho)
        assert rs == Ho or rs in ((8, 16, 32, 64) if forced else (16, 32, 64))
        _tiles(table, Ho, rs, 1, step, "stem Ho=%d rs=%d" % (Ho, rs))
        if forced and per_row <= 40 and Ho >= 17:
            assert segs >= 2


def test_the_bench_blocks_and_the_gate(plan):
    """SSD-MobileNetV2@512 at batch 64 on 1024 SIMDs.  Block 3 (576 items per segment row, row pairs): 26 rows, 2880 items of
    28 loop rows, three on the busiest SIMD (16 rows on ten strips: 5120 items of 20, five).  Block 2 (576, stride 2): 19 rows,
    4032 items of 40 loop rows, four (16 rows: 4608 of 36, five).  The stem block (640): 32 rows as before.  And the gate:
    2048 items of 16 rows."""
    got = {}
    for (st, pr_, per_row, forced, Ho, rs, segs, items, step_), table in plan[1]:
        if not forced and (Ho, per_row) == (128, 576):
            got[(st, pr_)] = (rs, items, max(run for _, _, _, run in table), sum(run for _, _, _, run in table))
    assert got[(1, 1)] == (26, 2880, 28, 140) and got[(2, 0)] == (19, 4032, 40, 272), got
    stem = [(rs, items) for (_, _, per_row, forced, Ho, rs, _, items, _), _ in plan[3] if (per_row, forced, Ho) == (640, 0, 256)]
    assert stem == [(32, 5120)]
    assert plan[2] == (18, 10, 1, 0)
