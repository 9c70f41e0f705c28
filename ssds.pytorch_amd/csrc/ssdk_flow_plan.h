// ssdk_flow_plan.h -- the geometry of a register-flow block launch (ssdk_mbflow.hip): how a map is cut into 16-lane column
// strips and into segments of rows.  Plain C++ (no HIP types): launch_mbflow and mbflow_kernel read the same constexpr
// functions, and tests/test_flow_plan_cpu.py compiles them into a host program of its own.
//
// Columns.  A strip is the 16 lanes of a DPP row, one pixel per lane; the horizontal depthwise taps are lane shifts with
// `bound_ctrl`, so the first / last lane of a strip reads 0 for its missing neighbour.  A lane may therefore store its
// output if both neighbours sit in the strip -- or if the missing neighbour is the zero padding of the map:
//   kFlowHalo    strip k holds columns 14k - 1 .. 14k + 14 and stores lanes 1 .. 14: every strip carries two halo lanes.
//                (The stem instances: their image loads have the strip origin folded into the byte offsets.)
//   kFlowEdge    strip k holds columns 14k .. 14k + 15.  Strip 0 stores lanes 0 .. 14 (lane 0 is column 0: its left tap is
//                padding), strip k >= 1 lanes 1 .. 14, and lane 15 stores where it is column W - 1.  ceil((W - 2) / 14)
//                strips instead of ceil(W / 14): 9 instead of 10 at W = 128.  (Stride-1 blocks.)
//   kFlowParity  stride 2: a PAIR of strips holds the even / odd input columns of one range, 15 outputs per pair; the lane
//                mapping lives with the kernel (ssdk_mbflow.hip, header), here is only the count.
//
// Rows.  A segment of `rs` output rows reads rs + 2 input rows at stride 1 and 2 rs + 1 at stride 2, and the row loops run
// whole groups of rows (flow_row_step); the surplus rows of a segment are expanded and folded into accumulators nobody
// stores.  flow_plan_rows picks `rs` among the lengths whose full segments have no surplus (stride 2: the least, one row)
// by what the busiest SIMD then runs.
#pragma once

namespace ssdk {

enum FlowLayout { kFlowHalo = 0, kFlowEdge = 1, kFlowParity = 2 };

constexpr int kFlowLanes = 16;  // pixels of a strip
constexpr int kFlowPitch = 14;  // columns from one strip to the next (stride 1)

constexpr int flow_layout(int stride, bool stem) { return stride == 2 ? kFlowParity : (stem ? kFlowHalo : kFlowEdge); }

// strips per row of a map with Wo output columns
constexpr int flow_strips(int layout, int Wo) {
  if (layout == kFlowParity) return 2 * ((Wo + 14) / 15);
  if (layout == kFlowEdge) return Wo <= kFlowLanes ? 1 : (Wo - 2 + kFlowPitch - 1) / kFlowPitch;
  return (Wo + kFlowPitch - 1) / kFlowPitch;
}
// work items per row: NS neighbouring strips share a wave
constexpr int flow_groups(int strips, int ns) { return (strips + ns - 1) / ns; }

// kFlowHalo / kFlowEdge (stride 1: input column = output column): the column in lane 0 of a strip ...
constexpr int flow_strip_col0(int layout, int strip) { return layout == kFlowEdge ? strip * kFlowPitch : strip * kFlowPitch - 1; }
// ... and whether a lane stores its column (W = width of the map)
constexpr bool flow_lane_stores(int layout, int strip, int lane, int W) {
  const int col = flow_strip_col0(layout, strip) + lane;
  if (col < 0 || col >= W) return false;
  if (layout == kFlowEdge) return (lane >= 1 || strip == 0) && (lane <= kFlowLanes - 2 || col == W - 1);
  return lane >= 1 && lane <= kFlowLanes - 2;
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
// input rows one trip of the row loop covers: 4 with row pairs (two visits of two rows), 6 at stride 1 (two rotations of the
// three accumulator sets), 4 at stride 2
constexpr int flow_row_step(int stride, bool pair) { return pair ? 4 : (stride == 1 ? 6 : 4); }
constexpr int flow_rows_needed(int stride, int out_rows) { return stride == 1 ? out_rows + 2 : 2 * out_rows + 1; }
constexpr int flow_rows_run(int stride, bool pair, int out_rows) {
  const int step = flow_row_step(stride, pair);
  return (flow_rows_needed(stride, out_rows) + step - 1) / step * step;
}
constexpr int flow_surplus(int stride, bool pair, int out_rows) { return flow_rows_run(stride, pair, out_rows) - flow_rows_needed(stride, out_rows); }
// the least surplus a segment length can have: 2 rs + 1 is odd, the stride-2 step is 4
constexpr int flow_min_surplus(int stride) { return stride == 1 ? 0 : 1; }
constexpr int flow_segs(int Ho, int rs) { return (Ho + rs - 1) / rs; }
// segment s covers output rows [first, first + rows)
constexpr int flow_seg_first(int rs, int s) { return s * rs; }
constexpr int flow_seg_rows(int Ho, int rs, int s) { return (s + 1) * rs <= Ho ? rs : Ho - s * rs; }
// rows the loops of one strip run over the whole map (the last segment may be shorter, and may have a surplus)
constexpr int flow_map_rows_run(int stride, bool pair, int Ho, int rs) {
  int sum = 0;
  for (int s = 0; s < flow_segs(Ho, rs); ++s) sum += flow_rows_run(stride, pair, flow_seg_rows(Ho, rs, s));
  return sum;
}

constexpr int kFlowRsMin = 12, kFlowRsMax = 64;  // below 12 rows the two halo rows of a segment cost too much
constexpr int kFlowRsMinForced = 4;              // forced launches (tests): short segments, several per small map
constexpr int kFlowRsGate = 16;
constexpr long kFlowMinItems = 2048;

// Whether a block with `per_row` = N * groups work items per segment row is this kernel's at all: 2048 items of 16 rows.
constexpr bool flow_takes(long per_row, int Ho) { return per_row * flow_segs(Ho, kFlowRsGate) >= kFlowMinItems; }

struct FlowRows {
  int rs, segs;
  long items;
};

// What a segment length costs.  The kernel is bound by VALU issue, an item is a wave, and the waves of a launch spread evenly
// over the SIMDs: the busiest SIMD runs ceil(items / simds) items of flow_rows_run(rs) rows each, whatever the number of
// waves it holds at a time.  (Measured, DESIGN.md section 4.6: 24 -> 144 -> 24 at 128 x 128, batch 64, nine strips on 1024
// SIMDs: rs 26 = 3 x 28 rows, 71 us; rs 30 = 3 x 32, 80 us; rs 16 = 5 x 20, 81 us; ten strips at rs 26 = 4 x 28, 94 us.)
constexpr long flow_rows_cost(long per_row, int Ho, int stride, bool pair, int rs, int simds) {
  const long items = per_row * flow_segs(Ho, rs);
  return (items + simds - 1) / simds * flow_rows_run(stride, pair, rs < Ho ? rs : Ho);
}

// Rows per segment: among the lengths in [kFlowRsMin, kFlowRsMax] (a `forced` launch: from kFlowRsMinForced) whose full
// segments run the least surplus, the cheapest; ties go to the fewer rows over the map, then to the shorter segment.  On a
// small map every length costs one item per SIMD, so the shortest wins: a forced launch there runs several segments.
constexpr FlowRows flow_plan_rows(long per_row, int Ho, int stride, bool pair, bool forced, int simds) {
  int best = 0, best_rows = 0;
  long best_cost = 0;
  for (int rs = forced ? kFlowRsMinForced : kFlowRsMin; rs <= kFlowRsMax; ++rs) {
    if (flow_surplus(stride, pair, rs) != flow_min_surplus(stride)) continue;
    const long cost = flow_rows_cost(per_row, Ho, stride, pair, rs, simds);
    const int rows = flow_map_rows_run(stride, pair, Ho, rs < Ho ? rs : Ho);
    if (!best || cost < best_cost || (cost == best_cost && rows < best_rows)) {
      best = rs;
      best_cost = cost;
      best_rows = rows;
    }
  }
  const int rs = best < Ho ? best : Ho;
  return FlowRows{rs, flow_segs(Ho, rs), per_row * flow_segs(Ho, rs)};
}

// The stem instances keep the rule they had: the longest of 64 / 32 / 16 rows that gives 4096 items (forced: down to 8 rows,
// until there are 2048).  Their zero-surplus lengths measured no faster (34 rows: 83.5 against 79.8 us of 32 rows).
constexpr FlowRows flow_plan_rows_halving(long per_row, int Ho, bool forced) {
  int rs = 64;
  while (rs > 16 && per_row * flow_segs(Ho, rs) < 4096) rs >>= 1;
  if (forced)
    while (rs > 8 && per_row * flow_segs(Ho, rs) < kFlowMinItems) rs >>= 1;
  if (rs > Ho) rs = Ho;
  return FlowRows{rs, flow_segs(Ho, rs), per_row * flow_segs(Ho, rs)};
}

}  // namespace ssdk
