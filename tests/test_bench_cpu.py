"""bench.py's forward check must be able to fail (Weak 2 / Next 1c): `judge_heads` is fed the statistics of
the driver's own bf16 line (loc floors at 0.5 - 0.8 of the signal) with a good plan, then with zeros, a constant, shuffled
values and noise of the right size in one head at a time.  CPU only, no kernels."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _logit(p):
    p = p.float().clamp(1e-7, 1 - 1e-7)
    return torch.log(p) - torch.log1p(-p)


def _case(floor_sigma):
    g = torch.Generator().manual_seed(17)
    ref_loc = [torch.randn(4, 24, 8, 8, generator=g) * 0.8, torch.randn(4, 24, 4, 4, generator=g) * 0.7]
    ref_conf = [torch.sigmoid(torch.randn(4, 480, 8, 8, generator=g) * 0.6 - 4), torch.sigmoid(torch.randn(4, 480, 4, 4, generator=g) * 0.5 - 4)]

    def noisy_loc(t):
        return t + floor_sigma * float(t.std()) * torch.randn(t.shape, generator=g)

    def noisy_conf(t):
        lg = _logit(t)
        return torch.sigmoid(lg + floor_sigma * float(lg.std()) * torch.randn(t.shape, generator=g))

    floor = ([noisy_loc(t) for t in ref_loc], [noisy_conf(t) for t in ref_conf])
    plan = ([noisy_loc(t) for t in ref_loc], [noisy_conf(t) for t in ref_conf])
    return g, ref_loc, ref_conf, floor, plan


@pytest.mark.parametrize("floor_sigma", [0.08, 0.5, 0.8])
def test_forward_check_passes_a_plan_at_the_floor_and_fails_dead_heads(floor_sigma):
    g, ref_loc, ref_conf, floor, plan = _case(floor_sigma)
    rows, worst, corr_ok = bench.judge_heads(plan[0], plan[1], floor[0], floor[1], ref_loc, ref_conf)
    assert worst <= 1.0 and corr_ok, rows
    prior = float(torch.sigmoid(torch.tensor(-4.0)))

    def perm(t):
        return t.flatten()[torch.randperm(t.numel(), generator=g)].view_as(t)

    for name, mk_loc, mk_conf in (
            ("zeros", torch.zeros_like, lambda t: torch.full_like(t, prior)),
            ("shuffled", perm, perm),
            ("noise", lambda t: torch.randn(t.shape, generator=g) * float(t.std()),
             lambda t: torch.sigmoid(torch.randn(t.shape, generator=g) * float(_logit(t).std()) - 4))):
        for head in ("loc", "conf"):
            for level in (0, 1):
                bl = [mk_loc(t) if (head == "loc" and i == level) else p for i, (t, p) in enumerate(zip(ref_loc, plan[0]))]
                bc = [mk_conf(t) if (head == "conf" and i == level) else p for i, (t, p) in enumerate(zip(ref_conf, plan[1]))]
                rows, worst, corr_ok = bench.judge_heads(bl, bc, floor[0], floor[1], ref_loc, ref_conf)
                assert not (worst <= 1.0 and corr_ok), (name, head, level, floor_sigma, rows)


def test_round4_rule_alone_admitted_a_zero_head():
    """Why the correlation rule exists: at the bf16 floors of the driver's line (0.5 - 0.8) the error rule alone passes zeros."""
    g, ref_loc, ref_conf, floor, plan = _case(0.8)
    zl = [torch.zeros_like(ref_loc[0]), plan[0][1]]
    rows, worst, corr_ok = bench.judge_heads(zl, plan[1], floor[0], floor[1], ref_loc, ref_conf)
    assert worst <= 1.0 and not corr_ok, rows


def test_dump_outputs_writes_every_array_as_float32_npy(tmp_path):
    """--dump-outputs: one DIR/<name>.npy per returned array, 16-bit floats and integers as float32, float64 kept, values
    unchanged."""
    import numpy as np

    g = torch.Generator().manual_seed(3)
    scores = torch.rand(4, 100, generator=g)
    boxes = torch.randn(4, 100, 4, generator=g).to(torch.bfloat16)
    classes = torch.randint(0, 80, (4, 100), generator=g)
    wide = torch.randn(4, 3, generator=g, dtype=torch.float64)
    out = bench.dump_outputs(str(tmp_path / "d"), {"scores": scores, "boxes": boxes, "classes": classes, "wide": wide})
    assert out == {"scores.npy": [4, 100], "boxes.npy": [4, 100, 4], "classes.npy": [4, 100], "wide.npy": [4, 3]}
    assert sorted(os.listdir(tmp_path / "d")) == ["boxes.npy", "classes.npy", "scores.npy", "wide.npy"]
    for name, t in (("scores", scores), ("boxes", boxes), ("classes", classes)):
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == np.float32 and np.array_equal(a, t.float().numpy()), name
    w = np.load(tmp_path / "d" / "wide.npy")
    assert w.dtype == np.float64 and np.array_equal(w, wide.numpy())


def test_dump_outputs_samples_the_same_images_under_the_cap(tmp_path):
    """Above the cap every array keeps the same fixed, seeded rows (their indices in image_index.npy) and the files stay
    under the cap; a second dump picks the same rows."""
    import numpy as np

    n = 1000
    scores = torch.arange(n * 10, dtype=torch.float32).view(n, 10)
    boxes = torch.arange(n * 40, dtype=torch.float32).view(n, 10, 4)
    cap = 16 << 10
    dirs = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        bench.dump_outputs(str(d), {"scores": scores, "boxes": boxes}, cap_bytes=cap)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= cap + 3 * 128  # + one .npy header per file
        dirs.append(d)
    idx = np.load(dirs[0] / "image_index.npy")
    assert idx.dtype == np.float64 and 1 <= len(idx) < n and np.all(np.diff(idx) > 0)
    rows = idx.astype(np.int64)
    assert np.array_equal(np.load(dirs[0] / "scores.npy"), scores.numpy()[rows])
    assert np.array_equal(np.load(dirs[0] / "boxes.npy"), boxes.numpy()[rows])
    for f in ("image_index.npy", "scores.npy", "boxes.npy"):
        assert np.array_equal(np.load(dirs[0] / f), np.load(dirs[1] / f)), f


def test_steps_below_one_are_refused(monkeypatch):
    """--steps sets the number of timed steps: zero timed steps have no last step to report or dump."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3", "--warmup", "0", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.steps == 3 and a.warmup == 0 and a.dump_outputs == "out"


def test_timed_region_times_exactly_steps_after_warmup():
    """`warmup` untimed calls, then exactly `steps` calls between the two barriers; the last call's output is returned."""
    log = []

    def step():
        log.append("step")
        return len(log)

    elapsed, out = bench.timed_region(step, 7, 3, lambda: log.append("barrier"), 1, None,
                                      before_timed=lambda: log.append("hook"))
    assert log == ["step"] * 3 + ["hook", "barrier"] + ["step"] * 7 + ["barrier"]
    assert out == len(log) - 1 and elapsed >= 0
