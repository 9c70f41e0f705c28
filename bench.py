#!/usr/bin/env python
"""bench.py -- images/sec of the detection hot path (fwd + decode + NMS) of SSD-MobileNetV2@512 on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic images already resident in HBM:
backbone + extras + multibox heads forward, decode of every level and NMS.  BASELINE.json's metric is quoted on
`configs[1]` (SSD + MobileNetV2 @512x512 bf16, batch 64, one MI355X); with N > 1 every rank runs the same per-GPU
batch (weak scaling, replicas only: inference has no collective -- SURVEY.md 8e).  `--gpus N` without a launcher
(WORLD_SIZE unset) re-executes itself under torch.distributed.run with N ranks on 127.0.0.1.

Other BASELINE configs through the same file: `--cfg experiments/cfgs/fpn_resnet50_640.yml --batch 32` (config 3),
`--cfg experiments/cfgs/bifpn_regnetx008_896.yml --batch 16 --dtype fp16 --graph 1` (config 5).

`--dump-outputs DIR` writes what the last timed step returned on rank 0 -- the detections a caller of the step receives
(scores.npy, boxes.npy, classes.npy, float32) -- after the timed region.  Weights and images are seeded, so the same
arguments give the same inputs on every run and two builds can be compared output for output.

The whole step runs in line on one stream by default.  Serving-loop pipelining is an option (--tail-stream 1): the
latency-bound end of the decode stage (levelsel_kernel + nmswalk_kernel: per-level select + box decode, NMS) is then
enqueued on its own HIP stream and runs under the NEXT step's forward pass while the HBM-bound scan16_kernel stays in
line on the main stream.  It was the default in round 1 (+3 % with that round's decode stage); since round 2 it is
within noise of the in-line step (round 3, same box: 45.89 / 45.90 k in line, 45.78 / 45.73 k img/s with it), so the simpler path is
the one that is timed.  All work of the K steps completes inside the timed region (device-wide synchronize on both
sides).  After the timed loop the last step is re-run in line (bit-equal outputs required: side-stream plans and the tail
stream must not change a bit) and, on rank 0 of an N=1 run, the numpy oracle decodes the GPU's own head outputs of a sample
of images (must reproduce the timed detections) and `forward_check` runs the timed plan's kernels on the same architecture
with seeded O(1) weights against its fp32 CPU forward (bar: twice PyTorch-ROCm's own 16-bit error + 0.02; the per-op
kernel names must equal the timed plan's): all three together are `verified`, and a failure of any is a SystemExit instead
of a number.  (On the reference's init, which the timed model carries, a forward comparison decides nothing -- the box
heads of levels 1-5 are ~1e-9 -- so those numbers are reported as `part_of_verified: false`.)

Prints ONE JSON line (rank 0).  Besides the driver's contract fields it carries
  roofline      HBM roofline of the dominant hand-written kernel of the decode stage (scan_kernel: the one pass over
                the conf tensors), from hipEvents recorded live inside the timed region (the Decoder's ssdk_ctx ring),
                on the bench input AND on SURVEY 8d's microbench heads (`realistic_heads`); the whole decode+NMS stage
                against SURVEY 8d's 1.465 MB/img; MFMA utilisation of the head convs
  stages        per-stage milliseconds (forward / decode+NMS kernels) for orientation
  cpu_baseline  the CPU path on this host (torch fp32 forward of the same module + the numpy oracle's Decoder) on a
                bounded sample of the same workload (N=1 runs only), plus -- when profiles/r*_cpu_reference.json is
                committed -- the REFERENCE's own code timed in the build container (it cannot travel to the GPU box)
"""
import argparse
import glob
import json
import os
import socket
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "ssds.pytorch_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling
MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 / fp16 MFMA peak (MI355X_MICROARCH.md), no sparsity


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU per step")
    ap.add_argument("--cfg", default=os.path.join(ROOT, "experiments", "cfgs", "ssd_mobilenetv2_512.yml"))
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"], help="compute dtype of the network")
    ap.add_argument("--cpu-sample", type=int, default=4, help="images for the CPU baseline (0 = skip)")
    ap.add_argument("--graph", type=int, default=0, help="1: replay the step as one captured hipGraph")
    ap.add_argument("--tail-stream", type=int, default=0,
                    help="1: the tail kernel of the decode stage on its own stream (overlaps the next step's forward)")
    ap.add_argument("--layers", type=int, default=0, help="1: add the per-layer table (us, TFLOP/s, GB/s) to the JSON")
    ap.add_argument("--channels-last", type=int, default=int(os.environ.get("SSDK_CHANNELS_LAST", "0")))
    ap.add_argument("--main-priority", type=int, default=0,
                    help="-1: run the forward + scan on a high-priority stream (the overlapped tail kernel then only takes "
                         "CUs the forward leaves idle)")
    ap.add_argument("--stub-cpu", type=int, default=0,
                    help="(tests/test_ddp_cpu.py) 1: exercise ONLY the launcher / rank / timing logic on CPU under gloo with a "
                         "sleeping step -- no model, no kernels, prints a line marked data='stub'; never a measurement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned (scores, boxes, classes of rank 0) "
                         "as DIR/<name>.npy in float32 (at most 64 MB in all: a fixed, seeded sample of images beyond that)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be >= 1 (the number of timed steps)")
    return args


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays, cap_bytes=DUMP_CAP_BYTES, seed=0):
    """--dump-outputs: `arrays` (name -> tensor or array, all with the batch as the first dimension) -> out_dir/<name>.npy,
    float64 kept, everything else as float32.  When they exceed `cap_bytes` together, every array is cut to the same fixed,
    seeded sample of images (ascending), whose indices go to out_dir/image_index.npy.  Returns {file name: shape}."""
    import numpy as np

    host = OrderedDict()
    for k, v in arrays.items():
        if hasattr(v, "detach"):  # torch tensor (numpy has no bfloat16: every non-float64 dtype goes through float32)
            v = v.detach().cpu()
            v = v.double() if v.dtype.is_floating_point and v.element_size() == 8 else v.float()
            v = v.numpy()
        a = np.asarray(v)
        host[k] = a if a.dtype == np.float64 else a.astype(np.float32)
    rows = {a.shape[0] for a in host.values()}
    if len(rows) != 1:
        raise ValueError("dump_outputs: the arrays do not share a batch dimension: %s" % {k: a.shape for k, a in host.items()})
    n = rows.pop()
    if sum(a.nbytes for a in host.values()) > cap_bytes:
        per_image = sum(a.nbytes // max(n, 1) for a in host.values()) + 8  # + its float64 index
        keep = cap_bytes // per_image
        if keep < 1:
            raise ValueError("dump_outputs: one image's outputs (%d bytes) exceed the cap of %d bytes" % (per_image, cap_bytes))
        idx = np.sort(np.random.RandomState(seed).choice(n, int(keep), replace=False))
        host = OrderedDict((k, a[idx]) for k, a in host.items())
        host["image_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    written = OrderedDict()
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(a))
        written[k + ".npy"] = list(a.shape)
    return written


def timed_region(step, steps, warmup, barrier, world, reduce_max, before_timed=None):
    """The driver's contract: `warmup` untimed steps, then exactly `steps` steps bracketed by barrier (+ device
    synchronize, inside `barrier`) on both sides; the elapsed time is the MAX over ranks.  Returns (seconds, last out)."""
    out = None
    for _ in range(warmup):
        step()
    if before_timed is not None:
        before_timed()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        elapsed = reduce_max(elapsed)
    return elapsed, out


def stub_main(args):
    """--stub-cpu 1: the same launcher / env / barrier / MAX-over-ranks / rank-0-print path as the real bench, on CPU under
    gloo; rank r sleeps (r + 1) * 2 ms per step so that the MAX reduction is observable (tests/test_ddp_cpu.py)."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")

    def barrier():
        if world > 1:
            dist.barrier()

    def reduce_max(v):
        t = torch.tensor([v], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    elapsed, _ = timed_region(lambda: time.sleep(0.002 * (rank + 1)), args.steps, args.warmup, barrier, world, reduce_max)
    if rank == 0:
        print(json.dumps({"metric": "stub (launcher / rank logic only)", "value": round(world * args.batch * args.steps / elapsed, 2),
                          "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
                          "vs_baseline": None, "dtype": "none", "data": "stub",
                          "config": {"workload": "CPU stub of the rank logic", "batch_per_gpu": args.batch,
                                     "global_batch": args.batch * world}}))
    if world > 1:
        dist.destroy_process_group()


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` (no launcher): become `python -m torch.distributed.run --nproc-per-node N bench.py ...`."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.execv(sys.executable, cmd)


def scan_traffic_bytes(cfg_stem=None):
    """(HBM read bytes per scan_kernel launch, source file) from the newest committed separate `rocprofv3 --pmc
    FETCH_SIZE` pass of this command (raw KB x 1024 x 2, the gfx950 correction of MI355X_MICROARCH.md), or (None, None).
    PMC collection cannot run inside the timed region, so this is a REPLAYED measurement: `traffic_source` names it.
    The headline command's passes are `profiles/r*_pmc_fetch_size_v*.csv`, another configuration's carry its cfg's name
    (`r*_pmc_fetch_size_<cfg>_v*.csv`, tools/run/profile_r04.sh)."""
    import csv

    pat = "r*_pmc_fetch_size_v*.csv" if cfg_stem is None else "r*_pmc_fetch_size_%s_v*.csv" % cfg_stem
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pat)))
    for f in reversed(files):
        for row in csv.DictReader(open(f)):
            if "scan16_kernel" in row["kernel"] or "scan_kernel" in row["kernel"]:
                return int(float(row["bytes_per_dispatch_x2_gfx950_correction"])), os.path.relpath(f, ROOT)
    return None, None


def scan_rocprof_avg_ns(cfg_stem=None):
    """(average launch duration of scan16_kernel in ns, calls, source file) from the newest committed `rocprofv3 --kernel-trace
    --stats` summary of this command (`profiles/r*_bench_kernel_stats_v*.csv`; another configuration's carries its cfg's name), or
    (None, None, None).  The kernel trace times a launch by its own begin / end timestamps: no hipEvent interval (4.6 us on this
    stack) inside the figure.  A REPLAYED measurement, like `traffic`: `frac_source` names the file."""
    import csv

    pat = "r*_bench_kernel_stats_v*.csv" if cfg_stem is None else "r*_bench_%s_kernel_stats_v*.csv" % cfg_stem
    for f in reversed(sorted(glob.glob(os.path.join(ROOT, "profiles", pat)))):
        for row in csv.DictReader(open(f)):
            if "scan16_kernel" in row["Name"] or "scan_kernel" in row["Name"]:
                return float(row["AverageNs"]), int(row["Calls"]), os.path.relpath(f, ROOT)
    return None, None, None


def reference_cpu_record():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cpu_reference.json")))
    if not files:
        return None
    rec = json.load(open(files[-1]))
    out = {"source": os.path.relpath(files[-1], ROOT), "host": rec["host"], "what": rec["what"], "threads": {}}
    for nt, v in rec["threads"].items():
        out["threads"][nt] = {"decoder_images_per_s": round(v["decoder_images_per_s"], 2),
                              "hot_path_images_per_s": round(v["hot_path_images_per_s"], 3)}
    return out


def judge_heads(plan_loc, plan_conf, floor_loc, floor_conf, ref_loc, ref_conf):
    """The decision of `forward_check` on CPU tensors: the plan's heads, PyTorch-ROCm's 16-bit heads (the noise floor) and the
    fp32 CPU heads of the same images -> (rows, worst ratio to the error bar, correlation rule satisfied).

    Per head tensor (class heads as logits: a sigmoid output near 0.01 hides its logit), with errors in units of the CENTRED
    rms of the fp32 reference (a class head's logits are -4 +- 0.6: their plain rms is ~4 of bias):
      * rms(plan - fp32) <= 2 x rms(floor - fp32) + 0.02;
      * corr(plan, fp32) >= corr(floor, fp32) - 0.05 - 3 sigma of the difference of two sample correlations of that size  (round 5; the
        sampling term: round 6).  Deep levels of a random-weight network executed in bf16 are
        0.5 - 0.9 rms away from fp32 for PyTorch-ROCm too, so the first rule alone admits an all-zero head (error 1.0) and,
        where the floor is above 0.7, noise of the right size (1.41); their correlation with fp32 is 0 while the floor's is
        0.6 - 0.99.  tests/test_bench_cpu.py feeds zeros, a constant, shuffled values and noise: every one fails."""
    import torch

    def logit(p):
        p = p.float().clamp(1e-7, 1.0 - 1e-7)
        return torch.log(p) - torch.log1p(-p)

    def centred(t):
        return t - t.mean()

    def rms(t):
        return float(t.pow(2).mean().sqrt())

    def corr(a, ref):
        ac, rc = centred(a), centred(ref)
        d = rms(ac) * rms(rc)
        return float((ac * rc).mean()) / d if d > 0 else 0.0

    rows, worst, corr_ok = [], 0.0, True
    for tag, gs, ts, cs, f in (("loc", plan_loc, floor_loc, ref_loc, lambda t: t.float()),
                               ("conf(logit)", plan_conf, floor_conf, ref_conf, logit)):
        for i, (gt, tt, ct) in enumerate(zip(gs, ts, cs)):
            ref, got, flo = f(ct), f(gt), f(tt)
            unit = max(rms(centred(ref)), 1e-30)
            r_plan, r_floor = rms(got - ref) / unit, rms(flo - ref) / unit
            c_plan, c_floor = corr(got, ref), corr(flo, ref)
            bar = 2.0 * r_floor + 0.02
            worst = max(worst, r_plan / bar)
            # (two executions are two draws of the 16-bit rounding noise: the sample correlation of n values scatters by
            #  (1 - r^2) / sqrt(n), the difference of two by sqrt(2) x that -- 0.07 per sigma on the 96 box deltas of four images
            #  at the 1 x 1 level, where PyTorch-ROCm's own r moved from 0.62 to 0.76 between two boxes and the fixed 0.05 turned
            #  one round-6 run into "no number"; nothing on the levels with >= 10^4 values)
            scatter = 3.0 * (1.0 - min(c_floor, 1.0) ** 2) * (2.0 / max(ref.numel(), 1)) ** 0.5
            corr_ok = corr_ok and (c_plan >= c_floor - 0.05 - scatter)
            rows.append({"tensor": "%s%d" % (tag, i), "ref_std": float("%.3g" % unit), "plan": float("%.3g" % r_plan),
                         "pytorch_rocm": float("%.3g" % r_floor), "bar": float("%.3g" % bar),
                         "corr_plan": float("%.4f" % c_plan), "corr_pytorch_rocm": float("%.4f" % c_floor)})
    return rows, worst, corr_ok


def forward_check(args, cfg, x, xs, S, tdt, dev, timed_kernels, seed=4242):
    """The part of `verified` that checks the NETWORK kernels (rank 0, N = 1, after the timed region).  The timed model
    carries the reference's init, on which no forward comparison discriminates (see the caller); so the same architecture
    is built again with seeded O(1) weights (conv ~ N(0, 1.5 / fan_in), BatchNorm weight ~ U(0.5, 1.5), biases ~ N(0, 0.1),
    class-head bias -4) and BatchNorm statistics calibrated on two random batches, and run
      * on the device through the recorded plan at the TIMED batch shape (the planner picks kernels by shape, so these are
        the timed run's kernels: the per-op kernel names must be identical),
      * in fp32 on the CPU on the S sampled images (the reference),
      * by PyTorch-ROCm / MIOpen in the model dtype on those images (the noise floor of 16-bit execution of a deep untrained
        network: 0.02 ... 0.6 rms depending on the level).
    Bars per head tensor (`judge_heads`): centred relative rms error <= 2 x PyTorch-ROCm's + 0.02 AND correlation with the
    fp32 reference >= PyTorch-ROCm's - 0.05 - the sampling scatter of a tensor of that size; class heads as logits."""
    import torch
    import torch.nn as nn

    from ssds.core import config
    from ssds.modeling import model_builder

    torch.manual_seed(seed)
    cal = model_builder.create_model(cfg.MODEL)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in cal.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.5 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.zero_()
                m.running_var.fill_(1.0)
                m.momentum = None  # cumulative average over the calibration batches
            else:
                for name, prm in m.named_parameters(recurse=False):
                    if prm.dim() == 2:  # BiFPN fusion weights (bifpn.py:35-38): some negative, cut by the relu
                        prm.copy_(torch.rand(prm.shape, generator=g) * 1.2 - 0.2)
        finals = list(cal.conf) if isinstance(cal.conf, nn.ModuleList) else [list(cal.conf.children())[-1]]
        for m in finals:  # an untrained-looking score distribution: logits ~ N(-4, ~1)
            m.weight.mul_(0.6)
            m.bias.copy_(m.bias * 3 - 4.0)
        H, W = cfg.MODEL.IMAGE_SIZE
        cal.train()
        for _ in range(2):
            cal(torch.rand((2, 3, H, W), generator=g))
        cal.eval()
        state = {k: v.clone() for k, v in cal.state_dict().items()}
        cl, cc = cal(xs)  # fp32 CPU reference on the sampled images
        dmodel = cal.to(dev, tdt)
        if args.channels_last:
            dmodel = dmodel.to(memory_format=torch.channels_last)
        gl, gc = dmodel(x)  # the timed batch shape -> the timed kernels
        plan = dmodel._plan(x) if hasattr(dmodel, "_plan") else None
        if plan is None or isinstance(plan, str):
            plans = [q for q in getattr(dmodel, "_neck_plans", {}).values() if not isinstance(q, str)]
            plan = plans[0] if plans else None
        kernels = None
        if plan is not None:
            plan.ctx.set_op_profiling(True)
            dmodel(x)
            torch.cuda.synchronize(dev)
            kernels = [k for k, _ in plan.ctx.op_timings()]
            plan.ctx.set_op_profiling(False)
        os.environ["SSDK_FUSED_CONV"] = "0"  # PyTorch-ROCm / MIOpen executing the same module in the same dtype: the floor
        try:
            tl, tc = dmodel(x[:S])
        finally:
            del os.environ["SSDK_FUSED_CONV"]
        torch.cuda.synchronize(dev)
    del state

    rows, worst, corr_ok = judge_heads([t[:S].cpu() for t in gl], [t[:S].cpu() for t in gc], [t.cpu() for t in tl],
                                       [t.cpu() for t in tc], cl, cc)
    same = (kernels == timed_kernels) if (kernels is not None and timed_kernels is not None) else None
    return {"weights": "seeded O(1) weights + calibrated BatchNorm statistics, same architecture and batch shape as the timed run",
            "images": S, "relative_rms_error": rows, "worst_ratio_to_bar": float("%.3g" % worst),
            "same_kernels_as_timed": same, "correlation_rule_ok": bool(corr_ok),
            "ok": bool(worst <= 1.0 and corr_ok and same is not False)}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)
    if args.stub_cpu:
        return stub_main(args)
    import numpy as np
    import torch
    import torch.distributed as dist

    from ssds import _native as N
    from ssds.core import config
    from ssds.modeling import model_builder
    from ssds.modeling.layers.decoder import Decoder

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device; there is no CPU path")
    if world != max(1, args.gpus) and rank == 0:
        print("bench.py: --gpus %d but the launcher started %d ranks; reporting n_gpus = %d" % (args.gpus, world, world),
              file=sys.stderr)
    if local_rank >= torch.cuda.device_count():
        raise SystemExit("rank %d: only %d HIP devices are visible" % (rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)  # "nccl" is RCCL on ROCm
    n_gpus = world
    tdt = torch.bfloat16 if args.dtype == "bf16" else torch.float16

    cfg = config.cfg_from_file(args.cfg)
    torch.manual_seed(1234)  # same random-init weights on every rank (reference init, conf bias -log 99)
    model = model_builder.create_model(cfg.MODEL).eval()
    cpu_state = {k: v.clone() for k, v in model.state_dict().items()} if (rank == 0 and args.cpu_sample) else None
    model = model.to(dev, tdt)
    if args.channels_last:
        model = model.to(memory_format=torch.channels_last)
    anchors = model_builder.create_anchors(cfg.MODEL, model, cfg.MODEL.IMAGE_SIZE)
    decoder = model_builder.create_decoder(cfg.POST_PROCESS)
    use_tail = bool(args.tail_stream and not args.graph)
    if use_tail:
        decoder.enable_tail_stream()
    H, W = cfg.MODEL.IMAGE_SIZE
    B = args.batch
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    x = torch.rand((B, 3, H, W), device=dev, generator=g).to(tdt)  # synthetic, resident in HBM
    if args.channels_last:
        x = x.contiguous(memory_format=torch.channels_last)

    @torch.no_grad()
    def step():
        loc, conf = model(x)
        return decoder(loc, conf, anchors)

    if args.graph:
        from ssds.utils.graph import GraphedInference

        graphed = GraphedInference(model, decoder, anchors, x)
        eager_step = step

        def step():  # noqa: F811 -- the timed step is one hipGraphLaunch (the input is the static, resident batch)
            return graphed(graphed.static_x)

    def barrier():
        if world > 1:
            dist.barrier(device_ids=[local_rank])
        torch.cuda.synchronize(dev)

    main_stream = torch.cuda.Stream(device=dev, priority=-1) if args.main_priority < 0 else torch.cuda.current_stream(dev)
    torch.cuda.set_stream(main_stream)
    def reduce_max(v):
        t = torch.tensor([v], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # event ring: recorded inside the timed region (not capturable: eager only)
    elapsed, out = timed_region(step, args.steps, args.warmup, barrier, world, reduce_max,
                                before_timed=lambda: decoder.set_profiling(not args.graph))
    timed_out = [o.clone() for o in out]
    dumped = None
    if args.dump_outputs and rank == 0:  # the detections of the LAST timed step, as a caller of the step receives them
        dumped = dump_outputs(args.dump_outputs, OrderedDict(zip(("scores", "boxes", "classes"), timed_out)))

    # ---- per-kernel times recorded live in the timed region -------------------------------------------
    nprof = min(args.steps, 256)
    if args.graph:  # per-kernel events cannot be recorded inside a captured graph: a few eager steps afterwards
        decoder.set_profiling(True)
        nprof = 5
        for _ in range(nprof):
            eager_step()
        torch.cuda.synchronize(dev)
    tim = np.array([decoder.timings_ms(i) for i in range(nprof)], dtype=np.float64)  # [steps, (scan, tail|level, nms)]
    scan_ms, tail_ms, nms_ms = tim.mean(0)
    decoder.set_profiling(False)

    # ---- the timed loop's result, recomputed in line: one stream, no tail stream, no side lane ---------------
    if use_tail:
        decoder.disable_tail_stream()
    plan = model._plan(x) if hasattr(model, "_plan") else None
    neck_plans = list(getattr(model, "_neck_plans", {}).values()) if plan is None else []
    plans = [p for p in ([plan] + neck_plans) if p is not None and not isinstance(p, str)]
    for p in plans:
        p.ctx.set_side_lane(False)
    with torch.no_grad():
        loc, conf = model(x)
        inline = Decoder(decoder.conf_threshold, decoder.nms_threshold, decoder.top_n, decoder.top_n_per_level,
                         decoder.rescore, decoder.use_diou)(loc, conf, anchors)
    torch.cuda.synchronize(dev)
    verified = all(torch.equal(a, b) for a, b in zip(timed_out, inline))
    for p in plans:
        p.ctx.set_side_lane(None)
    if not verified:
        raise SystemExit("bench.py: the timed (multi-stream) loop and the in-line step disagree -- no number reported")

    @torch.no_grad()
    def time_fn(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / n

    fwd_ms = time_fn(lambda: model(x), max(3, min(10, args.steps)))
    dec_ms = time_fn(lambda: decoder(loc, conf, anchors), max(3, min(20, args.steps)))

    # ---- SURVEY 8d microbench heads (same shapes): conf = sigmoid(N(-4.6, 1.5^2)), loc = N(0, 0.5^2) -----------------
    def stage_times(l_, c_, reps=20):
        d = Decoder(decoder.conf_threshold, decoder.nms_threshold, decoder.top_n, decoder.top_n_per_level,
                    decoder.rescore, decoder.use_diou)
        for _ in range(3):
            d(l_, c_, anchors)
        d.set_profiling(True)
        for _ in range(reps):
            d(l_, c_, anchors)
        torch.cuda.synchronize(dev)
        per_kernel = np.array([d.timings_ms(i) for i in range(reps)], dtype=np.float64).mean(0)
        d.set_profiling(2)  # ONE interval around the whole stage: no event (and no cache flush) between its launches
        for _ in range(reps):
            d(l_, c_, anchors)
        torch.cuda.synchronize(dev)
        whole = float(np.mean([d.timings_ms(i)[0] for i in range(reps)]))
        d.set_profiling(False)
        return tuple(per_kernel) + (whole,)

    g2 = torch.Generator(device=dev).manual_seed(4321 + rank)
    r_conf = [torch.sigmoid(torch.randn(c.shape, device=dev, generator=g2) * 1.5 - 4.6).to(tdt) for c in conf]
    r_loc = [(torch.randn(l.shape, device=dev, generator=g2) * 0.5).to(tdt) for l in loc]
    r_scan, r_tail, r_nms, r_whole = stage_times(r_loc, r_conf)
    i_scan, i_tail, i_nms, i_whole = stage_times(list(loc), list(conf))  # the bench's own heads, in line

    # ---- per-layer table (separate, untimed pass: one hipEvent per op of the recorded plan) ------------------
    layers, heads, body = None, None, None
    timed_kernels = None  # kernel name per op of the timed plan (forward_check compares its own plan's with these)
    if (plan is None or isinstance(plan, str)) and plans:
        plan = plans[0]  # FPN / BiFPN: the recorded plan of backbone + neck + shared towers (NeckPlanMixin)
    if plan is not None and not isinstance(plan, str):
        plan.ctx.set_side_lane(False)  # per-op times are taken in line (on two streams the intervals of neighbouring ops overlap)
        plan.ctx.set_op_profiling(True)
        acc = None
        with torch.no_grad():
            for _ in range(5):
                model(x)
                torch.cuda.synchronize(dev)
                t = plan.ctx.op_timings()
                acc = [a + b[1] for a, b in zip(acc, t)] if acc else [b[1] for b in t]
        plan.ctx.set_op_profiling(False)
        plan.ctx.set_side_lane(None)
        names = [k for k, _ in t]
        timed_kernels = list(names)
        layers = []
        for row, kern, ms5 in zip(plan.layer_table(), names, acc):
            ms = ms5 / 5.0
            layers.append({"layer": row["name"], "kernel": kern.replace("_kernel", ""), "us": round(ms * 1e3, 1),
                           "TFLOPs": round(row["flops"] / (ms * 1e-3) / 1e12, 1),
                           "GBps": round(row["bytes"] / (ms * 1e-3) / 1e9, 0), "kind": row["kind"]})
        hl = [(r, l) for r, l in zip(plan.layer_table(), layers) if r["kind"] in ("head", "tower")]
        h_flops = sum(r["flops"] for r, _ in hl)
        h_ms = sum(l["us"] for _, l in hl) * 1e-3
        bl = [(r, l) for r, l in zip(plan.layer_table(), layers) if r["kind"] in ("mbconv", "conv", "dw", "gconv", "stem", "pool", "fuse")]
        b_ms = sum(l["us"] for _, l in bl) * 1e-3
        b_bytes, b_flops = sum(r["bytes"] for r, _ in bl), sum(r["flops"] for r, _ in bl)
        body = {"ms": round(b_ms, 4), "algorithmic_bytes": b_bytes, "flops": b_flops,
                "achieved_GBps": round(b_bytes / (b_ms * 1e-3) / 1e9, 1), "hbm_frac": round(b_bytes / (b_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "achieved_TFLOPs": round(b_flops / (b_ms * 1e-3) / 1e12, 1),
                "note": "backbone + neck (every op of the plan that is not a head): the part of the step that dominates "
                        "by time; bytes = each op's input + output + weights once"}
        if h_ms > 0:
            # what an EMPTY event interval reads on this stack (two hipEventRecords back to back): every per-op time above
            # contains one.  `ms` / `frac` stay raw; `ms_net` / `frac_net` subtract it once per head op.
            nulls = []
            for _ in range(21):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                e1.record()
                torch.cuda.synchronize(dev)
                nulls.append(e0.elapsed_time(e1))
            null_ms = sorted(nulls)[len(nulls) // 2]
            net_ms = max(h_ms - len(hl) * null_ms, 1e-6)
            heads = {"flops": h_flops, "ms": round(h_ms, 4), "achieved_TFLOPs": round(h_flops / (h_ms * 1e-3) / 1e12, 1),
                     "peak_TFLOPs": MFMA_PEAK_TFLOPS, "frac": round(h_flops / (h_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                     "ops": len(hl), "empty_event_interval_us": round(null_ms * 1e3, 2), "ms_net": round(net_ms, 4),
                     "frac_net": round(h_flops / (net_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS, 4),
                     "note": "3x3 head convs of all levels (SSD: loc|conf as one GEMM per level; FPN / BiFPN: the 4+1 convs "
                             "of both shared towers on every level, fpn.py:10-18), summed algorithmic FLOPs / summed per-op "
                             "time, dense MFMA peak"}

    conf_bytes = sum(c.numel() * c.element_size() for c in conf)  # the scan kernel reads conf exactly once
    loc_bytes = sum(l.numel() * l.element_size() for l in loc)
    K, D, L = decoder.top_n_per_level, decoder.top_n, len(conf)
    stage_bytes = conf_bytes + loc_bytes + B * (2 * 24 * L * K + 24 * D)  # SURVEY.md 8d (1.465 MB/img at SSD@512 bf16)

    def stage(s_ms, t_ms, n_ms, whole_ms=None):
        """kernels_ms: one hipEvent interval per launch (scan16 | levelsel | nmswalk);
        stage_ms: ONE interval around the launches (what `stage_frac` uses when it was measured: every extra event costs ~4.6 us of GPU time on this
        stack and flushes the caches between the kernels it separates); else the sum of the three."""
        tot = whole_ms if whole_ms else s_ms + t_ms + n_ms
        kern = {"scan": round(float(s_ms), 5), "levelsel": round(float(t_ms), 5), "nmswalk": round(float(n_ms), 5)}
        return {"launches": 3, "kernels_ms": kern,
                "stage_ms": round(float(tot), 5),
                "stage_ms_is": "one event interval around the stage's 3 launches" if whole_ms else "sum of the intervals",
                "scan_GBps": round(conf_bytes / (s_ms * 1e-3) / 1e9, 1),
                "scan_frac": round(conf_bytes / (s_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "stage_GBps": round(stage_bytes / (tot * 1e-3) / 1e9, 1),
                "stage_frac": round(stage_bytes / (tot * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

    scan_gbs = conf_bytes / (scan_ms * 1e-3) / 1e9
    is_headline = os.path.basename(args.cfg) == "ssd_mobilenetv2_512.yml" and B == 64 and args.dtype == "bf16"
    traffic, traffic_src = scan_traffic_bytes(None if is_headline else os.path.splitext(os.path.basename(args.cfg))[0])
    # `frac` (hygiene item 9): the figure that can be reproduced from profiles/ -- algorithmic bytes over the
    # kernel's average duration in the committed rocprofv3 kernel trace of this command (all its launches: the timed loop's
    # all-ties input and the realistic heads of the stage measurement).  The live in-loop figure (a hipEvent pair around the
    # launch inside the timed region: + ~4.6 us of event interval, the forward's tail still draining) stays as `in_loop`.
    rp_ns, rp_calls, rp_src = scan_rocprof_avg_ns(None if is_headline else os.path.splitext(os.path.basename(args.cfg))[0])
    rp_gbs = conf_bytes / (rp_ns * 1e-9) / 1e9 if rp_ns else None
    roofline = {
        "kernel": "ssdk::scan16_kernel<%s> (threshold + exact top-k over the conf tensors, one pass)" % args.dtype,
        "bound": "hbm",
        "achieved": round(rp_gbs if rp_gbs else scan_gbs, 1),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round((rp_gbs if rp_gbs else scan_gbs) / HBM_PEAK_GBS, 4),
        "frac_source": ("%s: AverageNs %.0f over %d launches of this command's rocprofv3 --kernel-trace --stats run (replayed, not "
                        "a measurement of this run)" % (rp_src, rp_ns, rp_calls)) if rp_ns else "in_loop (no committed kernel trace of this configuration)",
        "in_loop": {"achieved": round(scan_gbs, 1), "frac": round(scan_gbs / HBM_PEAK_GBS, 4), "avg_launch_ms": round(float(scan_ms), 5),
                    "what": "hipEvents on the launch stream inside the timed region of THIS run, all-ties bench input"},
        "traffic": traffic,
        "traffic_source": (traffic_src + " (separate rocprofv3 --pmc FETCH_SIZE pass of this configuration's command, x2 gfx950 "
                           "correction; not a measurement of this run)") if traffic else None,
        "algorithmic_bytes_per_launch": int(conf_bytes),
        "avg_launch_ms": round(float(scan_ms), 5),
        "timing": "hipEvents on the launch stream inside the timed region (each event pair costs ~4.6 us of GPU time "
                  "on this stack: an empty interval measures 4.6 us)",
        "input": "reference init: every score is the same %s value just above the threshold (all ties)" % args.dtype,
        "decode_nms_stage": {
            "algorithmic_bytes": int(stage_bytes),
            "bench_input_overlapped": stage(scan_ms, tail_ms, nms_ms) if use_tail else None,
            "bench_input_in_line": stage(i_scan, i_tail, i_nms, i_whole),
            "realistic_heads_in_line": stage(r_scan, r_tail, r_nms, r_whole),
            "realistic_heads": "SURVEY 8d microbench heads, same shapes: conf = sigmoid(N(-4.6, 1.5^2)), loc = N(0, 0.5^2)",
        },
    }

    result = OrderedDict()
    name = "%s-%s@%d" % (cfg.MODEL.SSDS.upper().replace("SSD", "SSD", 1), cfg.MODEL.NETS, H)
    result["metric"] = "images/sec (fwd+decode+NMS) " + ("SSD-MobileNetV2@512" if is_headline else name)
    result["value"] = round(n_gpus * B * args.steps / elapsed, 2)
    result["unit"] = "images/sec"
    result["n_gpus"] = n_gpus
    result["steps"] = args.steps
    result["warmup"] = args.warmup
    result["ms_per_step"] = round(elapsed / args.steps * 1e3, 4)
    result["higher_is_better"] = True
    result["scaling"] = "weak"
    result["vs_baseline"] = None  # the reference publishes no numbers
    result["dtype"] = args.dtype
    result["data"] = "synthetic"
    result["verified"] = bool(verified)
    result["config"] = {
        "workload": ("SSD+MobileNetV2" if is_headline else name) + " @%dx%d %s, batch %d per GPU: backbone+neck+heads "
                    "forward, decode (thr .01, 300/level, rescore) + DIoU-NMS (.6, 100 dets); random-init weights "
                    "(reference init), torch.rand images resident in HBM" % (H, W, args.dtype, B),
        "cfg": os.path.relpath(args.cfg, ROOT),
        "batch_per_gpu": B,
        "global_batch": B * n_gpus,
        "image_size": [H, W],
        "parallelism": "replicas x%d (no collective)" % n_gpus,
        "fused_head_conv": os.environ.get("SSDK_FUSED_CONV", "1") != "0",
        "hipgraph": bool(args.graph),
        "decode_tail_stream": use_tail,
        "channels_last": bool(args.channels_last),
        "verification": "last step recomputed in line on one stream with a fresh Decoder: scores, boxes and classes "
                        "equal the timed loop's bit for bit",
    }
    result["roofline"] = roofline
    result["stages"] = {"forward_ms": round(fwd_ms, 4), "decode_nms_ms": round(dec_ms, 4)}
    if heads is not None:
        result["roofline"]["head_convs_mfma"] = heads
    if body is not None:
        result["roofline"]["backbone_by_time"] = body
    if layers is not None and args.layers:
        result["layers"] = layers
    if dumped is not None:
        result["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped, "of": "the last timed step, rank 0"}

    # ---- CPU leg (rank 0, N = 1), bounded sample of S images of the timed batch: -------------------------------------
    #   (1) checker: the numpy oracle's Decoder on the GPU's OWN head outputs of those images must reproduce the timed
    #       loop's detections (classes / order bit-exact, boxes 1e-3, scores 1e-4), and the GPU's heads must agree with
    #       the fp32 CPU forward of the same module (a wrong backbone decorrelates `loc`: cosine ~0; 16-bit rounding noise
    #       through the untrained network keeps it >= ~0.85) -- both go into `verified`;
    #   (2) baseline: torch fp32 forward + oracle decode + NMS of the same images, timed.
    if rank == 0 and world == 1 and args.cpu_sample > 0:
        from oracle import box_oracle as O  # checker / baseline only

        S = min(args.cpu_sample, B)
        config.reset_cfg()
        cfg2 = config.cfg_from_file(args.cfg)
        cpu_model = model_builder.create_model(cfg2.MODEL).eval()
        cpu_model.load_state_dict(cpu_state)
        xs = x[:S].float().cpu()
        oanch = OrderedDict((k, v.numpy()) for k, v in anchors.items())
        odec = O.Decoder(decoder.conf_threshold, decoder.nms_threshold, decoder.top_n, decoder.top_n_per_level,
                         decoder.rescore, decoder.use_diou)
        with torch.no_grad():
            cl, cc = cpu_model(xs[:1])  # warm (model and oracle)
            odec([t.numpy() for t in cl], [t.numpy() for t in cc], oanch)
            t0 = time.perf_counter()
            cl, cc = cpu_model(xs)
            odec([t.numpy() for t in cl], [t.numpy() for t in cc], oanch)
            cpu_s = time.perf_counter() - t0
        g_loc = [t[:S].float().cpu() for t in loc]
        g_conf = [t[:S].float().cpu() for t in conf]
        # Two stages, because the bench's own input ties EVERY raw score (reference init): the NMS order is then decided by
        # centre-rescored scores that differ in the last ulp, i.e. by the <= 1-ulp difference between the device's and
        # numpy's expf -- comparing final detections with an oracle that starts from the heads would compare two
        # arbitrary orders.  (a) per-level decode (order = raw score desc, flat index asc: exact under ties) of the GPU's
        # own heads: oracle vs device, classes bit-exact, boxes 1e-3, scores 1e-4; (b) the oracle's NMS on the DEVICE's
        # per-level output (same bits in -> same order) must give the device's final detections bit for bit; and the
        # sample decoded on its own must equal the timed batch's rows bit for bit (images are independent).
        from ssds.modeling.layers.box import decode_nms

        with torch.no_grad():
            (fs, fb, fc), (ms_, mb_, mc_) = decode_nms(
                [t[:S].contiguous() for t in loc], [t[:S].contiguous() for t in conf], anchors, decoder.conf_threshold,
                decoder.top_n_per_level, decoder.rescore, decoder.nms_threshold, decoder.top_n, decoder.use_diou,
                return_mid=True)
        torch.cuda.synchronize(dev)
        same_rows = all(torch.equal(a, b[:S]) for a, b in zip((fs, fb, fc), timed_out))
        wm = odec.decode_levels([t.numpy() for t in g_loc], [t.numpy() for t in g_conf], oanch)
        mid_ok = bool(np.array_equal(mc_.cpu().numpy(), wm[2]) and np.allclose(mb_.cpu().numpy(), wm[1], atol=1e-3, rtol=0)
                      and np.allclose(ms_.cpu().numpy(), wm[0], atol=1e-4, rtol=1e-4, equal_nan=True))
        wn = O.nms(ms_.cpu().numpy(), mb_.cpu().numpy(), mc_.cpu().numpy(), decoder.nms_threshold, decoder.top_n,
                   decoder.use_diou)
        nms_ok = all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((fs, fb, fc), wn))
        oracle_ok = bool(same_rows and mid_ok and nms_ok)
        if not oracle_ok:
            print("oracle check failed: sample rows equal the timed batch's %s, per-level decode vs oracle %s, oracle NMS on "
                  "the device's per-level output %s" % (same_rows, mid_ok, nms_ok), file=sys.stderr)
        # The reference-initialised network of the timed run cannot check the forward pass: its activations decay level by
        # level (box heads of ~1e-9 behind the first level, every class output = sigmoid(bias)), so any comparison on it
        # either has an absolute floor above the signal or compares rounding noise.  Reported for the record only:
        ref_init = {"loc_rms_per_level": ["%.1e" % float(rl.pow(2).mean().sqrt()) for rl in cl],
                    "loc_relative_rms_error": [float("%.3g" % (float((gl - rl).pow(2).mean().sqrt()) / max(float(rl.pow(2).mean().sqrt()), 1e-30)))
                                               for gl, rl in zip(g_loc, cl)],
                    "max_abs_conf_error": float("%.3g" % max(float((gc - rc).abs().max()) for gc, rc in zip(g_conf, cc))),
                    "part_of_verified": False}
        # The forward check that CAN fail (forward_check below): the same architecture with seeded O(1) weights and calibrated
        # BatchNorm statistics, the SAME batch shape (hence the same kernels: asserted by name), purely relative bars.
        fwd = forward_check(args, cfg2, x, xs, S, tdt, dev, timed_kernels)
        heads_ok = bool(fwd["ok"])
        result["verified"] = bool(verified and oracle_ok and heads_ok)
        result["forward_check"] = fwd
        result["forward_check"]["reference_init_heads_vs_fp32_cpu"] = ref_init
        result["config"]["verification"] += (
            "; numpy oracle on the GPU's own head outputs of %d images: per-level decode (classes bit-exact, boxes 1e-3, "
            "scores 1e-4), oracle NMS on the device's per-level output = the timed detections bit for bit: %s; forward pass: "
            "the same architecture with seeded, BatchNorm-calibrated weights at the timed batch shape (same kernels: %s) against "
            "its fp32 CPU forward on those images, centred relative rms error per head tensor <= 2 x the error of PyTorch-ROCm "
            "executing the module in %s + 0.02 and correlation with fp32 >= PyTorch-ROCm's - 0.05 - the sampling scatter of the tensor's size (worst ratio to the error bar %.2f): %s"
            % (S, oracle_ok, fwd["same_kernels_as_timed"], args.dtype, fwd["worst_ratio_to_bar"], heads_ok))
        if not (oracle_ok and heads_ok):
            print(json.dumps(result["config"]), file=sys.stderr)
            print(json.dumps(fwd), file=sys.stderr)
            raise SystemExit("bench.py: the timed outputs disagree with the oracle / the forward check failed -- no number reported")
        result["cpu_baseline"] = {
            "value": round(S / cpu_s, 3),
            "unit": "images/sec",
            "cores": int(torch.get_num_threads()),
            "kind": "port",
            "sample": "%d of the %d images of one batch: torch fp32 CPU forward of the same module (%d threads) "
                      "+ numpy oracle decode+NMS (1 thread), warmed, %.1f s" % (S, B, torch.get_num_threads(), cpu_s),
            "reference_on_build_host": reference_cpu_record(),
        }
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
