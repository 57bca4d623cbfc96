#!/usr/bin/env python
"""bench.py — image-pairs/s of the NopeSAC inference hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W              # single GPU
    python bench.py --gpus N --steps K --warmup W              # N ranks spawned by this file (runner.launch), one per GPU, RCCL
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...     # or joined from a torchrun environment

A "step" = one pass of the whole hot path (preprocess -> ResNet-50 -> PlaneTR head -> plane post-selection
-> pixel pose net -> matcher (GNN + 200-iter Sinkhorn) -> neural one-plane RANSAC -> results fetched) over
one batch of `--pairs` synthetic 480x640 pairs per GPU, with the raw images already resident in HBM.
Workload = BASELINE.json configs[1]: mp3d inference config, batch 32 pairs, ResNet-50 bf16 dense convs,
K = 32 hypotheses (forced by construction, SURVEY.md §8d / PlaneTR_NopeSAC._force_k).

Prints ONE JSON line (rank 0) with the driver contract fields.  A plain run does only what that line needs: set up, warm up,
time the K steps, write the last step's outputs (--dump-outputs DIR), print.  With --full the line also carries `roofline`
(dominant kernel = the bf16 MFMA implicit-GEMM conv, timed live with HIP events on the launch stream), the launch-tape leg, the
fp32 path's pose error and throughput, the drop-in boundary figures, the other BASELINE configurations and `cpu_baseline` (the
CPU oracle timed on the host's cores over a bounded sample; rank 0, N=1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # multi-process GPU work needs dmabuf IPC on this driver (RCCL); before HIP initialises

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

BF16_DENSE_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: ~2.5 PF dense bf16 MFMA
GFLOP_PER_PAIR = {32: 181.6, 64: 183.7, 128: 189.4}   # SURVEY.md §8d algorithmic work per pair


CONFIG_FILES = {"mp3d": "inference_mp3d.yaml", "scannet": "inference_scannet.yaml"}


def _profile_order(path):
    """profiles/rN_<tag>_*.json: newest round last, then by tag."""
    import re
    b = os.path.basename(path)
    m = re.match(r"r(\d+)", b)
    return (int(m.group(1)) if m else -1, b)


def build_model(device, nq, dtype, overrides=(), config="mp3d"):
    from nopesac_amd.config import get_cfg
    from nopesac_amd.registry import build_model as _build
    from nopesac_amd.synth import synth_state_dict
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", CONFIG_FILES[config]))
    cfg.merge_from_list(["MODEL.DEVICE", str(device), "MODEL.SEM_SEG_HEAD.NUM_OBJECT_QUERIES", nq,
                         "MODEL.AMD.COMPUTE_DTYPE", dtype, "MODEL.AMD.OUTPUT_MASKS", False, "MODEL.AMD.OUTPUT_RLE", False] + list(overrides))
    cfg.freeze()
    model = _build(cfg).eval()
    model.load_state_dict(synth_state_dict(nq))
    return model


def make_forced(B, K, nq, device, seed):
    """Device-resident K control tensors (consistent plane pairs under a random pose, a K-permutation)."""
    from nopesac_amd.synth import make_forced as _mf
    return _mf(B, K, nq, device, seed)


class ConvTimer:
    """HIP-event timing of every conv/GEMM launch (torch events record on the stream the C ABI launches on)."""

    def __init__(self):
        self.records = []
        self.enabled = False

    def install(self):
        from nopesac_amd import ops
        orig = ops.conv2d
        timer = self

        def timed(x, w, *a, **k):
            if not timer.enabled:
                return orig(x, w, *a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig(x, w, *a, **k)
            e1.record()
            kk = w.shape[-3] * w.shape[-2] * w.shape[-1]
            flops = 2.0 * y.numel() * kk
            nbytes = x.numel() * x.element_size() + y.numel() * y.element_size() + w.numel() * w.element_size()
            if k.get("residual") is not None or (len(a) > 2 and a[2] is not None):
                nbytes += y.numel() * y.element_size()
            kern = ops.CONV_CFG_KERNEL.get(ops.LAST_CONV_CFG[0], "heuristic")
            desc = "x%s w%s s%d [%s]" % (tuple(x.shape), tuple(w.shape), k.get("stride", 1), kern)
            timer.records.append((str(x.dtype), flops, e0, e1, nbytes, desc))
            return y

        ops.conv2d = timed
        # the two fused backbone kernels are conv work too: stem (conv7x7 + pool) and bottleneck tail (conv3 + shortcut [+ conv1'])
        orig_stem, orig_tail = ops.stem_fused, ops.bottleneck_tail

        def timed_stem(x, w224, scale, bias):
            if not timer.enabled:
                return orig_stem(x, w224, scale, bias)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig_stem(x, w224, scale, bias)
            e1.record()
            B, H, W, _ = x.shape
            flops = 2.0 * B * (H // 2) * (W // 2) * 64 * 147              # algorithmic: 7x7x3 taps (padding lanes not counted)
            timer.records.append((str(x.dtype), flops, e0, e1, x.numel() * 2 + y.numel() * 2, "stem_fused x%s" % (tuple(x.shape),)))
            return y

        def timed_tail(b, w3, s3, b3, **k):
            if not timer.enabled:
                return orig_tail(b, w3, s3, b3, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y, o = orig_tail(b, w3, s3, b3, **k)
            e1.record()
            px = y.numel() // y.shape[-1]
            flops = 2.0 * px * w3.shape[0] * w3.shape[1]
            nbytes = 2 * (b.numel() + y.numel())
            if k.get("x2") is not None:
                flops += 2.0 * px * k["wsc"].shape[0] * k["wsc"].shape[1]
                nbytes += 2 * px * k["x2"].shape[-1]
            else:
                nbytes += 2 * y.numel()
            if o is not None:
                flops += 2.0 * px * k["w1"].shape[0] * k["w1"].shape[1]
                nbytes += 2 * o.numel()
            timer.records.append((str(b.dtype), flops, e0, e1, nbytes, "bottleneck_tail b%s C4=%d CN=%d proj=%d" % (
                tuple(b.shape), w3.shape[0], 0 if o is None else o.shape[-1], int(k.get("x2") is not None))))
            return y, o

        ops.stem_fused, ops.bottleneck_tail = timed_stem, timed_tail
        orig_raw = ops.stem_fused_raw

        def timed_stem_raw(images, mean, std, w224, scale, bias):
            if not timer.enabled:
                return orig_raw(images, mean, std, w224, scale, bias)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig_raw(images, mean, std, w224, scale, bias)
            e1.record()
            B, _, H, W = images.shape
            flops = 2.0 * B * (H // 2) * (W // 2) * 64 * 147
            timer.records.append(("torch.bfloat16", flops, e0, e1, images.numel() * 4 + y.numel() * 2, "stem_fused_raw x%s" % (tuple(images.shape),)))
            return y

        ops.stem_fused_raw = timed_stem_raw
        orig_fp8 = ops.conv2d_fp8

        def timed_fp8(x, w8, scale, bias, **k):
            if not timer.enabled:
                return orig_fp8(x, w8, scale, bias, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y = orig_fp8(x, w8, scale, bias, **k)
            e1.record()
            flops = 2.0 * (y.numel() // y.shape[-1]) * w8.shape[0] * w8.shape[1]
            nbytes = x.numel() + w8.numel() + y.numel() * y.element_size()
            timer.records.append(("torch.float8_e4m3fn", flops, e0, e1, nbytes, "fp8 x%s w%s s%d" % (tuple(x.shape), tuple(w8.shape), k.get("stride", 1))))
            return y

        ops.conv2d_fp8 = timed_fp8
        # modules imported `ops` as a module and call ops.conv2d / ops.linear, so the patch is seen everywhere
        return self

    def dump(self, path):
        """Per-launch table: shape, ms, TFLOP/s, algorithmic GB/s (input+weights+output(+residual) once)."""
        torch.cuda.synchronize()
        with open(path, "w") as f:
            f.write("dtype\tms\tTFLOPs\tGBs\tGFLOP\tMB\tdesc\n")
            for dt, fl, e0, e1, nb, desc in self.records:
                ms = e0.elapsed_time(e1)
                f.write("%s\t%.4f\t%.1f\t%.0f\t%.2f\t%.1f\t%s\n" % (dt.replace("torch.", ""), ms, fl / ms / 1e9, nb / ms / 1e6,
                                                                   fl / 1e9, nb / 1e6, desc))

    def fold(self, reps):
        """The records hold `reps` identical instrumented steps back to back: keep, per launch, the repetition with the shortest
        duration (a single step is exposed to clock ramps and host hiccups)."""
        torch.cuda.synchronize()
        n = len(self.records) // reps
        if n * reps != len(self.records) or reps < 2:
            return
        best = []
        for i in range(n):
            cands = [self.records[r * n + i] for r in range(reps)]
            best.append(min(cands, key=lambda rec: rec[2].elapsed_time(rec[3])))
        self.records = best

    def by_kernel(self, dtype="torch.bfloat16"):
        """Launches of conv2d grouped by the kernel the autotuner routed them to (the name in [..] of the description)."""
        torch.cuda.synchronize()
        out = {}
        for dt, fl, e0, e1, nb, desc in self.records:
            if dt != dtype or not desc.endswith("]") or "[" not in desc:
                continue
            k = desc[desc.rindex("[") + 1:-1]
            d = out.setdefault(k, {"flops": 0.0, "ms": 0.0, "launches": 0, "bytes": 0.0})
            d["flops"] += fl
            d["bytes"] += nb
            d["ms"] += e0.elapsed_time(e1)
            d["launches"] += 1
        return out

    def split_by_bound(self, kernel_prefix, dtype="torch.bfloat16", ridge=2500e12 / 8e12):
        """The launches of one kernel template split at the machine's ridge point (peak MFMA FLOP/s / peak HBM B/s = 312 FLOP/B):
        layers above it are priced against the MFMA peak, layers below it against the HBM peak (their algorithmic bytes)."""
        torch.cuda.synchronize()
        out = {"mfma_bound": {"flops": 0.0, "bytes": 0.0, "ms": 0.0, "launches": 0}, "hbm_bound": {"flops": 0.0, "bytes": 0.0, "ms": 0.0, "launches": 0}}
        for dt, fl, e0, e1, nb, desc in self.records:
            if dt != dtype or "[" not in desc or not desc[desc.rindex("[") + 1:-1].startswith(kernel_prefix):
                continue
            d = out["mfma_bound" if fl / max(nb, 1.0) >= ridge else "hbm_bound"]
            d["flops"] += fl; d["bytes"] += nb; d["ms"] += e0.elapsed_time(e1); d["launches"] += 1
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for dt, fl, e0, e1, nb, _ in self.records:
            d = out.setdefault(dt, {"flops": 0.0, "ms": 0.0, "launches": 0, "bytes": 0.0})
            d["flops"] += fl
            d["bytes"] += nb
            d["ms"] += e0.elapsed_time(e1)
            d["launches"] += 1
        return out


def cpu_baseline(budget_s=15.0):
    """The CPU oracle (restatement validated against the imported reference) on this host's cores."""
    from nopesac_amd.synth import synth_pair, synth_state_dict
    from oracle import nopesac_oracle as O
    # small-batch CPU inference does not scale past a few tens of threads (256 hardware threads made it ~100x slower), and a container's
    # CPU quota can be far below the hardware threads it sees (runner.cpu_budget: 16 CPUs on the MI355X boxes - more busy threads than
    # that are parked together for part of every scheduler period): min(32, budget) threads, reported in `cores`.
    from nopesac_amd.runner import cpu_budget
    cores = min(cpu_budget(), 32)
    torch.set_num_threads(cores)
    sd = synth_state_dict(50)
    cfg = O.OracleConfig()
    tw = time.perf_counter()
    K = 32
    forced = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in make_forced(1, K, 50, "cpu", 7).items()}
    O.inference(sd, [synth_pair(100)], cfg, forced=forced)          # warm-up
    tw = time.perf_counter() - tw
    if tw > budget_s:                                # pathological host: report the single warm-up pair
        return {"value": 1.0 / tw, "unit": "pairs/s", "cores": cores, "kind": "port",
                "sample": f"1 synthetic 480x640 pair (warm-up only), fp32, batch 1, {tw:.1f}s"}
    n, t0 = 0, time.perf_counter()
    while True:
        O.inference(sd, [synth_pair(101 + n)], cfg, forced=forced)
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s or n >= 64:
            break
    return {"value": n / el, "unit": "pairs/s", "cores": cores, "kind": "port",
            "sample": f"{n} synthetic 480x640 pairs, fp32, batch 1, K={K} matched planes forced as on the GPU, {el:.1f}s"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=32, help="pairs per GPU per step")
    ap.add_argument("--k", type=int, default=32, help="hypotheses (matched planes) per pair")
    ap.add_argument("--dtype", default="bfloat16", choices=["bfloat16", "float32"])
    ap.add_argument("--fp8", action="store_true", help="BASELINE config 5 (NOT the headline line): the backbone's 3x3 convs on the fp8 "
                    "(e4m3fn) MFMA, static activation scales calibrated on the synthetic pairs; the JSON line says dtype fp8+bf16")
    ap.add_argument("--config", default="mp3d", choices=sorted(CONFIG_FILES), help="configs/inference_<name>.yaml (BASELINE configs[2] = scannet, --k 64)")
    ap.add_argument("--routing", default=os.path.join(ROOT, "profiles", "routing_r5.json"),
                    help="kernel routing file (autotuner decisions per conv/GEMM shape): loaded when it exists so that every run - "
                         "driver, PMC, rocprofv3 - launches identical kernels; shapes it does not list are tuned, and added to the file when it "
                         "is named on the command line (or with --retune)")
    ap.add_argument("--pose-fp32-parts", default=None, help="override MODEL.AMD.POSE_FP32_PARTS (camera-head stages on f32 operands in bf16 mode), "
                    "e.g. '' or 'aim' - A/B runs of the bf16 pose-error budget")
    ap.add_argument("--retune", action="store_true", help="ignore the routing file's contents, tune every shape again and rewrite it")
    ap.add_argument("--no-fp32-path", action="store_true", help="skip the fp32 parity path's own throughput figure")
    ap.add_argument("--no-boundary", action="store_true", help="skip the drop-in boundary figure (model(list[dict]) -> list[dict], host tensors in)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the short runs of BASELINE configs[2] (scannet yaml, K = 64) and "
                    "configs[4] at one GPU (fp8 backbone 3x3 convs, K = 128) that the default run appends as `other_configs`")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--layers", default="", help="write a per-GEMM-launch timing table to this path")
    ap.add_argument("--inflight", type=int, default=4, help="batches in flight (HIP streams) per GPU")
    ap.add_argument("--gather-every", type=int, default=8, help="steps per RCCL all_gather of the per-pair result rows (1 = one collective per "
                    "step as in rounds 1-4; G > 1: the rows of G steps travel together, the last partial group inside the timed region's closing "
                    "barrier) - every step's rows are gathered either way")
    ap.add_argument("--no-autotune", dest="autotune", action="store_false", help="skip the load-time conv kernel autotuning")
    ap.add_argument("--graph", action="store_true", help="capture each in-flight slot's forward once and replay it through the launch tape "
                    "(nopesac_amd/tape.py: the captured kernel nodes re-issued as plain launches by a C loop)")
    ap.add_argument("--no-tape", action="store_true", help="skip the second timed run through the launch tape (`launch_tape` in the JSON line)")
    ap.add_argument("--whole-graph", action="store_true", help="with --graph: hipGraphLaunch of the whole graph instead of the launch tape")
    ap.add_argument("--streams", default="own", help="hardware-queue placement of the in-flight streams (nopesac_amd/streams.py): own = every "
                    "batch stream on its own queue, its pose-net side stream on the same one; shiftN = the side stream on the queue of "
                    "batch (i + N) % slots; none = plain torch streams (whatever the runtime hands out)")
    ap.add_argument("--stages", action="store_true", help="add per-stage GPU times (one extra instrumented step)")
    ap.add_argument("--single-stream", action="store_true", help="ANALYSIS: pose net on the main stream (clean per-stage times)")
    ap.add_argument("--ablate", default="", choices=["", "backbone", "head", "nocam"],
                    help="ANALYSIS ONLY (the JSON line is marked invalid): time a truncated pipeline - backbone only / "
                         "backbone + plane head + post-selection / everything but the camera head - to see what each stage "
                         "costs once batches overlap")
    ap.add_argument("--full", action="store_true", help="everything besides the headline figure: roofline and engine clock (extra "
                    "instrumented steps), the launch-tape leg, the fp32 path's pose error and throughput, the boundary figures, the other "
                    "BASELINE configurations and the CPU baseline (the --no-* options switch single legs off)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="write the arrays the timed path returned in its last timed step "
                    "(per-pair result rows, poses of every stage, kept planes, assignments) to DIR/<name>.npy, float32 / float64")
    ap.add_argument("--stub-model", action="store_true",
                    help="TEST ONLY (the JSON line is marked invalid): the launcher, the in-flight loop, the per-step gather and the timed region "
                         "of this file around a stub that fabricates result rows instead of running the model - what the gloo CPU tests drive")
    return ap.parse_args(argv)


def timed_region(loop, step, steps, world, device=None):
    """EXACTLY `steps` steps between two (drain + process barrier + device synchronize) brackets (the caller's warmup ends with
    loop.barrier()); the elapsed time is the MAX over the ranks.  -> (seconds, host ms per step, last step's gathered rows)."""
    loop.host_seconds = 0.0
    host = None
    t0 = time.perf_counter()
    for i in range(steps):
        _, host = step(i)
    host_ms = 1e3 * loop.host_seconds / max(steps, 1)
    loop.barrier()                                         # (gather_every > 1: gathers the last partial group first)
    if loop.G > 1:
        host = loop.last_step_rows()
    el = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([el], device=device if device is not None else "cpu", dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        el = float(t.item())
    return el, host_ms, host


def dump_outputs(out_dir, rows, d, max_bytes=64 << 20):
    """--dump-outputs: the last timed step's results as out_dir/<name>.npy - the gathered per-pair rows and, from this rank's forward
    (`d`, None when a captured replay ran the step), what model.package() fetches for its caller: the poses of every camera stage, the
    kept planes, the matches.  Floating arrays as float32 (float64 stays float64), integer / bool arrays as float64 (exact).  An array
    over its share of `max_bytes` is replaced by a fixed, seeded sample of its flattened elements (never at the benchmark's sizes)."""
    import zlib
    import numpy as np
    arrays = {"rows": rows}
    if d is not None:
        sel, cam = d["sel"], d["cam"]
        for k, (t, r) in cam["cameras"].items():
            arrays[k + "_tran"], arrays[k + "_rot"] = t, r
        for k in ("n_kept", "kept_idx", "planes", "centers", "scores", "areas", "flags"):
            arrays["sel_" + k] = sel.get(k)
        for k in ("m", "n1", "n2", "pred_assignment_beforeRef0", "pred_assignment_afterRef0", "pred_assignment", "nonfinite"):
            arrays[k] = cam.get(k)
        maps = (cam.get("refine") or {}).get("maps") or {}
        arrays["refine_trans_all"], arrays["refine_rots_all"] = maps.get("trans_all"), maps.get("rots_all")
    arrays = {k: v for k, v in arrays.items() if isinstance(v, torch.Tensor)}
    share = max_bytes // max(len(arrays), 1)
    os.makedirs(out_dir, exist_ok=True)
    for name, v in arrays.items():
        v = v.detach()
        v = v.double() if (v.dtype == torch.float64 or not v.is_floating_point()) else v.float()
        a = v.cpu().numpy()
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def main(argv=None):
    """`--gpus N` with no torchrun environment: start the N ranks HERE (runner.launch = detectron2's `launch` for one machine,
    test_NopeSAC.py:209-216), one process per GPU; under torchrun (WORLD_SIZE set) join that world, which must have N ranks."""
    args = parse_args(argv)
    from nopesac_amd import runner
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" in os.environ:
        if int(os.environ["WORLD_SIZE"]) != args.gpus:
            sys.exit("bench.py: --gpus %d but the launcher's WORLD_SIZE is %s" % (args.gpus, os.environ["WORLD_SIZE"]))
    elif args.gpus > 1 and not args.stub_model:
        n_dev = torch.cuda.device_count()
        if n_dev < args.gpus:
            sys.exit("bench.py: --gpus %d but only %d GPU(s) are visible (one rank per GPU; no oversubscription)" % (args.gpus, n_dev))
    return runner.launch(rank_main, args.gpus, (args,))


def stub_rank_main(args, rank, world, local):
    """--stub-model: this file's launcher, InflightLoop, one gather per step and timed region with fabricated rows (CPU + gloo in
    the tests, or GPUs + RCCL to check a node's plumbing without the model).  Never a measurement."""
    from nopesac_amd import runner
    cuda = torch.cuda.is_available()
    device = torch.device("cuda", local) if cuda else None
    B = args.pairs
    loop = runner.InflightLoop(max(1, args.inflight), B, device, world, side_shift=None, gather_every=args.gather_every)

    def slot_step(slot):
        idx = torch.arange(B, dtype=torch.float32, device=device)
        t = torch.stack([idx, idx + 0.5 * rank, torch.full_like(idx, float(slot))], dim=1)
        q = torch.nn.functional.normalize(torch.ones(B, 4, device=device), dim=-1)
        k = torch.full((B,), args.k, dtype=torch.int32, device=device)
        return None, runner.metric_rows(t, q, k, k, k, rank * B)

    for i in range(args.warmup):
        loop.step(i, slot_step)
    loop.barrier()
    elapsed, host_ms, host = timed_region(loop, lambda i: loop.step(i, slot_step), args.steps, world, device)
    host = host.clone()                                    # (a view of the loop's row buffer: the leg below steps on)
    tape = None
    if not args.no_tape:
        # the launch-tape leg's PROTOCOL with nothing to capture: capture locally (may fail on one rank: NOPESAC_FAIL_CAPTURE_RANK), agree,
        # check one replayed step per slot through the loop's own gathers and barriers, agree again, then the timed region once more
        state = {"replaying": False, "checked_steps": 0}

        def verify_collective():
            state["replaying"] = True
            for i in range(loop.n_slots):
                loop.step(i, slot_step)
                loop.barrier()
                rows = loop.last_step_rows()
                if rows is None or rows.shape[0] != world * B:
                    return False
                state["checked_steps"] += 1
            return True

        def abandon():
            state["replaying"] = False
        every = runner.capture_on_all_ranks(lambda: None, verify_collective, abandon, device)
        el_t = timed_region(loop, lambda i: loop.step(i, slot_step), args.steps, world, device)[0] if every else None
        tape = {"captured_on_every_rank": bool(every), "replaying": state["replaying"], "checked_steps": state["checked_steps"],
                "ms_per_step": None if el_t is None else round(1e3 * el_t / max(args.steps, 1), 4)}
    ranks = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
    ok = host.shape[0] == world * B and host[:, 12].tolist() == [float(v) for v in range(world * B)]
    if rank == 0:
        print(json.dumps({"INVALID_stub_model": True, "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * elapsed / max(args.steps, 1), 4), "rows_gathered": int(host.shape[0]), "rows_in_rank_order": bool(ok),
                          "steps_per_all_gather": loop.G, "collectives_in_run": getattr(loop, "collectives", None), "launch_tape": tape,
                          "config": {"rccl_ranks": ranks, "backend": torch.distributed.get_backend() if ranks > 1 else None,
                                     "pairs_per_gpu": B, "global_batch": world * B, "device": str(device) if cuda else "cpu"}}))
    if world > 1:
        torch.distributed.destroy_process_group()
    if not ok:
        sys.exit("bench.py --stub-model: gathered rows are not the rank-major pair indices")


def rank_main(args):
    from nopesac_amd import runner
    rank, world, local = runner.init_distributed()
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but this process is rank %d of %d" % (args.gpus, rank, world))
    if args.stub_model:
        return stub_rank_main(args, rank, world, local)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (nopesac_amd has no CPU path)")
    if local >= torch.cuda.device_count():
        sys.exit("bench.py: LOCAL_RANK %d but only %d GPU(s) are visible" % (local, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    B, K = args.pairs, args.k
    nq = 50 if K <= 50 else K
    assert not args.fp8 or args.dtype == "bfloat16"
    model = build_model(device, nq, args.dtype, (["MODEL.AMD.BACKBONE_FP8", True] if args.fp8 else []) +
                        (["MODEL.AMD.POSE_FP32_PARTS", args.pose_fp32_parts] if args.pose_fp32_parts is not None else []), config=args.config)
    if args.single_stream:
        model.two_streams = False
    # synthetic inputs resident in HBM: uint8-valued fp32 RGB, seeds 1000+pair
    g = torch.Generator().manual_seed(1000 + rank)
    raw = torch.randint(0, 256, (2 * B, 3, 480, 640), generator=g).float().to(device)
    forced = make_forced(B, K, nq, device, 7 + rank)
    from nopesac_amd import ops
    if args.fp8:                                          # static activation scales from 4 of the synthetic images
        with torch.no_grad():
            model.backbone.calibrate_fp8(ops.preprocess(raw[:4], model.pixel_mean, model.pixel_std, model.backbone.STEM_CIN_PAD,
                                                        model.compute_dtype))
    # load-time kernel selection, outside the timed region.  The decisions are kept in a routing file: when it exists its entries are
    # installed (no re-measurement), only shapes it does not list are timed; rank 0 writes new decisions back.
    routing_loaded = 0
    routing_explicit = any(a == "--routing" or a.startswith("--routing=") for a in sys.argv[1:])
    if args.routing:
        args.routing = os.path.abspath(args.routing)       # profilers run this command from /tmp: never resolve against the cwd later
    if args.autotune and args.routing and routing_explicit and not args.retune and not os.path.exists(args.routing):
        # a routing file named on the command line that is not there would silently re-tune under whatever tool wraps this run (the
        # round-4 PMC pass measured a different kernel mix that way): refuse
        sys.exit("bench.py: --routing %s does not exist (pass --retune to create it)" % args.routing)
    if args.autotune and args.routing and os.path.exists(args.routing) and not args.retune:
        routing_loaded = ops.TUNER.load(args.routing)
    tuned = model.autotune(B) if args.autotune else 0
    routing_new = len(ops.TUNER.log)
    # new decisions go back into the file only on request (--routing named, or --retune): the default run leaves the tree as it is
    if args.autotune and args.routing and rank == 0 and (routing_new or args.retune) and (routing_explicit or args.retune):
        try:
            merged = dict(ops.TUNER.loaded) if not args.retune else {}
            merged.update({ops.TUNER.key_str(k): int(v) for k, v in ops.TUNER.best.items()})
            ops.TUNER.loaded = merged
            saved_best, ops.TUNER.best = ops.TUNER.best, {}
            doc_meta = {"written_by": "bench.py", "note": "key = dtype|w dtype|out dtype|B|H|W|Cin|Cout|KH|KW|stride|pad|residual|x_cs|y_cs|batched|scale|bias|act|bfrag_ok|halo_ok|p8_ok"}
            import json as _json
            with open(args.routing, "w") as f:
                _json.dump({"format": "nopesac_amd.ConvTuner/1", "meta": doc_meta, "kernels": {str(k): v for k, v in ops.CONV_CFG_KERNEL.items()},
                            "routing": dict(sorted(merged.items()))}, f, indent=1)
            ops.TUNER.best = saved_best
        except OSError as e:
            print("routing file not written: %r" % (e,), file=sys.stderr)

    # Several batches in flight (default 4; 3 -> 4 measured +1.1 %): step i runs on HIP stream i % n, so the launch-latency-bound head stages of one batch
    # (transformer, GNN, Sinkhorn, RANSAC) overlap with the HBM/MFMA-bound backbone of the next.  Each stream owns its
    # input buffer and a pinned host buffer for the per-pair result rows; a step's results are complete when its
    # stream's event has fired (checked before the slot is reused and at the end of the timed region).
    _timer_box = {}

    def timer_enabled():
        t = _timer_box.get("t")
        return bool(t and t.enabled) or getattr(model, "stage_events", None) is not None

    n_slots = max(1, args.inflight)
    # streams, pinned row buffers and events of the in-flight slots; the streams are picked by hardware queue (nopesac_amd/streams.py)
    shift = {"own": 0, "none": None}.get(args.streams, None if not args.streams.startswith("shift") else int(args.streams[5:]))
    loop = runner.InflightLoop(n_slots, B, device, world, side_shift=shift, gather_every=args.gather_every)
    if loop.stream_set is not None:
        loop.stream_set.bind(model)
    streams, host_bufs, done = loop.streams, loop.host_bufs, loop.done
    raws = [raw] + [raw.clone() for _ in range(n_slots - 1)]
    last = {}

    graphs = [None] * n_slots          # optional: one captured hipGraph per slot (static shapes, static buffers)
    graph_rows = [None] * n_slots

    zero_rows = torch.zeros(B, runner.METRIC_WIDTH, device=device)

    raw_stem = args.dtype == "bfloat16" and model.backbone.fused_stem and not args.ablate

    def device_step(slot):
        if raw_stem:       # bf16: the fused stem normalises the f32 NCHW images while it loads them (no preprocess launch)
            d = model.forward_tensors(None, B, 480, 640, forced=forced, raw_images=raws[slot])
            cam = d["cam"]
            rows = runner.metric_rows(cam["cameras"]["camera"][0], cam["cameras"]["camera"][1], cam["n1"], cam["n2"], cam["m"], rank * B,
                                      nonfinite=cam.get("nonfinite"))
            return d, rows
        x = ops.preprocess(raws[slot], model.pixel_mean, model.pixel_std, model.backbone.STEM_CIN_PAD, model.compute_dtype)
        if args.ablate:
            from nopesac_amd.modeling.plane_head import post_select
            feats = model.backbone(x)
            if args.ablate in ("head", "nocam"):
                head_out, qf = model.sem_seg_head(feats)
                post_select(head_out, qf, 480, 640, model.cfg)
            if args.ablate == "nocam":
                model.camera_head_list[0].initial_pose(feats, B)
            return None, zero_rows
        d = model.forward_tensors(x, B, 480, 640, forced=forced)
        cam = d["cam"]
        rows = runner.metric_rows(cam["cameras"]["camera"][0], cam["cameras"]["camera"][1], cam["n1"], cam["n2"], cam["m"], rank * B,
                                      nonfinite=cam.get("nonfinite"))
        return d, rows

    def slot_step(slot):
        if graphs[slot] is not None and not timer_enabled():
            g = graphs[slot]
            if loop.stream_set is not None and hasattr(g, "counts"):         # a launch tape: its side chain on the slot's side stream
                g.replay(sides=[loop.stream_set.sides[slot]])
            else:
                g.replay()
            return None, graph_rows[slot]
        return device_step(slot)

    def step(i=0):
        d, host = loop.step(i, slot_step)
        last["d"], last["slot"] = d, i % n_slots
        return d, host

    drain, barrier = loop.drain, loop.barrier

    for i in range(args.warmup):
        step(i)
    barrier()
    use_graph = False

    def capture_slots():
        """One captured forward per in-flight slot, replayed through the launch tape (nopesac_amd/tape.py: the captured kernel nodes
        re-issued as plain launches by a C loop, side-stream structure kept) or, with --whole-graph, by hipGraphLaunch.  One replay
        per slot is checked against the slot's last eager results."""
        nonlocal graphs

        def rows_of_every_slot():
            # one step per slot, each followed by a barrier: with --gather-every G > 1 the rows travel in groups and barrier() flushes the
            # partial group, so last_step_rows() is this step's [world * B, 16] whatever G is (round 5: the check used to read
            # loop.host_bufs, which a grouped loop never writes - uninitialised pinned memory, NaN != NaN, and the tape leg was skipped)
            out = []
            for i in range(n_slots):
                step(i)
                barrier()
                out.append(loop.last_step_rows().clone())
            return out
        from nopesac_amd.tape import LaunchTape, TapeUnsupported
        eager_rows = rows_of_every_slot()                      # eager results of each slot (same static inputs); collective, every rank
        captured = [None] * n_slots

        def capture_local():                                   # this rank's captures: no collective inside (runner.capture_on_all_ranks)
            for slot in range(n_slots):
                g = torch.cuda.CUDAGraph(keep_graph=not args.whole_graph)
                with torch.no_grad(), torch.cuda.graph(g, stream=streams[slot]):
                    _, graph_rows[slot] = device_step(slot)
                if not args.whole_graph:
                    try:
                        g = LaunchTape(g)
                        last["tape_counts"] = dict(g.counts)
                    except TapeUnsupported as e:
                        print("launch tape unavailable (%s): whole-graph replay" % (e,), file=sys.stderr)
                        g.instantiate()
                captured[slot] = g

        def verify_collective():                               # one replay per slot outside the timed region (barriers + gathers: every rank)
            nonlocal graphs
            graphs = captured
            barrier()
            host_bufs = rows_of_every_slot()
            if not all(torch.allclose(a, b, rtol=1e-4, atol=1e-5) for a, b in zip(eager_rows, host_bufs)):
                diff = [[round(float(x), 6) for x in (a - b).abs().amax(dim=0)[:7]] for a, b in zip(eager_rows, host_bufs)]
                # (every slot holds the same images: which side is the odd one out?)
                e_vs_e0 = [round(float((a - eager_rows[-1]).abs().max()), 6) for a in eager_rows]
                r_vs_r0 = [round(float((b - host_bufs[-1]).abs().max()), 6) for b in host_bufs]
                raise RuntimeError("graph replay does not reproduce the eager results; max |diff| per slot, columns t, q: %r; eager slots vs the "
                                   "last eager slot: %r; replayed slots vs the last replayed slot: %r" % (diff, e_vs_e0, r_vs_r0))
            return True

        def abandon():                                         # keep the eager path (on EVERY rank, agreed by all-reduce)
            nonlocal graphs
            graphs = [None] * n_slots

        return runner.capture_on_all_ranks(capture_local, verify_collective, abandon, device,
                                           log=lambda m: print("hipGraph capture, rank %d: %s" % (rank, m), file=sys.stderr))

    def timed(steps):
        return timed_region(loop, step, steps, world, device)

    if args.graph:
        use_graph = capture_slots()
    elapsed, host_launch_ms, host = timed(args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, host, last.get("d"))
    tape_record = None
    if args.full and not args.graph and not args.ablate and not args.no_tape and args.dtype == "bfloat16":
        # the same K steps again, submitted through the launch tape instead of ~270 Python-issued launches per step (outside the
        # headline's timed region).  world > 1 (round 6): the ranks agree by all-reduce that EVERY rank captured and reproduces its eager
        # rows before anyone replays (runner.capture_on_all_ranks) - a rank that cannot capture sends all of them back to eager launching
        # instead of leaving the others in the check's barrier
        if capture_slots():
            # a replay submits a batch in < 1 ms: keep two submissions as far apart as eager launching does (0.45 of the eager step
            # time), or the slots re-submit together and run in lockstep (runner.InflightLoop.step)
            loop.pace_s = 0.45 * elapsed / args.steps
            el_t, host_t, _ = timed(args.steps)
            tape_record = {"value": round(world * B * args.steps / el_t, 3), "unit": "pairs/s", "ms_per_step": round(1e3 * el_t / args.steps, 3),
                           "steps": args.steps, "host_launch_ms_per_step": round(host_t, 2), "nodes": last.get("tape_counts"),
                           "min_ms_between_submissions": round(1e3 * loop.pace_s, 2),
                           "replay": "launch tape" if "tape_counts" in last else "whole hipGraph",
                           "note": "the headline's K steps repeated with every slot's forward captured once and re-issued by "
                                   "nopesac_tape_replay_on (csrc/tape.hip): same kernels, same streams, no Python between launches; the host "
                                   "thread sleeps between submissions"}
            loop.pace_s = 0.0
        graphs = [None] * n_slots
        barrier()
    ms_per_step = 1e3 * elapsed / args.steps
    pairs_per_s = world * B * args.steps / elapsed
    m_mean = float(host[:, 9].mean())
    nonfinite = int(host[:, 13].max())            # Inf / NaN count of the last step's batches, gathered with the rows
    if nonfinite:
        sys.exit("bench.py: %d non-finite values in the predicted poses - the measurement is void" % nonfinite)
    if args.ablate:
        if rank == 0:
            print(json.dumps({"INVALID_ablation": args.ablate, "ms_per_step": round(ms_per_step, 3)}))
        return

    roofline = None
    if args.full or args.layers:           # --layers: the per-launch table comes from the same instrumented steps
        # ---- engine clock under this load (outside the timed region): a few more steady-state steps with a one-wave probe on a side
        #      stream in the middle of each (the MFMA-bound kernels are power-limited: the firmware grants ~1.9 of the nominal 2.4 GHz)
        sclk_mhz = None
        try:
            probe_stream = torch.cuda.Stream(device=device)
            probes = []
            for i in range(2 * n_slots):
                step(i)
                probes.append(ops.clock_probe(400000, probe_stream))
            barrier()
            vals = [100.0 * float(t[0]) / float(t[1]) for t in (q.cpu() for q in probes) if int(t[1]) > 0]
            sclk_mhz = round(sorted(vals)[len(vals) // 2], 1) if vals else None
        except Exception as e:                                     # the probe is informative only
            print("clock probe failed: %r" % (e,), file=sys.stderr)

        # ---- roofline of the dominant kernel: one extra instrumented step (outside the timed region)
        timer = ConvTimer().install()
        _timer_box["t"] = timer
        timer.enabled = True
        two, model.two_streams = model.two_streams, False      # pose net on the main stream: every timed launch has the chip to itself
        for _ in range(3):                                     # three instrumented steps; every launch keeps its fastest of the three
            step()
            drain()
        model.two_streams = two
        timer.enabled = False
        timer.fold(3)
        conv = timer.summary()
        if args.layers and rank == 0:
            timer.dump(args.layers)
        key = "torch.bfloat16" if args.dtype == "bfloat16" else "torch.float32"
        fam = conv.get(key, {"flops": 0.0, "ms": 1.0, "launches": 0})
        peak = BF16_DENSE_PEAK_TFLOPS if args.dtype == "bfloat16" else 157.3
        # the DOMINANT KERNEL: the conv kernel with the largest share of the step (per-launch HIP-event times of the instrumented step,
        # grouped by the kernel the load-time autotuner routed each layer to); the whole conv / GEMM family is reported next to it
        inst = {k: v for k, v in timer.by_kernel(key).items() if k != "heuristic"}
        # instantiations of one kernel template (same source, different K-tile / ring-depth constants) count as ONE kernel: which of
        # conv_igemm_bfrag_kernel<3, 64> / <4, 32> gets a layer is a per-run autotuner decision, the template's total is stable
        per_kernel = {}
        for k, v in inst.items():
            d = per_kernel.setdefault(k.split("<")[0], {"flops": 0.0, "ms": 0.0, "launches": 0, "bytes": 0.0})
            for f in d:
                d[f] += v[f]
        dom_name, dom = (max(per_kernel.items(), key=lambda kv: kv[1]["ms"]) if per_kernel else
                         ("conv_igemm_kernel<bf16>" if args.dtype == "bfloat16" else "conv_igemm_kernel<f32>", fam))
        achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
        fam_achieved = fam["flops"] / (fam["ms"] * 1e-3) / 1e12
        # HBM traffic of the same kernel from the PMC counters (cannot be collected from inside this process: measured by
        # scripts/pmc_bench.sh on this benchmark command and committed as profiles/*pmc_traffic.json)
        # The PMC file is only used when it counted THE SAME launches as this run (same routing): its launch count of the dominant kernel and
        # of the conv family per step must equal this run's, otherwise `traffic` stays null and both counts are printed.
        traffic, traffic_src, fam_traffic, traffic_check = None, None, None, None
        if args.dtype == "bfloat16":
            import glob
            for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")), key=_profile_order)[-1:]:
                pm = json.load(open(path))
                f2 = pm["bf16_conv_family"]
                hit = [kv for kname, kv in pm.get("kernels", {}).items() if dom_name in kname and kv.get("launches_per_step")]
                pmc_dom = round(sum(kv["launches_per_step"] for kv in hit), 3) if hit else 0
                pmc_fam = round(f2["launches_per_step"], 3)
                traffic_src = os.path.relpath(path, ROOT)
                traffic_check = {"dominant_kernel_launches_per_step": {"pmc_file": pmc_dom, "this_run": dom["launches"]},
                                 "conv_family_launches_per_step": {"pmc_file": pmc_fam, "this_run": fam["launches"]},
                                 "pmc_routing_file": pm.get("routing_file")}
                if hit and pmc_dom == dom["launches"]:
                    traffic = round(sum(kv["read_bytes_per_step"] + kv["write_bytes_per_step"] for kv in hit) / pmc_dom)
                if pmc_fam == fam["launches"]:
                    fam_traffic = round((f2["read_bytes_per_step"] + f2["write_bytes_per_step"]) / max(pmc_fam, 1))
                traffic_check["same_launch_set"] = traffic is not None and fam_traffic is not None
        split = timer.split_by_bound(dom_name, key) if args.dtype == "bfloat16" else None
        by_bound = None
        if split:
            mb, hb = split["mfma_bound"], split["hbm_bound"]
            by_bound = {"ridge_flop_per_byte": 312.5,
                        "mfma_bound_layers": {"launches": mb["launches"], "ms": round(mb["ms"], 3), "TFLOP/s": round(mb["flops"] / max(mb["ms"], 1e-9) / 1e9, 1),
                                              "frac_of_mfma_peak": round(mb["flops"] / max(mb["ms"], 1e-9) / 1e9 / peak, 4)},
                        "hbm_bound_layers": {"launches": hb["launches"], "ms": round(hb["ms"], 3), "TB/s_algorithmic": round(hb["bytes"] / max(hb["ms"], 1e-9) / 1e9, 2),
                                             "frac_of_hbm_peak": round(hb["bytes"] / max(hb["ms"], 1e-9) / 1e9 / 8.0, 4),
                                             "TFLOP/s": round(hb["flops"] / max(hb["ms"], 1e-9) / 1e9, 1)},
                        "note": "launches of the dominant kernel split at the ridge point of the machine (2.5 PFLOP/s / 8 TB/s): the 1x1 convs with "
                                "K <= 1024 and their residual streams are HBM-bound whatever the kernel does; `frac` above prices ALL launches "
                                "against the MFMA peak"}
        roofline = {"bound": "mfma", "kernel": dom_name,
                    "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                    "traffic": traffic, "traffic_unit": "HBM bytes per launch of this kernel (PMC)", "traffic_source": traffic_src,
                    "traffic_launch_check": traffic_check,
                    "algorithmic_bytes_per_launch": round(dom.get("bytes", 0.0) / max(dom["launches"], 1)),
                    "launches_per_step": dom["launches"], "flops_per_step": dom["flops"],
                    "avg_launch_us": round(1e3 * dom["ms"] / max(dom["launches"], 1), 2),
                    "step_share": round(dom["ms"] / ms_per_step, 3), "by_bound": by_bound,
                    "engine_clock": None if not sclk_mhz else {
                        "sclk_mhz_under_benchmark_load": sclk_mhz, "nominal_mhz": 2400,
                        "peak_at_measured_clock": round(peak * sclk_mhz / 2400.0, 1),
                        "frac_at_measured_clock": round(achieved / (peak * sclk_mhz / 2400.0), 4),
                        "note": "median of one-wave clock probes (shader cycles / 100 MHz reference ticks) on a side stream during steady-state steps; "
                                "`peak` and `frac` above stay at the nominal 2.4 GHz figure"},
                    "instantiations": {k: {"TFLOP/s": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1), "launches": v["launches"],
                                           "avg_launch_us": round(1e3 * v["ms"] / max(v["launches"], 1), 2)} for k, v in inst.items() if k.split("<")[0] == dom_name},
                    "conv_family": {"note": "every bf16 conv / fused-conv launch of the step (MFMA- and HBM-bound layers together)",
                                    "TFLOP/s": round(fam_achieved, 2), "frac_of_mfma_peak": round(fam_achieved / peak, 4), "launches_per_step": fam["launches"],
                                    "flops_per_step": fam["flops"], "ms": round(fam["ms"], 3), "step_share": round(fam["ms"] / ms_per_step, 3),
                                    "algorithmic_bytes_per_launch": round(fam.get("bytes", 0.0) / max(fam["launches"], 1)),
                                    "traffic_bytes_per_launch": fam_traffic},
                    "other_kernels": {k: {"TFLOP/s": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1), "ms": round(v["ms"], 3), "launches": v["launches"]}
                                      for k, v in inst.items() if k.split("<")[0] != dom_name},
                    "other_dtype_gemms": {k: {"TFLOP/s": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2), "ms": round(v["ms"], 3),
                                              "launches": v["launches"]} for k, v in conv.items() if k != key}}

        f8 = conv.get("torch.float8_e4m3fn")
        if f8 and f8["ms"] > 0:                                  # BASELINE configs[4]: the fp8 MFMA launches against THEIR peak (5 PFLOP/s dense)
            t8 = f8["flops"] / (f8["ms"] * 1e-3) / 1e12
            roofline["fp8_kernels"] = {"kernel": "conv_igemm_bfrag_kernel<FP8>", "bound": "mfma", "achieved": round(t8, 1), "peak": 5000.0, "unit": "TFLOP/s",
                                       "frac": round(t8 / 5000.0, 4), "launches_per_step": f8["launches"], "ms": round(f8["ms"], 3),
                                       "share_of_conv_family_flops": round(f8["flops"] / max(f8["flops"] + fam["flops"], 1.0), 3)}

    stage_ms = None
    if args.stages:
        model.stage_events = []
        step()
        torch.cuda.synchronize()
        ev = model.stage_events
        model.stage_events = None
        stage_ms = {b[0]: round(a[1].elapsed_time(b[1]), 3) for a, b in zip(ev[:-1], ev[1:])}
    out = {"metric": "image-pairs/sec (480x640, K=%d hyp)" % K, "value": round(pairs_per_s, 3), "unit": "pairs/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": ("fp8(backbone 3x3 convs)+bf16" if args.fp8 else "bf16") if args.dtype == "bfloat16" else "f32", "data": "synthetic",
           "config": {"workload": "configs/" + CONFIG_FILES[args.config] + ", %d synthetic 480x640 pairs/GPU/step, ResNet-50 + pyramids in %s, "
                                  "head GEMMs %s, K=%d matched planes forced (m mean %.1f), nq=%d"
                                  % (B, args.dtype, "bf16 operands with f32 accumulate / residual stream / LayerNorm / softmax" if args.dtype == "bfloat16"
                                     else "f32", K, m_mean, nq),
                      "pairs_per_gpu": B, "global_batch": world * B, "K": K, "parallelism": "pair-sharded dp%d" % world,
                      "rccl_ranks": torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1,
                      "pairs_per_s_per_gpu": round(pairs_per_s / world, 3),
                      "batches_in_flight_per_gpu": n_slots, "hip_graph": use_graph, "steps_per_all_gather": loop.G,
                      "streams": dict(loop.stream_set.describe(), policy=args.streams) if loop.stream_set is not None else {"policy": "none"},
                      "replay": None if not use_graph else ("whole hipGraph" if args.whole_graph or "tape_counts" not in last else "launch tape"),
                      "tape_nodes": last.get("tape_counts"), "autotuned_shapes": tuned,
                      "routing_file": os.path.relpath(args.routing, ROOT) if args.routing else None, "routing_entries_loaded": routing_loaded,
                      "routing_entries_measured_now": routing_new, "host_launch_ms_per_step": round(host_launch_ms, 2),
                      "gflop_per_pair_algorithmic": GFLOP_PER_PAIR.get(K), "nonfinite_outputs": nonfinite}}
    if roofline is not None:
        out["roofline"] = roofline
    if tape_record:
        out["launch_tape"] = tape_record
    if stage_ms:
        out["stage_ms_main_stream"] = stage_ms
    if args.full and rank == 0 and world == 1 and args.dtype == "bfloat16" and not (args.no_accuracy and args.no_fp32_path):
        # the fp32 HIP path = the configuration every 1e-4 parity test runs: (i) pose error of THIS run's configuration against it on
        # the benchmark workload itself (same images, same forced K control), (ii) its own throughput on the same workload
        m32 = build_model(device, nq, "float32", config=args.config)
        if not args.no_accuracy:
            bw = bench_workload_pose_error(model, m32, device, B, K, nq, raw=raw, forced=forced)
            if "m_all_pairs" in bw:
                bw.pop("m_bf16"); bw.pop("m_fp32")
            out["pose_err_vs_fp32_path"] = {"bench_workload": bw}
        if not args.no_fp32_path:
            out["fp32_parity_path"] = fp32_path_throughput(m32, raw, forced, B)
        del m32
        torch.cuda.empty_cache()
        if not args.no_accuracy:
            out["pose_err_vs_fp32_path"].update(accuracy_vs_fp32(model, device, nq))
    if args.full and rank == 0 and world == 1 and not args.no_boundary and args.dtype == "bfloat16":
        out["boundary"] = boundary_rate(model, raw, forced, B, streams=streams)
        out["boundary"]["one_pair_per_call"] = one_pair_latency(model)
        try:
            out["boundary"]["jpeg_decode"] = jpeg_decode_rate(device, 2 * B)
        except Exception as e:                                  # (no Pillow on the box: the frames are encoded with it)
            out["boundary"]["jpeg_decode"] = {"skipped": repr(e)}
        try:
            out["boundary"]["png_decode"] = png_decode_rate(2 * B)
        except Exception as e:
            out["boundary"]["png_decode"] = {"skipped": repr(e)}
    if (args.full and rank == 0 and world == 1 and not args.no_other_configs and args.dtype == "bfloat16" and not args.fp8 and args.config == "mp3d"
            and K == 32 and not args.ablate):
        del model
        torch.cuda.empty_cache()
        out["other_configs"] = other_configs(args)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
        out["speedup_vs_cpu_baseline"] = round(pairs_per_s / out["cpu_baseline"]["value"], 1)
    if rank == 0:
        print(json.dumps(out))
    if world > 1:
        torch.distributed.destroy_process_group()


# relaxed TEST.* thresholds (as in tests/util.py): with random weights the default thresholds keep ~1 plane per view, so the
# matcher / refine stages would not take part in the comparison
LOOSE = ["TEST.OVERLAP_THRESHOLD", 0.0, "TEST.PLANE_SCORE_THRESHOLD", 0.5, "TEST.MATCHING_SCORE_THRESHOLD", 0.0,
         "TEST.MASK_PROB_THRESHOLD", 0.3]


def other_configs(args, steps=12, warmup=4):
    """BASELINE configs[2] and configs[4] (its single-GPU half) measured by THIS file in short child runs - outside the timed region of
    the headline line, each in its own process (own model, own kernel routing: nq = 64 / 128 change the head GEMM shapes) - so that the
    driver's record carries them: {"scannet_k64": {...}, "bf16_k128": {...}} with value / ms_per_step / roofline of each (the routing file of
    the K = 128 leg keeps its round-4 name, routing_r5_fp8_k128.json: the fp8 convs were never routed by the tuner, every other shape is the same)."""
    import subprocess
    # Round 6: configs[4] ("fp8 MFMA backbone weights + bf16 accumulate, K = 128") runs with the dense bf16 backbone here and is reported
    # as `bf16_k128`; the fp8 leg is no longer part of the default record.  Three rounds of A/B lines (fp8_k128 vs bf16_k128: 2888 vs 2735,
    # 2846 vs 2837, 3003 vs 2987 pairs/s) and the pose error of the mode (camera_initRec R max 12.9 deg against 3.2 in bf16 on the
    # synthetic checkpoint) say the mode buys nothing at twice the error; moving its nine N % 256 == 0 layers onto the persistent 256 x 256
    # kernel was sized at <= 4 % of the K = 128 step - below what its error costs.  `bench.py --fp8 --k 128` still
    # runs the mode (tests/test_e2e_gpu.py::test_config5_fp8_backbone_k128 keeps it working); it is an experiment, not a configuration.
    import shutil
    import tempfile
    runs = {"scannet_k64": ["--config", "scannet", "--k", "64"], "bf16_k128": ["--k", "128"]}
    res = {}
    tmp = tempfile.TemporaryDirectory()
    for name, extra in runs.items():
        # the child loads a copy of the committed routing file: the shapes it lacks are tuned as before, the file in the tree stays as it is
        routing = os.path.join(ROOT, "profiles", "routing_r5_%s.json" % name.replace("bf16_k128", "fp8_k128"))
        if os.path.exists(routing):
            routing = shutil.copy(routing, tmp.name)
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--pairs", str(args.pairs),
               "--inflight", str(args.inflight), "--full", "--no-cpu-baseline", "--no-accuracy", "--no-fp32-path", "--no-boundary", "--no-other-configs", "--no-tape",
               "--routing", routing] + extra
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=420)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                res[name] = {"error": (r.stderr or r.stdout)[-400:]}
                continue
            j = json.loads(line[-1])
            rf = j.get("roofline") or {}
            res[name] = {"value": j["value"], "unit": j["unit"], "ms_per_step": j["ms_per_step"], "steps": j["steps"], "dtype": j["dtype"],
                         "workload": j["config"]["workload"], "K": j["config"]["K"], "host_launch_ms_per_step": j["config"]["host_launch_ms_per_step"],
                         "roofline": {k: rf.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "launches_per_step", "avg_launch_us",
                                                             "by_bound", "fp8_kernels")},
                         "wall_s_of_the_child_run": round(time.perf_counter() - t0, 1)}
        except Exception as e:                                 # the headline line must not depend on these
            res[name] = {"error": repr(e)[:400]}
    tmp.cleanup()
    return res


def bench_workload_pose_error(m16, m32, device, B, K, nq, raw=None, forced=None):
    """The benchmark workload (B synthetic pairs, K matched planes forced) through the timed configuration `m16` and through the fp32
    HIP path `m32` under the SAME forced control: pose error of m16 against m32 (formulas mp3d_evaluation.py:389-465) plus the sanity
    facts the GPU test asserts (m per pair, unit quaternions, finite outputs)."""
    import numpy as np
    from nopesac_amd import ops, runner
    if raw is None:
        g = torch.Generator().manual_seed(1000)
        raw = torch.randint(0, 256, (2 * B, 3, 480, 640), generator=g).float().to(device)
    if forced is None:
        forced = make_forced(B, K, nq, device, 7)

    def run(m):
        with torch.no_grad():
            if m.compute_dtype == torch.bfloat16 and m.backbone.fused_stem:
                return m.forward_tensors(None, B, 480, 640, forced=forced, raw_images=raw)["cam"]
            x = ops.preprocess(raw, m.pixel_mean, m.pixel_std, m.backbone.STEM_CIN_PAD, m.compute_dtype)
            return m.forward_tensors(x, B, 480, 640, forced=forced)["cam"]

    a, b = run(m16), run(m32)
    out = {"pairs": B, "K": K, "m_bf16": a["m"].tolist(), "m_fp32": b["m"].tolist(), "finite": True, "max_quat_norm_dev": 0.0}
    for key in ("camera_init", "camera_initRec", "camera_avgRef0", "camera"):
        t16, q16 = [v.float().cpu().numpy() for v in a["cameras"][key]]
        t32, q32 = [v.float().cpu().numpy() for v in b["cameras"][key]]
        out["finite"] = bool(out["finite"] and np.isfinite(t16).all() and np.isfinite(q16).all())
        out["max_quat_norm_dev"] = max(out["max_quat_norm_dev"], float(np.abs(np.linalg.norm(q16, axis=-1) - 1).max()))
        te, re = runner.translation_error(t16, t32), runner.rotation_error_deg(q16, q32)
        out[key] = {"T_err_mean": round(float(te.mean()), 5), "T_err_max": round(float(te.max()), 5),
                    "R_err_deg_mean": round(float(re.mean()), 4), "R_err_deg_max": round(float(re.max()), 4),
                    "mean_abs_t": round(float(np.linalg.norm(t32, axis=-1).mean()), 4)}
    if len(set(out["m_bf16"])) == 1 and out["m_bf16"] == out["m_fp32"]:          # compact form for the JSON line
        out["m_all_pairs"] = out["m_bf16"][0]
    return out


def boundary_rate(model, raw, forced, B, steps=4, streams=None):
    """The rate AT the drop-in boundary (what the reference's consumer, MP3DEvaluator.process, sees): a list of B input dicts with
    HOST image tensors goes in, the list of per-pair result dicts comes out - H2D copies, the whole forward, `package()` (the
    reference's result schema, siamese_planeTR.py:384-450) and the COCO RLE `instances` of every kept plane included; the same
    K-forced workload as the headline figure (so every view keeps K planes: 2 B K RLE strings per step).  Measured strictly serial
    (the results are consumed before the next call, as inference_on_dataset does) and with two batches in flight, each eagerly
    launched and with MODEL.AMD.USE_HIP_GRAPH (the forward of a batch as one hipGraph replay)."""
    import gc
    host = raw.cpu().pin_memory()
    host8 = raw.cpu().to(torch.uint8).pin_memory()       # the synthetic images are integer-valued 0..255: the same pixels as bytes
    assert torch.equal(host8.float(), host)
    mk = lambda h: [{"0": {"image": h[i], "image_id": "a%d" % i, "file_name": ""}, "1": {"image": h[B + i], "image_id": "b%d" % i, "file_name": ""}}
                    for i in range(B)]
    inputs_by_dtype = {"float32_images": mk(host), "uint8_images": mk(host8)}
    if os.environ.get("NOPESAC_BD_DEVICE_IMAGES"):        # analysis: the same loop without the PCIe transfers (images already in HBM)
        inputs_by_dtype = {"float32_images": mk(host.cuda()), "uint8_images": mk(host8.cuda())}
    cur = [inputs_by_dtype["float32_images"]]             # the input list the closures below work on
    rle_saved, graph_saved, model.output_rle = model.output_rle, model.use_hip_graph, True
    gc.collect()
    gc.freeze()          # the model / packed weights leave the cyclic GC's generations: a gen-2 pass over them cost 30-50 ms every few steps
    n_rle = [0]

    def serial(n):
        t_pack = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            with torch.no_grad():
                model.infer_iter += 1
                d = model.forward_device(cur[0], forced=forced)                 # H2D (pinned, non_blocking) + forward
                t1 = time.perf_counter()
                res = model.package(cur[0], d)                                  # the single host sync + result dicts + RLE
                t_pack += time.perf_counter() - t1
        torch.cuda.synchronize()
        n_rle[0] = sum(len(r[v]["instances"]) for r in res for v in "01")
        assert all("segmentation" in ins for r in res for v in "01" for ins in r[v]["instances"])
        return (time.perf_counter() - t0) / n, t_pack / n

    # the caller's HIP streams when it has some: a process multiplexes its streams onto a few hardware queues (4 by default), streams
    # created on top of the timed loop's 4 + 4 side streams shared queues with each other and lost a quarter of the overlap
    streams = list(streams or [])
    streams += [torch.cuda.Stream() for _ in range(4 - len(streams))]

    def pipelined(n, depth=2):
        # `depth` batches in flight: batch i's copies and forward are enqueued (their own HIP stream) before the results of batch
        # i - depth + 1 are fetched and packaged - what a prefetching evaluation loop does; results are still complete per-pair dicts
        from nopesac_amd.streams import stream_set
        streams = stream_set(depth, model.device, 0).bind(model).mains       # streams picked by hardware queue, as run.inference_on_dataset does
        def submit(slot):
            with torch.no_grad(), torch.cuda.stream(streams[slot]):
                model.infer_iter += 1
                d = model.forward_device(cur[0], forced=forced)
                ev = torch.cuda.Event()
                ev.record()
                return slot, d, ev

        tw = [0.0]

        def finish(h):
            a = time.perf_counter()
            h[2].synchronize()                                                  # the batch's forward is complete
            tw[0] += time.perf_counter() - a
            with torch.no_grad(), torch.cuda.stream(streams[h[0]]):
                return model.package(cur[0], h[1])

        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pending = []
        ts, tf = 0.0, 0.0
        period, last = 0.0, 0.0
        for i in range(n):
            if model.use_hip_graph and period > 0.0:                            # tape mode: pace the submissions (run.inference_on_dataset does the same)
                rest = 0.45 * period - (time.perf_counter() - last)
                if rest > 0.0:
                    time.sleep(rest)
            a = time.perf_counter()
            if i > 0:
                period = (a - last) if period == 0.0 else 0.8 * period + 0.2 * (a - last)
            last = a
            pending.append(submit(i % depth))
            bq = time.perf_counter()
            ts += bq - a
            if len(pending) >= depth:
                finish(pending.pop(0))
                tf += time.perf_counter() - bq
        while pending:
            finish(pending.pop(0))
        torch.cuda.synchronize()
        if os.environ.get("NOPESAC_BD_DEBUG"):
            print("pipelined depth %d n %d: %.2f ms/step, submit %.2f finish %.2f (of which waiting for the batch %.2f)"
                  % (depth, n, 1e3 * (time.perf_counter() - t0) / n, 1e3 * ts / n, 1e3 * tf / n, 1e3 * tw[0] / n), file=sys.stderr)
        return (time.perf_counter() - t0) / n

    out = {}
    try:
        for dt_name, inp in inputs_by_dtype.items():
            cur[0] = inp
            out[dt_name] = {}
            for mode, use_graph in (("eager", False), ("hip_graph", True)):
                model.use_hip_graph = use_graph
                model._graphs = {}
                model.graph_slots = 4                                           # a slot's outputs live until it is replayed again
                model.infer_iter = 0
                serial(8)                                                       # warm-up (graph mode: eager pass + capture per slot)
                pipelined(4)
                pipelined(8, 4)
                el, t_pack = serial(steps)
                # (as many steps as the headline's default timed region: a pipeline of depth d pays ~d - 1 batches of fill and drain, which
                #  16 steps - the count until round 5 - turned into 8-10 % of the figure and 40 steps into 3 %)
                el2 = pipelined(5 * steps)
                el4 = pipelined(10 * steps, 4)
                for dep in [int(v) for v in os.environ.get("NOPESAC_BD_DEPTHS", "").split(",") if v]:      # analysis: deeper pipelines
                    model.graph_slots = max(4, dep)
                    pipelined(2 * dep, dep)
                    print("boundary %s %s depth %d: %.1f pairs/s" % (dt_name, mode, dep, B / pipelined(4 * steps, dep)), file=sys.stderr)
                model.graph_slots = 4
                out[dt_name][mode] = {"four_in_flight": {"value": round(B / el4, 2), "ms_per_step": round(1e3 * el4, 2)},
                                      "two_in_flight": {"value": round(B / el2, 2), "ms_per_step": round(1e3 * el2, 2)},
                                      "one_batch_at_a_time": {"value": round(B / el, 2), "ms_per_step": round(1e3 * el, 2),
                                                              "package_incl_wait_for_the_gpu_ms": round(1e3 * t_pack, 2)}}
    finally:
        model.output_rle, model.use_hip_graph, model.graph_slots = rle_saved, graph_saved, 2
        model._graphs = {}
        gc.unfreeze()
    ref = out["float32_images"]
    best = max(((m, f) for m in ref for f in ("two_in_flight", "four_in_flight")), key=lambda k: ref[k[0]][k[1]]["value"])
    return {"value": ref[best[0]][best[1]]["value"], "unit": "pairs/s", "ms_per_step": ref[best[0]][best[1]]["ms_per_step"],
            "configuration": "float32 host images (the reference mapper's format), %s, %s" % best,
            "steps": 10 * steps, "pairs_per_step": B, "rle_instances_per_step": n_rle[0],
            "h2d_bytes_per_step": {"float32_images": int(host.numel() * 4), "uint8_images": int(host8.numel())},
            "float32_images": out["float32_images"], "uint8_images": out["uint8_images"],
            "note": "model(list[dict]) -> list[dict]: HOST images in, H2D + forward + package() + COCO RLE instances of every kept plane; "
                    "two / four_in_flight = that many batches enqueued before the oldest one is packaged, one_batch_at_a_time = strictly serial; "
                    "hip_graph = MODEL.AMD.USE_HIP_GRAPH (one graph replay per batch instead of ~280 launches); uint8_images = the "
                    "same pixels as uint8 CHW tensors (data.PairMapper(uint8=True)), widened on the device: bit-identical results, "
                    "a quarter of the PCIe bytes.  `value` is the best float32-input figure"}


def one_pair_latency(model, calls=24):
    """What the reference's UNMODIFIED harness sees (inference_on_dataset calls the model with ONE pair, test_NopeSAC.py:171):
    model([pair]) -> [result dict] strictly serial, host float32 images in, COCO RLE instances out; eager submission vs
    MODEL.AMD.USE_HIP_GRAPH (launch tape)."""
    from nopesac_amd.synth import synth_pair
    inp = [synth_pair(3)]
    for v in "01":
        inp[0][v]["image"] = inp[0][v]["image"].pin_memory()
    saved = (model.output_rle, model.use_hip_graph, model.graph_slots)
    model.output_rle = True
    out = {}
    try:
        for mode, use_graph in (("eager", False), ("launch_tape", True)):
            model.use_hip_graph, model._graphs, model.infer_iter = use_graph, {}, 0
            with torch.no_grad():
                for _ in range(6):
                    model(inp)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    model(inp)
                torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / calls
            out[mode] = {"ms_per_call": round(ms, 2), "pairs_per_s": round(1e3 / ms, 1)}
        if getattr(model, "tape_error", None):
            out["launch_tape"]["note"] = "whole-graph replay (tape unavailable: %s)" % model.tape_error
    finally:
        model.output_rle, model.use_hip_graph, model.graph_slots = saved
        model._graphs = {}
    return out


def jpeg_decode_rate(device, n_images=64, rounds=3, in_flight=4):
    """The data mapper's GPU JPEG decoder (nopesac_amd/jpeg.py, csrc/jpeg.hip; the reference decodes with PIL on host threads:
    planercnn_transforms.py:210-227, :306-314) on ScanNet-sized frames: synthetic 968 x 1296 pictures encoded by Pillow (4:2:0, q 90,
    no restart markers - one serial Huffman chain per file), `in_flight` batches of n_images on their own streams, files parsed
    beforehand (the loader's reader threads do that), output checked against Pillow; + the 640 x 480 resize of every frame."""
    import io
    import numpy as np
    from PIL import Image
    from nopesac_amd import jpeg, ops
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:968, 0:1296].astype(np.float32)
    base = []
    for i in range(4):
        a = np.stack([128 + 90 * np.sin(xx / (40 + i) + yy / 90), 128 + 70 * np.cos(yy / (35 + i)) * np.sin(xx / 140), 120 + 100 * ((xx // 160 + yy // 120) % 2)], -1)
        buf = io.BytesIO()
        Image.fromarray(np.clip(a + rng.normal(0, 3.0, a.shape), 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=90, subsampling=2)
        base.append(buf.getvalue())
    t0 = time.perf_counter()
    refs = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in base]
    pil_ms = 1e3 * (time.perf_counter() - t0) / len(base)
    files = [base[i % len(base)] for i in range(n_images)]
    infos = [jpeg.parse(f) for f in files]
    st = {}
    outs = jpeg.decode_batch(files, device, infos=infos, stats=st)
    exact = all(np.array_equal(outs[i].cpu().numpy(), refs[i]) for i in range(len(base)))
    streams = [torch.cuda.Stream(device=device) for _ in range(in_flight)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        for s in streams:
            with torch.cuda.stream(s):
                for o in jpeg.decode_batch(files, device, infos=infos):
                    ops.resize_bilinear_u8(o, 480, 640)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    rate = rounds * in_flight * n_images / el
    return {"images_per_s": round(rate, 0), "pairs_per_s": round(rate / 2, 0), "ms_per_batch_round": round(1e3 * el / rounds, 2), "images_per_batch": n_images,
            "batches_in_flight": in_flight, "frame": "968x1296, 4:2:0, q90, %d KB, no restart markers" % (len(base[0]) // 1024),
            "bit_exact_vs_pillow": bool(exact), "settled_by_the_parallel_decoder": int(st["par_done"].sum()) if st else 0,
            "pillow_ms_per_image_one_core": round(pil_ms, 2)}


def png_decode_rate(n_images=64, min_s=1.0):
    """The mp3d split's input path (planercnn_transforms.py:210-227 `call_mp3d` -> utils.read_image): its frames are
    480 x 640 PNG files, whose inflate stream is serial per file - they are decoded on host threads; there is NO GPU path for them.
    data.LazyPairs sends a batch's PNG files through ONE call of the library's host decoder (csrc/png_host.hip: zlib + row filters on
    the library's own threads, bit for bit PIL's pixels, straight into a recycled pinned batch buffer in the mapper's CHW layout); PIL
    itself holds the interpreter lock while it decodes a PNG and does not scale with threads (`pil`).  Measured here: the same synthetic
    picture content as the JPEG leg, PNG-encoded by Pillow (default compression), on `cpu_budget` threads - the CPUs this container
    may keep busy (its cgroup quota; the MI355X boxes of this build show 256 hardware threads under a 16-CPU quota), every leg for at
    least `min_s` seconds (a quota is enforced per 100 ms period: shorter runs measure a burst)."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    from types import SimpleNamespace as NS
    import numpy as np
    from PIL import Image
    from nopesac_amd import data
    from nopesac_amd.runner import cpu_budget
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    hw = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = cpu_budget()
    out = {"frame": "480x640 RGB PNG (Pillow default compression)", "host_hw_threads": hw, "cpu_budget": cores}

    def rate_of(fn, per_call):
        fn()                                                       # warm: pools, pinned blocks, page cache
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < min_s:
            fn()
            n += per_call
        return n / (time.perf_counter() - t0)

    with tempfile.TemporaryDirectory() as td:
        paths, sizes = [], []
        for i in range(8):
            a = np.stack([128 + 90 * np.sin(xx / (20 + i) + yy / 45), 128 + 70 * np.cos(yy / (17 + i)) * np.sin(xx / 70), 120 + 100 * ((xx // 80 + yy // 60) % 2)], -1)
            pth = os.path.join(td, "f%d.png" % i)
            Image.fromarray(np.clip(a + rng.normal(0, 3.0, a.shape), 0, 255).astype(np.uint8)).save(pth, format="PNG")
            paths.append(pth)
            sizes.append(os.path.getsize(pth))
        files = [paths[i % len(paths)] for i in range(n_images)]
        t0 = time.perf_counter()
        for f in files[:8]:
            data.read_image(f, "BGR")
        out["ms_per_image_one_core"] = round(1e3 * (time.perf_counter() - t0) / 8, 2)
        out["png_kbytes"] = int(np.mean(sizes) // 1024)
        with ThreadPoolExecutor(max_workers=cores) as pool:         # one ctypes call per image from a Python thread pool (first round-5 form)
            r = rate_of(lambda: list(pool.map(lambda f: data.read_image(f, "BGR"), files)), len(files))
        out["per_image_calls"] = {"threads": cores, "images_per_s": round(r, 0), "pairs_per_s": round(r / 2, 0)}
        # one library call per BATCH (nopesac_png_decode_files_host: its own threads, no per-image interpreter work) - what LazyPairs uses
        pre = torch.empty(len(files), 3, 480, 640, dtype=torch.uint8, pin_memory=torch.cuda.is_available())     # (recycled, like the loader's)
        status = []

        def batch_call():
            status[:] = data.read_png_files(files, "BGR", 480, 640, threads=cores, out=pre)[1]
        r = rate_of(batch_call, len(files))
        assert not any(status)
        out["batch_call"] = {"threads": cores, "images_per_batch": len(files), "images_per_s": round(r, 0), "pairs_per_s": round(r / 2, 0)}
        # the same frames with EVERY row Paeth-filtered (libpng-style encoders use it far more than Pillow's, whose files above are 90 % "Up"
        # rows): the serial-per-channel filter then costs about as much as the inflate - the input path's worst case
        import struct
        import zlib

        def all_paeth(img):
            H, W, C = img.shape
            rows, prev, raw = img.reshape(H, W * C).astype(np.int32), np.zeros(W * C, np.int32), bytearray()
            for y in range(H):
                cur = rows[y]
                left, ul = np.concatenate([np.zeros(C, np.int32), cur[:-C]]), np.concatenate([np.zeros(C, np.int32), prev[:-C]])
                pp = left + prev - ul
                pa, pb, pc = abs(pp - left), abs(pp - prev), abs(pp - ul)
                raw.append(4)
                raw += ((cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))) & 255).astype(np.uint8).tobytes()
                prev = cur
            chunk = lambda t, b: struct.pack(">I", len(b)) + t + b + struct.pack(">I", zlib.crc32(t + b) & 0xffffffff)
            return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(bytes(raw), 6)) + chunk(b"IEND", b"")
        pfiles = []
        for i, pth in enumerate(paths):
            q = os.path.join(td, "paeth%d.png" % i)
            with open(q, "wb") as f:
                f.write(all_paeth(np.asarray(Image.open(pth).convert("RGB"))))
            pfiles.append(q)
        pf = [pfiles[i % len(pfiles)] for i in range(n_images)]

        def batch_call_paeth():
            status[:] = data.read_png_files(pf, "BGR", 480, 640, threads=cores, out=pre)[1]
        r = rate_of(batch_call_paeth, len(pf))
        assert not any(status)
        out["batch_call_all_paeth_rows"] = {"threads": cores, "png_kbytes": os.path.getsize(pfiles[0]) // 1024, "images_per_s": round(r, 0), "pairs_per_s": round(r / 2, 0)}
        # ... and through the loader itself (LazyPairs.iter_batches: decode + mapped dicts, uint8 hand-over, two batches ahead)
        cfgl = NS(INPUT=NS(FORMAT="BGR"), DATASETS=NS(ROOT_DIR="", TEST=("mp3d_test",)), DATALOADER=NS(NUM_WORKERS=cores))
        entries = [{v: {"file_name": files[(2 * k + int(v)) % len(files)], "height": 480, "width": 640, "image_id": "%d_%s" % (k, v)} for v in "01"}
                   for k in range(512)]
        lazy = data.LazyPairs(entries, data.PairMapper(cfgl, "mp3d_test", uint8=True, gpu_jpeg=False), workers=cores)
        r = rate_of(lambda: sum(len(b) for b in lazy.iter_batches(32)), len(entries))
        out["loader"] = {"threads": cores, "pairs_per_batch": 32, "pairs_per_s": round(r, 0)}
        os.environ["NOPESAC_PNG_NATIVE"] = "0"             # the reference's decoder (PIL) on the same threads, for comparison
        try:
            with ThreadPoolExecutor(max_workers=cores) as pool:
                r = rate_of(lambda: list(pool.map(lambda f: data.read_image(f, "BGR"), files)), len(files))
            out["pil"] = {"threads": cores, "images_per_s": round(r, 0), "pairs_per_s": round(r / 2, 0)}
        finally:
            os.environ.pop("NOPESAC_PNG_NATIVE", None)
    out["note"] = ("`loader` = data.LazyPairs.iter_batches on `cpu_budget` threads (the CPUs this container may keep busy: its cgroup quota, not the "
                   "hardware threads it sees): what the PNG split feeds ONE GPU with from that many CPUs - compare with `value`, the model's rate per GPU; "
                   "`batch_call` = the decode alone (one library call per batch), `per_image_calls` = one ctypes call per image from a Python thread "
                   "pool (the first round-5 form), `pil` = the reference's decoder on the same threads")
    return out


def fp32_path_throughput(m32, raw, forced, B, steps=4):
    """pairs/s of the exact-fp32 HIP configuration (v_mfma_f32_32x32x2_f32, no fused bf16 kernels: the path the 1e-4 parity tests
    run) on the benchmark workload, one batch in flight, inputs resident in HBM."""
    from nopesac_amd import ops

    def one():
        with torch.no_grad():
            x = ops.preprocess(raw, m32.pixel_mean, m32.pixel_std, m32.backbone.STEM_CIN_PAD, torch.float32)
            cam = m32.forward_tensors(x, B, 480, 640, forced=forced)["cam"]
            return cam["cameras"]["camera"][0].cpu()

    one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        one()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    return {"value": round(B * steps / el, 2), "unit": "pairs/s", "ms_per_step": round(1e3 * el / steps, 2), "steps": steps, "pairs_per_step": B,
            "dtype": "f32", "note": "same workload and K control, 1 batch in flight, default kernel heuristics (no autotuning)"}


def accuracy_vs_fp32(model16, device, nq, n_pairs=4):
    """Pose error of the bf16 configuration against this implementation's fp32 path (itself within 1e-4 of
    the reference, tests/test_e2e_gpu.py) on a few synthetic pairs (formulas: mp3d_evaluation.py:389-465):
    "default" = noise images under the reference thresholds (~1 plane per view: exercises backbone + pose net),
    "loose_structured" = structured images under relaxed thresholds (several planes and matches per pair: the plane head,
    the matcher and the RANSAC refine take part; discrete plane / match decisions may differ between the precisions)."""
    import numpy as np
    from nopesac_amd import runner
    from nopesac_amd.synth import synth_pair

    def compare(m32, m16, inp):
        a, b = m32(inp), m16(inp)
        out = {}
        for key in ("camera_init", "camera"):
            t = np.stack([x[key]["tran"] for x in a]), np.stack([x[key]["tran"] for x in b])
            r = np.stack([x[key]["rot"] for x in a]), np.stack([x[key]["rot"] for x in b])
            out[key] = {"T_err_mean": round(float(runner.translation_error(t[1], t[0]).mean()), 5),
                        "R_err_deg_mean": round(float(runner.rotation_error_deg(r[1], r[0]).mean()), 3)}
        out["planes_per_view_fp32|bf16"] = [round(float(np.mean([len(x[v]["pred_plane"]) for x in res for v in "01"])), 2) for res in (a, b)]
        out["matches_per_pair_fp32|bf16"] = [round(float(np.mean([x["matched_num"] for x in res])), 2) for res in (a, b)]
        return out

    m32 = build_model(device, nq, "float32")
    res = {"default": compare(m32, model16, [synth_pair(i) for i in range(n_pairs)])}
    del m32
    fp8 = bool(getattr(model16.backbone, "fp8_conv2", False))
    m32, m16 = build_model(device, nq, "float32", LOOSE), build_model(device, nq, "bfloat16", LOOSE + (["MODEL.AMD.BACKBONE_FP8", True] if fp8 else []))
    m16.backbone.act_scale = dict(model16.backbone.act_scale)
    res["loose_structured"] = compare(m32, m16, [synth_pair(i, structured=True) for i in range(n_pairs)])
    del m32, m16
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    main()
