"""One optimiser step over the whole model, fused against per-trainer: the seven trainers of the synthetic checkpoint (652 tensors,
75.3 M floats) with seeded gradients, stepped (a) by optim.ModelOptimizer.step - upload, gather, norm, clip coefficient, step - and
(b) by the seven HeadTrainer.step_from_cfg calls on copies of the parameters (sumsq + scale_by + adamw_step per tensor), both with
SOLVER.CLIP_GRADIENTS full_model, in one process, alternating the two.

    python scripts/model_optimizer_bench.py                       # times, launch counts, bytes -> profiles/model_optimizer.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o opt -- python scripts/model_optimizer_bench.py --trace-steps 5 --trace-path fused
    python scripts/model_optimizer_bench.py --stats DIR/.../opt_kernel_stats.csv     # adds each launch's time and share of the copy rate
(--trace-path per_trainer traces the other path; --stats-parent adds its rows.)

Times are device events around a window of at least --window seconds of steps, after a warm-up of both paths, repeated --rounds times
(median, min .. max).  Bytes are what each streaming launch must move, from the sizes here; the rate they are held against is the
6.3 TB/s float4-copy rate of an MI355X.  A run without a GPU prints the counts and bytes and says that nothing was timed."""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import _lib, ops, optim  # noqa: E402
from nopesac_amd import training as T  # noqa: E402
from nopesac_amd.config import get_cfg  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402

COPY_RATE = 6.3e12                     # bytes / s, float4 copy on an MI355X
CALLS = []                             # (entry point, launches) since the last reset
# kernels of the two paths as a trace names them
FUSED_KERNELS = ("opt_gather_kernel", "sumsq_partial_kernel", "sumsq_final_kernel", "clip_coef_kernel", "opt_step_kernel")
PARENT_KERNELS = ("sumsq_accum_kernel", "sumsq_partial_kernel", "sumsq_final_kernel", "clip_coef_kernel", "scale_by_kernel", "adamw_step_kernel")


def record_library_calls():
    """Count every library call and the kernel launches behind it (sumsq above 16384 elements is two launches, everything else here one)."""
    _lib.load()
    entries = vars(_lib.C)

    def wrap(name, fn):
        def call(*args):
            CALLS.append((name, 2 if name == "nopesac_sumsq_accumulate_f32" and args[1] > 16384 else 0 if name == "nopesac_sumsq_workspace_floats" else 1))
            return fn(*args)
        return call
    for name, fn in list(entries.items()):
        entries[name] = wrap(name, fn)


def solver_cfg():
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.OPTIMIZER", "ADAMW", "SOLVER.BASE_LR", 1e-4, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.WEIGHT_DECAY_NORM", 0.0,
                         "SOLVER.BACKBONE_MULTIPLIER", 0.1, "SOLVER.CLIP_GRADIENTS.ENABLED", True, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model",
                         "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.01])
    return cfg


def trainers(sd, dev):
    return [T.BackboneTrainer.from_state_dict(sd, dev), T.CameraHeadTrainer.from_state_dict(sd, 50, dev, conv_stacks=True),
            T.MatchingHeadTrainer.from_state_dict(sd, 50, dev), T.PlaneInstanceHeadsTrainer.from_state_dict(sd, 50, dev),
            T.PlaneDecoderTrainer.from_state_dict(sd, 50, dev), T.PlanePyramidTrainer.from_state_dict(sd, dev),
            T.PlaneEncoderTrainer.from_state_dict(sd, dev)]


def seed_grads(trs, dev):
    g = torch.Generator(device="cpu")
    g.manual_seed(7)
    for tr in trs:
        for p in tr.params.values():
            p.grad = (torch.randn(p.shape, generator=g) * 1e-3).to(dev)


def stream_bytes(sizes):
    """The bytes each streaming launch of the fused step must move (AdamW), from the sizes alone."""
    n = sum(sizes)
    arena = ops.opt_unit_map(sizes)[2]
    return {"opt_gather_kernel": 4 * n + 4 * arena,                 # every gradient read once, every arena float written once
            "sumsq_partial_kernel": 4 * arena,                      # the arena read once
            "sumsq_final_kernel": 4 * 256,
            "opt_step_kernel": 4 * n * 4 + 4 * n * 3}               # p, G, M1, M2 read; p, M1, M2 written


def window(fn, seconds):
    """ms per call over a window of at least `seconds` between two device events."""
    steps = 1
    while True:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(steps):
            fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1])
        if ms >= 1e3 * seconds:
            return ms / steps, steps
        steps = max(steps + 1, int(steps * 1.3e3 * seconds / max(ms, 1e-3)))


def read_stats(path):
    """rocprofv3 --stats kernel rows -> {kernel name fragment: (calls, average ns)} for the kernels of both paths."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for frag in set(FUSED_KERNELS + PARENT_KERNELS):
                if frag in row["Name"]:
                    calls, avg = out.get(frag, (0, 0.0))
                    c = int(row["Calls"])
                    out[frag] = (calls + c, (avg * calls + float(row["AverageNs"]) * c) / (calls + c))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many steps of each path after a warm-up and exit (for a kernel trace)")
    ap.add_argument("--trace-path", choices=("fused", "per_trainer"), default="fused", help="the path a --trace-steps run executes (warm-up included)")
    ap.add_argument("--stats-parent", default=None, help="kernel stats CSV of a --trace-steps --trace-path per_trainer run")
    ap.add_argument("--stats", default=None, help="kernel stats CSV of a --trace-steps run: adds per-launch times to the report")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_optimizer.txt"))
    a = ap.parse_args()
    have_gpu = torch.cuda.is_available()
    dev = torch.device("cuda:0" if have_gpu else "cpu")
    sd = synth_state_dict(50)
    cfg = solver_cfg()
    fused_trs = trainers(sd, dev)
    sizes = [p.numel() for tr in fused_trs for p in tr.params.values()]
    nbytes = stream_bytes(sizes)
    res = {"tensors": len(sizes), "floats": sum(sizes), "below_4096": sum(1 for n in sizes if n < 4096), "stream_bytes": nbytes,
           "stream_bytes_total": sum(nbytes.values()), "traffic_floor_ms": 1e3 * sum(nbytes.values()) / COPY_RATE}
    lines = ["model optimiser: %d tensors, %d floats (%d tensors below 4096 elements), AdamW, full-model clip" % (res["tensors"], res["floats"], res["below_4096"]),
             "bytes the streaming launches of the fused step must move: " + ", ".join("%s %.1f MB" % (k, v / 1e6) for k, v in nbytes.items()),
             "  total %.2f GB; at the 6.3 TB/s float4-copy rate that is %.3f ms" % (res["stream_bytes_total"] / 1e9, res["traffic_floor_ms"])]
    if not have_gpu:
        lines.append("no GPU: nothing was timed, no launch was counted")
        print("\n".join(lines))
        print(json.dumps(res))
        return
    parent_trs = trainers(sd, dev)
    seed_grads(fused_trs, dev)
    seed_grads(parent_trs, dev)
    opt = optim.ModelOptimizer.from_cfg(fused_trs, cfg)
    lr = float(cfg.SOLVER.BASE_LR)

    def fused():
        opt.step(lr=lr)

    def parent():
        for tr in parent_trs:
            tr.step_from_cfg(cfg)
    if a.trace_steps:                                                 # one path alone, so that a trace's rows belong to it
        fn = fused if a.trace_path == "fused" else parent
        for _ in range(3 + a.trace_steps):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"path": a.trace_path, "steps": 3 + a.trace_steps}))
        return
    for _ in range(3):                                                # warm-up of both paths (code objects, moments, scratch)
        fused()
        parent()
    torch.cuda.synchronize()
    record_library_calls()
    for name, fn in (("fused", fused), ("per_trainer", parent)):
        del CALLS[:]
        fn()
        res[name + "_library_calls"] = len([c for c in CALLS if c[1]])
        res[name + "_kernel_launches"] = sum(c[1] for c in CALLS)
    torch.cuda.synchronize()
    times = {"fused": [], "per_trainer": []}
    for _ in range(a.rounds):
        for name, fn in (("fused", fused), ("per_trainer", parent)):
            ms, steps = window(fn, a.window)
            times[name].append(ms)
            res.setdefault(name + "_steps_per_window", []).append(steps)
    for name, ts in times.items():
        ts = sorted(ts)
        res[name + "_ms"] = {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "rounds": ts}
    f, p = res["fused_ms"], res["per_trainer_ms"]
    lines += ["kernel launches per step (library calls that launch; torch's own fills and the table upload not counted): fused %d (%d calls), per trainer %d (%d calls)"
              % (res["fused_kernel_launches"], res["fused_library_calls"], res["per_trainer_kernel_launches"], res["per_trainer_library_calls"]),
              "ms per step, device events around windows of >= %.1f s, %d alternating rounds, median (min .. max):" % (a.window, a.rounds),
              "  ModelOptimizer.step            %.3f (%.3f .. %.3f)" % (f["median"], f["min"], f["max"]),
              "  seven step_from_cfg            %.3f (%.3f .. %.3f)" % (p["median"], p["min"], p["max"]),
              "  ratio of medians %.1f x; the fused step's window holds the host's table fill and enqueue as well as the kernels" % (p["median"] / f["median"]),
              "  fused step against the traffic floor: %.1f x" % (f["median"] / res["traffic_floor_ms"])]
    if a.stats:
        stats = read_stats(a.stats)
        res["kernel_stats"] = {k: {"calls": c, "average_us": ns / 1e3} for k, (c, ns) in stats.items()}
        lines.append("per launch of the fused step, from a separate rocprofv3 --kernel-trace --stats run of that path alone: calls, average us,")
        lines.append("and for the streaming launches the share of the 6.3 TB/s copy rate that their bytes reach in that time:")
        for k in FUSED_KERNELS:
            if k in stats:
                c, ns = stats[k]
                share = "  %5.1f %% of the copy rate" % (100.0 * nbytes[k] / (ns * 1e-9) / COPY_RATE) if k in nbytes else ""
                lines.append("  %-22s %7d calls  %10.1f us%s" % (k, c, ns / 1e3, share))
        lines.append("  sum of the averages %.1f us per step" % sum(stats[k][1] / 1e3 for k in FUSED_KERNELS if k in stats))
        if a.stats_parent:
            pst = read_stats(a.stats_parent)
            res["kernel_stats_per_trainer"] = {k: {"calls": c, "average_us": ns / 1e3} for k, (c, ns) in pst.items()}
            lines.append("per launch of the per-trainer path, traced the same way:")
            for k in PARENT_KERNELS:
                if k in pst:
                    lines.append("  %-22s %7d calls  %10.1f us" % (k, pst[k][0], pst[k][1] / 1e3))
    else:
        lines.append("per-launch kernel times: not measured in this run (see the usage text: a separate kernel-trace run)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
