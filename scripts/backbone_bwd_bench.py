"""Backward of the backbone (csrc/backbone_bwd.hip, training.BackboneTrainer) at N = 8 images of 480 x 640:
(a) forward and backward of the trainer per stage (stem + pool, res2 .. res5) and as a whole;
(b) ops.conv2d_dgrad_strided against the scalar gather ops.conv2d_dgrad(stride=2) takes, at the six stride-2 layers.
Every figure: median (min .. max) of --reps single calls, each between two events, after warm-up; the engine clock is read on the
device at the end.  Prints one JSON line and writes profiles/backbone_bwd.txt.  `--images N` changes the batch."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import state_dict_spec, synth_tensor  # noqa: E402
from nopesac_amd.training import BACKBONE_MAPS, BackboneTrainer  # noqa: E402

H, W = 480, 640
# (layer, k, input h, w, Cin, Cout)
LAYERS = (("res3.0.conv2", 3, 120, 160, 128, 128), ("res4.0.conv2", 3, 60, 80, 256, 256), ("res5.0.conv2", 3, 30, 40, 512, 512),
          ("res3.0.shortcut", 1, 120, 160, 256, 512), ("res4.0.shortcut", 1, 60, 80, 512, 1024), ("res5.0.shortcut", 1, 30, 40, 1024, 2048))


def timed(fn, reps, warmup=2):
    """median, min, max (ms) of `reps` single runs, each between two events, after `warmup` runs"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_bwd.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N = a.images
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    lines, res = [], {"images": N, "size": [H, W], "reps": a.reps}

    # ---- (a) the trainer per stage
    sd = {k: synth_tensor(k, shape) for k, shape in state_dict_spec(50).items() if k.startswith("backbone.")}
    tr = BackboneTrainer.from_state_dict(sd, dev)
    x = torch.zeros(N, H, W, 4, device=dev)
    x[..., :3] = rnd(N, H, W, 3)
    lines.append("(a) BackboneTrainer per stage, ms: forward (tape kept) | backward from a unit-normal gradient at the stage's output")
    stages, t = {}, x
    for name in ("stem",) + BACKBONE_MAPS:
        src = t.detach().requires_grad_(name != "stem")
        run = (lambda s: tr.stem(s)) if name == "stem" else (lambda s, n=name: tr.stage(s, n))
        fwd = timed(lambda: run(src), a.reps)
        y = run(src)
        d = rnd(*y.shape)

        def bwd():
            tr._clear_grads()
            torch.autograd.backward(y, d, retain_graph=True)
        stages[name] = {"forward_ms": fwd, "backward_ms": timed(bwd, a.reps), "output": list(y.shape)}
        lines.append("  %-5s -> %-22s fwd %8.3f (%.3f .. %.3f)   bwd %8.3f (%.3f .. %.3f)" % ((name, tuple(y.shape)) + fwd + stages[name]["backward_ms"]))
        t = y.detach()
        del y, d
    cots = {k: rnd(*v.shape) for k, v in tr.forward(x).items()}
    whole_f = timed(lambda: tr.forward(x), a.reps)

    def step():
        tr.forward(x)
        tr.backward_from(cots)
    whole = timed(step, a.reps)
    res.update(stages=stages, forward_ms=whole_f, forward_backward_ms=whole)
    lines.append("  whole backbone: forward %.3f (%.3f .. %.3f), forward + backward_from at the four maps %.3f (%.3f .. %.3f)" % (whole_f + whole))
    del tr, cots

    # ---- (b) the strided dgrad against the gather
    lines.append("")
    lines.append("(b) input gradient of the six stride-2 layers, B = %d: ops.conv2d_dgrad_strided (parity GEMMs on the f32 MFMA) against" % N)
    lines.append("    ops.conv2d_dgrad(stride=2) (one scalar thread per input element); ms, TFLOP/s at 2 x the forward's MACs;")
    lines.append("    layers as the forward names them: Cin -> Cout, input h x w (the dgrad reads Cout channels of dY and writes Cin of dX)")
    layers = []
    for name, k, h, w, cin, cout in LAYERS:
        pad = (k - 1) // 2
        oh, ow = (h + 2 * pad - k) // 2 + 1, (w + 2 * pad - k) // 2 + 1
        dy, wt = rnd(N, oh, ow, cout), rnd(cout, cin, k, k) / (cin * k * k) ** 0.5
        out = torch.empty(N, h, w, cin, device=dev)
        new = timed(lambda: ops.conv2d_dgrad_strided(dy, wt, (h, w), stride=2, pad=pad, out=out), a.reps)
        a_new = out.clone()
        old = timed(lambda: ops.conv2d_dgrad(dy, wt, (h, w), stride=2, pad=pad, out=out), max(3, a.reps // 2), warmup=1)
        diff = float((a_new - out).abs().max() / out.abs().max())
        flop = 2.0 * N * oh * ow * cout * cin * k * k
        layers.append({"layer": name, "strided_ms": new, "gather_ms": old, "strided_tflops": flop / new[0] / 1e9, "speedup": old[0] / new[0],
                       "max_diff_over_max": diff})
        lines.append("  %-16s %4d -> %4d  %3d x %3d   strided %8.3f (%.3f .. %.3f) %6.1f TF   gather %9.3f (%.3f .. %.3f)   x%.1f   (max diff / max %.1e)"
                     % ((name, cin, cout, h, w) + new + (layers[-1]["strided_tflops"],) + old + (old[0] / new[0], diff)))
    res["layers"] = layers
    probe = ops.clock_probe()
    torch.cuda.synchronize()
    cyc, ticks = probe.tolist()
    res.update(device=torch.cuda.get_device_name(0), engine_clock_mhz=round(100.0 * cyc / max(ticks, 1), 1))
    head = ["Backward of the backbone at %d images of %d x %d, f32 (scripts/backbone_bwd_bench.py)" % (N, H, W),
            "%s, engine clock read on the device at the end %.0f MHz; median (min .. max) of %d single calls between two events, after warm-up"
            % (res["device"], res["engine_clock_mhz"], a.reps), ""]
    print("\n".join(head + lines))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(head + lines) + "\n")


if __name__ == "__main__":
    main()
