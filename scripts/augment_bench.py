"""Times the training-time augmentation (nopesac_amd/augment.py, csrc/augment.hip) on 64 images of 480 x 640 and writes
profiles/augment.txt:

    python scripts/augment_bench.py [--out profiles/augment.txt] [--images 64] [--iters 200]

Legs: every row identity (a copy with a layout change), every row with every stage on (the worst case: jitter with hue, grey off so
that the colour reaches the blur, blur at sigma 2), and a table sampled with the reference's distribution; each with the uint8 CHW output
and with the normalised f32 NHWC output.  Every leg is timed with device events around `iters` back-to-back calls after a warm-up, the
legs taken in turn three times (the spread is printed).  Per leg: the bytes it must move (3 bytes per pixel read, once more for the
contrast pre-pass of rows that jitter, plus the output's 3 or 16 bytes per pixel) and the share of the 6.3 TB/s float4-copy rate of an
MI355X that these bytes reach in the measured time.  Last, the same sampled table through augment_pil (Pillow on the host) on 16
processes, as images per second.  A run without a GPU fails: nothing here is a CPU measurement of the kernels."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.3e12                     # bytes / s, float4 copy on an MI355X (profiles/model_optimizer.txt)
H, W = 480, 640


def _pil_worker(args):
    from nopesac_amd.augment import AugmentParams, augment_pil
    images, rows = args
    p = AugmentParams(rows)
    return sum(int(augment_pil(im, p.row(k))[0, 0, 0]) for k, im in enumerate(images))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment.txt"))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--cpus", type=int, default=16)
    a = ap.parse_args()
    import torch
    from nopesac_amd import augment as AUG
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU - nothing is timed without one")
    dev = torch.device("cuda:0")
    n = a.images
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    images = np.stack([np.clip(np.stack([(xx * (k % 5 + 1)) % 256, (yy * 3 + k) % 256, (xx + yy + 7 * k) % 256], -1) + rng.integers(-20, 20, (H, W, 3)),
                               0, 255).astype(np.uint8) for k in range(n)])
    src = torch.from_numpy(images).to(dev)
    mean, std = torch.tensor([103.53, 116.28, 123.675], device=dev), torch.tensor([1.0, 1.0, 1.0], device=dev)
    worst = AUG.AugmentRow(True, (AUG.SATURATION, AUG.HUE, AUG.BRIGHTNESS, AUG.CONTRAST), (1.37, 0.55, 1.8, 0.2), False, True, 2.0)
    sampled = AUG.sample_params(n, seed=0, step=0)
    tables = {"identity": AUG.AugmentParams.identity(n), "every stage on": AUG.AugmentParams.from_rows([worst] * n), "sampled": sampled}
    legs = [(name, form) for name in tables for form in ("u8 CHW", "f32 NHWC")]
    dev_tables = {k: t.to(dev) for k, t in tables.items()}

    def call(name, form):
        if form == "u8 CHW":
            return AUG.augment(src, dev_tables[name])
        return AUG.augment(src, dev_tables[name], chw=False, normalized=True, mean=mean, std=std)

    def nbytes(name, form):
        jit = int(((tables[name].rows["flags"] & AUG.JITTER) != 0).sum())
        return H * W * (3 * n + 3 * jit + (3 if form == "u8 CHW" else 16) * n)

    for leg in legs:
        for _ in range(10):
            call(*leg)
    torch.cuda.synchronize()
    times = {leg: [] for leg in legs}
    for _ in range(3):
        for leg in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                call(*leg)
            e1.record()
            e1.synchronize()
            times[leg].append(e0.elapsed_time(e1) / a.iters)
    s = sampled.rows["flags"]
    lines = ["training-time augmentation, %d images of %d x %d, %s" % (n, H, W, torch.cuda.get_device_name(0)),
             "device events around %d back-to-back calls per window, 3 windows per leg taken in turn: median (min .. max) ms per call of %d images"
             % (a.iters, n),
             "bytes: 3 per pixel read, 3 more for the contrast pre-pass of a row that jitters, 3 (u8 CHW) or 16 (f32 NHWC) written;",
             "share = those bytes over the time, against the %.1f TB/s float4-copy rate" % (COPY_RATE / 1e12),
             "sampled table: %d of %d rows jitter, %d grey, %d blur" % (((s & AUG.JITTER) != 0).sum(), n, ((s & AUG.GREY) != 0).sum(), ((s & AUG.BLUR) != 0).sum()), ""]
    for leg in legs:
        t = sorted(times[leg])
        b = nbytes(*leg)
        lines.append("  %-15s %-9s %8.4f (%7.4f .. %7.4f) ms   %7.1f k images/s   %7.2f MB   %5.1f %% of the copy rate"
                     % (leg[0], leg[1], t[1], t[0], t[2], n / t[1], b / 1e6, 100.0 * b / (t[1] * 1e-3) / COPY_RATE))
    # the same sampled table through Pillow on the host
    from concurrent.futures import ProcessPoolExecutor
    import multiprocessing as mp
    chunks = [(images[k::a.cpus], sampled.rows[k::a.cpus]) for k in range(a.cpus)]
    with ProcessPoolExecutor(max_workers=a.cpus, mp_context=mp.get_context("spawn")) as pool:
        list(pool.map(_pil_worker, chunks))                   # warm-up: imports
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            list(pool.map(_pil_worker, chunks))
        dt = (time.perf_counter() - t0) / reps
    lines += ["", "  augment_pil (Pillow on the host), the same sampled table on %d processes: %.1f images/s (%.1f ms for the %d images)"
              % (a.cpus, n / dt, dt * 1e3, n)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
