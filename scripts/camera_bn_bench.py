"""The grouped training-mode BatchNorm launches of the camera head's conv stacks (csrc/camera_bn_train.hip) at the nine distinct layer
shapes of the pixel pose net at B = 8 pairs of 480 x 640 images (res3 at 60 x 80): the siamese tower's three resolutions with two groups
of B images, 256 channels, and a branch's six layers with one group of B pairs, 128 channels.  Per shape: statistics (with the running
update), apply and backward, each entry call between two device events, warmed up, the median of 7; the bytes the call cannot avoid
(statistics: c read once - the second pass hits the cache; apply: c read, y written; backward: dy and c read twice, dc written) over that
time as a share of the 6.3 TB/s float4-copy rate of an MI355X (profiles/model_optimizer.txt).  Then the whole
CameraHeadTrainer(conv_stacks=True).camera_head_losses forward + backward with batch_stats True against False.  Writes
profiles/camera_bn_train.txt.  Nothing is gated on these numbers."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.training import BN_EPS, BN_MOMENTUM  # noqa: E402

COPY_RATE = 6.3e12                     # bytes / s, float4 copy on an MI355X (profiles/model_optimizer.txt)
# (layer, groups, positions per image, channels): n = pairs x positions rows per group
SHAPES = [("convs_backbone.0/1", 2, 60 * 80, 256), ("convs_backbone.3/4", 2, 30 * 40, 256), ("convs_backbone.6/7", 2, 15 * 20, 256),
          ("branch.0", 1, 15 * 20, 128), ("branch.1", 1, 8 * 10, 128), ("branch.2", 1, 8 * 10, 128), ("branch.3", 1, 4 * 5, 128),
          ("branch.4", 1, 4 * 5, 128), ("branch.5", 1, 2 * 3, 128)]


def timed(fn, reps, warmup=3):
    """median, min, max of `reps` single calls (ms), each between two events, after `warmup` calls"""
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
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera_bn_train.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.pairs
    g = torch.Generator().manual_seed(11)
    lines = ["grouped training-mode BatchNorm of the camera head's conv stacks, %d pairs of 480 x 640, %s" % (B, torch.cuda.get_device_name(0)),
             "one entry call between two device events, median (min .. max) of %d after 3 warm-up calls; share = compulsory bytes over the "
             "time against the %.1f TB/s float4-copy rate" % (a.reps, COPY_RATE / 1e12),
             "launches per call: statistics 2, apply 1, backward 3 (whatever the number of groups)", ""]
    for name, G, pos, C in SHAPES:
        n = B * pos
        c = torch.randn(G * n, C, generator=g).to(dev)
        dy = torch.randn(G * n, C, generator=g).to(dev)
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        mean, _, rstd = ops.bn_train_grouped_stats(c, G, eps=BN_EPS, momentum=BN_MOMENTUM)
        full = c.numel() * 4
        calls = (("stats", lambda: ops.bn_train_grouped_stats(c, G, eps=BN_EPS, momentum=BN_MOMENTUM, running_mean=rm, running_var=rv), full),
                 ("apply", lambda: ops.bn_train_grouped_apply(c, gamma, beta, mean, rstd, ops.ACT_LEAKY, G), 2 * full),
                 ("backward", lambda: ops.bn_train_grouped_backward(dy, c, gamma, beta, mean, rstd, ops.ACT_LEAKY, G), 5 * full))
        lines.append("%-20s G = %d, n = %6d rows per group, C = %3d" % (name, G, n, C))
        for what, fn, nbytes in calls:
            med, lo, hi = timed(fn, a.reps)
            lines.append("  %-9s %8.4f (%7.4f .. %7.4f) ms   %8.3f MB   %5.1f %% of the copy rate"
                         % (what, med, lo, hi, nbytes / 1e6, 100.0 * nbytes / (med * 1e-3) / COPY_RATE))

    from nopesac_amd.training import CameraHeadTrainer
    from tests import golden_inputs as GI
    from tests.util import make_model, nhwc
    c = GI.camera_train_case(50, tuple([7, 2, 19, 33] * ((B + 3) // 4))[:B], 80)
    head = make_model(dev).camera_head_list[0]
    feats = {k: torch.cat([nhwc(c["feats1"][k]), nhwc(c["feats2"][k])]).to(dev) for k in ("res3", "res4", "res5")}
    d = lambda k: c[k].to(dev)
    lines += ["", "CameraHeadTrainer(conv_stacks=True): camera_head_losses forward + backward, %d pairs (no optimiser step)" % B]
    for flag in (False, True):
        tr = CameraHeadTrainer.from_head(head, conv_stacks=True, batch_stats=flag)

        def fwd_bwd():
            losses = tr.camera_head_losses(head, feats, B, d("gt_planes1"), d("gt_planes2"), d("n1"), d("n2"), d("gt_A"), d("gt_pose"), d("planes1"),
                                           d("planes2"), d("n1"), d("n2"), d("A"), d("rand_rot"), d("rand_trans"))
            tr.backward(losses)
        med, lo, hi = timed(fwd_bwd, a.reps)
        lines.append("  batch_stats=%-5s %8.3f (%7.3f .. %7.3f) ms" % (flag, med, lo, hi))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
