"""What the plane gradients of the camera head and the device-side compaction of the matched queries cost (csrc/two_view_train.hip), at
nq = 50 and 16 pairs (the reference's IMS_PER_BATCH) and 32 pairs.  Device events, warm-up, the median of 11, the two variants of each
comparison ALTERNATED in one process (a, b, a, b, ...), so clock and cache state drift hits both alike:
  1. CameraHeadTrainer.camera_head_losses + backward with plane_grads off and on (on: two launches of geo_sequence_backward, two of
     refine_score_maps_backward_geo per _Aux pass pair, and the 8-wide dX of the encoder's first Linear);
  2. ops.match_compact + ops.match_compact_backward against the same gather written in torch indexing on the same device, without a
     host sync (masked sort of match_q, gather, mask multiply, zero padding; scatter_add for the backward).
Writes profiles/two_view_bwd.txt.  Nothing is gated on these numbers."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import ops  # noqa: E402

NQ, NMAX = 50, 20


def alternated(fa, fb, reps, warmup=3):
    """median (min .. max) in ms of `reps` single calls of each of two variants, alternated, each call between two device events"""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ts = ([], [])
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            ts[k].append(ev[0].elapsed_time(ev[1]))
    out = []
    for t in ts:
        t.sort()
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def torch_compact(x, params, match_q, n):
    N, nq, _ = x.shape
    nmax = match_q.shape[1]
    key = torch.where(torch.arange(nmax, device=x.device)[None] < n[:, None], match_q, torch.full_like(match_q, nq)).long()
    srt, _ = key.sort(dim=1)
    live = (srt < nq)
    idx = srt.clamp(max=nq - 1)
    pad = lambda t: torch.cat([t, t.new_zeros(N, nq - nmax, t.shape[2])], 1)
    x_c = pad(x.gather(1, idx[..., None].expand(-1, -1, 256)) * live[..., None])
    p_c = pad(params.gather(1, idx[..., None].expand(-1, -1, 3)) * live[..., None])
    return x_c, p_c, idx, live


def torch_compact_backward(g_c, idx, live):
    N, nq, _ = g_c.shape
    nmax = idx.shape[1]
    return torch.zeros_like(g_c).scatter_add_(1, idx[..., None].expand(-1, -1, 256), g_c[:, :nmax] * live[..., None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_view_bwd.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    from nopesac_amd.training import CameraHeadTrainer
    from tests import golden_inputs as GI
    from tests.util import make_model, nhwc
    head = make_model(dev).camera_head_list[0]
    lines = ["plane gradients of the camera head and the compaction of the matched queries, nq = %d, %s" % (NQ, torch.cuda.get_device_name(0)),
             "one call between two device events, median (min .. max) of %d after 3 warm-up calls, the two variants alternated in one process" % a.reps, ""]
    for B in a.pairs:
        c = GI.camera_train_case(NQ, tuple([7, 2, 19, 33] * ((B + 3) // 4))[:B], 80)
        feats = {k: torch.cat([nhwc(c["feats1"][k]), nhwc(c["feats2"][k])]).to(dev) for k in ("res3", "res4", "res5")}
        d = lambda k: c[k].to(dev)
        tr = CameraHeadTrainer.from_head(head)
        planes = (d("planes1").requires_grad_(True), d("planes2").requires_grad_(True))
        fixed = (d("gt_planes1"), d("gt_planes2"), d("n1"), d("n2"), d("gt_A"), d("gt_pose"))
        tail = (d("n1"), d("n2"), d("A"), d("rand_rot"), d("rand_trans"))

        def run(flag):
            p = planes if flag else (planes[0].detach(), planes[1].detach())
            tr.backward(tr.camera_head_losses(head, feats, B, *fixed, *p, *tail, plane_grads=flag))
        (off, on) = alternated(lambda: run(False), lambda: run(True), a.reps)
        lines.append("%d pairs: CameraHeadTrainer.camera_head_losses + backward (108 tensors, no optimiser step)" % B)
        lines.append("  plane_grads=False %8.3f (%7.3f .. %7.3f) ms" % off)
        lines.append("  plane_grads=True  %8.3f (%7.3f .. %7.3f) ms   (+%.3f ms)" % (*on, on[0] - off[0]))
        N = 2 * B
        g = torch.Generator().manual_seed(3)
        x = torch.randn(N, NQ, 256, generator=g).to(dev)
        params = torch.randn(N, NQ, 3, generator=g).to(dev)
        mq = torch.stack([torch.randperm(NQ, generator=g)[:NMAX] for _ in range(N)]).to(torch.int32).to(dev)
        n = torch.randint(1, NMAX + 1, (N,), generator=g).to(torch.int32).to(dev)
        g_c = torch.randn(N, NQ, 256, generator=g).to(dev)

        def hip():
            _, _, _, rank, _ = ops.match_compact(x, params, mq, n)
            ops.match_compact_backward(g_c, rank)

        def eager():
            _, _, idx, live = torch_compact(x, params, mq, n)
            torch_compact_backward(g_c, idx, live)
        x_c, _, _, rank, _ = ops.match_compact(x, params, mq, n)
        tx, _, idx, live = torch_compact(x, params, mq, n)
        assert torch.equal(x_c, tx) and torch.equal(ops.match_compact_backward(g_c, rank), torch_compact_backward(g_c, idx, live))
        (th, te) = alternated(hip, eager, a.reps)
        lines.append("%d images: matched queries to the front + the scatter back (x [%d, %d, 256], nmax = %d)" % (N, N, NQ, NMAX))
        lines.append("  match_compact + backward (2 launches) %8.4f (%7.4f .. %7.4f) ms" % th)
        lines.append("  torch indexing, no host sync          %8.4f (%7.4f .. %7.4f) ms" % te)
        lines.append("")
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
