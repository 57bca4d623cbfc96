"""Backward of the pixel pose net's conv stacks at 16 pairs (32 images), 480 x 640 (csrc/conv_bwd.hip): per layer, the dgrad and wgrad
time next to the library's own f32 forward conv of the same layer (same FLOPs), and one full CameraHeadTrainer(conv_stacks=True) step
(forward, backward, AdamW).  Prints a table and one JSON line.  `--pairs N` changes the batch."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nopesac_amd import ops  # noqa: E402
from nopesac_amd.synth import state_dict_spec  # noqa: E402

P = "camera_head_list.0."
LAYERS = [("pixel_decoder.layer_3", (15, 20), 1), ("pixel_decoder.adapter_2", (30, 40), 1), ("pixel_decoder.layer_2", (30, 40), 1),
          ("pixel_decoder.adapter_1", (60, 80), 1), ("pixel_decoder.layer_1", (60, 80), 1), ("pixel_decoder.mask_features", (60, 80), 1),
          ("convs_backbone.0.0", (60, 80), 1), ("convs_backbone.1.0", (60, 80), 1), ("convs_backbone.3.0", (30, 40), 1),
          ("convs_backbone.4.0", (30, 40), 1), ("convs_backbone.6.0", (15, 20), 1), ("convs_backbone.7.0", (15, 20), 1)]
for _i, _hw in enumerate([(15, 20), (15, 20), (8, 10), (8, 10), (4, 5), (4, 5)]):
    LAYERS.append((f"convs_trans.{_i}.0", _hw, 0.5))                    # (one branch of two: images = pairs)


def timed(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    spec = state_dict_spec(50)
    rows, out = [], {"pairs": a.pairs}
    print("%-30s %9s %9s %9s %8s %8s %8s %6s %6s" % ("layer", "fwd us", "dgrad us", "wgrad us", "fwd TF", "dgr TF", "wgr TF", "dg/f", "wg/f"))
    for name, (H, W), per in LAYERS:
        Cout, Cin, k, _ = spec[P + name + ".weight"]
        s = 2 if name.startswith("convs_trans") and int(name.split(".")[1]) % 2 == 1 else 1
        pad = (k - 1) // 2
        B = int(2 * a.pairs * per)
        Cx = Cin + (-Cin) % 8
        x = torch.randn(B, H, W, Cx, device=dev)
        w = torch.randn(Cout, Cin, k, k, device=dev) / (Cin * k * k) ** 0.5
        w_f = torch.nn.functional.pad(w.permute(0, 2, 3, 1), (0, Cx - Cin)).contiguous()
        OH, OW = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
        dy = torch.randn(B, OH, OW, Cout, device=dev)
        flop = 2.0 * B * OH * OW * Cout * Cin * k * k
        tf = timed(lambda: ops.conv2d(x, w_f, stride=s, pad=pad)) * 1e3
        dx = torch.zeros(B, H, W, Cx, device=dev)
        td = timed(lambda: ops.conv2d_dgrad(dy, w, (H, W), stride=s, pad=pad, out=dx[..., :Cin])) * 1e3
        tw = timed(lambda: ops.conv2d_wgrad(x, dy, k, stride=s, pad=pad, cin=Cin)) * 1e3
        r = {"layer": name, "fwd_us": tf, "dgrad_us": td, "wgrad_us": tw, "fwd_tflops": flop / tf / 1e6, "dgrad_tflops": flop / td / 1e6,
             "wgrad_tflops": flop / tw / 1e6}
        rows.append(r)
        print("%-30s %9.1f %9.1f %9.1f %8.1f %8.1f %8.1f %6.2f %6.2f" % (name, tf, td, tw, r["fwd_tflops"], r["dgrad_tflops"], r["wgrad_tflops"],
                                                                         td / tf, tw / tf))
    out["layers"] = rows

    from nopesac_amd.training import CameraHeadTrainer
    from tests import golden_inputs as GI
    from tests.util import make_model, nhwc
    B = a.pairs
    c = GI.camera_train_case(50, tuple([7, 2, 19, 33] * ((B + 3) // 4))[:B], 80)
    head = make_model(dev).camera_head_list[0]
    feats = {k: torch.cat([nhwc(c["feats1"][k]), nhwc(c["feats2"][k])]).to(dev) for k in ("res3", "res4", "res5")}
    tr = CameraHeadTrainer.from_head(head, conv_stacks=True)
    d = lambda k: c[k].to(dev)

    def step():
        losses = tr.camera_head_losses(head, feats, B, d("gt_planes1"), d("gt_planes2"), d("n1"), d("n2"), d("gt_A"), d("gt_pose"), d("planes1"),
                                       d("planes2"), d("n1"), d("n2"), d("A"), d("rand_rot"), d("rand_trans"))
        tr.backward(losses)
        tr.step(lr=1e-6)

    out["train_step_ms"] = timed(step, a.steps)
    print("full CameraHeadTrainer(conv_stacks=True) step at %d pairs: %.2f ms" % (B, out["train_step_ms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
