"""Byte-for-byte A/B of the two 256-row conv kernels (csrc/conv_p8.hip, csrc/conv_p8n.hip): the case lists of test_conv2d_p8,
test_conv2d_p8_stream_k, test_conv2d_p8n and test_conv2d_p8n_split_k with every variant, the tests' own seeded inputs, one sha256
per output.  Run it in a fresh process per build and compare the listings line by line:
  python scripts/conv_p8_ab.py                                    this tree's library
  NOPESAC_AB_LIBRARY=<other .so> python scripts/conv_p8_ab.py     another build of the library on the same inputs
"""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nopesac_amd import _lib, ops  # noqa: E402

P8_CASES = [(2, 30, 40, 256, 256, 3, 1, 1), (3, 31, 29, 128, 256, 3, 2, 1), (2, 24, 32, 512, 512, 1, 1, 0), (1, 15, 20, 64, 256, 3, 1, 1),
            (2, 9, 7, 64, 256, 1, 1, 0), (1, 17, 16, 128, 256, 1, 1, 0), (1, 12, 20, 192, 256, 1, 1, 0), (5, 60, 80, 64, 512, 3, 1, 1)]
P8_VARIANTS = [0, 32, 64, 0 | (3 << 8), 32 | (1 << 8)]
SK_CASES = [(2, 30, 40, 256, 256, 3, 1, 1), (3, 31, 29, 128, 256, 3, 2, 1), (2, 24, 32, 512, 512, 1, 1, 0), (1, 15, 20, 64, 256, 3, 1, 1),
            (2, 9, 7, 64, 256, 1, 1, 0), (1, 12, 20, 192, 256, 1, 1, 0), (5, 60, 80, 64, 512, 3, 1, 1), (16, 30, 40, 256, 256, 3, 1, 1)]
SK_VARIANTS = [0, 32, 32 | 64, 32 | (5 << 8), 0 | (19 << 8), 32 | (64 << 8)]
P8N_CASES = [(2, 30, 40, 128, 128, 3, 1, 1), (3, 31, 29, 128, 128, 3, 2, 1), (2, 24, 32, 512, 256, 1, 1, 0), (1, 15, 20, 64, 128, 3, 1, 1),
             (2, 9, 7, 64, 128, 1, 1, 0), (1, 17, 16, 128, 128, 1, 1, 0), (1, 12, 20, 192, 128, 1, 1, 0), (1, 12, 20, 256, 128, 1, 1, 0),
             (1, 12, 20, 320, 384, 1, 1, 0), (5, 60, 80, 64, 256, 3, 1, 1), (1, 15, 20, 2048, 128, 3, 1, 1)]
P8N_VARIANTS = [0, 32, 0 | (3 << 8), 32 | (1 << 8)]
SPLIT_CASES = [(2, 15, 20, 2048, 128, 3, 1, 1, 3, 0), (4, 15, 20, 2048, 128, 3, 1, 1, 8, 0), (1, 15, 20, 512, 128, 3, 1, 1, 5, 0),
               (1, 9, 7, 128, 128, 1, 1, 0, 2, 0), (3, 16, 16, 256, 256, 3, 2, 1, 4, 0), (6, 15, 20, 1024, 128, 3, 1, 1, 4, 3),
               (2, 12, 20, 320, 384, 1, 1, 0, 5, 0)]
ACTS = ["ACT_RELU", "ACT_NONE", "ACT_LEAKY"]


def main():
    device = torch.device("cuda")
    L = _lib.load()

    def inputs(case, residual):
        B, H, W, Cin, Cout, k, s, p = case[:8]
        g = torch.Generator().manual_seed(sum(case))
        x = torch.randn(B, Cin, H, W, generator=g).bfloat16()
        w = (torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)).bfloat16()
        scale, bias = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
        OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        res = torch.randn(B, Cout, OH, OW, generator=g).permute(0, 2, 3, 1).contiguous().to(device) if residual else None
        return (x.permute(0, 2, 3, 1).contiguous().to(device), w.permute(0, 2, 3, 1).contiguous().to(device), scale.to(device), bias.to(device),
                res, OH, OW)

    def line(name, case, variant, y):
        torch.cuda.synchronize()
        a = y.contiguous().cpu().view(torch.uint8).numpy()
        print("%s %s variant=%d %s%s %s" % (name, "x".join(map(str, case)), variant, str(y.dtype).replace("torch.", ""), list(y.shape),
                                            hashlib.sha256(a.tobytes()).hexdigest()))

    st = torch.cuda.current_stream().cuda_stream
    for sk in (False, True):
        ws = ops.p8_sk_workspace(device) if sk else None
        for case in (SK_CASES if sk else P8_CASES):
            B, H, W, Cin, Cout, k, s, p = case
            x, w, sc, bi, res, OH, OW = inputs(case, True)
            for variant in (SK_VARIANTS if sk else P8_VARIANTS):
                y = torch.full((B, OH, OW, Cout), float("nan"), device=device)
                args = (x.data_ptr(), w.data_ptr(), sc.data_ptr(), bi.data_ptr(), res.data_ptr(), y.data_ptr(), B, H, W, Cin, Cout, k, k, s, p, Cin,
                        Cout, Cout, ops.ACT_RELU, 0, variant)
                rc = L.nopesac_conv2d_nhwc_p8_sk(*args, ws.data_ptr(), ws.numel(), st) if sk else L.nopesac_conv2d_nhwc_p8(*args, st)
                assert rc == 0
                line("p8_stream_k" if sk else "p8", case, variant, y)
    for case in P8N_CASES:
        B, H, W, Cin, Cout, k, s, p = case
        x, w, sc, bi, _, OH, OW = inputs(case, False)
        for variant in P8N_VARIANTS:
            if variant >> 8 and B * H * W * Cin * Cout * k * k > 3e10:       # (the test skips one workgroup on the long-K case)
                continue
            for act in ACTS:
                y = torch.full((B, OH, OW, Cout), float("nan"), device=device, dtype=torch.bfloat16)
                rc = L.nopesac_conv2d_nhwc_p8n(x.data_ptr(), w.data_ptr(), sc.data_ptr(), bi.data_ptr(), y.data_ptr(), B, H, W, Cin, Cout, k, k, s, p,
                                               Cin, Cout, getattr(ops, act), variant, st)
                assert rc == 0
                line("p8n/" + act, case, variant, y)
    for case in SPLIT_CASES:
        B, H, W, Cin, Cout, k, s, p, splits, cap = case
        x, w, sc, bi, _, OH, OW = inputs(case, False)
        ws = torch.full((splits * B * OH * OW * Cout,), float("nan"), device=device)
        for act in ACTS:
            wide = torch.full((B, OH, OW, Cout + 16), float("nan"), device=device, dtype=torch.bfloat16)
            y = wide[..., 8:8 + Cout]
            rc = L.nopesac_conv2d_nhwc_p8n_splitk(x.data_ptr(), w.data_ptr(), sc.data_ptr(), bi.data_ptr(), y.data_ptr(), B, H, W, Cin, Cout, k, k, s, p,
                                                  Cin, Cout + 16, getattr(ops, act), 32 | (cap << 8), splits, ws.data_ptr(), ws.numel() * 4, st)
            assert rc == 0
            line("p8n_split_k/" + act, case, 32 | (cap << 8), wide)


if __name__ == "__main__":
    main()
