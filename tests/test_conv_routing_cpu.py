"""CPU half of the conv routing sweep: every key of the committed routing files parses back into its call, ops.conv_eligibility
reproduces the key's shape flags and the routed configuration is a candidate there, conv2d hands the tuner the same key and the same
candidates as before eligibility became a function, the row sampler covers the edges, and the comparators of tests/conv_routing.py fail
on planted kernel faults (negative controls: a CPU F.conv2d of the same operands plays the kernel)."""
import random

import pytest
import torch
import torch.nn.functional as F

from tests import conv_routing as CR

KEYS = CR.load_routing()
KEY_LIST = sorted(KEYS)


class _Stop(Exception):
    pass


def _legacy_eligibility(x_dtype, w_dtype, out_dtype, B, H, W, Cin, Cout, KH, KW, stride, pad, has_residual, x_cs, y_cs, r_cs, batched,
                        has_scale, has_bias, act, aligned):
    """The eligibility block conv2d held inline before ops.conv_eligibility (verbatim but for tensors -> flags), and its candidate tuple."""
    from nopesac_amd import ops
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    bfrag_ok = (x_dtype == torch.bfloat16 and w_dtype == torch.bfloat16 and not batched and Cin % 64 == 0 and Cout % 128 == 0
                and x_cs % 8 == 0 and KH * KW <= 32 and (act & ~(0xff | ops.ACT_RES_AFTER)) == 0
                and (B * H * W + pad * W + pad) * x_cs * 2 < 2 ** 31)
    halo_ok = (bfrag_ok and KH == 3 and KW == 3 and stride == 1 and pad == 1 and not has_residual and x_cs == Cin and y_cs == Cout
               and out_dtype == torch.bfloat16 and has_scale and has_bias and (act & ~0xff) == 0)
    p8_ok = (x_dtype == torch.bfloat16 and w_dtype == torch.bfloat16 and not batched and Cin % 64 == 0 and Cout % 256 == 0
             and x_cs % 8 == 0 and KH * KW <= 32 and (act & ~(0xff | ops.ACT_RES_AFTER)) == 0
             and (B * H * W + pad * W + pad) * x_cs * 2 < 2 ** 31 and B * H * W < 2 ** 23 and x_cs < 2 ** 24 and KH * KW * Cin < 2 ** 24
             and Cout * KH * KW * Cin * 2 < 2 ** 31 and out_dtype in ops._DT and x_cs % 8 == 0
             and (y_cs % (4 if out_dtype == torch.float32 else 8) == 0)
             and (not has_residual or (r_cs % (4 if out_dtype == torch.float32 else 8) == 0 and out_dtype != torch.float8_e4m3fn))
             and aligned)
    p8_sk_ok = p8_ok and (-(-(B * OH * OW) // 256)) * (Cout // 256) <= 1024 and KH * KW * Cin >= 512
    p8n_ok = (x_dtype == torch.bfloat16 and w_dtype == torch.bfloat16 and out_dtype == torch.bfloat16 and not batched and not has_residual
              and Cin % 64 == 0 and Cout % 128 == 0 and x_cs % 8 == 0 and y_cs % 8 == 0 and KH * KW <= 32
              and act in (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_LEAKY)
              and (B * H * W + pad * W + pad) * x_cs * 2 < 2 ** 31 and B * H * W < 2 ** 23 and x_cs < 2 ** 24 and KH * KW * Cin < 2 ** 24
              and Cout * KH * KW * Cin * 2 < 2 ** 31 and (B * OH * OW + 256) * y_cs * 2 < 2 ** 31
              and aligned)
    p8n_tiles = (-(-(B * OH * OW) // 256)) * (Cout // 128) if Cout % 128 == 0 else 0
    p8n_splits = min(8, Cin // 64, 256 // p8n_tiles) if p8n_tiles else 0
    p8n_split_ok = p8n_ok and KH * KW * Cin >= 4096 and p8n_splits >= 2 and p8n_splits * B * OH * OW * Cout * 4 < 2 ** 31
    extra = (((ops.CFG_BFRAG3, ops.CFG_BFRAG32) if bfrag_ok else ()) + ((ops.CFG_HALO16, ops.CFG_HALO8) if halo_ok else ())
             + ((ops.CFG_P8,) if p8_ok else ()) + ((ops.CFG_P8_SK,) if (p8_sk_ok and ops.P8_SK_TUNABLE[0]) else ())
             + (((ops.CFG_P8N,) + ((ops.CFG_P8N_TAP,) if KH * KW > 1 else ())) if (p8n_ok and ops.P8N_TUNABLE[0]) else ())
             + ((ops.CFG_P8N_SPLIT,) if (p8n_split_ok and ops.P8N_TUNABLE[0]) else ()))
    return (bfrag_ok, halo_ok, p8_ok, p8_sk_ok, p8n_ok, p8n_splits, p8n_split_ok), extra


def _args(c, aligned=True):
    return (c.x_dtype, c.w_dtype, c.out_dtype, c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad, c.residual, c.x_cs, c.y_cs,
            c.Cout if c.residual else 0, c.batched, c.scale, c.bias, c.act, aligned)


# ---------------------------------------------------------------------------------------------------------------------------- keys

def test_the_three_routing_files_hold_54_distinct_keys():
    assert len(KEYS) == 54
    assert len({CR.key_id(k) for k in KEYS}) == 54          # readable ids of the GPU sweep are unique


@pytest.mark.parametrize("key", KEY_LIST, ids=[CR.key_id(k) for k in KEY_LIST])
def test_key_parses_reproduces_its_flags_and_routes_to_a_candidate(key, monkeypatch):
    from nopesac_amd import ops
    c = CR.parse_key(key)
    assert ops.TUNER.key_str(CR.key_tuple(c)) == key
    el = CR.eligibility(c)
    assert (el.bfrag_ok, el.halo_ok, el.p8_ok) == (c.bfrag_ok, c.halo_ok, c.p8_ok)
    for sk in (False, True):
        monkeypatch.setattr(ops, "P8_SK_TUNABLE", [sk])
        legacy, extra = _legacy_eligibility(*_args(c))
        assert tuple(el) == legacy
        assert ops.conv_tuner_extras(el, c.KH, c.KW) == extra
    monkeypatch.setattr(ops, "P8_SK_TUNABLE", [False])         # the benchmark's switches
    cands = ops.ConvTuner.CANDIDATES + ops.conv_tuner_extras(el, c.KH, c.KW)
    for name, cfg in KEYS[key].items():
        assert cfg in cands, (name, cfg, cands)


@pytest.mark.parametrize("key", KEY_LIST, ids=[CR.key_id(k) for k in KEY_LIST])
def test_conv2d_hands_the_tuner_the_routing_key_and_candidates(key, monkeypatch):
    """ops.conv2d on (unbacked) CPU tensors of the key's shape, stopped inside ConvTuner.choose: the key it builds is the routing key
    byte for byte, the candidates are the pre-refactor tuple in the pre-refactor order."""
    from nopesac_amd import ops
    c = CR.parse_key(key)
    OH, OW = (c.H + 2 * c.pad - c.KH) // c.stride + 1, (c.W + 2 * c.pad - c.KW) // c.stride + 1
    x = torch.empty(c.B, c.H, c.W, c.x_cs, dtype=c.x_dtype)[..., :c.Cin]
    w = torch.empty(((c.B,) if c.batched else ()) + (c.Cout, c.KH, c.KW, c.Cin), dtype=c.w_dtype)
    out = torch.empty(c.B, OH, OW, c.y_cs, dtype=c.out_dtype)[..., :c.Cout]
    res = torch.empty(c.B, OH, OW, c.Cout, dtype=c.out_dtype) if c.residual else None
    sc = torch.empty(c.Cout) if c.scale else None
    bi = torch.empty(c.Cout) if c.bias else None
    seen = []

    def choose(k, launch, extra=()):
        seen.append((k, extra))
        raise _Stop

    monkeypatch.setattr(ops, "_chk", lambda t, dtype=None, contiguous=True: t)      # (the device check: these tensors never launch)
    monkeypatch.setattr(ops.TUNER, "measuring", True)
    monkeypatch.setattr(ops.TUNER, "choose", choose)
    with pytest.raises(_Stop):
        ops.conv2d(x, w, sc, bi, res, stride=c.stride, pad=c.pad, act=c.act, out=out, batched_weights=c.batched)
    (k, extra), = seen
    assert ops.TUNER.key_str(k) == key
    assert extra == _legacy_eligibility(*_args(c))[1]


def _random_calls():
    """3000 argument tuples: random shapes, dtypes, strides, epilogue words and alignment around the kernels' limits.  The lists hold
    B * H * W on both sides of 2 ** 23 and of 2 ** 24 (B 2 / 3 x H 480 x W 19200, B 64 x H 240 x W 640), M over 2 ** 23, and few
    256 x 128 tiles under a long K (B 1 - 4, H 1 / 15, W 20 / 80, Cin 2048: 256 // tiles over the cap of 8); repeated values weight the
    sample towards calls some kernel is eligible for."""
    rnd = random.Random(5)
    bf16 = (torch.bfloat16, torch.bfloat16)
    dts = [bf16, (torch.float32, torch.bfloat16), (torch.float32, torch.float32), bf16, bf16]
    outs = [torch.bfloat16, torch.float32, torch.float8_e4m3fn, torch.bfloat16]
    acts = [0, 1, 2, 3, 0x101, 0x102, 0x200, 0x201, 0, 1]
    for _ in range(3000):
        xd, wd = rnd.choice(dts)
        Cin, Cout = rnd.choice([3, 64, 128, 320, 2048, 256, 2048]), rnd.choice([4, 128, 256, 300, 512, 128])
        k = rnd.choice([1, 3, 7, 3])
        yield (xd, wd, rnd.choice(outs), rnd.choice([1, 2, 3, 4, 64, 700, 2]), rnd.choice([1, 15, 60, 240, 480, 15]),
               rnd.choice([20, 80, 640, 19200, 20]), Cin, Cout, k, k, rnd.choice([1, 2, 1]), rnd.choice([0, k // 2]), rnd.random() < 0.3,
               Cin + rnd.choice([0, 0, 4, 8, 0, 0]), Cout + rnd.choice([0, 0, 4, 8, 0, 0]), rnd.choice([Cout, Cout + 4]), rnd.random() < 0.1,
               rnd.random() < 0.7, rnd.random() < 0.7, rnd.choice(acts), rnd.random() < 0.9)


def test_conv_eligibility_matches_the_inline_block_off_the_routed_shapes():
    """Random shapes, dtypes, strides, epilogue words and alignment around the kernels' limits."""
    from nopesac_amd import ops
    for args in _random_calls():
        legacy, extra = _legacy_eligibility(*args)
        el = ops.conv_eligibility(*args)
        assert tuple(el) == legacy, args
        assert ops.conv_tuner_extras(el, args[8], args[9]) == extra


def test_the_random_sample_takes_every_flag_both_ways():
    """The legacy function alone over the sample: every flag is True for some calls and False for others, the slice count runs from
    below 2 up to the cap of 8, and each limit the C entry points and the old Python mirror stated differently is hit from both sides
    (a flag that is constant over the sample would test nothing)."""
    from nopesac_amd import ops
    flags = {n: [0, 0] for n in ops.ConvEligibility._fields if n != "p8n_splits"}
    splits, mid, big_m, capped = set(), 0, 0, 0
    for args in _random_calls():
        el = ops.ConvEligibility(*_legacy_eligibility(*args)[0])
        for n in flags:
            flags[n][bool(getattr(el, n))] += 1
        splits.add(el.p8n_splits)
        B, H, W, Cin, Cout, k, _, stride, pad = args[3:12]
        M = B * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
        mid += 2 ** 23 <= B * H * W < 2 ** 24
        big_m += M >= 2 ** 23
        tiles = -(-M // 256) * (Cout // 128) if Cout % 128 == 0 else 0
        capped += tiles > 0 and min(Cin // 64, 256 // tiles) > 8
    print("random sample, legacy flags [False, True]: %s; B*H*W in [2**23, 2**24): %d, M >= 2**23: %d, slice count capped at 8: %d"
          % (flags, mid, big_m, capped))
    assert all(f and t for f, t in flags.values()), flags
    assert {0, 1, 2, 8} <= splits and max(splits) == 8
    assert mid and big_m and capped


def test_config_ids_match_the_header_and_the_launchers_share_one_predicate():
    """NPS_CONV_CFG_* of the header are ops.CFG_* and, with NPS_CONV_T128 .. DMA32, the keys of CONV_CFG_KERNEL; every launcher source
    checks its arguments through csrc/conv_forms.h and holds no dims / 2 GB / 24-bit check of its own."""
    import os
    import re
    from nopesac_amd import _lib, ops
    text = open(_lib.HEADER_PATH).read()
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NPS_CONV_CFG_(\w+) (\d+)", text)}
    assert ids and ids == {n[4:]: v for n, v in vars(ops).items() if n.startswith("CFG_")}
    base = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NPS_CONV_(AUTO|T128|T64|DMA64|DMA32) (\d+)", text)}
    assert sorted(base.values()) == list(ops.ConvTuner.CANDIDATES)
    assert set(ids.values()) | set(base.values()) - {0} == set(ops.CONV_CFG_KERNEL)
    csrc = os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "nopesac_amd", "csrc")
    forms = open(os.path.join(csrc, "conv_forms.h")).read()
    for name, calls in (("conv_igemm.hip", ["conv_bfrag_refusal(c)"]), ("conv_p8.hip", ["conv_p8_refusal(c)", "conv_p8_sk_refusal(c)"]),
                        ("conv_p8n.hip", ["conv_p8n_refusal(c)", "conv_p8n_split_refusal(c, splits)"]),
                        ("conv3x3_halo.hip", ["conv_halo_refusal(c)"])):
        src = open(os.path.join(csrc, name)).read()
        launcher = src[src.index("static int bfrag_launch("):] if name == "conv_igemm.hip" else src      # (nopesac_conv2d_nhwc_ex: not routed by a mask)
        assert '#include "conv_forms.h"' in src and "conv_call_refusal(c)" in launcher, name
        for call in calls:
            assert call in launcher and "inline const char* %s(" % call.split("(")[0] in forms, (name, call)
        checks = " ".join(re.findall(r"NPS_CHECK_ARG\(.*?\);", launcher, flags=re.S))          # the argument checks the launcher keeps
        for own in ("B > 0", "KH * KW <= 32", "Cin % 64", "Cout % 128", "Cout % 256", "1 << 23", "1 << 24", "2 GB", "x_cstride >= Cin"):
            assert own not in checks, (name, own)


@pytest.mark.parametrize("key, want, extra", [
    # the pose net's first conv (layer_3): 75 tiles of 256 x 128 -> 3 split-K slices; routed to 15 by hand
    ("bfloat16|bfloat16|bfloat16|64|15|20|2048|128|3|3|1|1|False|2048|128|False|False|False|0|True|False|False",
     (True, False, False, False, True, 3, True), (7, 8, 13, 14, 15)),
    # the 19200-row 256 -> 1536 GEMM: 450 tiles (no split-K), K = 256 too short for stream-K
    ("bfloat16|bfloat16|bfloat16|1|1|19200|256|1536|1|1|1|0|False|256|1536|False|False|True|0|True|False|True",
     (True, False, True, False, True, 0, False), (7, 8, 11, 13)),
    # res3's stride-2 1x1 projection at 64 x 60 x 80
    ("bfloat16|bfloat16|bfloat16|64|60|80|512|1024|1|1|2|0|False|512|1024|False|True|True|0|True|False|True",
     (True, False, True, False, True, 0, False), (7, 8, 11, 13)),
    # 3x3 with scale + bias + leaky: the halo kernels too, and stream-K (75 tiles, K = 2304)
    ("bfloat16|bfloat16|bfloat16|64|15|20|256|256|3|3|1|1|False|256|256|False|True|True|2|True|True|True",
     (True, True, True, True, True, 1, False), (7, 8, 9, 10, 11, 12, 13, 14)),
    # bf16 -> fp8 e4m3: bfrag and p8 only (p8n writes bf16)
    ("bfloat16|bfloat16|float8_e4m3fn|64|15|20|2048|512|1|1|1|0|False|2048|512|False|True|True|1|True|False|True",
     (True, False, True, True, False, 0, False), (7, 8, 11, 12)),
    # f32 activations x bf16 weights, residual after the ReLU: the conv_igemm family only
    ("float32|bfloat16|bfloat16|64|15|20|256|256|1|1|1|0|True|256|256|False|True|True|257|False|False|False",
     (False, False, False, False, False, 1, False), ()),
])
def test_pinned_keys(key, want, extra, monkeypatch):
    from nopesac_amd import ops
    monkeypatch.setattr(ops, "P8_SK_TUNABLE", [True])
    monkeypatch.setattr(ops, "P8N_TUNABLE", [True])
    c = CR.parse_key(key)
    el = CR.eligibility(c)
    assert tuple(el) == want
    assert ops.conv_tuner_extras(el, c.KH, c.KW) == extra


# ---------------------------------------------------------------------------------------------------------------------------- sampler

@pytest.mark.parametrize("B, OH, OW", [(64, 15, 20), (64, 60, 80), (1, 1, 19200), (32, 1, 50), (1, 1, 32), (2, 3, 5)])
def test_sample_rows_covers_the_edges(B, OH, OW):
    M = B * OH * OW
    rows = CR.sample_rows(M, B, OH, OW, seed=3)
    s = set(rows.tolist())
    assert rows.dtype == torch.long and torch.equal(rows, rows.unique()) and int(rows.min()) >= 0 and int(rows.max()) < M
    assert 0 in s and M - 1 in s
    assert len(rows) == min(M, 1536) or len(rows) >= 1536
    assert set(range(min(64, M))) <= s and set(range(max(0, M - 64), M)) <= s
    for t in CR.TILE_HEIGHTS:
        for j in (1, (M - 1) // t):
            if 1 <= j and j * t + 1 < M:
                assert {j * t - 2, j * t - 1, j * t, j * t + 1} <= s, (t, j)
    P = OH * OW
    for b in (0, B - 1):
        for oh, ow in ((0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1), (0, OW // 2), (OH // 2, 0)):
            assert b * P + oh * OW + ow in s
    assert torch.equal(rows, CR.sample_rows(M, B, OH, OW, seed=3))


# ---------------------------------------------------------------------------------------------------------------------------- controls

# scaled-down versions of routed keys: 3x3 pad 1 bf16 (+ scale, bias, ReLU), res4's 1x1 stride-2 projection, layer_3's 3x3 Cin = 2048
# (the split-K shape: no scale / bias), the bf16 -> fp8 GEMM, and the f32 x bf16 conv with the residual after the ReLU (act 257)
CONTROL_KEYS = {
    "3x3_bf16": "bfloat16|bfloat16|bfloat16|2|30|40|256|256|3|3|1|1|False|256|256|False|True|True|1|True|True|True",
    "1x1_stride2": "bfloat16|bfloat16|bfloat16|2|30|40|256|256|1|1|2|0|False|256|256|False|True|True|0|True|False|True",
    "3x3_cin2048": "bfloat16|bfloat16|bfloat16|1|15|20|2048|128|3|3|1|1|False|2048|128|False|False|False|0|True|False|False",
    "fp8_out": "bfloat16|bfloat16|float8_e4m3fn|2|15|20|512|256|1|1|1|0|False|512|256|False|True|True|1|True|False|True",
    "res_after": "float32|bfloat16|bfloat16|2|15|20|256|256|1|1|1|0|True|256|256|False|True|True|257|False|False|False",
}
FAULTS = {
    "drop_k_tile": ["3x3_bf16", "1x1_stride2", "3x3_cin2048", "fp8_out", "res_after"],
    "shift_row_tile": ["3x3_bf16", "1x1_stride2", "3x3_cin2048", "fp8_out", "res_after"],
    "tail_row_unwritten": ["3x3_bf16", "1x1_stride2", "3x3_cin2048", "fp8_out", "res_after"],
    "pad_tap_from_previous_row": ["3x3_bf16", "3x3_cin2048"],
    "bias_first_128_channels": ["3x3_bf16", "1x1_stride2", "fp8_out", "res_after"],
    "residual_before_act": ["res_after"],
}
MARGIN = 4.0        # every planted fault must exceed the tolerance by at least this factor
_CACHE = {}


def _control(name):
    """(call, sampled rows, r, A) of a control case, built once."""
    if name not in _CACHE:
        key = CONTROL_KEYS[name]
        c = CR.parse_key(key)
        call = CR.build_call(c, torch.device("cpu"), CR.key_seed(key))
        rows = CR.sample_rows(call.M, c.B, call.OH, call.OW, CR.key_seed(key))
        _CACHE[name] = (call, rows) + CR.reference_rows(call, rows)
    return _CACHE[name]


def _emulate(call, fault=None):
    """A CPU 'kernel' of the call: float32 F.conv2d of the operands the kernel reads, its epilogue in float32, rounded to the output
    dtype - with one planted fault."""
    from nopesac_amd import ops
    c = call.case
    x = call.x.float()
    if c.x_dtype == torch.float32 and c.w_dtype == torch.bfloat16:
        x = x.to(torch.bfloat16).float()                 # the A-tile load of conv_igemm rounds f32 activations to bf16
    w = call.w.float().clone()
    bias = call.bias.clone() if call.bias is not None else None
    xn = x.permute(0, 3, 1, 2)
    pad = c.pad
    if fault == "drop_k_tile":                           # one 64-channel K-tile (centre tap) missing from the last 128-channel column tile
        n0, c0, kh, kw = c.Cout - 128, 64 if c.Cin >= 128 else 0, c.KH // 2, c.KW // 2
        w[n0:n0 + 128, kh, kw, c0:c0 + 64] = 0
    if fault == "pad_tap_from_previous_row":             # the left padding column reads the previous row's last pixel (address - 1 pixel)
        xp = F.pad(xn, (pad, pad, pad, pad))
        xp[:, :, pad + 1:pad + c.H, 0] = xn[:, :, 0:c.H - 1, c.W - 1]
        xn, pad = xp, 0
    if fault == "bias_first_128_channels":
        bias[128:] = 0
    acc = F.conv2d(xn, w.permute(0, 3, 1, 2), stride=c.stride, padding=pad).permute(0, 2, 3, 1)
    v = acc * call.scale if call.scale is not None else acc
    v = v + bias if bias is not None else v
    act, res_after = c.act & 0xff, bool(c.act & ops.ACT_RES_AFTER)
    if fault == "residual_before_act":
        res_after = not res_after
    if call.residual is not None:
        rs = call.residual.float()
        y = CR._act(v, act) + rs if res_after else CR._act(v + rs, act)
    else:
        y = CR._act(v, act)
    y = y.to(c.out_dtype).contiguous()
    flat = y.view(-1, c.Cout)
    M = flat.shape[0]
    if fault == "shift_row_tile":                        # the second 256-row tile written one row up (each row holds the next row's result)
        t0 = 256 if M >= 2 * 256 + 1 else 0
        flat[t0:t0 + 256] = flat[t0 + 1:t0 + 257].clone()
    if fault == "tail_row_unwritten":                    # the last row of the M tail never stored (a zeroed buffer: no NaN to give it away)
        flat[M - 1] = 0
    return y


def _ratios(name, fault):
    call, rows, r, A = _control(name)
    y = _emulate(call, fault)
    ref = CR.error_ratio(CR.output_rows(call, y, rows), r, A, call.case.out_dtype)[0]
    return ref, CR.full_agreement(y, _emulate(call))


@pytest.mark.parametrize("name", sorted(CONTROL_KEYS))
def test_control_without_a_fault_passes(name):
    ref, full = _ratios(name, None)
    assert ref <= 1.0 and full == 0.0, (ref, full)


@pytest.mark.parametrize("name, fault", [(n, f) for f, names in FAULTS.items() for n in names])
def test_planted_fault_fails_the_comparators(name, fault):
    ref, full = _ratios(name, fault)
    print("control %-12s %-26s reference/tolerance %.3g  full_agreement %.3g" % (name, fault, ref, full))
    assert ref >= MARGIN and full >= MARGIN, (ref, full)
