"""tests/conv_f32_forms.py without a GPU: the restated dispatch uses the source's constants, the case lists reach all six builds of the
f32 conv kernel and every edge the sweep names, the float64 references are F.conv2d and its autograd, the committed float32 figures are
what the CPU measures, the restatement of the kernel's summation stands within the limit, and every planted error fails it."""
import re

import pytest
import torch
from torch.nn import functional as F

from tests import conv_f32_forms as CF
from tests.util import ROOT

FORMS = {c.name: CF.generic_form(CF.call_of(c)) for c in CF.FORWARD_CASES}
CALLS = {c.name: CF.call_of(c) for c in CF.FORWARD_CASES}


def _src(name):
    return open(ROOT + "/nopesac_amd/csrc/" + name).read()


def test_the_constants_are_the_sources():
    common, igemm, act = _src("conv_common.h"), _src("conv_igemm.hip"), _src("common.h")
    m = re.search(r"struct Cfg<float> \{ static constexpr int BK = (\d+); static constexpr int VECW = (\d+); \};", common)
    assert m and (int(m.group(1)), int(m.group(2))) == (CF.BK, CF.VECW)
    assert [int(v) for v in re.findall(r"constexpr int FLUSH = (\d+);", igemm)] == [CF.FLUSH]
    # the flush skips the last tile, and the second accumulator is added at the end
    assert "if ((kt % FLUSH) == FLUSH - 1 && kt + 1 < nk) {" in igemm and "acc[i][j][r] += acc_hi[i][j][r];" in igemm
    cfg = igemm[igemm.index("static int launch_cfg("):igemm.index("static int launch_dtype(")]
    m = re.search(r"if constexpr \(sizeof\(T\) == 4\) \{\s*//[^\n]*\n\s*if \(vec == VW && p\.K >= (\d+)\) \{\s*hipLaunchKernelGGL\(\(conv_igemm_kernel<TA, T, BM, BN, VW, 1, true>\)", cfg)
    assert m and int(m.group(1)) == CF.TWO_LEVEL_K
    dt = igemm[igemm.index("static int launch_dtype("):igemm.index("}  // namespace nps")]
    # the vector width: Cin, K, x_cs, w_bs multiples of it, x and w aligned to its bytes
    assert "return p.Cin % v == 0 && p.K % v == 0 && p.x_cs % xm == 0 && p.w_bs % v == 0 &&" in dt
    assert "((uintptr_t)p.x % xa == 0) && ((uintptr_t)p.w % (v * sizeof(T)) == 0);" in dt
    assert "const long long tiles128 = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128) * (p.batched ? p.B : 1);" in dt
    m = re.search(r"const bool small_k_stream = p\.KH \* p\.KW == 1 && p\.K <= (\d+);", dt)
    assert m and int(m.group(1)) == CF.STREAM_K
    m = re.search(r"if \(p\.N > (\d+) && tiles128 >= (\d+) && !small_k_stream\) return launch_cfg<TA, T, 128, 128>\(p, stream, vec\);\s*"
                  r"return launch_cfg<TA, T, 64, 64>\(p, stream, vec\);", dt)
    assert m and (int(m.group(1)), int(m.group(2))) == (CF.SMALL_N, CF.AUTO_TILES)
    assert "if (p.force == 1) return launch_cfg<TA, T, 128, 128>(p, stream, vec);" in dt and "if (p.force == 2) return launch_cfg<TA, T, 64, 64>(p, stream, vec);" in dt
    assert 'if (!strcmp(e, "t128")) { p.force = 1; p.use_glds = 0; }' in igemm and 'else if (!strcmp(e, "t64")) { p.force = 2; p.use_glds = 0; }' in igemm
    m = re.search(r"const int q = nwg / (\d+), r = nwg % (\d+), xcd = bid % (\d+), within = bid / (\d+);", igemm)
    assert m and {int(v) for v in m.groups()} == {CF.XCDS}
    assert "act == NPS_ACT_LEAKY ? 0.01f * v : v" in act and abs(CF.LEAKY_SLOPE - 0.01) < 1e-9 and CF.LEAKY_SLOPE != 0.01
    # the dgrad's inner call: Cin and Cout swapped, pad = KH - 1 - pad, the library's own choice of build
    bwd = _src("conv_bwd.hip")
    assert ("return nopesac_conv2d_nhwc_ex(dy, w_ws, nullptr, nullptr, nullptr, dx, B, H, W, Cout, Cin, KH, KW, 1, KH - 1 - pad, dy_cstride, "
            "dx_cstride,") in bwd and "NPS_ACT_NONE, NPS_DT_F32, NPS_DT_F32, NPS_CONV_AUTO, stream);" in bwd


def test_the_xcd_remap_is_a_permutation():
    for nwg in (1, 7, 8, 9, 17, 192):
        assert sorted(CF.xcd_remap(b, nwg) for b in range(nwg)) == list(range(nwg))


def test_generic_form_by_hand():
    call = CF.Call(1, 70, 24, 512, 512, 1, 512, 0, 0, 0, False, "t64")
    assert CF.generic_form(call) == (64, 4, True)
    assert CF.generic_form(call._replace(K=508, Cin=508, x_cs=508)) == (64, 4, False)
    assert CF.generic_form(call._replace(x_align=4)) == (64, 1, False) and CF.generic_form(call._replace(x_cs=513, force="t128")) == (128, 1, False)
    assert CF.generic_form(call._replace(w_align=8)) == (64, 1, False) and CF.generic_form(call._replace(w_bs=6)) == (64, 1, False)
    auto = CF.Call(1, 12288, 256, 36, 4, 9, 4, 0, 0, 0, False, None)
    assert CF.generic_form(auto) == (128, 4, False)
    assert CF.generic_form(auto._replace(M=12160)) == (64, 4, False)                   # 190 tiles
    assert CF.generic_form(auto._replace(N=64, M=64 * 12288)) == (64, 4, False)        # N <= 64
    assert CF.generic_form(auto._replace(taps=1, K=256, Cin=256, x_cs=256)) == (64, 4, False)      # the HBM-bound 1x1
    assert CF.generic_form(auto._replace(taps=1, K=260, Cin=260, x_cs=260)) == (128, 4, False)
    assert CF.generic_form(auto._replace(M=128, B=96, batched=True, w_bs=256 * 36)) == (128, 4, False)    # grid.y counts


def test_the_forward_cases_reach_every_build_and_edge():
    cases = CF.FORWARD_CASES
    assert len({c.name for c in cases}) == len(cases)
    assert set(FORMS.values()) == {(bm, vec, two) for bm in (64, 128) for vec, two in ((4, False), (4, True), (1, False))}
    by = lambda pred: [c for c in cases if pred(c)]
    # VEC 1 each way
    v1 = by(lambda c: FORMS[c.name][1] == 1)
    assert any((c.Cin, c.k, c.s, c.p) == (3, 7, 2, 3) for c in v1) and any((c.Cin, c.k) == (5, 3) for c in v1)
    assert any(c.Cin % 4 == 0 and CALLS[c.name].x_cs % 4 == 0 and CALLS[c.name].x_align == 4 for c in v1)
    assert any(c.Cin % 4 == 0 and CALLS[c.name].x_cs % 4 != 0 and CALLS[c.name].x_align == 0 for c in v1)
    assert {27, 147} <= {CALLS[c.name].K for c in v1}
    # K tails at VEC 4; a K below one tile
    v4 = by(lambda c: FORMS[c.name][1] == 4)
    assert {0, 4, 12} <= {CALLS[c.name].K % CF.BK for c in v4} and any(CALLS[c.name].K < CF.BK for c in v4)
    # flush boundaries of the two-level build, for each tile size at least the first and the last; the long chain
    nk = lambda c: -(-CALLS[c.name].K // CF.BK)
    two = by(lambda c: FORMS[c.name][2])
    assert {32, 33, 39, 40, 41, 288} <= {nk(c) for c in two if FORMS[c.name][0] == 64} and {32, 41, 288} <= {nk(c) for c in two if FORMS[c.name][0] == 128}
    assert {512, 516, 624, 640, 644, 4608} <= {CALLS[c.name].K for c in two}
    assert any(c.k == 3 for c in two) and any(c.batched for c in two) and any(c.linear for c in two)
    # VEC 1 gives up two-level: a long K on one chain
    assert any(CALLS[c.name].K >= CF.TWO_LEVEL_K and FORMS[c.name] == (bm, 1, False) for c in cases for bm in (64,))
    assert {644, 4608} <= {CALLS[c.name].K for c in v1}
    for bm in (64, 128):
        mine = by(lambda c: FORMS[c.name][0] == bm)
        assert {1, bm - 1, 0} <= {CALLS[c.name].M % bm for c in mine} and any(CALLS[c.name].M < bm for c in mine)
        # a tile across two images under general addressing
        assert any(c.B >= 2 and not c.batched and (c.k > 1 or c.s > 1) and (CF.out_hw(c)[0] * CF.out_hw(c)[1]) % bm != 0
                   and CF.out_hw(c)[0] * CF.out_hw(c)[1] < bm < CALLS[c.name].M for c in mine)
        assert {1, 9} <= {CF.tile_count(CALLS[c.name], FORMS[c.name]) for c in mine}
        assert any(c.Cout > bm for c in mine)                                           # more than one tile column
        assert {True, False} == {CF.epilogue_vector(c) for c in mine}
        assert {(a, r) for a in CF.ACTS for r in ("none", "before", "after")} == {
            (c.act, "none" if c.rp is None else ("after" if c.res_after else "before")) for c in mine if c.name.startswith("epi_")}
    assert {1, 7, 8, 9, 17} <= {CF.tile_count(CALLS[c.name], FORMS[c.name]) for c in cases if FORMS[c.name][0] == 64}
    assert {1, 3, 31, 33, 64, 65, 300} <= {c.Cout for c in cases}
    assert any(c.Cout == 300 and c.yp == (0, 4) for c in cases) and any(c.Cout == 300 and c.rp is not None and sum(c.rp) > 0 for c in cases)
    # addressing
    dense = lambda c: (c.k, c.s, c.p) == (1, 1, 0)
    assert any(dense(c) for c in cases) and {(1, 2), (3, 1), (3, 2), (7, 2)} <= {(c.k, c.s) for c in cases if not dense(c)}
    assert any(c.k == 3 and c.H == 1 for c in cases) and any(c.k == 3 and c.W == 1 for c in cases) and any(c.k == 3 and c.p == 0 for c in cases)
    # the epilogue: scale x bias, both paths; misaligned y, misaligned residual, Cout % 4
    epi = by(lambda c: c.name.startswith("epi_"))
    for vec in (True, False):
        assert {(s, b) for s in (True, False) for b in (True, False)} == {(c.scale, c.bias) for c in epi if CF.epilogue_vector(c) == vec}
    assert any(c.Cout % 4 == 0 and c.yp[0] % 4 != 0 for c in cases) and any(c.Cout % 4 == 0 and c.rp and c.rp[0] % 4 != 0 for c in cases)
    assert any(c.Cout % 4 != 0 and not CF.epilogue_vector(c) for c in cases)
    # batched weights
    bat = by(lambda c: c.batched)
    assert all(CALLS[c.name].w_bs == c.Cout * CALLS[c.name].K and CALLS[c.name].M == CF.out_hw(c)[0] * CF.out_hw(c)[1] for c in bat)
    assert any(c.B > 1 and c.bbias for c in bat) and any(c.B > 1 and c.bias and not c.bbias for c in bat) and any(not c.bias for c in bat)
    assert any(c.B == 1 and c.bias for c in bat) and any(c.k == 3 for c in bat) and any(c.bbias and c.Cout % 4 != 0 for c in bat)
    assert any(CF.tile_count(CALLS[c.name], FORMS[c.name]) > 1 for c in bat)
    assert all(c.bias for c in cases if c.bbias) and all(c.batched for c in cases if c.bbias)
    # ops.linear: slices of x, out and residual
    lin = by(lambda c: c.linear)
    assert all((c.B, c.H, c.k) == (1, 1, 1) for c in lin) and any(sum(c.xp) and sum(c.yp) and c.rp and sum(c.rp) for c in lin)
    # the host's own choice, once per tile size
    auto = {FORMS[c.name][0]: c for c in cases if c.force is None}
    assert set(auto) == {64, 128} and CALLS[auto[128].name].M == 12288 and auto[128].Cout == 256 and auto[128].name in CF.DEVICE_REFERENCE
    assert -(-CALLS[auto[128].name].M // 128) * -(-auto[128].Cout // 128) == CF.AUTO_TILES


def test_the_dgrad_cases():
    cases = CF.DGRAD_CASES
    assert len(set(cases)) == len(cases)
    base = {c[:6] for c in cases if c[-1] == "base"}
    assert base == {(k, b, h, w, ci, co) for k in (1, 3) for h, w in ((1, 1), (2, 3), (5, 9), (7, 10)) for b in (1, 2)
                    for ci, co in ((4, 4), (12, 8), (64, 132), (132, 64), (5, 7))}
    forms = {c: CF.generic_form(CF.dgrad_call(c)) for c in cases + CF.PRODUCTION_CASES}
    assert all(forms[c][1] == 1 for c in cases if c[4:6] == (5, 7)) and all(forms[c] == (64, 4, True) for c in base_keys(cases, 3, 64))
    assert CF.dgrad_call((3, 1, 5, 9, 132, 64, "base")).K == 576
    assert {"dy_slice", "dy_off1", "dx304"} <= {c[-1] for c in cases}
    assert all(forms[c][1] == 1 for c in cases if c[-1] == "dy_off1") and all(forms[c][1] == 4 for c in cases if c[-1] == "dy_slice")
    assert any(c[4] == 300 and c[-1] == "dx304" for c in cases) and CF.DX_PAD["dx304"] == (0, 4) and CF.FILL == 7.0
    assert {(c[0], c[4], c[5], c[-1]) for c in CF.PRODUCTION_CASES} == {(3, 256, 256, "base"), (3, 300, 128, "dx304"), (1, 1024, 128, "base")}
    assert all(c[1] == 1 for c in CF.PRODUCTION_CASES) and max(CF.dgrad_call(c).K for c in CF.PRODUCTION_CASES) == 2304
    assert all(c in cases for c in CF.IDENTITY_CASES)
    assert {s[0] for s in CF.ROTATION_SHAPES} == {1, 3} and CF.ROTATION_PIXELS[0] == (2, 3)
    for k, H, W, _, _ in CF.ROTATION_SHAPES:
        assert 1 <= CF.ROTATION_PIXELS[0][0] < H - 1 and 1 <= CF.ROTATION_PIXELS[0][1] < W - 1
        assert set(CF.ROTATION_PIXELS[1:]) == {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}


def base_keys(cases, k, cout):
    return [c for c in cases if c[0] == k and c[5] == cout and c[-1] in ("base", "dy_slice")]


def _close(a, b):
    return float((a - b).abs().max()) <= 1e-13 * max(float(b.abs().max()), 1.0)


@pytest.mark.parametrize("name", [c.name for c in CF.FORWARD_CASES if c.name not in CF.DEVICE_REFERENCE], ids=str)
def test_the_forward_reference_and_the_restatement(name):
    """F.conv2d equals the tap-by-tap statement; the allowance is positive wherever the result is not exactly zero; the float32
    restatement of the kernel's summation stands within the limit and writes every element"""
    c, t32 = CF.FORWARD[name], CF.forward_inputs(name)
    t = {k: None if v is None else v.double() for k, v in t32.items()}
    ref, A = CF.forward_reference(name)
    assert tuple(ref.shape) == (c.B,) + CF.out_hw(c) + (c.Cout,)
    assert _close(CF.forward_eval(c, t, CF.conv_taps), ref)
    assert _close(CF.forward_magnitudes(c, t, CF.conv_taps, ref), CF.forward_magnitudes(c, t, CF.conv_torch, ref))
    assert bool((A > 0).all()) or bool((ref[A == 0] == 0).all())
    got = CF.emulate_forward(name)
    assert got.dtype == torch.float32 and not bool(torch.isnan(got).any())
    assert CF.forward_worst(name, got)[0] <= CF.limit(CF.family(c))


def test_the_reference_by_hand():
    """one output element of a strided, padded, batched case summed in a Python loop"""
    c = CF.FORWARD["bat_k3"]
    t = {k: v.double() for k, v in CF.forward_inputs(c.name).items() if v is not None}
    ref = CF.forward_reference(c.name)[0]
    for b, oh, ow, n in ((0, 0, 0, 0), (1, 4, 8, 11), (1, 2, 3, 5)):
        s = 0.0
        for kh in range(3):
            for kw in range(3):
                ih, iw = oh + kh - 1, ow + kw - 1
                if 0 <= ih < c.H and 0 <= iw < c.W:
                    s += float(t["x"][b, ih, iw] @ t["w"][b, n, kh, kw])
        s = s * float(t["scale"][n]) + float(t["bias"][b, n]) + float(t["residual"][b, oh, ow, n])
        assert abs(max(s, 0.0) - float(ref[b, oh, ow, n])) <= 1e-12


@pytest.mark.parametrize("key", CF.DGRAD_CASES[::4] + CF.SLICE_CASES, ids=str)
def test_the_dgrad_reference_and_the_restatement(key):
    c = CF.dgrad_inputs(key)
    ref, A = CF.dgrad_reference(key)
    assert _close(CF.dgrad_taps(c["dy"].double(), c["w"].double(), c["pad"]), ref)
    assert bool((A > 0).all()) or bool((ref[A == 0] == 0).all())
    got = CF.emulate_dgrad(key)
    assert not bool(torch.isnan(got).any()) and CF.dgrad_worst(key, got)[0] <= CF.limit("dgrad")


def test_the_rotation_and_the_one_hot_statement():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(7, 5, 3, 3, generator=g)
    wf = CF.rotate(w)
    assert all(float(wf[ci, kh, kw, co]) == float(w[co, ci, 2 - kh, 2 - kw]) for ci in range(5) for kh in range(3) for kw in range(3) for co in range(7))
    for ph, pw in CF.ROTATION_PIXELS:
        dy = torch.zeros(1, 5, 6, 7)
        dy[0, ph, pw, 3] = 1.0
        auto = CF.dgrad_autograd(dy, w, 1)[0]
        want = CF.one_hot_expected(w, 5, 6, ph, pw, 3)
        assert torch.equal(auto, want)                                       # (== : autograd may write -0.0 where the statement has +0.0)
        assert int((want != 0).sum()) == 5 * (9 if (ph, pw) == (2, 3) else 4)
        # the emulation of the library's route gives the statement's bits
        A = CF.im2col(dy, 3, 1, 1).reshape(1, -1, 63)
        assert CF.same_bits(CF.accumulate(A, wf.reshape(5, -1), False).reshape(5, 6, 5), want)


def test_the_committed_f32_figures_are_measured():
    got = CF.f32_worst()
    assert set(got) == set(CF.F32_WORST) == {"fwd_single", "fwd_two_level", "fwd_vec1", "dgrad"}
    for fam, v in got.items():
        assert CF.F32_WORST[fam] / 2 <= v <= CF.F32_WORST[fam] * 2, (fam, v)


@pytest.mark.parametrize("plant", CF.FORWARD_PLANTS)
def test_every_planted_forward_error_fails(plant):
    hit = [c.name for c in CF.FORWARD_CASES if CF.plant_applies(c.name, plant) and c.name not in CF.DEVICE_REFERENCE]
    assert len(hit) >= 3, hit
    if plant == "no_hi":
        assert {64, 128} == {FORMS[n][0] for n in hit}
    if plant == "flush_last":
        assert {32, 40} <= {-(-CALLS[n].K // CF.BK) for n in hit}
    if plant == "res_side":
        assert {CF.ACT_RELU, CF.ACT_LEAKY, CF.ACT_SIGMOID} == {CF.FORWARD[n].act for n in hit}
    for name in hit:
        assert CF.forward_worst(name, CF.emulate_forward(name, plant))[0] > CF.limit(CF.family(CF.FORWARD[name])), (plant, name)
    # and changes nothing where it does not apply
    quiet = next(c.name for c in CF.FORWARD_CASES if not CF.plant_applies(c.name, plant))
    assert CF.same_bits(CF.emulate_forward(quiet, plant), CF.emulate_forward(quiet))


@pytest.mark.parametrize("plant", CF.DGRAD_PLANTS)
def test_every_planted_rotation_error_fails(plant):
    axis = 2 if plant == "no_kh_flip" else 3
    hit = [c for c in CF.DGRAD_CASES if c[0] == 3 and c[axis] > 1]
    assert len(hit) >= 20
    for key in hit[::3]:
        assert CF.dgrad_worst(key, CF.emulate_dgrad(key, plant))[0] > CF.limit("dgrad"), (plant, key)
    # a 1x1 has nothing to flip
    key = next(c for c in CF.DGRAD_CASES if c[0] == 1)
    assert CF.same_bits(CF.emulate_dgrad(key, plant), CF.emulate_dgrad(key))
    # the one-hot statement sees one mis-rotated tap bit for bit
    w = CF.dgrad_inputs((3, 1, 5, 9, 12, 8, "base"))["w"]
    dy = torch.zeros(1, 5, 6, 8)
    dy[0, 2, 3, 1] = 1.0
    got = CF.accumulate(CF.im2col(dy, 3, 1, 1).reshape(1, -1, 72), CF.rotate(w, plant).reshape(12, -1), False).reshape(5, 6, 12)
    assert not CF.same_bits(got, CF.one_hot_expected(w, 5, 6, 2, 3, 1))


def test_the_buffers_are_slices_with_sentinels():
    for name in ("lin_slices_odd", "n300_res_wide", "bat_k3", "x_off4"):
        c, t = CF.FORWARD[name], CF.forward_inputs(name)
        b = CF.forward_buffers(name, "cpu")
        assert b["x"].data_ptr() % 16 == CALLS[name].x_align and b["w"].data_ptr() % 16 == 0
        assert torch.equal(b["x"].reshape(t["x"].shape), t["x"]) and bool(torch.isnan(b["y"]).all())
        for k, pad in (("x", c.xp), ("y", c.yp), ("r", c.rp)):
            if pad is not None:
                C = b[k].shape[-1]
                assert b[k + "_buf"].shape[-1] == C + sum(pad)
                assert bool((b[k + "_buf"][..., :pad[0]] == CF.FILL).all()) and bool((b[k + "_buf"][..., pad[0] + C:] == CF.FILL).all())
    b = CF.dgrad_buffers((3, 2, 5, 9, 300, 8, "dx304"), "cpu")
    assert b["dx_buf"].shape[-1] == 304 and bool((b["dx_buf"][..., 300:] == 7.0).all()) and bool(torch.isnan(b["dx"]).all())
