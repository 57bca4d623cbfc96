"""CPU half of the bottleneck-tail form sweep: the host-only form selector of csrc/pwchain.hip picks what the if-chain of
nopesac_bottleneck_tail_bf16_ex picked before it became a function, the production tails keep their pinned forms, a forced ineligible
form is refused before any HIP call, and the comparators of the GPU sweep fail on planted kernel faults (negative controls: a CPU float32
emulation of the tail plays the kernel)."""
import pytest
import torch

from nopesac_amd.ops import BOTTLENECK_TAIL_CONFIGS
from tests import conv_routing as CR
from tests import tail_forms as TF

NO_RT4, NO_RT8, RT4_LATE, NO_RT4H, RT8_WIDE, NO_STREAM = 1, 2, 4, 8, 16, 32


def _legacy_form(C, C4, CN, C2, M, x2_stride, same_res, sw):
    """The if-chain of nopesac_bottleneck_tail_bf16_ex before the selector (verbatim but for launches -> form names, getenv -> switch
    bits, x2 -> C2 > 0, and x2_H == OH && x2_W == OW -> same_res); None where it set 'unsupported channel configuration'."""
    x2 = C2 > 0
    c2 = C2 if x2 else 0
    no_rt4 = bool(sw & NO_RT4)
    if not x2 and not no_rt4 and M % 128 == 0:
        for c, c4, cn in ((128, 512, 128), (128, 512, 0), (64, 256, 64), (64, 256, 128), (64, 256, 0)):
            if C == c and C4 == c4 and CN == cn:
                return "rt4_late" if sw & RT4_LATE else "rt4"
    no_rt8 = bool(sw & NO_RT8)
    if not no_rt4 and not no_rt8 and M % 64 == 0 and C == 128 and C4 == 512 and not sw & NO_RT4H:
        if not x2 and CN == 256:
            return "rt4h"
        if x2 and CN == 128 and c2 == 256:
            return "rt4h"
    if not no_rt4 and not no_rt8 and M % 128 == 0 and C == 128 and C4 == 512:
        if not x2 and CN == 256:
            return "rt8"
        if x2 and CN == 128 and c2 == 256:
            return "rt8"
    if x2 and not no_rt4 and M % 128 == 0 and x2_stride == 1 and same_res:
        if C == 64 and C4 == 256 and CN == 64 and c2 == 64:
            return "rt4_proj"
        if C == 64 and C4 == 256 and CN == 0 and c2 == 64:
            return "rt4_proj"
    for c, c4, cn, cc2 in ((64, 256, 64, 0), (64, 256, 128, 0), (64, 256, 64, 64), (64, 256, 0, 0), (64, 256, 0, 64), (128, 512, 128, 0),
                           (128, 512, 256, 0), (128, 512, 128, 256), (128, 512, 0, 0), (128, 512, 0, 256)):
        if C == c and C4 == c4 and CN == cn and c2 == cc2:
            return "pw"
    if not x2 and M % 128 == 0 and C == 256 and C4 == 1024 and CN == 256 and sw & RT8_WIDE:
        return "rt8"
    if not x2 and not sw & NO_STREAM:
        if C == 256 and C4 == 1024 and CN == 256:
            return "stream"
        if C == 256 and C4 == 1024 and CN == 0:
            return "stream"
    for c, c4, cn, cc2 in ((256, 1024, 256, 0), (256, 1024, 512, 0), (256, 1024, 256, 512), (256, 1024, 0, 0), (256, 1024, 0, 512)):
        if C == c and C4 == c4 and CN == cn and c2 == cc2:
            return "wide"
    return None


def _name(form):
    from nopesac_amd import ops
    return ops.TAIL_FORMS[form] if form >= 0 else None


# ---------------------------------------------------------------------------------------------------------------------------- selector

def test_form_names_match_the_header():
    import os
    import re
    from nopesac_amd import _lib, ops
    text = open(_lib.HEADER_PATH).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NPS_TAIL_(\w+) (\d+)", text) if not m.group(1).startswith("SW_")}
    assert ids.pop("forms") == len(ops.TAIL_FORMS)
    assert {n: i for i, n in enumerate(ops.TAIL_FORMS)} == ids
    sw = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NPS_TAIL_SW_(\w+) (\d+)", text)}
    assert {"NOPESAC_TAIL_" + k: v for k, v in sw.items()} == ops.TAIL_SWITCHES
    assert (NO_RT4, NO_RT8, RT4_LATE, NO_RT4H, RT8_WIDE, NO_STREAM) == tuple(ops.TAIL_SWITCHES[k] for k in (
        "NOPESAC_TAIL_NO_RT4", "NOPESAC_TAIL_NO_RT8", "NOPESAC_TAIL_RT4_LATE", "NOPESAC_TAIL_NO_RT4H", "NOPESAC_TAIL_RT8_WIDE",
        "NOPESAC_TAIL_NO_STREAM"))
    src = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "nopesac_amd", "csrc", "pwchain.hip")).read()
    for env in ops.TAIL_SWITCHES:                # every switch bit is set from its environment variable
        assert 'getenv("%s")' % env in src, env


@pytest.mark.parametrize("cfg", sorted(BOTTLENECK_TAIL_CONFIGS), ids=lambda c: "C%d-%d_cn%d_c2_%d" % c)
def test_selector_matches_the_old_chain(cfg):
    """Every config with and without a projection source, M = 128k / 128k + 64 / odd, stride 1 / 2, same resolution or not, all 64
    switch combinations: the selector's default is the old chain's choice and is always among the eligible forms."""
    from nopesac_amd import ops
    C, C4, CN, C2 = cfg
    n = 0
    for c2 in sorted({C2, 0, 2 * C if C > 64 else 64}):
        for M in (128 * 75, 128 * 300 + 64, 128 * 9 + 64, 4801, 351, 64, 128):
            for stride, same_res in ((1, True), (1, False), (2, False), (2, True)):
                for sw in range(64):
                    form, mask = ops.bottleneck_tail_forms(C, C4, CN, c2, M, stride, same_res, sw)
                    want = _legacy_form(C, C4, CN, c2, M, stride, same_res, sw)
                    assert _name(form) == want, (C, C4, CN, c2, M, stride, same_res, sw, _name(form), want)
                    if want is not None:
                        assert (mask >> form) & 1, (C, C4, CN, c2, M, stride, same_res, sw, mask)
                    else:
                        assert mask == 0
                    n += 1
    assert n >= 2 * 7 * 4 * 64


def test_eligibility_mask_is_the_union_of_the_old_chain_over_the_switches():
    """A form is eligible exactly where some switch combination made the old chain pick it (rt4 / rt4_late: the same configs), so the
    mask neither offers a form the dispatcher never ran there nor hides one it could run."""
    from nopesac_amd import ops
    for (C, C4, CN, C2) in sorted(ops.BOTTLENECK_TAIL_CONFIGS):
        for M in (128 * 75, 128 * 300 + 64, 4801):
            for stride, same_res in ((1, True), (2, False)):
                picked = {_legacy_form(C, C4, CN, C2, M, stride, same_res, sw) for sw in range(64)}
                _, mask = ops.bottleneck_tail_forms(C, C4, CN, C2, M, stride, same_res, 0)
                assert {ops.TAIL_FORMS[f] for f in TF.forms_of(mask)} == picked - {None}, (C, C4, CN, C2, M, stride, picked)


@pytest.mark.parametrize("B", [64, 2])
def test_production_tails_keep_their_forms(B):
    """The default form of every tail the backbone launches (bf16 steps: res2 / res3; fp8 mode and NOPESAC_TAIL_RES4_FUSED=1: res4)."""
    from nopesac_amd import ops
    got = {}
    for name, (cfg, want) in TF.PRODUCTION.items():
        _, OH, OW, H2, W2, s = TF.stage_call(cfg, B)
        form, mask = ops.bottleneck_tail_forms(*cfg, B * OH * OW, s, (H2, W2) == (OH, OW), 0)
        got[name] = _name(form)
    assert got == {name: want for name, (cfg, want) in TF.PRODUCTION.items()}


def test_forced_ineligible_form_is_refused_without_a_gpu():
    """nopesac_bottleneck_tail_bf16_form refuses a form outside the eligibility mask - rt4 / rt4h / rt8 at an M they would overrun, rt4 on a
    projection block, a form with no launcher for the config, an id out of range - with the argument error, before any HIP call."""
    from nopesac_amd import _lib
    lib = _lib.load()
    P = 16                                                     # any 16-byte aligned non-null address: nothing is dereferenced

    def call(C, C4, CN, C2, B, OH, OW, form, proj=False, stride=1, H2=0, W2=0):
        res, x2 = (None, P) if proj else (P, None)
        return lib.nopesac_bottleneck_tail_bf16_form(P, P, P, P, res, x2, P if proj else None, P if proj else None, P if proj else None,
                                                     B, OH, OW, H2, W2, stride, C, C4, C2, P, P if CN else None, P if CN else None,
                                                     P if CN else None, CN, P if CN else None, 1, form, None)

    cases = [
        ((64, 256, 64, 0, 3, 9, 13, 1), b"rt4"),                                         # M = 351: a ragged 128-pixel tile
        ((128, 512, 256, 0, 1, 60, 79, 4), b"rt4h"),                                     # M = 4740: not a multiple of 64
        ((128, 512, 256, 0, 1, 60, 80, 5), b"rt8"),                                      # M = 4800 = 37.5 x 128
        ((256, 1024, 256, 0, 3, 30, 40, 5), b"rt8"),                                     # M = 3600
        ((64, 256, 64, 64, 2, 16, 24, 1, True, 1, 16, 24), b"rt4"),                       # rt4 has no projection form
        ((64, 256, 64, 64, 2, 16, 24, 3, True, 2, 32, 48), b"rt4_proj"),                  # rt4_proj: same-resolution stride-1 source only
        ((256, 1024, 512, 0, 2, 30, 40, 6), b"stream"),                                  # no CN = 512 streaming kernel
        ((64, 256, 64, 0, 2, 16, 24, 7), b"wide"),                                       # wide: C = 256 only
    ]
    for args, name in cases:
        rc = call(*args)
        assert rc == -1, (args, rc)
        msg = lib.nopesac_last_error()
        assert b"not eligible" in msg and b"(" + name + b")" in msg, (args, msg)
        with pytest.raises(_lib.HipKernelError):
            _lib.check(rc, "nopesac_bottleneck_tail_bf16_form")
    for form in (-1, 8):
        assert call(64, 256, 64, 0, 2, 16, 24, form) == -1 and b"out of range" in lib.nopesac_last_error()
    # the shared argument checks still come first
    assert call(64, 256, 64, 0, 0, 16, 24, 1) == -1 and b"bad args" in lib.nopesac_last_error()


# ---------------------------------------------------------------------------------------------------------------------------- controls

# scaled-down calls of the sweep: an identity block, res3.0's stride-2 projection (6 x 10 outputs: every 64-pixel tile crosses an image
# row) and an fp8-o identity block
CONTROLS = {
    "identity_c64": ((64, 256, 64, 0), (2, 12, 16, 0, 0, 1), False),
    "proj_s2_c128": ((128, 512, 128, 256), (2, 6, 10, 12, 20, 2), False),
    "fp8_o_c64": ((64, 256, 64, 0), (2, 12, 16, 0, 0, 1), True),
}
FAULTS = {
    "conv3_drops_last_16_k": ["identity_c64", "proj_s2_c128"],
    "stride2_gather_wrong_row": ["proj_s2_c128"],
    "residual_after_relu": ["identity_c64"],
    "bn_sc_swapped_with_bn3": ["proj_s2_c128"],
    "o_tile_shifted_bn1": ["identity_c64", "proj_s2_c128"],
    "last_tile_y_col_tile_unwritten": ["identity_c64", "proj_s2_c128"],
    "fp8_o_unsaturated": ["fp8_o_c64"],
}
MARGIN = 5.0        # every planted fault must exceed the comparators' bound by at least this factor
_CACHE = {}


def _control(name):
    if name not in _CACHE:
        cfg, shape, o_fp8 = CONTROLS[name]
        c = TF.build_tail(cfg, *shape, torch.device("cpu"), seed=17)
        rows = CR.sample_rows(c.M, c.B, c.OH, c.OW, seed=17)
        y0, o0 = TF.emulate(c, o_fp8=o_fp8)
        _CACHE[name] = (c, rows, TF.reference_y(c, rows), y0, o0, TF.emulate(c)[1] if o_fp8 else None)
    return _CACHE[name]


def _ratios(name, fault):
    """(sampled y vs f64, sampled o vs f64 of the emulated y, full agreement with the fault-free emulation, fp8 o vs its bf16 o)."""
    c, rows, (ry, Ay), y0, o0, o16 = _control(name)
    o_fp8 = CONTROLS[name][2]
    y, o = TF.emulate(c, fault, o_fp8=o_fp8)
    ym = TF.rows_of(y, rows)
    ref_y = CR.error_ratio(ym, ry, Ay, torch.bfloat16)[0]
    full = CR.full_agreement(y, y0)
    ref_o = fp8 = 0.0
    if o_fp8:
        _, o16f = TF.emulate(c, fault)           # the same call with a bf16 o: the fp8 o must be it, converted
        fp8 = TF.fp8_ratio(o, o16f)
    elif c.CN:
        ro, Ao = TF.reference_o(c, ym)
        ref_o = CR.error_ratio(TF.rows_of(o, rows), ro, Ao, torch.bfloat16)[0]
        full = max(full, CR.full_agreement(o, o0))
    return ref_y, ref_o, full, fp8


@pytest.mark.parametrize("name", sorted(CONTROLS))
def test_control_without_a_fault_passes(name):
    ref_y, ref_o, full, fp8 = _ratios(name, None)
    assert ref_y <= 1.0 and ref_o <= 1.0 and full == 0.0 and fp8 == 0.0, (ref_y, ref_o, full, fp8)


@pytest.mark.parametrize("name, fault", [(n, f) for f, names in FAULTS.items() for n in names])
def test_planted_fault_fails_the_comparators(name, fault):
    ref_y, ref_o, full, fp8 = _ratios(name, fault)
    print("control %-13s %-31s y/tol %.3g  o/tol %.3g  full_agreement %.3g  fp8 %.3g" % (name, fault, ref_y, ref_o, full, fp8))
    if fault == "fp8_o_unsaturated":
        assert fp8 >= MARGIN, fp8
    else:
        assert max(ref_y, ref_o) >= MARGIN and full >= MARGIN, (ref_y, ref_o, full)
