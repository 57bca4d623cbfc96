"""CPU half of the head sweep: the host-only transformer-tail form selector of csrc/enc_tail.hip picks what the if-chain of et_launch picked
before it became a function, the production tails keep their pinned forms, a forced ineligible form is refused before any HIP call, and the
per-element comparators of the GPU sweep fail on planted kernel faults (negative controls: CPU float32 emulations with the kernels'
rounding points play the kernels)."""
import pytest
import torch

from tests import head_forms as HF

SW_32, SW_64, SW_ROWS, SW_ROWS3 = 1, 2, 4, 8


def _legacy_form(M, pre_norm, skip_ffn, sw):
    """The if-chain of et_launch before the selector (verbatim but for launches -> form names and getenv -> switch bits)."""
    if not pre_norm and not skip_ffn and M >= 2048 and not sw & SW_32 and not sw & SW_64:
        nr = 3 if ((M + 127) // 128 <= 160 and (M + 95) // 96 <= 256) else 4
        if sw & SW_ROWS:
            nr = 3 if sw & SW_ROWS3 else 4
        return "t96" if nr == 3 else "t128"
    elif not pre_norm and not skip_ffn and M >= 2048 and not sw & SW_32:
        return "t64"
    else:
        return "t32"


def _ms():
    g = torch.Generator().manual_seed(5)
    ms = {1, 2, 31, 32, 33, 95, 96, 97, 127, 128, 129, 2047, 2048, 2049, 2100, 3200, 4096, 8192, 19200, 20479, 20480, 20481, 20482,
          24575, 24576, 24577, 25000}
    ms |= {int(v) for v in torch.randint(1, 25001, (300,), generator=g)}
    return sorted(ms)


def test_form_names_match_the_header():
    import os
    import re
    from nopesac_amd import _lib, ops
    text = open(_lib.HEADER_PATH).read()
    ids = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define NPS_ETAIL_(\w+) (\d+)", text) if not m.group(1).startswith("SW_")}
    assert ids.pop("forms") == len(ops.TRANSFORMER_TAIL_FORMS)
    assert {n: i for i, n in enumerate(ops.TRANSFORMER_TAIL_FORMS)} == {"t" + k: v for k, v in ids.items()}
    sw = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define NPS_ETAIL_SW_(\w+) (\d+)", text)}
    assert sw == {"32": SW_32, "64": SW_64, "ROWS": SW_ROWS, "ROWS3": SW_ROWS3}
    assert sorted(ops.TRANSFORMER_TAIL_SWITCHES.values()) == [SW_32, SW_64, SW_ROWS, SW_ROWS3]
    src = open(os.path.join(os.path.dirname(_lib.HEADER_PATH), "..", "nopesac_amd", "csrc", "enc_tail.hip")).read()
    for env in ("NOPESAC_ENC_TAIL_32", "NOPESAC_ENC_TAIL_64", "NOPESAC_ENC_TAIL_ROWS"):
        assert 'getenv("%s")' % env in src, env


def test_selector_matches_the_old_chain():
    """M = 1..25000 sampled with every boundary, pre_norm x skip_ffn, all 16 switch combinations: the selector's default is the old chain's
    choice, and it is eligible whenever the projections fit the 32-token kernel."""
    from nopesac_amd import ops
    n = 0
    for M in _ms():
        for pre, skip in ((0, 0), (1, 0), (1, 1)):
            for sw in range(16):
                if sw & SW_ROWS3 and not sw & SW_ROWS:
                    continue                                  # ROWS3 implies ROWS
                for nproj in (0, 768, 1024, 1056):
                    form, mask = ops.transformer_tail_forms(M, pre, skip, nproj, sw)
                    want = _legacy_form(M, pre, skip, sw)
                    assert ops.TRANSFORMER_TAIL_FORMS[form] == want, (M, pre, skip, sw, nproj, form, want)
                    assert (mask >> form) & 1 or (form == 0 and nproj > 1024), (M, pre, skip, sw, nproj, mask)
                    n += 1
    assert n > 300 * 3 * 12 * 4


def test_eligibility_follows_the_kernels():
    """The 64- / 96- / 128-token forms at every M of the post-norm tail (they guard or clamp every row, also below 2048), never for the pre-norm
    or skip_ffn forms (they have no such path); the 32-token form for every call whose projections fit its four rounds."""
    from nopesac_amd import ops
    for M in (1, 7, 100, 2047, 2100, 19200, 25000):
        assert ops.transformer_tail_forms(M, 0, 0, 768)[1] == 0b1111
        assert ops.transformer_tail_forms(M, 0, 0, 2048)[1] == 0b1110
        assert ops.transformer_tail_forms(M, 1, 0, 768)[1] == 0b0001
        assert ops.transformer_tail_forms(M, 1, 1, 256)[1] == 0b0001
        assert ops.transformer_tail_forms(M, 1, 1, 1056)[1] == 0


def test_production_tails_keep_their_forms():
    from nopesac_amd import ops
    got, want = {}, {}
    for key in HF.production_tails():
        _, entry, M, pre, skip, _, n_pos, n_proj, _, _ = key
        form, mask = ops.transformer_tail_forms(M, pre, skip, n_pos + n_proj, 0)
        got[key], want[key] = ops.TRANSFORMER_TAIL_FORMS[form], HF.PRODUCTION[key]
        assert (mask >> form) & 1
    assert got == want
    assert {HF.PRODUCTION[k] for k in HF.production_tails() if k[2] == 19200} == {"t96"}


def test_forced_ineligible_form_is_refused_without_a_gpu():
    """nopesac_transformer_tail_bf16_form refuses a form outside the eligibility mask - a wide-token form on the pre-norm or skip_ffn tail,
    the 32-token form with more than 1024 projection columns, an id out of range - with the argument error, before any HIP call."""
    from nopesac_amd import _lib
    lib = _lib.load()
    P = 16                                                     # any 16-byte aligned non-null address: nothing is dereferenced

    def call(M, pre, skip, n_pos, form):
        ffn = None if skip else P
        return lib.nopesac_transformer_tail_bf16_form(P, P, P, P, P, P, ffn, ffn, ffn, ffn, ffn, ffn, P, 50, P, None, None, None, pre, skip,
                                                      P, None, P, n_pos, None, None, None, 0, M, None, None, 0, 0, form, None)

    for args, name in (((3200, 1, 0, 512, 1), b"t64"), ((3200, 1, 0, 512, 2), b"t96"), ((100, 1, 1, 256, 3), b"t128"),
                       ((19200, 0, 0, 1056, 0), None)):
        rc = call(*args)
        assert rc == -1, (args, rc)
        msg = lib.nopesac_last_error()
        if name is None:
            assert b"> 1024 on the 32-token kernel" in msg, msg
        else:
            assert b"not eligible" in msg and b"(" + name + b")" in msg, (args, msg)
        with pytest.raises(_lib.HipKernelError):
            _lib.check(rc, "nopesac_transformer_tail_bf16_form")
    for form in (-1, 4):
        assert call(3200, 0, 0, 512, form) == -1 and b"out of range" in lib.nopesac_last_error()
    # the shared argument checks still come first
    assert call(0, 0, 0, 512, 2) == -1 and b"null pointer" in lib.nopesac_last_error()


# ---------------------------------------------------------------------------------------------------------------------------- controls
MARGIN = 8.0
_CACHE = {}


def _tail_control(pre_norm):
    key = ("tail", pre_norm)
    if key not in _CACHE:
        # 2 images x 100 tokens would do; 230 leaves a ragged 96-token tile (230 = 2 x 96 + 38) and wraps pos inside a tile
        c = HF.build_tail(230, pre_norm, False, 64, 32, 50, "cpu", seed=11)
        rows = torch.arange(c.M)
        _CACHE[key] = (c, rows, HF.tail_reference(c, rows))
    return _CACHE[key]


def _tail_ratio(pre_norm, fault):
    c, rows, ref = _tail_control(pre_norm)
    emu = HF.tail_reference(c, rows, fault=fault, dtype=torch.float32)
    worst = 0.0
    for k in ("n", "u"):
        r, E = ref[k]
        worst = max(worst, HF.error_ratio(emu[k][0], r, HF.out_tol(r, E, torch.float32))[0])
    n32 = emu["n"][0].float()
    o_emu = HF.tail_outputs_reference(c, rows, n32, fault=fault, dtype=torch.float64)
    o_ref = HF.tail_outputs_reference(c, rows, n32)
    # ypos16 against f64 n + pos: the kernel's bf16 output within half a unit of its own f32 n + pos
    rpos = n32.double() + c.pos[rows % c.pos_rows].double()
    worst = max(worst, HF.error_ratio(o_emu["ypos16"].float(), rpos, HF.out_tol(rpos, 0 * rpos + 2.0 ** -22 * rpos.abs(), torch.bfloat16))[0])
    for k in ("proj_pos", "proj"):
        v_emu = o_emu[k][0].to(torch.bfloat16).float()        # the fault's projection, stored as the kernel stores it
        r, A = o_ref[k]
        worst = max(worst, HF.error_ratio(v_emu, r, HF.out_tol(r, HF.GEMM * A, torch.bfloat16))[0])
    return worst


TAIL_FAULTS = ["pos_row_off_by_one_at_tile_edge", "linear2_last_k_step_skipped", "b1_missing_on_one_hidden_tile",
               "ln_a_uses_ln_b_params_for_one_wave", "ragged_tile_reads_last_row", "proj_pos_from_n_for_one_tile"]


@pytest.mark.parametrize("pre_norm", [False, True], ids=["post", "pre"])
def test_tail_control_without_a_fault_passes(pre_norm):
    assert _tail_ratio(pre_norm, None) <= 1.0


@pytest.mark.parametrize("fault", TAIL_FAULTS)
def test_tail_planted_fault_fails(fault):
    q = _tail_ratio(False, fault)
    print("control tail %-40s worst / tol %.3g" % (fault, q))
    assert q >= MARGIN, q


def _att_control():
    if "att" not in _CACHE:
        c = HF.build_attention(2, 40, 70, (256, 256, 256), False, seed=3, device=None)
        _CACHE["att"] = (c, [HF.attention_reference(c, b, qlen=37 if b else None, klen=66 if b else None) for b in range(2)])
    return _CACHE["att"]


def _att_ratio(fault):
    c, refs = _att_control()
    worst = 0.0
    for b in range(2):
        o, _ = HF.attention_reference(c, b, qlen=37 if b else None, klen=66 if b else None, fault=fault, dtype=torch.float32)
        r, E = refs[b]
        worst = max(worst, HF.error_ratio(o, r, HF.out_tol(r, E, torch.float32))[0])
    return worst


ATT_FAULTS = ["key_mask_at_nk_minus_1", "running_max_rescale_skipped", "v_rows_shifted_in_second_tile", "scale_applied_twice_in_one_head"]


def test_attention_control_without_a_fault_passes():
    assert _att_ratio(None) <= 1.0


@pytest.mark.parametrize("fault", ATT_FAULTS)
def test_attention_planted_fault_fails(fault):
    q = _att_ratio(fault)
    print("control attention %-35s worst / tol %.3g" % (fault, q))
    assert q >= MARGIN, q


def _gnn_control():
    if "gnn" not in _CACHE:
        nq = 100
        W = HF.build_gnn_weights(21)
        x = HF.gnn_features(2, nq, 22)
        n = [100, 70]                                          # a cross pair: set 0 attends to set 1 (70 keys), 100 live query rows
        _CACHE["gnn"] = (W, x, n, HF.gnn_reference(W, x[0], x[1], n[0], n[1]))
    return _CACHE["gnn"]


def _gnn_ratio(fault):
    W, x, n, (r, E) = _gnn_control()
    nkey = n[0] if fault == "klen_from_query_set" else n[1]
    o, _ = HF.gnn_reference(W, x[0], x[1], n[0], nkey, fault=fault, dtype=torch.float32)
    return HF.error_ratio(o, r, HF.out_tol(r, E, torch.float32))[0]


GNN_FAULTS = ["klen_from_query_set", "second_query_block_reuses_block_0_q", "chunk2_rescale_skipped", "residual_added_before_ln2"]


def test_gnn_control_without_a_fault_passes():
    assert _gnn_ratio(None) <= 1.0


@pytest.mark.parametrize("fault", GNN_FAULTS)
def test_gnn_planted_fault_fails(fault):
    q = _gnn_ratio(fault)
    print("control gnn %-41s worst / tol %.3g" % (fault, q))
    assert q >= MARGIN, q
