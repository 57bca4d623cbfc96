"""MatchingHeadTrainer without a GPU: which state-dict tensors it trains, the norm / non-norm weight-decay split extended to the GNN's
LayerNorms (train_NopeSAC.py:94-128) without touching the camera head's, and the argument checks of the entry points of
csrc/matcher_bwd.hip."""
import ctypes

import pytest

from nopesac_amd import _lib
from nopesac_amd.synth import synth_state_dict
from nopesac_amd.training import CameraHeadTrainer, MatchingHeadTrainer, is_norm_parameter

PFX = "camera_head_list.0."
MPFX = "matching_head."


def _expected_matcher_keys():
    keys = ["bin_score", "planeApp_proj.weight", "planeApp_proj.bias", "planeDesc_proj.weight", "planeDesc_proj.bias"]
    for i in range(18):
        p = f"gnn.layers.{i}."
        keys += [p + n + ".weight" for n in ("q_proj", "k_proj", "v_proj", "merge", "mlp.0", "mlp.2")]
        keys += [p + n + leaf for n in ("norm1", "norm2") for leaf in (".weight", ".bias")]
    return [MPFX + k for k in keys]


def test_matcher_parameter_names():
    sd = synth_state_dict(50)
    names = MatchingHeadTrainer.parameter_names(sd.keys())
    assert len(names) == 185 and sorted(names) == sorted(_expected_matcher_keys())
    assert all(sd[k].is_floating_point() for k in names)
    assert sum(sd[k].numel() for k in names) == 11946497
    assert not set(names) & set(CameraHeadTrainer.parameter_names(sd.keys(), conv_stacks=True))


def test_norm_rule_covers_exactly_the_gnn_layernorms():
    sd = synth_state_dict(50)
    names = MatchingHeadTrainer.parameter_names(sd.keys())
    norm = {k for k in names if is_norm_parameter(k)}
    want = {f"{MPFX}gnn.layers.{i}.{n}.{leaf}" for i in range(18) for n in ("norm1", "norm2") for leaf in ("weight", "bias")}
    assert norm == want and len(norm) == 72
    assert not is_norm_parameter(MPFX + "bin_score")


def test_norm_rule_of_the_camera_head_is_unchanged():
    """The rule stated in is_norm_parameter's docstring before the matcher was added: pixel_decoder.*.norm.{weight,bias} and
    convs_*.i.1.{weight,bias}, for every camera-head key of the state dict (buffers included), with and without the prefix."""
    def rule(key):
        parts = key[len(PFX):].split(".") if key.startswith(PFX) else key.split(".")
        if parts[0] == "pixel_decoder":
            return len(parts) == 4 and parts[2] == "norm"
        if parts[0] in ("pixel_decoder", "convs_backbone", "convs_trans", "convs_rots"):
            return len(parts) == 4 and parts[2] == "1" and parts[3] in ("weight", "bias")
        return False
    keys = [k for k in synth_state_dict(50) if k.startswith(PFX)]
    assert len(keys) > 179
    for k in keys:
        assert is_norm_parameter(k) == rule(k), k
        assert is_norm_parameter(k[len(PFX):]) == rule(k), k
    assert sum(is_norm_parameter(k) for k in keys) == 46


def _lib_or_skip():
    try:
        return _lib.load()
    except RuntimeError as e:            # pragma: no cover - the library is built by build()
        pytest.skip(str(e))


def test_matcher_backward_entry_points_reject_bad_arguments():
    """Every new entry point checks its arguments before any HIP call: NPS_E_ARG and a message, no device needed."""
    L = _lib_or_skip()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    E = -1

    def rejected(rc, word):
        msg = L.nopesac_last_error().decode()
        return rc == E and word in msg

    att = lambda *a: L.nopesac_attention_small_backward(*a)
    # attention: Lq / Lk outside 1..128, heads * 32 wider than a row stride (each of the seven strides), null outputs, null input
    assert rejected(att(p, 256, p, 256, p, 256, p, 256, 1, 129, 50, 8, 0.1, None, None, p, 256, p, 256, p, 256, None), "bad dims")
    assert rejected(att(p, 256, p, 256, p, 256, p, 256, 1, 50, 0, 8, 0.1, None, None, p, 256, p, 256, p, 256, None), "bad dims")
    for bad in range(7):
        st = [256] * 7
        st[bad] = 255
        assert rejected(att(p, st[0], p, st[1], p, st[2], p, st[3], 1, 50, 50, 8, 0.1, None, None, p, st[4], p, st[5], p, st[6], None), "wider")
    assert rejected(att(p, 256, p, 256, p, 256, p, 256, 1, 50, 50, 8, 0.1, None, None, p, 256, None, 256, p, 256, None), "null output")
    assert rejected(att(None, 256, p, 256, p, 256, p, 256, 1, 50, 50, 8, 0.1, None, None, p, 256, p, 256, p, 256, None), "null input")
    # LayerNorm: D != 256, no rows, null outputs, workspace too small
    ln = L.nopesac_layernorm_backward
    assert L.nopesac_layernorm_backward_workspace_floats(257) == 9 * 512 and L.nopesac_layernorm_backward_workspace_floats(1) == 512
    assert rejected(ln(p, p, p, 4, 128, 1e-5, p, p, p, p, 1 << 20, None), "bad dims")
    assert rejected(ln(p, p, p, 0, 256, 1e-5, p, p, p, p, 1 << 20, None), "bad dims")
    assert rejected(ln(p, p, p, 4, 256, 1e-5, None, p, p, p, 1 << 20, None), "null output")
    assert rejected(ln(p, p, p, 4, 256, 1e-5, p, p, p, None, 1 << 20, None), "null output")
    assert rejected(ln(p, p, p, 33, 256, 1e-5, p, p, p, p, 512, None), "workspace")
    # Sinkhorn training twin, forward and backward: nq outside 1..128, iters < 0, null outputs
    fw = lambda nq, iters, ls, loss: L.nopesac_matcher_sinkhorn_train(p, p, p, p, p, p, p, 4.0, 8.0, iters, p, 1, nq, ls, p, p, loss, None)
    assert rejected(fw(0, 3, p, p), "bad dims") and rejected(fw(129, 3, p, p), "bad dims") and rejected(fw(50, -1, p, p), "bad dims")
    assert rejected(fw(50, 3, None, p), "null output") and rejected(fw(50, 3, p, None), "null output")
    bw = lambda nq, iters, dd, db: L.nopesac_matcher_sinkhorn_train_backward(p, p, p, p, p, p, p, 4.0, 8.0, iters, p, p, p, p, 1, nq, dd, db, None)
    assert rejected(bw(0, 3, p, p), "bad dims") and rejected(bw(129, 3, p, p), "bad dims") and rejected(bw(50, -1, p, p), "bad dims")
    assert rejected(bw(50, 3, None, p), "null output") and rejected(bw(50, 3, p, None), "null output")
    # the loss on existing log scores: nq outside 1..128, null outputs, null input
    el = lambda nq, ls, st, lo: L.nopesac_matcher_emb_loss(ls, p, p, p, 1, nq, st, lo, None)
    assert rejected(el(0, p, p, p), "bad dims") and rejected(el(129, p, p, p), "bad dims")
    assert rejected(el(50, p, None, p), "null output") and rejected(el(50, p, p, None), "null output") and rejected(el(50, None, p, p), "null input")
    # descriptor dot: nq outside 1..128, D != 256, null outputs
    dd = lambda nq, D, o0, o1: L.nopesac_desc_dot_backward(p, p, p, p, p, 1, nq, D, o0, o1, None)
    assert rejected(dd(0, 256, p, p), "bad dims") and rejected(dd(129, 256, p, p), "bad dims") and rejected(dd(50, 128, p, p), "bad dims")
    assert rejected(dd(50, 256, None, p), "null output") and rejected(dd(50, 256, p, None), "null output")
