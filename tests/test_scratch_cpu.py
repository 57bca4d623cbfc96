"""The workspace-size entries of include/nopesac_hip.h and the argument stage of nopesac_sumsq_accumulate_f32, library loaded only (no GPU):
each size entry returns the formula its header comment states - the expression its launcher checks against -, is never negative, and the
sum of squares refuses a missing or short workspace instead of running another algorithm."""
import ctypes

import pytest

from nopesac_amd import _lib

H = _lib.H
RPS = H.NPS_BN_TRAIN_RPS


def _lib_or_skip():
    try:
        return _lib.load()
    except RuntimeError as e:            # pragma: no cover - the library is built by build()
        pytest.skip(str(e))


def _sumsq_slices(n):
    if n <= 16384:
        return 0
    chunk = ((n + 255) // 256 + 4095) // 4096 * 4096
    return -(-n // chunk)


# entry -> (the header's formula, argument sets; the last argument set of each is degenerate)
SIZES = {
    "nopesac_bn_train_workspace_floats": (lambda n, C: -(-n // RPS) * 2 * C, [(RPS, 8), (RPS + 1, 8), (130, 4), (4 * 15 * 20 * 4, 256)]),
    "nopesac_linear_backward_workspace_floats": (lambda N, K, S: S * (N * K + N), [(128, 132, 1), (256, 1024, 7), (4, 4, 1024)]),
    "nopesac_mask_product_wgrad_workspace_floats": (lambda L, B, nq, cr, S: S * B * (L * nq + cr) * H.NPS_MASK_PRODUCT_WS_ROW_FLOATS,
                                                    [(1, 2, 3, 0, 1), (2, 2, 7, 2, 2), (3, 32, 50, 2, 16)]),
    "nopesac_attention_train_backward_workspace_floats": (lambda B, h, Lq: B * h * Lq * H.NPS_ATT_TRAIN_WS_ROW_FLOATS, [(2, 2, 5), (32, 8, 50), (1, 1, 1)]),
    "nopesac_groupnorm_workspace_floats": (lambda B, G: B * 16 * G * 2, [(2, 32), (1, 1), (32, 256)]),
    "nopesac_groupnorm_backward_workspace_floats": (lambda B, C: B * 2 * C, [(2, 64), (1, 4), (32, 256)]),
    "nopesac_conv2d_p8n_splitk_workspace_bytes": (lambda S, M, Cout: S * M * Cout * 4, [(2, 300, 128), (16, 32 * 15 * 20, 128), (3, 1, 256)]),
    "nopesac_sumsq_workspace_floats": (_sumsq_slices, [(1,), (16384,), (16385,), (70001,), (4096 * 256,), (4096 * 256 + 1,), (1 << 33,)]),
}


@pytest.mark.parametrize("entry", sorted(SIZES))
def test_size_entry_is_the_formula_of_its_header_comment(entry):
    L = _lib_or_skip()
    formula, cases = SIZES[entry]
    fn = getattr(L, entry)
    assert entry not in _lib.STATUS and fn.restype is ctypes.c_int64          # a value, not a status
    for args in cases:
        assert fn(*args) == formula(*args) >= 0, (entry, args)


def test_sumsq_slice_rule():
    """5 slices at 16385, 256 at 4096 * 256, and one element more doubles the slice length: 129."""
    L = _lib_or_skip()
    f = L.nopesac_sumsq_workspace_floats
    assert [f(n) for n in (16384, 16385, 4096 * 256, 4096 * 256 + 1)] == [0, 5, 256, 129]
    assert all(0 <= f(n) <= 256 for n in (16386, 99999, 1 << 20, (1 << 20) + 4097, 1 << 28, (1 << 40) + 3))


@pytest.mark.parametrize("entry", sorted(SIZES))
def test_size_entry_is_never_negative(entry):
    """Zero and negative arguments, one position at a time and all at once: 0 or positive."""
    L = _lib_or_skip()
    fn = getattr(L, entry)
    good = SIZES[entry][1][0]
    for bad in (0, -1, -(1 << 20)):
        for i in range(len(good)):
            args = list(good)
            args[i] = bad
            assert fn(*args) >= 0, (entry, args)
        assert fn(*([bad] * len(good))) >= 0, (entry, bad)


def test_sumsq_refuses_a_missing_or_short_workspace():
    """Argument checks precede any launch (no device needed).  Above 16384 elements a null workspace, or one a float short of the size
    entry's value, is NPS_E_ARG with a message that names the workspace: there is no fallback to the one-workgroup kernel.  At 16384
    a null workspace passes that check - with a null accumulator the call is then refused for the accumulator, not for the workspace."""
    L = _lib_or_skip()
    E = H.NPS_E_ARG
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f = L.nopesac_sumsq_accumulate_f32
    need = L.nopesac_sumsq_workspace_floats(16385)
    assert need == 5
    assert f(p, 16385, p, None, 0, None) == E and b"workspace" in L.nopesac_last_error()
    assert f(p, 16385, p, None, 256, None) == E and b"workspace" in L.nopesac_last_error()
    assert f(p, 16385, p, p, need - 1, None) == E and b"workspace" in L.nopesac_last_error()
    assert f(p, 16385, None, p, need, None) == E and b"workspace" not in L.nopesac_last_error()       # a full workspace: refused for `out`
    assert f(p, 16384, None, None, 0, None) == E and b"workspace" not in L.nopesac_last_error()        # no workspace needed: refused for `out`
    assert f(p, 0, p, None, 0, None) == E and f(None, 16384, p, None, 0, None) == E
