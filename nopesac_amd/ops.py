"""Thin typed wrappers: torch tensors (device memory + the current HIP stream) -> C-ABI calls.

torch is plumbing here (allocation, streams); every computation below runs in libnopesac_hip.so.
All wrappers enqueue on torch's current stream and never synchronise.  This is the one module through which device pointers of
caller-supplied tensors reach the library (inference, conv backward, the training path's backward kernels and optimiser): what the C side
cannot see - device, dtype, strides, element counts - is checked here, with explicit raises that stay in force under `python -O`.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import ctypes
import functools
import os

import torch

from . import _lib

_H = _lib.H                                     # the constants of include/nopesac_hip.h (H is a height below)
F32, BF16, FP8 = _H.NPS_DT_F32, _H.NPS_DT_BF16, _H.NPS_DT_FP8         # FP8: OCP e4m3fn bytes
ACT_NONE, ACT_RELU, ACT_LEAKY, ACT_SIGMOID = _H.NPS_ACT_NONE, _H.NPS_ACT_RELU, _H.NPS_ACT_LEAKY, _H.NPS_ACT_SIGMOID
ACT_RES_AFTER = _H.NPS_ACT_RES_AFTER         # OR-able: residual is added after the activation
ACT_BIAS_BATCHED = _H.NPS_ACT_BIAS_BATCHED   # OR-able (set by conv2d): with batched weights, bias is [B, Cout]
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float8_e4m3fn: FP8}


class OpsArgumentError(AssertionError, ValueError):
    """A wrapper's argument check failed.  Raised explicitly (not `assert`): the checks stay in force under `python -O`.
    (Subclasses AssertionError so that callers written against the first version keep working.)"""


def _require(cond, msg="argument check failed"):
    if not cond:
        raise OpsArgumentError(msg if isinstance(msg, str) else repr(msg))


_C = _lib.C                                     # the library as the wrappers call it: a refused call raises HipKernelError by itself


def _L():
    """The raw library, for callers that read an entry point's status themselves (tests, scripts)."""
    return _lib.load()


try:                                            # torch.cuda.current_stream() builds a Stream object through four layers of Python
    _raw_stream, _raw_device = torch._C._cuda_getCurrentRawStream, torch._C._cuda_getDevice   # (8 us per launch, a fifth of the submit time)
except AttributeError:                          # a torch build without the private accessors
    _raw_stream = _raw_device = None


def _stream():
    """hipStream_t (as an int) of torch's current stream on the current device."""
    if _raw_stream is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


_NO_CPU_PATH = "nopesac_amd ops need device tensors (there is no CPU path)"


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:                           # (raised in place, not through _require: these two run for every tensor of every launch)
        raise OpsArgumentError(_NO_CPU_PATH)
    return t.data_ptr()


def _chk(t: torch.Tensor, dtype=None, contiguous=True):
    if not t.is_cuda:
        raise OpsArgumentError(_NO_CPU_PATH)
    if dtype is not None and t.dtype != dtype:
        raise OpsArgumentError(repr((t.dtype, dtype)))
    if contiguous and not t.is_contiguous():
        raise OpsArgumentError('argument check failed: t.is_contiguous()')
    return t


def _sized(t: torch.Tensor, dtype, n: int, what: str) -> torch.Tensor:
    """A contiguous device tensor of `dtype` with exactly n elements."""
    _chk(t, dtype)
    if t.numel() != n:
        raise OpsArgumentError("%s: %d elements expected, got shape %s" % (what, n, tuple(t.shape)))
    return t


def _lengths(t: Optional[torch.Tensor], B: int, what: str) -> Optional[torch.Tensor]:
    """The per-set lengths of a ragged batch (attention's qlen / klen): None, or int32 [B] on the device."""
    return None if t is None else _sized(t, torch.int32, B, what)


def _rows(t: torch.Tensor, rows: int, cols: int, what: str) -> int:
    """f32 device matrix [rows, >= cols] with unit column stride (a column slice of a wider buffer is allowed) -> its row stride."""
    _chk(t, torch.float32, contiguous=False)
    if not (t.dim() == 2 and t.shape[0] == rows and t.shape[1] >= cols and t.stride(1) == 1):
        raise OpsArgumentError("%s: [%d, >= %d] with unit column stride expected, got shape %s, strides %s"
                               % (what, rows, cols, tuple(t.shape), tuple(t.stride())))
    return t.stride(0)


class ConvTuner:
    """Load-time autotuner: for every distinct conv/GEMM problem signature, time the kernel configurations the
    library offers (they all compute the same result) and remember the fastest.  Off by default; a model turns
    it on for one dedicated, single-stream pass (PlaneTR_NopeSAC.autotune) and then freezes it."""
    CANDIDATES = (0, 1, 2, 3, 4)

    def __init__(self):
        self.best = {}
        self.loaded = {}          # key_str -> cfg from a routing file (ConvTuner.load)
        self.measuring = False
        self.log = []

    def choose(self, key, launch, extra=()):
        cfg = self.best.get(key)
        if cfg is None and self.loaded:
            cfg = self.loaded.get(self.key_str(key))
            if cfg is not None:
                self.best[key] = cfg
        cands = tuple(self.CANDIDATES) + tuple(extra)
        if cfg is not None or not self.measuring:
            return cfg if (cfg is not None and cfg in cands) else 0     # a remembered cfg this call is not eligible for -> heuristic
        times = {}
        ok = []
        for c in cands:
            try:
                launch(c)                                 # warm (first-touch, icache)
                ok.append(c)
            except _lib.HipKernelError:
                # the entry point refuses the call: a configuration from a stale routing file, or one of the few conditions the
                # entry points add to the eligibility mask (csrc/conv_forms.h: the bfrag / halo pointers' own alignment, bfrag's
                # fp8-output form).  The candidate is dropped, tuning goes on.  Configuration 0 (the library's own heuristic) must
                # work - its failure is the caller's error
                if c == 0:
                    raise
        cands = tuple(ok)
        for rnd in range(3):                              # three interleaved rounds, keep each candidate's best: robust to
            for c in cands:                               # a noisy neighbour / clock ramp during one candidate's window
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(6):
                    launch(c)
                e1.record()
                e1.synchronize()
                t = e0.elapsed_time(e1) / 6
                times[c] = min(times.get(c, t), t)
        cfg = min(times, key=times.get)
        if times[cfg] > 0.97 * times[0]:      # keep the heuristic unless a candidate is clearly faster
            cfg = 0
        self.best[key] = cfg
        self.log.append((key, cfg, times))
        return cfg

    # ---- persistent routing: the decisions of one tuning pass as a JSON file, so that the benchmark, the PMC / rocprofv3 scripts
    # and the driver's runs all launch IDENTICAL kernels (profiles/routing_*.json; `bench.py --routing`)
    @staticmethod
    def key_str(key) -> str:
        return "|".join(str(v).replace("torch.", "") for v in key)

    def save(self, path: str, meta: dict = None):
        import json
        rows = {self.key_str(k): int(v) for k, v in self.best.items()}
        with open(path, "w") as f:
            json.dump({"format": "nopesac_amd.ConvTuner/1", "meta": meta or {}, "kernels": {str(k): v for k, v in CONV_CFG_KERNEL.items()},
                       "routing": dict(sorted(rows.items()))}, f, indent=1)

    def load(self, path: str) -> int:
        """Install a saved routing: shapes it lists are never re-measured (shapes it does not list fall back to the built-in
        heuristic unless `measuring` is switched on again).  Returns the number of entries."""
        import json
        with open(path) as f:
            doc = json.load(f)
        _require(doc.get("format") == "nopesac_amd.ConvTuner/1", "not a ConvTuner routing file")
        self.loaded = {k: int(v) for k, v in doc["routing"].items()}
        return len(self.loaded)


TUNER = ConvTuner()
CFG_BFRAG3, CFG_BFRAG32 = _H.NPS_CONV_CFG_BFRAG3, _H.NPS_CONV_CFG_BFRAG32       # tuner-only configurations: nopesac_conv2d_nhwc_bfrag, K-tile 64 / 32
CFG_HALO16, CFG_HALO8 = _H.NPS_CONV_CFG_HALO16, _H.NPS_CONV_CFG_HALO8          # tuner-only: nopesac_conv3x3_halo_bf16, 16x16 / 16x8 pixel tiles
CFG_P8 = _H.NPS_CONV_CFG_P8             # tuner-only: nopesac_conv2d_nhwc_p8 (256x256x64 tiles, phase-interleaved 8-wave schedule)
CFG_P8N, CFG_P8N_TAP = _H.NPS_CONV_CFG_P8N, _H.NPS_CONV_CFG_P8N_TAP            # tuner-only: nopesac_conv2d_nhwc_p8n (256x128 tiles: the Cout % 128 == 0 layers, round 5), channel- / tap-major K order
CFG_P8N_SPLIT = _H.NPS_CONV_CFG_P8N_SPLIT                                    # tuner-only: nopesac_conv2d_nhwc_p8n_splitk (few tiles x long K: the pose net's first conv; round 6)
CFG_P8_SK = _H.NPS_CONV_CFG_P8_SK       # tuner-only: nopesac_conv2d_nhwc_p8_sk (the same kernel with stream-K work distribution, round 5)
# NOPESAC_P8_CAP_1X1=n (experiment, round 5): persistent workgroups of the p8 kernel on 1x1 layers (the HBM-bound ones) capped at n
P8_CAP_1X1 = [int(os.environ.get("NOPESAC_P8_CAP_1X1", "0"))]
P8_VARIANT = [32]                      # variant handed to nopesac_conv2d_nhwc_p8: 32 = channel-major K order (better L2 reuse of the taps)
# added to nopesac_conv2d_nhwc_bfrag's variant for stride-1 KxK convs: channel-major K order (round 4: same time in isolation, 95 instead
# of 149 MB read from HBM per launch on res3's 3x3 layers; stride 2 measured slower and stays tap-major).  NOPESAC_BFRAG_KMAJOR=0: A/B runs
BFRAG_KMAJOR = [0 if os.environ.get("NOPESAC_BFRAG_KMAJOR") == "0" else 256]
LAST_CONV_CFG = [0]                    # kernel configuration of the most recent conv2d launch (0 = the library's heuristic)
CONV_CFG_KERNEL = {1: "conv_igemm_kernel<128x128>", 2: "conv_igemm_kernel<64x64>", 3: "conv_igemm_glds_kernel<BK=64>", 4: "conv_igemm_glds_kernel<BK=32>",
                   7: "conv_igemm_bfrag_kernel<3, 64, false>", 8: "conv_igemm_bfrag_kernel<4, 32, false>", 9: "conv3x3_halo_kernel<16, 16>",
                   10: "conv3x3_halo_kernel<16, 8>", 11: "conv_igemm_p8_kernel", 12: "conv_igemm_p8_kernel<stream-K>",
                   13: "conv_igemm_p8n_kernel", 14: "conv_igemm_p8n_kernel<tap-major>", 15: "conv_igemm_p8n_kernel<split-K>"}
P8N_TUNABLE = [os.environ.get("NOPESAC_P8N", "1") != "0"]           # NOPESAC_P8N=0: the tuner never offers the 256x128-tile kernel (A/B runs)
P8_SK_TUNABLE = [os.environ.get("NOPESAC_P8_SK", "0") == "1"]      # NOPESAC_P8_SK=1: the tuner may pick the stream-K form (wins isolated launches, loses 1.2 % in the four-in-flight loop: profiles/r5_b_*)
_SCRATCH = {}                          # (device index, stream handle) -> the stream's scratch arena, f32 (grown on demand, never shrunk)
_P8_SK_WS = {}                         # (device index, stream handle) -> workspace tensor of the stream-K conv


def _stream_key(device) -> tuple:
    return (device.index if device.index is not None else torch.cuda.current_device(), _stream())


def scratch(device, nbytes: int) -> torch.Tensor:
    """The one place a kernel workspace comes from: f32, at least `nbytes` long (rounded up to whole floats), 16-byte aligned, content
    undefined.  For partials that one wrapper's launches write and then read, nothing else: no result and no state lives here.
    Not capturing: the ONE buffer of (device, current stream), whole - launches of one stream are ordered, so every op on it shares
    the buffer; it grows to the largest request and is kept.  A wrapper that needs two regions alive at once asks once and slices.
    Capturing: a fresh torch.empty from the capture's private pool, never cached, so that every captured graph owns its scratch - two
    graphs replayed side by side must not share one, and a stream handle (which torch hands out round-robin from a small pool) does not
    tell two captures apart."""
    n = (int(nbytes) + 3) // 4
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(n, device=device, dtype=torch.float32)
    key = _stream_key(device)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < n:
        buf = _SCRATCH[key] = torch.empty(n, device=device, dtype=torch.float32)
    return buf                          # (no view of n elements: the launchers take "at least", and a slice costs what a torch.empty did)


def p8_sk_workspace(device) -> torch.Tensor:
    """The stream-K conv's workspace for the CURRENT stream of `device` (arrival counters + partial-tile slabs, 128 MB).  Not scratch():
    its first 16 KB are STATE - arrival counters that must be zero on entry and that the kernel leaves zero - and any other user of the
    arena would scribble on them.  So it keeps a buffer of its own, zeroed once, under scratch()'s rule: one per (device, stream) outside
    a capture; inside one a fresh buffer with a fresh zero fill (harmlessly replayed) from the capture's private pool, never cached."""
    capturing = torch.cuda.is_current_stream_capturing()
    ws = None if capturing else _P8_SK_WS.get(_stream_key(device))
    if ws is None:
        ws = torch.empty(int(_C.nopesac_conv2d_p8_sk_workspace_bytes()), device=device, dtype=torch.uint8)
        ws[:16384].zero_()
        if not capturing:
            _P8_SK_WS[_stream_key(device)] = ws
    return ws


def _frag_weights(w: torch.Tensor) -> torch.Tensor:
    """Fragment-major copy of a conv weight [Cout,KH,KW,Cin], made once and kept ON the weight tensor object (packed weights
    are static and long-lived; an address-keyed cache would hand out stale fragments when a freed weight's memory is reused).
    `linear()` passes a fresh 4-D view of the packed matrix on every call: the copy then lives on the view's base tensor."""
    holder = w
    base = w._base
    if base is not None and base.numel() == w.numel() and base.storage_offset() == w.storage_offset() and base.is_contiguous():
        holder = base
    f = getattr(holder, "_nps_frag", None)
    if f is None:
        f = mfma_fragment_major(w.reshape(w.shape[0], -1))
        holder._nps_frag = f
    return f


ConvEligibility = namedtuple("ConvEligibility", "bfrag_ok halo_ok p8_ok p8_sk_ok p8n_ok p8n_splits p8n_split_ok")


@functools.lru_cache(maxsize=None)
def conv_eligibility(x_dtype, w_dtype, out_dtype, B, H, W, Cin, Cout, KH, KW, stride, pad, has_residual, x_cs, y_cs, r_cs, batched,
                     has_scale, has_bias, act, aligned) -> ConvEligibility:
    """Which tuner-only kernel configurations conv2d may offer for one call (no GPU; the library decides: nopesac_conv2d_nhwc_forms,
    whose predicates are also the entry points' argument checks).  `act` is conv2d's act word (ACT_RES_AFTER / ACT_BIAS_BATCHED
    included); `aligned`: every buffer the call touches (x, w, out, residual, scale, bias) is 16-byte aligned.  Memoised: conv2d asks
    on every launch."""
    splits = ctypes.c_int(0)
    forms = _C.nopesac_conv2d_nhwc_forms
    m = forms(_DT.get(x_dtype, -1), _DT.get(w_dtype, -1), _DT.get(out_dtype, -1), B, H, W, Cin, Cout, KH, KW, stride, pad, x_cs, y_cs, r_cs,
              bool(batched), bool(has_residual), bool(has_scale), bool(has_bias), act, bool(aligned), ctypes.byref(splits))
    _lib.check(min(m, 0), forms.__name__)             # the result is a value: the mask, or NPS_E_ARG
    return ConvEligibility(*(bool(m >> c & 1) for c in (CFG_BFRAG3, CFG_HALO16, CFG_P8, CFG_P8_SK, CFG_P8N)), splits.value,
                           bool(m >> CFG_P8N_SPLIT & 1))


def conv_tuner_extras(el: ConvEligibility, KH: int, KW: int) -> tuple:
    """The tuner-only configurations conv2d offers ConvTuner.choose on top of CANDIDATES (0-4), in the order it offers them."""
    return (((CFG_BFRAG3, CFG_BFRAG32) if el.bfrag_ok else ()) + ((CFG_HALO16, CFG_HALO8) if el.halo_ok else ())
            + ((CFG_P8,) if el.p8_ok else ()) + ((CFG_P8_SK,) if (el.p8_sk_ok and P8_SK_TUNABLE[0]) else ())
            + (((CFG_P8N,) + ((CFG_P8N_TAP,) if KH * KW > 1 else ())) if (el.p8n_ok and P8N_TUNABLE[0]) else ())
            + ((CFG_P8N_SPLIT,) if (el.p8n_split_ok and P8N_TUNABLE[0]) else ()))


def conv2d(x: torch.Tensor, w: torch.Tensor, scale=None, bias=None, residual=None, *, stride=1, pad=0, act=ACT_NONE,
           out: Optional[torch.Tensor] = None, out_dtype=None, x_channels: Optional[int] = None,
           batched_weights: bool = False) -> torch.Tensor:
    """NHWC conv / linear.  x: [B,H,W,Cx] (a channel slice view of a wider buffer is allowed: only the
    last-dim stride may exceed the channel count); w: [Cout,KH,KW,Cin] or [B,Cout,KH,KW,Cin] when
    `batched_weights`.  `out` may be a channel-slice view of a wider NHWC buffer."""
    _require(x.dim() == 4 and x.stride(3) == 1, 'argument check failed: x.dim() == 4 and x.stride(3) == 1')
    B, H, W, Cx = x.shape
    x_cs = x.stride(2)
    _require(x.stride(1) == W * x_cs and x.stride(0) == H * W * x_cs, "x must be pixel-dense NHWC")
    if batched_weights:
        _require(w.dim() == 5 and w.shape[0] == B and w.is_contiguous(), 'argument check failed: w.dim() == 5 and w.shape[0] == B and w.is_contiguous()')
        Cout, KH, KW, Cin = w.shape[1:]
        w_bs = Cout * KH * KW * Cin
    else:
        _require(w.dim() == 4 and w.is_contiguous(), 'argument check failed: w.dim() == 4 and w.is_contiguous()')
        Cout, KH, KW, Cin = w.shape
        w_bs = 0
    _require(Cin == (x_channels or Cx), (Cin, Cx))
    mixed = x.dtype == torch.float32 and w.dtype == torch.bfloat16     # f32 activations x bf16 weights
    _require(w.dtype == x.dtype or mixed, 'argument check failed: w.dtype == x.dtype or mixed')
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    out_dtype = out_dtype or (out.dtype if out is not None else x.dtype)
    if out is None:
        out = torch.empty((B, OH, OW, Cout), device=x.device, dtype=out_dtype)
    _require(out.shape == (B, OH, OW, Cout) and out.stride(3) == 1 and out.dtype == out_dtype, 'argument check failed: out.shape == (B, OH, OW, Cout) and out.stride(3) == 1 and out.dtype == out_dtype')
    y_cs = out.stride(2)
    _require(out.stride(1) == OW * y_cs and out.stride(0) == OH * OW * y_cs, 'argument check failed: out.stride(1) == OW * y_cs and out.stride(0) == OH * OW * y_cs')
    r_cs = 0
    if residual is not None:
        _require(residual.shape == out.shape and residual.dtype == out_dtype and residual.stride(3) == 1, 'argument check failed: residual.shape == out.shape and residual.dtype == out_dtype and residual.stride(3) == 1')
        r_cs = residual.stride(2)
    if batched_weights and bias is not None and bias.numel() == B * Cout and B > 1:
        act |= ACT_BIAS_BATCHED                                   # per-batch bias rows [B, Cout]
    for v in (scale, bias):
        if v is not None:
            _chk(v, torch.float32)
            _require(v.numel() == Cout or (v is bias and (act & ACT_BIAS_BATCHED)), 'argument check failed: v.numel() == Cout or (v is bias and (act & ACT_BIAS_BATCHED))')
    el = conv_eligibility(x.dtype, w.dtype, out_dtype, B, H, W, Cin, Cout, KH, KW, stride, pad, residual is not None, x_cs, y_cs, r_cs,
                          batched_weights, scale is not None, bias is not None, act,
                          all(t is None or t.data_ptr() % 16 == 0 for t in (x, w, out, residual, scale, bias)))
    p8n_splits = el.p8n_splits

    def launch(cfg):
        if cfg == CFG_P8N_SPLIT:
            ws = scratch(x.device, int(_C.nopesac_conv2d_p8n_splitk_workspace_bytes(p8n_splits, B * OH * OW, Cout)))
            _C.nopesac_conv2d_nhwc_p8n_splitk(_p(x), _p(w), _p(scale), _p(bias), _p(out), B, H, W, Cin, Cout, KH, KW, stride, pad, x_cs,
                                              y_cs, act, 32, p8n_splits, _p(ws), ws.numel() * 4, _stream())
            return
        if cfg in (CFG_P8N, CFG_P8N_TAP):
            _C.nopesac_conv2d_nhwc_p8n(_p(x), _p(w), _p(scale), _p(bias), _p(out), B, H, W, Cin, Cout, KH, KW, stride, pad, x_cs, y_cs,
                                       act, 32 if cfg == CFG_P8N else 0, _stream())
            return
        if cfg == CFG_P8_SK:
            ws = p8_sk_workspace(x.device)
            _C.nopesac_conv2d_nhwc_p8_sk(_p(x), _p(w), _p(scale), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout, KH, KW, stride,
                                         pad, x_cs, y_cs, r_cs, act, _DT[out_dtype], P8_VARIANT[0], _p(ws), ws.numel(), _stream())
            return
        if cfg == CFG_P8:
            _C.nopesac_conv2d_nhwc_p8(_p(x), _p(w), _p(scale), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout, KH, KW, stride,
                                      pad, x_cs, y_cs, r_cs, act, _DT[out_dtype],
                                      P8_VARIANT[0] | ((P8_CAP_1X1[0] << 8) if KH * KW == 1 else 0), _stream())
            return
        if cfg in (CFG_HALO16, CFG_HALO8):
            _C.nopesac_conv3x3_halo_bf16(_p(x), _p(_frag_weights(w)), _p(scale), _p(bias), _p(out), B, H, W, Cin, Cout, act,
                                         0 if cfg == CFG_HALO16 else 1, _stream())
            return
        if cfg in (CFG_BFRAG3, CFG_BFRAG32):
            _C.nopesac_conv2d_nhwc_bfrag(_p(x), _p(_frag_weights(w)), _p(scale), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout,
                                         KH, KW, stride, pad, x_cs, y_cs, r_cs, act, _DT[out_dtype],
                                         (3 if cfg == CFG_BFRAG3 else 32) + (BFRAG_KMAJOR[0] if (KH * KW > 1 and stride == 1) else 0), _stream())
            return
        _C.nopesac_conv2d_nhwc_ex(_p(x), _p(w), _p(scale), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout, KH, KW,
                                  stride, pad, x_cs, y_cs, r_cs, w_bs, act, 2 if mixed else _DT[x.dtype], _DT[out_dtype],
                                  cfg, _stream())

    cfg = 0
    if TUNER.measuring or TUNER.best or TUNER.loaded:
        # everything that decides which kernel configurations are eligible (bfrag_ok / halo_ok) is part of the key
        key = (x.dtype, w.dtype, out_dtype, B, H, W, Cin, Cout, KH, KW, stride, pad, residual is not None, x_cs, y_cs, w_bs != 0,
               scale is not None, bias is not None, act, el.bfrag_ok, el.halo_ok, el.p8_ok)
        cfg = TUNER.choose(key, launch, conv_tuner_extras(el, KH, KW))
    try:
        launch(cfg)
    except _lib.HipKernelError:
        if cfg == 0:
            raise
        TUNER.best[key] = cfg = 0      # a stale routing entry the entry point rejects for this shape: heuristic from now on
        launch(0)
    LAST_CONV_CFG[0] = cfg             # read by bench.py's per-launch timer to attribute the launch to a kernel
    return out


def _rows4d(t: torch.Tensor, width: int) -> torch.Tensor:
    """View `t` ([..., width]: contiguous, or a column slice of a contiguous wider buffer) as a
    [1,1,rows,width] NHWC tensor whose pixel stride is the buffer's row stride."""
    _require(t.stride(-1) == 1 and t.shape[-1] == width, 'argument check failed: t.stride(-1) == 1 and t.shape[-1] == width')
    rows = t.numel() // width
    rs = width if t.is_contiguous() else t.stride(-2)
    if t.dim() > 2 and not t.is_contiguous():
        for d in range(t.dim() - 2):     # leading dims must be dense multiples of the row stride
            _require(t.stride(d) == t.stride(d + 1) * t.shape[d + 1], "unsupported row layout")
    return torch.as_strided(t, (1, 1, rows, width), (rows * rs, rows * rs, rs, 1), t.storage_offset())


def linear(x: torch.Tensor, w: torch.Tensor, bias=None, *, act=ACT_NONE, residual=None, out=None, scale=None,
           out_dtype=None) -> torch.Tensor:
    """y = act((x @ w.T) * scale + bias + residual).  x [..., K] / out [..., N] / residual [..., N] may be
    column slices of wider row-major buffers (free concatenation); w [N, K] contiguous."""
    K = x.shape[-1]
    N = w.shape[0]
    y = conv2d(_rows4d(x, K), w.view(N, 1, 1, K), scale, bias, None if residual is None else _rows4d(residual, N), act=act,
               out=None if out is None else _rows4d(out, N), out_dtype=out_dtype)
    return out if out is not None else y.view(*x.shape[:-1], N)


def preprocess(images_nchw: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, cpad: int, out_dtype) -> torch.Tensor:
    x = _chk(images_nchw, torch.float32)
    B, C, H, W = x.shape
    y = torch.empty((B, H, W, cpad), device=x.device, dtype=out_dtype)
    _C.nopesac_preprocess_nchw_to_nhwc(_p(x), _p(y), _p(_chk(mean, torch.float32)), _p(_chk(std, torch.float32)), B, C, H, W,
                                       cpad, _DT[out_dtype], _stream())
    return y


def stem_fused(x: torch.Tensor, w224: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """bf16 conv7x7/s2 + BN + ReLU + maxpool3x3/s2 in one kernel.  x [B,H,W,4] bf16, w224 [64,224] bf16."""
    _chk(x, torch.bfloat16); _chk(w224, torch.bfloat16); _chk(scale, torch.float32); _chk(bias, torch.float32)
    B, H, W, C = x.shape
    _require(C == 4 and w224.shape == (64, 224), 'argument check failed: C == 4 and w224.shape == (64, 224)')
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (CH + 2 - 3) // 2 + 1, (CW + 2 - 3) // 2 + 1
    y = torch.empty((B, PH, PW, 64), device=x.device, dtype=torch.bfloat16)
    _C.nopesac_stem_fused_bf16(_p(x), _p(w224), _p(scale), _p(bias), _p(y), B, H, W, _stream())
    return y


def stem_fused_raw(images: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, w224: torch.Tensor, scale: torch.Tensor,
                   bias: torch.Tensor) -> torch.Tensor:
    """`preprocess` + `stem_fused` in one kernel: images f32 NCHW [B,3,H,W] (0-255), per-channel mean / std f32[3]."""
    _chk(images, torch.float32); _chk(mean, torch.float32); _chk(std, torch.float32)
    _chk(w224, torch.bfloat16); _chk(scale, torch.float32); _chk(bias, torch.float32)
    B, C, H, W = images.shape
    _require(C == 3 and mean.numel() == 3 and std.numel() == 3 and w224.shape == (64, 224), 'argument check failed: C == 3 and mean.numel() == 3 and std.numel() == 3 and w224.shape == (64, 224)')
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (CH + 2 - 3) // 2 + 1, (CW + 2 - 3) // 2 + 1
    y = torch.empty((B, PH, PW, 64), device=images.device, dtype=torch.bfloat16)
    _C.nopesac_stem_fused_raw_bf16(_p(images), _p(mean), _p(std), _p(w224), _p(scale), _p(bias), _p(y), B, H, W, _stream())
    return y


def stem_fused_raw_shifted(images: torch.Tensor, pad3: torch.Tensor, w224_folded: torch.Tensor, scale: torch.Tensor,
                           bias_folded: torch.Tensor) -> torch.Tensor:
    """The raw-image stem with the normalisation folded into weights / shift (see `fold_stem_normalisation`): the patch holds the
    pixel values minus 128, exact in bf16."""
    _chk(images, torch.float32); _chk(pad3, torch.float32); _chk(w224_folded, torch.bfloat16); _chk(scale, torch.float32); _chk(bias_folded, torch.float32)
    B, C, H, W = images.shape
    _require(C == 3 and pad3.numel() == 3 and w224_folded.shape == (64, 224), 'argument check failed: C == 3 and pad3.numel() == 3 and w224_folded.shape == (64, 224)')
    CH, CW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (CH + 2 - 3) // 2 + 1, (CW + 2 - 3) // 2 + 1
    y = torch.empty((B, PH, PW, 64), device=images.device, dtype=torch.bfloat16)
    _C.nopesac_stem_fused_raw_shifted_bf16(_p(images), _p(pad3), _p(w224_folded), _p(scale), _p(bias_folded), _p(y), B, H, W, _stream())
    return y


def fold_stem_normalisation(w_o773: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, mean: torch.Tensor, std: torch.Tensor):
    """Operands of `stem_fused_raw_shifted` from the stem's f32 weights [64,7,7,3] (o, kh, kw, c), its folded-BN scale / shift and the
    per-channel pixel mean / std:  sum_k w (v - mean) / std = sum_k (w / std) (v - 128) + sum_k (w / std) (128 - mean).
    -> (pad3 f32[3] = mean - 128, w224 bf16 [64,224] in the fused stem's (kh, kw padded to 8, c padded to 4) order, bias' f32[64])."""
    wd, m, s = w_o773.double(), mean.double().view(1, 1, 1, 3), std.double().view(1, 1, 1, 3)
    wf = wd / s
    const = (wf * (128.0 - m)).sum(dim=(1, 2, 3))
    w8 = w_o773.new_zeros(64, 7, 8, 4, dtype=torch.float32)
    w8[:, :, :7, :3] = wf.float()
    return ((mean.float() - 128.0).contiguous(), w8.reshape(64, 224).to(torch.bfloat16).contiguous(),
            (bias.double() + scale.double() * const).float().contiguous())


BOTTLENECK_TAIL_CONFIGS = {(64, 256, 0, 0), (64, 256, 64, 0), (64, 256, 128, 0), (64, 256, 0, 64), (64, 256, 64, 64),          # (C, C4, CN, C2)
                           (128, 512, 0, 0), (128, 512, 128, 0), (128, 512, 256, 0), (128, 512, 0, 256), (128, 512, 128, 256),
                           (256, 1024, 0, 0), (256, 1024, 256, 0), (256, 1024, 512, 0), (256, 1024, 0, 512), (256, 1024, 256, 512)}


def mfma_fragment_major(w2d: torch.Tensor) -> torch.Tensor:
    """[N,K] (N % 32 == 0, K % 16 == 0) -> same shape, re-ordered [N/32][K/16][2][32][8]: the order in which a wave's 64 lanes
    consume the matrix as v_mfma_f32_32x32x16_bf16 operands (lane = 32*(k%16 >= 8) + n%32 holds 8 consecutive k)."""
    N, K = w2d.shape
    _require(N % 32 == 0 and K % 16 == 0, 'argument check failed: N % 32 == 0 and K % 16 == 0')
    return w2d.view(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


def mlp_padded_k(N: int, K: int) -> int:
    """K as the chained-MLP kernel pads it (csrc/mlp_chain.hip: two K blocks of the layer's width class)."""
    q = 128 * (4 if N <= 256 else 2 if N <= 512 else 1)        # an even number of blocks of 64 * ksplit channels (ksplit = 4 / tiles per wave)
    return -(-K // q) * q


class MlpLayer:
    """One Linear of a chained MLP stack, packed for nopesac_mlp_chain_bf16: bf16 weights [Np, Kp] (zero padded, MFMA
    fragment-major), f32 bias [Np]."""
    __slots__ = ("w", "bias", "N", "K")

    def __init__(self, w2d: torch.Tensor, bias: Optional[torch.Tensor]):
        N, K = w2d.shape
        _require(N <= _lib.MLP_MAX_WIDTH, f"mlp_pack: N = {N} exceeds NOPESAC_MLP_MAX_WIDTH")
        Np, Kp = -(-N // 32) * 32, mlp_padded_k(N, K)
        wp = torch.zeros(Np, Kp, device=w2d.device, dtype=torch.bfloat16)
        wp[:N, :K] = w2d.to(torch.bfloat16)
        self.w = mfma_fragment_major(wp)
        self.bias = None
        if bias is not None:
            self.bias = torch.zeros(Np, device=w2d.device, dtype=torch.float32)
            self.bias[:N] = bias.float()
        self.N, self.K = N, K


def mlp_chain(x: torch.Tensor, layers, acts, outs, x_bcast: Optional[torch.Tensor] = None, rows_per: int = 1, restarts=None):
    """A stack of Linear(+bias)(+act) layers over the rows of x in ONE launch (bf16 MFMA operands, f32 activations: the rounding
    points of one ops.linear per layer).  x [rows, Kx] f32 (may be a column slice of a wider row-major buffer); x_bcast [P, Kb]:
    optional prefix columns shared by `rows_per` consecutive rows (row r reads x_bcast[r // rows_per]); layers: [MlpLayer];
    acts: [ACT_*] per layer; outs: per layer None or an f32 [rows, N] tensor (may be a column slice) that receives the layer's
    output - the last one is required.  restarts: per layer True if the layer starts a new stack over the SAME input rows."""
    _require(len(layers) == len(acts) == len(outs) and 1 <= len(layers) <= _lib.MLP_MAX_LAYERS, "mlp_chain: layers / acts / outs")
    _require(x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1, "mlp_chain: x must be f32 [rows, K] with unit column stride")
    rows = x.shape[0]
    c = _lib.MlpChain()
    c.x, c.x_ld, c.x_width = _p(x), x.stride(0), x.shape[1]
    c.xb, c.xb_ld, c.xb_width, c.xb_rows_per = None, 0, 0, 1
    if x_bcast is not None:
        _require(x_bcast.dtype == torch.float32 and x_bcast.dim() == 2 and x_bcast.stride(1) == 1 and rows_per >= 1
                 and x_bcast.shape[0] * rows_per >= rows, "mlp_chain: x_bcast")
        c.xb, c.xb_ld, c.xb_width, c.xb_rows_per = _p(x_bcast), x_bcast.stride(0), x_bcast.shape[1], rows_per
    c.rows, c.n_layers = rows, len(layers)
    for i, (l, a, o) in enumerate(zip(layers, acts, outs)):
        e = c.layers[i]
        e.w, e.bias, e.K, e.N, e.act = _p(l.w), _p(l.bias), l.K, l.N, a
        e.reserved = 1 if (restarts is not None and restarts[i]) else 0        # NOPESAC_MLP_RESTART: reads the chain input again
        e.out, e.out_ld = None, 0
        if o is not None:
            _require(o.dtype == torch.float32 and o.dim() == 2 and o.shape == (rows, l.N) and o.stride(1) == 1, "mlp_chain: out tensor")
            e.out, e.out_ld = _p(o), o.stride(0)
    _C.nopesac_mlp_chain_bf16(ctypes.byref(c), _stream())
    return outs[-1]


def mfma_fragment_major_fp8(w2d: torch.Tensor) -> torch.Tensor:
    """[N,K] one-byte elements (N % 32 == 0, K % 64 == 0) -> same shape, re-ordered [N/32][K/64][2][64][16]: the two 16-byte
    pieces h = 0, 1 that lane l = 32*half + n%32 feeds to v_mfma_f32_32x32x64_f8f6f4 hold k = kf*64 + 32*half + 16*h + 0..15."""
    N, K = w2d.shape
    _require(N % 32 == 0 and K % 64 == 0 and w2d.element_size() == 1, 'argument check failed: N % 32 == 0 and K % 64 == 0 and w2d.element_size() == 1')
    return w2d.view(N // 32, 32, K // 64, 2, 2, 16).permute(0, 2, 4, 3, 1, 5).contiguous().view(N, K)


FP8_MAX = 448.0            # largest finite e4m3fn


def quantize_weights_fp8(w: torch.Tensor):
    """Conv weight [Cout,KH,KW,Cin] (any float dtype) -> (fp8 fragment-major matrix [Cout, KH*KW*Cin], per-output-channel
    scale f32[Cout]) with w ~= w8 * scale[:, None]; symmetric, amax -> 448 per output channel."""
    w2 = w.reshape(w.shape[0], -1).float()
    sc = w2.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX
    w8 = (w2 / sc[:, None]).clamp(-FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)
    return mfma_fragment_major_fp8(w8), sc.contiguous()


def conv2d_fp8(x: torch.Tensor, w8frag: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, *, ksize: int, stride=1, pad=0,
               act=ACT_NONE, out_dtype=torch.bfloat16, residual=None, variant: int = 0) -> torch.Tensor:
    """fp8 (e4m3fn) NHWC conv on the K = 64 fp8 MFMA.  x [B,H,W,Cin] float8_e4m3fn, w8frag from `quantize_weights_fp8`
    ([Cout, k*k*Cin]); `scale` carries the de-quantisation (bn_scale * w_scale * x_scale).  variant 0 = by Cin."""
    _require(x.dtype == torch.float8_e4m3fn and w8frag.dtype == torch.float8_e4m3fn and x.is_contiguous() and w8frag.is_contiguous(), 'argument check failed: x.dtype == torch.float8_e4m3fn and w8frag.dtype == torch.float8_e4m3fn and x.is_contiguous() and w8frag.is_contiguous()')
    B, H, W, Cin = x.shape
    Cout = w8frag.shape[0]
    _require(w8frag.shape[1] == ksize * ksize * Cin, 'argument check failed: w8frag.shape[1] == ksize * ksize * Cin')
    _chk(scale, torch.float32); _chk(bias, torch.float32)
    OH = (H + 2 * pad - ksize) // stride + 1
    OW = (W + 2 * pad - ksize) // stride + 1
    out = torch.empty((B, OH, OW, Cout), device=x.device, dtype=out_dtype)
    if residual is not None:
        _chk(residual, out_dtype)
        _require(residual.shape == out.shape, 'argument check failed: residual.shape == out.shape')
    if not variant:
        variant = 3 if Cin % 128 == 0 else 32
    _C.nopesac_conv2d_nhwc_fp8(_p(x), _p(w8frag), _p(scale), _p(bias), _p(residual), _p(out), B, H, W, Cin, Cout, ksize, ksize,
                               stride, pad, Cin, Cout, Cout if residual is not None else 0, act, _DT[out_dtype], variant, _stream())
    return out


def _forms_by_id(ids: dict, count: int) -> tuple:
    """Form names in the order of their header ids, which must be exactly 0 .. count - 1 (count: the header's NPS_*_FORMS)."""
    _require(sorted(ids.values()) == list(range(count)), f"form ids {ids} are not 0 .. {count - 1}")
    return tuple(sorted(ids, key=ids.get))


# the kernel forms of the fused bottleneck tail, indexed by form id (NPS_TAIL_* of include/nopesac_hip.h)
TAIL_FORMS = _forms_by_id({"pw": _H.NPS_TAIL_PW, "rt4": _H.NPS_TAIL_RT4, "rt4_late": _H.NPS_TAIL_RT4_LATE, "rt4_proj": _H.NPS_TAIL_RT4_PROJ,
                           "rt4h": _H.NPS_TAIL_RT4H, "rt8": _H.NPS_TAIL_RT8, "stream": _H.NPS_TAIL_STREAM, "wide": _H.NPS_TAIL_WIDE},
                          _H.NPS_TAIL_FORMS)
# A/B switch bits of the default selection (NPS_TAIL_SW_*), by the environment variable that sets each
TAIL_SWITCHES = {"NOPESAC_TAIL_" + sw: getattr(_H, "NPS_TAIL_SW_" + sw) for sw in ("NO_RT4", "NO_RT8", "RT4_LATE", "NO_RT4H", "RT8_WIDE", "NO_STREAM")}


def bottleneck_tail_forms(C, C4, CN, C2, M, stride=1, same_res=False, switches=0):
    """(default form id or -1, bitmask of eligible form ids) of a bottleneck tail over M pixels (C2 = 0: identity block; same_res: the
    projection source has the output's height and width) under the NPS_TAIL_SW_* switch bits.  Host only: needs no GPU."""
    mask = ctypes.c_uint(0)
    form = _C.nopesac_bottleneck_tail_forms(C, C4, CN, C2, M, stride, int(bool(same_res)), switches, ctypes.byref(mask))
    return form, mask.value


def bottleneck_tail(b, w3, s3, b3, *, residual=None, x2=None, wsc=None, ssc=None, bsc=None, stride=1, w1=None, s1=None, b1=None,
                    o_fp8: bool = False, form=None, y=None, o=None):
    """Fused conv3 + shortcut + ReLU (+ the next block's conv1) of a bf16 bottleneck; returns (y, o or None).
    b [B,OH,OW,C]; residual [B,OH,OW,C4] or projection source x2 [B,H2,W2,C2] with wsc [C4,C2]; w1 [CN,C4].
    The weight matrices are expected in `mfma_fragment_major` order.  o_fp8: o is written as float8_e4m3fn.
    form: a TAIL_FORMS id to launch instead of the default selection (an ineligible one raises); y / o: contiguous output buffers
    to write instead of new ones."""
    _chk(b, torch.bfloat16); _chk(w3, torch.bfloat16)
    B, OH, OW, C = b.shape
    C4 = w3.shape[0]
    CN = 0 if w1 is None else w1.shape[0]
    C2 = 0 if x2 is None else x2.shape[3]
    _require((C, C4, CN, C2) in BOTTLENECK_TAIL_CONFIGS, (C, C4, CN, C2))
    if y is None:
        y = torch.empty((B, OH, OW, C4), device=b.device, dtype=torch.bfloat16)
    _chk(y, torch.bfloat16)
    _require(y.shape == (B, OH, OW, C4), 'argument check failed: y.shape == (B, OH, OW, C4)')
    o_dt = torch.float8_e4m3fn if o_fp8 else torch.bfloat16
    if CN and o is None:
        o = torch.empty((B, OH, OW, CN), device=b.device, dtype=o_dt)
    if CN:
        _chk(o, o_dt)
        _require(o.shape == (B, OH, OW, CN), 'argument check failed: o.shape == (B, OH, OW, CN)')
    else:
        _require(o is None, 'argument check failed: o is None without w1')
    if residual is not None:
        _chk(residual, torch.bfloat16)
        _require(residual.shape == y.shape, 'argument check failed: residual.shape == y.shape')
    if x2 is not None:
        _chk(x2, torch.bfloat16); _chk(wsc, torch.bfloat16)
    H2, W2 = (x2.shape[1], x2.shape[2]) if x2 is not None else (0, 0)
    args = (_p(b), _p(w3), _p(s3), _p(b3), _p(residual), _p(x2), _p(wsc), _p(ssc), _p(bsc), B, OH, OW, H2, W2, stride, C, C4, C2, _p(y),
            _p(w1), _p(s1), _p(b1), CN, _p(o), FP8 if o_fp8 else BF16)
    if form is None:
        _C.nopesac_bottleneck_tail_bf16_ex(*args, _stream())
    else:
        _C.nopesac_bottleneck_tail_bf16_form(*args, int(form), _stream())
    return y, o


def maxpool(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    _chk(x)
    B, H, W, C = x.shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    y = torch.empty((B, OH, OW, C), device=x.device, dtype=x.dtype)
    _C.nopesac_maxpool_nhwc(_p(x), _p(y), B, H, W, C, k, stride, pad, _DT[x.dtype], _stream())
    return y


def upsample2x_bilinear(x: torch.Tensor, addend=None, act=ACT_NONE) -> torch.Tensor:
    _chk(x)
    B, H, W, C = x.shape
    y = torch.empty((B, 2 * H, 2 * W, C), device=x.device, dtype=x.dtype)
    if addend is not None:
        _chk(addend, x.dtype)
        _require(addend.shape == y.shape, 'argument check failed: addend.shape == y.shape')
    _C.nopesac_upsample2x_bilinear_nhwc(_p(x), _p(addend), _p(y), B, H, W, C, act, _DT[x.dtype], _stream())
    return y


def upsample2x_nearest_add(x: torch.Tensor, lateral: torch.Tensor) -> torch.Tensor:
    _chk(x); _chk(lateral, x.dtype)
    B, H, W, C = x.shape
    _require(lateral.shape == (B, 2 * H, 2 * W, C), 'argument check failed: lateral.shape == (B, 2 * H, 2 * W, C)')
    y = torch.empty_like(lateral)
    _C.nopesac_upsample2x_nearest_add_nhwc(_p(x), _p(lateral), _p(y), B, H, W, C, _DT[x.dtype], _stream())
    return y


def groupnorm(x: torch.Tensor, gamma, beta, groups: int, eps: float, act=ACT_NONE) -> torch.Tensor:
    _chk(x)
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    ws = scratch(x.device, 4 * int(_C.nopesac_groupnorm_workspace_floats(B, groups)))
    _C.nopesac_groupnorm_nhwc(_p(x), _p(_chk(gamma, torch.float32)), _p(_chk(beta, torch.float32)), _p(y), B, H * W, C,
                              groups, eps, act, _DT[x.dtype], _p(ws), _stream())
    return y


def layernorm(x: torch.Tensor, gamma, beta, res=None, addend=None, eps=1e-5):
    """-> y (and y + addend if `addend` [rows_a, D] is given; row index taken modulo rows_a)."""
    _chk(x, torch.float32)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if addend is not None else None
    if res is not None:
        _chk(res, torch.float32)
        _require(res.shape == x.shape, 'argument check failed: res.shape == x.shape')
    a_rows = 0 if addend is None else _chk(addend, torch.float32).numel() // D
    _C.nopesac_layernorm(_p(x), _p(res), _p(_chk(gamma, torch.float32)), _p(_chk(beta, torch.float32)), _p(y),
                         _p(addend), a_rows, _p(y2), rows, D, eps, _stream())
    return (y, y2) if addend is not None else y


def layernorm_ex(x: torch.Tensor, gamma, beta, res=None, addend=None, eps=1e-5, want=("y",)):
    """LayerNorm with a chosen set of outputs: "y" (f32), "y16" (bf16 copy), "y2" (y + addend, f32), "y2_16" (bf16).
    Returns a dict with exactly the requested tensors (one launch)."""
    _chk(x, torch.float32)
    D = x.shape[-1]
    rows = x.numel() // D
    out = {k: torch.empty(x.shape, device=x.device, dtype=torch.bfloat16 if k.endswith("16") else torch.float32) for k in want}
    _require(set(want) <= {"y", "y16", "y2", "y2_16"} and want, 'argument check failed: set(want) <= {"y", "y16", "y2", "y2_16"} and want')
    if res is not None:
        _chk(res, torch.float32)
        _require(res.shape == x.shape, 'argument check failed: res.shape == x.shape')
    a_rows = 0 if addend is None else _chk(addend, torch.float32).numel() // D
    _require(addend is not None or not ({"y2", "y2_16"} & set(want)), 'argument check failed: addend is not None or not ({"y2", "y2_16"} & set(want))')
    _C.nopesac_layernorm_ex(_p(x), _p(res), _p(_chk(gamma, torch.float32)), _p(_chk(beta, torch.float32)), _p(out.get("y")),
                            _p(addend), a_rows, _p(out.get("y2")), _p(out.get("y16")), _p(out.get("y2_16")), rows, D, eps,
                            _stream())
    return out


def add_rows(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _chk(a, torch.float32); _chk(b, torch.float32)
    D = a.shape[-1]
    out = torch.empty_like(a)
    _C.nopesac_add_rows(_p(a), _p(b), _p(out), a.numel() // D, D, b.numel() // D, _stream())
    return out


def softmax_rows(x: torch.Tensor, out_dtype=None, pad_to: int = 0) -> torch.Tensor:
    """softmax over the last dim; with out_dtype (float32 / bfloat16) and / or pad_to > D the result is written into rows of
    max(D, pad_to) elements of that type, zero beyond D (one launch instead of softmax + zero fill + strided cast copy)."""
    _chk(x, torch.float32)
    D = x.shape[-1]
    out_dtype = out_dtype or torch.float32
    if out_dtype == torch.float32 and pad_to <= D:
        y = torch.empty_like(x)
        _C.nopesac_softmax_rows(_p(x), _p(y), x.numel() // D, D, _stream())
        return y
    ld = max(D, pad_to)
    y = torch.empty(x.shape[:-1] + (ld,), device=x.device, dtype=out_dtype)
    _C.nopesac_softmax_rows_pad(_p(x), _p(y), x.numel() // D, D, ld, _DT[out_dtype], _stream())
    return y


def cached_constant(cache: dict, key, make):
    """A read-only device tensor built once per key and shared by every later call ON ANY STREAM: the stream that builds it is waited
    for before the tensor is published, so that a batch on another stream can never read it half-written (the kernels that fill it
    are not ordered against other streams by anything else)."""
    t = cache.get(key)
    if t is None:
        t = make()
        first = t[0] if isinstance(t, tuple) else t
        if first.is_cuda and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(first.device).synchronize()
        cache[key] = t
    return t


def metric_rows(trans, rot, n1, n2, m, pair_idx0: int, t_err=None, r_err=None, nonfinite=None) -> torch.Tensor:
    """[B,16] f32 result rows of the runner (runner.metric_rows on a GPU): one launch."""
    _chk(trans, torch.float32); _chk(rot, torch.float32); _chk(n1, torch.int32); _chk(n2, torch.int32); _chk(m, torch.int32)
    B = trans.shape[0]
    _require(trans.shape == (B, 3) and rot.shape == (B, 4) and n1.numel() == B and n2.numel() == B and m.numel() == B, "metric_rows: shapes")
    for v in (t_err, r_err):
        if v is not None:
            _chk(v, torch.float32)
    if nonfinite is not None:
        _chk(nonfinite, torch.int32)
    rows = torch.empty(B, 16, device=trans.device, dtype=torch.float32)
    _C.nopesac_metric_rows(_p(trans), _p(rot), _p(n1), _p(n2), _p(m), _p(t_err), _p(r_err), _p(nonfinite), int(pair_idx0), _p(rows),
                           B, _stream())
    return rows


def concat_cols(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """[a | b] along the last dim of two contiguous f32 row tensors."""
    _chk(a, torch.float32); _chk(b, torch.float32)
    rows, Da, Db = a.shape[0], a.shape[-1], b.shape[-1]
    _require(a.dim() == 2 and b.dim() == 2 and b.shape[0] == rows, "concat_cols: [rows, Da], [rows, Db]")
    out = torch.empty(rows, Da + Db, device=a.device, dtype=torch.float32)
    _C.nopesac_concat_cols(_p(a), Da, _p(b), Db, _p(out), rows, _stream())
    return out


def add_rows_bf16(a: torch.Tensor, b: torch.Tensor):
    """(a as bf16, a + b as bf16), b broadcast over blocks of b.shape[0] rows; one launch."""
    _chk(a, torch.float32); _chk(b, torch.float32)
    D = a.shape[-1]
    a16 = torch.empty(a.shape, device=a.device, dtype=torch.bfloat16)
    ab16 = torch.empty(a.shape, device=a.device, dtype=torch.bfloat16)
    _C.nopesac_add_rows_bf16(_p(a), _p(b), _p(a16), _p(ab16), a.numel() // D, D, b.numel() // D, _stream())
    return a16, ab16


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, Lq: int, Lk: int, heads: int, scale: float,
              qlen=None, klen=None, mfma_bf16: bool = False) -> torch.Tensor:
    """q [B*Lq, >=heads*32] etc. as (possibly column-sliced) row-major matrices -> o [B*Lq, heads*32]."""
    io16 = q.dtype == torch.bfloat16          # bf16 q/k/v in memory -> bf16 o (MFMA kernel only)
    for t in (q, k, v):
        _require(t.is_cuda and t.dtype == q.dtype and t.dim() == 2 and t.stride(1) == 1, 'argument check failed: t.is_cuda and t.dtype == q.dtype and t.dim() == 2 and t.stride(1) == 1')
    _require(q.dtype == torch.float32 or (io16 and mfma_bf16), 'argument check failed: q.dtype == torch.float32 or (io16 and mfma_bf16)')
    _require(q.shape[0] == B * Lq and k.shape[0] == B * Lk and v.shape[0] == B * Lk, 'argument check failed: q.shape[0] == B * Lq and k.shape[0] == B * Lk and v.shape[0] == B * Lk')
    _lengths(qlen, B, "attention: qlen"); _lengths(klen, B, "attention: klen")
    o = torch.empty((B * Lq, heads * 32), device=q.device, dtype=q.dtype)
    fn = _C.nopesac_attention_small_bf16io if io16 else (_C.nopesac_attention_small_bf16 if mfma_bf16 else _C.nopesac_attention_small)
    fn(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0), B, Lq, Lk,
       heads, scale, _p(qlen), _p(klen), _stream())
    return o


def transpose_hw_rows(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    _chk(x, torch.float32)
    B, C = x.shape[0], x.shape[-1]
    y = torch.empty_like(x)
    _C.nopesac_transpose_hw_rows(_p(x), _p(y), B, H, W, C, _stream())
    return y


def count_nonfinite(tensors, counter: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32[1] device counter += number of Inf / NaN values in the given f32 tensors (no host synchronisation)."""
    if counter is None:
        counter = torch.zeros(1, device=tensors[0].device, dtype=torch.int32)
    tensors = [t for t in tensors if t.numel()]
    for i in range(0, len(tensors), _H.NOPESAC_NONFINITE_MAX_TENSORS):
        grp = tensors[i:i + _H.NOPESAC_NONFINITE_MAX_TENSORS]
        for t in grp:
            _chk(t, torch.float32)
        ptrs = (ctypes.c_void_p * len(grp))(*[_p(t) for t in grp])
        cnts = (ctypes.c_int64 * len(grp))(*[t.numel() for t in grp])
        _C.nopesac_count_nonfinite_batch(ptrs, cnts, len(grp), _p(counter), _stream())
    return counter


class HostFetch:
    """A batch of device tensors on its way to the host, on the stream that was current at construction.  Up to 16 MB: ONE kernel per
    32 tensors (`nopesac_gather_bytes`) stores their bytes straight into one pinned, device-mapped host buffer (16-byte aligned
    segments) - no concatenation, no pad fills, no copy node, so a captured graph / launch tape can hold the fetch.  Larger sets: one
    torch.cat on the device + one copy.  `views()` hands out host tensors of the original dtype / shape (views of that buffer) once the caller
    knows the fetch has completed - after `wait()`, or after an event it recorded behind the fetch on the same stream.
    private_views = True (a fetch recorded in a graph: the buffer is written again by every replay): views() snapshots the buffer.
    dynamic = {name: int64[1] device tensor}: only that many leading BYTES of the named tensor are valid (known on the device only); the
    rest of its host view is undefined.  Such a tensor does not count towards the 16 MB bound of the kernel path."""
    KERNEL_MAX_BYTES, KERNEL_MAX_SEGMENTS, ALIGN = 16 << 20, _H.NOPESAC_GATHER_MAX_SEGMENTS, 16
    _zero_pad = {}

    def __init__(self, tensors: dict, private_views: bool = False, dynamic: Optional[dict] = None, host: Optional[torch.Tensor] = None):
        dynamic = dynamic or {}
        dev = [(k, t.detach().contiguous()) for k, t in tensors.items() if t.is_cuda]
        self.passthrough = {k: t.detach() for k, t in tensors.items() if not t.is_cuda}
        self.spans, self.host, self.stream, self.private_views = {}, None, None, bool(private_views)
        if not dev:
            return
        off, segs, fixed = 0, [], 0
        for k, t in dev:
            nb = t.numel() * t.element_size()
            self.spans[k] = (off, nb, t.dtype, tuple(t.shape))
            if nb:
                segs.append((t, nb, off, dynamic.get(k)))
                fixed += 0 if k in dynamic else nb
            off += nb + (-nb) % self.ALIGN
        self.stream = torch.cuda.current_stream()
        if not segs:
            self.host = torch.empty(0, dtype=torch.uint8)
            return
        if fixed <= self.KERNEL_MAX_BYTES:
            # (the bytes between segments are never read; `host`: a pinned uint8 buffer the caller allocated - inside a stream capture
            #  nothing may be allocated on the host)
            if host is not None:
                _require(host.dtype == torch.uint8 and host.is_pinned() and host.numel() >= off, "HostFetch: host buffer too small / not pinned")
            self.host = host[:off] if host is not None else torch.empty(off, dtype=torch.uint8, pin_memory=True)
            for i in range(0, len(segs), self.KERNEL_MAX_SEGMENTS):
                grp = segs[i:i + self.KERNEL_MAX_SEGMENTS]
                n = len(grp)
                for _, _, _, dyn in grp:
                    if dyn is not None:
                        _chk(dyn, torch.int64)
                ptrs = (ctypes.c_void_p * n)(*[_p(t) for t, _, _, _ in grp])
                sizes = (ctypes.c_int64 * n)(*[nb for _, nb, _, _ in grp])
                dyns = (ctypes.c_void_p * n)(*[_p(dyn) for _, _, _, dyn in grp])
                offs = (ctypes.c_int64 * n)(*[o for _, _, o, _ in grp])
                _C.nopesac_gather_bytes(ptrs, sizes, dyns, offs, n, self.host.data_ptr(), _stream())
            self._keep = [(t, dyn) for t, _, _, dyn in segs]                     # sources stay allocated until the object goes
            return
        _require(host is None, "HostFetch: more than KERNEL_MAX_BYTES of fixed-size tensors cannot go into a caller-provided buffer")
        d0 = dev[0][1].device
        z = HostFetch._zero_pad.get(d0)
        if z is None:
            z = HostFetch._zero_pad[d0] = torch.zeros(self.ALIGN, device=d0, dtype=torch.uint8)
        parts = []
        for k, t in dev:
            nb = t.numel() * t.element_size()
            if nb:
                parts.append(t.view(-1).view(torch.uint8))
            if (-nb) % self.ALIGN:
                parts.append(z[:(-nb) % self.ALIGN])
        flat = torch.cat(parts)
        self.host = torch.empty(flat.numel(), dtype=torch.uint8, pin_memory=True)
        self.host.copy_(flat, non_blocking=True)

    def wait(self) -> "HostFetch":
        if self.stream is not None:
            self.stream.synchronize()
        return self

    def host_bytes(self) -> int:
        return 0 if self.host is None else int(self.host.numel())

    def views(self) -> dict:
        out = dict(self.passthrough)
        host = self.host
        if self.private_views and host is not None:
            # (a plain memcpy into pageable memory: .clone() of a pinned tensor allocates PINNED memory - a hipHostMalloc of ~10 ms
            #  whenever the results of earlier calls still hold the allocator's cached blocks - and torch's copy_ from a pinned source
            #  measured 1-30 ms per call where numpy's copy of the same bytes takes 50 us)
            host = torch.from_numpy(self.host.numpy().copy())
        for k, (o, n, dt, shape) in self.spans.items():
            out[k] = host[o:o + n].view(dt).view(shape)
        return out


def gather_to_host(tensors: dict) -> dict:
    """{name: tensor} -> {name: host tensor of the same dtype / shape}.  Device tensors travel together: one concatenation on the
    device, one copy into a fresh pinned host buffer, one wait; the returned tensors are views of that buffer."""
    return HostFetch(tensors).wait().views()


def u8_to_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 tensor -> float32 (exact), e.g. the image planes of a batch after an 8-bit host-to-device copy."""
    _chk(x, torch.uint8)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    _chk(out, torch.float32)
    _require(out.numel() == x.numel(), "u8_to_f32: sizes differ")
    _C.nopesac_u8_to_f32(_p(x), _p(out), x.numel(), _stream())
    return out


def clock_probe(spin_cycles: int = 400000, stream=None) -> torch.Tensor:
    """Enqueue the engine-clock probe (one wave, ~0.2 ms) on `stream` (default: current); returns an int64[2] device tensor
    (shader cycles, 100 MHz ticks) valid once the stream has passed it: MHz = 100 * t[0] / t[1]."""
    out = torch.zeros(2, device="cuda", dtype=torch.int64)
    _C.nopesac_clock_probe(_p(out), int(spin_cycles), stream.cuda_stream if stream is not None else _stream())
    return out


def normalize_rows(x: torch.Tensor, canonical_sign: bool = False) -> torch.Tensor:
    _chk(x, torch.float32)
    D = x.shape[-1]
    y = torch.empty_like(x)
    _C.nopesac_normalize_rows(_p(x), _p(y), x.numel() // D, D, int(canonical_sign), _stream())
    return y


def postselect_planes(cls_logits, mask_prob, params, query_feat, H, W, score_thr, mask_thr, overlap_thr, planar: bool = False) -> dict:
    """mask_prob: [B,h,w,nq], or [B,nq,h,w] when `planar`."""
    _chk(cls_logits, torch.float32); _chk(mask_prob, torch.float32); _chk(params, torch.float32); _chk(query_feat, torch.float32)
    B, nq, _ = cls_logits.shape
    if planar:
        _, nq2, h, w = mask_prob.shape
    else:
        _, h, w, nq2 = mask_prob.shape
    _require(nq2 == nq, 'argument check failed: nq2 == nq')
    D = query_feat.shape[-1]
    dev = cls_logits.device
    i32 = dict(device=dev, dtype=torch.int32)
    f32 = dict(device=dev, dtype=torch.float32)
    out = {
        "n_kept": torch.empty(B, **i32), "kept_idx": torch.empty(B, nq, **i32), "planes": torch.empty(B, nq, 3, **f32),
        "feats": torch.empty(B, nq, D, **f32), "scores": torch.empty(B, nq, **f32), "areas": torch.empty(B, nq, **i32),
        "centers": torch.empty(B, nq, 2, **f32), "winner": torch.zeros(B, H, W, device=dev, dtype=torch.uint8),
        "flags": torch.empty(B, **i32),
    }
    work = torch.empty(B, 9 * nq + 8, **i32)
    _C.nopesac_postselect_planes_ex(_p(cls_logits), _p(mask_prob), _p(params), _p(query_feat), B, nq, D, h, w, H, W,
                                    score_thr, mask_thr, overlap_thr, _p(out["n_kept"]), _p(out["kept_idx"]),
                                    _p(out["planes"]), _p(out["feats"]), _p(out["scores"]), _p(out["areas"]),
                                    _p(out["centers"]), _p(out["winner"]), _p(out["flags"]), _p(work), int(planar), _stream())
    return out


def matcher_sinkhorn(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, offset_mult, normal_mult, iters, match_thr):
    B, nq, _ = desc_dot.shape
    for t in (desc_dot, planes1, planes2, cam7, bin_score):
        _chk(t, torch.float32)
    _chk(n1, torch.int32); _chk(n2, torch.int32)
    log_scores = torch.empty(B, nq + 1, nq + 1, device=desc_dot.device, dtype=torch.float32)
    assignment = torch.empty(B, nq, nq, device=desc_dot.device, dtype=torch.float32)
    _C.nopesac_matcher_sinkhorn(_p(desc_dot), _p(planes1), _p(planes2), _p(cam7), _p(n1), _p(n2), _p(bin_score),
                                offset_mult, normal_mult, iters, match_thr, B, nq, _p(log_scores), _p(assignment), _stream())
    return log_scores, assignment


def geo_sequence(assignment, planes1, planes2, n1, n2, init_trans, init_rot, warp_in_ref=True):
    B, nq, _ = assignment.shape
    for t in (assignment, planes1, planes2, init_trans, init_rot):
        _chk(t, torch.float32)
    dev = assignment.device
    f32 = dict(device=dev, dtype=torch.float32)
    geo_local, geo_global = torch.empty(B, nq, 6, **f32), torch.empty(B, nq, 6, **f32)
    sig, geo_enc = torch.empty(B, nq, **f32), torch.empty(B, nq, 8, **f32)
    m = torch.empty(B, device=dev, dtype=torch.int32)
    _C.nopesac_geo_sequence(_p(assignment), _p(planes1), _p(planes2), _p(n1), _p(n2), _p(init_trans), _p(init_rot), B, nq,
                            int(warp_in_ref), _p(geo_local), _p(geo_global), _p(sig), _p(geo_enc), _p(m), _stream())
    return geo_local, geo_global, sig, geo_enc, m


def ransac_score_maps(geo_local, rot_raw, trans_raw, init_rot, init_trans, m, diagnostics=True):
    B, nq, _ = geo_local.shape
    for t in (geo_local, rot_raw, trans_raw, init_rot, init_trans):
        _chk(t, torch.float32)
    dev = geo_local.device
    f32 = dict(device=dev, dtype=torch.float32)
    out = {"rots_all": torch.empty(B, nq + 1, 4, **f32), "trans_all": torch.empty(B, nq + 1, 3, **f32),
           "normal_score": torch.empty(B, nq + 1, nq, **f32), "param_score": torch.empty(B, nq + 1, nq, **f32),
           "dn_sum": torch.empty(B, nq + 1, **f32), "dl2_sum": torch.empty(B, nq + 1, **f32)}
    if diagnostics:
        for k in ("l2_dist", "normal_angle", "offset_dist"):
            out[k] = torch.empty(B, nq + 1, nq, **f32)
    _C.nopesac_ransac_score_maps(_p(geo_local), _p(rot_raw), _p(trans_raw), _p(init_rot), _p(init_trans), _p(m), B, nq,
                                 _p(out["rots_all"]), _p(out["trans_all"]), _p(out["normal_score"]), _p(out["param_score"]),
                                 _p(out.get("l2_dist")), _p(out.get("normal_angle")), _p(out.get("offset_dist")),
                                 _p(out["dn_sum"]), _p(out["dl2_sum"]), _stream())
    return out


def ransac_soft_vote(sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat,
                     fused_rot, fused_trans, rots_w, rots_b, trans_w, trans_b, maps, init_rot, init_trans, m, mode: int):
    B, NH, _ = sf_rot.shape
    nq = NH - 1
    dev = sf_rot.device
    f32 = dict(device=dev, dtype=torch.float32)
    out = {"pred_rot": torch.empty(B, 4, **f32), "pred_trans": torch.empty(B, 3, **f32), "avg_rot": torch.empty(B, 4, **f32),
           "avg_trans": torch.empty(B, 3, **f32), "score_rot": torch.empty(B, NH, **f32), "score_trans": torch.empty(B, NH, **f32)}
    args = [sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot,
            fused_trans, rots_w, rots_b, trans_w, trans_b, maps["rots_all"], maps["trans_all"], maps["dn_sum"], maps["dl2_sum"],
            init_rot, init_trans]
    for t in args:
        _chk(t, torch.float32)
    _C.nopesac_ransac_soft_vote(*[_p(t) for t in args], _p(m), B, nq, mode, _p(out["pred_rot"]), _p(out["pred_trans"]),
                                _p(out["avg_rot"]), _p(out["avg_trans"]), _p(out["score_rot"]), _p(out["score_trans"]), _stream())
    return out


PLANE_CAM_REF_LOSS_NAMES = ("loss_tran_planeAvgReg", "loss_rot_planeAvgReg", "loss_tran_planeSoftReg", "loss_rot_planeSoftReg",
                            "loss_rotIdx", "loss_transIdx", "loss_paramL2_dist")


def plane_cam_ref_losses(vote: dict, maps: dict, m, gt_pose, weight: float = 1.0):
    """The seven refinement losses of the training-side twin (include/nopesac_hip.h: nopesac_plane_cam_ref_losses; reference
    camera_head.py:883-921) -> f32[7] in PLANE_CAM_REF_LOSS_NAMES order.  `vote` from ransac_soft_vote(mode | 16), `maps` from
    ransac_score_maps(diagnostics=True)."""
    _require("l2_dist" in maps, "plane_cam_ref_losses: ransac_score_maps must run with diagnostics=True (the parameter loss reads l2_dist)")
    B, NH, _ = maps["rots_all"].shape
    _chk(gt_pose, torch.float32)
    _require(tuple(gt_pose.shape) == (B, 7) and m.dtype == torch.int32 and m.numel() == B, "plane_cam_ref_losses: gt_pose [B,7], m int32[B]")
    args = [vote["pred_rot"], vote["pred_trans"], vote["avg_rot"], vote["avg_trans"], maps["rots_all"], maps["trans_all"],
            vote["score_rot"], vote["score_trans"], maps["l2_dist"]]
    for t in args:
        _chk(t, torch.float32)
    losses = torch.empty(7, device=gt_pose.device, dtype=torch.float32)
    _C.nopesac_plane_cam_ref_losses(*[_p(t) for t in args], _p(m), _p(gt_pose), B, NH - 1, float(weight), _p(losses), _stream())
    return losses


def camera_pose_loss(est_trans, est_rot, gt_trans, gt_rot, weight: float = 1.0, trans_eps: float = 0.0):
    """CameraPoseLoss / the AIM's reconstruction losses (include/nopesac_hip.h: nopesac_camera_pose_loss) -> f32[2] = (l_x, l_q) * weight.
    `gt_trans` / `gt_rot` may be column views of one [B,7] pose tensor (row strides are passed on)."""
    for t in (est_trans, est_rot):
        _chk(t, torch.float32)
    for t in (gt_trans, gt_rot):
        _chk(t, torch.float32, contiguous=False)
        _require(t.dim() == 2 and t.stride(1) == 1, "camera_pose_loss: gt rows must be dense")
    B = est_trans.shape[0]
    _require(tuple(est_trans.shape) == (B, 3) and tuple(est_rot.shape) == (B, 4) and tuple(gt_trans.shape) == (B, 3) and
             tuple(gt_rot.shape) == (B, 4), "camera_pose_loss: shapes")
    out = torch.empty(2, device=est_trans.device, dtype=torch.float32)
    _C.nopesac_camera_pose_loss(_p(est_trans), _p(est_rot), _p(gt_trans), gt_trans.stride(0), _p(gt_rot), gt_rot.stride(0), B,
                                float(trans_eps), float(weight), _p(out), _stream())
    return out


def refilter_assignment(assignment, planes1, planes2, n1, n2, rot, trans):
    B, nq, _ = assignment.shape
    out = torch.empty_like(assignment)
    _C.nopesac_refilter_assignment(_p(_chk(assignment, torch.float32)), _p(planes1), _p(planes2), _p(n1), _p(n2), _p(_chk(rot, torch.float32)),
                                   _p(_chk(trans, torch.float32)), B, nq, _p(out), _stream())
    return out


def force_k_select(logits: torch.Tensor, query_feat: torch.Tensor, perm: torch.Tensor, noise: torch.Tensor, B: int, K: int):
    """Benchmark-only K control in one launch (include/nopesac_hip.h: nopesac_force_k_select) -> feats f32 [2B,nq,D], n_kept int32 [2B]."""
    _chk(logits, torch.float32); _chk(query_feat, torch.float32); _chk(perm, torch.int64); _chk(noise, torch.float32)
    nq, n_cls, D = logits.shape[1], logits.shape[2], query_feat.shape[2]
    _require(logits.shape[0] >= B and query_feat.shape[0] >= B and query_feat.shape[1] == nq and perm.shape == (B, K) and noise.shape == (B, K, D),
             "force_k_select: shapes")
    feats = torch.empty(2 * B, nq, D, device=logits.device, dtype=torch.float32)
    n_kept = torch.empty(2 * B, device=logits.device, dtype=torch.int32)
    _C.nopesac_force_k_select(_p(logits), n_cls, _p(query_feat), _p(perm), _p(noise), B, nq, K, D, _p(feats), _p(n_kept), _stream())
    return feats, n_kept


def rle_labels(winner: torch.Tensor, kept_idx: torch.Tensor, n_kept: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """winner uint8 [V,H,W] -> column-major uint8 [V,W,H] map of kept-plane ordinals (0xFF = none)."""
    _chk(winner, torch.uint8); _chk(kept_idx, torch.int32); _chk(n_kept, torch.int32); _chk(flags, torch.int32)
    V, H, W = winner.shape
    labels = torch.empty((V, W, H), device=winner.device, dtype=torch.uint8)
    _C.nopesac_rle_labels(_p(winner), _p(kept_idx), _p(n_kept), _p(flags), _p(labels), V, H, W, kept_idx.shape[1],
                          _stream())
    return labels


def rle_transitions(labels: torch.Tensor, n_kept: torch.Tensor, nq: int, offsets: torch.Tensor = None,
                    positions: torch.Tensor = None) -> torch.Tensor:
    """counts int32 [V,nq] of mask flips per (view, plane); with offsets (int64 [V,nq]) + positions (int32 buffer) also
    writes the ascending flip positions."""
    _chk(labels, torch.uint8); _chk(n_kept, torch.int32)
    V, W, H = labels.shape
    counts = torch.empty((V, nq), device=labels.device, dtype=torch.int32)
    if positions is not None:
        _chk(offsets, torch.int64); _chk(positions, torch.int32)
    _C.nopesac_rle_transitions(_p(labels), _p(n_kept), _p(offsets) if positions is not None else None, _p(counts),
                               _p(positions) if positions is not None else None, V, W * H, nq, _stream())
    return counts


def decode_masks(winner: torch.Tensor, kept_idx: torch.Tensor, n_kept: torch.Tensor, flags: torch.Tensor, total: int) -> torch.Tensor:
    """bool [total, H, W]: the dense masks of every kept plane of every view, view after view (total = sum(n_kept), known to the
    caller); one launch for the whole batch."""
    _chk(winner, torch.uint8); _chk(kept_idx, torch.int32); _chk(n_kept, torch.int32); _chk(flags, torch.int32)
    V, H, W = winner.shape
    n64 = n_kept.to(torch.int64)
    offsets = (torch.cumsum(n64, 0) - n64).contiguous()
    masks = torch.empty((max(total, 1), H, W), device=winner.device, dtype=torch.uint8)
    _C.nopesac_decode_masks(_p(winner), _p(kept_idx), _p(n_kept), _p(flags), _p(offsets), _p(masks), V, H, W, kept_idx.shape[1],
                            _stream())
    return masks[:total].view(torch.bool)


def rle_compress(positions: torch.Tensor, offsets: torch.Tensor, counts: torch.Tensor, H: int, W: int):
    """Flip positions of n masks (device: positions int32 buffer, offsets int64 [n], counts int32 [n]) -> COCO counts strings on
    the device: (bytes uint8 [total], out_off int64 [n], lens int32 [n], bbox float64 [n,4]) - all device tensors; one host
    sync inside (the total string length sizes the byte buffer)."""
    _chk(positions, torch.int32); _chk(offsets, torch.int64); _chk(counts, torch.int32)
    n = counts.numel()
    dev = counts.device
    lens = torch.empty(n, device=dev, dtype=torch.int32)
    bbox = torch.empty(n, 4, device=dev, dtype=torch.float64)
    _C.nopesac_rle_compress_device(_p(positions), _p(offsets), _p(counts), n, H, W, _p(lens), _p(bbox), None, None, _stream())
    ends = torch.cumsum(lens.to(torch.int64), 0)
    out_off = (ends - lens).contiguous()
    total = int(ends[-1].item())                                         # host sync
    out = torch.empty(max(total, 1), device=dev, dtype=torch.uint8)
    _C.nopesac_rle_compress_device(_p(positions), _p(offsets), _p(counts), n, H, W, None, None, _p(out), _p(out_off), _stream())
    return out[:total], out_off, lens, bbox


def rle_compress_capped(positions: torch.Tensor, offsets: torch.Tensor, counts: torch.Tensor, H: int, W: int, cap: int):
    """rle_compress without the host sync: the strings go into a byte buffer of FIXED capacity `cap`; a string that would cross it
    is not written.  Returns (bytes uint8 [cap], out_off int64 [n], lens int32 [n], bbox float64 [n,4], total int64 [1]) - device
    tensors; the caller checks out_off[-1] + lens[-1] (= total) <= cap once those have reached the host."""
    _chk(positions, torch.int32); _chk(offsets, torch.int64); _chk(counts, torch.int32)
    n = counts.numel()
    dev = counts.device
    lens = torch.empty(n, device=dev, dtype=torch.int32)
    bbox = torch.empty(n, 4, device=dev, dtype=torch.float64)
    _C.nopesac_rle_compress_device(_p(positions), _p(offsets), _p(counts), n, H, W, _p(lens), _p(bbox), None, None, _stream())
    ends = torch.cumsum(lens.to(torch.int64), 0)
    out_off = (ends - lens).contiguous()
    out = torch.empty(int(cap), device=dev, dtype=torch.uint8)
    _C.nopesac_rle_compress_device_capped(_p(positions), _p(offsets), _p(counts), n, H, W, _p(lens), _p(out), _p(out_off), int(cap),
                                          _stream())
    return out, out_off, lens, bbox, ends[-1:]


# ---- plane AP evaluator (csrc/plane_eval.hip): RLE strings -> runs -> bit masks -> IoU -> true-positive assignment
PLANE_AP_COLS = ("score", "label", "tp_mask", "tp_plane", "tp_normal", "tp_offset", "normal_err_deg", "offset_err", "best_iou", "gt_id")
assert len(PLANE_AP_COLS) == _H.NPS_PLANE_AP_COLS       # the names of the row the header sizes


def _or_dummy(t: torch.Tensor, n: int = 1) -> torch.Tensor:
    """t, or n zeros in its place when it is empty: the library still wants a buffer to point at."""
    return t if t.numel() else torch.zeros(n, device=t.device, dtype=t.dtype)


def rle_string_runs(data: torch.Tensor, str_off: torch.Tensor):
    """Compressed COCO counts strings, concatenated (data uint8 [total], str_off int64 [n+1]) -> (runs int32 [total], n_runs int32 [n]):
    mask i's run lengths are runs[str_off[i] : str_off[i] + n_runs[i]] (a mask never has more runs than bytes)."""
    _chk(data, torch.uint8); _chk(str_off, torch.int64)
    n = str_off.numel() - 1
    _require(n >= 0, "rle_string_runs: str_off holds n + 1 offsets")
    data = _or_dummy(data)                      # only 0-byte strings
    runs = torch.empty(max(data.numel(), 1), device=data.device, dtype=torch.int32)
    n_runs = torch.empty(n, device=data.device, dtype=torch.int32)
    _C.nopesac_rle_string_runs(_p(data), _p(str_off), n, _p(runs), _p(n_runs), _stream())
    return runs, n_runs


def rle_runs_to_bits(runs: torch.Tensor, run_off: torch.Tensor, n_runs: torch.Tensor, H: int, W: int, bits: torch.Tensor = None):
    """Run lengths (runs int32, run_off int64 [n+1], n_runs int32 [n]) -> (bits uint32-as-int32 [n, ceil(H W / 32)], area int32 [n],
    bad int32 [n]).  bad[i] = 1 (words zero): a negative run, or runs that do not cover exactly H W pixels.  bits: a caller's buffer
    of at least n rows."""
    _chk(runs, torch.int32); _chk(run_off, torch.int64); _chk(n_runs, torch.int32)
    n, words = n_runs.numel(), (H * W + 31) // 32
    _require(run_off.numel() == n + 1, "rle_runs_to_bits: run_off holds n + 1 offsets")
    dev = runs.device
    runs = _or_dummy(runs)                      # only masks without a run (all bad)
    if bits is None:
        bits = torch.empty((max(n, 1), words), device=dev, dtype=torch.int32)[:n]
    else:
        _chk(bits, torch.int32)
        _require(bits.numel() >= n * words, "rle_runs_to_bits: bits buffer too small")
    starts = torch.empty(max(runs.numel(), 1), device=dev, dtype=torch.int32)
    area = torch.empty(n, device=dev, dtype=torch.int32)
    bad = torch.empty(n, device=dev, dtype=torch.int32)
    _C.nopesac_rle_runs_to_bits(_p(runs), _p(run_off), _p(n_runs), n, H, W, _p(starts), _p(bits), _p(area), _p(bad), _stream())
    return bits, area, bad


def poly_to_bits(xy: torch.Tensor, poly_off: torch.Tensor, mask_off: torch.Tensor, H: int, W: int, bits: torch.Tensor = None):
    """COCO polygons (xy float64 [2 * points], x first; poly_off int64 [polygons + 1] in points; mask_off int64 [n + 1] in polygons)
    -> (bits uint32-as-int32 [n, ceil(H W / 32)], area int32 [n], bad int32 [n]), the layout of rle_runs_to_bits: cocoapi's
    rleFrPoly + merge, bit for bit.  bad[i] = 1 (words zero): no polygon, a polygon of fewer than 3 points, a coordinate that is not
    finite or too large, more boundary points than the header's cap.  bits: a caller's buffer of at least n rows."""
    _chk(xy, torch.float64); _chk(poly_off, torch.int64); _chk(mask_off, torch.int64)
    n, n_polys, words = mask_off.numel() - 1, poly_off.numel() - 1, (H * W + 31) // 32
    _require(n >= 0 and n_polys >= 0 and xy.numel() % 2 == 0, "poly_to_bits: mask_off / poly_off hold n + 1 offsets, xy holds pairs")
    dev = mask_off.device
    n_points = xy.numel() // 2
    xy = _or_dummy(xy, 2)                       # only masks without a point (all bad)
    if bits is None:
        bits = torch.empty((max(n, 1), words), device=dev, dtype=torch.int32)[:n]
    else:
        _chk(bits, torch.int32)
        _require(bits.numel() >= n * words, "poly_to_bits: bits buffer too small")
    toggles = torch.empty((max(n, 1), words), device=dev, dtype=torch.int32)
    area = torch.empty(n, device=dev, dtype=torch.int32)
    bad = torch.empty(n, device=dev, dtype=torch.int32)
    _C.nopesac_poly_to_bits(_p(xy), _p(poly_off), _p(mask_off), n_points, n_polys, n, H, W, _p(toggles), _p(bits), _p(area), _p(bad),
                            _stream())
    return bits, area, bad


def mask_iou_bits(dt_bits, dt_area, dt_off, gt_bits, gt_area, gt_off, iscrowd, iou_off, total: int, max_dt: int, max_gt: int):
    """Pairwise mask IoU of V views in one launch: view v's predictions are rows dt_off[v]:dt_off[v+1] of dt_bits, its GT masks rows
    gt_off[v]:gt_off[v+1] of gt_bits (iscrowd uint8 per GT mask or None) -> (iou float64 [total], inter int32 [total]), view v's
    [n_dt, n_gt] block at iou_off[v].  total = iou_off[V]; max_dt / max_gt: the largest per-view counts (the caller has them)."""
    for t in (dt_bits, dt_area, gt_bits, gt_area):
        _chk(t, torch.int32)
    for t in (dt_off, gt_off, iou_off):
        _chk(t, torch.int64)
    if iscrowd is not None:
        _chk(iscrowd, torch.uint8)
    V = dt_off.numel() - 1
    _require(gt_off.numel() == V + 1 and iou_off.numel() == V + 1 and dt_bits.dim() == 2 and gt_bits.dim() == 2
             and dt_bits.shape[1] == gt_bits.shape[1], "mask_iou_bits: shapes")
    dev = dt_bits.device
    iou = torch.zeros(max(total, 1), device=dev, dtype=torch.float64)
    inter = torch.zeros(max(total, 1), device=dev, dtype=torch.int32)
    _C.nopesac_mask_iou_bits(_p(dt_bits), _p(dt_area), _p(dt_off), _p(gt_bits), _p(gt_area), _p(gt_off), _p(iscrowd), _p(iou_off), V,
                             max(dt_bits.shape[1], 1), max_dt, max_gt, _p(iou), _p(inter), _stream())
    return iou[:total], inter[:total]


def plane_ap_assign(iou, iou_off, dt_off, gt_off, score, pred_label, pred_plane, gt_label, gt_plane, max_dt: int, max_gt: int,
                    iou_thresh: float, normal_thresh: float, offset_thresh: float) -> torch.Tensor:
    """The reference's score-ordered true-positive assignment (mp3d_evaluation.py:570-649) for V views in one launch ->
    rows float64 [n_pred, 10] (PLANE_AP_COLS), in the predictions' own order."""
    _chk(iou, torch.float64); _chk(score, torch.float32); _chk(pred_label, torch.int32); _chk(pred_plane, torch.float32)
    _chk(gt_label, torch.int32); _chk(gt_plane, torch.float32)
    for t in (iou_off, dt_off, gt_off):
        _chk(t, torch.int64)
    V, n = dt_off.numel() - 1, score.numel()
    _require(gt_off.numel() == V + 1 and iou_off.numel() == V + 1 and pred_label.numel() == n and pred_plane.numel() == 3 * n
             and gt_plane.numel() == 3 * gt_label.numel(), "plane_ap_assign: shapes")
    rows = torch.full((n, len(PLANE_AP_COLS)), float("nan"), device=score.device, dtype=torch.float64)
    _C.nopesac_plane_ap_assign(_p(iou), _p(iou_off), _p(dt_off), _p(gt_off), _p(score), _p(pred_label), _p(pred_plane), _p(gt_label),
                               _p(gt_plane), V, max_dt, max_gt, float(iou_thresh), float(normal_thresh), float(offset_thresh), _p(rows),
                               _stream())
    return rows


# ---- two-view reconstruction AP (csrc/recon_eval.hip): planes of both views in one frame, merged entries, errors, true positives
RECON_AP_COLS = ("score", "tp_all", "tp_no_offset", "tp_no_normal", "tp_no_mask", "tp_no_normal_offset", "index0", "index1")
assert len(RECON_AP_COLS) == _H.NPS_RECON_AP_COLS       # the names of the row the header sizes


def recon_ap_assign(iou, iou_off, dt_off, gt_off, score, pred_plane, gt_plane, pred_cam, gt_cam, pred_corr, pred_corr_off, gt_corr,
                    gt_corr_off, n_rows: int, max_dt: int, max_gt: int, err_off=None, err_total: int = 0):
    """The per-pair part of the reference's `eval.py --evaluate AP` for P pairs in one launch (include/nopesac_hip.h states the
    rules).  Views 2 i and 2 i + 1 of iou_off / dt_off / gt_off (int64 [2 P + 1]) are pair i's; pred_cam / gt_cam float64 [P, 7]
    (position, quaternion wxyz); pred_corr / gt_corr int32 [., 2] with int64 offsets [P + 1].  n_rows = number of predictions - number
    of predicted correspondences (the caller has both).  Returns (rows float64 [n_rows, 8] (RECON_AP_COLS), n_gt_entries int32 [P],
    bad int32 [P]); a bad pair's rows stay zero.  err_off (int64 [P + 1]) with err_total: also the three error matrices of every
    pair, flat float64 [err_total], pair i's [3, entries, GT entries] block at err_off[i] - a fourth result."""
    _chk(iou, torch.float64); _chk(score, torch.float32); _chk(pred_plane, torch.float32); _chk(gt_plane, torch.float32)
    _chk(pred_cam, torch.float64); _chk(gt_cam, torch.float64); _chk(pred_corr, torch.int32); _chk(gt_corr, torch.int32)
    for t in (iou_off, dt_off, gt_off, pred_corr_off, gt_corr_off):
        _chk(t, torch.int64)
    P, n = pred_corr_off.numel() - 1, score.numel()
    _require(P >= 0 and dt_off.numel() == 2 * P + 1 and gt_off.numel() == 2 * P + 1 and iou_off.numel() == 2 * P + 1
             and gt_corr_off.numel() == P + 1 and pred_cam.numel() == 7 * P and gt_cam.numel() == 7 * P and pred_plane.numel() == 3 * n
             and gt_plane.numel() % 3 == 0 and pred_corr.numel() % 2 == 0 and gt_corr.numel() % 2 == 0 and 0 <= n_rows <= n,
             "recon_ap_assign: shapes")
    dev = pred_cam.device
    iou = _or_dummy(iou)                        # no view with both predictions and GT
    rows = torch.zeros((n_rows, len(RECON_AP_COLS)), device=dev, dtype=torch.float64)
    n_gt_entries = torch.zeros(P, device=dev, dtype=torch.int32)
    bad = torch.zeros(P, device=dev, dtype=torch.int32)
    errs = None
    if err_off is not None:
        _chk(err_off, torch.int64)
        _require(err_off.numel() == P + 1 and err_total >= 0, "recon_ap_assign: err_off holds P + 1 offsets")
        errs = torch.zeros(max(err_total, 1), device=dev, dtype=torch.float64)
    _C.nopesac_recon_ap_assign(_p(iou), _p(iou_off), _p(dt_off), _p(gt_off), _p(score), _p(pred_plane), _p(gt_plane), _p(pred_cam),
                               _p(gt_cam), _p(pred_corr), _p(pred_corr_off), _p(gt_corr), _p(gt_corr_off), P, max_dt, max_gt, int(n_rows),
                               _p(rows), _p(n_gt_entries), _p(bad), _p(errs), _p(err_off), _stream())
    return (rows, n_gt_entries, bad) if errs is None else (rows, n_gt_entries, bad, errs[:err_total])


# ---- the reconstruction as meshes (csrc/recon_mesh.hip): merged plane parameters, vertex / face counts, the fill
MESH_LDS_WORDS = _H.NPS_MESH_LDS_WORDS


def mesh_lds_words(H: int, W: int, stride: int) -> int:
    """LDS words a workgroup of recon_mesh_count / _fill needs for an H x W mask at `stride` (the header states the formula)."""
    hs, ws = -(-H // stride), -(-W // stride)
    return hs * (-(-ws // 32) | 1) + 2 * (hs + 1)


def _mesh_mask_args(who: str, bits, H: int, W: int, stride: int) -> int:
    _require(H > 0 and W > 0 and H * W <= 0x7fffffdf, f"{who}: H, W > 0 and H W < 2^31 - 32")
    _require(stride >= 1, f"{who}: stride >= 1 (got {stride})")
    _require(mesh_lds_words(H, W, stride) <= MESH_LDS_WORDS,
             f"{who}: a {H} x {W} mask at stride {stride} needs {mesh_lds_words(H, W, stride)} LDS words, NPS_MESH_LDS_WORDS is {MESH_LDS_WORDS}")
    _chk(bits, torch.int32)
    words = (H * W + 31) // 32
    _require(bits.dim() == 2 and (bits.shape[0] == 0 or bits.shape[1] == words), f"{who}: bits is int32 [n, ceil(H W / 32)]")
    return bits.shape[0]


def recon_mesh_merge(planes, view_off, cams, corr, corr_off, max_n: int):
    """merge_plane_params_from_local_params for P pairs in one launch (include/nopesac_hip.h states the rules): planes f32 [total, 3],
    view_off int64 [2 P + 1] (pair i owns views 2 i and 2 i + 1), cams float64 [P, 7] (position, quaternion wxyz), corr int32 [., 2]
    with corr_off int64 [P + 1]; max_n: the largest per-view plane count (the caller has it).  Returns (merged float64 [total, 3],
    bad int32 [P]); a bad pair's planes stay zero."""
    _require(0 <= max_n <= PLANE_MAX_QUERIES, f"recon_mesh_merge: at most {PLANE_MAX_QUERIES} planes per view (got {max_n})")
    _chk(planes, torch.float32); _chk(view_off, torch.int64); _chk(cams, torch.float64); _chk(corr, torch.int32); _chk(corr_off, torch.int64)
    P, total = corr_off.numel() - 1, planes.numel() // 3
    _require(P >= 0 and view_off.numel() == 2 * P + 1 and cams.numel() == 7 * P and planes.numel() == 3 * total and corr.numel() % 2 == 0,
             "recon_mesh_merge: shapes")
    dev = cams.device
    merged = torch.zeros((total, 3), device=dev, dtype=torch.float64)
    bad = torch.zeros(P, device=dev, dtype=torch.int32)
    corr = _or_dummy(corr, 2)                   # no correspondence at all
    _C.nopesac_recon_mesh_merge(_p(planes) if total else None, _p(view_off), _p(cams), _p(corr), _p(corr_off), P, int(max_n), total,
                                _p(merged) if total else None, _p(bad), _stream())
    return merged, bad


def recon_mesh_count(bits, H: int, W: int, stride: int = 1):
    """Per instance (bits int32 [n, ceil(H W / 32)], the layout of rle_runs_to_bits) -> (n_vert int32 [n], n_face int32 [n]) of the
    dense mesh of the mask m[::stride, ::stride]."""
    n = _mesh_mask_args("recon_mesh_count", bits, H, W, stride)
    n_vert = torch.empty(n, device=bits.device, dtype=torch.int32)
    n_face = torch.empty(n, device=bits.device, dtype=torch.int32)
    _C.nopesac_recon_mesh_count(_p(bits), n, H, W, stride, _p(n_vert), _p(n_face), _stream())
    return n_vert, n_face


def recon_mesh_fill(bits, H: int, W: int, stride: int, planes, inst_view, kinv, cams, vert_off, face_off, n_verts: int, n_faces: int):
    """The dense meshes of n instances in one launch: planes float64 [n, 3] (each in its view's frame), inst_view int32 [n] indexing
    kinv float64 [V, 9] and cams float64 [V, 7], vert_off / face_off int64 [n + 1] (exclusive scans of recon_mesh_count's counts) with
    their totals n_verts / n_faces.  Returns (verts f32 [n_verts, 3], uvs f32 [n_verts, 2], faces int32 [n_faces, 3], bad int32 [n])."""
    n = _mesh_mask_args("recon_mesh_fill", bits, H, W, stride)
    _require(n_verts >= 0 and n_faces >= 0, "recon_mesh_fill: n_verts, n_faces >= 0")
    _chk(planes, torch.float64); _chk(inst_view, torch.int32); _chk(kinv, torch.float64); _chk(cams, torch.float64)
    _chk(vert_off, torch.int64); _chk(face_off, torch.int64)
    V = kinv.numel() // 9
    _require(planes.numel() == 3 * n and inst_view.numel() == n and kinv.numel() == 9 * V and cams.numel() == 7 * V
             and vert_off.numel() == n + 1 and face_off.numel() == n + 1, "recon_mesh_fill: shapes")
    dev = bits.device
    verts = torch.empty((n_verts, 3), device=dev, dtype=torch.float32)
    uvs = torch.empty((n_verts, 2), device=dev, dtype=torch.float32)
    faces = torch.empty((n_faces, 3), device=dev, dtype=torch.int32)
    bad = torch.zeros(n, device=dev, dtype=torch.int32)
    _C.nopesac_recon_mesh_fill(_p(bits), n, H, W, stride, _p(planes), _p(inst_view), V, _p(kinv), _p(cams), _p(vert_off), _p(face_off),
                               int(n_verts), int(n_faces), _p(verts) if n_verts else None, _p(uvs) if n_verts else None,
                               _p(faces) if n_faces else None, _p(bad), _stream())
    return verts, uvs, faces, bad


GNN_PREFETCH =os.environ.get("NOPESAC_GNN_PREFETCH", "1") != "0"


def gnn_layer(x: torch.Tensor, x_off: int, src: torch.Tensor, src_off: int, out: torch.Tensor, out_off: int, n_sets: int, lens, W: dict,
              W_next: Optional[dict] = None, next_sets: int = 0):
    """One fused GNN layer (csrc/gnn_layer.hip): x/src/out f32 [sets, nq, 256]; lens int32 [sets] (indexed like x / src);
    W: fragment-major bf16 weights "wq" (pre-scaled), "wk", "wv", "wm", "w0", "w2" and f32 "g1", "b1", "g2", "b2".
    W_next / next_sets: the weights and the set count of the NEXT launch - with few plane sets (one pair per call) extra workgroups
    of this launch read them into the L2s the next launch will run on (nopesac_gnn_layer_bf16_pf)."""
    for t in (x, src, out):
        _chk(t, torch.float32)
        _require(t.dim() == 3 and t.shape[2] == 256, 'argument check failed: t.dim() == 3 and t.shape[2] == 256')
    nq = x.shape[1]
    _require(nq <= 128 and src.shape[1] == nq and out.shape[1] == nq, 'gnn_layer: nq <= 128, src / out with the same nq')
    _require(x_off + n_sets <= x.shape[0] and src_off + n_sets <= src.shape[0] and out_off + n_sets <= out.shape[0], 'argument check failed: x_off + n_sets <= x.shape[0] and src_off + n_sets <= src.shape[0] and out_off + n_sets <= out.shape[0]')
    if lens is not None:
        _chk(lens, torch.int32)
    nxt = None
    if W_next is not None and GNN_PREFETCH and next_sets > 0:
        nxt = (ctypes.c_void_p * 6)(*[_p(W_next[k]) for k in ("wq", "wk", "wv", "wm", "w0", "w2")])
    _C.nopesac_gnn_layer_bf16_pf(_p(x), x_off, _p(src), src_off, _p(out), out_off, n_sets, nq, _p(lens), _p(lens),
                                 _p(W["wq"]), _p(W["wk"]), _p(W["wv"]), _p(W["wm"]), _p(W["w0"]), _p(W["w2"]),
                                 _p(W["g1"]), _p(W["b1"]), _p(W["g2"]), _p(W["b2"]), nxt, int(next_sets) if nxt is not None else 0, _stream())
    return out


def encoder_tail(attn: torch.Tensor, src: torch.Tensor, W: dict, pos=None, want=("y", "y16", "ypos16")) -> dict:
    """Fused out-proj + residual + LN1 + FFN + residual + LN2 of a post-norm encoder layer (csrc/enc_tail.hip).
    attn bf16 [M,256], src f32 [M,256]; W: fragment-major bf16 "wo", "w1", "w2" + f32 "bo", "g1", "be1", "b1", "b2", "g2", "be2"."""
    _chk(attn, torch.bfloat16); _chk(src, torch.float32)
    M = src.shape[0]
    _require(attn.shape == (M, 256) and src.shape == (M, 256), 'argument check failed: attn.shape == (M, 256) and src.shape == (M, 256)')
    out = {k: torch.empty(M, 256, device=src.device, dtype=torch.float32 if k == "y" else torch.bfloat16) for k in want}
    if pos is not None:
        _chk(pos, torch.float32)
    _C.nopesac_encoder_tail_bf16(_p(attn), _p(src), _p(W["wo"]), _p(W["bo"]), _p(W["g1"]), _p(W["be1"]), _p(W["w1"]), _p(W["b1"]),
                                 _p(W["w2"]), _p(W["b2"]), _p(W["g2"]), _p(W["be2"]), _p(pos), 0 if pos is None else pos.shape[0],
                                 _p(out.get("y")), _p(out.get("y16")), _p(out.get("ypos16")), M, _stream())
    return out


def resize_bilinear_u8(img: torch.Tensor, out_h: int, out_w: int) -> torch.Tensor:
    """uint8 [H,W,C] (device) -> uint8 [out_h,out_w,C], cv2 INTER_LINEAR fixed-point semantics."""
    _chk(img, torch.uint8)
    H, W, C = img.shape
    out = torch.empty((out_h, out_w, C), device=img.device, dtype=torch.uint8)
    _C.nopesac_resize_bilinear_u8(_p(img), H, W, C, _p(out), out_h, out_w, _stream())
    return out


def resize_bilinear_u8_batch(imgs, out_h: int, out_w: int, chw: bool = True) -> torch.Tensor:
    """n uint8 [H,W,C] device images of ONE size lying evenly spaced in one buffer (views of jpeg.decode_batch's output) -> uint8
    [n,C,out_h,out_w] (chw) or [n,out_h,out_w,C], one launch; None if the images are not laid out like that."""
    a = imgs[0]
    _chk(a, torch.uint8)
    H, W, C = a.shape
    n = len(imgs)
    stride = (imgs[1].data_ptr() - a.data_ptr()) if n > 1 else H * W * C
    st = a.untyped_storage().data_ptr()
    if stride < H * W * C or any(im.shape != a.shape or not im.is_contiguous() or im.data_ptr() != a.data_ptr() + k * stride
                                 or im.untyped_storage().data_ptr() != st for k, im in enumerate(imgs)):
        return None
    out = torch.empty((n, C, out_h, out_w) if chw else (n, out_h, out_w, C), device=a.device, dtype=torch.uint8)
    _C.nopesac_resize_bilinear_u8_batch(_p(a), n, stride, H, W, C, _p(out), out_h, out_w, 1 if chw else 0, _stream())
    return out


def augment_workspace_bytes(n: int, H: int, W: int) -> int:
    """Bytes of scratch augment_images needs for n images of H x W (the contrast pre-pass's luma partials)."""
    out = ctypes.c_int64()
    _C.nopesac_augment_workspace_bytes(int(n), int(H), int(W), ctypes.byref(out))
    return out.value


def augment_images(src, params, *, chw_out: Optional[torch.Tensor] = None, nhwc_out: Optional[torch.Tensor] = None,
                   mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None) -> None:
    """The training-time augmentation of csrc/augment.hip on n uint8 [H,W,3] device images of ONE size: `src` a contiguous [n,H,W,3]
    tensor, or a list of views lying evenly spaced in one buffer (jpeg.decode_batch's output, read in place).  params: an
    augment.AugmentParams with its device copy (.to(device)).  Outputs, at least one: chw_out uint8 [n,3,H,W]; nhwc_out f32 [n,H,W,4]
    = (v - mean) / std with a zero pad channel (mean, std f32[3]), bit for bit what `preprocess` makes of the float image."""
    if isinstance(src, torch.Tensor):
        _chk(src, torch.uint8)
        _require(src.dim() == 4, "augment_images: [n,H,W,3] expected")
        n, H, W, C = src.shape
        a, stride = src, H * W * C
    else:
        a = src[0]
        _chk(a, torch.uint8)
        _require(a.dim() == 3, "augment_images: [H,W,3] images expected")
        H, W, C = a.shape
        n = len(src)
        stride = (src[1].data_ptr() - a.data_ptr()) if n > 1 else H * W * C
        st = a.untyped_storage().data_ptr()
        _require(stride >= H * W * C and all(im.shape == a.shape and im.is_contiguous() and im.data_ptr() == a.data_ptr() + k * stride
                                             and im.untyped_storage().data_ptr() == st for k, im in enumerate(src)),
                 "augment_images: the images must have one size and lie evenly spaced in one buffer")
    rows, dev_rows = params.rows, params.device_rows
    _require(len(rows) == n and rows.flags["C_CONTIGUOUS"] and rows.itemsize == 40, "augment_images: one 40-byte parameter row per image")
    _require(dev_rows is not None and dev_rows.device == a.device, "augment_images: params.to(device) first")
    _sized(dev_rows, torch.int32, 10 * n, "augment_images: device rows")
    _require(chw_out is not None or nhwc_out is not None, "augment_images: no output asked for")
    if chw_out is not None:
        _sized(chw_out, torch.uint8, n * 3 * H * W, "augment_images: chw_out")
    if nhwc_out is not None:
        _sized(nhwc_out, torch.float32, n * H * W * 4, "augment_images: nhwc_out")
        _sized(mean, torch.float32, 3, "augment_images: mean")
        _sized(std, torch.float32, 3, "augment_images: std")
    nbytes = augment_workspace_bytes(n, H, W)
    ws = scratch(a.device, nbytes)
    _C.nopesac_augment_u8(_p(a), n, stride, H, W, C, rows.ctypes.data, _p(dev_rows), _p(chw_out), _p(nhwc_out),
                          _p(mean) if nhwc_out is not None else None, _p(std) if nhwc_out is not None else None, _p(ws), ws.numel() * 4, _stream())


# ---- ground truth for training (csrc/train_targets.hip; nopesac_amd/targets.py) ---------------------------------------------------------
LABEL_MAX_IDS, LABEL_TABLE_SLOTS = _lib.H.NPS_LABEL_MAX_IDS, _lib.H.NPS_LABEL_TABLE_SLOTS


def _out(out: Optional[torch.Tensor], shape, dtype, device, what: str) -> torch.Tensor:
    """The caller's output buffer (any shape of the right size: contiguous, `dtype`, on `device`) viewed as `shape`, or a fresh one."""
    n = 1
    for s in shape:
        n *= int(s)
    if out is None:
        return torch.empty(tuple(shape), device=device, dtype=dtype)
    _require(out.device == device, what + ": output on another device")
    return _sized(out, dtype, n, what).view(tuple(shape))


def label_ids(labels: torch.Tensor, nmax_limit: int = _lib.H.NPS_PLANE_MAX_TARGETS, out=None):
    """labels int32 [B, H, W] -> (ids int32 [B, LABEL_MAX_IDS], n_all int32 [B], n int32 [B], bad int32 [B]) on the device: per image the
    distinct labels ascending, a leading 0 dropped (torch.unique + `if plane_ids[0] == 0`, siamese_planeTR.py:488-495), their number,
    n = min(n_all, nmax_limit), and bad = 1 for an image with more than LABEL_MAX_IDS distinct labels (n_all = n = 0 there).  No host
    sync.  out: optionally the four buffers."""
    _chk(labels, torch.int32)
    _require(labels.dim() == 3, "label_ids: labels [B, H, W] expected")
    B, H, W = labels.shape
    dev, o = labels.device, (out or (None,) * 4)
    _require(len(o) == 4, "label_ids: out = (ids, n_all, n, bad)")
    ids = _out(o[0], (B, LABEL_MAX_IDS), torch.int32, dev, "label_ids: ids")
    n_all, n, bad = (_out(t, (B,), torch.int32, dev, "label_ids: " + k) for t, k in zip(o[1:], ("n_all", "n", "bad")))
    _C.nopesac_label_ids(_p(labels), B, H, W, int(nmax_limit), _p(ids), _p(n_all), _p(n), _p(bad), _stream())
    return ids, n_all, n, bad


def label_targets_workspace_bytes(B: int, nmax: int, H: int, W: int) -> int:
    """Bytes of scratch label_targets needs (the integer partial sums of every NPS_LABEL_CHUNK pixels)."""
    out = ctypes.c_int64()
    _C.nopesac_label_targets_workspace_bytes(int(B), int(nmax), int(H), int(W), ctypes.byref(out))
    return out.value


def label_targets(labels: torch.Tensor, ids: torch.Tensor, n: torch.Tensor, nmax: int, out=None):
    """labels int32 [B, H, W], ids int32 [B, LABEL_MAX_IDS] (label_ids), n int32 [B] on the device -> (masks uint8 [B, nmax, H, W],
    plane_centers f32 [B, nmax, 2], pixel_centers f32 [B, 2, H, W]): masks[b, j] = ids[b, j] == labels[b], rows j >= n[b] zero; the
    centres are bit for bit those of plane_targets on these masks.  The label map is read once per pass, not once per plane."""
    _chk(labels, torch.int32)
    _require(labels.dim() == 3, "label_targets: labels [B, H, W] expected")
    B, H, W = labels.shape
    nmax, dev = int(nmax), labels.device
    _sized(ids, torch.int32, B * LABEL_MAX_IDS, "label_targets: ids")
    _sized(n, torch.int32, B, "label_targets: n")
    _require(ids.device == dev and n.device == dev, "label_targets: ids / n on another device")
    _require(1 <= nmax <= PLANE_MAX_TARGETS, "label_targets: nmax=%d outside 1..%d" % (nmax, PLANE_MAX_TARGETS))
    o = out or (None,) * 3
    _require(len(o) == 3, "label_targets: out = (masks, plane_centers, pixel_centers)")
    masks = _out(o[0], (B, nmax, H, W), torch.uint8, dev, "label_targets: masks")
    centers = _out(o[1], (B, nmax, 2), torch.float32, dev, "label_targets: plane_centers")
    pixel = _out(o[2], (B, 2, H, W), torch.float32, dev, "label_targets: pixel_centers")
    ws = scratch(dev, label_targets_workspace_bytes(B, nmax, H, W))
    _C.nopesac_label_targets(_p(labels), _p(ids), _p(n), B, nmax, H, W, _p(masks), _p(centers), _p(pixel), _p(ws), ws.numel() * 4, _stream())
    return masks, centers, pixel


def bits_to_masks(bits: torch.Tensor, offsets: torch.Tensor, nmax: int, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The bit-packed masks of rle.segmentation_bits (int32 [N, ceil(H W / 32)], bit p = x H + y) and the views' exclusive offsets (int64
    [B + 1] on the device) -> masks uint8 [B, nmax, H, W] row-major: view b gets its first nmax rows, the rows it lacks are zero."""
    _chk(bits, torch.int32); _chk(offsets, torch.int64)
    H, W, nmax = int(H), int(W), int(nmax)
    _require(H >= 1 and W >= 1, "bits_to_masks: H, W >= 1")
    words = (H * W + 31) // 32
    _require(bits.dim() == 2 and (bits.shape[0] == 0 or bits.shape[1] == words), "bits_to_masks: bits [N, %d] expected, got %s" % (words, tuple(bits.shape)))
    _require(offsets.dim() == 1 and offsets.numel() >= 2 and offsets.device == bits.device, "bits_to_masks: offsets int64 [B + 1] on the bits' device")
    _require(1 <= nmax <= PLANE_MAX_TARGETS, "bits_to_masks: nmax=%d outside 1..%d" % (nmax, PLANE_MAX_TARGETS))
    B, N = offsets.numel() - 1, int(bits.shape[0])
    masks = _out(out, (B, nmax, H, W), torch.uint8, bits.device, "bits_to_masks: masks")
    _C.nopesac_bits_to_masks(_p(bits) if N else None, N, _p(offsets), B, nmax, H, W, _p(masks), _stream())
    return masks


def depth_from_u16(src: torch.Tensor, scale: float = 1000.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint16 depth (the 16-bit PNG's millimetres; torch.uint16, or int16 holding the same bits) -> f32 of the same shape,
    (float)v / scale with an IEEE division: numpy's astype(float32) / 1000."""
    _require(src.dtype in (torch.uint16, torch.int16), "depth_from_u16: uint16 (or int16 bits) expected, got %s" % src.dtype)
    _chk(src)
    _require(src.numel() >= 1 and float(scale) > 0.0, "depth_from_u16: an empty image, or scale <= 0")
    res = _out(out, tuple(src.shape), torch.float32, src.device, "depth_from_u16: out")
    _C.nopesac_depth_u16_to_f32(_p(src), src.numel(), float(scale), _p(res), _stream())
    return res


def coordinate_map(kinv: torch.Tensor, H: int, W: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kinv f32 [B, 3, 3] or [B, 9] (K^-1, inverted on the host in float64 and rounded once) -> k_inv_dot_xy1 f32 [B, 3, H, W] of
    get_coordinate_map (siamese_planeTR.py:815-839): K^-1 . (x, y, 1) with x = col / W * 640, y = row / H * 480 in f32."""
    _chk(kinv, torch.float32)
    _require(kinv.dim() in (2, 3) and kinv.numel() == 9 * kinv.shape[0], "coordinate_map: kinv [B, 3, 3] expected")
    B, H, W = kinv.shape[0], int(H), int(W)
    res = _out(out, (B, 3, H, W), torch.float32, kinv.device, "coordinate_map: out")
    _C.nopesac_coordinate_map(_p(kinv), B, H, W, _p(res), _stream())
    return res


def mask_head(c1: torch.Tensor, t1: torch.Tensor, w_lat_frag: torch.Tensor, scale, bias, mask_w: torch.Tensor, mask_b: torch.Tensor,
              sigmoid: bool = True, want_p1: bool = False, planar: bool = False, fold: Optional[torch.Tensor] = None, taps1: bool = False,
              pipe: bool = False):
    """Fused lateral conv + bilinear add + per-image mask GEMM (csrc/mask_head.hip).  c1 [B,H,W,256] / t1 [B,H/2,W/2,256] bf16;
    mask_w [B,nq,256] (any float dtype), mask_b [B,nq] f32 -> prob f32 [B,H,W,nq] ([B,nq,H,W] when `planar`) (and p1 bf16 if asked).
    `pipe`: the persistent software-pipelined kernel (round-5 experiment, slower; bit-identical) instead of two workgroups per CU."""
    _chk(c1, torch.bfloat16); _chk(t1, torch.bfloat16); _chk(w_lat_frag, torch.bfloat16)
    B, H, W, C = c1.shape
    nq = mask_w.shape[1] if fold is None else fold.shape[0] // B
    _require(C == 256 and t1.shape == (B, H // 2, W // 2, 256) and nq <= 128 and nq % 2 == 0 and (H * W) % 128 == 0,
             'mask_head: C == 256, t1 at half resolution, nq even and <= 128, H * W a multiple of 128')
    nqp = 64 if nq <= 64 else 128                                                       # planes padded to whole pairs of 32-wide MFMA tiles
    if fold is not None:          # both operands straight from the folded plane embeddings [B * nq, >= 257] f32, one launch
        _chk(fold, torch.float32)
        _require(fold.dim() == 2 and fold.shape[0] == B * nq and fold.shape[1] >= 257 and fold.is_contiguous(), "mask_head: fold [B * nq, >= 257]")
        mw = torch.empty(B, nqp // 32, 16, 2, 32, 8, device=c1.device, dtype=torch.bfloat16)
        mb = torch.empty(B, nqp, device=c1.device, dtype=torch.float32)
        _C.nopesac_mask_operands(_p(fold), fold.shape[1], _p(mw), _p(mb), B, nq, nqp, _stream())
    else:
        mw = torch.zeros(B, nqp, 256, device=c1.device, dtype=torch.bfloat16)
        mw[:, :nq] = mask_w
        mw = mw.view(B, nqp // 32, 32, 16, 2, 8).permute(0, 1, 3, 4, 2, 5).contiguous()    # per-image MFMA fragment-major
        mb = torch.zeros(B, nqp, device=c1.device, dtype=torch.float32)
        mb[:, :nq] = mask_b
    prob = torch.empty((B, nq, H, W) if planar else (B, H, W, nq), device=c1.device, dtype=torch.float32)
    p1 = torch.empty(B, H, W, 256, device=c1.device, dtype=torch.bfloat16) if want_p1 else None
    _C.nopesac_mask_head_bf16(_p(c1), _p(t1), _p(w_lat_frag), _p(scale), _p(bias), _p(mw), _p(mb), _p(prob), _p(p1), B, H, W, nq,
                              int(sigmoid) | (2 if planar else 0) | (4 if taps1 else 0) | (8 if pipe else 0), _stream())
    return (prob, p1) if want_p1 else prob


def decoder_tail(attn: torch.Tensor, tgt: torch.Tensor, W: dict, pos=None, want=("y", "y16", "ypos16")) -> dict:
    """Pre-norm decoder tail (csrc/enc_tail.hip, pre_norm = 1): out-proj + residual, LN3, FFN + residual, next norm.
    W: fragment-major bf16 "wo", "w1", "w2"; f32 "bo", "b1", "b2", "g3", "be3" (norm3), "gn", "ben" (next norm).
    want: "y" (f32 residual stream), "y16" / "ypos16" (bf16 of the normalised result / + pos), "yn" (f32 normalised)."""
    _chk(attn, torch.bfloat16); _chk(tgt, torch.float32)
    M = tgt.shape[0]
    _require(attn.shape == (M, 256) and tgt.shape == (M, 256), 'argument check failed: attn.shape == (M, 256) and tgt.shape == (M, 256)')
    out = {k: torch.empty(M, 256, device=tgt.device, dtype=torch.float32 if k in ("y", "yn") else torch.bfloat16) for k in want}
    if pos is not None:
        _chk(pos, torch.float32)
    _C.nopesac_decoder_tail_bf16(_p(attn), _p(tgt), _p(W["wo"]), _p(W["bo"]), _p(W["g3"]), _p(W["be3"]), _p(W["w1"]), _p(W["b1"]),
                                 _p(W["w2"]), _p(W["b2"]), _p(W["gn"]), _p(W["ben"]), _p(pos), 0 if pos is None else pos.shape[0],
                                 _p(out.get("y")), _p(out.get("y16")), _p(out.get("ypos16")), _p(out.get("yn")), M, _stream())
    return out


TAIL_PREFETCH = os.environ.get("NOPESAC_TAIL_PREFETCH", "1") != "0"
# the kernel forms of the transformer tail, indexed by form id (NPS_ETAIL_* of include/nopesac_hip.h): tokens per workgroup
TRANSFORMER_TAIL_FORMS = _forms_by_id({"t32": _H.NPS_ETAIL_32, "t64": _H.NPS_ETAIL_64, "t96": _H.NPS_ETAIL_96, "t128": _H.NPS_ETAIL_128}, _H.NPS_ETAIL_FORMS)
# A/B switch bits of the default selection (NPS_ETAIL_SW_*); NOPESAC_ENC_TAIL_ROWS sets ROWS, and ROWS3 as well when it is 3
TRANSFORMER_TAIL_SWITCHES = {"NOPESAC_ENC_TAIL_32": _H.NPS_ETAIL_SW_32, "NOPESAC_ENC_TAIL_64": _H.NPS_ETAIL_SW_64,
                             "NOPESAC_ENC_TAIL_ROWS": _H.NPS_ETAIL_SW_ROWS, "NOPESAC_ENC_TAIL_ROWS=3": _H.NPS_ETAIL_SW_ROWS3}


def transformer_tail_forms(M, pre_norm, skip_ffn=False, n_proj_total=0, switches=0):
    """(default form id, bitmask of eligible form ids) of a transformer tail over M tokens whose projections are n_proj_total = n_pos +
    n_proj wide, under the NPS_ETAIL_SW_* switch bits.  Host only: needs no GPU."""
    mask = ctypes.c_uint(0)
    form = _C.nopesac_transformer_tail_forms(M, int(bool(pre_norm)), int(bool(skip_ffn)), n_proj_total, switches, ctypes.byref(mask))
    return form, mask.value


def transformer_tail(attn: torch.Tensor, src: torch.Tensor, W: dict, *, pre_norm: bool, skip_ffn: bool = False, pos=None,
                     want=("y",), proj_pos=None, proj=None, prefetch=None, form=None, out=None) -> dict:
    """The tail of a transformer layer + the input projections of the next attention in one launch (nopesac_transformer_tail_bf16).
    W: "wo", "bo", "ga", "bea" (first norm) and - unless skip_ffn - "w1", "b1", "w2", "b2", "gb", "beb" (second norm); fragment-major
    bf16 matrices, f32 vectors.  proj_pos / proj = (fragment-major weight, f32 bias or None, width): projections of the normalised
    result + pos / of the normalised result, returned as "proj_pos" / "proj" (bf16 [M, width]).  want: any of "y", "y16", "ypos16", "yn".
    prefetch = (tensors, workgroups): the weight tensors and the workgroup count of the NEXT tail launch - with few rows (one pair per
    call) extra workgroups of this launch read them into the L2s the next launch will run on (nopesac_transformer_tail_bf16_pf).
    form: a TRANSFORMER_TAIL_FORMS id to launch instead of the default selection (an ineligible one raises); out: contiguous output
    buffers to write (by the names above) instead of new ones."""
    _chk(attn, torch.bfloat16); _chk(src, torch.float32)
    M = src.shape[0]
    _require(attn.shape == (M, 256) and src.shape == (M, 256), "transformer_tail: attn / src [M, 256]")
    given = dict(out or {})
    if pos is not None:
        _chk(pos, torch.float32)
    wa, ba, na = proj_pos if proj_pos is not None else (None, None, 0)
    wb, bb, nb = proj if proj is not None else (None, None, 0)
    shapes = {k: (256, torch.float32 if k in ("y", "yn") else torch.bfloat16) for k in want}
    if na:
        shapes["proj_pos"] = (na, torch.bfloat16)
    if nb:
        shapes["proj"] = (nb, torch.bfloat16)
    _require(set(given) <= set(shapes), "transformer_tail: out holds a buffer that was not asked for")
    out = {}
    for k, (n, dt) in shapes.items():
        t = given.get(k)
        if t is None:
            t = torch.empty(M, n, device=src.device, dtype=dt)
        _chk(t, dt)
        _require(t.shape == (M, n), "transformer_tail: out[%s] must be [M, %d]" % (k, n))
        out[k] = t
    g = W.get
    nptr = nbytes = None
    n_next = next_wg = 0
    if prefetch is not None and TAIL_PREFETCH and M <= 64 * 32:
        tens = [t for t in prefetch[0] if t is not None][:8]
        if tens and prefetch[1] > 0:
            n_next, next_wg = len(tens), int(prefetch[1])
            nptr = (ctypes.c_void_p * n_next)(*[_p(t) for t in tens])
            nbytes = (ctypes.c_int64 * n_next)(*[t.numel() * t.element_size() for t in tens])
    args = (_p(attn), _p(src), _p(W["wo"]), _p(W["bo"]), _p(W["ga"]), _p(W["bea"]), _p(g("w1")), _p(g("b1")), _p(g("w2")), _p(g("b2")),
            _p(g("gb")), _p(g("beb")), _p(pos), 0 if pos is None else pos.shape[0], _p(out.get("y")), _p(out.get("y16")), _p(out.get("ypos16")),
            _p(out.get("yn")), int(pre_norm), int(skip_ffn), _p(wa), _p(ba), _p(out.get("proj_pos")), na, _p(wb), _p(bb), _p(out.get("proj")), nb,
            M, nptr, nbytes, n_next, next_wg)
    if form is None:
        _C.nopesac_transformer_tail_bf16_pf(*args, _stream())
    else:
        _C.nopesac_transformer_tail_bf16_form(*args, int(form), _stream())
    return out


class PoseBranchTail:
    """Operands of nopesac_posenet_branch_tail_bf16, packed once: layers 1..5 of the two pose-net branches (ConvW objects with folded
    BatchNorm) as fragment-major bf16 weights + pointer tables (the ctypes arrays keep the tensors alive)."""

    def __init__(self, convs_trans, convs_rots):
        import ctypes
        self.keep = []
        ws, ss, bs = [], [], []
        for c in list(convs_trans) + list(convs_rots):
            _require(c.cout == 128 and c.cin == 128 and c.kh == 3 and c.kw == 3 and c.scale is not None and c.bias is not None,
                     "pose-net branch tail: 3x3, 128 -> 128 convs with folded BatchNorm")
            wf = mfma_fragment_major(c.w(torch.bfloat16).reshape(128, -1))
            self.keep += [wf, c.scale, c.bias]
            ws.append(wf.data_ptr()); ss.append(c.scale.data_ptr()); bs.append(c.bias.data_ptr())
        _require(len(ws) == 10, "pose-net branch tail: five layers per branch")
        arr = ctypes.c_void_p * 10
        self.w, self.s, self.b = arr(*ws), arr(*ss), arr(*bs)


def posenet_branch_tail(x_trans: torch.Tensor, x_rots: torch.Tensor, packed: PoseBranchTail):
    """Layers 1..5 of both pose-net branches in one launch.  x_*: layer-0 outputs [B,15,20,128] bf16 -> two [B,2,3,128] f32 tensors."""
    _chk(x_trans, torch.bfloat16); _chk(x_rots, torch.bfloat16)
    B, H, W, C = x_trans.shape
    _require(x_rots.shape == x_trans.shape, "pose-net branch tail: the two branches have the same shape")
    yt = torch.empty((B, 2, 3, 128), device=x_trans.device, dtype=torch.float32)
    yr = torch.empty_like(yt)
    _C.nopesac_posenet_branch_tail_bf16(_p(x_trans), _p(x_rots), packed.w, packed.s, packed.b, _p(yt), _p(yr), B, H, W, C, _stream())
    return yt, yr


def conv3x3_c64(x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, bias: torch.Tensor, act: int = ACT_RELU) -> torch.Tensor:
    """bf16 3x3/s1/p1 conv 64 -> 64 + BN + act from an LDS halo tile (csrc/conv3x3_c64.hip).  x [B,H,W,64], w [64,3,3,64]."""
    _chk(x, torch.bfloat16); _chk(w, torch.bfloat16); _chk(scale, torch.float32); _chk(bias, torch.float32)
    B, H, W, C = x.shape
    _require(C == 64 and tuple(w.shape) == (64, 3, 3, 64), 'argument check failed: C == 64 and tuple(w.shape) == (64, 3, 3, 64)')
    y = torch.empty_like(x)
    _C.nopesac_conv3x3_c64_bf16(_p(x), _p(_frag_weights(w)), _p(scale), _p(bias), _p(y), B, H, W, act, _stream())
    return y


# ---------------------------------------------------------------- backward of the pixel pose net's conv stacks (csrc/conv_bwd.hip)
def wgrad_splits(pixels: int, Cout: int, N: int) -> int:
    """Split-K factor of conv2d_wgrad: about 1024 workgroups over the 128 x 128 output tiles, at least 256 pixels per split."""
    tiles = ((Cout + 127) // 128) * ((N + 127) // 128)
    return max(1, min(256, -(-1024 // tiles), pixels // 256))


def _nhwc_cs(t: torch.Tensor) -> int:
    """Channel stride of a pixel-dense NHWC tensor (a channel slice of a wider buffer is allowed)."""
    _require(t.dim() == 4 and t.stride(3) == 1, "NHWC tensor with unit channel stride expected")
    B, H, W, _ = t.shape
    cs = t.stride(2)
    _require(t.stride(1) == W * cs and t.stride(0) == H * W * cs, "x must be pixel-dense NHWC")
    return cs


def conv2d_dgrad(dy: torch.Tensor, w: torch.Tensor, in_hw, *, stride: int = 1, pad: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of conv2d with respect to its input.  dy [B,OH,OW,Cout] f32 NHWC, w [Cout,Cin,KH,KW] (state-dict layout), in_hw = (H, W)
    -> dx [B,H,W,Cin] (or into `out`, which may be a channel slice of a wider buffer)."""
    _chk(dy, torch.float32, contiguous=False); _chk(w, torch.float32)
    _require(w.dim() == 4, "w must be [Cout, Cin, KH, KW]")
    Cout, Cin, KH, KW = w.shape
    B, OH, OW, C = dy.shape
    _require(C == Cout, (C, Cout))
    H, W = int(in_hw[0]), int(in_hw[1])
    _require((H + 2 * pad - KH) // stride + 1 == OH and (W + 2 * pad - KW) // stride + 1 == OW, "dy does not match the input size")
    if out is None:
        out = torch.empty((B, H, W, Cin), device=dy.device, dtype=torch.float32)
    _require(out.shape == (B, H, W, Cin) and out.dtype == torch.float32, "out must be [B, H, W, Cin] f32")
    wws = scratch(dy.device, 4 * w.numel()) if stride == 1 else None        # the rotated weights: the call's only workspace
    _C.nopesac_conv2d_dgrad_f32(_p(dy), _p(w), _p(out), _p(wws), wws.numel() * 4 if stride == 1 else 0, B, H, W, Cin, Cout, KH, KW,
                                stride, pad, _nhwc_cs(dy), _nhwc_cs(out), _stream())
    return out


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, kernel_size: int, *, stride: int = 1, pad: int = 0, cin: Optional[int] = None,
                 splits: Optional[int] = None) -> torch.Tensor:
    """Gradient of conv2d with respect to its weights.  x [B,H,W,Cx] f32 NHWC (the first `cin` channels are the conv's input; the
    rest - zero padding - get no gradient), dy [B,OH,OW,Cout] -> dw [Cout,cin,k,k] (state-dict layout).  Split-K over pixel ranges into
    scratch(), reduced in a fixed order."""
    _chk(x, torch.float32, contiguous=False); _chk(dy, torch.float32, contiguous=False)
    B, H, W, Cx = x.shape
    Cin = int(cin or Cx)
    _require(Cin <= Cx, (Cin, Cx))
    KH = KW = int(kernel_size)
    Bd, OH, OW, Cout = dy.shape
    _require(Bd == B and (H + 2 * pad - KH) // stride + 1 == OH and (W + 2 * pad - KW) // stride + 1 == OW, "dy does not match x")
    S = int(splits or wgrad_splits(B * OH * OW, Cout, KH * KW * Cin))
    ws = scratch(x.device, int(_C.nopesac_conv2d_wgrad_workspace_bytes(Cout, Cin, KH, KW, S)))
    dw = torch.empty((Cout, Cin, KH, KW), device=x.device, dtype=torch.float32)
    _C.nopesac_conv2d_wgrad_f32(_p(x), _p(dy), _p(dw), _p(ws), ws.numel() * 4, B, H, W, Cin, Cout, KH, KW, stride, pad, _nhwc_cs(x),
                                _nhwc_cs(dy), S, _stream())
    return dw


def conv2d_dgrad_strided(dy: torch.Tensor, w: torch.Tensor, in_hw, *, stride: int = 2, pad: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Gradient of a stride-2 conv2d with respect to its input, on the f32 MFMA (csrc/backbone_bwd.hip: one GEMM per parity class of the
    input pixels, no multiply meets an inserted zero).  dy [B,OH,OW,Cout] f32 NHWC, w [Cout,Cin,k,k] (state-dict layout), k 1 or 3,
    pad = (k - 1) / 2, in_hw = (H, W), any H, W >= 1 -> dx [B,H,W,Cin] (or into `out`); dy and out may be channel slices of wider
    buffers.  Every element of dx is written (k = 1: odd rows / columns as exact zeros).  Cin, Cout and dy's channel stride % 4 == 0."""
    _chk(dy, torch.float32, contiguous=False); _chk(w, torch.float32)
    _require(w.dim() == 4 and dy.dim() == 4, "dy must be [B, OH, OW, Cout] and w [Cout, Cin, KH, KW]")
    _require(stride == 2, "conv2d_dgrad_strided: stride 2 (conv2d_dgrad takes stride 1)")
    Cout, Cin, KH, KW = w.shape
    B, OH, OW, C = dy.shape
    _require(C == Cout, (C, Cout))
    H, W = int(in_hw[0]), int(in_hw[1])
    _require(H >= 1 and W >= 1 and (H + 2 * pad - KH) // 2 + 1 == OH and (W + 2 * pad - KW) // 2 + 1 == OW, "dy does not match the input size")
    if out is None:
        out = torch.empty((B, H, W, Cin), device=dy.device, dtype=torch.float32)
    _chk(out, torch.float32, contiguous=False)
    _require(out.shape == (B, H, W, Cin), "out must be [B, H, W, Cin] f32")
    wws = scratch(dy.device, 4 * w.numel())                               # the repacked weights (NPS_DGRAD_S2_WORKSPACE_BYTES): the call's only workspace
    _C.nopesac_conv2d_dgrad_s2_f32(_p(dy), _p(w), _p(out), _p(wws), wws.numel() * 4, B, H, W, Cin, Cout, KH, KW, int(pad), _nhwc_cs(dy),
                                   _nhwc_cs(out), _stream())
    return out


def maxpool3x3s2_backward(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Backward of the 3x3 / stride-2 / pad-1 max-pool of x [B,H,W,C] f32 (ops.maxpool(x, 3, 2, 1)): each window's dY goes to its first
    maximum in row-major order over the in-bounds taps, as torch.max_pool2d; overlapping windows add in row-major window order."""
    _chk(x, torch.float32); _chk(dy, torch.float32)
    _require(x.dim() == 4, x.shape)
    B, H, W, C = x.shape
    _require(dy.shape == (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), (dy.shape, x.shape))
    dx = torch.empty_like(x)
    _C.nopesac_maxpool3x3s2_backward_f32(_p(x), _p(dy), _p(dx), B, H, W, C, _stream())
    return dx


def frozen_bn_act_backward(g: torch.Tensor, y: torch.Tensor, scale: torch.Tensor, act: int = ACT_RELU, want_dz: bool = False):
    """Backward of y = act(conv * scale + shift [+ residual]) (FrozenBN folded, act NONE or RELU) from the saved post-activation output:
    dz = y > 0 ? g : 0 (RELU) or g, dc = dz * scale.  g, y: [..., C] f32 with unit channel stride, rows dense or [rows, C] with a row
    stride -> dc (dense, g's shape), or (dc, dz) when want_dz (the residual's gradient).  No affine gradients."""
    _chk(g, torch.float32, contiguous=False); _chk(y, torch.float32, contiguous=False); _chk(scale, torch.float32)
    _require(g.shape == y.shape and g.dim() >= 2, (g.shape, y.shape))
    _require(act in (ACT_NONE, ACT_RELU), act)
    C = g.shape[-1]
    _require(scale.numel() == C, (scale.numel(), C))
    rows = g.numel() // C

    def row_stride(t):
        if t.is_contiguous():
            return C
        return _rows(t, rows, C, "frozen_bn_act_backward")

    g_ld, y_ld = row_stride(g), row_stride(y)
    dc = torch.empty(g.shape, device=g.device, dtype=torch.float32)
    dz = torch.empty_like(dc) if want_dz else None
    _C.nopesac_frozen_bn_act_backward_f32(_p(g), _p(y), _p(scale), int(act), rows, C, g_ld, y_ld, _p(dc), _p(dz), _stream())
    return (dc, dz) if want_dz else dc


def _bn_vecs(C, *vs):
    for v in vs:
        _chk(v, torch.float32)
        _require(v.numel() == C, (v.numel(), C))


def bn_act_forward(c: torch.Tensor, gamma, beta, mean, var, eps: float, act=ACT_LEAKY) -> torch.Tensor:
    """Inference-mode BatchNorm (stored statistics, affine gamma / beta) + activation on a contiguous [..., C] f32 tensor."""
    _chk(c, torch.float32)
    C = c.shape[-1]
    _bn_vecs(C, gamma, beta, mean, var)
    y = torch.empty_like(c)
    _C.nopesac_bn_act_forward_f32(_p(c), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), int(act), c.numel() // C, C, _p(y), _stream())
    return y


def bn_act_backward(dy: torch.Tensor, c: torch.Tensor, gamma, beta, mean, var, eps: float, act=ACT_LEAKY):
    """Backward of bn_act_forward from the saved conv output c -> (dc, dgamma, dbeta)."""
    _chk(dy, torch.float32); _chk(c, torch.float32)
    _require(dy.shape == c.shape, (dy.shape, c.shape))
    C = c.shape[-1]
    rows = c.numel() // C
    _bn_vecs(C, gamma, beta, mean, var)
    dc = torch.empty_like(c)
    dg = torch.empty(C, device=c.device, dtype=torch.float32)
    db = torch.empty(C, device=c.device, dtype=torch.float32)
    ws = scratch(c.device, 4 * int(_C.nopesac_bn_act_backward_workspace_floats(rows, C)))
    _C.nopesac_bn_act_backward_f32(_p(dy), _p(c), _p(gamma), _p(beta), _p(mean), _p(var), float(eps), int(act), rows, C, _p(dc), _p(dg),
                                   _p(db), _p(ws), ws.numel(), _stream())
    return dc, dg, db


def groupnorm_backward(x: torch.Tensor, dy: torch.Tensor, gamma, beta, groups: int, eps: float, act=ACT_NONE):
    """Backward of groupnorm(x, gamma, beta, groups, eps, act) (act: NONE or RELU) -> (dx, dgamma, dbeta)."""
    _chk(x, torch.float32); _chk(dy, torch.float32)
    _require(dy.shape == x.shape and x.dim() == 4, (dy.shape, x.shape))
    _require(act in (ACT_NONE, ACT_RELU), act)
    B, H, W, C = x.shape
    _chk(gamma, torch.float32); _chk(beta, torch.float32)
    dx = torch.empty_like(x)
    dg = torch.empty(C, device=x.device, dtype=torch.float32)
    db = torch.empty(C, device=x.device, dtype=torch.float32)
    ws = scratch(x.device, 4 * int(_C.nopesac_groupnorm_backward_workspace_floats(B, C)))
    _C.nopesac_groupnorm_backward_f32(_p(x), _p(dy), _p(gamma), _p(beta), B, H * W, C, groups, float(eps), int(act == ACT_RELU), _p(dx),
                                      _p(dg), _p(db), _p(ws), ws.numel(), _stream())
    return dx, dg, db


def maxpool_backward(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """Backward of the 2x2 / stride-2 max-pool of x [B,H,W,C] f32: dY to the window's first maximum (row-major), as torch.max_pool2d."""
    _chk(x, torch.float32); _chk(dy, torch.float32)
    B, H, W, C = x.shape
    _require(dy.shape == (B, H // 2, W // 2, C), (dy.shape, x.shape))
    dx = torch.empty_like(x)
    _C.nopesac_maxpool2x2_backward_f32(_p(x), _p(dy), _p(dx), B, H, W, C, _stream())
    return dx


def upsample2x_nearest_add_backward(dy: torch.Tensor):
    """Backward of upsample2x_nearest_add(x, lateral): (dx [B,H,W,C] = 2x2 block sums of dy, dlateral = dy)."""
    _chk(dy, torch.float32)
    B, H2, W2, C = dy.shape
    _require(H2 % 2 == 0 and W2 % 2 == 0, dy.shape)
    dx = torch.empty((B, H2 // 2, W2 // 2, C), device=dy.device, dtype=torch.float32)
    _C.nopesac_upsample2x_nearest_add_backward_f32(_p(dy), _p(dx), B, H2 // 2, W2 // 2, C, _stream())
    return dx, dy


def _bn_train_src(src: torch.Tensor, up: bool):
    """The input of a training-mode BatchNorm kernel -> (B, H, W, C, channel stride, n, shape of v): plain form [rows, C] (rows may be
    strided) or pixel-dense NHWC (a channel slice of a wider buffer is allowed); upsampled form: NHWC, v = its bilinear 2x upsampling."""
    _chk(src, torch.float32, contiguous=False)
    if src.dim() == 2 and not up:
        _require(src.stride(1) == 1 and src.stride(0) >= src.shape[1], "rows of unit channel stride expected")
        rows, C = src.shape
        _require(rows > 0 and C > 0 and C % 4 == 0 and src.stride(0) % 4 == 0, "rows of a multiple of 4 channels (and such a stride) expected")
        return rows, 1, 1, C, src.stride(0), rows, (rows, C)
    cs = _nhwc_cs(src)
    B, H, W, C = src.shape
    _require(B > 0 and H > 0 and W > 0 and C > 0 and C % 4 == 0 and cs % 4 == 0, "a multiple of 4 channels (and such a channel stride) expected")
    return (B, H, W, C, cs, 4 * B * H * W, (B, 2 * H, 2 * W, C)) if up else (B, H, W, C, cs, B * H * W, (B, H, W, C))


def bn_train_workspace_floats(n: int, C: int) -> int:
    """The library's nopesac_bn_train_workspace_floats, what both training-BatchNorm launchers check against."""
    return int(_C.nopesac_bn_train_workspace_floats(n, C))


def bn_train_groups_workspace_floats(groups: int, n: int, C: int) -> int:
    """The library's nopesac_bn_train_groups_workspace_floats, what the view-group launchers check against (n = all rows)."""
    out = ctypes.c_int64(0)
    _C.nopesac_bn_train_groups_workspace_floats(int(groups), int(n), int(C), ctypes.addressof(out))
    return int(out.value)


def _bn_train_groups(groups, B: int, what: str) -> int:
    """The view groups of a training-BatchNorm call: G groups of B / G consecutive images (rows of the matrix form)."""
    _require(isinstance(groups, int) and not isinstance(groups, bool) and 1 <= groups <= _H.NPS_BN_TRAIN_MAX_GROUPS and B % groups == 0,
             "%s: 1 <= groups <= %d dividing the %d images (rows) expected, got %r" % (what, _H.NPS_BN_TRAIN_MAX_GROUPS, B, groups))
    return groups


def bn_train_stats(src: torch.Tensor, *, up: bool = False, eps: float = 1e-5, momentum: float = 0.1, running_mean=None, running_var=None,
                   groups: int = 1):
    """Batch statistics of a training-mode BatchNorm over v = src ([rows, C] or NHWC) or, with `up`, v = upsample2x_bilinear(src) evaluated
    on the fly -> (mean, biased var, rstd = 1 / sqrt(var + eps)), [C] each.  running_mean / running_var (both or neither) are updated in
    place on the device as torch.nn.BatchNorm2d does (momentum, unbiased variance); no host sync.  One value per channel is refused.
    groups = G > 1: the images (rows of the matrix form) are G view groups of consecutive ones with their own statistics, [G, C] each,
    every group's with the bits of a call on its sub-tensor; the running buffers take them in group order, as G module calls would."""
    B, H, W, C, cs, n, _ = _bn_train_src(src, up)
    G = _bn_train_groups(groups, B, "bn_train_stats")
    _require(n // G >= 2, "bn_train_stats: more than one value per channel expected")
    _require((running_mean is None) == (running_var is None), "running_mean and running_var come together")
    if running_mean is not None:
        _bn_vecs(C, running_mean, running_var)
    mean, var, rstd = (torch.empty(C if G == 1 else (G, C), device=src.device, dtype=torch.float32) for _ in range(3))
    if G == 1:
        ws = scratch(src.device, 4 * bn_train_workspace_floats(n, C))
        _C.nopesac_bn_train_stats_f32(_p(src), int(up), B, H, W, C, cs, float(eps), float(momentum), _p(mean), _p(var), _p(rstd), _p(running_mean),
                                      _p(running_var), _p(ws), ws.numel(), _stream())
    else:
        ws = scratch(src.device, 4 * bn_train_groups_workspace_floats(G, n, C))
        _C.nopesac_bn_train_groups_stats_f32(_p(src), int(up), B, H, W, C, cs, G, float(eps), float(momentum), _p(mean), _p(var), _p(rstd),
                                             _p(running_mean), _p(running_var), _p(ws), ws.numel(), _stream())
    return mean, var, rstd


def bn_train_apply(src: torch.Tensor, gamma, beta, mean, rstd, act=ACT_RELU, addend: Optional[torch.Tensor] = None, *, up: bool = False,
                   groups: int = 1) -> torch.Tensor:
    """act(gamma (v - mean) rstd + beta) (+ addend, after the activation) for v as in bn_train_stats; act: NONE or RELU.  Dense output.
    groups = G > 1: mean / rstd are [G, C], each row takes its view group's."""
    B, H, W, C, cs, n, shape = _bn_train_src(src, up)
    G = _bn_train_groups(groups, B, "bn_train_apply")
    _require(act in (ACT_NONE, ACT_RELU), act)
    _bn_vecs(C, gamma, beta)
    _bn_vecs(G * C, mean, rstd)
    if addend is not None:
        _chk(addend, torch.float32)
        _require(tuple(addend.shape) == shape, (tuple(addend.shape), shape))
    y = torch.empty(shape, device=src.device, dtype=torch.float32)
    if G == 1:
        _C.nopesac_bn_train_apply_f32(_p(src), int(up), B, H, W, C, cs, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act), _p(addend), _p(y), _stream())
    else:
        _C.nopesac_bn_train_groups_apply_f32(_p(src), int(up), B, H, W, C, cs, G, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act), _p(addend),
                                             _p(y), _stream())
    return y


def bn_train_backward(dy: torch.Tensor, src: torch.Tensor, gamma, beta, mean, rstd, act=ACT_RELU, *, up: bool = False, batch_stats: bool = True,
                      groups: int = 1, group_sums: bool = False):
    """Backward of bn_train_apply through the batch statistics, from the same input (v is recomputed) -> (dsrc, dgamma, dbeta): plain form
    dsrc = dv, dense in v's shape; with `up` dsrc = the gradient at src [B, H, W, C], the bilinear adjoint of dv gathered in the same launch
    (dv is never written).  batch_stats=False: mean / rstd are stored statistics, constants of the backward (dv = gamma rstd dz).  The
    addend's gradient is dy itself.  groups = G > 1: mean / rstd [G, C]; every view group's dsrc comes from its own sums S2_g = sum dz xhat,
    S1_g = sum dz, and dgamma / dbeta add them in group order; group_sums=True appends them, [G, 2, C] = (S2_g, S1_g)."""
    B, H, W, C, cs, n, shape = _bn_train_src(src, up)
    G = _bn_train_groups(groups, B, "bn_train_backward")
    _require(act in (ACT_NONE, ACT_RELU), act)
    _chk(dy, torch.float32)
    _require(tuple(dy.shape) == shape, (tuple(dy.shape), shape))
    _bn_vecs(C, gamma, beta)
    _bn_vecs(G * C, mean, rstd)
    dsrc = torch.empty(tuple(src.shape) if up else shape, device=src.device, dtype=torch.float32)
    dg = torch.empty(C, device=src.device, dtype=torch.float32)
    db = torch.empty(C, device=src.device, dtype=torch.float32)
    if G == 1:
        ws = scratch(src.device, 4 * bn_train_workspace_floats(n, C))
        _C.nopesac_bn_train_backward_f32(_p(dy), _p(src), int(up), B, H, W, C, cs, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act), int(bool(batch_stats)), _p(dsrc), _p(dg),
                                         _p(db), _p(ws), ws.numel(), _stream())
        sums = torch.stack([dg, db])[None] if group_sums else None
    else:
        sums = torch.empty(G, 2, C, device=src.device, dtype=torch.float32)
        ws = scratch(src.device, 4 * bn_train_groups_workspace_floats(G, n, C))
        _C.nopesac_bn_train_groups_backward_f32(_p(dy), _p(src), int(up), B, H, W, C, cs, G, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act),
                                                int(bool(batch_stats)), _p(dsrc), _p(dg), _p(db), _p(sums), _p(ws), ws.numel(), _stream())
    return (dsrc, dg, db, sums) if group_sums else (dsrc, dg, db)


def _bn_grouped_src(c: torch.Tensor, groups: int):
    """The input of a grouped training-mode BatchNorm kernel, contiguous f32 [..., C] cut into `groups` runs of consecutive rows
    -> (G, rows per group, C)."""
    _chk(c, torch.float32)
    _require(isinstance(groups, int) and not isinstance(groups, bool) and 1 <= groups <= _H.NPS_BN_GROUPED_MAX_GROUPS,
             "bn_train_grouped: 1 <= groups <= %d expected, got %r" % (_H.NPS_BN_GROUPED_MAX_GROUPS, groups))
    _require(c.dim() >= 2 and c.numel() > 0, "bn_train_grouped: [..., C] with at least one row expected, got %s" % (tuple(c.shape),))
    C = c.shape[-1]
    _require(C % 4 == 0, "bn_train_grouped: a multiple of 4 channels expected, got %d" % C)
    rows = c.numel() // C
    _require(rows % groups == 0, "bn_train_grouped: %d rows do not divide into %d groups" % (rows, groups))
    return groups, rows // groups, C


def bn_train_grouped_workspace_floats(groups: int, n: int, C: int) -> int:
    """The library's nopesac_bn_train_grouped_workspace_floats, what both grouped training-BatchNorm launchers check against."""
    out = ctypes.c_int64(0)
    _C.nopesac_bn_train_grouped_workspace_floats(int(groups), int(n), int(C), ctypes.addressof(out))
    return int(out.value)


def bn_train_grouped_stats(c: torch.Tensor, groups: int, *, eps: float, momentum: float, running_mean=None, running_var=None):
    """Batch statistics of a training-mode BatchNorm per group of rows of c [..., C] (group g: rows [g n, (g + 1) n) of the rows x C
    matrix) -> (mean, biased var, rstd = 1 / sqrt(var + eps)), [groups, C] each.  running_mean / running_var [C] (both or neither) take
    the groups' statistics one after the other, in place on the device, as `groups` calls of torch.nn.BatchNorm2d in a row do
    (momentum, unbiased variance); no host sync.  One value per channel and group is refused."""
    G, n, C = _bn_grouped_src(c, groups)
    _require(n >= 2, "bn_train_grouped_stats: more than one value per channel and group expected")
    _require((running_mean is None) == (running_var is None), "running_mean and running_var come together")
    if running_mean is not None:
        _bn_vecs(C, running_mean, running_var)
    mean, var, rstd = (torch.empty((G, C), device=c.device, dtype=torch.float32) for _ in range(3))
    ws = scratch(c.device, 4 * bn_train_grouped_workspace_floats(G, n, C))
    _C.nopesac_bn_train_grouped_stats_f32(_p(c), G, n, C, float(eps), float(momentum), _p(mean), _p(var), _p(rstd), _p(running_mean),
                                          _p(running_var), _p(ws), ws.numel(), _stream())
    return mean, var, rstd


def bn_train_grouped_apply(c: torch.Tensor, gamma, beta, mean, rstd, act=ACT_LEAKY, groups: int = 1) -> torch.Tensor:
    """act(gamma (c - mean_g) rstd_g + beta) with mean, rstd [groups, C]; act: NONE, RELU or LEAKY (slope 0.01)."""
    G, n, C = _bn_grouped_src(c, groups)
    _require(act in (ACT_NONE, ACT_RELU, ACT_LEAKY), act)
    _bn_vecs(C, gamma, beta)
    _bn_vecs(G * C, mean, rstd)
    y = torch.empty_like(c)
    _C.nopesac_bn_train_grouped_apply_f32(_p(c), G, n, C, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act), _p(y), _stream())
    return y


def bn_train_grouped_backward(dy: torch.Tensor, c: torch.Tensor, gamma, beta, mean, rstd, act=ACT_LEAKY, groups: int = 1, *,
                              batch_stats: bool = True):
    """Backward of bn_train_grouped_apply through every group's batch statistics, from the saved input c (z is recomputed with the
    forward's expression) -> (dc, dgamma, dbeta); dgamma / dbeta sum the groups in group order.  batch_stats=False: mean / rstd are
    constants of the backward (dc = gamma rstd dz)."""
    G, n, C = _bn_grouped_src(c, groups)
    _require(act in (ACT_NONE, ACT_RELU, ACT_LEAKY), act)
    _chk(dy, torch.float32)
    _require(dy.shape == c.shape, (tuple(dy.shape), tuple(c.shape)))
    _bn_vecs(C, gamma, beta)
    _bn_vecs(G * C, mean, rstd)
    dc = torch.empty_like(c)
    dg = torch.empty(C, device=c.device, dtype=torch.float32)
    db = torch.empty(C, device=c.device, dtype=torch.float32)
    ws = scratch(c.device, 4 * bn_train_grouped_workspace_floats(G, n, C))
    _C.nopesac_bn_train_grouped_backward_f32(_p(dy), _p(c), G, n, C, _p(gamma), _p(beta), _p(mean), _p(rstd), int(act), int(bool(batch_stats)),
                                             _p(dc), _p(dg), _p(db), _p(ws), ws.numel(), _stream())
    return dc, dg, db


def upsample2x_bilinear_backward(du: torch.Tensor) -> torch.Tensor:
    """The adjoint of upsample2x_bilinear: du [B, 2H, 2W, C] f32 -> dx [B, H, W, C]."""
    _chk(du, torch.float32)
    _require(du.dim() == 4 and du.shape[1] % 2 == 0 and du.shape[2] % 2 == 0 and du.numel() > 0 and du.shape[3] % 4 == 0, tuple(du.shape))
    B, H2, W2, C = du.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, C), device=du.device, dtype=torch.float32)
    _C.nopesac_upsample2x_bilinear_backward_f32(_p(du), _p(dx), B, H2 // 2, W2 // 2, C, _stream())
    return dx


def transpose_batched(x: torch.Tensor) -> torch.Tensor:
    """[B, rows, cols] f32 -> contiguous [B, cols, rows]."""
    _chk(x, torch.float32)
    _require(x.dim() == 3, x.shape)
    B, R, Cc = x.shape
    y = torch.empty((B, Cc, R), device=x.device, dtype=torch.float32)
    _C.nopesac_transpose_batched_f32(_p(x), B, R, Cc, _p(y), _stream())
    return y


def corr_softmax(x1: torch.Tensor, x2: torch.Tensor, pad_to: int = 0) -> torch.Tensor:
    """The pixel pose net's correlation softmax (camera_head.py:1117-1133) in f32: x1, x2 [B,h,w,C] -> A [B,h,w,max(h w, pad_to)], channel =
    view-2 position in (w, h) order, softmax over the h w channels, zeros beyond."""
    _chk(x1, torch.float32); _chk(x2, torch.float32)
    B, h, w, C = x1.shape
    _require(x2.shape == x1.shape, (x1.shape, x2.shape))
    x2t = transpose_hw_rows(x2.reshape(B, h * w, C), h, w)
    corr = conv2d(x1, x2t.view(B, h * w, 1, 1, C), batched_weights=True)
    return softmax_rows(corr, pad_to=pad_to)


def corr_softmax_backward(a: torch.Tensor, da: torch.Tensor, x1: torch.Tensor, x2: torch.Tensor):
    """Backward of corr_softmax: A [B,h,w,ld] (ld >= h w: the padded channels carry no gradient), dA like A, the inputs x1 / x2
    [B,h,w,C] -> (dx1, dx2).  dS = A (dA - sum dA A); dx1 = dS x2t, dx2t = dS^T x1 on the batched f32 GEMM; dx2 back to (h, w) order."""
    _chk(a, torch.float32); _chk(da, torch.float32); _chk(x1, torch.float32); _chk(x2, torch.float32)
    B, h, w, C = x1.shape
    P = h * w
    _require(a.shape[:3] == (B, h, w) and a.shape[3] >= P and da.shape == a.shape and x2.shape == x1.shape, (a.shape, da.shape, x1.shape))
    ld = a.shape[3]
    ds = torch.empty((B, h, w, P), device=a.device, dtype=torch.float32)
    ds_t = torch.empty((B, P, P), device=a.device, dtype=torch.float32)
    _C.nopesac_corr_softmax_backward_f32(_p(a), _p(da), B, P, P, ld, ld, _p(ds), _p(ds_t), _stream())
    x2t = transpose_hw_rows(x2.reshape(B, P, C), h, w)                      # [B, P (w,h order), C]
    dx1 = conv2d(ds, transpose_batched(x2t).view(B, C, 1, 1, P), batched_weights=True)            # [B,h,w,C]
    dx2t = conv2d(ds_t.view(B, h, w, P), transpose_batched(x1.reshape(B, P, C)).view(B, C, 1, 1, P), batched_weights=True)
    dx2 = transpose_hw_rows(dx2t.reshape(B, P, C), w, h).view(B, h, w, C)
    return dx1, dx2


# ---- backward kernels and optimiser of the training path (csrc/refine_bwd.hip, csrc/matcher_bwd.hip; nopesac_amd/training.py) --------------
# The kernels index from the integer dimensions passed beside the pointers, so every wrapper checks what the C side cannot see: device,
# dtype, density and that each tensor holds the element count those dimensions imply.  Ranges the entry points refuse themselves
# (nq, Lq, Lk <= 128, D <= 4, step >= 1, ...) are not restated: they surface as HipKernelError.
def transpose_rows(x: torch.Tensor) -> torch.Tensor:
    """[rows, cols] f32 (rows may be strided) -> contiguous [cols, rows]."""
    _require(x.dim() == 2, "transpose_rows: [rows, cols]")
    ld = _rows(x, x.shape[0], x.shape[1], "transpose_rows: x")
    y = torch.empty(x.shape[1], x.shape[0], device=x.device, dtype=torch.float32)
    _C.nopesac_transpose_f32(_p(x), x.shape[0], x.shape[1], ld, _p(y), _stream())
    return y


def col_sum(x: torch.Tensor) -> torch.Tensor:
    """Column sums [cols] of [rows, cols] f32 (rows may be strided), in a fixed order."""
    _require(x.dim() == 2, "col_sum: [rows, cols]")
    ld = _rows(x, x.shape[0], x.shape[1], "col_sum: x")
    out = torch.empty(x.shape[1], device=x.device, dtype=torch.float32)
    _C.nopesac_col_sum_f32(_p(x), x.shape[0], x.shape[1], ld, _p(out), _stream())
    return out


def relu_backward(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """y > 0 ? g : 0 for the output y of a ReLU and its gradient g."""
    _chk(g, torch.float32)
    _sized(y, torch.float32, g.numel(), "relu_backward: y")
    out = torch.empty_like(g)
    _C.nopesac_relu_backward_f32(_p(g), _p(y), g.numel(), _p(out), _stream())
    return out


def ransac_score_maps_backward(geo_local, rot_raw, trans_raw, init_rot, init_trans, m, g_normal_score, g_param_score, g_l2_dist):
    """Backward of ransac_score_maps: the gradients of normal_score / param_score / l2_dist [B,nq+1,nq] ->
    (g_rot_raw [B,nq,4], g_trans_raw [B,nq,3], g_init_rot [B,4], g_init_trans [B,3])."""
    _chk(geo_local, torch.float32)
    _require(geo_local.dim() == 3 and geo_local.shape[2] == 6, "ransac_score_maps_backward: geo_local [B,nq,6]")
    B, nq, _ = geo_local.shape
    _sized(rot_raw, torch.float32, B * nq * 4, "ransac_score_maps_backward: rot_raw")
    _sized(trans_raw, torch.float32, B * nq * 3, "ransac_score_maps_backward: trans_raw")
    _sized(init_rot, torch.float32, B * 4, "ransac_score_maps_backward: init_rot")
    _sized(init_trans, torch.float32, B * 3, "ransac_score_maps_backward: init_trans")
    _sized(m, torch.int32, B, "ransac_score_maps_backward: m")
    for t in (g_normal_score, g_param_score, g_l2_dist):
        _sized(t, torch.float32, B * (nq + 1) * nq, "ransac_score_maps_backward: score gradient [B,nq+1,nq]")
    f32 = dict(device=geo_local.device, dtype=torch.float32)
    out = (torch.empty(B, nq, 4, **f32), torch.empty(B, nq, 3, **f32), torch.empty(B, 4, **f32), torch.empty(B, 3, **f32))
    _C.nopesac_refine_score_maps_backward(_p(geo_local), _p(rot_raw), _p(trans_raw), _p(init_rot), _p(init_trans), _p(m), B, nq,
                                          _p(g_normal_score), _p(g_param_score), _p(g_l2_dist), *[_p(t) for t in out], _stream())
    return out


def ransac_soft_vote_backward(sf_rot, sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot,
                              fused_trans, rots_w, rots_b, trans_w, trans_b, m, g_pred_rot, g_pred_trans, g_avg_rot, g_avg_trans, g_score_rot,
                              g_score_trans) -> dict:
    """Backward of ransac_soft_vote (mode | 16) -> the gradients of the score features g_sf_rot / g_sf_trans [B,nq+1,64], of the initial pose
    features g_init_rot_feat / g_init_trans_feat [B,256], of the per-plane features g_fused_rot / g_fused_trans [B,nq,256] and the PER-PAIR
    partials pb_<parameter> [B, size of the parameter] of the eight parameter gradients (sum them with col_sum)."""
    _chk(sf_rot, torch.float32)
    _require(sf_rot.dim() == 3 and sf_rot.shape[2] == 64, "ransac_soft_vote_backward: sf_rot [B,nq+1,64]")
    B, NH, _ = sf_rot.shape
    nq = NH - 1
    inputs = (sf_trans, reg_rot_w, reg_rot_b, reg_trans_w, reg_trans_b, init_rot_feat, init_trans_feat, fused_rot, fused_trans, rots_w,
              rots_b, trans_w, trans_b, g_pred_rot, g_pred_trans, g_avg_rot, g_avg_trans, g_score_rot, g_score_trans)
    sizes = (B * NH * 64, 64, 1, 64, 1, B * 256, B * 256, B * nq * 256, B * nq * 256, 4 * 256, 4, 3 * 256, 3, B * 4, B * 3, B * 4, B * 3,
             B * NH, B * NH)
    for t, n in zip(inputs, sizes):
        _sized(t, torch.float32, n, "ransac_soft_vote_backward: an argument behind sf_rot, in the entry point's order")
    _sized(m, torch.int32, B, "ransac_soft_vote_backward: m")
    f32 = dict(device=sf_rot.device, dtype=torch.float32)
    out = {"g_sf_rot": torch.empty(B, NH, 64, **f32), "g_sf_trans": torch.empty(B, NH, 64, **f32), "g_init_rot_feat": torch.empty(B, 256, **f32),
           "g_init_trans_feat": torch.empty(B, 256, **f32), "g_fused_rot": torch.empty(B, nq, 256, **f32),
           "g_fused_trans": torch.empty(B, nq, 256, **f32), "pb_rots_w": torch.empty(B, 4 * 256, **f32), "pb_rots_b": torch.empty(B, 4, **f32),
           "pb_trans_w": torch.empty(B, 3 * 256, **f32), "pb_trans_b": torch.empty(B, 3, **f32), "pb_reg_rot_w": torch.empty(B, 64, **f32),
           "pb_reg_rot_b": torch.empty(B, 1, **f32), "pb_reg_trans_w": torch.empty(B, 64, **f32), "pb_reg_trans_b": torch.empty(B, 1, **f32)}
    _C.nopesac_refine_vote_backward(_p(sf_rot), *[_p(t) for t in inputs[:13]], _p(m), B, nq, *[_p(t) for t in inputs[13:]],
                                    *[_p(t) for t in out.values()], _stream())         # (out is in the entry point's argument order)
    return out


def plane_cam_ref_losses_backward(vote: dict, maps: dict, m, gt_pose, g_losses, weight: float = 1.0):
    """Backward of plane_cam_ref_losses: g_losses f32[7] -> the gradients of (pred_rot [B,4], pred_trans [B,3], avg_rot, avg_trans,
    score_rot [B,nq+1], score_trans, l2_dist [B,nq+1,nq]); `maps` needs rots_all / trans_all only (the hypothesis the index losses pick
    is a constant)."""
    _chk(gt_pose, torch.float32)
    _require(gt_pose.dim() == 2 and gt_pose.shape[1] == 7, "plane_cam_ref_losses_backward: gt_pose [B,7]")
    B = gt_pose.shape[0]
    _chk(vote["score_rot"], torch.float32)
    _require(vote["score_rot"].dim() == 2 and vote["score_rot"].shape[0] == B, "plane_cam_ref_losses_backward: score_rot [B,nq+1]")
    NH = vote["score_rot"].shape[1]
    args = ((vote["pred_rot"], B * 4), (vote["pred_trans"], B * 3), (vote["avg_rot"], B * 4), (vote["avg_trans"], B * 3),
            (maps["rots_all"], B * NH * 4), (maps["trans_all"], B * NH * 3), (vote["score_rot"], B * NH), (vote["score_trans"], B * NH))
    for t, n in args:
        _sized(t, torch.float32, n, "plane_cam_ref_losses_backward: vote / maps")
    _sized(m, torch.int32, B, "plane_cam_ref_losses_backward: m")
    _sized(g_losses, torch.float32, 7, "plane_cam_ref_losses_backward: g_losses")
    f32 = dict(device=gt_pose.device, dtype=torch.float32)
    out = (torch.empty(B, 4, **f32), torch.empty(B, 3, **f32), torch.empty(B, 4, **f32), torch.empty(B, 3, **f32), torch.empty(B, NH, **f32),
           torch.empty(B, NH, **f32), torch.empty(B, NH, NH - 1, **f32))
    _C.nopesac_refine_losses_backward(*[_p(t) for t, _ in args], _p(m), _p(gt_pose), _p(g_losses), B, NH - 1, float(weight),
                                      *[_p(t) for t in out], _stream())
    return out


def normalize_rows_backward(x: torch.Tensor, g: torch.Tensor, canonical_sign: bool = False) -> torch.Tensor:
    """Backward of normalize_rows(x, canonical_sign) at its input x for the output gradient g."""
    _chk(x, torch.float32)
    _sized(g, torch.float32, x.numel(), "normalize_rows_backward: g")
    D = x.shape[-1]
    out = torch.empty_like(x)
    _C.nopesac_normalize_rows_backward(_p(x), _p(g), x.numel() // D, D, int(canonical_sign), _p(out), _stream())
    return out


def camera_pose_loss_backward(est_trans, est_rot, gt_trans, gt_rot, g_out, weight: float = 1.0, trans_eps: float = 0.0):
    """Backward of camera_pose_loss: g_out f32[2] -> the gradients of all four pose arguments ([B,3] / [B,4], dense).  `gt_trans` /
    `gt_rot` may be column views of one [B,7] pose tensor, as in the forward (row strides are passed on)."""
    _chk(est_trans, torch.float32)
    _require(est_trans.dim() == 2 and est_trans.shape[1] == 3, "camera_pose_loss_backward: est_trans [B,3]")
    B = est_trans.shape[0]
    _sized(est_rot, torch.float32, B * 4, "camera_pose_loss_backward: est_rot")
    st = _rows(gt_trans, B, 3, "camera_pose_loss_backward: gt_trans")
    sq = _rows(gt_rot, B, 4, "camera_pose_loss_backward: gt_rot")
    _require(gt_trans.shape[1] == 3 and gt_rot.shape[1] == 4, "camera_pose_loss_backward: gt_trans [B,3], gt_rot [B,4]")
    _sized(g_out, torch.float32, 2, "camera_pose_loss_backward: g_out")
    f32 = dict(device=est_trans.device, dtype=torch.float32)
    out = (torch.empty(B, 3, **f32), torch.empty(B, 4, **f32), torch.empty(B, 3, **f32), torch.empty(B, 4, **f32))
    _C.nopesac_camera_pose_loss_backward(_p(est_trans), _p(est_rot), _p(gt_trans), st, _p(gt_rot), sq, B, float(trans_eps), float(weight),
                                         _p(g_out), *[_p(t) for t in out], _stream())
    return out


def attention_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_out: torch.Tensor, B: int, Lq: int, Lk: int, heads: int,
                       scale: float, qlen=None, klen=None, out=None):
    """Backward of attention (f32, head dim 32) for the output gradient d_out [B*Lq, >= heads*32]: -> (dq, dk, dv), each [rows, heads*32];
    the softmax is recomputed.  Like q / k / v, d_out and `out` = (dq, dk, dv) may be column slices of wider matrices."""
    W = heads * 32
    sq, sk, sv = _rows(q, B * Lq, W, "attention_backward: q"), _rows(k, B * Lk, W, "attention_backward: k"), _rows(v, B * Lk, W, "attention_backward: v")
    sg = _rows(d_out, B * Lq, W, "attention_backward: d_out")
    _lengths(qlen, B, "attention_backward: qlen"); _lengths(klen, B, "attention_backward: klen")
    if out is None:
        out = tuple(torch.empty(rows, W, device=q.device, dtype=torch.float32) for rows in (B * Lq, B * Lk, B * Lk))
    dq, dk, dv = out
    so = [_rows(t, rows, W, "attention_backward: out") for t, rows in ((dq, B * Lq), (dk, B * Lk), (dv, B * Lk))]
    _C.nopesac_attention_small_backward(_p(q), sq, _p(k), sk, _p(v), sv, _p(d_out), sg, B, Lq, Lk, heads, float(scale), _p(qlen), _p(klen),
                                        _p(dq), so[0], _p(dk), so[1], _p(dv), so[2], _stream())
    return dq, dk, dv


def layernorm_backward(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor, eps: float = 1e-5):
    """Backward of layernorm over D = 256: x [rows, 256] (the LayerNorm input), gamma [256], dy like x -> (dx, dgamma, dbeta)."""
    _chk(x, torch.float32)
    D = x.shape[-1]
    rows = x.numel() // D
    _sized(gamma, torch.float32, D, "layernorm_backward: gamma")
    _sized(dy, torch.float32, rows * D, "layernorm_backward: dy")
    dx, dgamma, dbeta = torch.empty_like(x), torch.empty_like(gamma), torch.empty_like(gamma)
    ws = scratch(x.device, 4 * int(_C.nopesac_layernorm_backward_workspace_floats(rows)))
    _C.nopesac_layernorm_backward(_p(x), _p(gamma), _p(dy), rows, D, float(eps), _p(dx), _p(dgamma), _p(dbeta), _p(ws), ws.numel(), _stream())
    return dx, dgamma, dbeta


def desc_dot_backward(g: torch.Tensor, d0: torch.Tensor, d1: torch.Tensor, n1: torch.Tensor, n2: torch.Tensor):
    """Backward of dots[b] = d0[b] d1[b]^T / 16: g [B,nq,nq], d0 / d1 [B,nq,256], n1 / n2 int32 [B] -> (dd0, dd1), zero rows beyond n1 / n2."""
    _chk(d0, torch.float32)
    _require(d0.dim() == 3, "desc_dot_backward: d0 [B,nq,D]")
    B, nq, D = d0.shape
    _sized(d1, torch.float32, B * nq * D, "desc_dot_backward: d1")
    _sized(g, torch.float32, B * nq * nq, "desc_dot_backward: g")
    _sized(n1, torch.int32, B, "desc_dot_backward: n1"); _sized(n2, torch.int32, B, "desc_dot_backward: n2")
    dd0, dd1 = torch.empty_like(d0), torch.empty_like(d0)
    _C.nopesac_desc_dot_backward(_p(g), _p(d0), _p(d1), _p(n1), _p(n2), B, nq, D, _p(dd0), _p(dd1), _stream())
    return dd0, dd1


def _matcher_pairs(n1, n2, gt_corr, B: int, nq: int):
    """The operands every training entry point of the matcher takes: n1 / n2 int32 [B], gt_corr uint8 [B,nq+1,nq+1] (with the dustbin)."""
    _sized(n1, torch.int32, B, "matcher training: n1"); _sized(n2, torch.int32, B, "matcher training: n2")
    _sized(gt_corr, torch.uint8, B * (nq + 1) * (nq + 1), "matcher training: gt_corr [B,nq+1,nq+1] (dustbin row and column included)")


def _matcher_inputs(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, gt_corr):
    """The inputs matcher_sinkhorn_train and its backward share -> (B, nq)."""
    _chk(desc_dot, torch.float32)
    _require(desc_dot.dim() == 3 and desc_dot.shape[1] == desc_dot.shape[2], "matcher training: desc_dot [B,nq,nq]")
    B, nq, _ = desc_dot.shape
    _sized(planes1, torch.float32, B * nq * 3, "matcher training: planes1"); _sized(planes2, torch.float32, B * nq * 3, "matcher training: planes2")
    _sized(cam7, torch.float32, B * 7, "matcher training: cam7"); _sized(bin_score, torch.float32, 1, "matcher training: bin_score")
    _matcher_pairs(n1, n2, gt_corr, B, nq)
    return B, nq


def matcher_emb_loss(log_scores: torch.Tensor, gt_corr: torch.Tensor, n1: torch.Tensor, n2: torch.Tensor):
    """embedding_loss_forward (matching_head.py:135-139) on the log scores [B,nq+1,nq+1] of matcher_sinkhorn -> (pair_stats [B,2] = the
    pair's sum of -min(score, 0) over the entries gt_corr selects and their count, loss [2] = (2 * sum / count over the batch, count))."""
    _chk(log_scores, torch.float32)
    _require(log_scores.dim() == 3 and log_scores.shape[1] == log_scores.shape[2], "matcher_emb_loss: log_scores [B,nq+1,nq+1]")
    B, nq = log_scores.shape[0], log_scores.shape[1] - 1
    _matcher_pairs(n1, n2, gt_corr, B, nq)
    stats = torch.empty(B, 2, device=log_scores.device, dtype=torch.float32)
    loss = torch.empty(2, device=log_scores.device, dtype=torch.float32)
    _C.nopesac_matcher_emb_loss(_p(log_scores), _p(gt_corr), _p(n1), _p(n2), B, nq, _p(stats), _p(loss), _stream())
    return stats, loss


def matcher_sinkhorn_train(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, offset_mult, normal_mult, iters: int, gt_corr):
    """matcher_sinkhorn without the assignment, keeping every iteration's potentials for the backward pass ->
    (log_scores [B,nq+1,nq+1], uv [B,iters,2,nq+1], pair_stats [B,2], loss [2]) (the last two as matcher_emb_loss)."""
    B, nq = _matcher_inputs(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, gt_corr)
    f32 = dict(device=desc_dot.device, dtype=torch.float32)
    iters = int(iters)
    out = (torch.empty(B, nq + 1, nq + 1, **f32), torch.empty(B, max(iters, 0), 2, nq + 1, **f32), torch.empty(B, 2, **f32), torch.empty(2, **f32))
    _C.nopesac_matcher_sinkhorn_train(_p(desc_dot), _p(planes1), _p(planes2), _p(cam7), _p(n1), _p(n2), _p(bin_score), float(offset_mult),
                                      float(normal_mult), iters, _p(gt_corr), B, nq, *[_p(t) for t in out], _stream())
    return out


def matcher_sinkhorn_train_backward(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, offset_mult, normal_mult, iters: int, gt_corr, uv,
                                    loss, g_loss):
    """Gradient of loss[0] * g_loss[0] through the unrolled iterations: uv from matcher_sinkhorn_train, loss [2] from it or from
    matcher_emb_loss, g_loss f32[1] -> (d_desc_dot [B,nq,nq], d_bin_pairs [B] = per-pair partials of d bin_score)."""
    B, nq = _matcher_inputs(desc_dot, planes1, planes2, cam7, n1, n2, bin_score, gt_corr)
    iters = int(iters)
    _sized(uv, torch.float32, B * max(iters, 0) * 2 * (nq + 1), "matcher_sinkhorn_train_backward: uv [B,iters,2,nq+1]")
    _sized(loss, torch.float32, 2, "matcher_sinkhorn_train_backward: loss"); _sized(g_loss, torch.float32, 1, "matcher_sinkhorn_train_backward: g_loss")
    d_dots = torch.empty_like(desc_dot)
    d_bin = torch.empty(B, device=desc_dot.device, dtype=torch.float32)
    _C.nopesac_matcher_sinkhorn_train_backward(_p(desc_dot), _p(planes1), _p(planes2), _p(cam7), _p(n1), _p(n2), _p(bin_score), float(offset_mult),
                                               float(normal_mult), iters, _p(gt_corr), _p(uv), _p(loss), _p(g_loss), B, nq, _p(d_dots),
                                               _p(d_bin), _stream())
    return d_dots, d_bin


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int):
    """One torch.optim.AdamW update of `param` and its two moment buffers in place (step counts from 1)."""
    _chk(param, torch.float32)
    n = param.numel()
    _sized(grad, torch.float32, n, "adamw_step: grad"); _sized(exp_avg, torch.float32, n, "adamw_step: exp_avg")
    _sized(exp_avg_sq, torch.float32, n, "adamw_step: exp_avg_sq")
    _C.nopesac_adamw_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, float(lr), float(beta1), float(beta2), float(eps),
                          float(weight_decay), int(step), _stream())


def sgd_step(param, grad, momentum_buf, lr: float, momentum: float, weight_decay: float, first_step: bool):
    """One torch.optim.SGD(momentum) update of `param` and its momentum buffer in place."""
    _chk(param, torch.float32)
    n = param.numel()
    _sized(grad, torch.float32, n, "sgd_step: grad"); _sized(momentum_buf, torch.float32, n, "sgd_step: momentum_buf")
    _C.nopesac_sgd_step(_p(param), _p(grad), _p(momentum_buf), n, float(lr), float(momentum), float(weight_decay), int(first_step), _stream())


def sumsq_accumulate(x: torch.Tensor, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """acc[0] += sum x^2 (one launch per tensor on the same accumulator, fixed order); a new zero accumulator without `acc`."""
    _chk(x, torch.float32)
    if acc is None:
        acc = torch.zeros(1, device=x.device, dtype=torch.float32)
    _sized(acc, torch.float32, 1, "sumsq_accumulate: acc")
    n_ws = int(_C.nopesac_sumsq_workspace_floats(x.numel()))                             # 0: the one-workgroup form, no workspace
    _C.nopesac_sumsq_accumulate_f32(_p(x), x.numel(), _p(acc), _p(scratch(x.device, 4 * n_ws)) if n_ws else None, n_ws, _stream())
    return acc


def clip_coefficient(sumsq: torch.Tensor, max_norm: float) -> torch.Tensor:
    """f32[1] = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)): torch.nn.utils.clip_grad_norm_'s coefficient, on the device."""
    _sized(sumsq, torch.float32, 1, "clip_coefficient: sumsq")
    coef = torch.empty(1, device=sumsq.device, dtype=torch.float32)
    _C.nopesac_clip_coefficient(_p(sumsq), float(max_norm), _p(coef), _stream())
    return coef


def scale_by(x: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """x *= coef[0] in place (coef: a device scalar, e.g. clip_coefficient's)."""
    _chk(x, torch.float32)
    _sized(coef, torch.float32, 1, "scale_by: coef")
    _C.nopesac_scale_by_f32(_p(x), x.numel(), _p(coef), _stream())
    return x


# ---- model-wide optimiser step (csrc/optimizer.hip; nopesac_amd/optim.py) -----------------------------------------------------------------
OPT_CHUNK, OPT_ALIGN, OPT_MAX_GROUPS, OPT_MAX_SEGMENTS = _H.NPS_OPT_CHUNK, _H.NPS_OPT_ALIGN, _H.NPS_OPT_MAX_GROUPS, _H.NPS_OPT_MAX_SEGMENTS
OPT_PRESENT, OPT_FIRST = _H.NPS_OPT_PRESENT, _H.NPS_OPT_FIRST
OPT_MODES = {"ADAMW": _H.NPS_OPT_ADAMW, "SGD": _H.NPS_OPT_SGD}


def opt_unit_map(sizes):
    """The ONE place the layout of the optimiser arenas and the work split of the two kernels are derived: segment sizes (elements, each
    >= 1) -> (offsets int64 [S], units int32 [U, 2] = (segment, chunk index) per workgroup, arena_floats).  Every segment starts at a
    multiple of OPT_ALIGN floats, right behind its predecessor's padded end; it is cut into ceil(n / OPT_CHUNK) units, none of which
    crosses its end.  Host arithmetic only (numpy): what tests/test_model_optimizer_cpu.py proves before a table reaches a GPU."""
    import numpy as np
    sizes = np.asarray(list(sizes), dtype=np.int64).reshape(-1)
    if sizes.size == 0 or sizes.size > OPT_MAX_SEGMENTS or int(sizes.min()) < 1:
        raise OpsArgumentError("opt_unit_map: 1..%d segments of at least one element each, got %d (smallest %s)"
                               % (OPT_MAX_SEGMENTS, sizes.size, sizes.min() if sizes.size else None))
    padded = (sizes + OPT_ALIGN - 1) // OPT_ALIGN * OPT_ALIGN
    offsets = np.concatenate([np.zeros(1, np.int64), np.cumsum(padded)[:-1]])
    chunks = (sizes + OPT_CHUNK - 1) // OPT_CHUNK
    if int(chunks.sum()) >= 2 ** 31:
        raise OpsArgumentError("opt_unit_map: %d units (a grid holds at most 2^31 - 1)" % int(chunks.sum()))
    segment = np.repeat(np.arange(sizes.size, dtype=np.int64), chunks)
    first = np.repeat(np.cumsum(chunks) - chunks, chunks)
    units = np.stack([segment, np.arange(segment.size, dtype=np.int64) - first], axis=1).astype(np.int32)
    return offsets, units, int(padded.sum())


class OptLayout:
    """The static tables of one set of parameters for opt_gather / opt_step, built from LIVE tensors only (data_ptr(), numel()) and kept
    with them: params are f32, contiguous, on one device (any 4-byte alignment: a misaligned one takes the kernels' scalar path) and
    must not be re-seated while the layout lives; `groups[i]` in 0..OPT_MAX_GROUPS-1 is the hyper-parameter group of params[i].
    sources() writes the per-step table into one of two pinned staging buffers, alternated behind an event each, so that an upload
    still in flight is never overwritten, and enqueues its copy on the current stream."""

    def __init__(self, params, groups):
        import numpy as np
        params, groups = list(params), [int(g) for g in groups]
        _require(len(params) == len(groups) and len(params) >= 1, "OptLayout: one group index per parameter, at least one parameter")
        dev = params[0].device
        for i, p in enumerate(params):
            _chk(p, torch.float32)
            _require(p.device == dev and p.numel() >= 1, "OptLayout: parameter %d: empty or on %s, not %s" % (i, p.device, dev))
            _require(0 <= groups[i] < OPT_MAX_GROUPS, "OptLayout: group %d outside 0..%d" % (groups[i], OPT_MAX_GROUPS - 1))
        spans = sorted((p.data_ptr(), p.data_ptr() + 4 * p.numel()) for p in params)
        _require(all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "OptLayout: two parameters share memory")
        self.params, self.device, self.n_groups = params, dev, max(groups) + 1
        self.sizes = np.array([p.numel() for p in params], dtype=np.int64)
        self.offsets, self.units, self.arena_floats = opt_unit_map(self.sizes)
        self.n_segments, self.n_units = len(params), int(self.units.shape[0])
        seg = np.zeros((self.n_segments, 4), dtype=np.int64)                    # nopesac_opt_segment: param, offset, n, (group, reserved)
        seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3] = [p.data_ptr() for p in params], self.offsets, self.sizes, groups
        _require(seg.strides == (ctypes.sizeof(_lib.OptSegment), 8) and self.units.strides == (ctypes.sizeof(_lib.OptUnit), 4)
                 and ctypes.sizeof(_lib.OptSource) == 16, "OptLayout: the header's table rows are not the rows written here")
        self.segments_dev = torch.from_numpy(seg).to(dev)
        self.units_dev = torch.from_numpy(np.ascontiguousarray(self.units)).to(dev)
        self.sources_dev = torch.zeros(self.n_segments, 2, dtype=torch.int64, device=dev)     # nopesac_opt_source: src, (flags, reserved)
        self._staging = [torch.zeros(self.n_segments, 2, dtype=torch.int64).pin_memory() for _ in range(2)]
        self._events = [None, None]
        self._slot = 0

    def arena(self) -> torch.Tensor:
        """A zeroed f32 arena of this layout (G, M1 or M2): torch allocates it, the library allocates nothing."""
        return torch.zeros(self.arena_floats, device=self.device, dtype=torch.float32)

    def view(self, arena: torch.Tensor, i: int) -> torch.Tensor:
        """Segment i of an arena, in the shape of its parameter."""
        o = int(self.offsets[i])
        return arena[o:o + int(self.sizes[i])].view(self.params[i].shape)

    def sources(self, grads, first=None, absent_as_zeros: bool = False) -> torch.Tensor:
        """This step's source table on the device: grads[i] is the gradient of params[i] (f32, contiguous, same element count; kept
        alive by the caller until the gather is enqueued) or None = absent; first[i] marks a segment's first SGD momentum step.
        absent_as_zeros: an absent segment is PRESENT with a null source - the gather fills zeros and the step runs over it."""
        _require(len(grads) == self.n_segments and (first is None or len(first) == self.n_segments), "OptLayout.sources: one entry per parameter")
        self._slot ^= 1
        if self._events[self._slot] is not None:
            self._events[self._slot].synchronize()                              # the upload of two steps ago: long done, never a wait in practice
        host = self._staging[self._slot]
        rows = host.numpy()
        for i, g in enumerate(grads):
            flags = OPT_FIRST if (first is not None and first[i]) else 0
            if g is None:
                rows[i, 0], rows[i, 1] = 0, (flags | OPT_PRESENT) if absent_as_zeros else 0
                continue
            _chk(g, torch.float32)
            if g.numel() != self.sizes[i] or g.device != self.device:
                raise OpsArgumentError("OptLayout.sources: gradient %d: shape %s on %s for a parameter of %d elements on %s"
                                       % (i, tuple(g.shape), g.device, self.sizes[i], self.device))
            rows[i, 0], rows[i, 1] = g.data_ptr(), flags | OPT_PRESENT
        self.sources_dev.copy_(host, non_blocking=True)
        ev = self._events[self._slot] = self._events[self._slot] or torch.cuda.Event()
        ev.record()
        return self.sources_dev

    def _arena(self, t: Optional[torch.Tensor], what: str):
        _require(t is not None, what + ": missing")
        _sized(t, torch.float32, self.arena_floats, what)
        _require(t.device == self.device and t.data_ptr() % 16 == 0, "%s: on %s and 16-byte aligned" % (what, self.device))
        return _p(t)


def opt_gather(layout: OptLayout, sources: torch.Tensor, G: torch.Tensor) -> torch.Tensor:
    """One launch: G[offset_i + j] = grads_i[j] for every present segment, zeros for every absent one (and in the padding)."""
    _sized(sources, torch.int64, 2 * layout.n_segments, "opt_gather: sources")
    _C.nopesac_opt_gather(_p(layout.segments_dev), _p(sources), _p(layout.units_dev), layout.n_segments, layout.n_units,
                          layout._arena(G, "opt_gather: G"), layout.arena_floats, _stream())
    return G


def opt_step(layout: OptLayout, sources: torch.Tensor, G: torch.Tensor, M1: Optional[torch.Tensor], M2: Optional[torch.Tensor],
             coef: Optional[torch.Tensor], optimizer: str, groups, step: int, betas=(0.9, 0.999), eps: float = 1e-8, momentum: float = 0.0):
    """One launch: every present segment's parameter and moments take one AdamW / SGD step from G * coef[0] (coef None: 1) with the
    {lr, weight_decay} of its group - the bits of scale_by followed by adamw_step / sgd_step per tensor.  groups: [(lr, weight_decay)],
    at most OPT_MAX_GROUPS; step counts from 1 (AdamW's bias correction); M1 = exp_avg or the momentum buffer (None for SGD without
    momentum), M2 = exp_avg_sq (None for SGD)."""
    name = str(optimizer).upper()
    if name not in OPT_MODES:
        raise NotImplementedError(f"no optimizer type {optimizer}")           # train_NopeSAC.py:158
    groups = [(float(lr), float(wd)) for lr, wd in groups]
    _require(layout.n_groups <= len(groups) <= OPT_MAX_GROUPS, "opt_step: %d..%d groups, got %d" % (layout.n_groups, OPT_MAX_GROUPS, len(groups)))
    _sized(sources, torch.int64, 2 * layout.n_segments, "opt_step: sources")
    sgd = name == "SGD"
    a = _lib.OptStepArgs()
    a.segments, a.sources, a.units = _p(layout.segments_dev), _p(sources), _p(layout.units_dev)
    a.n_units, a.arena_floats, a.n_segments = layout.n_units, layout.arena_floats, layout.n_segments
    a.G = layout._arena(G, "opt_step: G")
    a.M1 = None if (sgd and float(momentum) == 0.0) else layout._arena(M1, "opt_step: M1")
    a.M2 = None if sgd else layout._arena(M2, "opt_step: M2")
    a.coef = None if coef is None else _p(_sized(coef, torch.float32, 1, "opt_step: coef"))
    _require(coef is None or coef.device == layout.device, "opt_step: coef on another device")
    a.mode, a.n_groups, a.step = OPT_MODES[name], len(groups), int(step)
    a.beta1, a.beta2, a.eps, a.momentum = float(betas[0]), float(betas[1]), float(eps), float(momentum)
    for k, (lr, wd) in enumerate(groups):
        a.groups[k].lr, a.groups[k].weight_decay = lr, wd
    _C.nopesac_opt_step(ctypes.byref(a), _stream())


# ---- set criterion of the plane head (csrc/plane_criterion.hip) --------------------------------------------------------------------------
PLANE_MAX_QUERIES, PLANE_MAX_TARGETS, PLANE_MAX_LAYERS = _lib.H.NPS_PLANE_MAX_QUERIES, _lib.H.NPS_PLANE_MAX_TARGETS, _lib.H.NPS_PLANE_MAX_LAYERS
PLANE_MAX_GROUPS = _lib.H.NPS_PLANE_MAX_GROUPS
PLANE_COST_NAMES = ("cost_class", "cost_mask", "cost_dice", "cost_center", "cost_param", "cost_offset", "cost_angle")


def plane_targets(masks: torch.Tensor, n_host: torch.Tensor, n: torch.Tensor):
    """prepare_targets (siamese_planeTR.py:498-504): masks uint8 [B, nmax, H, W], n int32 [B] on the host and on the device -> plane_centers
    [B, nmax, 2] (centroid of (x / W, y / H) per mask) and pixel_centers [B, 2, H, W] (sum of centre x mask)."""
    _chk(masks, torch.uint8); _chk(n, torch.int32)
    _require(n_host.dtype == torch.int32 and not n_host.is_cuda and n_host.is_contiguous(), "n_host: contiguous int32 on the host")
    B, nmax, H, W = masks.shape
    centers = torch.empty(B, nmax, 2, device=masks.device, dtype=torch.float32)
    pixel = torch.empty(B, 2, H, W, device=masks.device, dtype=torch.float32)
    _C.nopesac_plane_targets(_p(masks), n_host.data_ptr(), _p(n), B, nmax, H, W, _p(centers), _p(pixel), _stream())
    return centers, pixel


class PlaneCriterionCall:
    """One argument block (nopesac_plane_criterion) for the cost, loss and gradient entries, filled from tensors that it keeps alive.
    preds: pred_logits [L*B, nq, 2], pred_mask_logits [L*B, nq, h, w] in ANY dense stride order, pred_centers [L*B, nq, 2], pred_params
    [L*B, nq, 3], pixel_centers [B, 2, h, w] (any dense stride order) or None; targets: masks, n, n_host, plane_centers, plane_params,
    pixel_centers, depth, k_inv_dot_xy1.  groups = G view groups of B / G consecutive batch elements each (the header's `groups`): the
    losses become [G, 6 L + 2], num_masks a float for every group or a sequence of G floats; groups=1 is the ungrouped call."""

    def __init__(self, L: int, preds: dict, targets: dict, weights: dict, num_masks=0.0, groups: int = 1):
        lg, ml, ce, pa, px = (preds.get(k) for k in ("pred_logits", "pred_mask_logits", "pred_centers", "pred_params", "pixel_centers"))
        for t in (lg, ce, pa, targets["plane_centers"], targets["plane_params"], targets["pixel_centers"], targets["depth"], targets["k_inv_dot_xy1"]):
            _chk(t, torch.float32)
        _chk(targets["masks"], torch.uint8); _chk(targets["n"], torch.int32)
        nh = targets["n_host"]
        _require(nh.dtype == torch.int32 and not nh.is_cuda and nh.is_contiguous(), "n_host: contiguous int32 on the host")
        LB, nq, h, w = ml.shape
        B, nmax, H, W = targets["masks"].shape
        _require(LB == L * B and ml.dtype == torch.float32 and lg.shape == (LB, nq, 2) and ce.shape == (LB, nq, 2) and pa.shape == (LB, nq, 3),
                 (ml.shape, lg.shape, ce.shape, pa.shape))
        _require(px is None or (px.shape == (B, 2, h, w) and px.dtype == torch.float32), "pixel_centers")
        G = int(groups)
        _require(1 <= G <= PLANE_MAX_GROUPS and B % G == 0, "groups=%d: 1..%d groups that divide B=%d" % (G, PLANE_MAX_GROUPS, B))
        per_group = isinstance(num_masks, (list, tuple)) or getattr(num_masks, "ndim", 0) == 1          # else one value (or None / 0: the default)
        if per_group:
            num_masks = [float(v) for v in num_masks]
            _require(len(num_masks) == G, "num_masks: %d values for %d groups" % (len(num_masks), G))
        dev = ml.device
        self.keep = (preds, targets)
        self.dims = (L, B, nq, nmax, h, w, H, W)
        self.groups = G
        self.ml, self.px = ml, px
        f32 = dict(device=dev, dtype=torch.float32)
        ws_floats = int(_C.nopesac_plane_criterion_workspace_floats(L, B, nq, nmax, h, w))
        self.ws = torch.empty(max(ws_floats, 1), **f32)
        self.cost = torch.empty(LB, nq, nmax, **f32)
        self.match_q = torch.empty(LB, nmax, device=dev, dtype=torch.int32)
        self.match_gt = torch.empty(LB, nq, device=dev, dtype=torch.int32)
        self.losses = torch.empty(6 * L + 2, **f32) if G == 1 else torch.empty(G, 6 * L + 2, **f32)
        self.mask_stats = torch.empty(LB, nmax, 4, **f32)
        self.q_valid = torch.empty(B, H, W, device=dev, dtype=torch.uint8)
        self.q_stats = torch.empty(B, 2, **f32)
        a = self.args = _lib.PlaneCriterionArgs()
        a.pred_logits, a.pred_mask_logits, a.pred_centers, a.pred_params, a.pixel_centers = _p(lg), _p(ml), _p(ce), _p(pa), _p(px)
        a.ml_stride_i, a.ml_stride_q, a.ml_stride_y, a.ml_stride_x = ml.stride()
        if px is not None:
            a.pc_stride_b, a.pc_stride_c, a.pc_stride_y, a.pc_stride_x = px.stride()
        a.masks, a.n, a.n_host = _p(targets["masks"]), _p(targets["n"]), nh.data_ptr()
        a.tgt_centers, a.tgt_params, a.tgt_pixel_centers = _p(targets["plane_centers"]), _p(targets["plane_params"]), _p(targets["pixel_centers"])
        a.depth, a.k_inv_dot_xy1 = _p(targets["depth"]), _p(targets["k_inv_dot_xy1"])
        a.L, a.B, a.nq, a.nmax, a.h, a.w, a.H, a.W, a.num_classes = L, B, nq, nmax, h, w, H, W, lg.shape[-1]
        for k in PLANE_COST_NAMES:
            setattr(a, k, float(weights[k]))
        a.eos_coef, a.num_masks, a.groups = float(weights["eos_coef"]), (0.0 if per_group else float(num_masks or 0.0)), G
        if per_group:
            self.num_masks_groups = (ctypes.c_float * G)(*num_masks)           # read on the host at every launch: kept alive here
            a.num_masks_groups = ctypes.addressof(self.num_masks_groups)
        a.cost, a.match_q, a.match_gt = _p(self.cost), _p(self.match_q), _p(self.match_gt)
        a.losses, a.mask_stats, a.q_valid, a.q_stats = _p(self.losses), _p(self.mask_stats), _p(self.q_valid), _p(self.q_stats)
        a.ws, a.ws_floats = _p(self.ws), ws_floats


def plane_match_costs(call: PlaneCriterionCall) -> torch.Tensor:
    """The matcher's cost matrices [L*B, nq, nmax] (matcher.py:98-163)."""
    _C.nopesac_plane_match_costs(ctypes.byref(call.args), _stream())
    return call.cost


def plane_assign(call: PlaneCriterionCall):
    """Linear sum assignment of call.cost on the device -> (match_q int32 [L*B, nmax], match_gt int32 [L*B, nq])."""
    L, B, nq, nmax = call.dims[:4]
    _C.nopesac_plane_assign(_p(call.cost), call.args.n_host, call.args.n, L, B, nq, nmax, _p(call.match_q), _p(call.match_gt), _stream())
    return call.match_q, call.match_gt


def plane_losses(call: PlaneCriterionCall) -> torch.Tensor:
    """The unweighted losses [6 L + 2] ([G, 6 L + 2] of a grouped call) for call.match_q / call.match_gt (criterion.py)."""
    _C.nopesac_plane_losses(ctypes.byref(call.args), _stream())
    return call.losses


def plane_losses_backward(call: PlaneCriterionCall, g_losses: torch.Tensor):
    """Gradients of sum(g_losses * losses) -> (d_logits, d_mask_logits, d_centers, d_params, d_pixel_centers or None), the mask and centre-map
    gradients in the stride order of the inputs."""
    _chk(g_losses, torch.float32)
    L, B, nq = call.dims[:3]
    _require(g_losses.numel() == call.groups * (6 * L + 2), g_losses.shape)
    f32 = dict(device=call.ml.device, dtype=torch.float32)
    d_lg, d_ce, d_pa = torch.empty(L * B, nq, 2, **f32), torch.empty(L * B, nq, 2, **f32), torch.empty(L * B, nq, 3, **f32)
    d_ml = torch.empty_strided(call.ml.shape, call.ml.stride(), **f32)
    d_px = None if call.px is None else torch.empty_strided(call.px.shape, call.px.stride(), **f32)
    a = call.args
    a.g_losses, a.d_logits, a.d_mask_logits, a.d_centers, a.d_params, a.d_pixel_centers = _p(g_losses), _p(d_lg), _p(d_ml), _p(d_ce), _p(d_pa), _p(d_px)
    _C.nopesac_plane_losses_backward(ctypes.byref(a), _stream())
    return d_lg, d_ml, d_ce, d_pa, d_px


def plane_corr_matrix(gt_corrs: torch.Tensor, match1: torch.Tensor, match2: torch.Tensor, nq: int) -> torch.Tensor:
    """process_plane_corr_matrix (siamese_planeTR.py:566-623): gt_corrs int32 [B, K, 2] (rows padded with -1), match1 / match2 int32 [B, nmax]
    (query of each gt plane in the two views) -> uint8 [B, nq+1, nq+1] with the dustbin row and column."""
    _chk(gt_corrs, torch.int32); _chk(match1, torch.int32); _chk(match2, torch.int32)
    B, K, _ = gt_corrs.shape
    _require(match1.shape == match2.shape and match1.shape[0] == B, (match1.shape, match2.shape))
    out = torch.empty(B, nq + 1, nq + 1, device=gt_corrs.device, dtype=torch.uint8)
    _C.nopesac_plane_corr_matrix(_p(gt_corrs), K, _p(match1), _p(match2), B, nq, match1.shape[1], _p(out), _stream())
    return out


# ---------------------------------------------------------------- the plane head's outputs in front of the two-view heads (csrc/two_view_train.hip)
def ransac_score_maps_backward_geo(geo_local, rot_raw, trans_raw, init_rot, init_trans, m, g_normal_score, g_param_score, g_l2_dist):
    """The cotangent of ransac_score_maps that ransac_score_maps_backward leaves out: the gradients of normal_score / param_score / l2_dist
    [B,nq+1,nq] -> g_geo_local [B,nq,6] (exact zeros in rows j >= m)."""
    _chk(geo_local, torch.float32)
    _require(geo_local.dim() == 3 and geo_local.shape[2] == 6, "ransac_score_maps_backward_geo: geo_local [B,nq,6]")
    B, nq, _ = geo_local.shape
    _sized(rot_raw, torch.float32, B * nq * 4, "ransac_score_maps_backward_geo: rot_raw")
    _sized(trans_raw, torch.float32, B * nq * 3, "ransac_score_maps_backward_geo: trans_raw")
    _sized(init_rot, torch.float32, B * 4, "ransac_score_maps_backward_geo: init_rot")
    _sized(init_trans, torch.float32, B * 3, "ransac_score_maps_backward_geo: init_trans")
    _sized(m, torch.int32, B, "ransac_score_maps_backward_geo: m")
    for t in (g_normal_score, g_param_score, g_l2_dist):
        _sized(t, torch.float32, B * (nq + 1) * nq, "ransac_score_maps_backward_geo: score gradient [B,nq+1,nq]")
    out = torch.empty(B, nq, 6, device=geo_local.device, dtype=torch.float32)
    _C.nopesac_refine_score_maps_backward_geo(_p(geo_local), _p(rot_raw), _p(trans_raw), _p(init_rot), _p(init_trans), _p(m), B, nq,
                                              _p(g_normal_score), _p(g_param_score), _p(g_l2_dist), _p(out), _stream())
    return out


def geo_sequence_backward(assignment, planes1, planes2, n1, n2, init_trans, init_rot, g_geo_local, g_geo_enc, warp_in_ref=True):
    """Backward of geo_sequence with respect to the planes: g_geo_local [B,nq,6], g_geo_enc [B,nq,8] -> (g_planes1, g_planes2) [B,nq,3]
    (exact zeros for unmatched planes and planes at or beyond n1 / n2; the pose is a constant)."""
    _chk(assignment, torch.float32)
    _require(assignment.dim() == 3 and assignment.shape[1] == assignment.shape[2], "geo_sequence_backward: assignment [B,nq,nq]")
    B, nq, _ = assignment.shape
    _sized(planes1, torch.float32, B * nq * 3, "geo_sequence_backward: planes1")
    _sized(planes2, torch.float32, B * nq * 3, "geo_sequence_backward: planes2")
    _sized(n1, torch.int32, B, "geo_sequence_backward: n1")
    _sized(n2, torch.int32, B, "geo_sequence_backward: n2")
    _sized(init_trans, torch.float32, B * 3, "geo_sequence_backward: init_trans")
    _sized(init_rot, torch.float32, B * 4, "geo_sequence_backward: init_rot")
    _sized(g_geo_local, torch.float32, B * nq * 6, "geo_sequence_backward: g_geo_local")
    _sized(g_geo_enc, torch.float32, B * nq * 8, "geo_sequence_backward: g_geo_enc")
    f32 = dict(device=assignment.device, dtype=torch.float32)
    out = (torch.empty(B, nq, 3, **f32), torch.empty(B, nq, 3, **f32))
    _C.nopesac_geo_sequence_backward(_p(assignment), _p(planes1), _p(planes2), _p(n1), _p(n2), _p(init_trans), _p(init_rot), B, nq,
                                     int(bool(warp_in_ref)), _p(g_geo_local), _p(g_geo_enc), _p(out[0]), _p(out[1]), _stream())
    return out


def match_compact(x, params, match_q, n, check: bool = False):
    """The matched queries of every image to the front, in ascending query index: x [N,nq,256], params [N,nq,3], match_q int32 [N,nmax],
    n int32 [N] -> (x_c, params_c, order int32 [N,nq], rank int32 [N,nq], bad int32 [N]); rows behind n[i] are zeros, order / rank are -1
    where nothing lies.  An image whose input breaks the contract (an index outside [0,nq), a query named twice, n[i] outside
    [0, min(nq,nmax)]) is compacted as n[i] = 0 and flagged in `bad`: read it at a sync the caller already pays (match_compact_check), or
    pass check=True to raise ValueError here (one host sync)."""
    _chk(x, torch.float32)
    _require(x.dim() == 3 and x.shape[2] == 256, "match_compact: x [N,nq,256]")
    N, nq, _ = x.shape
    _sized(params, torch.float32, N * nq * 3, "match_compact: params [N,nq,3]")
    _chk(match_q, torch.int32)
    _require(match_q.dim() == 2 and match_q.shape[0] == N, "match_compact: match_q [N,nmax]")
    _sized(n, torch.int32, N, "match_compact: n")
    dev = x.device
    x_c, params_c = torch.empty(N, nq, 256, device=dev, dtype=torch.float32), torch.empty(N, nq, 3, device=dev, dtype=torch.float32)
    order, rank = torch.empty(N, nq, device=dev, dtype=torch.int32), torch.empty(N, nq, device=dev, dtype=torch.int32)
    bad = torch.empty(N, device=dev, dtype=torch.int32)
    _C.nopesac_match_compact(_p(x), _p(params), _p(match_q), _p(n), N, nq, match_q.shape[1], _p(x_c), _p(params_c), _p(order), _p(rank),
                             _p(bad), _stream())
    if check:
        match_compact_check(bad)
    return x_c, params_c, order, rank, bad


def match_compact_check(bad: torch.Tensor):
    """ValueError if match_compact flagged an image (reads `bad` on the host)."""
    flagged = torch.nonzero(bad).flatten().tolist()
    if flagged:
        raise ValueError("match_compact: match_q / n of image(s) %s break the contract (index outside [0,nq), a query named twice, or n "
                         "outside [0, min(nq,nmax)])" % flagged)


def match_compact_backward(g_x_c, rank):
    """The scatter back of match_compact: g_x_c [N,nq,256], rank int32 [N,nq] -> g_x [N,nq,256] (zero rows for unmatched queries)."""
    _chk(g_x_c, torch.float32)
    _require(g_x_c.dim() == 3 and g_x_c.shape[2] == 256, "match_compact_backward: g_x_c [N,nq,256]")
    N, nq, _ = g_x_c.shape
    _sized(rank, torch.int32, N * nq, "match_compact_backward: rank [N,nq]")
    out = torch.empty_like(g_x_c)
    _C.nopesac_match_compact_backward(_p(g_x_c), _p(rank), N, nq, _p(out), _stream())
    return out


def corr_compact(gt_corr, order1, order2, n1, n2):
    """gt_corr uint8 [B,nq+1,nq+1] (plane_corr_matrix) gathered through both views' `order` of match_compact, the dustbin index mapped to
    itself; entries outside the live block [n1, n2] (plus dustbins) are zero."""
    _chk(gt_corr, torch.uint8)
    _require(gt_corr.dim() == 3 and gt_corr.shape[1] == gt_corr.shape[2] and gt_corr.shape[1] >= 2, "corr_compact: gt_corr [B,nq+1,nq+1]")
    B, nq = gt_corr.shape[0], gt_corr.shape[1] - 1
    _sized(order1, torch.int32, B * nq, "corr_compact: order1 [B,nq]")
    _sized(order2, torch.int32, B * nq, "corr_compact: order2 [B,nq]")
    _sized(n1, torch.int32, B, "corr_compact: n1")
    _sized(n2, torch.int32, B, "corr_compact: n2")
    out = torch.empty_like(gt_corr)
    _C.nopesac_corr_compact(_p(gt_corr), _p(order1), _p(order2), _p(n1), _p(n2), B, nq, _p(out), _stream())
    return out


# ---------------------------------------------------------------- backward of the plane head's instance heads (csrc/plane_head_bwd.hip)
def sigmoid_backward(g: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """g y (1 - y) for the output y of a sigmoid and its gradient g."""
    _chk(g, torch.float32)
    _sized(y, torch.float32, g.numel(), "sigmoid_backward: y")
    out = torch.empty_like(g)
    _C.nopesac_sigmoid_backward_f32(_p(g), _p(y), g.numel(), _p(out), _stream())
    return out


def mask_product_splits(L: int, B: int, nq: int, hw: int, center_rows: int = 0) -> int:
    """Pixel-range count of mask_product_backward's wgrad launch: about 512 workgroups over the (128-row tile, image) pairs, at least
    256 pixels per range."""
    tiles = -(-(L * nq + center_rows) // 128) * B
    return max(1, min(64, -(-512 // tiles), hw // 256))


def mask_product_workspace_floats(L: int, B: int, nq: int, center_rows: int, splits: int) -> int:
    """The library's nopesac_mask_product_wgrad_workspace_floats, what the wgrad launcher checks against."""
    return int(_C.nopesac_mask_product_wgrad_workspace_floats(L, B, nq, center_rows, splits))


def mask_product_backward(d_logits: torch.Tensor, fold: torch.Tensor, p1: torch.Tensor, d_center: Optional[torch.Tensor] = None,
                          w_center: Optional[torch.Tensor] = None, *, splits: Optional[int] = None, d_fold: Optional[torch.Tensor] = None,
                          d_beta: Optional[torch.Tensor] = None, which: str = "both"):
    """Backward of the folded mask product M[l,b,q,p] = sum_k fold[l,b,q,k] p1[b,p,k] + beta[l,b,q] (+ the 256 -> 2 pixel-centre conv
    Z = w_center p1 + b_center joined as two shared rows per image).  d_logits [L, B, nq, h, w] f32 contiguous (pixel-minor: what
    plane_losses_backward returns for a contiguous input), fold = the L*B*nq rows [.., 256] (unit column stride, rows may be a column
    slice of a wider matrix), p1 [B, h, w, 256] pixel-dense NHWC (may be a channel slice), d_center [B, 2, h, w] = the gradient in
    front of the centre map's sigmoid with w_center [2, 256], or both None
    -> (d_fold [L, B, nq, 256], d_beta [L, B, nq], d_p1 [B, h, w, 256]) and, with the centre rows, (+ d_w_center [2, 256], d_b_center [2]).
    d_fold / d_beta: optional outputs (column slices of one wider gradient matrix).  which = "wgrad" / "dgrad": only that launch (the
    other outputs are None).  Two launches + the fixed-order reduction; the partial tiles live in scratch()."""
    _chk(d_logits, torch.float32)
    _chk(p1, torch.float32, contiguous=False)
    _require(d_logits.dim() == 5 and p1.dim() == 4, "mask_product_backward: d_logits [L,B,nq,h,w], p1 [B,h,w,256]")
    _require(which in ("both", "wgrad", "dgrad"), which)
    L, B, nq, h, w = d_logits.shape
    _require(p1.shape[:3] == (B, h, w) and p1.stride(3) == 1 and p1.stride(1) == w * p1.stride(2),
             "mask_product_backward: p1 [B,h,w,C] with unit channel stride and dense rows; got %s, strides %s" % (tuple(p1.shape), tuple(p1.stride())))
    C = p1.shape[3]
    rows = L * B * nq
    _chk(fold, torch.float32, contiguous=False)
    fold2 = fold.reshape(rows, fold.shape[-1]) if fold.dim() != 2 else fold
    fold_ld = _rows(fold2, rows, C, "mask_product_backward: fold")
    _require(fold2.shape[1] == C, "mask_product_backward: fold must have %d columns" % C)
    _require((d_center is None) == (w_center is None), "mask_product_backward: d_center and w_center go together")
    extra = 0
    if d_center is not None:
        _sized(d_center, torch.float32, B * 2 * h * w, "mask_product_backward: d_center")
        _sized(w_center, torch.float32, 2 * C, "mask_product_backward: w_center")
        extra = 2
    dev = p1.device
    f32 = dict(device=dev, dtype=torch.float32)
    out_f = out_b = d_p1 = d_wc = d_bc = None
    if which != "dgrad":
        out_f = torch.empty(L, B, nq, C, **f32) if d_fold is None else d_fold
        out_b = torch.empty(L, B, nq, **f32) if d_beta is None else d_beta
        of2 = out_f.view(rows, C) if out_f.dim() != 2 else out_f
        ob = out_b.view(rows) if out_b.dim() != 1 else out_b
        of_ld = _rows(of2, rows, C, "mask_product_backward: d_fold")
        _chk(ob, torch.float32, contiguous=False)
        _require(ob.shape == (rows,) and ob.stride(0) >= 1, "mask_product_backward: d_beta")
        if extra:
            d_wc, d_bc = torch.empty(2, C, **f32), torch.empty(2, **f32)
        S = int(splits or mask_product_splits(L, B, nq, h * w, extra))
        ws = scratch(dev, 4 * mask_product_workspace_floats(L, B, nq, extra, S))
        _C.nopesac_mask_product_wgrad_f32(_p(d_logits), _p(d_center), _p(p1), _p(of2), of_ld, _p(ob), ob.stride(0), _p(d_wc), _p(d_bc), _p(ws),
                                          ws.numel(), L, B, nq, h, w, C, p1.stride(2), p1.stride(0), S, _stream())
    if which != "wgrad":
        d_p1 = torch.empty(B, h, w, C, **f32)
        _C.nopesac_mask_product_dgrad_f32(_p(d_logits), _p(d_center), _p(fold2), fold_ld, _p(w_center), _p(d_p1), L, B, nq, h, w, C,
                                          d_p1.stride(2), d_p1.stride(0), _stream())
    if extra:
        return out_f, out_b, d_p1, d_wc, d_bc
    return out_f, out_b, d_p1


# ---------------------------------------------------------------- training kernels of the plane head's decoder (csrc/decoder_train.hip)
ATT_TRAIN_TQ, ATT_TRAIN_TK = _H.NPS_ATT_TRAIN_TQ, _H.NPS_ATT_TRAIN_TK        # query rows per workgroup / keys per LDS tile


def dropout_stream(step: int, layer: int, site: int) -> int:
    """The counter stream of one dropout site of the decoder: step * 64 + layer * 8 + site, site 0 .. 5 = self-attention probabilities,
    dropout1, cross-attention probabilities, dropout2, FFN inner, dropout3."""
    _require(0 <= site < 6 and 0 <= layer < 8 and step >= 0, "dropout_stream: step >= 0, layer 0..7, site 0..5")
    return int(step) * 64 + int(layer) * 8 + int(site)


def dropout_keep_mask(shape, p: float, seed: int, stream: int, device=None) -> torch.Tensor:
    """uint8 tensor of `shape`: 1 where the counter-based dropout (csrc/dropout.h) keeps the element of that row-major index at rate p
    under (seed, stream), else 0 - the decision every kernel here recomputes, materialised.  p outside [0, 1) raises HipKernelError."""
    shape = tuple(int(s) for s in shape)
    out = torch.empty(shape, device=device if device is not None else torch.device("cuda", torch.cuda.current_device()), dtype=torch.uint8)
    _C.nopesac_dropout_keep_mask(_p(out), out.numel(), float(p), int(seed), int(stream), _stream())
    return out


def dropout(x: torch.Tensor, p: float, seed: int, stream: int, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """keep ? x / (1 - p) : 0 [+ residual] on a dense f32 tensor, the element's row-major index as the counter.  Without a residual the
    same call on the gradient is the backward."""
    _chk(x, torch.float32)
    if residual is not None:
        _sized(residual, torch.float32, x.numel(), "dropout: residual")
    y = torch.empty_like(x)
    _C.nopesac_dropout_f32(_p(x), _p(residual), _p(y), x.numel(), float(p), int(seed), int(stream), _stream())
    return y


def attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, B: int, Lq: int, Lk: int, heads: int, scale: float, qlen=None, klen=None,
                    *, p: float = 0.0, seed: int = 0, stream: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """attention (f32, head dim 32) for any Lq, Lk, tiled over the keys, with dropout on the probabilities:
    o = (keep o softmax(s)) v / (1 - p), keep from the counter at the index in [B, heads, Lq, Lk].  q / k / v / out may be column slices."""
    W = heads * 32
    sq, sk, sv = _rows(q, B * Lq, W, "attention_train: q"), _rows(k, B * Lk, W, "attention_train: k"), _rows(v, B * Lk, W, "attention_train: v")
    _lengths(qlen, B, "attention_train: qlen"); _lengths(klen, B, "attention_train: klen")
    o = torch.empty(B * Lq, W, device=q.device, dtype=torch.float32) if out is None else out
    so = _rows(o, B * Lq, W, "attention_train: out")
    _C.nopesac_attention_train_forward(_p(q), sq, _p(k), sk, _p(v), sv, _p(o), so, B, Lq, Lk, heads, float(scale), _p(qlen), _p(klen), float(p),
                                       int(seed), int(stream), _stream())
    return o


def attention_train_backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_out: torch.Tensor, B: int, Lq: int, Lk: int, heads: int,
                             scale: float, qlen=None, klen=None, *, p: float = 0.0, seed: int = 0, stream: int = 0, out=None):
    """Backward of attention_train (and, at p = 0, of attention) for any Lq, Lk: -> (dq, dk, dv).  Softmax statistics and the dropout mask
    are recomputed; nothing of the forward launch is needed.  Strides as attention_backward."""
    W = heads * 32
    sq, sk, sv = (_rows(q, B * Lq, W, "attention_train_backward: q"), _rows(k, B * Lk, W, "attention_train_backward: k"),
                  _rows(v, B * Lk, W, "attention_train_backward: v"))
    sg = _rows(d_out, B * Lq, W, "attention_train_backward: d_out")
    _lengths(qlen, B, "attention_train_backward: qlen"); _lengths(klen, B, "attention_train_backward: klen")
    if out is None:
        out = tuple(torch.empty(rows, W, device=q.device, dtype=torch.float32) for rows in (B * Lq, B * Lk, B * Lk))
    dq, dk, dv = out
    so = [_rows(t, rows, W, "attention_train_backward: out") for t, rows in ((dq, B * Lq), (dk, B * Lk), (dv, B * Lk))]
    ws = scratch(q.device, 4 * int(_C.nopesac_attention_train_backward_workspace_floats(B, heads, Lq)))
    _C.nopesac_attention_train_backward(_p(q), sq, _p(k), sk, _p(v), sv, _p(d_out), sg, B, Lq, Lk, heads, float(scale), _p(qlen), _p(klen),
                                        float(p), int(seed), int(stream), _p(dq), so[0], _p(dk), so[1], _p(dv), so[2], _p(ws), ws.numel(),
                                        _stream())
    return dq, dk, dv


# ---------------------------------------------------------------- Linear backward with the operands read in place (csrc/linear_bwd.hip)
LINEAR_BWD_TILE, LINEAR_BWD_STAGE = _H.NPS_LINEAR_BWD_TILE, _H.NPS_LINEAR_BWD_STAGE       # output tile edge / rows of M per LDS stage


def encoder_dropout_stream(step: int, layer: int, site: int) -> int:
    """The counter stream of one dropout site of the plane head's encoder: -(step * 32 + layer * 4 + site) - 1, site 0 .. 3 = attention
    probabilities, dropout1, FFN inner, dropout2.  Negative, so disjoint from every decoder stream (dropout_stream >= 0) under one seed."""
    _require(0 <= site < 4 and 0 <= layer < 8 and step >= 0, "encoder_dropout_stream: step >= 0, layer 0..7, site 0..3")
    return -(int(step) * 32 + int(layer) * 4 + int(site)) - 1


def linear_backward_splits(M: int, K: int, N: int) -> int:
    """Row-range count of linear_backward's dW / db launch: about 512 workgroups over the 128 x 128 tiles of dW, at least 256 rows each."""
    tiles = -(-N // LINEAR_BWD_TILE) * -(-K // LINEAR_BWD_TILE)
    return max(1, min(256, -(-512 // tiles), M // 256))


def linear_backward(x: Optional[torch.Tensor], w: torch.Tensor, g: torch.Tensor, *, y: Optional[torch.Tensor] = None, p: float = 0.0,
                    seed: int = 0, stream: int = 0, want=(True, True, True), dx: Optional[torch.Tensor] = None,
                    splits: Optional[int] = None, ws: Optional[torch.Tensor] = None):
    """Backward of y = act(x W^T + b): x [M, K], w [N, K] dense, g [M, N] the gradient at the output -> (dx [M, K], dw [N, K], db [N]),
    None where `want` = (dx, dw, db) says no.  The gradient is gated as it is loaded: y (the saved output) = the ReLU's y > 0; p > 0 = the
    counter-based dropout behind the Linear at the row-major index in [M, N] under (seed, stream), times 1 / (1 - p).  x, g, y and the
    optional output `dx` may be column slices of wider row-major buffers; nothing is copied or transposed.  Deterministic.  `splits` /
    `ws`: the row-range count of the dW / db launch and its workspace (default: linear_backward_splits, scratch())."""
    _require(g.dim() == 2 and w.dim() == 2, "linear_backward: g [M, N], w [N, K]")
    M, N = g.shape
    K = w.shape[1]
    _require(w.shape[0] == N, "linear_backward: w [%d, K] expected, got %s" % (N, tuple(w.shape)))
    _chk(w, torch.float32)
    gs = _rows(g, M, N, "linear_backward: g")
    want_dx, want_dw, want_db = (bool(t) for t in want)
    xs = ys = ds = 0
    if want_dw:
        _require(x is not None and x.dim() == 2 and x.shape[1] == K, "linear_backward: x [M, %d] expected" % K)
        xs = _rows(x, M, K, "linear_backward: x")
    if y is not None:
        _require(y.dim() == 2 and y.shape[1] == N, "linear_backward: y [M, %d] expected" % N)
        ys = _rows(y, M, N, "linear_backward: y")
    f32 = dict(device=g.device, dtype=torch.float32)
    if want_dx:
        if dx is None:
            dx = torch.empty(M, K, **f32)
        _require(dx.dim() == 2 and dx.shape[1] == K, "linear_backward: dx [M, %d] expected" % K)
        ds = _rows(dx, M, K, "linear_backward: dx")
    else:
        dx = None
    dw = torch.empty(N, K, **f32) if want_dw else None
    db = torch.empty(N, **f32) if want_db else None
    S = int(splits or linear_backward_splits(M, K, N))
    n_ws = 0
    if want_dw or want_db:
        if ws is None:
            ws = scratch(g.device, 4 * int(_C.nopesac_linear_backward_workspace_floats(N, K, S)))
        _chk(ws, torch.float32)
        n_ws = ws.numel()
    else:
        ws = None
    _C.nopesac_linear_backward_f32(_p(x) if want_dw else None, xs, _p(w), _p(g), gs, _p(y), ys, float(p), int(seed), int(stream), _p(dx), ds, _p(dw),
                                   _p(db), _p(ws), n_ws, M, K, N, S, _stream())
    return dx, dw, db
