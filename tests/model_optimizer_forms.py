"""The model-wide optimiser (nopesac_amd/optim.py, csrc/optimizer.hip) as data: the segment sizes at which the two kernels change path,
toy trainers whose keys reach every optimiser group, parameters and gradients that lie inside larger prefilled buffers (aligned and
one float off), a numpy restatement of the kernels' index arithmetic, and float64 restatements of a clipped model step built on
tests/stream_forms.py (whose references, floors and FLOOR_FACTOR are the project's rule: docs/kernels.md "Stream sweep").
Imports without a GPU."""
from __future__ import annotations

import numpy as np
import torch

from tests import stream_forms as S

F64, F32 = torch.float64, torch.float32
CHUNK, ALIGN, THREADS = 4096, 64, 256        # include/nopesac_hip.h NPS_OPT_CHUNK / NPS_OPT_ALIGN, the kernels' workgroup
# the chunk (4095 / 4096 / 4097, 2 chunks + 5), float4 (1, 3, 255 / 256 / 257) and sumsq one-workgroup (16385) boundaries
SIZES = (1, 3, 255, 256, 257, 4095, 4096, 4097, 2 * 4096 + 5, 16385)
EMBED_KEY, NORM_KEY = "sem_seg_head.query_embed.weight", "sem_seg_head.context2plane_decoder.norm.weight"
LANES = np.arange(4)
GUARD, PAD = 12345.0, 8                      # the prefill of the surrounding buffers; floats of guard on either side (a multiple of 4)


def key_for(i: int) -> str:
    """A state-dict key for toy tensor i such that every run of three tensors holds a plain, a norm and an embedding key."""
    if i % 3 == 1:
        return NORM_KEY if i == 1 else "sem_seg_head.context2plane_decoder.layers.%d.norm1.weight" % i
    if i % 3 == 2:
        return EMBED_KEY if i == 2 else "sem_seg_head.query_embed.w%d" % i
    return "toy.w%d" % i


def solver_cfg(*pairs):
    """The default solver with every optimiser group and multiplier told apart; `pairs`: further KEY, value overrides."""
    from nopesac_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.OPTIMIZER", "ADAMW", "SOLVER.BASE_LR", 0.01, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.WEIGHT_DECAY_NORM", 0.5,
                         "SOLVER.WEIGHT_DECAY_EMBED", 0.25, "SOLVER.BACKBONE_MULTIPLIER", 0.1] + list(pairs))
    return cfg


def toy_classes():
    from nopesac_amd.training import HeadTrainer

    class BackboneToy(HeadTrainer):
        LR_MULTIPLIER = "BACKBONE_MULTIPLIER"
    return HeadTrainer, BackboneToy


def values(n: int, seed: int) -> torch.Tensor:
    return S.randn(S.gen(7000 + 131 * seed + n), n).float()


def guarded(t: torch.Tensor, device, misalign: bool = False):
    """-> (buffer, view): a copy of t (flat) inside a larger buffer prefilled with GUARD, PAD floats in front and behind; with
    `misalign` the view starts one float off a 16-byte boundary."""
    off = PAD + (1 if misalign else 0)
    buf = torch.full((t.numel() + 2 * PAD + 1,), GUARD, dtype=F32, device=device)
    view = buf[off:off + t.numel()]
    view.copy_(t.reshape(-1))
    assert (view.data_ptr() % 16 != 0) == misalign
    return buf, view


def guards_intact(buf: torch.Tensor, n: int, misalign: bool = False) -> bool:
    off = PAD + (1 if misalign else 0)
    b = buf.cpu()
    return bool((b[:off] == GUARD).all()) and bool((b[off + n:] == GUARD).all())


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.detach().cpu().contiguous().reshape(-1), b.detach().cpu().contiguous().reshape(-1)
    return a.shape == b.shape and bool((a.view(torch.int32) == b.view(torch.int32)).all())


def padding_is_zero(layout, arena: torch.Tensor) -> bool:
    """Every float of an arena outside the live slices [offset, offset + n) is +0."""
    live = torch.zeros(layout.arena_floats, dtype=torch.bool)
    for o, n in zip(layout.offsets.tolist(), layout.sizes.tolist()):
        live[o:o + n] = True
    a = arena.cpu()
    return bool((a[~live].view(torch.int32) == 0).all())


# ---- the kernels' index arithmetic, restated (csrc/optimizer.hip: opt_unit, the float4 body, the scalar tail / scalar path)
def _unit(sizes, offsets, arena_floats, seg, chunk):
    if seg < 0 or seg >= len(sizes) or chunk < 0:
        return None
    n, off, base = int(sizes[seg]), int(offsets[seg]), chunk * CHUNK
    if n <= 0 or off < 0 or off % ALIGN or off > arena_floats - n or base >= n:
        return None
    return n, off, base, min(n - base, CHUNK)


def emulate_step(sizes, offsets, units, arena_floats, aligned):
    """Run opt_step_kernel's addressing over the unit map: -> (stores per element of every segment, loads in bounds?).  `aligned[s]`:
    whether segment s's parameter is 16-byte aligned (the float4 path) or not (the scalar path).  Arena-side and parameter-side
    accesses use the same element index, so one count serves both."""
    stores = [np.zeros(int(n), np.int32) for n in sizes]
    loads_ok = True
    tid = np.arange(THREADS)
    for seg, chunk in np.asarray(units).tolist():
        u = _unit(sizes, offsets, arena_floats, seg, chunk)
        if u is None:
            continue
        n, off, base, cnt = u
        nfull = cnt >> 2 if aligned[seg] else 0
        if nfull > 0:
            for j in range(CHUNK // 4 // THREADS):
                v = j * THREADS + tid
                vc = np.where(v < nfull, v, nfull - 1)
                loads_ok &= bool((vc >= 0).all() and (base + 4 * vc + 3 < n).all() and (off + base + 4 * vc + 3 < arena_floats).all())
                stores[seg][(base + 4 * v[v < nfull])[:, None] + LANES] += 1             # (distinct indices within one statement)
        done = nfull * 4
        rest = cnt - done
        if rest == 0:
            continue
        for b in range(0, CHUNK // THREADS, 4):
            if b * THREADS >= rest:
                break
            for k in range(4):
                r = (b + k) * THREADS + tid
                e = done + np.where(r < rest, r, rest - 1)
                loads_ok &= bool((e >= 0).all() and (base + e < n).all())
                stores[seg][base + done + r[r < rest]] += 1
    return stores, loads_ok


def emulate_gather(sizes, offsets, units, arena_floats, aligned, present):
    """opt_gather_kernel's addressing: -> (arena stores per float of the whole arena, source loads in bounds?)."""
    arena = np.zeros(arena_floats, np.int32)
    loads_ok = True
    tid = np.arange(THREADS)
    for seg, chunk in np.asarray(units).tolist():
        u = _unit(sizes, offsets, arena_floats, seg, chunk)
        if u is None:
            continue
        n, off, base, cnt = u
        g = off + base
        nvec, nfull = (cnt + 3) >> 2, cnt >> 2
        if not present[seg] or aligned[seg]:
            body = nvec if not present[seg] else nfull
            for j in range(CHUNK // 4 // THREADS):
                v = j * THREADS + tid
                if present[seg] and nfull > 0:
                    vc = np.where(v < nfull, v, nfull - 1)
                    loads_ok &= bool((base + 4 * vc + 3 < n).all())
                arena[(g + 4 * v[v < body])[:, None] + LANES] += 1
            if present[seg] and nvec > nfull:
                e = nfull * 4 + tid[:4]
                loads_ok &= bool((base + np.where(e < cnt, e, cnt - 1) < n).all())
                arena[g + e] += 1
            continue
        for b in range(CHUNK // THREADS):
            e = b * THREADS + tid
            loads_ok &= bool((base + np.where(e < cnt, e, cnt - 1) < n).all())
            arena[g + e[e < nvec * 4]] += 1
    return arena, loads_ok


# ---- float64 restatements
def clipped_steps_ref(p0s, grads_by_step, name, wds, momentum, max_norm, dtype=F64):
    """Steps of the whole model with full-model clipping: per step ONE coefficient from the norm over all tensors' gradients
    (S.clip_ref on their concatenation), then S.optimiser_steps per tensor on the scaled gradients at lr = S.STEP_LR[name].
    -> (parameters, S magnitudes, coefficients per step).  max_norm None: no clipping."""
    coefs = []
    scaled = [[] for _ in p0s]
    for grads in grads_by_step:
        coef = torch.ones((), dtype=F64)
        if max_norm is not None:
            coef = S.clip_ref(torch.cat([g.reshape(-1) for g in grads]), max_norm)[2]
        coefs.append(coef)
        for i, g in enumerate(grads):
            scaled[i].append(g.double() * coef)
    out = [S.optimiser_steps(p0, scaled[i], name, wds[i], momentum, dtype) for i, p0 in enumerate(p0s)]
    return [o[0] for o in out], [o[1] for o in out], coefs


def clipped_step_bound(name: str) -> float:
    """The allowance of a parameter after clipped steps, per element against S: FLOOR_FACTOR x (the optimiser's own floor + the clipped
    gradient's floor).  The step is linear in the gradient for SGD (momentum included) and scale-invariant up to eps for AdamW, so a
    relative error d of the scaled gradient moves the terms added to p - all of which S contains - by at most d; the two families'
    errors add.  Both floors are the existing ones of tests/stream_forms.py (never below 2^-24)."""
    return S.FLOOR_FACTOR * (S.floor_optimiser(name) + S.floor_clipped_gradient())


def coef_bound() -> float:
    """The clip coefficient, relative: it is 1 / (norm + 1e-6) of a sum of squares, whose allowance is the sum's (test_clip_grad_norm_against_f64)."""
    return S.FLOOR_FACTOR * S.floor_sumsq()


def real_sizes():
    """The element counts of the tensors the seven trainers hold on the synthetic checkpoint (652), from synth.state_dict_spec shapes and
    each trainer's parameter_names - on the CPU."""
    from nopesac_amd import training as T
    from nopesac_amd.synth import state_dict_spec
    spec = state_dict_spec(50)
    keys = list(spec)
    names = (T.BackboneTrainer.parameter_names(keys) + T.CameraHeadTrainer.parameter_names(keys, True) + T.MatchingHeadTrainer.parameter_names(keys)
             + T.PlaneInstanceHeadsTrainer.parameter_names(keys) + T.PlaneDecoderTrainer.parameter_names(keys)
             + T.PlanePyramidTrainer.parameter_names(keys) + T.PlaneEncoderTrainer.parameter_names(keys))
    assert len(names) == len(set(names))
    return [int(np.prod(spec[k])) if len(spec[k]) else 1 for k in names]
