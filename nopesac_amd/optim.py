"""One optimiser step for the whole model (the reference's Trainer.build_optimizer + build_lr_scheduler, train_NopeSAC.py:88-169).

ModelOptimizer steps ANY set of trainers (nopesac_amd/training.py) at once: the gradient norm of full-model clipping is taken over
every parameter of every trainer (FullModelGradientClippingOptimizer, train_NopeSAC.py:139-153 - HeadTrainer.clip_grad_norm sees one
trainer only, so clipping over more than one trainer belongs here; HeadTrainer.step_from_cfg remains the single-trainer form), there
is ONE step counter, the learning rate follows detectron2's WarmupMultiStepLR (lr_at), gradients can be averaged across ranks between
the gather and the norm (`reduce`, average_across_ranks), and the optimiser state can be saved and resumed.

A step is a fixed number of launches whatever the number of tensors: the per-step source table's upload, nopesac_opt_gather (every
.grad into the flat arena G), the optional reduce, the norm of G (ops.sumsq_accumulate, two launches in its deterministic slice order)
and ops.clip_coefficient, then nopesac_opt_step (csrc/optimizer.hip) over the parameters and the moment arenas M1 / M2.  The update is
HeadTrainer.step's, bit for bit: the same operations in the same order as ops.scale_by + ops.adamw_step / ops.sgd_step per tensor.
Parameters are updated in place and never re-seated, so every trainer's write_back keeps working.  No host synchronisation anywhere.

Not here: a whole-model training forward (each trainer's backward is still called by its user), capture of the step into a graph,
bf16 / AMP parameters, Nesterov momentum, BIAS_LR_FACTOR / WEIGHT_DECAY_BIAS (the reference's build_optimizer ignores them too)."""
from __future__ import annotations

from bisect import bisect_right
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .training import HeadTrainer


def lr_at(cfg, it: int) -> float:
    """detectron2's WarmupMultiStepLR at iteration `it`: BASE_LR * warmup(it) * GAMMA ** bisect_right(STEPS, it).  The optimiser's k-th
    step, counted from 0, uses lr_at(cfg, k) (the reference advances the scheduler after the step)."""
    S = cfg.SOLVER
    if S.LR_SCHEDULER_NAME != "WarmupMultiStepLR":
        raise NotImplementedError("SOLVER.LR_SCHEDULER_NAME %r (the reference's configs use WarmupMultiStepLR)" % (S.LR_SCHEDULER_NAME,))
    it, warmup_iters = int(it), int(S.WARMUP_ITERS)
    if S.WARMUP_METHOD not in ("linear", "constant"):
        raise NotImplementedError("SOLVER.WARMUP_METHOD %r (linear or constant)" % (S.WARMUP_METHOD,))
    if it >= warmup_iters:
        warmup = 1.0
    elif S.WARMUP_METHOD == "constant":
        warmup = float(S.WARMUP_FACTOR)
    else:
        alpha = it / warmup_iters
        warmup = float(S.WARMUP_FACTOR) * (1 - alpha) + alpha
    return float(S.BASE_LR) * warmup * float(S.GAMMA) ** bisect_right([int(s) for s in S.STEPS], it)


def average_across_ranks(flat: torch.Tensor) -> torch.Tensor:
    """The `reduce` of data-parallel training: all_reduce(SUM) of the flat gradient buffer, in place, then division by the world size.
    Does nothing without an initialised process group or at world size 1."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return flat
    dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    return flat.div_(dist.get_world_size())


def parameter_table(trainers: Sequence[HeadTrainer], cfg=None, *, weight_decay: float = 0.01, weight_decay_norm: Optional[float] = None,
                    weight_decay_embed: Optional[float] = None):
    """The tensors of `trainers` in order, and their hyper-parameter groups: -> (keys, params, group index per key, groups), groups =
    the distinct (learning-rate multiplier, weight decay) pairs in order of first appearance.  A tensor's multiplier is its trainer's
    lr_multiplier(cfg) (1 without a cfg), its decay HeadTrainer._weight_decay of its key - what step_from_cfg hands to step.  A key held
    by two trainers (RefineTrainer's keys are a subset of CameraHeadTrainer's) and a seventeenth group are ValueErrors."""
    keys: List[str] = []
    params: List[torch.Tensor] = []
    index: List[int] = []
    groups: List[Tuple[float, float]] = []
    owner: Dict[str, int] = {}
    for t, tr in enumerate(trainers):
        mult = 1.0 if cfg is None else float(tr.lr_multiplier(cfg))
        for k, p in tr.params.items():
            if k in owner:
                raise ValueError("state-dict key %r is held by two trainers (%d: %s and %d: %s)"
                                 % (k, owner[k], type(trainers[owner[k]]).__name__, t, type(tr).__name__))
            owner[k] = t
            pair = (mult, float(HeadTrainer._weight_decay(k, weight_decay, weight_decay_norm, weight_decay_embed)))
            if pair not in groups:
                if len(groups) == ops.OPT_MAX_GROUPS:
                    raise ValueError("more than %d distinct (lr multiplier, weight decay) groups (key %r)" % (ops.OPT_MAX_GROUPS, k))
                groups.append(pair)
            keys.append(k); params.append(p); index.append(groups.index(pair))
    if not keys:
        raise ValueError("no parameters to optimise")
    return keys, params, index, groups


class ModelOptimizer:
    """AdamW / SGD(momentum) over every parameter of `trainers`, with full-model gradient clipping (max_norm; None = off).

        opt = ModelOptimizer.from_cfg([backbone, encoder, pyramid, decoder, heads, matcher, camera], cfg)
        ...every trainer's backward...                                   # leaves p.grad on its parameters
        coef = opt.step()                                                # lr_at(cfg, opt.steps); device f32[1], 1 = not clipped
        opt.zero_grad(); opt.save(path)

    Without a `reduce`, a parameter whose .grad is None adds nothing to the norm and neither it nor its moments move (HeadTrainer.step
    does the same).  With one, an absent gradient counts as zeros and the tensor is stepped: a rank cannot skip what another steps.
    `reduce(G)` runs on the flat f32 gradient arena (zero padding between tensors included), in place, on the current stream."""

    def __init__(self, trainers: Sequence[HeadTrainer], *, optimizer: str = "ADAMW", betas=(0.9, 0.999), eps: float = 1e-8,
                 momentum: float = 0.9, weight_decay: float = 0.01, weight_decay_norm: Optional[float] = None,
                 weight_decay_embed: Optional[float] = None, max_norm: Optional[float] = None,
                 reduce: Optional[Callable[[torch.Tensor], object]] = None, cfg=None):
        self.optimizer = str(optimizer).upper()
        if self.optimizer not in ops.OPT_MODES:
            raise NotImplementedError(f"no optimizer type {optimizer}")       # train_NopeSAC.py:158
        self.trainers, self.cfg, self.reduce = list(trainers), cfg, reduce
        self.betas, self.eps, self.momentum = (float(betas[0]), float(betas[1])), float(eps), float(momentum)
        self.max_norm = None if max_norm is None or float(max_norm) <= 0.0 else float(max_norm)
        self.keys, self.params, self.group_index, self.groups = parameter_table(
            self.trainers, cfg, weight_decay=weight_decay, weight_decay_norm=weight_decay_norm, weight_decay_embed=weight_decay_embed)
        dev = self.params[0].device
        for k, p in zip(self.keys, self.params):
            if p.dtype != torch.float32 or not p.is_contiguous() or not p.is_cuda or p.device != dev:
                raise ValueError("parameter %r: %s, %s, on %s - ModelOptimizer takes contiguous f32 tensors on one GPU (%s)"
                                 % (k, p.dtype, "contiguous" if p.is_contiguous() else "not contiguous", p.device, dev))
        self.layout = ops.OptLayout(self.params, self.group_index)
        self.G = self.layout.arena()
        self.M1 = self.layout.arena() if self.optimizer == "ADAMW" or self.momentum != 0.0 else None
        self.M2 = self.layout.arena() if self.optimizer == "ADAMW" else None
        self.stepped = [False] * len(self.keys)
        self.steps = 0
        self.grad_norm_sq: Optional[torch.Tensor] = None
        self._one = torch.ones(1, device=dev, dtype=torch.float32)

    @classmethod
    def from_cfg(cls, trainers: Sequence[HeadTrainer], cfg, reduce: Optional[Callable] = None) -> "ModelOptimizer":
        """The reference's solver settings, the keys HeadTrainer.step_from_cfg reads: SOLVER.OPTIMIZER, WEIGHT_DECAY(_NORM / _EMBED),
        MOMENTUM, CLIP_GRADIENTS (full_model only) and every trainer's *_MULTIPLIER; the schedule's keys are read by lr_at at each step.
        `reduce` defaults to average_across_ranks when a process group of more than one rank exists."""
        S = cfg.SOLVER
        cg = S.CLIP_GRADIENTS
        max_norm = None
        if cg.ENABLED and cg.CLIP_TYPE == "full_model" and cg.CLIP_VALUE > 0.0:
            max_norm = float(cg.CLIP_VALUE)
        elif cg.ENABLED:
            raise NotImplementedError("SOLVER.CLIP_GRADIENTS.CLIP_TYPE %r (the reference's configs use full_model)" % (cg.CLIP_TYPE,))
        dist = torch.distributed
        if reduce is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            reduce = average_across_ranks
        return cls(trainers, optimizer=str(S.OPTIMIZER), momentum=float(S.MOMENTUM), weight_decay=float(S.WEIGHT_DECAY),
                   weight_decay_norm=float(S.WEIGHT_DECAY_NORM), weight_decay_embed=float(S.WEIGHT_DECAY_EMBED), max_norm=max_norm,
                   reduce=reduce, cfg=cfg)

    def group_hyperparameters(self, lr: float) -> List[Tuple[float, float]]:
        """[(learning rate, weight decay)] of the groups at base rate `lr`: lr * multiplier formed in Python double, as step_from_cfg
        forms it, and rounded to f32 once where it enters the argument block."""
        return [(float(lr) * mult, wd) for mult, wd in self.groups]

    def step(self, lr: Optional[float] = None) -> torch.Tensor:
        """One step of every parameter that has a gradient.  -> the clip coefficient (device f32[1]; 1 = not clipped, also with
        clipping off); `grad_norm_sq` keeps the device f32[1] sum of squares of a clipping step (None with clipping off)."""
        if lr is None:
            if self.cfg is None:
                raise ValueError("step(): a learning rate, or a cfg for the schedule (ModelOptimizer.from_cfg)")
            lr = lr_at(self.cfg, self.steps)
        grads = [None if p.grad is None else p.grad.contiguous() for p in self.params]
        for k, g in zip(self.keys, grads):
            if g is not None and g.dtype != torch.float32:
                raise ValueError("gradient of %r is %s, not f32" % (k, g.dtype))
        absent_as_zeros = self.reduce is not None
        taking = [absent_as_zeros or g is not None for g in grads]
        first = [t and not s for t, s in zip(taking, self.stepped)]
        with torch.no_grad():
            sources = self.layout.sources(grads, first, absent_as_zeros)
            ops.opt_gather(self.layout, sources, self.G)
            if self.reduce is not None:
                self.reduce(self.G)
            coef = None
            self.grad_norm_sq = None
            if self.max_norm is not None:
                self.grad_norm_sq = ops.sumsq_accumulate(self.G)
                coef = ops.clip_coefficient(self.grad_norm_sq, self.max_norm)
            ops.opt_step(self.layout, sources, self.G, self.M1, self.M2, coef, self.optimizer, self.group_hyperparameters(lr), self.steps + 1,
                         self.betas, self.eps, self.momentum)
        self.steps += 1
        self.stepped = [s or t for s, t in zip(self.stepped, taking)]
        return self._one if coef is None else coef

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    # ---- state
    def _moment_names(self) -> Tuple[str, ...]:
        return ("exp_avg", "exp_avg_sq") if self.optimizer == "ADAMW" else ("momentum_buffer",)

    def state_dict(self) -> dict:
        """{"steps", "optimizer", "state": {state-dict key: {"exp_avg", "exp_avg_sq"} or {"momentum_buffer"}, plus "stepped"}} with
        host tensors in the parameters' shapes (this copy waits for the device)."""
        arenas = (self.M1, self.M2)
        state = {}
        for i, k in enumerate(self.keys):
            entry = {"stepped": bool(self.stepped[i])}
            for name, arena in zip(self._moment_names(), arenas):
                entry[name] = torch.zeros(self.params[i].shape) if arena is None else self.layout.view(arena, i).detach().cpu().clone()
            state[k] = entry
        return {"steps": int(self.steps), "optimizer": self.optimizer, "state": state}

    def load_state_dict(self, sd: dict):
        """Raises ValueError on another optimiser, key set or tensor shape; nothing is changed then."""
        if sd.get("optimizer") != self.optimizer:
            raise ValueError("state of optimizer %r, this one is %r" % (sd.get("optimizer"), self.optimizer))
        state = sd["state"]
        if set(state) != set(self.keys):
            missing, extra = sorted(set(self.keys) - set(state)), sorted(set(state) - set(self.keys))
            raise ValueError("state-dict keys differ: missing %s, unexpected %s" % (missing[:5], extra[:5]))
        names = self._moment_names()
        for i, k in enumerate(self.keys):
            for name in names:
                if name not in state[k] or tuple(state[k][name].shape) != tuple(self.params[i].shape):
                    raise ValueError("%s of %r: shape %s expected" % (name, k, tuple(self.params[i].shape)))
        with torch.no_grad():
            for i, k in enumerate(self.keys):
                for name, arena in zip(names, (self.M1, self.M2)):
                    if arena is not None:
                        self.layout.view(arena, i).copy_(state[k][name].to(torch.float32))
        self.stepped = [bool(state[k]["stepped"]) for k in self.keys]
        self.steps = int(sd["steps"])

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        self.load_state_dict(torch.load(path, map_location="cpu"))
