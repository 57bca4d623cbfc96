"""The driver from images to an optimiser step (reference PlaneTR_NopeSAC.forward in training, siamese_planeTR.py:215-299, under
configs/train_mp3d_step3.yaml): TrainStep wires the seven trainers of nopesac_amd/training.py, the mappers and ModelOptimizer.

    ts = TrainStep.from_model(model, cfg, seed=0)
    losses = ts.step(entries)            # map_batch -> pair_targets -> losses -> one backward -> ModelOptimizer.step(); device scalars
    ts.check()                           # one host read: the matcher's input contract and a finite total - as often as the caller likes
    ts.write_back(); sd = ts.state_dict()

The backbone runs once on the 2B augmented images (view 1's first).  The plane head - encoder, decoder + pyramid, instance heads,
criterion - runs ONCE on them with groups=2: the criterion's normalisers and the pyramid's BatchNorm statistics
are per view, as the reference's two forward_single calls have them, and the detection losses are the per-view mean.  TwoViewLosses adds
the matching head's embedding loss and the camera head's losses on the last layer's outputs split by view.  One backward runs over the
six heads' graph; the backbone's maps enter it as leaves, and the gradients that arrive there - the plane head's and, through the camera
trainer's feature_grads, the pose net's - are summed and sent through the backbone in the same step (BackboneTrainer.backward_from).
Single rank only: the per-view num_masks all-reduce of the reference is not wired."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import ops
from .optim import ModelOptimizer
from .training import (BackboneTrainer, CameraHeadTrainer, MatchingHeadTrainer, PlaneCriterion, PlaneDecoderTrainer, PlaneEncoderTrainer,
                       PlaneInstanceHeadsTrainer, PlanePyramidTrainer, TwoViewLosses, joint_backward)

MODULES = ("backbone", "encoder", "pyramid", "decoder", "heads", "matcher", "camera")
MAPS = ("res2", "res3", "res4", "res5")
ENCODER_DROPOUT = 0.1                    # nn.Transformer's default, which the reference's plane head keeps (no config key names it)


class TrainStep:
    """See the module's text.  `modules` names the trainers the optimiser steps (default: all seven).  The others still run, forward and
    backward, and their gradients are dropped: their parameters, optimiser state and counters of steps do not move (running BatchNorm
    buffers of the pyramid and the camera tower are updated by every forward, stepped or not, as in the reference's train mode)."""

    def __init__(self, model, cfg, trainers: Dict[str, object], seed: int = 0, modules: Optional[Sequence[str]] = None,
                 dropout: float = ENCODER_DROPOUT):
        from .data import PairMapper
        from .targets import TargetMapper
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("TrainStep: one rank only (the per-view num_masks all-reduce is not wired)")
        self.model, self.cfg, self.seed, self.dropout = model, cfg, int(seed), float(dropout)
        self.trainers = dict(trainers)
        self.modules = tuple(MODULES if modules is None else modules)
        unknown = [m for m in self.modules if m not in MODULES]
        if unknown or not self.modules:
            raise ValueError("TrainStep: modules %r; the trainers are %r" % (unknown or self.modules, MODULES))
        self.camera_head = model.camera_head_list[0]
        self.criterion = PlaneCriterion.from_cfg(cfg)
        self.trainers["heads"].criterion = self.criterion
        self.two_view = TwoViewLosses(self.trainers["matcher"], self.trainers["camera"], self.camera_head)
        self.targets = TargetMapper.from_cfg(cfg, model.device)
        self.mapper = PairMapper(cfg, device=model.device, train=True, seed=self.seed)
        self.optimizer = ModelOptimizer.from_cfg([self.trainers[m] for m in MODULES if m in self.modules], cfg)
        self.steps = 0
        self._total: Optional[torch.Tensor] = None
        self._leaves: Dict[str, torch.Tensor] = {}

    @classmethod
    def from_model(cls, model, cfg, seed: int = 0, modules: Optional[Sequence[str]] = None, dropout: float = ENCODER_DROPOUT) -> "TrainStep":
        head = model.sem_seg_head
        trainers = {"backbone": BackboneTrainer.from_backbone(model.backbone),
                    "encoder": PlaneEncoderTrainer.from_head(head, feature_grads=True),
                    "pyramid": PlanePyramidTrainer.from_head(head, feature_grads=True),
                    "decoder": PlaneDecoderTrainer.from_head(head),
                    "heads": PlaneInstanceHeadsTrainer.from_head(head, cfg),
                    "matcher": MatchingHeadTrainer.from_head(model.matching_head),
                    "camera": CameraHeadTrainer.from_head(model.camera_head_list[0], conv_stacks=True, feature_grads=True, batch_stats=True)}
        return cls(model, cfg, trainers, seed, modules, dropout)

    # ---- forward
    def images(self, mapped: Sequence[dict]) -> torch.Tensor:
        """The mapper's dicts -> the backbone's input: 2B images (view 1's first), normalised, f32 NHWC with the stem's zero channel."""
        m = self.model
        imgs = [x["0"]["image"] for x in mapped] + [x["1"]["image"] for x in mapped]
        return ops.preprocess(m._to_device_batch(imgs), m.pixel_mean, m.pixel_std, m.backbone.STEM_CIN_PAD, torch.float32)

    def losses(self, images: torch.Tensor, pair: dict, step: int) -> Dict[str, torch.Tensor]:
        """images [2B, H, W, 4] f32 (self.images), pair = TargetMapper.pair_targets(entries) -> the reference's training dict: the
        weighted detection losses as the per-view mean (every key of weight_dict the criterion produced), losses_emb_0 and the camera
        head's 32 losses (34 with rand_cam_on), autograd tape attached."""
        T = self.trainers
        B = images.shape[0] // 2
        feats = T["backbone"].forward(images)
        self._leaves = {k: feats[k].detach().requires_grad_(True) for k in MAPS}
        plane, idx = T["encoder"].losses(T["heads"], T["decoder"], T["pyramid"], self._leaves, pair["targets"], p=self.dropout,
                                         seed=self.seed, step=step, groups=2)
        mq, n = idx["match_q"][0], pair["targets"]["n"]
        hs_last = T["heads"]._inputs["hs"][-1]
        tv = self.two_view.losses(hs_last, T["heads"].last["pred_params"], mq[:B], mq[B:], n[:B], n[B:], pair,
                                  {k: self._leaves[k] for k in ("res3", "res4", "res5")}, B, seed=self.seed, step=step)
        views = [self.criterion.weighted(g) for g in self.criterion.last["group_losses"]]      # (w l1 + w l2) / 2, siamese_planeTR.py:228-235
        return {**{k: (views[0][k] + views[1][k]) / 2 for k in views[0]}, **tv}

    def backward(self, losses: Dict[str, torch.Tensor]):
        """One backward over the six heads, then the backbone from the sum of what arrived at its maps."""
        T = self.trainers
        for t in self._leaves.values():
            t.grad = None
        joint_backward([T[m] for m in MODULES if m != "backbone"], losses)
        d = {}
        for k, leaf in self._leaves.items():
            g = leaf.grad
            cam = T["camera"].input_grads.get(k)
            if cam is not None:
                g = cam if g is None else g + cam
            if g is not None:
                d[k] = g
        T["backbone"].backward_from(d)

    def step(self, entries: Sequence[dict], step: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """One training step on B dataset pairs -> the loss dict as detached device scalars.  No host read beyond the mappers'."""
        step = self.steps if step is None else int(step)
        mapped = self.mapper.map_batch(list(entries), step=step, keep_device=True)
        pair = self.targets.pair_targets(entries)
        losses = self.losses(self.images(mapped), pair, step)
        self.backward(losses)
        self.optimizer.step()
        for m in MODULES:
            if m not in self.modules:                      # ran, not stepped: its gradients are dropped
                for p in self.trainers[m].params.values():
                    p.grad = None
        out = {k: v.detach() for k, v in losses.items()}
        self._total = torch.stack(list(out.values())).sum()
        self.steps = step + 1
        return out

    def check(self):
        """One host read: TwoViewLosses.check() and a finite summed loss of the last step."""
        self.two_view.check()
        if self._total is not None and not bool(torch.isfinite(self._total)):
            raise FloatingPointError("TrainStep: the summed loss of step %d is not finite" % (self.steps - 1))

    # ---- state
    def write_back(self):
        """Every trainer's tensors (and running buffers) into the inference model."""
        m, T = self.model, self.trainers
        T["backbone"].write_back(m.backbone)
        for k in ("encoder", "pyramid", "decoder", "heads"):
            T[k].write_back(m.sem_seg_head)
        T["matcher"].write_back(m.matching_head)
        T["camera"].write_back(self.camera_head)

    def _buffers(self) -> Dict[str, torch.Tensor]:
        return {**self.trainers["pyramid"].buffers, **self.trainers["camera"].buffers}

    def state_dict(self) -> dict:
        """Parameters, optimiser state, the step counter, the seed, and the running buffers and counters of pyramid and camera trainer
        (host copies)."""
        return {"steps": int(self.steps), "seed": int(self.seed), "modules": list(self.modules), "optimizer": self.optimizer.state_dict(),
                "params": {k: p.detach().cpu().clone() for t in self.trainers.values() for k, p in t.params.items()},
                "buffers": {k: v.detach().cpu().clone() for k, v in self._buffers().items()}}

    def load_state_dict(self, sd: dict):
        if list(sd["modules"]) != list(self.modules):
            raise ValueError("TrainStep: the state steps %r, this one %r" % (sd["modules"], self.modules))
        params = {k: p for t in self.trainers.values() for k, p in t.params.items()}
        buffers = self._buffers()
        if set(sd["params"]) != set(params) or set(sd["buffers"]) != set(buffers):
            raise ValueError("TrainStep: another set of tensors")
        self.optimizer.load_state_dict(sd["optimizer"])
        with torch.no_grad():
            for k, p in params.items():
                p.copy_(sd["params"][k])
            for k, v in buffers.items():
                v.copy_(sd["buffers"][k])
        self.steps, self.seed = int(sd["steps"]), int(sd["seed"])
        self.mapper.seed = self.seed
