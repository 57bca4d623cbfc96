"""The shape of nopesac_amd/training.py's class hierarchy and its one statement of the optimiser groups (no device, no library): every
trainer derives from HeadTrainer, only CameraHeadTrainer from RefineTrainer, the shared methods exist once, and parameter_group puts every
key of every trainer into the group the reference's build_optimizer (train_NopeSAC.py:88-135) gives its module type - checked against
regular expressions restated here and against the counts taken from the code before the groups were stated in one place."""
import re

import pytest

from nopesac_amd import training as T
from nopesac_amd.synth import synth_state_dict

TRAINERS = (T.RefineTrainer, T.CameraHeadTrainer, T.MatchingHeadTrainer, T.PlaneInstanceHeadsTrainer, T.PlaneDecoderTrainer,
            T.PlanePyramidTrainer)
NOT_CAMERA = TRAINERS[2:]

# norm module types (GroupNorm, BatchNorm2d, LayerNorm) and nn.Embedding by their places in the reference's modules
NORM = [re.compile(p) for p in (
    r"^camera_head_list\.0\.pixel_decoder\.[a-z_0-9]+\.norm\.(weight|bias)$",                    # Conv2d(norm=GroupNorm)
    r"^camera_head_list\.0\.convs_(backbone|trans|rots)\.\d+\.1\.(weight|bias)$",                # Sequential(conv, BatchNorm2d, LeakyReLU)
    r"^matching_head\.gnn\.layers\.\d+\.norm[12]\.(weight|bias)$",
    r"^sem_seg_head\.context2plane_decoder\.(layers\.\d+\.norm[123]|norm)\.(weight|bias)$",
    r"^sem_seg_head\.top_down\.[a-z_0-9.]+\.1\.(weight|bias)$")]                                   # conv_bn_relu
EMBED = re.compile(r"^sem_seg_head\.query_embed\.weight$")

#                      tensors, norm, embed, plain
COUNTS = {"refine": (80, 0, 0, 80), "camera": (108, 0, 0, 108), "camera_convs": (179, 46, 0, 133), "matcher": (185, 72, 0, 113),
          "heads": (24, 0, 0, 24), "decoder": (111, 38, 1, 72), "pyramid": (24, 16, 0, 8)}


def _group(key):
    return "embed" if EMBED.match(key) else "norm" if any(p.match(key) for p in NORM) else "plain"


@pytest.fixture(scope="module")
def trainers():
    sd = synth_state_dict(50)
    return {"refine": T.RefineTrainer.from_state_dict(sd, 50, "cpu"), "camera": T.CameraHeadTrainer.from_state_dict(sd, 50, "cpu"),
            "camera_convs": T.CameraHeadTrainer.from_state_dict(sd, 50, "cpu", conv_stacks=True),
            "matcher": T.MatchingHeadTrainer.from_state_dict(sd, 50, "cpu"), "heads": T.PlaneInstanceHeadsTrainer.from_state_dict(sd, 50, "cpu"),
            "decoder": T.PlaneDecoderTrainer.from_state_dict(sd, 50, "cpu"), "pyramid": T.PlanePyramidTrainer.from_state_dict(sd, "cpu")}


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_every_key_is_in_the_references_group(trainers, name):
    tr = trainers[name]
    groups = {k: T.parameter_group(k) for k in tr.params}
    assert groups == {k: _group(k) for k in tr.params}
    count = lambda g: sum(v == g for v in groups.values())
    assert (len(groups), count("norm"), count("embed"), count("plain")) == COUNTS[name]
    decay = {"plain": 0.5, "norm": 0.25, "embed": 0.125}
    assert all(tr._weight_decay(k, 0.5, 0.25, 0.125) == decay[g] for k, g in groups.items())
    assert all(tr._weight_decay(k, 0.5, None, None) == 0.5 for k in groups)
    if name in ("camera_convs", "matcher"):
        assert all(T.is_norm_parameter(k) == (g == "norm") for k, g in groups.items())
    if name == "pyramid":
        assert len(tr.buffers) == 24 and not set(tr.buffers) & set(tr.params)


def test_the_five_largest_sets_are_disjoint(trainers):
    keys = [k for name in ("camera_convs", "matcher", "heads", "decoder", "pyramid") for k in trainers[name].params]
    assert len(keys) == 523 == len(set(keys))


def test_the_hierarchy():
    assert all(issubclass(c, T.HeadTrainer) for c in TRAINERS) and issubclass(T.CameraHeadTrainer, T.RefineTrainer)
    for c in NOT_CAMERA:
        assert not issubclass(c, T.RefineTrainer)
        assert not any(hasattr(c, m) for m in ("_mlp", "_lin", "warp_in_ref"))
    assert not hasattr(T.MatchingHeadTrainer, "losses")
    assert issubclass(T.PlaneDecoderTrainer, T.ChainedTrainer) and issubclass(T.PlanePyramidTrainer, T.ChainedTrainer)
    assert (T.PlaneDecoderTrainer.OUTPUT, T.PlanePyramidTrainer.OUTPUT) == ("hs", "p1")


def test_the_shared_methods_exist_once():
    classes = {c for t in TRAINERS for c in t.__mro__ if c is not object}
    assert classes == set(TRAINERS) | {T.HeadTrainer, T.ChainedTrainer}
    owners = lambda m: {c for c in classes if m in c.__dict__}
    for m in ("_clear_grads", "_collect", "_watch", "_weight_decay", "step", "step_from_cfg", "clip_grad_norm", "lr_multiplier", "_copy_into"):
        assert owners(m) == {T.HeadTrainer}, m
    assert owners("write_back") == {T.HeadTrainer, T.PlanePyramidTrainer}                # the pyramid adds its buffers
    assert owners("backward_from") == {T.ChainedTrainer}
    assert owners("backward") == {T.HeadTrainer, T.ChainedTrainer, T.PlaneInstanceHeadsTrainer}     # sum of losses / the chain / the criterion's weights


def test_prefix_and_multiplier_are_class_attributes(trainers):
    from nopesac_amd.config import get_cfg
    cfg = get_cfg()
    prefixes = {c: c.KEY_PREFIX for c in TRAINERS}
    assert prefixes == {T.RefineTrainer: T.PREFIX, T.CameraHeadTrainer: T.PREFIX, T.MatchingHeadTrainer: T.MATCHER_PREFIX,
                        T.PlaneInstanceHeadsTrainer: T.PLANE_PREFIX, T.PlaneDecoderTrainer: T.PLANE_PREFIX, T.PlanePyramidTrainer: T.PLANE_PREFIX}
    assert {type(tr) for tr in trainers.values()} == set(TRAINERS)
    for tr in trainers.values():
        plane = tr.KEY_PREFIX == T.PLANE_PREFIX
        assert tr.LR_MULTIPLIER == ("SEM_SEG_HEAD_MULTIPLIER" if plane else None)
        assert tr.lr_multiplier(cfg) == (float(cfg.SOLVER.SEM_SEG_HEAD_MULTIPLIER) if plane else 1.0)
        assert all(k.startswith(tr.KEY_PREFIX) for k in tr.params)


class _Head:
    """What write_back needs of an inference head: raw tensors by un-prefixed key, and invalidate()."""

    def __init__(self, tensors, prefix):
        self.tensors = {k[len(prefix):]: t.detach().clone().zero_() for k, t in tensors.items()}
        self._spec_keys, self.invalidated = list(self.tensors), 0

    def raw(self, key):
        return self.tensors[key]

    def invalidate(self):
        self.invalidated += 1


def test_write_back_copies_parameters_and_only_the_pyramids_buffers(trainers):
    import torch
    for name in ("camera_convs", "pyramid", "decoder"):
        tr = trainers[name]
        head = _Head({**tr.params, **tr.buffers} if hasattr(tr, "buffers") else tr.params, tr.KEY_PREFIX)
        tr.write_back(head)
        assert head.invalidated == 1
        same = lambda k, t: torch.equal(head.raw(k[len(tr.KEY_PREFIX):]), t.detach())
        assert all(same(k, t) for k, t in tr.params.items())
        if name == "pyramid":
            assert all(same(k, t) for k, t in tr.buffers.items())
        if name == "camera_convs":                                                        # fixed inputs: never written back
            assert tr.buffers and all(float(head.raw(k[len(tr.KEY_PREFIX):]).abs().sum()) == 0 for k in tr.buffers)
            assert any(float(t.abs().sum()) != 0 for t in tr.buffers.values())
