"""TrainStep (nopesac_amd/train_step.py) on the device: B = 2 pairs of the synthetic checkpoint, entries as
tests/test_two_view_training_gpu.py::_entries builds them (its records drawn at the image size), with real image files.  Images are
480 x 640, the only size the camera head admits: the pose net correlates the two views' 15 x 20 maps (1/32 of the image) into a volume
of 15 x 20 = 300 channels, and the first conv of its two branches has exactly 300 input channels (96 x 128 gives 12 and is refused by
the conv launcher).  The label maps and depths are 480 x 640 too: criterion scale 4 against p1 at 120 x 160."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import test_two_view_training_gpu as TV
from tests.util import ROOT

pytestmark = pytest.mark.gpu
B, IH, IW = 2, 480, 640


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _image_dir():
    import tempfile

    from PIL import Image
    d = tempfile.mkdtemp(prefix="train_step_")
    rng = np.random.default_rng(7)
    for name in ("a0", "a1", "b0", "b1"):
        smooth = rng.integers(0, 256, (IH // 8, IW // 8, 3), dtype=np.uint8).repeat(8, 0).repeat(8, 1)
        Image.fromarray(((smooth.astype(np.int32) + rng.integers(-20, 21, (IH, IW, 3))).clip(0, 255)).astype(np.uint8)).save(os.path.join(d, name + ".png"))
    return d


def entries():
    d = _image_dir()
    size = TV.H, TV.W
    TV.H, TV.W = IH, IW                                    # _records draws its label maps and depths at the module's H x W
    try:
        out = TV._entries()
    finally:
        TV.H, TV.W = size
    for e, p in zip(out, "ab"):
        for v in "01":
            e[v] = dict(e[v], file_name=os.path.join(d, "%s%s.png" % (p, v)))
    return out


def _cfg(device, augmentation=False):
    from nopesac_amd.config import get_cfg
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "inference_mp3d.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(device), "MODEL.AMD.COMPUTE_DTYPE", "float32", "DATALOADER.AUGMENTATION", bool(augmentation)])
    return cfg


def make_step(device, seed=0, modules=None, dropout=0.0, augmentation=False):
    """A TrainStep over a model of its own (the synthetic checkpoint)."""
    from nopesac_amd.registry import build_model
    from nopesac_amd.synth import synth_state_dict
    from nopesac_amd.train_step import TrainStep
    cfg = _cfg(device, augmentation)
    model = build_model(cfg).eval()
    model.load_state_dict(synth_state_dict(50))
    return TrainStep.from_model(model, cfg, seed=seed, modules=modules, dropout=dropout)


def _all_params(ts):
    return {k: p for t in ts.trainers.values() for k, p in t.params.items()}


def test_composition_and_key_set(device):
    """Dropout 0, no augmentation: the loss dict is, bit for bit, the hand composition from the pieces of earlier commits - the backbone
    once, the plane head PER VIEW with groups=1, (w l1 + w l2) / 2, TwoViewLosses on the concatenated hs[-1], pred_params and match_q -
    and holds the 6 L + 2 detection names, losses_emb_0 and the camera head's 32 names, nothing else."""
    ts = make_step(device)
    E = entries()
    images = ts.images(ts.mapper.map_batch(E, step=0, keep_device=True))
    pair = ts.targets.pair_targets(E)
    got = {k: v.detach().clone() for k, v in ts.losses(images, pair, 0).items()}
    ref = make_step(device)
    T = ref.trainers
    feats = {k: v.detach() for k, v in T["backbone"].forward(images).items()}
    t = ref.criterion.prepare_targets(pair["targets"])
    per, hs, pp, mq = [], [], [], []
    for v in range(2):
        sl = slice(v * B, (v + 1) * B)
        tv_ = {k: (x[sl].contiguous() if torch.is_tensor(x) else x) for k, x in t.items()}
        losses, idx = T["encoder"].losses(T["heads"], T["decoder"], T["pyramid"], {k: f[sl].contiguous() for k, f in feats.items()}, tv_, p=0.0,
                                          seed=0, step=0)
        per.append(ref.criterion.weighted(losses))
        hs.append(T["heads"]._inputs["hs"][-1].detach())
        pp.append(T["heads"].last["pred_params"].detach())
        mq.append(idx["match_q"][0])
    want = {k: (per[0][k] + per[1][k]) / 2 for k in per[0]}
    n = pair["targets"]["n"]
    want.update(ref.two_view.losses(torch.cat(hs), torch.cat(pp), mq[0], mq[1], n[:B], n[B:], pair, {k: feats[k] for k in ("res3", "res4", "res5")}, B))
    L = 3
    names = {k + s for k in ("loss_ce", "loss_mask", "loss_dice", "loss_center_ins", "loss_param_l1", "loss_param_cos") for s in [""] + ["_%d" % i for i in range(L - 1)]}
    names |= {"loss_center_pixel", "loss_q", "losses_emb_0"}
    camera = set(got) - names
    assert names <= set(got) and len(camera) == 32 and len(got) == 6 * L + 2 + 1 + 32, sorted(got)
    assert set(got) == set(want)
    bad = [k for k in got if not _bits(got[k], want[k])]
    for k in bad:
        print("composition %s: one pass %.9g, per view %.9g" % (k, float(got[k]), float(want[k])))
    assert not bad, bad


STILL = "sem_seg_head.context2plane_decoder.layers.0.norm1.weight"


def test_one_step_gradients_buffers_and_the_modules_switch(device):
    """After one step every one of the 652 tensors has a finite gradient of its own shape and moved - but one: the first decoder layer's
    norm1 normalises the all-zero initial target (pre-norm, tgt = 0), so xhat = 0, the gradient of its weight is exactly 0 in the
    reference too, and WEIGHT_DECAY_NORM = 0 leaves it where it is (tests/test_plane_encoder_training_gpu.py excepts the same key)."""
    E = entries()
    ts = make_step(device)
    before = {k: p.detach().clone() for k, p in _all_params(ts).items()}
    bufs = {k: v.clone() for k, v in ts._buffers().items()}
    assert len(before) == 652
    out = ts.step(E)
    ts.check()
    assert all(v.dim() == 0 and not v.requires_grad for v in out.values())
    for k, p in _all_params(ts).items():
        assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        assert torch.equal(p.detach(), before[k]) == (k == STILL), k
    assert float(_all_params(ts)[STILL].grad.abs().max()) == 0.0
    counters = {k: int(v) - int(bufs[k]) for k, v in ts._buffers().items() if k.endswith("num_batches_tracked")}
    pyr = [d for k, d in counters.items() if k in ts.trainers["pyramid"].buffers]
    cam = [d for k, d in counters.items() if k in ts.trainers["camera"].buffers]
    assert pyr == [2] * 8 and set(cam) == {1, 2} and len(cam) == 18, (pyr, cam)      # the siamese tower per view, the branch layers once
    two = make_step(device, modules=("camera", "matcher"))
    two.step(E)
    moved = {k for k, p in _all_params(two).items() if not torch.equal(p.detach(), before[k])}
    want = set(two.trainers["camera"].params) | set(two.trainers["matcher"].params)
    assert moved == want and len(want) == 364
    assert all(p.grad is None for m in ("backbone", "encoder", "pyramid", "decoder", "heads") for p in two.trainers[m].params.values())


def test_determinism_and_resume(device):
    """dropout 0.1 and sampled augmentation on: one seed, the same bits after 2 steps; another seed, other bits; a state_dict taken after
    step 1 and loaded into a fresh TrainStep gives the step 2 of the uninterrupted one"""
    E = entries()
    runs = []
    for seed in (3, 3, 4):
        ts = make_step(device, seed=seed, dropout=0.1, augmentation=True)
        l0 = ts.step(E)
        sd = ts.state_dict() if len(runs) == 0 else None
        l1 = ts.step(E)
        runs.append((ts, l0, l1, sd))
    a, b, c = runs
    pa, pb, pc = (_all_params(r[0]) for r in runs)
    assert all(_bits(a[2][k], b[2][k]) for k in a[2]) and all(_bits(pa[k], pb[k]) for k in pa)
    assert not all(_bits(a[2][k], c[2][k]) for k in a[2]) and not all(_bits(pa[k], pc[k]) for k in pa)
    fresh = make_step(device, seed=0, dropout=0.1, augmentation=True)
    fresh.load_state_dict(a[3])
    assert fresh.steps == 1 and fresh.seed == 3
    l1 = fresh.step(E)
    pf = _all_params(fresh)
    assert all(_bits(l1[k], a[2][k]) for k in l1) and all(_bits(pf[k], pa[k]) for k in pa)
    assert all(torch.equal(v, a[0]._buffers()[k]) for k, v in fresh._buffers().items())


def test_it_trains_and_writes_back(device):
    """one fixed batch, dropout 0, no augmentation: the summed loss after 20 steps is lower than at step 0; write_back, then inference on
    the same pair returns finite poses"""
    E = entries()
    ts = make_step(device)
    first = None
    for it in range(21):
        out = ts.step(E, step=it)
        total = float(torch.stack(list(out.values())).sum())
        first = total if first is None else first
    ts.check()
    print("summed loss: step 0 %.6f, step 20 %.6f" % (first, total))
    assert np.isfinite(total) and total < first, (first, total)
    ts.write_back()
    mapped = ts.mapper.map_batch(E, keep_device=True)
    res = ts.model(mapped)
    for r in res:
        assert all(bool(np.isfinite(np.asarray(r["camera"][k], dtype=np.float64)).all()) for k in ("tran", "rot"))
