"""Bit-level digest of the training path (nopesac_amd/training.py), for holding a refactor of it to equality: every trainer runs two
rounds of losses -> backward -> step_from_cfg on fixed-seed inputs at the small shapes of the GPU suites (B = 2, nq = 50 for the camera
head and the matcher with 5 Sinkhorn iterations, nq = 7 and a 6 x 8 encoder map for the plane head), and the script prints one sha256
per configuration over the losses, every gradient by sorted key, input_grads, the parameters after both steps, the optimiser state and
the buffers (`heads_groups2` / `pyramid_groups2`: the same rounds on view groups) - and the ordered list of library entry points the rounds called (run-length encoded; --calls count prints only its length
and hash).  Everything on this path is f32 and deterministic, so two commits that compute the same thing print the same text.  Only
public API of the trainers is used.

    python scripts/training_digest.py > digest.txt        # at either commit; compare the files"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import _lib  # noqa: E402
from nopesac_amd import training as T  # noqa: E402
from nopesac_amd.config import get_cfg  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from tests import golden_inputs as GI  # noqa: E402
from tests.util import make_model, nhwc  # noqa: E402

CALLS = []                             # the entry points called since the last reset, in order
ROUNDS = 2


def record_library_calls():
    _lib.load()
    entries = vars(_lib.C)

    def wrap(name, fn):
        def call(*args):
            CALLS.append(name)
            return fn(*args)
        return call
    for name, fn in list(entries.items()):
        entries[name] = wrap(name, fn)


class Digest:
    def __init__(self):
        self.h = hashlib.sha256()

    def add(self, tag: str, tensors: dict):
        for k in sorted(tensors):
            t = tensors[k]
            self.h.update(("%s/%s" % (tag, k)).encode())
            if t is not None:
                t = t.detach().cpu().contiguous()
                self.h.update(("%s%s" % (t.dtype, tuple(t.shape))).encode())
                self.h.update(t.numpy().tobytes())

    def trainer(self, tag: str, tr):
        self.add(tag + ".params", tr.params)
        self.add(tag + ".buffers", getattr(tr, "buffers", {}))
        self.add(tag + ".state", {"%s/%s" % (k, s): v for k, st in tr.state.items() for s, v in st.items()})
        self.h.update(("%s.steps=%d" % (tag, tr.steps)).encode())


def solver_cfg():
    """The default solver with every optimiser group told apart and the global-norm clip active."""
    cfg = get_cfg()
    cfg.merge_from_list(["SOLVER.OPTIMIZER", "ADAMW", "SOLVER.BASE_LR", 0.01, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.WEIGHT_DECAY_NORM", 0.5,
                         "SOLVER.WEIGHT_DECAY_EMBED", 0.25, "SOLVER.SEM_SEG_HEAD_MULTIPLIER", 0.5, "SOLVER.CLIP_GRADIENTS.ENABLED", True,
                         "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.01])
    return cfg


def rounds(d: Digest, trainers: dict, one_round):
    """ROUNDS x (one_round(i) -> (losses, grads, input_grads); step_from_cfg of every trainer), then the trainers' tensors."""
    cfg = solver_cfg()
    del CALLS[:]                       # (the inference launches that made the inputs are not the trainers')
    for i in range(ROUNDS):
        losses, grads, input_grads = one_round(i)
        d.add("losses%d" % i, losses)
        d.add("grads%d" % i, grads)
        d.add("input_grads%d" % i, input_grads)
        for tr in trainers.values():
            tr.step_from_cfg(cfg)
    for tag, tr in trainers.items():
        d.trainer(tag, tr)


# ---- the configurations ------------------------------------------------------------------------------------------------------------------
def refine(dev, d):
    from tests.test_training_gpu import _batch
    nq = 50
    cases, st, geo, di, gt = _batch(nq, (7, 32), (67, 92))
    tr = T.RefineTrainer.from_state_dict(synth_state_dict(nq), nq, dev)
    to = lambda t: t.to(dev)
    f = {k: to(st(k)).requires_grad_(True) for k in ("trans_feat", "rot_feat", "init_trans", "init_rot")}

    def one(i):
        losses = tr.losses(to(di["A"]), to(di["p1"]), to(di["p2"]), to(di["n1"]), to(di["n2"]), f["init_trans"], f["init_rot"], f["trans_feat"],
                           f["rot_feat"], to(gt), suffix="initCamRef", weight=0.5)
        return losses, tr.backward(losses), tr.input_grads
    rounds(d, {"refine": tr}, one)


def camera(conv_stacks, **kw):
    def run(dev, d):
        from tests.test_pose_net_training_gpu import _losses, _setup
        nq, c, sd, model, head, feats = _setup(dev)
        tr = T.CameraHeadTrainer.from_head(head, conv_stacks=conv_stacks, feature_grads=conv_stacks, **kw)

        def one(i):
            losses = _losses(tr, head, feats, c, dev)
            grads = tr.backward(losses)
            d.add("conv_feats%d" % i, dict(enumerate(tr.conv_feats)))
            d.add("recorded%d" % i, {"%s%d" % (k, j): t for k, ts in tr.recorded.items() for j, t in enumerate(ts)})
            return losses, grads, tr.input_grads
        rounds(d, {"camera": tr}, one)
    return run


def matcher(dev, d):
    from tests.test_matcher_training_gpu import HEAD_CASES, _pad, gt_corr_case
    nq, picked = 50, HEAD_CASES[:1] + HEAD_CASES[2:3]                  # (7, 5) and (32, 33) planes
    cases = [GI.matcher_case(n1, n2, s) for n1, n2, s in picked]
    to = lambda t: t.to(dev)
    app = to(torch.stack([_pad(c[0], nq) for c in cases] + [_pad(c[1], nq) for c in cases])).requires_grad_(True)
    n_all = to(torch.tensor([c[0] for c in picked] + [c[1] for c in picked], dtype=torch.int32))
    cam7, p1, p2 = to(torch.stack([c[2] for c in cases])), to(torch.stack([_pad(c[3], nq) for c in cases])), to(torch.stack([_pad(c[4], nq) for c in cases]))
    gt = to(torch.stack([gt_corr_case(n1, n2, s, nq) for n1, n2, s in picked]))
    tr = T.MatchingHeadTrainer.from_state_dict(synth_state_dict(nq), nq, dev)

    def one(i):
        losses = tr.matching_losses(app, n_all, cam7, p1, p2, gt, suffix="t", iterations=5)
        grads = tr.backward(losses)
        d.add("last%d" % i, tr.last)
        return losses, grads, tr.input_grads
    rounds(d, {"matcher": tr}, one)


NQ_PLANE, H5, W5 = 7, 6, 8


def plane_inputs(dev):
    """The frozen trunk's tensors of the plane head at B = 2 on a 6 x 8 encoder map, and targets at the mask resolution."""
    from tests.test_plane_heads_training_gpu import _head_targets
    head = make_model(dev, nq=NQ_PLANE).sem_seg_head
    feats = {k: nhwc(v).to(dev) for k, v in GI.feature_maps(21, H5, W5, batch=2).items()}
    memory, pos, p1 = head.decoder_training_inputs(feats)
    _, f32_feats = head.pyramid_training_inputs(feats)
    hs = head.training_inputs(feats)[0]
    return dict(memory=memory, pos=pos, p1=p1, hs=hs, feats=f32_feats, targets=_head_targets("border_s4", dev, p1.shape[1], p1.shape[2]))


def plane_trainers(dev):
    from tests import plane_pyramid_forms as P
    sd = synth_state_dict(NQ_PLANE)
    c = P.pyramid_inputs((2, H5, W5))                                  # the pyramid at its settled biases, as the suite trains it
    pyr_sd = dict({k: v for k, v in sd.items() if k.startswith(P.PREFIX)}, **c["sd"], **c["bufs"])
    return (T.PlaneInstanceHeadsTrainer.from_state_dict(sd, NQ_PLANE, dev), T.PlaneDecoderTrainer.from_state_dict(sd, NQ_PLANE, dev),
            T.PlanePyramidTrainer.from_state_dict(pyr_sd, dev, feature_grads=True))


def heads(groups=None):
    """groups=2: the criterion on view groups (one image each at B = 2), with the per-group losses in the digest."""
    kw = {} if groups is None else {"groups": groups}

    def run(dev, d):
        x = plane_inputs(dev)
        tr, _, _ = plane_trainers(dev)
        hs, p1 = x["hs"].clone().requires_grad_(True), x["p1"].clone().requires_grad_(True)

        def one(i):
            losses, indices = tr.losses(hs, p1, x["targets"], **kw)
            grads = tr.backward(losses)
            d.add("indices%d" % i, {k: v for k, v in indices.items() if torch.is_tensor(v)})
            if groups is not None:
                for g, per in enumerate(tr.criterion.last["group_losses"]):
                    d.add("group%d.losses%d" % (g, i), per)
            return losses, grads, tr.input_grads
        rounds(d, {"heads": tr}, one)
    return run


def decoder(p):
    def run(dev, d):
        x = plane_inputs(dev)
        hd, dec, _ = plane_trainers(dev)

        def one(i):
            losses, _ = dec.losses(hd, x["memory"], x["pos"], x["p1"], x["targets"], p=p, seed=3, step=i)
            grads = dec.backward(losses)
            d.add("dec.grads%d" % i, dec.grads)
            return losses, grads, dec.input_grads
        rounds(d, {"decoder": dec, "heads": hd}, one)
    return run


def pyramid(groups=None):
    """groups=2: the BatchNorm statistics and the criterion on view groups (one image each at B = 2)."""
    kw = {} if groups is None else {"groups": groups}

    def run(dev, d):
        x = plane_inputs(dev)
        hd, _, pyr = plane_trainers(dev)

        def one(i):
            losses, _ = pyr.losses(hd, x["feats"], x["memory"], x["hs"], x["targets"], **kw)
            grads = pyr.backward(losses)
            d.add("pyr.grads%d" % i, pyr.grads)
            return losses, grads, pyr.input_grads
        rounds(d, {"pyramid": pyr, "heads": hd}, one)
    return run


def shared_memory(dev, d):
    """Decoder (p = 0.1) and pyramid on one memory leaf, both in front of the instance heads: one graph, the heads' backward."""
    x = plane_inputs(dev)
    hd, dec, pyr = plane_trainers(dev)
    leaf = x["memory"].detach().clone().requires_grad_(True)

    def one(i):
        for t in [leaf] + list(dec.params.values()) + list(pyr.params.values()):
            t.grad = None
        p1 = pyr.forward(x["feats"], leaf, 2)
        hs = dec.forward(leaf, x["pos"], 2, 0.1, 3, i)
        losses, _ = hd.losses(hs, p1, x["targets"])
        grads = dict(hd.backward(losses))
        grads.update({k: t.grad for tr in (dec, pyr) for k, t in tr.params.items()})
        return losses, grads, dict(hd.input_grads, memory=leaf.grad)
    rounds(d, {"decoder": dec, "pyramid": pyr, "heads": hd}, one)


def backbone(dev, d):
    """BackboneTrainer at N = 2, 64 x 96 (tests/backbone_forms.py): forward, backward_from unit-normal cotangents at the four maps."""
    from tests import backbone_forms as BF
    x, cots = BF.net_inputs(BF.NET_CASES[0])
    tr = T.BackboneTrainer.from_state_dict(BF.backbone_state_dict(), dev)
    x, cots = x.to(dev), {k: v.to(dev) for k, v in cots.items()}

    def one(i):
        feats = tr.forward(x)
        return {k: v.detach() for k, v in feats.items()}, tr.backward_from(cots), tr.input_grads
    rounds(d, {"backbone": tr}, one)


def train_step(dev, d):
    """Two TrainStep steps on two 480 x 640 pairs (the only size the camera head admits), dropout and augmentation on."""
    import tempfile

    from nopesac_amd.registry import build_model
    from nopesac_amd.train_step import TrainStep
    from tests import train_step_forms as F
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "inference_mp3d.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(dev), "MODEL.AMD.COMPUTE_DTYPE", "float32", "DATALOADER.AUGMENTATION", True])
    model = build_model(cfg).eval()
    model.load_state_dict(synth_state_dict(50))
    ts = TrainStep.from_model(model, cfg, seed=5)
    entries = F.pair_entries(2, 480, 640, tempfile.mkdtemp(prefix="digest_"))
    del CALLS[:]
    for i in range(ROUNDS):
        d.add("losses%d" % i, ts.step(entries))
        d.add("grads%d" % i, {k: p.grad for t in ts.trainers.values() for k, p in t.params.items()})
    ts.check()
    for tag, tr in ts.trainers.items():
        d.add(tag + ".params", tr.params)
        d.add(tag + ".buffers", getattr(tr, "buffers", {}))
    sd = ts.optimizer.state_dict()
    d.add("optimizer", {"%s/%s" % (k, n): v for k, st in sd["state"].items() for n, v in st.items() if torch.is_tensor(v)})


CONFIGS = (("refine", refine), ("camera", camera(False)), ("camera_conv_stacks", camera(True)), ("matcher", matcher), ("heads", heads()),
           ("decoder_p0", decoder(0.0)), ("decoder_p0.1", decoder(0.1)), ("pyramid", pyramid()), ("decoder_pyramid_shared_memory", shared_memory),
           ("backbone", backbone), ("camera_conv_stacks_batch_stats", camera(True, batch_stats=True)), ("heads_groups2", heads(2)),
           ("pyramid_groups2", pyramid(2)), ("train_step", train_step))


def run_length(names):
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return ["%s x%d" % (n[len("nopesac_"):], k) if k > 1 else n[len("nopesac_"):] for n, k in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", choices=("list", "count"), default="list")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    record_library_calls()
    for name, fn in CONFIGS:
        if a.only and name not in a.only.split(","):
            continue
        d = Digest()
        fn(dev, d)
        torch.cuda.synchronize()
        print("digest %-30s %s" % (name, d.h.hexdigest()))
        print("calls  %-30s n=%d sha256=%s" % (name, len(CALLS), hashlib.sha256("\n".join(CALLS).encode()).hexdigest()))
        if a.calls == "list":
            line = "   "
            for item in run_length(CALLS):
                if len(line) + len(item) > 150:
                    print(line)
                    line = "   "
                line += " " + item
            print(line)
        sys.stdout.flush()


if __name__ == "__main__":
    main()
