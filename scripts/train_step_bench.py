"""One two-view training step (nopesac_amd/train_step.py) at the workload's shape - `--pairs` pairs of 480 x 640 (IMS_PER_BATCH 16),
dropout on, all seven trainers stepped - split into mapper (decode, augmentation, targets, normalisation) / forward / backward /
optimiser between device events, with the number of library entry points one step calls; against the SAME step with the plane head
run per view (two groups=1 passes on B images each, the form of the commits before the view groups).  The two
forms alternate round by round after a warm-up of both; the median over `--rounds` is reported with min and max of the total.  Prints
one JSON line; profiles/train_step.txt records a run.  Nothing is gated on these numbers."""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nopesac_amd import _lib  # noqa: E402
from nopesac_amd.config import get_cfg  # noqa: E402
from nopesac_amd.registry import build_model  # noqa: E402
from nopesac_amd.synth import synth_state_dict  # noqa: E402
from nopesac_amd.train_step import TrainStep  # noqa: E402
from tests import train_step_forms as F  # noqa: E402

CALLS = []


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


class PerViewStep(TrainStep):
    """TrainStep with the plane head run once per view on B images (groups=1) and the weighted loss dicts averaged."""

    def losses(self, images, pair, step):
        T = self.trainers
        B = images.shape[0] // 2
        feats = T["backbone"].forward(images)
        self._leaves = {k: feats[k].detach().requires_grad_(True) for k in ("res2", "res3", "res4", "res5")}
        t = self.criterion.prepare_targets(pair["targets"])
        per, hs, pp, mq = [], [], [], []
        for v in range(2):
            sl = slice(v * B, (v + 1) * B)
            tv = {k: (x[sl].contiguous() if torch.is_tensor(x) else x) for k, x in t.items()}
            losses, idx = T["encoder"].losses(T["heads"], T["decoder"], T["pyramid"], {k: f[sl] for k, f in self._leaves.items()}, tv,
                                              p=self.dropout, seed=self.seed, step=step)
            per.append(self.criterion.weighted(losses))
            hs.append(T["heads"]._inputs["hs"][-1])
            pp.append(T["heads"].last["pred_params"])
            mq.append(idx["match_q"][0])
        n = pair["targets"]["n"]
        two = self.two_view.losses(torch.cat(hs), torch.cat(pp), mq[0], mq[1], n[:B], n[B:], pair,
                                   {k: self._leaves[k] for k in ("res3", "res4", "res5")}, B, seed=self.seed, step=step)
        return {**{k: (per[0][k] + per[1][k]) / 2 for k in per[0]}, **two}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    record_library_calls()
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(ROOT, "configs", "inference_mp3d.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(dev), "MODEL.AMD.COMPUTE_DTYPE", "float32", "DATALOADER.AUGMENTATION", True])
    entries = F.pair_entries(a.pairs, 480, 640, tempfile.mkdtemp(prefix="train_step_bench_"))
    forms = {}
    for name, cls in (("one_pass_groups2", TrainStep), ("plane_head_per_view", PerViewStep)):
        model = build_model(cfg).eval()
        model.load_state_dict(synth_state_dict(50))
        forms[name] = cls.from_model(model, cfg, seed=1)

    def run(ts, step):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        mapped = ts.mapper.map_batch(entries, step=step, keep_device=True)
        pair = ts.targets.pair_targets(entries)
        images = ts.images(mapped)
        ev[1].record()
        losses = ts.losses(images, pair, step)
        ev[2].record()
        ts.backward(losses)
        ev[3].record()
        ts.optimizer.step()
        ev[4].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(4)]
    calls = {}
    for name, ts in forms.items():
        run(ts, 0)
        del CALLS[:]
        run(ts, 1)
        calls[name] = len(CALLS)
    times = {name: [] for name in forms}
    for r in range(a.rounds):
        for name, ts in forms.items():
            times[name].append(run(ts, 2 + r))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out = {"pairs": a.pairs, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        tot = [sum(t) for t in ts]
        out[name] = dict({k: round(med([t[i] for t in ts]), 2) for i, k in enumerate(("mapper_ms", "forward_ms", "backward_ms", "optimiser_ms"))},
                         total_ms=round(med(tot), 2), total_min_ms=round(min(tot), 2), total_max_ms=round(max(tot), 2), library_calls=calls[name])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
