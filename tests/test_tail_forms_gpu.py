"""GPU half of the bottleneck-tail form sweep: every config of ops.BOTTLENECK_TAIL_CONFIGS at its stage's production size (B = 64, 2 and
3), on every kernel form the selector finds eligible, with a bf16 and (CN > 0) an fp8 o.  y is pinned to a float64 reference and o to a
float64 conv1 of the kernel's own y at ~1.5k sampled rows, the fp8 o to the bf16 o converted bit for bit, both outputs to the default
form over the whole tensor, and each launch to its second launch bit for bit; nothing may be written past y or o.  One backbone forward
per mode that reaches the fused tail checks that the sweep holds every tail call the model makes."""
import os

import pytest
import torch

from nopesac_amd.ops import BOTTLENECK_TAIL_CONFIGS
from tests import conv_routing as CR
from tests import tail_forms as TF

pytestmark = pytest.mark.gpu

CALLS = [(cfg, B) for cfg in sorted(BOTTLENECK_TAIL_CONFIGS) for B in TF.SWEEP_B]
WORST = {}            # form name -> {"y": (ratio, call id), "o": (ratio, call id)}
CHECKED = []          # (call id, form name, o dtype) of every combination that passed its checks


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16}[t.element_size()])


def _sweep_keys():
    """(C, C4, CN, C2, B, OH, OW, H2, W2, stride, o dtype) of every call the sweep makes."""
    keys = set()
    for cfg, B in CALLS:
        for dt in (("bf16", "fp8") if cfg[2] else ("none",)):
            keys.add(cfg + TF.stage_call(cfg, B) + (dt,))
    return keys


def _note(form, what, ratio, cid):
    w = WORST.setdefault(form, {})
    if ratio > w.get(what, (-1.0,))[0]:
        w[what] = (ratio, cid)


@pytest.mark.parametrize("cfg, B", CALLS, ids=[TF.call_id(cfg, B) for cfg, B in CALLS])
def test_every_eligible_form_matches_f64(cfg, B, device):
    from nopesac_amd import ops
    cid = TF.call_id(cfg, B)
    shape = TF.stage_call(cfg, B)
    _, OH, OW, H2, W2, stride = shape
    seed = CR.key_seed(cid)
    c = TF.build_tail(cfg, *shape, device, seed)
    sw = sum(bit for env, bit in ops.TAIL_SWITCHES.items() if os.environ.get(env) is not None)
    default, mask = ops.bottleneck_tail_forms(*cfg, c.M, stride, (H2, W2) == (OH, OW), sw)
    assert default >= 0 and (mask >> default) & 1, (default, mask)
    forms = [default] + [f for f in TF.forms_of(mask) if f != default]
    rows = CR.sample_rows(c.M, B, OH, OW, seed)
    ry, Ay = TF.reference_y(c, rows)
    dts = (False, True) if c.CN else (False,)
    failures = []
    ref_out = {}                                   # o_fp8 -> (y, o) of the default form
    over448 = False
    for f in forms:
        name = ops.TAIL_FORMS[f]
        bf16_out = None
        for o_fp8 in dts:
            tag = "%s/%s" % (name, ("fp8" if o_fp8 else "bf16") if c.CN else "no o")
            y, o, ybuf, obuf = TF.run_tail(c, f, o_fp8)
            torch.cuda.synchronize()
            bad = []
            if not bool(torch.isfinite(y).all()):
                bad.append("y: %d non-finite values" % int((~torch.isfinite(y)).sum()))
            if not bool(ybuf[c.M:].isnan().all()):
                bad.append("y: written past its end")
            if c.CN:
                if not bool(torch.isfinite(o.float()).all()):
                    bad.append("o: %d non-finite values" % int((~torch.isfinite(o.float())).sum()))
                if not bool(obuf[c.M:].float().isnan().all()):
                    bad.append("o: written past its end")
            if bad:
                failures.append("%s: %s" % (tag, "; ".join(bad)))
                continue
            ym = TF.rows_of(y, rows)
            if not o_fp8:
                ratio, (i, n) = CR.error_ratio(ym, ry, Ay, torch.bfloat16)
                _note(name, "y", ratio, cid)
                if ratio > 1.0:
                    failures.append("%s: y row %d channel %d at %.3g x the tolerance" % (tag, int(rows[i]), n, ratio))
                if c.CN:
                    ro, Ao = TF.reference_o(c, ym)
                    ratio, (i, n) = CR.error_ratio(TF.rows_of(o, rows), ro, Ao, torch.bfloat16)
                    _note(name, "o", ratio, cid)
                    if ratio > 1.0:
                        failures.append("%s: o row %d channel %d at %.3g x the tolerance" % (tag, int(rows[i]), n, ratio))
                    over448 = over448 or bool((o.float() > 448.0).any())
                bf16_out = (y, o)
            else:
                y16, o16 = bf16_out
                if not torch.equal(_bits(y), _bits(y16)):
                    failures.append("%s: y differs from the bf16-o launch" % tag)
                if not torch.equal(_bits(o), _bits(TF.q8(o16))):
                    failures.append("%s: fp8 o is not the bf16 o converted (%.3g)" % (tag, TF.fp8_ratio(o, o16)))
            if o_fp8 not in ref_out:
                ref_out[o_fp8] = (y, o)
            else:
                y0, o0 = ref_out[o_fp8]
                agree = max(CR.full_agreement(y, y0), CR.full_agreement(o, o0) if c.CN else 0.0)
                if agree > 1.0:
                    failures.append("%s: against the default form at %.3g x the bound" % (tag, agree))
            y2, o2, _, _ = TF.run_tail(c, f, o_fp8)
            torch.cuda.synchronize()
            if not torch.equal(_bits(y2), _bits(y)) or (c.CN and not torch.equal(_bits(o2), _bits(o))):
                failures.append("%s: a second launch is not bit-identical" % tag)
            del y2, o2, ybuf, obuf
            CHECKED.append((cid, name, ("fp8" if o_fp8 else "bf16") if c.CN else "none"))
    # the default selection (form=None) launches the selector's default form
    y, o, _, _ = TF.run_tail(c, None, False)
    torch.cuda.synchronize()
    y0, o0 = ref_out[False]
    if not torch.equal(_bits(y), _bits(y0)) or (c.CN and not torch.equal(_bits(o), _bits(o0))):
        failures.append("default selection: differs from the forced default form %s" % ops.TAIL_FORMS[default])
    if c.CN:
        assert over448, "no o value above e4m3fn's 448: the fp8 saturation is not exercised"
    assert not failures, failures
    del c, ref_out, y, o
    torch.cuda.empty_cache()


def _fresh_model(device, overrides=()):
    """A bf16 model with the synthetic checkpoint, built now (Backbone.__init__ reads the tail environment switches)."""
    from nopesac_amd.config import get_cfg
    from nopesac_amd.registry import build_model
    from nopesac_amd.synth import synth_state_dict
    cfg = get_cfg()
    cfg.merge_from_file(os.path.join(CR.ROOT, "configs", "inference_mp3d.yaml"))
    cfg.merge_from_list(["MODEL.DEVICE", str(device), "MODEL.AMD.COMPUTE_DTYPE", "bfloat16"] + list(overrides))
    cfg.freeze()
    model = build_model(cfg).eval()
    model.load_state_dict(synth_state_dict(50))
    return model


MODES = {"bf16": ((), {}), "fp8": (("MODEL.AMD.BACKBONE_FP8", True), {}), "res4_fused": ((), {"NOPESAC_TAIL_RES4_FUSED": "1"}),
         "res3_edges_unfused": ((), {"NOPESAC_RES3_EDGES_UNFUSED": "1"})}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sweep_holds_every_tail_the_backbone_launches(mode, device, monkeypatch):
    """One backbone forward of one 480 x 640 pair (B = 2) per mode that reaches the fused tail, every ops.bottleneck_tail call recorded:
    each (config, batch, spatial size, source, stride, o dtype) must be one the sweep above runs."""
    from nopesac_amd import ops
    from nopesac_amd.synth import synth_pair
    overrides, env = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    model = _fresh_model(device, overrides)
    inp = [synth_pair(0)]
    if mode == "fp8":
        model.calibrate_fp8(inp)
    seen = []
    orig = ops.bottleneck_tail

    def tail(b, w3, s3, b3, **kw):
        B, OH, OW, C = b.shape
        x2, w1 = kw.get("x2"), kw.get("w1")
        C2, CN = (x2.shape[3] if x2 is not None else 0), (w1.shape[0] if w1 is not None else 0)
        H2, W2 = (x2.shape[1], x2.shape[2]) if x2 is not None else (0, 0)
        stride = kw.get("stride", 1) if x2 is not None else 1
        dt = ("fp8" if kw.get("o_fp8") else "bf16") if CN else "none"
        seen.append((C, w3.shape[0], CN, C2, B, OH, OW, H2, W2, stride, dt))
        return orig(b, w3, s3, b3, **kw)

    monkeypatch.setattr(ops, "bottleneck_tail", tail)
    x = model.preprocess_image(inp)
    assert x.shape[0] == 2 and tuple(x.shape[1:3]) == (480, 640), x.shape
    with torch.no_grad():
        model.backbone(x)
    torch.cuda.synchronize()
    assert seen, "no fused tail launched"
    assert set(seen) <= _sweep_keys(), sorted(set(seen) - _sweep_keys())
    if mode in ("fp8", "res4_fused"):
        assert any(k[0] == 256 for k in seen), "res4 tails expected in this mode"
    del model
    torch.cuda.empty_cache()


def test_zz_worst_ratio_per_form(capsys):
    """The sweep's summary: combinations checked and the worst sampled error / tolerance of y and o per form."""
    with capsys.disabled():
        print("\nbottleneck tail sweep: %d (call, form, o dtype) combinations checked" % len(CHECKED))
        for form in sorted(WORST):
            w = WORST[form]
            n = sum(1 for _, f, _ in CHECKED if f == form)
            print("  %-9s %3d combos  y %.3f (%s)  o %s" % (form, n, w["y"][0], w["y"][1],
                                                          "%.3f (%s)" % w["o"] if "o" in w else "-"))
    assert all(v[0] <= 1.0 for w in WORST.values() for v in w.values())
