"""GPU half of the conv routing sweep: at every shape the committed routing files route (the 54 distinct keys of routing_r5*.json, at
their production size), every kernel configuration the tuner could offer is forced through ops.conv2d and pinned to a float64 reference
at ~1.5k sampled output rows, to configuration 0 over the whole output, and to its own second launch bit for bit.  Each routing entry is
checked to launch exactly its configuration, and one bf16 forward per benchmark leg checks that the routing files hold every conv shape
the benchmark launches."""
import os

import pytest
import torch

from tests import conv_routing as CR

pytestmark = pytest.mark.gpu

KEYS = CR.load_routing()
KEY_LIST = sorted(KEYS)
FAMILY = {0: "conv_igemm (0-4)", 1: "conv_igemm (0-4)", 2: "conv_igemm (0-4)", 3: "conv_igemm (0-4)", 4: "conv_igemm (0-4)",
          7: "bfrag (7/8)", 8: "bfrag (7/8)", 9: "halo (9/10)", 10: "halo (9/10)", 11: "p8 (11)", 12: "p8 stream-K (12)",
          13: "p8n (13/14)", 14: "p8n (13/14)", 15: "p8n split-K (15)"}
WORST = {}            # family -> (worst sampled error / tolerance, key id, configuration)
REJECTED = []         # (key id, configuration) of 1-4 launches the C entry point turned down


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _forced(ops, call, cfg, m):
    """ops.conv2d of the call with the tuner forced to `cfg` (fresh decisions, nothing loaded): (output, its buffer, configuration that ran,
    the key and candidates conv2d handed the tuner)."""
    seen = []

    def choose(key, launch, extra=()):
        seen.append((key, extra))
        return cfg

    m.setattr(ops.TUNER, "measuring", True)
    m.setattr(ops.TUNER, "best", {})
    m.setattr(ops.TUNER, "loaded", {})
    m.setattr(ops.TUNER, "choose", choose)
    out, wide = call.new_out()
    CR.run_conv(call, out)
    torch.cuda.synchronize()
    return out, wide, ops.LAST_CONV_CFG[0], seen


@pytest.mark.parametrize("key", KEY_LIST, ids=[CR.key_id(k) for k in KEY_LIST])
def test_every_candidate_at_the_routed_shape_matches_f64(key, device, monkeypatch):
    from nopesac_amd import ops
    kid = CR.key_id(key)
    c = CR.parse_key(key)
    call = CR.build_call(c, device, CR.key_seed(key))
    rows = CR.sample_rows(call.M, c.B, call.OH, call.OW, CR.key_seed(key))
    r, A = CR.reference_rows(call, rows)
    monkeypatch.setattr(ops, "P8_SK_TUNABLE", [True])          # stream-K is a real candidate under NOPESAC_P8_SK=1
    extra = ops.conv_tuner_extras(call.el, c.KH, c.KW)
    out0 = None
    failures = []
    for cfg in ops.ConvTuner.CANDIDATES + extra:
        with monkeypatch.context() as m:
            out, wide, ran, seen = _forced(ops, call, cfg, m)
            (k, ex), = seen
            assert ops.TUNER.key_str(k) == key and ex == extra, (ops.TUNER.key_str(k), ex, extra)
            if ran != cfg:
                assert ran == 0 and cfg in (1, 2, 3, 4), "configuration %d rejected by the C entry point at %s: conv_eligibility " \
                                                         "does not mirror its checks" % (cfg, kid)
                REJECTED.append((kid, cfg))
                continue
            y = out.float()
            if not bool(torch.isfinite(y).all()):
                failures.append("cfg %d: %d non-finite outputs" % (cfg, int((~torch.isfinite(y)).sum())))
                continue
            if wide.shape[-1] > c.Cout and not bool(wide[..., c.Cout:].float().isnan().all()):
                failures.append("cfg %d: wrote outside its channel slice" % cfg)
            ratio, (i, n) = CR.error_ratio(CR.output_rows(call, out, rows), r, A, c.out_dtype)
            fam = FAMILY[cfg]
            if ratio > WORST.get(fam, (-1.0,))[0]:
                WORST[fam] = (ratio, kid, cfg)
            if ratio > 1.0:
                failures.append("cfg %d: sampled row %d channel %d at %.3g x the tolerance" % (cfg, int(rows[i]), n, ratio))
            if out0 is None:
                out0 = out
            else:
                agree = CR.full_agreement(out, out0)
                if agree > 1.0:
                    failures.append("cfg %d: full output against configuration 0 at %.3g x the bound" % (cfg, agree))
            again, _, ran2, _ = _forced(ops, call, cfg, m)
            if ran2 != cfg or not torch.equal(_bits(again), _bits(out)):
                failures.append("cfg %d: a second launch is not bit-identical" % cfg)
            del again, out, wide, y
    assert not failures, failures

    # every routing file that holds the key: installed into a fresh tuner state, conv2d launches exactly the recorded configuration
    for name, want in KEYS[key].items():
        with monkeypatch.context() as m:
            m.setattr(ops, "P8_SK_TUNABLE", [os.environ.get("NOPESAC_P8_SK", "0") == "1"])
            m.setattr(ops.TUNER, "measuring", False)
            m.setattr(ops.TUNER, "best", {})
            m.setattr(ops.TUNER, "loaded", {})
            ops.TUNER.load(CR.routing_path(name))
            out, _ = call.new_out()
            CR.run_conv(call, out)
            torch.cuda.synchronize()
            assert ops.LAST_CONV_CFG[0] == want, (name, want, ops.LAST_CONV_CFG[0])
            del out
    del call, out0
    torch.cuda.empty_cache()


# one routed key per kernel whose eligibility bit is clear for a reason its entry point can see (Cout = 64 / Cout = 128: no 128- / 256-wide
# column tile); the 64 -> 64 key is the only routed bf16 key outside bfrag's, halo's and p8n's bits
_K64 = "bfloat16|bfloat16|bfloat16|64|120|160|64|64|1|1|1|0|False|64|64|False|True|True|1|False|False|False"
_K128 = "bfloat16|bfloat16|bfloat16|64|60|80|128|128|3|3|1|1|False|128|128|False|True|True|1|True|True|False"
REFUSED = {"bfrag": (_K64, "bfrag_ok"), "halo": (_K64, "halo_ok"), "p8": (_K128, "p8_ok"), "p8n": (_K64, "p8n_ok"),
           "p8n_splitk": (_K64, "p8n_split_ok")}


@pytest.mark.parametrize("kernel", sorted(REFUSED))
def test_entry_point_refuses_a_routed_call_outside_its_bit(kernel, device):
    """The entry point, called directly on the key's real tensors, turns the call down with the argument error (HipKernelError from
    _lib.check) before any launch: the output buffer keeps its NaN fill."""
    from nopesac_amd import _lib, ops
    key, flag = REFUSED[kernel]
    assert key in KEYS
    c = CR.parse_key(key)
    call = CR.build_call(c, device, CR.key_seed(key))
    assert not getattr(call.el, flag)
    out, wide = call.new_out()
    L, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    x, w, sc, bi, y = (t.data_ptr() for t in (call.x, call.w, call.scale, call.bias, out))
    dims = (c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.stride, c.pad)
    if kernel == "bfrag":
        rc = L.nopesac_conv2d_nhwc_bfrag(x, w, sc, bi, None, y, *dims, c.x_cs, c.y_cs, 0, c.act, ops.BF16, 3, st)
    elif kernel == "halo":
        rc = L.nopesac_conv3x3_halo_bf16(x, w, sc, bi, y, c.B, c.H, c.W, c.Cin, c.Cout, c.act, 0, st)
    elif kernel == "p8":
        rc = L.nopesac_conv2d_nhwc_p8(x, w, sc, bi, None, y, *dims, c.x_cs, c.y_cs, 0, c.act, ops.BF16, 32, st)
    elif kernel == "p8n":
        rc = L.nopesac_conv2d_nhwc_p8n(x, w, sc, bi, y, *dims, c.x_cs, c.y_cs, c.act, 32, st)
    else:
        ws = torch.empty(2 * call.M * c.Cout, device=device, dtype=torch.float32)
        rc = L.nopesac_conv2d_nhwc_p8n_splitk(x, w, sc, bi, y, *dims, c.x_cs, c.y_cs, c.act, 32, 2, ws.data_ptr(), ws.numel() * 4, st)
    with pytest.raises(_lib.HipKernelError, match="needs Cin % 64 == 0 and Cout %"):
        _lib.check(rc, "nopesac_conv2d_nhwc_" + kernel)
    assert rc == -1
    torch.cuda.synchronize()
    assert bool(wide.isnan().all())
    del call, out, wide
    torch.cuda.empty_cache()


# the benchmark's three legs (bench.py): headline mp3d K = 32, and the `other_configs` legs with the routing file each one loads
LEGS = {"headline_mp3d_k32": ("mp3d", 32, "routing_r5.json"), "scannet_k64": ("scannet", 64, "routing_r5_scannet_k64.json"),
        "bf16_k128": ("mp3d", 128, "routing_r5_fp8_k128.json")}
# Conv shapes a leg launches that its own routing file lacks (bench.py tunes them afresh in every run of that leg).  The K = 128 file was
# tuned with the fp8 backbone, whose 3x3 / projection convs do not go through conv2d; the leg now runs the bf16 backbone, so ten of its
# backbone shapes are unrouted there.  All ten are routed in routing_r5.json, so the sweep above checks every candidate at them.
UNROUTED = {"headline_mp3d_k32": set(), "scannet_k64": set(), "bf16_k128": {
    "bfloat16|bfloat16|bfloat16|64|120|160|128|128|3|3|2|1|False|128|128|False|True|True|1|True|False|False",
    "bfloat16|bfloat16|bfloat16|64|15|20|2048|512|1|1|1|0|False|2048|512|False|True|True|1|True|False|True",
    "bfloat16|bfloat16|bfloat16|64|15|20|512|512|3|3|1|1|False|512|512|False|True|True|1|True|True|True",
    "bfloat16|bfloat16|bfloat16|64|30|40|1024|512|1|1|1|0|False|1024|512|False|True|True|1|True|False|True",
    "bfloat16|bfloat16|bfloat16|64|30|40|256|1024|1|1|1|0|True|256|1024|False|True|True|1|True|False|True",
    "bfloat16|bfloat16|bfloat16|64|30|40|256|256|3|3|1|1|False|256|256|False|True|True|1|True|True|True",
    "bfloat16|bfloat16|bfloat16|64|30|40|512|512|3|3|2|1|False|512|512|False|True|True|1|True|False|True",
    "bfloat16|bfloat16|bfloat16|64|60|80|128|128|3|3|1|1|False|128|128|False|True|True|1|True|True|False",
    "bfloat16|bfloat16|bfloat16|64|60|80|256|256|3|3|2|1|False|256|256|False|True|True|1|True|False|True",
    "bfloat16|bfloat16|bfloat16|64|60|80|512|1024|1|1|2|0|False|512|1024|False|True|True|0|True|False|True"}}


@pytest.mark.parametrize("leg", sorted(LEGS))
def test_routing_file_holds_every_conv_shape_the_benchmark_launches(leg, device, monkeypatch):
    """One bf16 forward of the benchmark's workload (32 pairs, built as bench.py builds it), every tuner key recorded: each must be in the
    routing file that leg loads (a file may hold more), but for the pinned UNROUTED shapes of the leg; every one is a key of the sweep
    above, so the sweep covers what the benchmark runs."""
    import bench
    from nopesac_amd import ops
    config, K, routing = LEGS[leg]
    B, nq = 32, (50 if K <= 50 else K)
    model = bench.build_model(device, nq, "bfloat16", (), config=config)
    g = torch.Generator().manual_seed(1000)
    raw = torch.randint(0, 256, (2 * B, 3, 480, 640), generator=g).float().to(device)
    forced = bench.make_forced(B, K, nq, device, 7)
    seen = set()
    orig = ops.TUNER.choose

    def choose(key, launch, extra=()):
        seen.add(ops.TUNER.key_str(key))
        return orig(key, launch, extra)

    monkeypatch.setattr(ops.TUNER, "measuring", False)
    monkeypatch.setattr(ops.TUNER, "best", {})
    monkeypatch.setattr(ops.TUNER, "loaded", {})
    monkeypatch.setattr(ops.TUNER, "choose", choose)
    ops.TUNER.load(CR.routing_path(routing))
    with torch.no_grad():
        if model.backbone.fused_stem:       # bench.py's device_step: the fused stem reads the raw f32 images
            model.forward_tensors(None, B, 480, 640, forced=forced, raw_images=raw)
        else:
            x = ops.preprocess(raw, model.pixel_mean, model.pixel_std, model.backbone.STEM_CIN_PAD, model.compute_dtype)
            model.forward_tensors(x, B, 480, 640, forced=forced)
    torch.cuda.synchronize()
    in_file = {k for k, files in KEYS.items() if routing in files}
    assert seen, "no conv2d launch went through the tuner"
    assert seen <= set(KEYS), sorted(seen - set(KEYS))
    assert seen - in_file == UNROUTED[leg], (sorted(seen - in_file - UNROUTED[leg]), sorted(UNROUTED[leg] - seen))
    del model, raw, forced
    torch.cuda.empty_cache()


def test_zz_worst_ratio_per_kernel_family(capsys):
    """The sweep's summary: the worst sampled error / tolerance per kernel family and the key where it occurred."""
    with capsys.disabled():
        print("\nconv routing sweep: worst sampled |kernel - f64| / tolerance per kernel family")
        for fam in sorted(WORST, key=lambda f: min(k for k, v in FAMILY.items() if v == f)):
            ratio, kid, cfg = WORST[fam]
            print("  %-18s %.3f  cfg %-2d %s" % (fam, ratio, cfg, kid))
        print("  rejected 1-4 launches: %s" % (REJECTED or "none"))
    assert all(v[0] <= 1.0 for v in WORST.values())
