"""GPU half of the head sweep: every transformer-tail call of the bf16 model on every eligible kernel form, every attention shape on the
builds that serve it and on the scalar f32 kernel, and the fused GNN layer with the product's offsets and aliasing - each against a float64
reference at sampled rows with a per-element error bound (tests/head_forms.py).  One bf16 forward per benchmark leg and one one-pair forward
confirm that the sweep covers every call the model makes."""
import pytest
import torch

from tests import head_forms as HF

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
WORST = {}           # family / form -> (worst ratio, case)


def _note(fam, q, case):
    if q > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (q, case)


@pytest.fixture(scope="module")
def device():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


# ---------------------------------------------------------------------------------------------------------------------------- tails
def _tail_cases():
    cases = []
    for key in HF.production_tails():
        _, entry, M, pre, skip, want, n_pos, n_proj, pos_rows, pf = key
        cases.append((entry, M, pre, skip, n_pos, n_proj, pos_rows, pf))
    cases.append(("encoder_tail", 19200, False, False, 0, 0, 300, False))       # the unchained entries
    cases.append(("encoder_tail", 600, False, False, 0, 0, 300, False))
    cases.append(("transformer_tail", 2100, False, False, 512, 256, 300, False))  # 7 x 300: ragged 96- and 128-token tiles
    cases.append(("transformer_tail", 2147, True, False, 512, 256, 50, False))
    cases.append(("transformer_tail", 37, True, True, 256, 0, 50, True))
    return sorted(set(cases))


def _case_id(c):
    entry, M, pre, skip, n_pos, n_proj, pos_rows, pf = c
    return "%s_M%d_%s%s_p%d+%d_pos%d%s" % (entry, M, "pre" if pre else "post", "_skip" if skip else "", n_pos, n_proj, pos_rows, "_pf" if pf else "")


@pytest.mark.parametrize("case", _tail_cases(), ids=_case_id)
def test_transformer_tail_forms_against_f64(case, device):
    from nopesac_amd import ops
    entry, M, pre, skip, n_pos, n_proj, pos_rows, pf = case
    c = HF.build_tail(M, pre, skip, n_pos, n_proj, pos_rows, device, seed=M + 7 * n_pos + 3 * pre + skip)
    rows = HF.sample_tail_rows(M, pos_rows, seed=M)
    ref = HF.tail_reference(c, rows)
    want = ("y", "y16", "ypos16", "yn") if pre else ("y", "y16", "ypos16")
    default, mask = ops.transformer_tail_forms(M, pre, skip, n_pos + n_proj, 0)
    forms = HF.forms_of(mask) if entry == "transformer_tail" else [None]
    first = None
    for form in forms:
        name = ops.TRANSFORMER_TAIL_FORMS[default if form is None else form]
        out, bufs = HF.run_tail(c, form, want, entry=entry)
        torch.cuda.synchronize()
        for k, b in bufs.items():                        # the spare rows behind M are untouched
            assert torch.isnan(b[M:].float()).all(), (name, k)
        got = {k: v[rows.to(device)].float().cpu() for k, v in out.items()}
        nk = got["yn"] if pre else got["y"]
        r, E = ref["n"]
        q = HF.error_ratio(nk, r, HF.out_tol(r, E, torch.float32))[0]
        if pre:
            ru, Eu = ref["u"]
            q = max(q, HF.error_ratio(got["y"], ru, HF.out_tol(ru, Eu, torch.float32))[0])
        _note("tail " + name, q, _case_id(case))
        assert q <= 1.0, (name, q)
        bo = HF.tail_outputs_reference(c, rows, nk)
        assert torch.equal(got["y16"].to(BF), bo["y16"]), name
        assert torch.equal(got["ypos16"].to(BF), bo["ypos16"]), name
        for k in ("proj_pos", "proj"):
            if k in got:
                rp, A = bo[k]
                qp = HF.error_ratio(got[k], rp, HF.out_tol(rp, HF.GEMM * A, BF))[0]
                _note("tail %s %s" % (name, k), qp, _case_id(case))
                assert qp <= 1.0, (name, k, qp)
        out2, _ = HF.run_tail(c, form, want, entry=entry)
        for k in out:
            assert torch.equal(out[k].view(torch.int16 if out[k].dtype == BF else torch.int32),
                               out2[k].view(torch.int16 if out2[k].dtype == BF else torch.int32)), ("repeat", name, k)
        if form == 0 and M <= 2048:                      # the launch with the weight prefetch workgroups computes the same bits
            out3, _ = HF.run_tail(c, form, want, prefetch=True)
            for k in out:
                assert torch.equal(out[k].float().nan_to_num(7.0), out3[k].float().nan_to_num(7.0)), ("prefetch", name, k)
        if form in (0, 1) and first is not None:         # the 32- and 64-token kernels sum in the same order: bit-identical
            for k in out:
                assert torch.equal(out[k].float(), first[k].float()), ("t64 vs t32", k)
        if form == 0:
            first = out


# ---------------------------------------------------------------------------------------------------------------------------- attention
def _attention_cases():
    cases = set()
    for key in HF.PRODUCTION:
        if key[0] == "attention":
            _, B, Lq, Lk, q_ld, k_ld, v_ld, _, _ = key
            cases.add((B, Lq, Lk, q_ld, k_ld, v_ld, "prod"))
    cases.add((4, 300, 300, 512, 512, 256, "ragged"))
    cases.add((4, 128, 128, 256, 256, 256, "ragged"))
    cases.add((3, 50, 300, 256, 1536, 1536, "ragged"))
    return sorted(cases)


@pytest.mark.parametrize("case", _attention_cases(), ids=lambda c: "B%d_q%d_k%d_ld%d-%d-%d_%s" % c)
def test_attention_against_f64(case, device):
    from nopesac_amd import ops
    B, Lq, Lk, q_ld, k_ld, v_ld, kind = case
    c = HF.build_attention(B, Lq, Lk, (q_ld, k_ld, v_ld), False, seed=B * 1000 + Lq + Lk, device=device)
    ql = kl = None
    if kind == "ragged":                                 # ragged lengths, an empty key set, an empty query set
        qv = [Lq, Lq - 5, 1, 0][:B] + [Lq] * max(0, B - 4)
        kv = [Lk - 1, 0, 33, Lk][:B] + [Lk] * max(0, B - 4)
        ql = torch.tensor(qv, dtype=torch.int32, device=device)
        kl = torch.tensor(kv, dtype=torch.int32, device=device)
    imgs = sorted({0, B - 1, B // 2})
    for build in ("mfma_bf16io", "mfma_f32io", "scalar_f32"):
        io16, mfma = build == "mfma_bf16io", build != "scalar_f32"
        q, k, v = (t.to(BF) for t in (c.q_d, c.k_d, c.v_d)) if io16 else (c.q_d, c.k_d, c.v_d)
        qa, ka, va = q[:, :256], k[:, :256], v[:, :256]
        o = ops.attention(qa, ka, va, B, Lq, Lk, 8, c.scale, ql, kl, mfma_bf16=mfma)
        o2 = ops.attention(qa, ka, va, B, Lq, Lk, 8, c.scale, ql, kl, mfma_bf16=mfma)
        torch.cuda.synchronize()
        assert torch.equal(o, o2), ("repeat", build)
        cr = c
        if io16:                                         # the reference reads what the kernel reads: the bf16 tensors
            cr = HF.build_attention(B, Lq, Lk, (q_ld, k_ld, v_ld), False, seed=B * 1000 + Lq + Lk, device=None)
            cr.q, cr.k, cr.v = q.cpu(), k.cpu(), v.cpu()
        fam = "attention %s %s" % (build, "w10" if (mfma and 256 < Lq <= 320) else ("w4" if mfma else "scalar"))
        for b in imgs:
            qn = None if ql is None else int(ql[b])
            kn = None if kl is None else int(kl[b])
            r, E = HF.attention_reference(cr, b, qlen=qn, klen=kn, mfma=mfma)
            got = o[b * Lq:(b + 1) * Lq].float().cpu()
            dt = BF if io16 else torch.float32
            qq, i = HF.error_ratio(got, r, HF.out_tol(r, E, dt))
            _note(fam, qq, "B%d_q%d_k%d img %d" % (B, Lq, Lk, b))
            assert qq <= 1.0, (build, b, qq, divmod(i, 256))
            if qn is not None:
                assert (got[qn:] == 0).all() and (kn > 0 or (got == 0).all()), (build, b)


# ---------------------------------------------------------------------------------------------------------------------------- GNN
@pytest.mark.parametrize("pairs", [32, 1])
@pytest.mark.parametrize("nq", [50, 64, 100, 128])
def test_gnn_layer_against_f64(nq, pairs, device):
    """A self launch and the two cross launches of one layer step with the product's offsets: the second cross launch reads `nxt` at set
    0 and writes it at set P.  Every row < nq against the f64 layer (rows >= the set's length get a zero message)."""
    from nopesac_amd import ops
    P = pairs
    W = HF.build_gnn_weights(nq + P)
    Wd, Wn = HF.gnn_weights_device(W, device), HF.gnn_weights_device(HF.build_gnn_weights(nq + P + 1), device)
    x = HF.gnn_features(2 * P, nq, nq * 3 + P)
    lens = HF.gnn_lengths(nq, 2 * P, nq)
    cur, ld = x.to(device), lens.to(device)
    pf = 2 * P <= 16

    def nan_buf():
        return torch.full((2 * P + 1, nq, 256), float("nan"), device=device)
    nxt = nan_buf()
    ops.gnn_layer(cur, 0, cur, 0, nxt, 0, 2 * P, ld, Wd, Wn if pf else None, P)
    nxt_plain = nan_buf()
    ops.gnn_layer(cur, 0, cur, 0, nxt_plain, 0, 2 * P, ld, Wd)
    crs = nan_buf()
    ops.gnn_layer(cur, 0, cur, P, crs, 0, P, ld, Wd)
    ops.gnn_layer(cur, P, crs, 0, crs, P, P, ld, Wd, Wn if pf else None, 2 * P)
    crs_plain = nan_buf()
    ops.gnn_layer(cur, 0, cur, P, crs_plain, 0, P, ld, Wd)
    ops.gnn_layer(cur, P, crs_plain, 0, crs_plain, P, P, ld, Wd)
    nxt2 = nan_buf()
    ops.gnn_layer(cur, 0, cur, 0, nxt2, 0, 2 * P, ld, Wd, Wn if pf else None, P)
    torch.cuda.synchronize()
    n = 2 * P                                            # (set 2P: the NaN guard, compared below)
    assert torch.equal(nxt[:n], nxt2[:n]), "repeat"
    assert torch.equal(nxt[:n], nxt_plain[:n]) and torch.equal(crs[:n], crs_plain[:n]), "W_next launch differs from the plain one"
    assert torch.isnan(nxt[2 * P]).all() and torch.isnan(crs[2 * P]).all(), "the spare set was written"
    assert torch.isfinite(nxt[:2 * P]).all() and torch.isfinite(crs[:2 * P]).all()
    nxt_c, crs_c = nxt.cpu(), crs.cpu()
    L = [int(v) for v in lens]
    sets = sorted({0, 1, 2, 3, 4, 5, 6, 7, 8, 9, P - 1, P, 2 * P - 1} & set(range(2 * P)))
    for s in sets:                                       # self: set s attends to itself
        r, E = HF.gnn_reference(W, x[s], x[s], L[s], L[s])
        q, i = HF.error_ratio(nxt_c[s], r, HF.out_tol(r, E, torch.float32))
        _note("gnn self", q, "nq%d P%d set %d (n %d)" % (nq, P, s, L[s]))
        assert q <= 1.0, ("self", s, L[s], q, divmod(i, 256))
    for b in sorted({0, 1, 2, 3, 4, P - 1} & set(range(P))):
        r, E = HF.gnn_reference(W, x[b], x[P + b], L[b], L[P + b])                  # view 0 attends to view 1
        q, i = HF.error_ratio(crs_c[b], r, HF.out_tol(r, E, torch.float32))
        _note("gnn cross", q, "nq%d P%d pair %d (n %d / %d)" % (nq, P, b, L[b], L[P + b]))
        assert q <= 1.0, ("cross 0", b, q, divmod(i, 256))
        r, E = HF.gnn_reference(W, x[P + b], crs_c[b], L[P + b], L[b])              # view 1 attends to the UPDATED view 0
        q, i = HF.error_ratio(crs_c[P + b], r, HF.out_tol(r, E, torch.float32))
        _note("gnn cross aliased", q, "nq%d P%d pair %d (n %d / %d)" % (nq, P, b, L[P + b], L[b]))
        assert q <= 1.0, ("cross 1", b, q, divmod(i, 256))


def test_gnn_empty_key_set_gives_a_zero_message(device):
    """nkey = 0: the message is 0 before the merge projection, so the output is x + LN2(relu(x W0x + bf16(LN1(0)) W0m) W2) - finite."""
    from nopesac_amd import ops
    nq = 64
    W = HF.build_gnn_weights(5)
    x = HF.gnn_features(2, nq, 6)
    lens = torch.tensor([40, 0], dtype=torch.int32)
    out = torch.full((2, nq, 256), float("nan"), device=device)
    ops.gnn_layer(x.to(device), 0, x.to(device), 1, out, 0, 1, lens.to(device), HF.gnn_weights_device(W, device))
    got = out[0].cpu()
    assert torch.isfinite(got).all()
    r, E = HF.gnn_reference(W, x[0], x[1], 40, 0)
    q = HF.error_ratio(got, r, HF.out_tol(r, E, torch.float32))[0]
    _note("gnn cross", q, "empty key set")
    assert q <= 1.0, q


# ---------------------------------------------------------------------------------------------------------------------------- inventory
@pytest.mark.parametrize("leg", ["headline_mp3d_k32", "scannet_k64", "bf16_k128", "one_pair"])
def test_every_head_call_of_a_forward_is_in_the_inventory(leg, device, monkeypatch):
    import os
    import bench
    from nopesac_amd import ops
    from tests import conv_routing as CR
    from tests.test_conv_routing_gpu import LEGS
    for env in ops.TRANSFORMER_TAIL_SWITCHES:
        assert env.split("=")[0] not in os.environ, env
    config, K, routing = LEGS["headline_mp3d_k32" if leg == "one_pair" else leg]
    B = 1 if leg == "one_pair" else 32
    nq = 50 if K <= 50 else K
    seen = {}

    def rec(key, form=None):
        seen[key] = form

    o_tt, o_dt, o_et, o_att, o_gnn = ops.transformer_tail, ops.decoder_tail, ops.encoder_tail, ops.attention, ops.gnn_layer

    def tt(attn, src, W, *, pre_norm, skip_ffn=False, pos=None, want=("y",), proj_pos=None, proj=None, prefetch=None, **kw):
        M = src.shape[0]
        na, nb = (proj_pos[2] if proj_pos else 0), (proj[2] if proj else 0)
        pf = prefetch is not None and ops.TAIL_PREFETCH and M <= 64 * 32
        form = ops.TRANSFORMER_TAIL_FORMS[ops.transformer_tail_forms(M, pre_norm, skip_ffn, na + nb, 0)[0]]
        rec(HF.tail_key("transformer_tail", M, pre_norm, skip_ffn, want, na, nb, 0 if pos is None else pos.shape[0], pf), form)
        return o_tt(attn, src, W, pre_norm=pre_norm, skip_ffn=skip_ffn, pos=pos, want=want, proj_pos=proj_pos, proj=proj, prefetch=prefetch, **kw)

    def dt(attn, tgt, W, pos=None, want=("y", "y16", "ypos16")):
        M = tgt.shape[0]
        rec(HF.tail_key("decoder_tail", M, 1, 0, want, 0, 0, 0 if pos is None else pos.shape[0], False),
            ops.TRANSFORMER_TAIL_FORMS[ops.transformer_tail_forms(M, 1, 0, 0, 0)[0]])
        return o_dt(attn, tgt, W, pos=pos, want=want)

    def et(attn, src, W, pos=None, want=("y", "y16", "ypos16")):
        M = src.shape[0]
        rec(HF.tail_key("encoder_tail", M, 0, 0, want, 0, 0, 0 if pos is None else pos.shape[0], False),
            ops.TRANSFORMER_TAIL_FORMS[ops.transformer_tail_forms(M, 0, 0, 0, 0)[0]])
        return o_et(attn, src, W, pos=pos, want=want)

    def att(q, k, v, Bq, Lq, Lk, heads, scale, qlen=None, klen=None, mfma_bf16=False):
        rec(HF.attention_key(Bq, Lq, Lk, q.stride(0), k.stride(0), v.stride(0), q.dtype == BF and mfma_bf16, qlen is not None))
        return o_att(q, k, v, Bq, Lq, Lk, heads, scale, qlen, klen, mfma_bf16=mfma_bf16)

    def gnn(x, x_off, src, src_off, out, out_off, n_sets, lens, W, W_next=None, next_sets=0):
        rec(HF.gnn_key(n_sets, x.shape[1], x_off, src_off, out_off, x is src and x_off == src_off, src is out,
                       W_next is not None and ops.GNN_PREFETCH and next_sets > 0))
        return o_gnn(x, x_off, src, src_off, out, out_off, n_sets, lens, W, W_next, next_sets)

    for name, fn in (("transformer_tail", tt), ("decoder_tail", dt), ("encoder_tail", et), ("attention", att), ("gnn_layer", gnn)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(ops.TUNER, "measuring", False)
    monkeypatch.setattr(ops.TUNER, "best", {})
    monkeypatch.setattr(ops.TUNER, "loaded", {})
    ops.TUNER.load(CR.routing_path(routing))
    model = bench.build_model(device, nq, "bfloat16", (), config=config)
    g = torch.Generator().manual_seed(1000)
    raw = torch.randint(0, 256, (2 * B, 3, 480, 640), generator=g).float().to(device)
    forced = bench.make_forced(B, K, nq, device, 7)
    with torch.no_grad():
        if model.backbone.fused_stem:
            model.forward_tensors(None, B, 480, 640, forced=forced, raw_images=raw)
        else:
            x = ops.preprocess(raw, model.pixel_mean, model.pixel_std, model.backbone.STEM_CIN_PAD, model.compute_dtype)
            model.forward_tensors(x, B, 480, 640, forced=forced)
    torch.cuda.synchronize()
    print("\n%s: %d distinct head calls" % (leg, len(seen)))
    unlisted = sorted(set(seen) - set(HF.PRODUCTION), key=str)
    assert not unlisted, unlisted
    wrong = {k: (f, HF.PRODUCTION[k]) for k, f in seen.items() if f is not None and f != HF.PRODUCTION[k]}
    assert not wrong, wrong
    assert {k[0] for k in seen} == {"tail", "attention", "gnn"}
    del model, raw, forced
    torch.cuda.empty_cache()


def test_zz_worst_ratio_per_family_and_form(capsys):
    with capsys.disabled():
        print("\nhead sweep: worst sampled |kernel - f64| / tolerance per family and form")
        for fam in sorted(WORST):
            q, case = WORST[fam]
            print("  %-34s %.3f  %s" % (fam, q, case))
    assert WORST and all(q <= 1.0 for q, _ in WORST.values())
