"""GPU half of the stream sweep (tests/stream_forms.py): every build / path of the pooling, up-sampling, GroupNorm, LayerNorm, row-softmax,
re-layout, reduction and optimiser kernels at the sizes where their dispatch changes, each against a float64 reference of the same
operation.  Errors are judged per element against the magnitude S of the terms that make the element (never against the tensor's
maximum), no element is left out, exact kernels are compared bit for bit, and a bound is 8 x the f32 floor derived in the CPU half."""
import pytest
import torch

from tests import stream_forms as S

pytestmark = pytest.mark.gpu
WORST = {}           # family / form -> (worst error / bound, case)
F32, BF16 = torch.float32, torch.bfloat16


def _note(fam, q, case):
    print("%s %s: error / bound %.3g" % (fam, case, q))
    if q > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (q, case)


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    v = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[a.element_size()]
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(v), b.view(v))


def _exact(fam, got, want, case):
    ok = _same_bits(got, want)
    _note(fam, 0.0 if ok else float("inf"), case)
    assert ok, (fam, case)


def _put(t, device, mis):
    t = t.to(device)
    return S.misaligned(t) if mis else t


# ---------------------------------------------------------------------------------------------------------------------------- 1. pool / upsample
@pytest.mark.parametrize("case", S.POOL_CASES, ids=S.pool_case_id)
def test_pool_and_upsample_builds_against_f64(case, device):
    from nopesac_amd import ops
    dtype, C, mis = case
    bound = S.FLOOR_FACTOR * S.floor_bilinear()
    for H, W in S.POOL_HW:
        x, addend = S.pool_inputs(dtype, C, H, W)
        xd, ad = _put(x, device, mis == "x"), _put(addend, device, mis == "other")
        tag = "%s %dx%d" % (S.pool_case_id(case), H, W)
        if mis != "other":                                          # the max-pool has no second operand
            form = S.pool_form(dtype, C, mis is None)
            for k, s, p in S.POOL_KSP:
                if S.pool_out(H, k, s, p) is None or S.pool_out(W, k, s, p) is None:
                    continue
                _exact("maxpool " + form, ops.maxpool(xd, k, s, p), S.maxpool_ref(x, k, s, p).to(dtype), "%s k%d s%d p%d" % (tag, k, s, p))
        for act, add in S.bilinear_variants():
            if mis == "other" and not add:
                continue
            form = S.pool_form(dtype, C, mis is None or (mis == "other" and not add))
            got = ops.upsample2x_bilinear(xd, ad if add else None, act)
            ref, Sm, z = S.bilinear_ref(x, addend if add else None, act)
            assert float(z.abs().min()) > S.MARGIN
            vt = "%s act%d%s" % (tag, act, "+addend" if add else "")
            if dtype == F32:
                q = S.quotient(got, ref, Sm) / bound
            else:                                                   # within one bf16 ulp of the float64 result
                q = float(((got.double().cpu() - ref).abs() / S.bf16_ulp(ref)).max())
            _note("bilinear " + form, q, vt)
            assert q <= 1.0, (vt, q)
        form = S.pool_form(dtype, C, mis is None)
        got = ops.upsample2x_nearest_add(xd, ad)
        ref, _ = S.nearest_add_ref(x, addend)
        if dtype == F32:                                            # one correctly rounded add
            _exact("nearest_add " + form, got, S.up2(x) + addend, tag)
        else:
            q = float(((got.double().cpu() - ref).abs() / S.bf16_ulp(ref)).max())
            _note("nearest_add " + form, q, tag)
            assert q <= 1.0, (tag, q)


def test_pool_refuses_a_window_larger_than_the_input(device):
    from nopesac_amd import _lib, ops
    x = torch.zeros(1, 1, 1, 4, device=device)
    y = torch.full((1, 1, 1, 4), 7.0, device=device)
    with pytest.raises(_lib.HipKernelError, match="maxpool"):
        ops._C.nopesac_maxpool_nhwc(x.data_ptr(), y.data_ptr(), 1, 1, 1, 4, 2, 2, 0, ops._DT[F32], ops._stream())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


@pytest.mark.parametrize("op", S.POOL_OPS)
def test_pool_and_upsample_grid_stride(op, device):
    """More items than 16384 workgroups x 256 threads: every thread of the scalar f32 build makes a second trip."""
    from nopesac_amd import ops
    dtype, C, H, W = S.POOL_GRID_CASE
    assert 4 * H * W * C > S.GRID_LIMIT and S.pool_form(dtype, C, True) == "f32x1"
    g = S.gen(1999)
    tag = "1x%dx%dx%d" % (2 * H, 2 * W, C)
    if op == "maxpool":
        x = S.randn(g, 1, 2 * H, 2 * W, C).float()
        _exact("maxpool f32x1 grid-stride", ops.maxpool(x.to(device), 3, 1, 1), S.maxpool_ref(x, 3, 1, 1).float(), tag)
        return
    x, addend = S.randn(g, 1, H, W, C).float(), S.randn(g, 1, 2 * H, 2 * W, C).float()
    if op == "nearest_add":
        _exact("nearest_add f32x1 grid-stride", ops.upsample2x_nearest_add(x.to(device), addend.to(device)), S.up2(x) + addend, tag)
        return
    ref, Sm, _ = S.bilinear_ref(x, addend, S.ACT_NONE)
    q = S.quotient(ops.upsample2x_bilinear(x.to(device), addend.to(device), S.ACT_NONE), ref, Sm) / (S.FLOOR_FACTOR * S.floor_bilinear())
    _note("bilinear f32x1 grid-stride", q, tag)
    assert q <= 1.0, q


# ---------------------------------------------------------------------------------------------------------------------------- 2. GroupNorm
@pytest.mark.parametrize("case", S.gn_cases(), ids=S.gn_case_id)
def test_groupnorm_paths_against_f64(case, device):
    from nopesac_amd import ops
    C, G, HW, B, aligned = case
    form = S.groupnorm_form(C, G, aligned)
    assert form != S.REFUSED
    for dtype in (F32, BF16):
        for ratio in S.GN_RATIOS:
            x, gamma, beta = S.gn_inputs(C, G, HW, B, dtype, ratio)
            xd = _put(x.view(B, HW, 1, C), device, not aligned)
            bound = S.FLOOR_FACTOR * S.floors_groupnorm()[S.gn_floor_key(form, ratio)]
            for act in (S.ACT_NONE, S.ACT_RELU):
                ref, Sm, z = S.groupnorm_ref(x, gamma, beta, G, act)
                assert float(z.abs().min()) > S.MARGIN
                got = ops.groupnorm(xd, gamma.to(device), beta.to(device), G, S.GN_EPS, act).view(B, HW, C)
                q = S.quotient(got, ref, Sm) / bound if dtype == F32 else S.quotient_bf16(got, ref, Sm, bound)
                tag = "%s %s ratio %g act%d" % (S.gn_case_id(case), S.DT_NAME[dtype], ratio, act)
                _note("groupnorm %s %s ratio %g" % (form.split("(")[0], S.DT_NAME[dtype], ratio), q, tag)
                assert q <= 1.0, (tag, form, q)


@pytest.mark.parametrize("C,G", S.GN_REFUSED_CG)
def test_groupnorm_refuses_and_writes_nothing(C, G, device):
    from nopesac_amd import _lib, ops
    assert S.groupnorm_form(C, G) == S.REFUSED
    x = torch.randn(2, 5, C, device=device)
    y = torch.full_like(x, 7.0)
    gamma, beta, ws = torch.ones(C, device=device), torch.zeros(C, device=device), torch.empty(2 * 16 * G * 2, device=device)
    with pytest.raises(_lib.HipKernelError, match="groupnorm"):
        ops._C.nopesac_groupnorm_nhwc(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), 2, 5, C, G, S.GN_EPS, S.ACT_NONE,
                                      ops._DT[F32], ws.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------- 3. LayerNorm
@pytest.mark.parametrize("rows", S.LN_ROWS)
@pytest.mark.parametrize("D", S.LN_D)
def test_layernorm_outputs_against_f64(D, rows, device):
    from nopesac_amd import ops
    c = S.ln_inputs(D, rows)
    dv = {k: v.to(device) for k, v in c.items()}
    bound = S.FLOOR_FACTOR * S.floor_layernorm()
    for res in (None, "res"):
        for ar in S.LN_ADDEND_ROWS:
            add = None if ar is None else c[ar]
            y, Sy, y2, S2 = S.layernorm_ref(c["x"], None if res is None else c["res"], c["gamma"], c["beta"], add)
            refs = {"y": (y, Sy), "y16": (y, Sy), "y2": (y2, S2), "y2_16": (y2, S2)}
            args = (dv["x"], dv["gamma"], dv["beta"], None if res is None else dv["res"], None if ar is None else dv[ar], S.LN_EPS)
            tag = "D%d rows%d res=%s addend=%s" % (D, rows, res, ar)
            plain = ops.layernorm(*args)
            outs = [("layernorm", {"y": plain} if ar is None else {"y": plain[0], "y2": plain[1]})]
            outs += [("layernorm_ex " + "+".join(w), ops.layernorm_ex(*args, want=w)) for w in (S.LN_WANTS_PLAIN if ar is None else S.LN_WANTS_ADDEND)]
            for name, out in outs:
                assert name == "layernorm" or set(out) == set(name.split(" ")[1].split("+")), (name, sorted(out))
                for k, got in out.items():
                    ref, Sm = refs[k]
                    assert got.dtype == (BF16 if k.endswith("16") else F32) and got.shape == ref.shape
                    q = S.quotient_bf16(got, ref, Sm, bound) if k.endswith("16") else S.quotient(got, ref, Sm) / bound
                    _note("layernorm " + k, q, tag + " " + name)
                    assert q <= 1.0, (tag, name, k, q)
                for k16, k32 in (("y16", "y"), ("y2_16", "y2")):       # the bf16 copy is the f32 result rounded, bit for bit
                    if k16 in out and k32 in out:
                        _exact("layernorm %s = bf16(%s)" % (k16, k32), out[k16], out[k32].to(BF16), tag)


def test_layernorm_refusals(device):
    from nopesac_amd import _lib, ops
    for D in S.LN_REFUSED_D:
        x, w = torch.randn(3, D, device=device), torch.ones(D, device=device)
        with pytest.raises(_lib.HipKernelError, match="layernorm"):
            ops.layernorm(x, w, w)
        with pytest.raises(_lib.HipKernelError, match="layernorm_ex"):
            ops.layernorm_ex(x, w, w, want=("y16",))
    x, w = torch.randn(3, 64, device=device), torch.ones(64, device=device)
    for want in (("y2",), ("y", "y2_16")):
        with pytest.raises((ops.OpsArgumentError, _lib.HipKernelError)):
            ops.layernorm_ex(x, w, w, want=want)
    y2 = torch.full_like(x, 7.0)
    with pytest.raises(_lib.HipKernelError, match="y2 needs addend"):      # the entry point's own check, behind the wrapper's
        ops._C.nopesac_layernorm_ex(x.data_ptr(), None, w.data_ptr(), w.data_ptr(), None, None, 0, y2.data_ptr(), None, None, 3, 64, S.LN_EPS, ops._stream())
    torch.cuda.synchronize()
    assert bool((y2 == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------- 4. row softmax
@pytest.mark.parametrize("case", S.SM_CASES, ids=S.sm_case_id)
def test_softmax_rows_forms_against_f64(case, device):
    from nopesac_amd import ops
    D, ld, dt = case
    form = S.softmax_form(D, ld, dt)
    bound = S.FLOOR_FACTOR * S.floor_softmax()
    for rows in S.SM_ROWS:
        x = S.sm_inputs(D, rows)
        p, Sm = S.softmax_ref(x)
        got = ops.softmax_rows(x.to(device), out_dtype=dt, pad_to=ld if (ld > D or dt == BF16) else 0).cpu()
        tag = "%s rows%d" % (S.sm_case_id(case), rows)
        assert got.shape == (rows, ld) and got.dtype == dt, tag
        assert float(got[:, D:].abs().sum()) == 0 and not bool(torch.signbit(got[:, D:].float()).any()), tag       # padding: +0 exactly
        assert bool((got[:, :D][torch.isinf(x)] == 0).all()), tag                                                  # exp(-inf) = 0 exactly
        q = S.quotient(got[:, :D], p, Sm) / bound if dt == F32 else S.quotient_bf16(got[:, :D], p, Sm, bound)
        _note("softmax_rows " + form, q, tag)
        assert q <= 1.0, (tag, q)
        if dt == F32:
            e = float((got[:, :D].double().sum(-1) - 1).abs().max())
            _note("softmax_rows %s row sum" % form, e / bound, tag)
            assert e <= bound, (tag, e)


# ---------------------------------------------------------------------------------------------------------------------------- 5. re-layout / exact
def test_add_rows_concat_and_hw_transpose_exact(device):
    from nopesac_amd import ops
    g = S.gen(5100)
    for rows, D, br in S.ADD_ROWS_CASES:
        a, b = S.randn(g, rows, D).float(), S.randn(g, br, D).float()
        _exact("add_rows", ops.add_rows(a.to(device), b.to(device)), a + b[torch.arange(rows) % br], "%dx%d b_rows %d" % (rows, D, br))
    for rows, Da, Db in S.CONCAT_CASES:
        a, b = S.randn(g, rows, Da).float(), S.randn(g, rows, Db).float()
        _exact("concat_cols", ops.concat_cols(a.to(device), b.to(device)), torch.cat([a, b], 1), "%d x (%d | %d)" % (rows, Da, Db))
    for B, H, W, C in S.HW_ROWS_CASES:
        x = S.randn(g, B, H * W, C).float()
        _exact("transpose_hw_rows", ops.transpose_hw_rows(x.to(device), H, W), S.transpose_hw_rows_ref(x, H, W).contiguous(), "%dx%dx%dx%d" % (B, H, W, C))


@pytest.mark.parametrize("rows,cols", S.TRANSPOSE_SHAPES)
def test_transposes_exact(rows, cols, device):
    from nopesac_amd import ops, training
    for B in S.TRANSPOSE_B:
        x = S.matrix_input(rows, cols, B)
        _exact("transpose_batched", ops.transpose_batched(x.to(device)), x.transpose(1, 2).contiguous(), "B%d %dx%d" % (B, rows, cols))
    for ld in (cols, cols + 5):                                    # dense, and a column slice of a wider buffer (x_ld > cols)
        xd = S.matrix_input(rows, ld)[0].to(device)
        sl = xd[:, ld - cols:]
        assert sl.stride(0) == ld
        _exact("training.transpose", training.transpose(sl), sl.cpu().t().contiguous(), "%dx%d ld %d" % (rows, cols, ld))


@pytest.mark.parametrize("n", S.U8_N)
def test_u8_to_f32_exact(n, device):
    from nopesac_amd import ops
    x = torch.randint(0, 256, (n,), generator=S.gen(5200 + n), dtype=torch.uint8)
    x[0], x[-1] = 255, (0 if n > 1 else 255)
    _exact("u8_to_f32", ops.u8_to_f32(x.to(device)), x.float(), "n%d" % n)


def test_add_rows_bf16_exact_and_refuses_misaligned(device):
    from nopesac_amd import _lib, ops
    g = S.gen(5300)
    for rows, D, br in S.ADD_ROWS_BF16_CASES:
        assert rows % br
        a, b = S.randn(g, rows, D).float(), S.randn(g, br, D).float()
        a16, ab16 = ops.add_rows_bf16(a.to(device), b.to(device))
        tag = "%dx%d b_rows %d" % (rows, D, br)
        _exact("add_rows_bf16 a", a16, a.to(BF16), tag)
        _exact("add_rows_bf16 a+b", ab16, (a + b[torch.arange(rows) % br]).to(BF16), tag)
        for who in ("a", "b"):                                     # an argument check, nothing is launched
            with pytest.raises(_lib.HipKernelError, match="alignment"):
                ops.add_rows_bf16(_put(a, device, who == "a"), _put(b, device, who == "b"))


@pytest.mark.parametrize("n", S.NONFINITE_N)
def test_count_nonfinite_exact(n, device):
    from nopesac_amd import ops
    x, bad = S.nonfinite_input(n)
    assert bad >= 1
    xd = x.to(device)
    counter = torch.zeros(1, device=device, dtype=torch.int32)
    for call in (1, 2):                                             # the counter is cumulative
        ops._C.nopesac_count_nonfinite(xd.data_ptr(), n, counter.data_ptr(), ops._stream())
        assert int(counter) == call * bad, (n, call, int(counter), bad)
    clean = torch.where(torch.isfinite(x), x, torch.zeros_like(x)).to(device)
    ops._C.nopesac_count_nonfinite(clean.data_ptr(), n, counter.data_ptr(), ops._stream())
    assert int(counter) == 2 * bad
    _note("count_nonfinite", 0.0, "n%d" % n)


def test_count_nonfinite_batch_exact(device):
    from nopesac_amd import ops
    pairs = [S.nonfinite_input(n, seed) for seed, n in enumerate(S.NONFINITE_N + (257, 2))]
    assert max(S.NONFINITE_N) > S.NONFINITE_BATCH_LIMIT
    total = sum(b for _, b in pairs)
    counter = ops.count_nonfinite([x.to(device) for x, _ in pairs])
    assert int(counter) == total
    ops.count_nonfinite([x.to(device) for x, _ in pairs[:2]], counter)
    assert int(counter) == total + pairs[0][1] + pairs[1][1]
    _note("count_nonfinite batch", 0.0, "%d tensors" % len(pairs))


@pytest.mark.parametrize("canon", [False, True], ids=["plain", "canonical"])
@pytest.mark.parametrize("D", S.NORMALIZE_D)
def test_normalize_rows_and_backward(D, canon, device):
    """The forward is compared bit for bit with the kernel's operation order restated with every step correctly rounded to f32
    (stream_forms.normalize_rows_f32: the kernel's sqrt and divide are the correctly rounded ones); the backward is held to 8 x its
    f32 floor."""
    from nopesac_amd import ops
    x, g = S.normalize_inputs(D)
    xz = torch.cat([x, torch.zeros(1, D)])                          # an all-zero row: 0 / 1e-12 = 0
    tag = "D%d canon %d" % (D, canon)
    got, want = ops.normalize_rows(xz.to(device), canon).cpu(), S.normalize_rows_f32(xz, canon)
    diff = got.view(torch.int32) - want.view(torch.int32)
    print("normalize_rows %s: %d of %d elements differ from the f32 restatement, by at most %d ulp; rows %s" %
          (tag, int((diff != 0).sum()), diff.numel(), int(diff.abs().max()), (diff != 0).any(1).nonzero().flatten().tolist()[:8]))
    _exact("normalize_rows", got, want, tag)
    xd, gd, out = x.to(device), g.to(device), torch.empty_like(x, device=device)
    ops._C.nopesac_normalize_rows_backward(xd.data_ptr(), gd.data_ptr(), x.shape[0], D, int(canon), out.data_ptr(), ops._stream())
    ref, Sm = S.normalize_rows_bwd_ref(x, g, canon)
    q = S.quotient(out, ref, Sm) / (S.FLOOR_FACTOR * S.floor_normalize_bwd())
    _note("normalize_rows backward", q, tag)
    assert q <= 1.0, (tag, q)


# ---------------------------------------------------------------------------------------------------------------------------- 6. reductions / optimiser
def _trainer(p):
    from nopesac_amd.training import RefineTrainer
    return RefineTrainer({"w": p}, nq=1)


@pytest.mark.parametrize("n", S.CLIP_N)
def test_clip_grad_norm_against_f64(n, device):
    from nopesac_amd import ops
    g = S.grad_input(n)
    form = S.sumsq_form(n)
    fam = "sumsq " + (form if isinstance(form, str) else form[0])
    bound = S.FLOOR_FACTOR * S.floor_sumsq()
    gd = g.to(device)
    accs = []
    ws = torch.empty(256, device=device)
    for _ in range(2):
        acc = torch.zeros(1, device=device)
        ops._C.nopesac_sumsq_accumulate_f32(gd.data_ptr(), n, acc.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        accs.append(acc.cpu())
    assert _same_bits(accs[0], accs[1]), "sum of squares differs run to run"
    ss, norm, _, _ = S.clip_ref(g, 1.0)
    q = float((accs[0].double()[0] - ss).abs() / ss) / bound
    _note(fam, q, "n%d %s" % (n, form))
    assert q <= 1.0, (n, q)
    qn = float((accs[0].double()[0].sqrt() - norm).abs() / norm) / bound
    assert qn <= 1.0, (n, qn)
    for max_norm, clips in ((0.25 * float(norm), True), (4.0 * float(norm), False)):
        _, _, coef, scaled = S.clip_ref(g, max_norm)
        tr = _trainer(torch.zeros(n, device=device))
        tr.params["w"].grad = gd.clone()
        c = tr.clip_grad_norm(max_norm).cpu()
        got = tr.params["w"].grad
        tag = "n%d %s" % (n, "clipping" if clips else "not clipping")
        assert (float(c) < 1.0) == clips, tag
        qc = float((c.double()[0] - coef).abs() / coef) / bound
        _note("clip coefficient", qc, tag)
        assert qc <= 1.0, (tag, qc)
        _exact("scale_by", got, g * c, tag)                          # one correctly rounded multiply by the coefficient
        if not clips:
            assert float(c) == 1.0 and _same_bits(got, g), tag
        qs = S.quotient(got, scaled, scaled.abs()) / (S.FLOOR_FACTOR * S.floor_clipped_gradient())
        _note("clipped gradient", qs, tag)
        assert qs <= 1.0, (tag, qs)


@pytest.mark.parametrize("config", S.STEP_CONFIGS, ids=lambda c: "%s_wd%g_mom%g" % c)
@pytest.mark.parametrize("n", S.STEP_N)
def test_optimiser_steps_against_f64(n, config, device):
    name, wd, mom = config
    p0 = S.grad_input(n)
    grads = [S.grad_input(n, k + 1) for k in range(S.STEPS)]
    tr = _trainer(p0.to(device))
    for g in grads:
        tr.params["w"].grad = g.to(device)
        tr.step(lr=S.STEP_LR[name], optimizer=name, weight_decay=wd, betas=S.ADAM_BETAS, eps=S.ADAM_EPS, momentum=mom)
    ref, Sm = S.optimiser_steps(p0, grads, name, wd, mom)
    q = S.quotient(tr.params["w"].detach(), ref, Sm) / (S.FLOOR_FACTOR * S.floor_optimiser(name))
    _note("optimiser " + name, q, "n%d wd %g momentum %g" % (n, wd, mom))
    assert q <= 1.0, (n, config, q)


@pytest.mark.parametrize("rows,cols,ld", S.col_sum_cases())
def test_col_sum_against_f64(rows, cols, ld, device):
    from nopesac_amd import training
    x = S.matrix_input(rows, ld)[0]
    sl = x.to(device)[:, ld - cols:]
    xs = x[:, ld - cols:].double()
    q = S.quotient(training.col_sum(sl), xs.sum(0), xs.abs().sum(0)) / (S.FLOOR_FACTOR * S.floor_col_sum())
    _note("col_sum", q, "%dx%d ld %d" % (rows, cols, ld))
    assert q <= 1.0, q


# ---------------------------------------------------------------------------------------------------------------------------- 4b. correlation softmax
@pytest.mark.parametrize("h,w", S.CORR_HW)
def test_corr_softmax_forward_and_backward_against_f64(h, w, device):
    """Forward: channel order (w, h) of the view-2 positions, zero padding.  Backward: from the float64 probabilities rounded to f32 in a
    padded buffer, noise in the padded gradient columns (no gradient flows from them)."""
    from nopesac_amd import ops
    c = S.corr_inputs(h, w)
    P, ld = h * w, S.corr_pad(h * w)
    ff, fb = S.floors_corr()
    x1, x2 = c["x1"].to(device), c["x2"].to(device)
    p, Sp = S.corr_ref(c["x1"], c["x2"])
    for pad_to in (0, ld):
        got = ops.corr_softmax(x1, x2, pad_to).cpu()
        tag = "%dx%d pad_to %d" % (h, w, pad_to)
        assert got.shape == (S.CORR_B, h, w, max(P, pad_to)), tag
        assert float(got[..., P:].abs().sum()) == 0, tag
        q = S.quotient(got[..., :P], p, Sp) / (S.FLOOR_FACTOR * ff)
        _note("corr_softmax forward", q, tag)
        assert q <= 1.0, (tag, q)
    a = torch.cat([p.float(), torch.zeros(S.CORR_B, h, w, ld - P)], -1)
    da = torch.cat([c["da"], c["noise"]], -1)
    dx1, dx2 = ops.corr_softmax_backward(a.to(device), da.to(device), x1, x2)
    r1, r2, S1, S2 = S.corr_bwd_ref(p.float(), c["da"], c["x1"], c["x2"])
    for name, got, ref, Sm in (("dx1", dx1, r1, S1), ("dx2", dx2, r2, S2)):
        q = S.quotient(got, ref, Sm) / (S.FLOOR_FACTOR * fb)
        _note("corr_softmax backward " + name, q, "%dx%d ld %d" % (h, w, ld))
        assert q <= 1.0, (h, w, name, q)


# ---------------------------------------------------------------------------------------------------------------------------- 7. norm / pool backward
@pytest.mark.parametrize("C", S.BN_C)
@pytest.mark.parametrize("rows", S.BN_ROWS)
def test_bn_act_forward_and_backward_against_f64(rows, C, device):
    from nopesac_amd import ops
    ins = S.bn_inputs(rows, C)
    c, dy, gamma, beta, mean, var = (t.to(device) for t in ins)
    floors = S.floors_bn()
    for act in S.BN_ACTS:
        r = S.bn_ref(*ins, act)
        assert float(r["z"].abs().min()) > S.MARGIN
        dc, dg, db = ops.bn_act_backward(dy, c, gamma, beta, mean, var, S.BN_EPS, act)
        got = {"y": ops.bn_act_forward(c, gamma, beta, mean, var, S.BN_EPS, act), "dc": dc, "dgamma": dg, "dbeta": db}
        for k in S.BN_KEYS:
            q = S.quotient(got[k], r[k], r["S" + k]) / (S.FLOOR_FACTOR * floors[k])
            _note("bn_act " + k, q, "rows%d C%d act%d grid %s" % (rows, C, act, S.bn_grid(rows, C)))
            assert q <= 1.0, (rows, C, act, k, q)


@pytest.mark.parametrize("case", S.gnb_cases(), ids=lambda c: "C%d_G%d_HW%d_B%d" % c)
def test_groupnorm_backward_against_f64(case, device):
    from nopesac_amd import ops
    C, G, HW, B = case
    x, dy, gamma, beta = S.gnb_inputs(*case)
    floors = S.floors_gnb()
    d = lambda t: t.view(B, HW, 1, C).to(device)
    for relu in (False, True):
        r = S.gnb_ref(x, dy, gamma, beta, G, relu)
        dx, dg, db = ops.groupnorm_backward(d(x), d(dy), gamma.to(device), beta.to(device), G, S.GN_EPS, S.ACT_RELU if relu else S.ACT_NONE)
        for k, got in (("dx", dx.view(B, HW, C)), ("dgamma", dg), ("dbeta", db)):
            q = S.quotient(got, r[k], r["S" + k]) / (S.FLOOR_FACTOR * floors[k])
            _note("groupnorm_backward %s cpg %d" % (k, C // G), q, "C%d G%d HW%d B%d relu %d" % (C, G, HW, B, relu))
            assert q <= 1.0, (case, relu, k, q)


@pytest.mark.parametrize("ties", [False, True], ids=["unique", "ties"])
@pytest.mark.parametrize("H,W", S.MPB_HW)
def test_maxpool_backward_exact(H, W, ties, device):
    from nopesac_amd import ops
    x, dy = S.mpb_inputs(H, W, ties)
    dx = ops.maxpool_backward(x.to(device), dy.to(device))
    _exact("maxpool_backward", dx, S.mpb_ref(x, dy), "%dx%d ties %d" % (H, W, ties))
    assert float(dx[:, H // 2 * 2:].abs().sum() + dx[:, :, W // 2 * 2:].abs().sum()) == 0         # an odd size: zero last row / column


@pytest.mark.parametrize("shape", S.UPB_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_nearest_add_backward_exact(shape, device):
    from nopesac_amd import ops
    B, H, W, C = shape
    dy = S.randn(S.gen(7800 + H + W), B, 2 * H, 2 * W, C).float()
    dyd = dy.to(device)
    dx, dl = ops.upsample2x_nearest_add_backward(dyd)
    _exact("upsample2x_nearest_add_backward", dx, S.upb_f32(dy), "x".join(map(str, shape)))
    assert dl is dyd or _same_bits(dl, dy)


# ---------------------------------------------------------------------------------------------------------------------------- 8. conv gradients
@pytest.mark.parametrize("case", S.dgrad_cases(), ids=lambda c: "k%d_p%d_%dx%d_cin%d_cout%d" % (c[0], c[1], c[2][0], c[2][1], c[3], c[4]))
def test_dgrad_stride2_gather_against_f64(case, device):
    """dy read from a channel slice of a wider buffer, dx written into a channel slice of a sentinel-filled one."""
    from nopesac_amd import ops
    k, pad, hw, cin, cout = case
    x, w, dyw = S.dgrad_inputs(*case)
    ref, Sm, _, _ = S.conv_grad_ref(x, w, dyw[..., :cout], 2, pad)
    out = torch.full((S.DGRAD_B, hw[0], hw[1], cin + S.DGRAD_DX_EXTRA), 7.0, device=device)
    ops.conv2d_dgrad(dyw.to(device)[..., :cout], w.to(device), hw, stride=2, pad=pad, out=out[..., :cin])
    assert bool((out[..., cin:] == 7.0).all())
    q = S.quotient(out[..., :cin], ref, Sm) / (S.FLOOR_FACTOR * S.floors_conv_grad()[0])
    _note("conv2d_dgrad stride 2", q, "k%d %dx%d cin%d cout%d" % (k, hw[0], hw[1], cin, cout))
    assert q <= 1.0, (case, q)


@pytest.mark.parametrize("case", S.wgrad_cases(), ids=S.wgrad_case_id)
def test_wgrad_tails_against_f64(case, device):
    from nopesac_amd import ops
    ch, (k, stride), P = case
    cin, cx, cout = ch
    x, dy, pad = S.wgrad_inputs(*case)
    _, _, ref, Sm = S.conv_grad_ref(x[..., :cin], torch.zeros(cout, cin, k, k), dy, stride, pad)
    xd, dyd = x.to(device), dy.to(device)
    for splits in S.wgrad_splits(P):
        got = ops.conv2d_wgrad(xd, dyd, k, stride=stride, pad=pad, cin=cin, splits=splits)
        q = S.quotient(got, ref, Sm) / (S.FLOOR_FACTOR * S.floors_conv_grad()[1])
        _note("conv2d_wgrad", q, "%s splits %d %s" % (S.wgrad_case_id(case), splits, S.wgrad_grid(cin, cout, k, P, splits)["grid"]))
        assert q <= 1.0, (case, splits, q)


def test_zz_worst_ratio_per_family_and_form(capsys):
    with capsys.disabled():
        print("\nstream sweep: worst |kernel - f64| / bound per family and form")
        for fam in sorted(WORST):
            q, case = WORST[fam]
            print("  %-44s %.3f  %s" % (fam, q, case))
    assert WORST and all(q <= 1.0 for q, _ in WORST.values())
