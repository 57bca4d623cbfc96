"""GPU half of the stage sweep (tests/stage_forms.py): every build of the matcher tail, of post-selection and the wavefront kernels of the
one-plane RANSAC at every plane count the benchmark legs run, each against a float64 reference of the same operation - discrete outputs
exact outside the decision margins the CPU half bounds, continuous ones within the f32 floor derived there."""
import pytest
import torch

from tests import stage_forms as S
from tests.util import rel_err

pytestmark = pytest.mark.gpu
WORST = {}           # family / build -> (worst error / bound, case)
NEG_PAD = torch.tensor(-1e30, dtype=torch.float32)


def _note(fam, q, case):
    if q > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (q, case)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _rel(got, ref):
    """rel_err where the reference is a number; NaN exactly where the reference is NaN."""
    got, ref = got.double().cpu().reshape(-1), ref.double().reshape(-1)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), "NaN pattern differs"
    return rel_err(got[~nan], ref[~nan]) if (~nan).any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------- Sinkhorn
@pytest.mark.parametrize("nq,build", S.SINK_GPU_CASES, ids=["nq%d_%s" % c for c in S.SINK_GPU_CASES])
def test_sinkhorn_builds_against_f64(nq, build, device, monkeypatch):
    """One launch of <= 12 ragged pairs per iteration count (200, and 0 and 1: setup and finalise without the averaging of 200 rounds).
    n1 = n2 = 0 gives log(0) marginals; the reference model never reaches it (its post-selection keeps at least one plane per view,
    by the arg-max and max-overlap fallbacks, and matching_head.py has no branch for it), so only an all-zero assignment is asserted."""
    from nopesac_amd import ops
    for k in S.SINK_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in S.sinkhorn_switches(nq, build).items():
        monkeypatch.setenv(k, v)
    c = S.sinkhorn_inputs(nq)
    dev = [c[k].to(device) for k in ("dot", "p1", "p2", "cam7", "n1", "n2")]
    bin_score = torch.tensor([S.BIN_SCORE], device=device)
    bound = S.sinkhorn_bound(nq)
    for iters in S.SINK_ITERS:
        args = (*dev, bin_score, S.OFFSET_MULT, S.NORMAL_MULT, iters, S.MATCH_THR)
        ls_d, A_d = ops.matcher_sinkhorn(*args)
        ls2, A2 = ops.matcher_sinkhorn(*args)
        torch.cuda.synchronize()
        ls, A = ls_d.cpu(), A_d.cpu()
        for b, r in enumerate(S.matcher_references(nq, iters)):
            n1, n2 = r["n1"], r["n2"]
            tag = "nq%d it%d pair %d (%d x %d)" % (nq, iters, b, n1, n2)
            assert float(A[b, n1:].abs().sum() + A[b, :, n2:].abs().sum()) == 0, tag
            if r["ls"] is None:
                assert float(A[b].abs().sum()) == 0, tag
                continue
            assert torch.equal(_bits(ls_d[b]), _bits(ls2[b])) and torch.equal(A_d[b], A2[b]), ("repeat", tag)
            pad = r["ls"] == -1e30
            assert bool((ls[b][pad] == NEG_PAD).all()) and not bool((ls[b][~pad] == NEG_PAD).any()), tag
            rows, cols = torch.tensor(list(range(n1)) + [nq]), torch.tensor(list(range(n2)) + [nq])
            sel = (rows[:, None], cols[None])
            err = S.block_rel_err(ls[b][sel], r["block"], r["pair_out"][sel])
            print("%s %s: rel_err %.3g (bound %.3g)" % (build, tag, err, bound))
            _note("sinkhorn " + build, err / bound, tag)
            assert err <= bound, (tag, err, bound)
            assert torch.equal(A[b][r["a_keep"]].double(), r["A"][r["a_keep"]]), tag
            assert bool(((A[b] == 0) | (A[b] == 1)).all()), tag


# ---------------------------------------------------------------------------------------------------------------------------- post-selection
@pytest.mark.parametrize("planar", [False, True], ids=["hwq", "qhw"])
@pytest.mark.parametrize("case", S.PS_GPU_CASES, ids=S.ps_case_id)
def test_postselect_builds_against_f64(case, planar, device, monkeypatch):
    from nopesac_amd import _lib, ops
    nq, geom, pair = case
    h, w, H, W, th = S.PS_GEOMETRIES[geom]
    monkeypatch.delenv("NOPESAC_PS_TH", raising=False)
    if th is not None:
        monkeypatch.setenv("NOPESAC_PS_TH", str(th))
    form = S.postselect_form(nq, h, w, H, W, th)
    ins, refs = S.postselect_case(case)
    prob = torch.stack([i[2] for i in ins])                                  # [2,nq,h,w]
    prob = prob.contiguous() if planar else prob.permute(0, 2, 3, 1).contiguous()
    st = lambda k: torch.stack([i[k] for i in ins]).to(device)
    args = (st(0), prob.to(device), st(1), st(3), H, W, S.SCORE_THR, S.MASK_THR, S.OVERLAP_THR)
    if form == S.REFUSED:                                                    # a host-side argument check: nothing is launched
        with pytest.raises(_lib.HipKernelError, match="too small for the LDS tile"):
            ops.postselect_planes(*args, planar=planar)
        return
    out = ops.postselect_planes(*args, planar=planar)
    out2 = ops.postselect_planes(*args, planar=planar)
    torch.cuda.synchronize()
    fam = "postselect <%d,%s>" % (form[1], "X4" if form[2] else "generic")
    for b, r in enumerate(refs):
        tag = "%s image %d" % (S.ps_case_id(case), b)
        o = {k: v[b].cpu() for k, v in out.items()}
        for k in out:
            assert torch.equal(out[k][b], out2[k][b]), ("repeat", k, tag)
        n = r["n_kept"]
        assert int(o["n_kept"]) == n and int(o["flags"]) == r["flags"], tag
        assert torch.equal(o["kept_idx"].long(), r["kept_idx"]), tag
        assert torch.equal(o["planes"], r["planes"]) and torch.equal(o["feats"], r["feats"]), tag
        e_s = float((o["scores"].double() - r["scores"]).abs().max())
        assert e_s <= 1e-6, (tag, e_s)
        inside = r["margin"] < S.PS_MARGIN
        n_out = int(inside.sum())
        assert torch.equal(o["winner"][~inside], r["winner"][~inside]), (tag, int((o["winner"] != r["winner"]).sum()))
        e_a = int((o["areas"].long() - r["areas"]).abs().max())
        assert e_a <= n_out, (tag, e_a, n_out)
        e_c = rel_err(o["centers"], r["centers"])
        assert e_c <= 2e-4, (tag, e_c)
        _note(fam + " scores", e_s / 1e-6, tag)
        _note(fam + " centres", e_c / 2e-4, tag)
        _note(fam + " winner+areas", float(int((o["winner"] != r["winner"]).sum()) > n_out or e_a > n_out), tag)


# ---------------------------------------------------------------------------------------------------------------------------- RANSAC
def _dev(c, device, *keys):
    return [c[k].to(device) for k in keys]


@pytest.mark.parametrize("warp_in_ref", [True, False], ids=["ref", "local"])
@pytest.mark.parametrize("nq", S.NQS)
def test_geo_sequence_against_f64(nq, warp_in_ref, device):
    from nopesac_amd import ops
    c = S.ransac_inputs(nq)
    out = ops.geo_sequence(*_dev(c, device, "A", "p1", "p2", "n1", "n2", "init_trans", "init_rot"), warp_in_ref=warp_in_ref)
    torch.cuda.synchronize()
    gl, gg, sig, enc, m = (t.cpu() for t in out)
    for b, mm in enumerate(c["ms"]):
        r = S.geo_sequence_reference(c, b, warp_in_ref)
        tag = "nq%d m%d" % (nq, mm)
        assert int(m[b]) == r["m"] == mm, tag
        for k, got in (("geo_local", gl), ("geo_global", gg), ("geo_enc", enc)):
            e = rel_err(got[b], r[k])
            _note("geo_sequence", e / 1e-6, tag + " " + k)
            assert e <= 1e-6, (tag, k, e)
            assert float(got[b, mm:].abs().sum()) == 0, (tag, k)
        assert torch.equal(sig[b].double(), r["sig"]), tag


@pytest.mark.parametrize("nq", S.NQS)
def test_ransac_score_maps_against_f64(nq, device):
    from nopesac_amd import ops
    c = S.ransac_inputs(nq)
    gl = torch.stack([S.geo_sequence_reference(c, b, True)["geo_local"].float() for b in range(len(c["ms"]))])
    m = torch.tensor(c["ms"], dtype=torch.int32)
    out = ops.ransac_score_maps(gl.to(device), *_dev(c, device, "rot_raw", "trans_raw", "init_rot", "init_trans"), m.to(device), diagnostics=True)
    torch.cuda.synchronize()
    for b, mm in enumerate(c["ms"]):
        r = S.score_maps_reference(gl[b], c["rot_raw"][b], c["trans_raw"][b], c["init_rot"][b], c["init_trans"][b], mm)
        for k in ("rots_all", "trans_all", "normal_score", "param_score", "l2_dist", "normal_angle", "offset_dist", "dn_sum", "dl2_sum"):
            got, ref = out[k][b].double().cpu(), r[k]
            tol = 1e-3 if k == "normal_angle" else 1e-4
            if k == "offset_dist":                       # the sign branch of the offset distance may go the other way next to n . n = 0
                got, ref = torch.where(r["offset_out"], ref, got), ref
            e = rel_err(got, ref)
            _note("ransac_score_maps", e / tol, "nq%d m%d %s" % (nq, mm, k))
            assert e <= tol, (nq, mm, k, e)
        assert float(out["normal_score"][b, mm + 1:].abs().sum() + out["normal_score"][b, :, mm:].abs().sum()) == 0
        assert float(out["dn_sum"][b, mm + 1:].abs().sum() + out["dl2_sum"][b, mm + 1:].abs().sum()) == 0


@pytest.mark.parametrize("train", [0, S.VOTE_TRAIN], ids=["infer", "train"])
@pytest.mark.parametrize("mode", S.VOTE_MODES)
@pytest.mark.parametrize("nq", S.NQS)
def test_ransac_soft_vote_against_f64(nq, mode, train, device):
    from nopesac_amd import ops
    c = S.ransac_inputs(nq)
    B = len(c["ms"])
    refs = [S.score_maps_reference(S.geo_sequence_reference(c, b, True)["geo_local"].float(), c["rot_raw"][b], c["trans_raw"][b],
                                   c["init_rot"][b], c["init_trans"][b], c["ms"][b]) for b in range(B)]
    maps32 = {k: torch.stack([r[k].float() for r in refs]) for k in ("rots_all", "trans_all", "dn_sum", "dl2_sum")}
    keys = ("sf_rot", "sf_trans", "reg_rot_w", "reg_rot_b", "reg_trans_w", "reg_trans_b", "init_rot_feat", "init_trans_feat", "fused_rot",
            "fused_trans", "rots_w", "rots_b", "trans_w", "trans_b")
    out = ops.ransac_soft_vote(*_dev(c, device, *keys), {k: v.to(device) for k, v in maps32.items()}, *_dev(c, device, "init_rot", "init_trans"),
                               torch.tensor(c["ms"], dtype=torch.int32, device=device), mode | train)
    torch.cuda.synchronize()
    for b, mm in enumerate(c["ms"]):
        r = S.soft_vote_reference(c, b, {k: v[b] for k, v in maps32.items()}, mode | train)
        tag = "nq%d m%d mode %d" % (nq, mm, mode | train)
        for k, tol in (("pred_rot", 1e-4), ("pred_trans", 1e-4), ("avg_rot", 1e-4), ("avg_trans", 1e-4), ("score_rot", 2e-4), ("score_trans", 2e-4)):
            e = _rel(out[k][b], r[k])
            _note("ransac_soft_vote " + ("train" if train else "mode %d" % mode), e / tol, tag + " " + k)
            assert e <= tol, (tag, k, e)
        assert float(out["score_rot"][b, mm + 1:].abs().sum() + out["score_trans"][b, mm + 1:].abs().sum()) == 0, tag


@pytest.mark.parametrize("nq", S.NQS)
def test_refilter_assignment_against_f64(nq, device):
    from nopesac_amd import ops
    c = S.ransac_inputs(nq)
    rot = c["init_rot"].clone()
    rot[1::2] = -rot[1::2]                                # every other quaternion with w < 0: canonicalised by the kernel
    out = ops.refilter_assignment(*_dev(c, device, "refilter_A", "p1", "p2", "n1", "n2"), rot.to(device), c["init_trans"].to(device)).cpu()
    wrong, kept, given = 0, 0.0, 0.0
    for b in range(len(c["ms"])):
        ref, keep = S.refilter_reference(c["refilter_A"][b], c["p1"][b], c["p2"][b], int(c["n1"][b]), int(c["n2"][b]), rot[b], c["init_trans"][b])
        wrong += int((out[b].double() != ref)[keep].sum())
        kept, given = kept + float(ref.sum()), given + float(c["refilter_A"][b, :int(c["n1"][b]), :int(c["n2"][b])].sum())
    assert 0 < kept < given
    _note("refilter_assignment", float(wrong), "nq%d: entries that differ" % nq)
    assert wrong == 0


def test_zz_worst_ratio_per_family_and_build(capsys):
    with capsys.disabled():
        print("\nstage sweep: worst |kernel - f64| / bound per family and build")
        for fam in sorted(WORST):
            q, case = WORST[fam]
            print("  %-36s %.3f  %s" % (fam, q, case))
    assert WORST and all(q <= 1.0 for q, _ in WORST.values())
