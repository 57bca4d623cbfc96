"""Host restatement (numpy, float64, plain loops and dicts) of the two-view reconstruction AP, written from its description - the
reference's offline eval.py --evaluate AP (evaluate_ap_by_idx, get_maskiou_merged / get_single2merge, evaluate_by_idx /
inst_bench_image / inst_bench / VOCap) and get_plane_params_in_global.  The CPU tests hold it against what the reference functions
themselves produced on the fixture seeds (tests/golden/K_recon_eval_*.npz); the GPU tests compare the kernel against it at shapes the
fixture does not cover.  Nothing here is shared with nopesac_amd.evaluation, and the routes differ from the kernel's on purpose: a
rotation MATRIX from the quaternion, np.linalg.eigh for the merged normal, a taken-list walk."""
import math

import numpy as np

COLS = ("score", "tp_all", "tp_no_offset", "tp_no_normal", "tp_no_mask", "tp_no_normal_offset", "index0", "index1")
CRITERIA = ("all", "-offset", "-normal", "-mask", "-normal-offset")
MASK_T = (0.5, 0.5, 0.5, 0.0, 0.5)
NORMAL_T = (30.0, 30.0, 1000.0, 30.0, 1000.0)
OFFSET_T = (1.0, 1000.0, 1.0, 1.0, 1000.0)


def rotation_matrix(q):
    """q = [w, x, y, z] -> the matrix of v -> q v q^-1 (a non-unit q is divided by |q|^2)."""
    w, x, y, z = (float(c) for c in q)
    n = w * w + x * x + y * y + z * z
    return np.array([[1 - 2 * (y * y + z * z) / n, 2 * (x * y - z * w) / n, 2 * (x * z + y * w) / n],
                     [2 * (x * y + z * w) / n, 1 - 2 * (x * x + z * z) / n, 2 * (y * z - x * w) / n],
                     [2 * (x * z - y * w) / n, 2 * (y * z + x * w) / n, 1 - 2 * (x * x + y * y) / n]], np.float64)


IDENTITY = {"position": [0.0, 0.0, 0.0], "rotation": [1.0, 0.0, 0.0, 0.0]}


def global_planes(planes, camera):
    """(offset [n], normal [n, 3]) of a view's planes (f32 [n, 3], normal * offset) in the common frame: flip y and z, rotate, shift,
    then the foot point of the origin on the plane through `end` with normal end - start."""
    p = np.asarray(planes, np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(camera["position"], np.float64).reshape(3)
    R = rotation_matrix(np.asarray(camera["rotation"], np.float64).reshape(4))
    off, nrm = np.zeros(len(p)), np.zeros((len(p), 3))
    for k in range(len(p)):
        end = R @ (p[k] * np.array([1.0, -1.0, -1.0])) + t
        b = end - t
        g = (end @ b) / (math.sqrt(b @ b) ** 2) * b
        off[k] = max(math.sqrt(g @ g), 1e-5)
        nrm[k] = g / off[k]
    return off, nrm


def entries(n0, n1, corrs):
    """[(index in view 0 or -1, index in view 1 or -1)]: view 0's planes outside every correspondence in index order, view 1's, then
    the correspondences in the order given."""
    corrs = [(int(a), int(b)) for a, b in corrs]
    used = ({a for a, _ in corrs}, {b for _, b in corrs})
    out = [(k, -1) for k in range(n0) if k not in used[0]] + [(-1, k) for k in range(n1) if k not in used[1]]
    return out + corrs


def merged_iou(pe, ge, iou0, iou1):
    out = np.zeros((len(pe), len(ge)), np.float64)
    ious = (iou0, iou1)
    for r, p in enumerate(pe):
        for c, g in enumerate(ge):
            p_merged, g_merged = p[0] >= 0 and p[1] >= 0, g[0] >= 0 and g[1] >= 0
            if p_merged and g_merged:
                out[r, c] = (iou0[p[0], g[0]] + iou1[p[1], g[1]]) / 2
            elif p_merged:
                v = 0 if g[0] >= 0 else 1
                out[r, c] = ious[v][p[v], g[v]]
            elif g_merged:
                v = 0 if p[0] >= 0 else 1
                out[r, c] = ious[v][p[v], g[v]]
            else:
                vp, vg = (0 if p[0] >= 0 else 1), (0 if g[0] >= 0 else 1)
                if vp == vg:
                    out[r, c] = ious[vp][p[vp], g[vp]]
    return out


def pair_errors(iou0, iou1, score0, score1, plane0, plane1, gt_plane0, gt_plane1, pred_cam, gt_cam, pred_corrs, gt_corrs):
    """One pair -> {"pred_entries", "gt_entries", "scores" [np], "err_offsets", "err_normals", "mask_iou" [np, ng]}."""
    score = (np.asarray(score0, np.float32).astype(np.float64), np.asarray(score1, np.float32).astype(np.float64))
    po, pn = zip(global_planes(plane0, pred_cam), global_planes(plane1, IDENTITY))
    go, gn = zip(global_planes(gt_plane0, gt_cam), global_planes(gt_plane1, IDENTITY))
    pe, ge = entries(len(score[0]), len(score[1]), pred_corrs), entries(len(go[0]), len(go[1]), gt_corrs)
    m_off, m_nrm, m_sc = [], [], []
    for a, b in pe:
        if a >= 0 and b >= 0:
            pair = np.stack([pn[0][a], pn[1][b]])
            w, v = np.linalg.eigh(pair.T @ pair)
            m_nrm.append(v[:, int(np.argmax(w))])
            m_off.append((po[0][a] + po[1][b]) / 2)
            m_sc.append(max(score[0][a], score[1][b]))
        else:
            v, k = (0, a) if a >= 0 else (1, b)
            m_nrm.append(pn[v][k]); m_off.append(po[v][k]); m_sc.append(score[v][k])
    g_off, g_nrm = [], []
    for a, b in ge:
        v, k = (0, a) if a >= 0 else (1, b)                 # a merged GT entry is view 0's plane
        g_off.append(go[v][k]); g_nrm.append(gn[v][k])
    err_off, err_nrm = np.zeros((len(pe), len(ge))), np.zeros((len(pe), len(ge)))
    for r in range(len(pe)):
        for c in range(len(ge)):
            err_off[r, c] = abs(m_off[r] - g_off[c])
            err_nrm[r, c] = math.acos(min(abs(float(m_nrm[r] @ g_nrm[c])), 1.0)) / math.pi * 180
    iou0 = np.asarray(iou0, np.float64).reshape(len(score[0]), len(go[0]))
    iou1 = np.asarray(iou1, np.float64).reshape(len(score[1]), len(go[1]))
    return {"pred_entries": pe, "gt_entries": ge, "scores": np.asarray(m_sc, np.float64), "err_offsets": err_off, "err_normals": err_nrm,
            "mask_iou": merged_iou(pe, ge, iou0, iou1)}


def walk(flags):
    """inst_bench_image on a 0 / 1 overlap [np, ng]: entries in entry order; each looks at the FIRST flagged GT entry only."""
    taken, tp = [], np.zeros(flags.shape[0], np.float64)
    for r in range(flags.shape[0]):
        first = next((c for c in range(flags.shape[1]) if flags[r, c]), None)
        if first is not None and first not in taken:
            taken.append(first)
            tp[r] = 1.0
    return tp


def pair_rows(*args):
    """pair_errors' arguments -> (rows [entries, 8] (COLS), number of GT entries, the errors dict)."""
    e = pair_errors(*args)
    rows = np.zeros((len(e["pred_entries"]), len(COLS)), np.float64)
    rows[:, 0] = e["scores"]
    for k in range(5):
        rows[:, 1 + k] = walk((e["mask_iou"] >= MASK_T[k]) & (e["err_normals"] <= NORMAL_T[k]) & (e["err_offsets"] <= OFFSET_T[k]))
    rows[:, 6:8] = np.asarray(e["pred_entries"], np.float64).reshape(-1, 2)
    return rows, len(e["gt_entries"]), e


def voc_ap(scores, tp, npos):
    """inst_bench + VOCap with their loops; ties keep the order of the rows.  No rows or npos = 0: 0."""
    if len(scores) == 0 or npos == 0:
        return 0.0
    order = sorted(range(len(scores)), key=lambda i: (-scores[i], i))
    ctp = cfp = 0.0
    rec, prec = [], []
    for i in order:
        ctp += tp[i]
        cfp += 1.0 - tp[i]
        rec.append(ctp / npos)
        prec.append(ctp / (cfp + ctp))
    mrec, mpre = [0.0] + rec + [1.0], [0.0] + prec + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    return sum((mrec[i] - mrec[i - 1]) * mpre[i] for i in range(1, len(mrec)) if mrec[i] != mrec[i - 1])


def table(rows, npos):
    rows = np.asarray(rows, np.float64).reshape(-1, len(COLS))
    out = {name: 100.0 * voc_ap(rows[:, 0], rows[:, 1 + k], npos) for k, name in enumerate(CRITERIA)}
    out["npos"] = float(npos)
    return out
