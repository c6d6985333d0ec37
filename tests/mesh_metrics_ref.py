"""fp64 numpy restatement of the mesh metrics (hands_eval_mesh_metrics_f32) and of the egoexo branch of the reference's
``eval_mpjpe_pa_ra`` (hands_eval_metrics_masked_f32), written from their definitions in include/hands_hip.h.

The mesh part restates published definitions (the FreiHAND evaluation's F-score and PCK-AUC; the similarity transform of
``compute_similarity_transform``, src/utils/eval_modules.py:136-187) -- the reference computes none of them, so its parity is
unpinned.  The masked part is pinned to the reference by tests/golden/eval_metrics_egoexo.npz.
"""
import numpy as np

F_THRESHOLDS = (0.005, 0.015)
PCK_THRESHOLDS = np.arange(100, dtype=np.float64) * 0.05 / 99.0
MESH_QUANTITIES = ("mpvpe/{}", "fscore/{}/5", "fscore/{}/15", "auc/{}/v", "auc/{}/j")


def nanmean2(r, l):
    """torch_utils.nanmean over the two hands: NaN where both are."""
    s = np.stack([np.asarray(r, np.float64), np.asarray(l, np.float64)], axis=1)
    n = (~np.isnan(s)).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.isnan(s), 0.0, s).sum(1) / n


def similarity_transform(S1, S2):
    """S1 (N,3) moved onto S2 (N,3) by scale, rotation and translation; NaN when S1 is constant (scale = 0 / 0)."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    mu1, mu2 = S1.mean(0), S2.mean(0)
    X1, X2 = S1 - mu1, S2 - mu2
    var1 = (X1 ** 2).sum()
    K = X1.T @ X2
    U, _, Vh = np.linalg.svd(K)
    V = Vh.T
    Z = np.eye(3)
    Z[2, 2] = 1.0 if np.linalg.det(U @ V.T) >= 0 else -1.0
    R = V @ Z @ U.T
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.trace(R @ K) / var1
        return scale * (S1 @ R.T) + (mu2 - scale * (R @ mu1))


def similarity_transform_as_reference(S1, S2):
    """What the reference's compute_similarity_transform makes of an (n,3) array: the rows are the points -- unless n is 2 or
    3, where it takes the array as (dimension, points) as it stands: two joints become three points in the plane, three joints
    the three columns.  The result has the layout of the input, and the caller's error runs along its rows."""
    S1, S2 = np.asarray(S1, np.float64), np.asarray(S2, np.float64)
    if S1.shape[0] not in (2, 3):
        return similarity_transform(S1, S2)
    X1, X2 = S1.T, S2.T                                   # (points, dimension) with dimension 2 or 3
    d = X1.shape[1]
    mu1, mu2 = X1.mean(0), X2.mean(0)
    K = (X1 - mu1).T @ (X2 - mu2)
    U, _, Vh = np.linalg.svd(K)
    Z = np.eye(d)
    Z[-1, -1] = 1.0 if np.linalg.det(U @ Vh) >= 0 else -1.0
    R = Vh.T @ Z @ U.T
    with np.errstate(invalid="ignore", divide="ignore"):
        scale = np.trace(R @ K) / ((X1 - mu1) ** 2).sum()
        return (scale * (X1 @ R.T) + (mu2 - scale * (R @ mu1))).T


def pck_auc(err):
    """Area under the PCK curve of the errors (metres) at the 100 thresholds k * 0.05 / 99, trapezoid rule, over 0.05."""
    pck = (np.asarray(err, np.float64)[None, :] <= PCK_THRESHOLDS[:, None]).mean(1)
    return float(((pck[1:] + pck[:-1]) * 0.5 * np.diff(PCK_THRESHOLDS)).sum() / 0.05)


def nn_distances(gt, pr):
    """d1_i = min_j |gt_i - pr_j|, d2_j = min_i |pr_j - gt_i|."""
    D = np.sqrt(((gt[:, None, :] - pr[None, :, :]) ** 2).sum(-1))
    return D.min(1), D.min(0)


def fscore(d1, d2, th):
    P, R = float((d1 < th).mean()), float((d2 < th).mean())
    return 2.0 * P * R / (P + R) if P + R > 0 else 0.0


def hand_mesh_metrics(pv, gv, pj, gj):
    """One hand (fp32 arrays): the ten values in the order of hands_mesh_eval_out, plus the distances they were cut from
    (``dist``: alignment -> (vertex errors, d1, d2, joint errors)) for the tests' count of threshold-straddling points."""
    pv, gv, pj, gj = (np.asarray(a, np.float32) for a in (pv, gv, pj, gj))
    if not all(np.isfinite(a).all() for a in (pv, gv, pj, gj)):
        return [np.nan] * 10, {}
    pv, gv = (pv - pj[:1]).astype(np.float64), (gv - gj[:1]).astype(np.float64)      # root alignment in fp32
    pj, gj = (pj - pj[:1]).astype(np.float64), (gj - gj[:1]).astype(np.float64)
    out, dist = [], {}
    for a in ("ra", "pa"):
        qv, qj = (pv, pj) if a == "ra" else (similarity_transform(pv, gv), similarity_transform(pj, gj))
        if not np.isfinite(qv).all():                   # a constant prediction: no similarity transform
            vals = [np.nan] * 4
            ev = d1 = d2 = np.full(len(pv), np.nan)
        else:
            ev = np.sqrt(((gv - qv) ** 2).sum(-1))
            d1, d2 = nn_distances(gv, qv)
            vals = [ev.mean() * 1000.0] + [fscore(d1, d2, th) for th in F_THRESHOLDS] + [pck_auc(ev)]
        ej = np.sqrt(((gj - qj) ** 2).sum(-1))
        out += vals + [pck_auc(ej) if np.isfinite(qj).all() else np.nan]
        dist[a] = (ev, d1, d2, ej)
    return out, dist


def evaluate_mesh(pred, targets, return_dist=False):
    """Dict of (B) fp64 arrays with the keys of hands_amd.evaluate_mesh_metrics."""
    B = len(pred["mano.v3d.cam.r"])
    keys = [q.format(a) for a in ("ra", "pa") for q in MESH_QUANTITIES]
    vals = {s: np.full((B, 10), np.nan) for s in "rl"}
    dists = {s: [{} for _ in range(B)] for s in "rl"}
    for s, hv in (("r", "right_valid"), ("l", "left_valid")):
        valid = np.asarray(targets[hv], np.float32) * np.asarray(targets["is_valid"], np.float32)
        for b in range(B):
            if valid[b] != 0:
                vals[s][b], dists[s][b] = hand_mesh_metrics(pred[f"mano.v3d.cam.{s}"][b], targets[f"mano.v3d.cam.{s}"][b],
                                                            pred[f"mano.j3d.cam.{s}"][b], targets[f"mano.j3d.cam.{s}"][b])
    out = {}
    for i, k in enumerate(keys):
        out[k + "/r"], out[k + "/l"] = vals["r"][:, i], vals["l"][:, i]
        out[k + "/h"] = nanmean2(vals["r"][:, i], vals["l"][:, i])
    return (out, dists) if return_dist else out


def evaluate_masked(pred, targets):
    """The nine keys of eval_mpjpe_pa_ra's egoexo branch (src/utils/eval_modules.py:231-317), millimetres."""
    B = len(pred["mano.j3d.cam.r"])
    isv = np.asarray(targets["is_valid"], np.float32)
    res = {}
    for s, hv in (("r", "right_valid"), ("l", "left_valid")):
        valid = np.asarray(targets[hv], np.float32) * isv
        rao, ab, pa = (np.full(B, np.nan) for _ in range(3))
        for b in range(B):
            sel = np.asarray(targets[f"joints3d_valid_{s}"][b]) != 0
            if not sel.any():
                continue
            g = np.asarray(targets[f"mano.j3d.cam.{s}"][b], np.float32)[sel]
            p = np.asarray(pred[f"mano.j3d.cam.{s}"][b], np.float32)[sel]
            ab[b] = np.sqrt(((g - p).astype(np.float64) ** 2).sum(-1)).mean()
            g, p = (g - g[:1]).astype(np.float64), (p - p[:1]).astype(np.float64)    # first flagged joint, fp32
            rao[b] = np.sqrt(((g - p) ** 2).sum(-1)).mean()
            pa[b] = np.sqrt(((g - similarity_transform_as_reference(p, g)) ** 2).sum(-1)).mean() * valid[b]
        res[s] = {"mpjpe/pa/rao": rao, "mpjpe/pa/abs": ab, "mpjpe/pa/ra": pa}
    out = {}
    for k in ("mpjpe/pa/rao", "mpjpe/pa/abs", "mpjpe/pa/ra"):
        out[k + "/r"], out[k + "/l"] = res["r"][k] * 1000.0, res["l"][k] * 1000.0
        out[k + "/h"] = nanmean2(res["r"][k], res["l"][k]) * 1000.0
    return out
