"""float64 numpy restatement of the temporal metrics (csrc/accel.hip, hands_amd/temporal.py): what the kernels are held to.

For x (T,N,D) holding consecutive frames, a[t] = (x[t-1] - 2 x[t] + x[t+1]) fps^2 and the error of row t is
mean_n |a_pred[t,n,:] - a_gt[t,n,:]|_2, defined for 1 <= t <= T-2.  Row t is NaN -- and its window is not looked at -- at the two
ends, where one of its three frames is not valid, and where the three frames do not carry one sequence id.  Inputs are taken as
the fp32 values they are given as and everything from the first subtraction on is fp64; non-finite coordinates in a valid
window go through the arithmetic as IEEE has it."""
import numpy as np

ACCEL_KEYS = ("acc", "acc/j", "acc/abs")


def _f64(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def window_ok(T, valid=None, seq_id=None):
    """(T) bool: row t has a window, all of it valid and of one sequence."""
    ok = np.zeros(T, bool)
    for t in range(1, T - 1):
        ok[t] = True
        if valid is not None:
            ok[t] = all(np.asarray(valid)[t + k] != 0 for k in (-1, 0, 1))
        if ok[t] and seq_id is not None:
            s = np.asarray(seq_id)
            ok[t] = s[t - 1] == s[t] == s[t + 1]
    return ok


def accel_error(gt, pred, valid=None, seq_id=None, fps=30.0):
    """hands_amd.accel_error: fp32 inputs -> (T) float64"""
    return accel_error_f64(_f64(gt), _f64(pred), valid, seq_id, fps)


def accel_error_f64(gt, pred, valid=None, seq_id=None, fps=30.0):
    """The same on float64 arrays taken as they are (the root-relative differences of evaluate_accel are not rounded to fp32)."""
    assert gt.dtype == pred.dtype == np.float64 and gt.shape == pred.shape and gt.ndim == 3
    T = gt.shape[0]
    fps2 = float(np.float32(fps)) ** 2
    out = np.full(T, np.nan)
    ok = window_ok(T, valid, seq_id)
    with np.errstate(all="ignore"):
        for t in np.nonzero(ok)[0]:
            ag = (gt[t - 1] - 2.0 * gt[t] + gt[t + 1]) * fps2
            ap = (pred[t - 1] - 2.0 * pred[t] + pred[t + 1]) * fps2
            d = ap - ag
            out[t] = np.sqrt((d * d).sum(-1)).mean()
    return out


def nanmean2(r, l):
    """nanmean of two rows, NaN where both are."""
    nr, nl = np.isnan(r), np.isnan(l)
    with np.errstate(all="ignore"):
        return (np.where(nr, 0.0, r) + np.where(nl, 0.0, l)) / ((~nr).astype(np.float64) + (~nl).astype(np.float64))


def hand_valid(targets, hand):
    """{right,left}_valid * is_valid != 0, the product in fp32 as the kernel forms it."""
    hv = np.asarray(targets["right_valid" if hand == "r" else "left_valid"], dtype=np.float32)
    return (hv * np.asarray(targets["is_valid"], dtype=np.float32)) != 0


def evaluate_accel(pred, targets, meta_info=None, fps=30.0, seq_id=None):
    """The nine keys of hands_amd.evaluate_accel_metrics, (T) float64 each."""
    if seq_id is None and meta_info is not None and "seq_id" in meta_info:
        seq_id = meta_info["seq_id"]
    out = {}
    for h in "rl":
        pv, gv = _f64(pred[f"mano.v3d.cam.{h}"]), _f64(targets[f"mano.v3d.cam.{h}"])
        pj, gj = _f64(pred[f"mano.j3d.cam.{h}"]), _f64(targets[f"mano.j3d.cam.{h}"])
        valid = hand_valid(targets, h)
        with np.errstate(all="ignore"):
            out[f"acc/{h}"] = accel_error_f64(gv - gj[:, :1], pv - pj[:, :1], valid, seq_id, fps)
            out[f"acc/j/{h}"] = accel_error_f64(gj - gj[:, :1], pj - pj[:, :1], valid, seq_id, fps)
        out[f"acc/abs/{h}"] = accel_error_f64(gj, pj, valid, seq_id, fps)
    for k in ACCEL_KEYS:
        out[f"{k}/h"] = nanmean2(out[f"{k}/r"], out[f"{k}/l"])
    return out


def all_valid(targets):
    """``targets`` with every flag 1: what the reference's acc_r / acc_l are before their masking."""
    T = len(np.asarray(targets["is_valid"]))
    return dict(targets, **{k: np.ones(T, np.float32) for k in ("is_valid", "right_valid", "left_valid")})


def sequence(T, V, seed=0, noise=3e-3):
    """Seeded inputs of the fused evaluation as fp32 numpy arrays: two hands on smooth paths around z = 0.6 / 0.7 m, ``noise``
    metres of noise on the prediction, every flag 1.  -> (pred, targets)"""
    rng = np.random.RandomState(seed)
    t = np.arange(T)[:, None, None] / 30.0
    pred, targets = {}, {}
    for h, centre in (("r", (-0.1, 0.0, 0.6)), ("l", (0.1, 0.02, 0.7))):
        shape = 0.04 * rng.randn(1, V + 21, 3)
        path = np.concatenate([0.05 * np.sin(3.0 * t + rng.rand()), 0.03 * np.cos(2.0 * t), 0.04 * t * t], -1)
        gt = (shape * (1.0 + 0.2 * np.sin(2.0 * t)) + path + np.asarray(centre)).astype(np.float32)
        pr = (gt + noise * rng.randn(T, V + 21, 3)).astype(np.float32)
        targets[f"mano.v3d.cam.{h}"], targets[f"mano.j3d.cam.{h}"] = gt[:, :V].copy(), gt[:, V:].copy()
        pred[f"mano.v3d.cam.{h}"], pred[f"mano.j3d.cam.{h}"] = pr[:, :V].copy(), pr[:, V:].copy()
    for k in ("is_valid", "right_valid", "left_valid"):
        targets[k] = np.ones(T, np.float32)
    return pred, targets


def split(d, sizes):
    """The rows of every array of ``d`` cut into consecutive batches of ``sizes``."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [{k: v[a:b] for k, v in d.items()} for a, b in zip(edges[:-1], edges[1:])]


def stream(batches, fps=30.0):
    """The streaming rule, without any carried state: ``batches`` is a list of (pred, targets, seq_id) of consecutive frames;
    -> the nine keys over the concatenated stream, row i scoring the window that ENDS at frame i (rows 0 and 1 NaN)."""
    cat = lambda ds: {k: np.concatenate([np.asarray(d[k]) for d in ds]) for k in ds[0]}
    pred, targets = cat([b[0] for b in batches]), cat([b[1] for b in batches])
    ids = None if batches[0][2] is None else np.concatenate([np.asarray(b[2]) for b in batches])
    one = evaluate_accel(pred, targets, fps=fps, seq_id=ids)
    return {k: np.concatenate([[np.nan], v[:-1]]) for k, v in one.items()}
