"""The Levenberg-Marquardt fit of MANO to 21 3-D joints of DESIGN.md section 7 ("MANO fitting"), restated in fp64 numpy, one hand at
a time.  It shares no code with the package; tests/test_fitting.py pins it against central differences and against
oracle.hands_oracle.mano_lbs, and tests/test_gpu_fitting.py holds csrc/fit.hip and hands_amd/fitting.py to it.

The unknowns are 16 rotations of the FULL pose (pose_mean added), beta (10) and a translation (3): 61 numbers, ordered
[delta_0 .. delta_15 | beta | t].  ``noise`` multiplies every residual and Jacobian entry by 1 + noise * N(0, 1): a twin run
with noise = 1e-15 shows what rounding-level differences do to a result.
"""
import math

import numpy as np

from smooth_ref import exp_so3, hat, log_so3  # noqa: F401  (the Log / Exp of DESIGN.md section 7, shared by both restatements)

PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
TIP_IDS = (744, 320, 443, 554, 671)
NU = 61                       # unknowns
MU_MIN, MU_MAX = 1e-9, 1e6


def config(iters=30, lambda_beta=1e-6, lambda_pose=1e-6, mu0=1e-3):
    return {"iters": int(iters), "lambda_beta": float(lambda_beta), "lambda_pose": float(lambda_pose), "mu0": float(mu0)}


def at_or_below(j, i):
    """joint i is joint j or one of its descendants"""
    while i >= 0:
        if i == j:
            return True
        i = PARENTS[i]
    return False


class Consts:
    """What the fit reads of a MANO asset, fp64: pose_mean (48), J_template (16,3), J_shapedirs (48,10) and the tip pack --
    v_template (5,3), shapedirs (5,3,10), lbs_weights (5,16) rows and posedirs columns (135,15) of the five tip vertices."""

    def __init__(self, pose_mean, J_template, J_shapedirs, tip_v, tip_sd, tip_w, tip_pd):
        f = lambda a, *s: np.asarray(a, np.float64).reshape(s)
        self.pose_mean, self.J_template, self.J_shapedirs = f(pose_mean, 48), f(J_template, 16, 3), f(J_shapedirs, 16, 3, 10)
        self.tip_v, self.tip_sd, self.tip_w, self.tip_pd = f(tip_v, 5, 3), f(tip_sd, 5, 3, 10), f(tip_w, 5, 16), f(tip_pd, 135, 5, 3)
        self.M = np.stack([exp_so3(self.pose_mean[3 * j:3 * j + 3]) for j in range(16)])       # M_0 = I


def consts_from_asset(asset, rounded=True):
    """From a ManoAsset.  ``rounded``: J_template and J_shapedirs rounded to fp32 as the packed constants of the device are;
    False keeps them in fp64, which is what the oracle's LBS computes with."""
    Jr = asset.J_regressor.astype(np.float64)
    Jt = Jr @ asset.v_template.astype(np.float64)
    Js = np.einsum("jv,vcl->jcl", Jr, asset.shapedirs.astype(np.float64))
    if rounded:
        Jt, Js = Jt.astype(np.float32), Js.astype(np.float32)
    tips = list(TIP_IDS)
    pd = asset.posedirs.reshape(135, 778, 3)[:, tips]
    return Consts(np.concatenate([np.zeros(3), asset.hands_mean]), Jt, Js, asset.v_template[tips], asset.shapedirs[tips],
                  asset.lbs_weights[tips], pd)


def rest_pose(C):
    return C.M.copy()


def evaluate(C, R, beta):
    """Forward kinematics and the five tips of the published LBS at rotations R (16,3,3) of the full pose and beta (10):
    J rest joints, Q world rotations, p posed joints, x[m, i] tip m as carried by joint i, A[m] = sum_i W_mi Q_i,
    joints (21,3) without the translation."""
    J = C.J_template + C.J_shapedirs @ beta
    Q, p = np.empty((16, 3, 3)), np.empty((16, 3))
    for i in range(16):
        if i == 0:
            Q[0], p[0] = R[0], J[0]
        else:
            a = PARENTS[i]
            Q[i], p[i] = Q[a] @ R[i], p[a] + Q[a] @ (J[i] - J[a])
    pf = (R[1:] - np.eye(3)).reshape(135)
    vp = C.tip_v + C.tip_sd @ beta + np.einsum("f,fmc->mc", pf, C.tip_pd)
    x = np.stack([np.stack([Q[i] @ (vp[m] - J[i]) + p[i] for i in range(16)]) for m in range(5)])
    A = np.einsum("mi,iab->mab", C.tip_w, Q)
    tips = np.einsum("mi,mic->mc", C.tip_w, x)
    return {"J": J, "Q": Q, "p": p, "vp": vp, "x": x, "A": A, "joints": np.concatenate([p, tips])}


def joints_of(C, R, beta):
    return evaluate(C, R, beta)["joints"]


def _noisy(a, noise, rng):
    return a if not noise else a * (1.0 + noise * rng.standard_normal(a.shape))


def residual(C, R, beta, t, y, w, cfg, noise=0.0, rng=None, E=None):
    """r (118): 63 data rows (rows of joints with w = 0 are 0 and their y is never read), 10 shape rows, 45 pose rows."""
    E = E or evaluate(C, R, beta)
    r = np.zeros(118)
    for k in range(21):
        if w[k] > 0:
            r[3 * k:3 * k + 3] = math.sqrt(w[k]) * (E["joints"][k] + t - y[k])
    r[63:73] = math.sqrt(cfg["lambda_beta"]) * beta
    for j in range(1, 16):
        r[73 + 3 * (j - 1):76 + 3 * (j - 1)] = math.sqrt(cfg["lambda_pose"]) * log_so3(C.M[j].T @ R[j])
    return _noisy(r, noise, rng)


def cross(v):
    return hat(v)


def jacobian(C, R, beta, w, cfg, noise=0.0, rng=None, E=None):
    """(118, 61), analytic, for the right perturbation R_j <- R_j Exp(delta_j)."""
    E = E or evaluate(C, R, beta)
    Q, p, x, A = E["Q"], E["p"], E["x"], E["A"]
    D = np.zeros((21, 3, NU))
    for j in range(16):
        for k in range(16):                                   # kinematic joints: strict descendants of j
            if k != j and at_or_below(j, k):
                D[k, :, 3 * j:3 * j + 3] = -cross(p[k] - p[j]) @ Q[j]
        for m in range(5):
            s = np.zeros(3)
            for i in range(16):
                if at_or_below(j, i):
                    s += C.tip_w[m, i] * (x[m, i] - p[j])
            blk = -cross(s) @ Q[j]
            if j >= 1:                                        # the pose blend shapes: d vec(R_j) = vec(R_j [e_a]x)
                for a in range(3):
                    dR = R[j] @ cross(np.eye(3)[a])
                    blk[:, a] += A[m] @ np.einsum("f,fc->c", dR.reshape(9), C.tip_pd[9 * (j - 1):9 * j, m])
            D[16 + m, :, 3 * j:3 * j + 3] = blk
    dp = np.empty((16, 3, 10))                                # d p_i / d beta along the chain
    for i in range(16):
        a = PARENTS[i]
        dp[i] = C.J_shapedirs[0] if i == 0 else dp[a] + Q[a] @ (C.J_shapedirs[i] - C.J_shapedirs[a])
    D[:16, :, 48:58] = dp
    for m in range(5):
        D[16 + m, :, 48:58] = sum(C.tip_w[m, i] * (Q[i] @ (C.tip_sd[m] - C.J_shapedirs[i]) + dp[i]) for i in range(16))
    D[:, :, 58:61] = np.eye(3)
    Jm = np.zeros((118, NU))
    for k in range(21):
        if w[k] > 0:
            Jm[3 * k:3 * k + 3] = math.sqrt(w[k]) * D[k]
    Jm[63:73, 48:58] = math.sqrt(cfg["lambda_beta"]) * np.eye(10)
    Jm[73:118, 3:48] = math.sqrt(cfg["lambda_pose"]) * np.eye(45)           # Gauss-Newton: d Log / d delta = I
    return _noisy(Jm, noise, rng)


def cholesky(A):
    """Lower factor, right-looking, or None at the first pivot that is not positive."""
    A = A.copy()
    n = A.shape[0]
    for k in range(n):
        if not A[k, k] > 0.0:
            return None
        d = math.sqrt(A[k, k])
        A[k, k] = d
        A[k + 1:, k] /= d
        for j in range(k + 1, n):
            A[j:, j] -= A[j:, k] * A[j, k]
    return np.tril(A)


def solve_chol(L, b):
    n = len(b)
    y = b.copy()
    for k in range(n):
        y[k] /= L[k, k]
        y[k + 1:] -= L[k + 1:, k] * y[k]
    for k in range(n - 1, -1, -1):
        y[k] /= L[k, k]
        y[:k] -= L[k, :k] * y[k]
    return y


def kabsch(X, Y, w):
    """Weighted rigid alignment Y ~ R X + t over the joints with w > 0: no scale, det R = +1.  SVD here; the device takes the
    rank-safe completion of csrc/procrustes_device.h, the same rotation wherever the cross-covariance has rank >= 2."""
    sel = [k for k in range(21) if w[k] > 0]
    ws = np.array([w[k] for k in sel])
    Xs, Ys = X[sel], Y[sel]
    mx, my = (ws[:, None] * Xs).sum(0) / ws.sum(), (ws[:, None] * Ys).sum(0) / ws.sum()
    K = np.einsum("k,ka,kb->ab", ws, Xs - mx, Ys - my)
    U, _, Vt = np.linalg.svd(K)
    V = Vt.T
    R = V @ np.diag([1.0, 1.0, np.linalg.det(V @ U.T)]) @ U.T
    return R, my - R @ mx


def rmse_of(C, R, beta, t, y, w):
    E = evaluate(C, R, beta)
    num = sum(w[k] * float(np.sum((E["joints"][k] + t - y[k]) ** 2)) for k in range(21) if w[k] > 0)
    return math.sqrt(num / sum(w[k] for k in range(21) if w[k] > 0))


def unfitted(C):
    return {"pose": rest_pose(C).astype(np.float32), "beta": np.zeros(10, np.float32), "transl": np.zeros(3, np.float32),
            "rmse": np.float32(np.nan), "steps": 0, "trace": [],
            "raw": {"pose": rest_pose(C), "beta": np.zeros(10), "transl": np.zeros(3), "rmse": float("nan")}}


def fit(C, y, w=None, valid=None, init=None, cfg=None, noise=0.0, seed=0):
    """One hand: y (21,3) fp32 metres, w (21) fp32 or None, valid a number or None, init (pose (16,3,3), beta (10), transl (3))
    fp32 or None.  -> pose, beta, transl, rmse (fp32, each rounded once), steps, and ``trace``: one (c, c', cholesky ok,
    accepted) per iteration."""
    cfg = cfg or config()
    rng = np.random.default_rng(seed)
    y32 = np.asarray(y, np.float32).reshape(21, 3)
    w = np.ones(21) if w is None else np.asarray(w, np.float32).astype(np.float64)
    sel = w > 0
    if (valid is not None and valid == 0) or sel.sum() < 4 or not np.isfinite(y32[sel]).all() or not np.isfinite(w[sel]).all():
        return unfitted(C)                                                     # a selected weight of +inf too
    y = np.where(sel[:, None], y32.astype(np.float64), 0.0)                    # unweighted joints are never read
    w = np.where(sel, w, 0.0)                                                  # nor is a weight that is negative or no number
    if init is not None:
        R, beta, t = (np.asarray(a, np.float32).astype(np.float64) for a in init)
        if not (np.isfinite(R).all() and np.isfinite(beta).all() and np.isfinite(t).all()):
            return unfitted(C)
        R = R.reshape(16, 3, 3).copy()
    else:
        R, beta = rest_pose(C), np.zeros(10)
        X = joints_of(C, R, beta)
        R0, tk = kabsch(X, y, w)
        R[0], t = R0, tk + R0 @ X[0] - X[0]                # MANO turns about the wrist joint: R0 (x - J_0) + J_0 + t = R0 x + tk
    mu, steps, trace = cfg["mu0"], 0, []
    r = residual(C, R, beta, t, y, w, cfg, noise, rng)
    c = float(r @ r)
    for _ in range(cfg["iters"]):
        E = evaluate(C, R, beta)
        Jm = jacobian(C, R, beta, w, cfg, noise, rng, E)
        H, g = Jm.T @ Jm, Jm.T @ r
        L = cholesky(H + mu * np.diag(np.diag(H)))
        ok, c2 = L is not None, float("nan")
        if ok:
            d = solve_chol(L, -g)
            R2 = np.stack([R[j] @ exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            beta2, t2 = beta + d[48:58], t + d[58:61]
            r2 = residual(C, R2, beta2, t2, y, w, cfg, noise, rng)
            c2 = float(r2 @ r2)
        accept = ok and c2 < c
        trace.append((c, c2, ok, accept))
        if accept:
            R, beta, t, r, c, steps, mu = R2, beta2, t2, r2, c2, steps + 1, max(mu / 3.0, MU_MIN)
        else:
            mu = min(5.0 * mu, MU_MAX)
    rm = rmse_of(C, R, beta, t, y, w)
    return {"pose": R.astype(np.float32), "beta": beta.astype(np.float32), "transl": t.astype(np.float32),
            "rmse": np.float32(rm), "steps": steps, "trace": trace, "raw": {"pose": R, "beta": beta, "transl": t, "rmse": rm}}


def pose_aa(C, R):
    """(48): [Log R_0, Log R_j - hands_mean_j], the axis-angle form process_data and the reference's targets use."""
    return np.concatenate([log_so3(np.asarray(R[j], np.float64)) for j in range(16)]) - C.pose_mean


# ---- inputs for the tests ----------------------------------------------------------------------------------------------------
def family_case(C, seed):
    """A case of the family of DESIGN.md section 7: the global rotation 2 randn(3) in axis-angle, fingers hands_mean + 0.5 randn,
    beta = randn, a translation; the target is the model's joints rounded to fp32.  Every fourth seed has five joints of weight 0."""
    rng = np.random.RandomState(seed)
    aa = np.concatenate([2.0 * rng.randn(3), C.pose_mean[3:] + 0.5 * rng.randn(45)])
    R = np.stack([exp_so3(aa[3 * j:3 * j + 3]) for j in range(16)])
    beta, t = rng.randn(10), np.array([0.05, -0.03, 0.6]) + 0.1 * rng.randn(3)
    y = (joints_of(C, R, beta) + t).astype(np.float32)
    w = np.ones(21, np.float32)
    if seed % 4 == 3:
        w[rng.choice(21, 5, replace=False)] = 0.0
    return y, w, (R, beta, t)


def step_parity_inputs(C, base, with_init):
    """Five hands for the step-parity test: y (5,21,3), w (5,21) -- ones, uneven weights, five joints of weight 0 whose
    coordinates are NaN -- and, ``with_init``, a caller's initial state (pose, beta, transl) near the truth, else None."""
    rng = np.random.RandomState(1000 + base)
    ys, ws, init = [], [], ([], [], [])
    for b in range(5):
        y, w, (R, beta, t) = family_case(C, base + b)
        if b in (1, 4):
            w = rng.uniform(0.25, 4.0, 21).astype(np.float32)
        if b == 2:
            w = np.ones(21, np.float32)
            w[rng.choice(21, 5, replace=False)] = 0.0
        y = y.copy()
        y[w == 0] = np.nan
        ys.append(y)
        ws.append(w)
        init[0].append(np.stack([R[j] @ exp_so3(0.2 * rng.randn(3)) for j in range(16)]))
        init[1].append(beta + 0.3 * rng.randn(10))
        init[2].append(t + 0.02 * rng.randn(3))
    init = tuple(np.stack(a).astype(np.float32) for a in init) if with_init else None
    return np.stack(ys), np.stack(ws), init


def fit_rows(C, y, w=None, valid=None, init=None, cfg=None, noise=0.0, seed=0):
    """``fit`` over the rows of a batch -> a list of its results."""
    return [fit(C, y[b], None if w is None else w[b], None if valid is None else valid[b],
                None if init is None else tuple(a[b] for a in init), cfg, noise, seed + b) for b in range(len(y))]


# the 16 cases of the full-run tests: seeds of family_case at which every accept / reject decision of the 30 iterations has a
# margin |c' - c| > 1e-9 c on the synthetic right asset (3, 7, 11, 15 have five joints of weight 0)
FULL_SEEDS = (0, 1, 3, 4, 5, 6, 7, 8, 9, 11, 13, 14, 15, 16, 17, 18)
_FULL = {}


def full_run_reference(C, key="r"):
    """y (16,21,3), w (16,21), the restatement's 30-iteration results and those of its noise = 1e-15 twin; computed once."""
    if key not in _FULL:
        ys, ws = zip(*[family_case(C, s)[:2] for s in FULL_SEEDS])
        y, w = np.stack(ys), np.stack(ws)
        _FULL[key] = (y, w, fit_rows(C, y, w), fit_rows(C, y, w, noise=1e-15, seed=77))
    return _FULL[key]
