"""The fit of MANO to surface correspondences, the correspondence step and the ICP loop of DESIGN.md section 7 ("MANO fitting to
surface correspondences and ICP registration"), restated in fp64 numpy, one hand at a time.  The fit stands on
tests/fit_verts_ref.py (``evaluate``, ``vertex_jacobian``, Log / Exp, Cholesky, Kabsch), the correspondences on
tests/surface_ref.py (``closest_on_mesh_1``, ``_segment``).  It shares no code with the package.
tests/test_fit_surf.py pins it against central differences and against fit_verts_ref; tests/test_gpu_fit_surf.py and
tests/test_gpu_register.py hold csrc/fit_surf.hip, csrc/mesh_correspond.hip and hands_amd/fitting.py to it.

Row k of a hand's P rows: a face f_k of ``faces`` (1538,3), coefficients b_k (3), a target y_k (3) and a weight w_k.
c_k = sum_i b_ki v_{faces[f_k][i]}; the residual is sqrt(w_k) A_k (c_k + t - y_k), A_k = n n^T + sqrt(tau) (I - n n^T) for a
non-zero normal n with tau != 1, else I.
"""
import math

import numpy as np

import fit_verts_ref as V
import surface_ref as SR
from fit_verts_ref import MU_MAX, MU_MIN, NU, NV, cholesky, exp_so3, log_so3, solve_chol  # noqa: F401

NF = 1538


def config(iters=30, lambda_beta=1e-6, lambda_pose=1e-6, mu0=1e-3, tangent_weight=1.0):
    return dict(V.config(iters, lambda_beta, lambda_pose, mu0), tangent_weight=float(tangent_weight))


def row_matrices(normals, tau, P):
    """A_k (P,3,3)."""
    A = np.broadcast_to(np.eye(3), (P, 3, 3)).copy()
    if normals is None or tau == 1.0:
        return A
    n = np.asarray(normals, np.float64)
    use = (n != 0).any(1)
    nn = n[:, :, None] * n[:, None, :]
    A[use] = nn[use] + math.sqrt(tau) * (np.eye(3) - nn[use])
    return A


def surface_points(v, tri, b):
    """c_k (P,3) from the vertices v (778,3), the rows' vertex triples tri (P,3) and coefficients b (P,3)."""
    return np.einsum("ki,kic->kc", b, v[tri])


def row_jacobian(C, R, E, tri, b):
    """d c_k / d [delta | beta | t] (P,3,61): the vertex Jacobian combined with b; the translation enters a row once."""
    D = V.vertex_jacobian(C, R, E)
    Jr = np.einsum("ki,kiau->kau", b, D[tri])
    Jr[:, :, 58:61] = np.eye(3)
    return Jr


def residual(C, R, beta, t, rows, cfg, E=None):
    """rows = (tri, b, y, w, A): r (3 P + 55): the data rows, 10 shape rows, 45 pose rows."""
    tri, b, y, w, A = rows
    E = E or V.evaluate(C, R, beta)
    e = surface_points(E["v"], tri, b) + t - y
    P = len(w)
    r = np.zeros(3 * P + 55)
    r[:3 * P] = (np.sqrt(w)[:, None] * np.einsum("kab,kb->ka", A, e)).reshape(-1)
    r[3 * P:3 * P + 10] = math.sqrt(cfg["lambda_beta"]) * beta
    for j in range(1, 16):
        r[3 * P + 10 + 3 * (j - 1):3 * P + 13 + 3 * (j - 1)] = math.sqrt(cfg["lambda_pose"]) * log_so3(C.M[j].T @ R[j])
    return r


def jacobian(C, R, beta, rows, cfg, E=None):
    tri, b, y, w, A = rows
    E = E or V.evaluate(C, R, beta)
    P = len(w)
    Jm = np.zeros((3 * P + 55, NU))
    Jm[:3 * P] = (np.sqrt(w)[:, None, None] * np.einsum("kab,kbu->kau", A, row_jacobian(C, R, E, tri, b))).reshape(3 * P, NU)
    Jm[3 * P:3 * P + 10, 48:58] = math.sqrt(cfg["lambda_beta"]) * np.eye(10)
    Jm[3 * P + 10:, 3:48] = math.sqrt(cfg["lambda_pose"]) * np.eye(45)
    return Jm


def rmse_of(E, t, rows):
    tri, b, y, w, _ = rows
    e = surface_points(E["v"], tri, b) + t - y
    return math.sqrt(float((w * (e ** 2).sum(1)).sum() / w.sum()))


def unfitted(C):
    u = V.unfitted(C)
    nanv = np.full((NV, 3), np.nan)
    u["verts"] = nanv.astype(np.float32)
    u["raw"]["verts"] = nanv
    return u


def fit(C, faces, y, face_idx, bary, w=None, normals=None, valid=None, init=None, cfg=None):
    """One hand: y (P,3) fp32, face_idx (P) integers, bary (P,3) fp32, w (P) fp32 or None, normals (P,3) fp32 or None.
    -> pose, beta, transl, rmse, j3d, verts (fp32, each rounded once), steps, ``trace`` and ``raw`` (fp64)."""
    cfg = cfg or config()
    tau = cfg["tangent_weight"]
    faces = np.asarray(faces, np.int64).reshape(NF, 3)
    y32, b32 = np.asarray(y, np.float32).reshape(-1, 3), np.asarray(bary, np.float32).reshape(-1, 3)
    P = len(y32)
    f = np.asarray(face_idx, np.int64).reshape(P)
    w = np.ones(P) if w is None else np.asarray(w, np.float32).astype(np.float64)
    sel = w > 0
    read_n = normals is not None and tau != 1.0
    n32 = np.asarray(normals, np.float32).reshape(P, 3) if read_n else None
    bad = (valid is not None and valid == 0) or sel.sum() < 4 or not np.isfinite(w[sel]).all()
    bad = bad or not (np.isfinite(y32[sel]).all() and np.isfinite(b32[sel]).all()) or ((f[sel] < 0) | (f[sel] >= NF)).any()
    bad = bad or (read_n and not np.isfinite(n32[sel]).all())
    if bad:
        return unfitted(C)
    # rows of weight 0 are never read: they leave
    tri, b, yy, ww = faces[f[sel]], b32[sel].astype(np.float64), y32[sel].astype(np.float64), w[sel]
    rows = (tri, b, yy, ww, row_matrices(n32[sel] if read_n else None, tau, int(sel.sum())))
    if init is not None:
        R, beta, t = (np.asarray(a, np.float32).astype(np.float64) for a in init)
        if not (np.isfinite(R).all() and np.isfinite(beta).all() and np.isfinite(t).all()):
            return unfitted(C)
        R = R.reshape(16, 3, 3).copy()
    else:
        R, beta = V.rest_pose(C), np.zeros(10)
        E = V.evaluate(C, R, beta)
        R0, tk = V.kabsch(surface_points(E["v"], tri, b), yy, ww)
        R[0], t = R0, tk + R0 @ E["J"][0] - E["J"][0]
    mu, steps, trace = cfg["mu0"], 0, []
    E = V.evaluate(C, R, beta)
    r = residual(C, R, beta, t, rows, cfg, E)
    c = float(r @ r)
    for _ in range(cfg["iters"]):
        Jm = jacobian(C, R, beta, rows, cfg, E)
        H, g = Jm.T @ Jm, Jm.T @ r
        L = cholesky(H + mu * np.diag(np.diag(H)))
        ok, c2 = L is not None, float("nan")
        if ok:
            d = solve_chol(L, -g)
            R2 = np.stack([R[j] @ exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            beta2, t2 = beta + d[48:58], t + d[58:61]
            E2 = V.evaluate(C, R2, beta2)
            r2 = residual(C, R2, beta2, t2, rows, cfg, E2)
            c2 = float(r2 @ r2)
        accept = ok and c2 < c
        trace.append((c, c2, ok, accept))
        if accept:
            R, beta, t, r, c, E, steps, mu = R2, beta2, t2, r2, c2, E2, steps + 1, max(mu / 3.0, MU_MIN)
        else:
            mu = min(5.0 * mu, MU_MAX)
    rm, j3d, verts = rmse_of(E, t, rows), E["joints"] + t, E["v"] + t
    return {"pose": R.astype(np.float32), "beta": beta.astype(np.float32), "transl": t.astype(np.float32), "rmse": np.float32(rm),
            "j3d": j3d.astype(np.float32), "verts": verts.astype(np.float32), "steps": steps, "trace": trace, "cost": c,
            "raw": {"pose": R, "beta": beta, "transl": t, "rmse": rm, "j3d": j3d, "verts": verts}}


def fit_rows(C, faces, y, face_idx, bary, w=None, normals=None, valid=None, init=None, cfg=None):
    g = lambda a, i: None if a is None else a[i]
    return [fit(C, faces, y[i], face_idx[i], bary[i], g(w, i), g(normals, i), g(valid, i),
                None if init is None else tuple(a[i] for a in init), cfg) for i in range(len(y))]


clear = V.clear


# ---- the correspondence step -------------------------------------------------------------------------------------------------
def _seg_t(p, a, b):
    ab = b - a
    L = SR._dot(ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(L > 0, SR._dot(p - a, ab) / L, 0.0)
    return np.clip(t, 0.0, 1.0)


def face_coefficients(p, a, b, c):
    """Per point p (P,3) and its triangle a, b, c (P,3 each): the coefficients (P,3) of the closest point, from the candidate
    surface_ref.point_triangle_pairs takes (ab, ac, bc, then the plane: the first of equal ones), and the unit normal (zero
    for a face without one)."""
    t1, t2, t3 = _seg_t(p, a, b), _seg_t(p, a, c), _seg_t(p, b, c)
    z = np.zeros_like(t1)
    cand = [np.stack([1 - t1, t1, z], -1), np.stack([1 - t2, z, t2], -1), np.stack([z, 1 - t3, t3], -1)]
    d2 = [SR._segment(p, a, b)[0], SR._segment(p, a, c)[0], SR._segment(p, b, c)[0]]
    n = SR._cross(b - a, c - a)
    nn = SR._dot(n, n)
    wa, wb, wc = SR._dot(n, SR._cross(b - p, c - p)), SR._dot(n, SR._cross(c - p, a - p)), SR._dot(n, SR._cross(a - p, b - p))
    inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(nn > 0, SR._dot(p - a, n) / nn, 0.0)
        v, w = np.where(nn > 0, wb / nn, 0.0), np.where(nn > 0, wc / nn, 0.0)
        unit = np.where((nn > 0)[:, None], n / np.sqrt(nn)[:, None], 0.0)
    pc = p - s[:, None] * n
    cand.append(np.stack([1 - v - w, v, w], -1))
    d2.append(np.where(inside, SR._dot(p - pc, p - pc), np.inf))
    pick = np.stack(d2).argmin(0)
    return np.take_along_axis(np.stack(cand), pick[None, :, None], 0)[0], unit


def correspond(points, verts, faces, w=None, max_dist=0.0):
    """One sample: dist (P), face_idx (P), closest (P,3), bary (P,3), normal (P,3), weights (P) -- fp64.  A query of weight 0 is
    not read: NaN / -1 / NaN / NaN / 0 / 0.  ``runner_up`` (P): the distance to the nearest OTHER face."""
    points = np.asarray(points, np.float64)
    P = len(points)
    w = np.ones(P) if w is None else np.asarray(w, np.float64)
    read = w > 0
    dist, idx, cl = np.full(P, np.nan), np.full(P, -1, np.int64), np.full((P, 3), np.nan)
    bary, normal = np.full((P, 3), np.nan), np.zeros((P, 3))
    q = np.where(read[:, None], points, 0.0)
    d, i, c = SR.closest_on_mesh_1(q[read], verts, faces) if read.any() else (dist[:0], idx[:0], cl[:0])
    dist[read], idx[read], cl[read] = d, i, c
    has = idx >= 0
    if has.any():
        T = np.asarray(verts, np.float64)[np.asarray(faces, np.int64).reshape(-1, 3)[idx[has]]]
        bary[has], normal[has] = face_coefficients(points[has], T[:, 0], T[:, 1], T[:, 2])
    with np.errstate(invalid="ignore"):
        gate = read & ((max_dist <= 0) | (dist <= max_dist))
    return {"dist": dist, "face_idx": idx, "closest": cl, "bary": bary, "normal": normal, "weights": np.where(gate, w, 0.0)}


def runner_up(points, verts, faces, face_idx):
    """Per point the fp64 distance to the nearest face other than face_idx[p] that is not the same triangle (a padded face list
    repeats faces)."""
    verts, F = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    out = np.empty(len(points))
    ok = SR.usable_faces(verts, F)
    T = verts[F[ok]]
    d2 = SR.point_triangle(points, T[:, 0], T[:, 1], T[:, 2], False)[0]
    ids = np.flatnonzero(ok)
    for k in range(len(points)):
        same = (F[ids] == F[face_idx[k]]).all(1)
        out[k] = np.sqrt(d2[k][~same].min())
    return out


def register(C, faces, points, init, w=None, valid=None, rounds=10, iters=3, lambda_beta=1e-6, lambda_pose=1e-6, mu0=1e-3,
             tangent_weight=0.1, max_dist=0.0):
    """The ICP loop for one hand, as hands_amd.register_mano runs it: every state is rounded to fp32 between the rounds, as the
    launches hand it on.  -> the last fitted round's result, ``dist`` (P) of the last correspondence, ``rounds_done`` and
    ``history``: per round the rms of the weighted distances of its correspondence."""
    points = np.asarray(points, np.float32)
    P = len(points)
    cfg = config(iters, lambda_beta, lambda_pose, mu0, tangent_weight)
    f0, b0 = np.zeros(P, np.int64), np.tile(np.array([1.0, 0.0, 0.0], np.float32), (P, 1))
    state = fit(C, faces, points, f0, b0, w, None, valid, init, dict(cfg, iters=0))
    done, history, dist = 0, [], np.full(P, np.nan)
    for r in range(rounds):
        cor = correspond(points, state["verts"], faces, w, max_dist)
        dist = cor["dist"]
        sel = cor["weights"] > 0
        history.append(float(np.sqrt((cor["weights"][sel] * dist[sel] ** 2).sum() / cor["weights"][sel].sum())) if sel.any() else float("nan"))
        new = fit(C, faces, points, cor["face_idx"], cor["bary"].astype(np.float32), cor["weights"].astype(np.float32),
                  cor["normal"].astype(np.float32), valid, (state["pose"], state["beta"], state["transl"]), cfg)
        if np.isfinite(new["rmse"]):
            state, done = new, r + 1
    out = dict(state)
    if done == 0:
        out["rmse"] = np.float32(np.nan)
    out.update(dist=dist, rounds_done=done, history=history)
    return out


def cloud_distance(points, verts, faces):
    """rms distance of the points to the surface."""
    return float(np.sqrt((SR.closest_on_mesh_1(points, verts, faces)[0] ** 2).mean()))


# ---- inputs for the tests ----------------------------------------------------------------------------------------------------
def surface_case(C, faces, seed, P, scale=0.5):
    """A state drawn as fit_verts_ref.family_case draws it (fingers hands_mean + ``scale`` randn) and P rows on its own posed
    surface: random faces, Dirichlet(1,1,1) coefficients (rounded to fp32), targets c_k + t rounded to fp32.
    -> y (P,3), face_idx (P) int32, bary (P,3), truth (R, beta, t)."""
    rng = np.random.RandomState(seed)
    aa = np.concatenate([2.0 * rng.randn(3), C.pose_mean[3:] + scale * rng.randn(45)])
    R = np.stack([exp_so3(aa[3 * j:3 * j + 3]) for j in range(16)])
    beta, t = rng.randn(10), np.array([0.05, -0.03, 0.6]) + 0.1 * rng.randn(3)
    f = rng.randint(0, NF, P).astype(np.int32)
    b = rng.dirichlet(np.ones(3), P).astype(np.float32)
    faces = np.asarray(faces, np.int64).reshape(NF, 3)
    y = (surface_points(V.vertices_of(C, R, beta), faces[f], b.astype(np.float64)) + t).astype(np.float32)
    return y, f, b, (R, beta, t)


def registration_case(C, faces, seed, P):
    """A cloud and a start for the ICP loop: the truth is drawn as surface_case draws it with fingers hands_mean + 0.3 randn;
    the cloud is P points uniform on the posed mesh (+ t), rounded to fp32; the start is the truth with every rotation turned
    by 0.05 rad about a random axis, beta + 0.1 randn and t moved by 5 mm in a random direction, rounded to fp32.
    -> points (P,3) fp32, start (pose, beta, transl) fp32, truth (R, beta, t)."""
    rng = np.random.RandomState(seed)
    aa = np.concatenate([2.0 * rng.randn(3), C.pose_mean[3:] + 0.3 * rng.randn(45)])
    R = np.stack([exp_so3(aa[3 * j:3 * j + 3]) for j in range(16)])
    beta, t = rng.randn(10), np.array([0.05, -0.03, 0.6]) + 0.1 * rng.randn(3)
    pts = (sample_surface(V.vertices_of(C, R, beta), faces, P, rng)[0] + t).astype(np.float32)
    unit = lambda: (lambda x: x / np.linalg.norm(x))(rng.randn(3))
    start = (np.stack([R[j] @ exp_so3(0.05 * unit()) for j in range(16)]).astype(np.float32),
             (beta + 0.1 * rng.randn(10)).astype(np.float32), (t + 0.005 * unit()).astype(np.float32))
    return pts, start, (R, beta, t)


STARVE = dict(rounds=3, iters=3, lambda_beta=100.0, lambda_pose=100.0, tangent_weight=0.1, max_dist=1e-4)


def starved_case(C, faces, seed, at_the_mean, P=128):
    """A noise-free cloud on the model's own surface with init = the truth, for the loop under STARVE: priors heavy enough to
    pull a hand that is away from the mean pose off its cloud in round 1, so that the 0.1 mm trim leaves round 2 fewer than four
    points (seed 30: one) -- while a hand AT the mean pose and beta = 0 (``at_the_mean``) feels no prior and is fitted in
    every round.  -> points (P,3) fp32, init fp32."""
    rng = np.random.RandomState(seed)
    if at_the_mean:
        R, beta = V.rest_pose(C).copy(), np.zeros(10)
        R[0] = exp_so3(2.0 * rng.randn(3))
    else:
        aa = np.concatenate([2.0 * rng.randn(3), C.pose_mean[3:] + 0.5 * rng.randn(45)])
        R, beta = np.stack([exp_so3(aa[3 * j:3 * j + 3]) for j in range(16)]), rng.randn(10)
    t = np.array([0.05, -0.03, 0.6])
    pts = (sample_surface(V.vertices_of(C, R, beta), faces, P, rng)[0] + t).astype(np.float32)
    return pts, (R.astype(np.float32), beta.astype(np.float32), t.astype(np.float32))


def sample_surface(verts, faces, n, rng):
    """n points uniform on the mesh by area (faces of zero area never drawn, a repeated face counted once) -> points (n,3) fp64, face (n), coefficients (n,3)."""
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    first = np.sort(np.unique(F, axis=0, return_index=True)[1])           # a padded list repeats faces: each counts once
    T = np.asarray(verts, np.float64)[F[first]]
    area = 0.5 * np.sqrt((np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]) ** 2).sum(1))
    pick = rng.choice(len(first), n, p=area / area.sum())
    f, T = first[pick], np.asarray(verts, np.float64)[F]
    u, v = rng.rand(n), rng.rand(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    b = np.stack([1 - u - v, u, v], 1)
    return np.einsum("ki,kic->kc", b, T[f]), f, b
