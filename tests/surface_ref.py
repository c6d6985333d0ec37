"""fp64 numpy restatement of the surface distances (hands_mesh_closest_f32, hands_eval_surface_metrics_f32 and
hands_amd.interhand_field), written from their definitions in include/hands_hip.h.

Point to triangle: the minimum of the in-plane projection -- taken only when all three barycentrics are >= 0 and the normal is
not zero -- and of the three clamped segment distances.  That form needs no special case for a degenerate face: a repeated
index or collinear vertices have a zero normal and leave the segments, a zero segment is its end point.  The reference
computes none of this (its interaction field goes to the nearest vertex through pytorch3d, which is absent), so the parity is
unpinned and the closed forms of tests/test_surface_metrics.py pin this file instead.
"""
import numpy as np

from mesh_metrics_ref import nanmean2, nn_distances, similarity_transform

SURF_KEYS = tuple(f"{q}/{a}" for q in ("p2s", "chamfer") for a in ("ra", "pa"))


def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def _segment(p, a, b):
    """Squared distance and closest point of the points p on the segments a b ((...,3) arrays that broadcast)."""
    ab = b - a
    L = _dot(ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(L > 0, _dot(p - a, ab) / L, 0.0)
    c = a + np.clip(t, 0.0, 1.0)[..., None] * ab
    return _dot(p - c, p - c), c


def _cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def point_triangle_pairs(p, a, b, c, want_point=True):
    """Squared distance and closest point of p on the triangle a, b, c; the four arrays (...,3) broadcast against each other."""
    cand = [_segment(p, a, b), _segment(p, a, c), _segment(p, b, c)]
    n = _cross(b - a, c - a)
    nn = _dot(n, n)
    wa = _dot(n, _cross(b - p, c - p))                     # the three barycentrics, times |n|^2
    wb = _dot(n, _cross(c - p, a - p))
    wc = _dot(n, _cross(a - p, b - p))
    inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(nn > 0, _dot(p - a, n) / nn, 0.0)
    pc = p - s[..., None] * n
    cand.append((np.where(inside, _dot(p - pc, p - pc), np.inf), pc))
    d2 = np.stack([x[0] for x in cand])
    if not want_point:
        return d2.min(0), None
    pick = d2.argmin(0)
    pts = np.stack([np.broadcast_to(x[1], pick.shape + (3,)) for x in cand])
    return d2.min(0), np.take_along_axis(pts, pick[None, ..., None], 0)[0]


def point_triangle(p, a, b, c, want_point=True):
    """Squared distances (P,F) and closest points (P,F,3) of the points p (P,3) on the triangles a, b, c (F,3 each)."""
    return point_triangle_pairs(np.asarray(p, np.float64)[:, None, :], *(np.asarray(x, np.float64)[None] for x in (a, b, c)),
                                want_point=want_point)


def usable_faces(verts, faces):
    """Mask (F) of the faces with every index inside [0, V) and every vertex finite."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(verts)
    ok = ((faces >= 0) & (faces < V)).all(1)
    fin = np.isfinite(np.asarray(verts, np.float64)).all(1)
    ok[ok] = fin[faces[ok]].all(1)
    return ok


def _nearest_face(q, T, cull):
    """Index of the nearest triangle of T (F,3,3) for each point of q (P,3), the lowest index among equal ones.  With ``cull``
    only the pairs that can hold the minimum are evaluated: a triangle lies inside the sphere (m, r) about its centroid, so
    its distance is at least |q - m| - r, and the minimum is at most the distance to the nearest first vertex; a face whose
    lower bound exceeds that is strictly farther than the winner.  The result is that of the full search (tests/
    test_surface_metrics.py compares the two)."""
    if not cull:
        return np.concatenate([point_triangle(q[i:i + 128], T[:, 0], T[:, 1], T[:, 2], False)[0].argmin(1)
                               for i in range(0, len(q), 128)])
    m = T.mean(1)
    r = np.sqrt(((T - m[:, None]) ** 2).sum(-1)).max(1) * (1 + 1e-12) + 1e-300
    lower = np.sqrt(((q[:, None] - m[None]) ** 2).sum(-1)) - r[None]
    upper = np.sqrt(((q[:, None] - T[None, :, 0]) ** 2).sum(-1)).min(1) * (1 + 1e-12)
    pi, fi = np.nonzero(lower <= upper[:, None])              # sorted by point, then by face; no point is left without a pair
    d2 = point_triangle_pairs(q[pi], T[fi, 0], T[fi, 1], T[fi, 2], False)[0]
    start = np.flatnonzero(np.r_[True, pi[1:] != pi[:-1]])
    best = np.minimum.reduceat(d2, start)
    hit = np.flatnonzero(d2 == np.repeat(best, np.diff(np.r_[start, len(pi)])))
    return fi[hit[np.unique(pi[hit], return_index=True)[1]]]


def closest_on_mesh_1(points, verts, faces, cull=True):
    """One sample: dist (P), face_idx (P), closest (P,3); +inf / -1 / NaN without a usable face, NaN / -1 / NaN for a
    non-finite query.  The lowest face index wins an exact tie."""
    points, verts = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    P = len(points)
    dist, idx, cl = np.full(P, np.inf), np.full(P, -1, np.int64), np.full((P, 3), np.nan)
    ok = usable_faces(verts, faces)
    fin = np.isfinite(points).all(1)
    if ok.any() and fin.any():
        T, q = verts[faces[ok]], points[fin]
        j = _nearest_face(q, T, cull)
        d2, cl[fin] = point_triangle_pairs(q, T[j, 0], T[j, 1], T[j, 2])
        dist[fin] = np.sqrt(d2)
        idx[fin] = np.flatnonzero(ok)[j]
    dist[~fin] = np.nan
    return dist, idx, cl


def closest_on_mesh(points, verts, faces, valid=None):
    """Batch: dist (B,P), face_idx (B,P), closest (B,P,3); a sample with valid[b] == 0 is NaN / -1 / NaN."""
    B, P = np.shape(points)[:2]
    dist, idx, cl = np.full((B, P), np.nan), np.full((B, P), -1, np.int64), np.full((B, P, 3), np.nan)
    for b in range(B):
        if valid is None or valid[b] != 0:
            dist[b], idx[b], cl[b] = closest_on_mesh_1(points[b], verts[b], faces)
    return dist, idx, cl


def distance_to_face(points, verts, faces, face_idx):
    """fp64 distance of points (P,3) to the face face_idx[p] of each; NaN where face_idx is -1."""
    points, verts, face_idx = np.asarray(points, np.float64), np.asarray(verts, np.float64), np.asarray(face_idx)
    out = np.full(len(points), np.nan)
    has = face_idx >= 0
    T = verts[np.asarray(faces, np.int64).reshape(-1, 3)[face_idx[has]]]
    out[has] = np.sqrt(point_triangle_pairs(points[has], T[:, 0], T[:, 1], T[:, 2])[0])
    return out


def hand_surface_metrics(pv, gv, pj, gj, faces):
    """One hand (fp32 arrays): p2s/ra, p2s/pa, chamfer/ra, chamfer/pa in millimetres."""
    pv, gv, pj, gj = (np.asarray(a, np.float32) for a in (pv, gv, pj, gj))
    if not all(np.isfinite(a).all() for a in (pv, gv, pj, gj)):
        return [np.nan] * 4
    X, Y = (pv - pj[:1]).astype(np.float64), (gv - gj[:1]).astype(np.float64)        # root alignment in fp32
    p2s, chamfer = [], []
    for a in ("ra", "pa"):
        Q = X if a == "ra" else similarity_transform(X, Y)
        if not np.isfinite(Q).all():                      # a constant prediction: no similarity transform
            p2s.append(np.nan), chamfer.append(np.nan)
            continue
        d1, d2 = nn_distances(Y, Q)
        chamfer.append(1000.0 * 0.5 * (d2.mean() + d1.mean()))
        if usable_faces(Y, faces).any():
            p2s.append(1000.0 * 0.5 * (closest_on_mesh_1(Q, Y, faces)[0].mean() + closest_on_mesh_1(Y, Q, faces)[0].mean()))
        else:
            p2s.append(np.nan)
    return p2s + chamfer


def evaluate_surface(pred, targets, faces_r, faces_l):
    """Dict of (B) fp64 arrays with the twelve keys of hands_amd.evaluate_surface_metrics."""
    B = len(pred["mano.v3d.cam.r"])
    vals = {s: np.full((B, 4), np.nan) for s in "rl"}
    for s, hv, faces in (("r", "right_valid", faces_r), ("l", "left_valid", faces_l)):
        valid = np.asarray(targets[hv], np.float32) * np.asarray(targets["is_valid"], np.float32)
        for b in range(B):
            if valid[b] != 0:
                vals[s][b] = hand_surface_metrics(pred[f"mano.v3d.cam.{s}"][b], targets[f"mano.v3d.cam.{s}"][b],
                                                  pred[f"mano.j3d.cam.{s}"][b], targets[f"mano.j3d.cam.{s}"][b], faces)
    out = {}
    for i, k in enumerate(SURF_KEYS):
        out[k + "/r"], out[k + "/l"] = vals["r"][:, i], vals["l"][:, i]
        out[k + "/h"] = nanmean2(vals["r"][:, i], vals["l"][:, i])
    return out


def interhand_field(v_r, v_l, faces_r, faces_l, contact_bnd=3e-3, dist_min=None, dist_max=None, valid=None):
    """dist.rl: right-hand vertices to the left-hand surface (metres, clamped to [dist_min, dist_max] where given), idx.rl the
    closest faces, contact.rl = dist.rl < contact_bnd; .lr the other way round.  ``raw.*`` keeps the distance before the clamp."""
    out = {}
    for k, (q, t, f) in (("rl", (v_r, v_l, faces_l)), ("lr", (v_l, v_r, faces_r))):
        d, i, _ = closest_on_mesh(q, t, f, valid)
        out["raw." + k] = d
        if dist_min is not None or dist_max is not None:
            d = np.where(np.isnan(d), d, np.clip(d, dist_min, dist_max))
        out["dist." + k], out["idx." + k], out["contact." + k] = d, i, (d < contact_bnd).astype(np.int64)
    return out
