"""fp64 numpy restatement of the signed distance, the sealing rule and the penetration quantities (hands_mesh_signed_f32 and
hands_amd/penetration.py), written from their definitions in include/hands_hip.h and DESIGN.md.  The unsigned distance and the
closest face come from tests/surface_ref.py; the analytic pins of tests/test_penetration_ref.py pin this file.
"""
import numpy as np

import surface_ref as SR


# ---- meshes the tests share ------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([[1.0, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    return v, np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])          # outward


def cube():
    """The cube [-1, 1]^3, two outward triangles per side: faces 2 s and 2 s + 1 make up side s (-x, +x, -y, +y, -z, +z)."""
    v = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def octahedron():
    v = np.array([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    return v, np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])


def uv_sphere(n_lon=12, n_lat=8, r=1.0):
    """A closed, outward UV sphere: two poles, n_lat - 1 rings of n_lon vertices; 2 n_lon (n_lat - 1) faces."""
    v = [[0.0, 0.0, r]]
    for i in range(1, n_lat):
        t = np.pi * i / n_lat
        v += [[r * np.sin(t) * np.cos(2 * np.pi * j / n_lon), r * np.sin(t) * np.sin(2 * np.pi * j / n_lon), r * np.cos(t)]
              for j in range(n_lon)]
    v.append([0.0, 0.0, -r])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    last = len(v) - 1
    f += [[last, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)] for j in range(n_lon)]
    return np.array(v), np.array(f)


# ---- the primitive ---------------------------------------------------------------------------------------------------------
def winding_number(points, verts, faces):
    """w (P) of the points (P,3) about the mesh: 1/(4 pi) times the sum of the Van Oosterom-Strackee solid angles of the usable
    faces; a term with both arguments of its atan2 zero is 0."""
    points, verts = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    faces = faces[SR.usable_faces(verts, faces)]
    if len(faces) == 0:
        return np.zeros(len(points))
    a, b, c = (verts[faces[:, k]][None] - points[:, None] for k in range(3))              # (P,F,3)
    la, lb, lc = (np.sqrt(SR._dot(x, x)) for x in (a, b, c))
    num = SR._dot(a, SR._cross(b, c))
    den = la * lb * lc + SR._dot(a, b) * lc + SR._dot(b, c) * la + SR._dot(c, a) * lb
    half = np.where((num == 0) & (den == 0), 0.0, np.arctan2(num, den))
    return half.sum(1) / (2 * np.pi)


def signed_distance(points, verts, faces, valid=None):
    """Batch: sdf (B,P), winding (B,P), face_idx (B,P).  No usable face: +inf / 0 / -1; a non-finite query or valid[b] == 0:
    NaN / NaN / -1."""
    dist, idx, _ = SR.closest_on_mesh(points, verts, faces, valid)
    w = np.full(dist.shape, np.nan)
    for b in range(len(dist)):
        fin = np.isfinite(np.asarray(points[b], np.float64)).all(1) & ~np.isnan(dist[b])
        if (valid is None or valid[b] != 0) and fin.any():
            w[b, fin] = winding_number(np.asarray(points[b])[fin], verts[b], faces)
    with np.errstate(invalid="ignore"):
        sdf = np.where(np.abs(w) >= 0.5, -dist, dist)
    return sdf, w, idx


# ---- sealing ---------------------------------------------------------------------------------------------------------------
def seal_mesh(faces, n_verts):
    """-> (faces with the fans appended, the loops as lists of vertex indices).  Boundary half-edges are those whose edge only
    one face uses; they must chain into simple closed loops; loop k, by lowest vertex, gets the vertex n_verts + k and the fan
    faces (j, i, n_verts + k) for its half-edges i -> j."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if ((faces < 0) | (faces >= n_verts)).any():
        raise ValueError("index out of range")
    use = {}
    for f in faces:
        for i, j in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            if i == j:
                raise ValueError("repeated index")
            use.setdefault((min(i, j), max(i, j)), []).append((int(i), int(j)))
    if any(len(u) > 2 for u in use.values()):
        raise ValueError("non-manifold edge")
    half = [u[0] for u in use.values() if len(u) == 1]
    nxt = dict(half)
    if len(nxt) != len(half) or sorted(nxt) != sorted(nxt.values()):
        raise ValueError("the boundary is not a set of simple loops")
    loops, seen = [], set()
    for s in sorted(nxt):
        if s not in seen:
            loop, v = [], s
            while v not in seen:
                seen.add(v)
                loop.append(v)
                v = nxt[v]
            loops.append(loop)
    fan = [[nxt[i], i, n_verts + k] for k, loop in enumerate(loops) for i in loop]
    return np.concatenate([faces, np.asarray(fan, np.int64).reshape(-1, 3)]), loops


def apply_seal(verts, loops):
    verts = np.asarray(verts)
    return np.concatenate([verts] + [verts[:, loop].mean(1, keepdims=True) for loop in loops], 1)


def edge_uses(faces):
    """{undirected edge: [directed half-edges]} of a face list: a closed, consistently oriented mesh has every edge twice, once
    in each direction."""
    use = {}
    for f in np.asarray(faces):
        for i, j in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            use.setdefault((min(i, j), max(i, j)), []).append((int(i), int(j)))
    return use


# ---- the public functions --------------------------------------------------------------------------------------------------
def _surfaces(v_r, v_l, faces_r, faces_l, seal):
    out = []
    for v, f in ((v_r, faces_r), (v_l, faces_l)):
        v = np.asarray(v, np.float64)
        if seal:
            f, loops = seal_mesh(f, v.shape[1])
            v = apply_seal(v, loops)
        out.append((v, np.asarray(f)))
    return out


def interhand_penetration(v_r, v_l, faces_r, faces_l, seal=True, valid=None):
    """sdf / winding / inside / pen.depth / pen.count, each with .rl and .lr; an invalid sample: NaN floats, 0 integers."""
    (s_r, f_r), (s_l, f_l) = _surfaces(v_r, v_l, faces_r, faces_l, seal)
    out = {}
    for k, q, t, f in (("rl", v_r, s_l, f_l), ("lr", v_l, s_r, f_r)):
        sdf, w, _ = signed_distance(np.asarray(q, np.float64), t, f, valid)
        with np.errstate(invalid="ignore"):
            inside = np.abs(w) >= 0.5
        out["sdf." + k], out["winding." + k], out["inside." + k] = sdf, w, inside.astype(np.int64)
        out["pen.depth." + k] = np.maximum(0.0, -sdf.min(1))                  # min and maximum keep a NaN
        out["pen.count." + k] = inside.sum(1)
    return out


def penetration_grid(v_r, v_l, G):
    """points (B,G^3,3) and cell volume (B) over the intersection of the two bounding boxes, the x index slowest."""
    v_r, v_l = np.asarray(v_r, np.float64), np.asarray(v_l, np.float64)
    lo, hi = np.maximum(v_r.min(1), v_l.min(1)), np.minimum(v_r.max(1), v_l.max(1))
    step = (hi - lo) / G
    i = np.arange(G) + 0.5
    ax = lo[:, None, :] + i[None, :, None] * step[:, None, :]
    B = len(v_r)
    pts = np.stack(np.broadcast_arrays(ax[:, :, None, None, 0], ax[:, None, :, None, 1], ax[:, None, None, :, 2]), -1)
    return pts.reshape(B, G ** 3, 3), np.where((step > 0).all(1), step.prod(1), 0.0)


def grid_windings(points, v_r, v_l, faces_r, faces_l, seal=True, valid=None):
    """The winding numbers (B,P) of given grid points about the right and about the left (sealed) hand."""
    (s_r, f_r), (s_l, f_l) = _surfaces(v_r, v_l, faces_r, faces_l, seal)
    return signed_distance(points, s_r, f_r, valid)[1], signed_distance(points, s_l, f_l, valid)[1]


def lens_volume(r1, r2, d):
    """The volume two balls of radii r1, r2 share, their centres d apart."""
    if d >= r1 + r2:
        return 0.0
    if d <= abs(r1 - r2):
        return 4.0 / 3.0 * np.pi * min(r1, r2) ** 3
    return np.pi * (r1 + r2 - d) ** 2 * (d * d + 2 * d * (r1 + r2) - 3 * (r1 - r2) ** 2) / (12 * d)


def evaluate_penetration(pred_v_r, pred_v_l, faces_r, faces_l, valid, seal=True):
    """pen/depth/{r,l,h} in mm and pen/count/{r,l,h}, (B) fp64 each, NaN for a sample that is not valid."""
    p = interhand_penetration(pred_v_r, pred_v_l, faces_r, faces_l, seal, valid)
    nan = np.isnan(p["pen.depth.rl"]) | np.isnan(p["pen.depth.lr"])
    out = {}
    for key, name, scale in (("pen/depth", "pen.depth", 1000.0), ("pen/count", "pen.count", 1.0)):
        r, l = (np.where(nan, np.nan, p[f"{name}.{k}"] * scale) for k in ("rl", "lr"))
        out[key + "/r"], out[key + "/l"], out[key + "/h"] = r, l, np.fmax(r, l) + 0 * (r + l)
    return out
