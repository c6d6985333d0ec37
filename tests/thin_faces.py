"""Scenes with nearly degenerate triangles for the mesh distance kernels (tests/test_thin_faces.py on the host,
tests/test_gpu_thin_faces.py on the device).  Plain seeded numpy, no torch: a host-only script can use them.

Single faces.  A row is (shape, L, height / L, centre): the long edge has length L, the apex stands height above it -- over a
foot that is uniform along the edge (`sliver`) or at its middle (`cap`) -- and the face sits about the origin or about CENTRE
(z = 0.5 m, where a coordinate's fp32 spacing is 6e-8 m: the rounded face is then at least that thick, whatever the row asked
for).  A row holds N_ORIENT random orientations, each in all six vertex orders (the routine is not symmetric in its first
vertex) -- more where MORE_ORIENT says so --, and every face has its own P queries, the same for its six orders:
  the three vertices, the three edge midpoints, the centroid;
  `around`: a point of the face plus up to L along each axis;
  `inplane`: in the face's plane on the line of the long edge, up to 4 L past either end, up to two heights beside the line;
  `above`: 1e-7 to 1e-4 m above or below a point of the interior;
  `far`: 0.3 m from the centroid.
Everything is built in fp64 from the fp32-rounded face, rounded to fp32 and clipped to |x| <= 0.6 m.

Meshes.  split_cube and collapsed_grid keep thin faces among ordinary neighbours; mesh_queries gives their query sets.
"""
import itertools

import numpy as np

import penetration_ref as PR
import render_ref
import surface_ref as SR

CENTRE = np.array([0.05, -0.03, 0.5])            # test_gpu_surface_metrics.CENTRE
SIZE = 0.05                                      # test_gpu_penetration.SIZE
LIMIT = 0.6
SHAPES = ("sliver", "cap")
LENGTHS = (1e-4, 1e-3, 1e-2, 1e-1)
RATIOS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
ORDERS = tuple(itertools.permutations(range(3)))
ROWS = tuple((s, L, r, c) for s in SHAPES for L in LENGTHS for r in RATIOS for c in (0, 1))
N_ORIENT = 16
P = 256
# Rows where 16 orientations showed fewer than about ten queries over the bar with the all-fp32 plane test (a face either fails
# for many of its queries or for none, and few of these faces fail): more orientations, until they showed twenty
# (tools/thin_face_table.py --rev <a revision before the fp64 plane test>)
MORE_ORIENT = {("sliver", 1e-4, 1e-4, 1): 32, ("sliver", 1e-4, 1e-6, 1): 24, ("sliver", 1e-3, 1e-4, 1): 24, ("sliver", 1e-3, 1e-5, 1): 24,
               ("cap", 1e-4, 1e-5, 0): 24, ("cap", 1e-4, 1e-6, 1): 32, ("cap", 1e-3, 1e-4, 0): 48, ("cap", 1e-3, 1e-5, 0): 96}


def n_orient(row):
    return MORE_ORIENT.get(ROWS[row], N_ORIENT)


FAMILIES = ("special", "around", "inplane", "above", "far")
_N_SPECIAL = 7


def rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def family_of(P=P):
    """(P) index into FAMILIES of each query of a face."""
    n = (P - _N_SPECIAL) // 4
    return np.r_[np.zeros(P - 4 * n, np.int64), np.repeat(np.arange(1, 5), n)]


def _frame(tri):
    """Of fp64 triangles (n,3,3): the ends of the longest edge (n,3 each), its unit direction, the unit in-plane direction
    towards the third vertex, the unit normal, and the height of the third vertex over the edge."""
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1], tri[:, 0] - tri[:, 2]], 1)
    k = (e ** 2).sum(-1).argmax(1)
    i = np.arange(len(tri))
    p0, p1, p2 = tri[i, k], tri[i, (k + 1) % 3], tri[i, (k + 2) % 3]
    u = (p1 - p0) / np.linalg.norm(p1 - p0, axis=1, keepdims=True)
    w = (p2 - p0) - ((p2 - p0) * u).sum(1, keepdims=True) * u
    h = np.linalg.norm(w, axis=1)
    w = np.where(h[:, None] > 0, w / np.maximum(h, 1e-300)[:, None], 0.0)
    return p0, p1, u, w, np.cross(u, w), h


def _inside(rng, tri, n):
    """n random points of each triangle (m,3,3) -> (m,n,3); barycentrics at least 0.05 each."""
    b = rng.dirichlet([1.0, 1.0, 1.0], (len(tri), n)) * 0.85 + 0.05
    return np.einsum("mnk,mkc->mnc", b, tri)


def inplane_queries(rng, tri, n, reach):
    p0, p1, u, w, _, h = _frame(tri)
    t = reach[:, None] * (1.0 - rng.rand(len(tri), n))                      # (0, reach]
    end = rng.rand(len(tri), n) < 0.5
    base = np.where(end[..., None], p1[:, None] + t[..., None] * u[:, None], p0[:, None] - t[..., None] * u[:, None])
    return base + (2 * h[:, None] * (2 * rng.rand(len(tri), n) - 1))[..., None] * w[:, None]


def above_queries(rng, tri, n):
    nrm = _frame(tri)[4]
    off = 10.0 ** rng.uniform(-7, -4, (len(tri), n)) * rng.choice([-1.0, 1.0], (len(tri), n))
    return _inside(rng, tri, n) + off[..., None] * nrm[:, None]


def single_faces(row, n_orient=None, P=P):
    """-> tri (n_orient, 3, 3) fp32 in the base order (ends of the long edge, apex) and queries (n_orient, P, 3) fp32."""
    shape, L, ratio, centre = ROWS[row]
    n_orient = n_orient or globals()["n_orient"](row)
    rng = np.random.RandomState(1000 + row)
    R = np.linalg.qr(rng.randn(n_orient, 3, 3))[0]
    foot = rng.rand(n_orient) if shape == "sliver" else np.full(n_orient, 0.5)
    u, w = R[:, :, 0], R[:, :, 1]
    c = CENTRE if centre else np.zeros(3)
    tri32 = np.float32(np.stack([c - 0.5 * L * u, c + 0.5 * L * u, c + ((foot - 0.5) * L)[:, None] * u + ratio * L * w], 1))
    tri = tri32.astype(np.float64)
    n = (P - _N_SPECIAL) // 4
    special = [tri[:, 0], tri[:, 1], tri[:, 2], 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2]),
               0.5 * (tri[:, 0] + tri[:, 2]), tri.mean(1)]
    special = np.stack(special + [tri.mean(1)] * (P - 4 * n - _N_SPECIAL), 1)
    around = _inside(rng, tri, n) + L * (2 * rng.rand(n_orient, n, 3) - 1)
    inplane = inplane_queries(rng, tri, n, np.full(n_orient, 4 * L))
    above = above_queries(rng, tri, n)
    d = rng.randn(n_orient, n, 3)
    far = tri.mean(1)[:, None] + 0.3 * d / np.linalg.norm(d, axis=-1, keepdims=True)
    q = np.concatenate([special, around, inplane, above, far], 1)
    return tri32, np.float32(np.clip(q, -LIMIT, LIMIT))


def all_orders(tri, q):
    """Every face in its six vertex orders, the order fastest: (6 n, 3, 3) and (6 n, P, 3)."""
    return np.ascontiguousarray(tri[:, np.array(ORDERS), :].reshape(-1, 3, 3)), np.repeat(q, len(ORDERS), 0)


def single_face_batch(rows=None, P=P):
    """The rows (default: all) as one batch: tri (B, 3, 3), queries (B, P, 3) and the row index (B) of each sample."""
    rows = range(len(ROWS)) if rows is None else rows
    parts = [all_orders(*single_faces(r, None, P)) for r in rows]
    return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
            np.concatenate([np.full(len(p[0]), r) for r, p in zip(rows, parts)]))


def pair_distance(tri, q):
    """The restatement's fp64 distance (n,P) of the points q (n,P,3) to their own face tri (n,3,3)."""
    a, b, c = (np.asarray(tri, np.float64)[:, None, k] for k in range(3))
    return np.sqrt(SR.point_triangle_pairs(np.asarray(q, np.float64), a, b, c, False)[0])


# ---- meshes ----------------------------------------------------------------------------------------------------------------
def split_cube(ratio):
    """penetration_ref.cube() with its face (a, b, c) = faces[0] replaced by (a, m, c), (m, b, c), (a, b, m), m the midpoint of
    a b moved ratio |a b| into the face: closed and outward as before, (a, b, m) is thin.  Scaled and placed as
    test_gpu_penetration.mesh.  -> verts (9,3) fp64, faces (14,3), the indices of the thin faces."""
    v, f = PR.cube()
    a, b, c = f[0]
    ab = v[b] - v[a]
    into = (v[c] - v[a]) - ((v[c] - v[a]) @ ab) / (ab @ ab) * ab
    m = 0.5 * (v[a] + v[b]) + ratio * np.linalg.norm(ab) * into / np.linalg.norm(into)
    v = np.concatenate([v, m[None]])
    f = np.concatenate([[[a, 8, c], [8, b, c], [a, b, 8]], f[1:]])
    return v @ rot([1, 2, 3], 0.3).T * SIZE + CENTRE, f, np.array([2])


def collapsed_grid(ratio, n=8, seed=5):
    """render_ref.mano_sized_mesh() (778 / 1538) with the first vertex of n faces, no two of them near each other, moved to
    within ratio L of the face's opposite edge (length L), over a foot 0.2 to 0.8 along it.  -> verts (778,3) fp64 (not placed),
    faces, the indices of the n thin faces."""
    v, f = render_ref.mano_sized_mesh()
    v = v.astype(np.float64)
    rng = np.random.RandomState(seed)
    used, thin = set(), []
    for k in rng.permutation(len(f)):
        i0, i1, i2 = f[k]
        ring = set(f[(f == i0).any(1)].ravel().tolist())
        if ring & used:
            continue
        e = v[i2] - v[i1]
        up = (v[i0] - v[i1]) - ((v[i0] - v[i1]) @ e) / (e @ e) * e
        v[i0] = v[i1] + rng.uniform(0.2, 0.8) * e + ratio * np.linalg.norm(e) * up / np.linalg.norm(up)
        used |= ring
        thin.append(k)
        if len(thin) == n:
            break
    assert len(thin) == n
    return v, f, np.array(thin)


def mesh_queries(verts, faces, thin, seed, per_face=48, n_clear=512, clear_min=5e-4):
    """Query sets (fp32) of a mesh given as fp32-representable verts:
      `verts`: the vertices plus noise of 0, 0.1, 2 and 8 mm, one level per vertex in turn (test_mano_counts);
      `thin`:  per thin face the `inplane` family (up to 4 L past the ends of its long edge) and the `above` family;
      `clear`: random points about the mesh and the in-plane family again, those at least clear_min from the surface in fp64.
    """
    verts = np.float32(verts).astype(np.float64)
    rng = np.random.RandomState(seed)
    level = np.array([0.0, 1e-4, 2e-3, 8e-3])
    out = {"verts": verts + level[np.arange(len(verts)) % 4][:, None] * rng.randn(len(verts), 3)}
    tri = verts[np.asarray(faces)[thin]]
    L = np.sqrt(((tri - np.roll(tri, 1, 1)) ** 2).sum(-1).max(1))
    inpl = inplane_queries(rng, tri, per_face, 4 * L).reshape(-1, 3)
    out["thin"] = np.concatenate([inpl, above_queries(rng, tri, per_face).reshape(-1, 3)])
    lo, hi = verts.min(0), verts.max(0)
    cand = np.concatenate([0.5 * (lo + hi) + 0.8 * (hi - lo) * (2 * rng.rand(n_clear, 3) - 1), inpl])
    cand = np.clip(np.float32(cand), -LIMIT, LIMIT).astype(np.float64)
    out["clear"] = cand[SR.closest_on_mesh_1(cand, verts, faces)[0] >= clear_min]
    return {k: np.clip(np.float32(x), -LIMIT, LIMIT) for k, x in out.items()}
