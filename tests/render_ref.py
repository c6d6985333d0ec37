"""Restatement of the soft-silhouette rasteriser (hands_amd/render.py, csrc/render.hip) in numpy, for the tests.

It restates the published algorithm -- pytorch3d's naive ``rasterize_meshes`` path followed by
``SoftSilhouetteShader`` -- with the settings of the reference's ``DiffRenderer`` (src/models/hands_light/renderer.py:
112-207), in pixel space, and in the number format it is called with: ``dtype=np.float64`` is the yardstick of the GPU
tests, ``dtype=np.float32`` run against it gives the error a float32 implementation may have (the tolerance of those tests).

Semantics (one hand; verts (N, 3) in the camera frame, faces (F, 3), K (3, 3), S = image size):
  * u = K00 X / Z + K02, v = K11 Y / Z + K12 (no skew), xn = 2u/S - 1, yn = 2v/S - 1, depth = Z;
  * output pixel (r, c) samples xn = (2c+1)/S - 1, yn = (2r+1)/S - 1;
  * edge(p, a, b) = (p.x-a.x)(b.y-a.y) - (p.y-a.y)(b.x-a.x); area = edge(v2, v0, v1); faces with |area| <= 1e-8 and faces
    with a vertex at Z <= 0 are skipped; barycentrics w0 = edge(p, v1, v2) / (area + 1e-8), w1 = edge(p, v2, v0) / .., w2 =
    edge(p, v0, v1) / ..; pz = w0 z0 + w1 z1 + w2 z2 (not clipped: it extrapolates outside the triangle);
  * d2 = min over the three edge segments of the squared distance (a segment of squared length <= 1e-8 is its end point);
    dist = -d2 if w0, w1, w2 > 0 else d2;
  * candidate: dist < blur_radius and pz >= 0; keep the faces_per_pixel candidates of smallest pz (ties: lower face index);
  * alpha = 1 - prod (1 - sigmoid(-dist / sigma));
  * face_idx / zbuf: the candidate of smallest pz among those that contain the pixel (-1 / 0 where none).
"""
import math

import numpy as np

SIGMA = 1e-5
BLUR_RADIUS = math.log(1.0 / 1e-6 - 1.0) * SIGMA
FACES_PER_PIXEL = 10
EPS = 1e-8


def _seg_d2(px, py, ax, ay, bx, by, one):
    ex, ey = bx - ax, by - ay
    l2 = ex * ex + ey * ey
    if l2 <= EPS:
        dx, dy = px - bx, py - by
        return dx * dx + dy * dy
    t = (ex * (px - ax) + ey * (py - ay)) / l2
    t = np.minimum(np.maximum(t, one * 0), one)
    dx, dy = px - (ax + t * ex), py - (ay + t * ey)
    return dx * dx + dy * dy


def candidates(verts, faces, K, S, dtype=np.float64, blur_radius=BLUR_RADIUS):
    """Every (pixel, face) candidate pair of one hand: arrays pix (r * S + c), face, pz, dist, wmin (smallest barycentric), inside."""
    dt = np.dtype(dtype).type
    V = np.asarray(verts).astype(dtype)
    Kd = np.asarray(K).astype(dtype)
    one, two = dt(1), dt(2)
    Sd = dt(S)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = Kd[0, 0] * V[:, 0] / V[:, 2] + Kd[0, 2]
        v = Kd[1, 1] * V[:, 1] / V[:, 2] + Kd[1, 2]
    xn, yn, zz = two * u / Sd - one, two * v / Sd - one, V[:, 2]
    grid = (two * np.arange(S).astype(dtype) + one) / Sd - one           # sample coordinate of pixel index 0..S-1
    blur = dt(blur_radius)
    margin = 2.0 * math.sqrt(max(blur_radius, 0.0)) + 4.0 / S              # window only: a pure speed-up, twice the reach of a candidate
    out = [[], [], [], [], [], []]
    for f, (i0, i1, i2) in enumerate(np.asarray(faces).astype(np.int64)):
        if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= V.shape[0]:       # an index out of range: skipped
            continue
        z0, z1, z2 = zz[i0], zz[i1], zz[i2]
        if not (z0 > 0 and z1 > 0 and z2 > 0):
            continue
        x0, y0, x1, y1, x2, y2 = xn[i0], yn[i0], xn[i1], yn[i1], xn[i2], yn[i2]
        area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
        if not (abs(area) > EPS):
            continue
        lo_x, hi_x = float(min(x0, x1, x2)) - margin, float(max(x0, x1, x2)) + margin
        lo_y, hi_y = float(min(y0, y1, y2)) - margin, float(max(y0, y1, y2)) + margin
        c0, c1 = np.searchsorted(grid, lo_x), np.searchsorted(grid, hi_x)
        r0, r1 = np.searchsorted(grid, lo_y), np.searchsorted(grid, hi_y)
        if c0 >= c1 or r0 >= r1:
            continue
        px, py = grid[None, c0:c1], grid[r0:r1, None]
        den = area + dt(EPS)
        w0 = ((px - x1) * (y2 - y1) - (py - y1) * (x2 - x1)) / den
        w1 = ((px - x2) * (y0 - y2) - (py - y2) * (x0 - x2)) / den
        w2 = ((px - x0) * (y1 - y0) - (py - y0) * (x1 - x0)) / den
        pz = w0 * z0 + w1 * z1 + w2 * z2
        d2 = np.minimum(np.minimum(_seg_d2(px, py, x0, y0, x1, y1, one), _seg_d2(px, py, x1, y1, x2, y2, one)),
                        _seg_d2(px, py, x2, y2, x0, y0, one))
        inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
        dist = np.where(inside, -d2, d2)
        keep = (dist < blur) & (pz >= 0)
        rr, cc = np.nonzero(keep)
        if rr.size == 0:
            continue
        out[0].append((rr + r0) * S + (cc + c0))
        out[1].append(np.full(rr.size, f, np.int64))
        out[2].append(pz[rr, cc].astype(np.float64))
        out[3].append(dist[rr, cc].astype(np.float64))
        out[4].append(np.minimum(np.minimum(w0, w1), w2)[rr, cc].astype(np.float64))
        out[5].append(inside[rr, cc])
    if not out[0]:
        return tuple(np.zeros(0, (np.int64, np.int64, np.float64, np.float64, np.float64, bool)[i]) for i in range(6))
    return tuple(np.concatenate(o) for o in out)


def depth_groups(pix, pz, tie_rel):
    """pix, pz sorted by (pixel, depth) -> a group number per candidate, ascending with (pixel, depth): a candidate starts a
    new group when its pixel changes or its depth exceeds its predecessor's by more than tie_rel x |depth|."""
    if pix.size == 0:
        return np.zeros(0, np.int64)
    new = np.ones(pix.size, bool)
    new[1:] = (pix[1:] != pix[:-1]) | (pz[1:] - pz[:-1] > tie_rel * np.abs(pz[1:]))
    return np.cumsum(new) - 1


def render(verts, faces, K, S, dtype=np.float64, sigma=SIGMA, blur_radius=BLUR_RADIUS, faces_per_pixel=FACES_PER_PIXEL,
           tie_rel=0.0):
    """One hand.  Returns a dict of (S, S) arrays:
    mask, mask_all (every candidate blended: what ignoring faces_per_pixel would give), n_cand, tie_gap (pz of candidate
    faces_per_pixel+1 minus pz of candidate faces_per_pixel, inf where there is no such candidate), face_idx, zbuf, z_gap
    (second nearest containing depth minus the nearest, inf where there is no second), win_wmin (smallest barycentric of the
    winning face, inf where none) and top (S, S, faces_per_pixel): the blended faces in blending order, -1 where fewer.

    tie_rel = 0 (the default) orders a pixel's candidates by the computed depth alone, the face index deciding between
    bit-equal depths only: depths that are equal in exact arithmetic but differ in the last bit are ordered by that rounding.
    tie_rel > 0 is the tie mode: depths at a pixel that differ by no more than tie_rel x |depth| from their neighbour in depth
    order count as EQUAL and are ordered by face index (the rule "ties: lower face index" for an implementation whose equal
    depths are bit-equal); tie_gap and z_gap are then taken between depth groups only (0 never occurs)."""
    pix, face, pz, dist, wmin, ins = candidates(verts, faces, K, S, dtype, blur_radius)
    n = S * S
    order = np.lexsort((face, pz, pix))                      # by pixel, then depth, then face index
    pix, face, pz, dist, wmin, ins = pix[order], face[order], pz[order], dist[order], wmin[order], ins[order]
    group = None
    if tie_rel > 0:
        group = depth_groups(pix, pz, tie_rel)
        order = np.lexsort((face, group))                    # the group number ascends with the pixel
        pix, face, pz, dist, wmin, ins, group = (a[order] for a in (pix, face, pz, dist, wmin, ins, group))
    n_cand = np.bincount(pix, minlength=n)
    start = np.concatenate(([0], np.cumsum(n_cand)[:-1]))
    rank = np.arange(pix.size) - start[pix]
    dt = np.dtype(dtype).type
    with np.errstate(over="ignore"):
        prob = (dt(1) / (dt(1) + np.exp((dist.astype(dtype)) / dt(sigma)))).astype(dtype)      # sigmoid(-dist / sigma)
    keep_all, keep_top = np.ones(n, dtype), np.ones(n, dtype)
    np.multiply.at(keep_all, pix, dt(1) - prob)
    top = rank < faces_per_pixel
    np.multiply.at(keep_top, pix[top], dt(1) - prob[top])
    tie_gap = np.full(n, np.inf)
    nxt = np.nonzero(rank == faces_per_pixel)[0]
    tie_gap[pix[nxt]] = pz[nxt] - pz[nxt - 1] if group is None else np.where(group[nxt] == group[nxt - 1], np.inf, pz[nxt] - pz[nxt - 1])
    top_faces = np.full((n, faces_per_pixel), -1, np.int64)
    top_faces[pix[top], rank[top]] = face[top]
    # nearest containing face
    ipix, iface, ipz, iw = pix[ins], face[ins], pz[ins], wmin[ins]
    igroup = None if group is None else group[ins]
    icount = np.bincount(ipix, minlength=n)
    istart = np.concatenate(([0], np.cumsum(icount)[:-1]))
    irank = np.arange(ipix.size) - istart[ipix]
    face_idx, zbuf = np.full(n, -1, np.int64), np.zeros(n)
    z_gap, win_wmin = np.full(n, np.inf), np.full(n, np.inf)
    first = irank == 0
    face_idx[ipix[first]], zbuf[ipix[first]], win_wmin[ipix[first]] = iface[first], ipz[first], iw[first]
    second = np.nonzero(irank == 1)[0]
    if igroup is None:
        z_gap[ipix[second]] = ipz[second] - ipz[second - 1]
    else:                                                    # the nearest containing depth of ANOTHER group
        win_group = np.full(n, -1, np.int64)
        win_group[ipix[first]] = igroup[first]
        other = igroup != win_group[ipix]
        np.minimum.at(z_gap, ipix[other], ipz[other] - zbuf[ipix[other]])
    sh = lambda a: a.reshape(S, S)
    return {"mask": sh((dt(1) - keep_top).astype(np.float64)), "mask_all": sh((dt(1) - keep_all).astype(np.float64)),
            "n_cand": sh(n_cand), "tie_gap": sh(tie_gap), "face_idx": sh(face_idx), "zbuf": sh(zbuf), "z_gap": sh(z_gap),
            "win_wmin": sh(win_wmin), "top": top_faces.reshape(S, S, faces_per_pixel)}


# ---------------------------------------------------------------------------------------------------------------------
# test meshes and poses

def ellipsoid_mesh(n_lat=19, n_lon=40, radii=(0.045, 0.03, 0.09), extra_verts=0):
    """Closed latitude / longitude grid: 2 poles + (n_lat - 1) rings of n_lon vertices = 2 + (n_lat-1) n_lon vertices and
    2 n_lon (n_lat - 1) faces; 19 x 40 gives 722 / 1440.  ``extra_verts`` splits that many faces of the middle ring at their
    centroid (+1 vertex, +2 faces each)."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            v.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    f = []
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            f.append((a, c, b))
            f.append((b, c, d))
    south = len(v) - 1
    for j in range(n_lon):
        f.append((south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    v = np.asarray(v, np.float64)
    f = [tuple(t) for t in f]
    first_mid = n_lon + 2 * n_lon * (n_lat // 2 - 1)
    for k in range(extra_verts):
        a, b, c = f[first_mid + 2 * k]
        m = (v[a] + v[b] + v[c]) / 3.0
        m = m / np.linalg.norm(m)
        v = np.vstack([v, m[None]])
        n = len(v) - 1
        f[first_mid + 2 * k] = (a, b, n)
        f += [(b, c, n), (c, a, n)]
    return (v * np.asarray(radii)).astype(np.float32), np.asarray(f, np.int32)


def mano_sized_mesh():
    """The grid with exactly MANO's counts, 778 vertices and 1538 faces: the 19 x 40 grid (722 / 1440), 56 faces split at their
    centroid (778 / 1552), and the first 14 faces of the north pole's fan left out (an open patch, like MANO's open wrist)."""
    v, f = ellipsoid_mesh(19, 40, extra_verts=56)
    f = f[14:]
    assert v.shape == (778, 3) and f.shape == (1538, 3)
    return v, np.ascontiguousarray(f)


def random_rotation(rng):
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def poses(verts, S, n=6, seed=0):
    """n posed copies of a mesh and their intrinsics: random rotations, depth 0.35-0.8 m, an off-centre principal point, the
    last hand partly out of frame.  The focal length scales with S so that the hand covers the same share of the image."""
    rng = np.random.RandomState(seed)
    V, Ks = [], []
    for i in range(n):
        R = random_rotation(rng)
        depth = 0.35 + 0.45 * rng.rand()
        f = 1000.0 * S / 224.0 * (1.0 + 0.1 * rng.randn())
        cx, cy = S / 2 + 0.08 * S * rng.randn(), S / 2 + 0.08 * S * rng.randn()
        t = np.array([0.02 * rng.randn(), 0.02 * rng.randn(), depth])
        if i == n - 1:
            t[0] = 0.5 * S * depth / f          # centred on the right image border
        V.append((verts.astype(np.float64) @ R.T + t).astype(np.float32))
        Ks.append(np.array([[f, 0.0, cx], [0.0, f * (1.0 + 0.02 * rng.randn()), cy], [0.0, 0.0, 1.0]], np.float32))
    return np.stack(V), np.stack(Ks)
