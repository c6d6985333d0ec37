"""Micro-scenes for the edge tests of the two mesh rasterisers (tests/test_gpu_raster_edges.py) and the CPU pins of the
restatements' tie mode (tests/test_render.py, tests/test_shaded_render.py).  numpy only.

Dyadic scenes.  K = [[S/2, 0, S/2], [0, S/2, S/2], [0, 0, 1]] makes xn = X / Z.  A triangle is given by its NDC corners (multiples
of 1/16, or of 2^-14 where stated) and a depth Z with few mantissa bits; its camera-frame vertex is (xn Z, yn Z, Z).  The product
is exact in float32, the IEEE quotient X / Z is then exactly xn again, and every further step of the projection is a scaling by
a power of two or an exact sum: the float32 projection equals the float64 one bit for bit (`assert_exact_projection`).  Pixel
samples are odd multiples of 1/S: none lies on a vertex or on an axis-aligned edge.  Translated congruent fronto-parallel
triangles have bit-equal float32 areas (`assert_tie_group`), hence bit-equal depths in both kernels (render.hip: zc, shade.hip:
bq.w; the other depth coefficients are exactly 0).

TIE_REL = 2^-16.  The depth gaps of these scenes are at least 2^-10 relative (64 x TIE_REL); the rounding spread of equal depths is
1-2 ulp (4.4e-16) in the float64 restatement and about 2e-7 (three barycentrics of 2^-24 each) in its float32 run (1/76 of TIE_REL)."""
import numpy as np

TIE_REL = 2.0 ** -16
SIGMA, BLUR = 2.0 ** -6, 2.0 ** -4          # different distances give visibly different alphas; reach sqrt(BLUR) = 0.25 NDC

BASE = ((-0.75, -0.5), (0.0, -0.5), (-0.75, 0.25))                     # the tie scenes' triangle, shifted by k/16 in x
FLAT = ((-0.75, -0.5), (0.0, -0.5), (-0.75, 0.0))                      # the shaded scenes': its hypotenuse 2x + 3y = -1.5 meets no sample
SMALL = ((-0.5, -0.9375), (-0.25, -0.9375), (-0.5, -0.6875))           # the list-boundary scenes' (S = 32, tile (0, 0))
GHOST = ((-2.0, 6.0), (6.0, 6.0), (6.0, -2.0))      # its box holds the image (it survives every tile's cull, grown or not), its
#                                                     interior x + y > 4 does not, and its nearest edge is sqrt(2) away: in the list
#                                                     of every tile, a candidate at no pixel
AWAY = ((7.0, 0.0), (7.5, 0.0), (7.0, 0.5))         # outside every tile's reach: culled


def dyadic_K(S, B=1):
    K = np.array([[S / 2, 0, S / 2], [0, S / 2, S / 2], [0, 0, 1]], np.float32)
    return np.stack([K] * B)


def tri(pts, z=1.0, dx=0.0, dy=0.0, flip=False):
    p = [(x + dx, y + dy) for x, y in pts]
    if flip:
        p = [p[0], p[2], p[1]]
    return np.array([[x * z, y * z, z] for x, y in p], np.float64)


def soup(tris):
    """Triangles (3, 3) -> verts (3 F, 3) float32, exactly the float64 values, and faces (F, 3) int32, no vertex shared."""
    v64 = np.concatenate(tris) if len(tris) else np.zeros((0, 3))
    v = v64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), v64)
    return v, np.arange(v.shape[0], dtype=np.int32).reshape(-1, 3)


def project(verts, K, S, dtype):
    V, K = np.asarray(verts).astype(dtype), np.asarray(K).astype(dtype)
    t = np.dtype(dtype).type
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = K[0, 0] * V[:, 0] / V[:, 2] + K[0, 2], K[1, 1] * V[:, 1] / V[:, 2] + K[1, 2]
        return t(2) * u / t(S) - t(1), t(2) * v / t(S) - t(1)


def areas(verts, faces, K, S, dtype):
    x, y = project(verts, K, S, dtype)
    i0, i1, i2 = np.asarray(faces).T
    return (x[i2] - x[i0]) * (y[i1] - y[i0]) - (y[i2] - y[i0]) * (x[i1] - x[i0])


def assert_exact_projection(verts, K, S):
    for a32, a64 in zip(project(verts, K, S, np.float32), project(verts, K, S, np.float64)):
        assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)
    # and no sample on a vertex or an axis-aligned line through one: 2 S xn is an even integer or no integer, never odd
    for a in project(verts, K, S, np.float64):
        k = S * (a + 1)                                # a sample has k = 2 c + 1
        assert not np.any((k == np.round(k)) & (np.round(k) % 2 == 1))


def assert_tie_group(verts, faces, K, S, group):
    a32, a64 = areas(verts, faces, K, S, np.float32)[group], areas(verts, faces, K, S, np.float64)[group]
    assert a32.dtype == np.float32 and np.array_equal(a32.astype(np.float64), a64)           # exact
    assert np.all(np.abs(a32) == np.abs(a32[0])) and abs(a32[0]) > 1e-3                       # bit-equal
    z = np.asarray(verts)[np.asarray(faces)[group]][:, :, 2]
    assert np.all(z == z[0, 0])                                                               # fronto-parallel, one depth


# ---------------------------------------------------------------------------------------------------------------------
# silhouette scenes (S = 64 unless stated)

def tie12(rev=False, flip=False):
    """Case 1: 12 congruent triangles at Z = 1, triangle k shifted by k/16 in x; face i is triangle i (rev: 11 - i)."""
    order = range(11, -1, -1) if rev else range(12)
    return soup([tri(BASE, 1.0, dx=k / 16, flip=flip) for k in order])


TIED_AT = (63, 64, 191, 192, 255, 256, 300, 512, 520, 530, 540, 599)
DEEP_AT = (10, 70, 100, 200, 258, 270, 400, 505, 515, 550, 590, 598)


def straddle(rev=False, n=600):
    """Case 2.  The 12 tied triangles at the face indices TIED_AT: 63/64 and 191/192 straddle two waves of pass 0, 255/256 two
    passes of one chunk, 300 and 512 lie in different chunks, 599 is the last lane of the partial last pass.  Pass 0 holds GHOSTs
    at the indices 100..199 and AWAY faces elsewhere: with its tied and deep faces 107 survivors at most, no flush; pass 1 is
    full of survivors (count 363 at most, within the 384 records and over 128: flush); pass 2 flushes as the last.  12 real
    faces at greater, distinct depths (DEEP_AT, the later the nearer) fill the top 10 where fewer than 10 tied faces reach.
    -> verts, faces, the tied face indices in triangle order."""
    tris = [tri(AWAY) if i < 256 and not 100 <= i < 200 else tri(GHOST, 4.0) for i in range(n)]
    for j, i in enumerate(DEEP_AT):
        tris[i] = tri(BASE, 2.0 * (1 + (11 - j) / 64), dx=(j % 6) / 8 - 0.125, dy=(j % 3) / 8)
    at = TIED_AT[::-1] if rev else TIED_AT
    for k, i in enumerate(at):
        tris[i] = tri(BASE, 1.0, dx=k / 16)
    v, f = soup(tris)
    return v, f, np.array(at)


def stack(n, descending):
    """Case 3 (S = 32): n fronto-parallel triangles at distinct depths 1 + j/1024, all in reach of tile (0, 0), no two
    consecutive ones at the same place (so which ten are blended shows in the mask)."""
    tris = []
    for k in range(n):
        j = n - 1 - k if descending else k
        tris.append(tri(SMALL, 1.0 + j / 1024, dx=(k % 8) / 16, dy=((k // 8) % 2) / 16))
    return soup(tris)


def last_only(n):
    """Case 3 (S = 32): n faces, the first n - 1 culled, the last one visible."""
    return soup([tri(AWAY)] * (n - 1) + [tri(SMALL, 1.0, dx=0.125)])


def needle():
    """Case 5: shortest edge 2^-14 (squared 3.7e-9 <= 1e-8: it counts as its end point), area 2^-14 > 1e-8."""
    h = 2.0 ** -14
    return soup([np.array([[-0.25, -0.5, 1.0], [-0.25 + h, -0.5, 1.0], [-0.25, 0.5, 1.0]])])


def tiny(area_log2):
    """Case 4: a right triangle with legs 2^-13 and 2^-13 (area 2^-26) or 2^-14 (2^-27) at (0.0625, -0.625), Z = 0.5."""
    a, b = 2.0 ** -13, 2.0 ** (area_log2 + 13)
    x, y, z = 0.0625, -0.625, 0.5
    return np.array([[x * z, y * z, z], [(x + a) * z, y * z, z], [x * z, (y + b) * z, z]])


def sized(S, B=3):
    """Case 6 / 8: B images of S x S with their own K, one triangle much larger than the image (|ndc| up to 16, one edge
    crossing the image near its centre) at 0.9 m and a small one across the image's last corner at 0.4 m.  The NDC corners are
    fixed, the camera-frame vertices are un-projected through each image's K.  -> verts (B, 6, 3), faces (2, 3), K (B, 3, 3)."""
    big = ((-16.0, -16.3), (16.0, 15.9), (-15.0, 16.0))
    px = 2.0 / S                                             # one pixel in NDC
    small = ((1 - 1.8 * px, 1 - 1.3 * px), (1 + 1.4 * px, 1 - 0.9 * px), (1 - 0.7 * px, 1 + 1.6 * px))
    V, Ks = [], []
    for b in range(B):
        f, cx, cy = S * (0.5 + 0.07 * b), S * (0.5 + 0.03 * b), S * (0.5 - 0.02 * b)
        K = np.array([[f, 0, cx], [0, 1.1 * f, cy], [0, 0, 1]], np.float32)
        K64 = K.astype(np.float64)
        rows = []
        for pts, z in ((big, 0.9), (small, 0.4)):
            for x, y in pts:
                u, v = (x + 1) * S / 2, (y + 1) * S / 2
                rows.append([(u - K64[0, 2]) * z / K64[0, 0], (v - K64[1, 2]) * z / K64[1, 1], z])
        V.append(np.array(rows, np.float32))
        Ks.append(K)
    return np.stack(V), np.array([[0, 1, 2], [3, 4, 5]], np.int32), np.stack(Ks)


# ---------------------------------------------------------------------------------------------------------------------
# shaded scenes

COLORS = ((0.25, 0.5, 0.75), (0.75, 0.25, 0.5), (0.5, 0.75, 0.25), (0.375, 0.375, 0.625))


def same_triangle_meshes(n=4):
    """Case 7: the same triangle (FLAT at Z = 1, twice: faces 0 and 1 of each mesh are the same place) in n meshes."""
    return [soup([tri(FLAT, 1.0), tri(FLAT, 1.0)]) for _ in range(n)]


def straddle_meshes():
    """Case 7, chunks: four meshes of GHOSTs with the tied triangle at (mesh, face) (0, 63), (0, 64), (0, 191), (0, 192),
    (1, 0), (1, 299), (2, 5), (3, 139).  Mesh 0 has 256 faces (one full pass: flush), mesh 1 300, mesh 2 10 (no flush of its own),
    mesh 3 140 (the last lane of the last pass)."""
    out = []
    for n, at in ((256, (63, 64, 191, 192)), (300, (0, 299)), (10, (5,)), (140, (139,))):
        tris = [tri(GHOST, 4.0)] * n
        for i in at:
            tris[i] = tri(FLAT, 1.0)
        out.append(soup(tris))
    return out
