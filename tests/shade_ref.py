"""Restatement of the shaded renderer's semantics (csrc/shade.hip, hands_amd/rend_utils.py) in numpy, fp64 by default.

The reference draws these pictures with pyrender on OpenGL (common/rend_utils.py::Renderer); pyrender is third party and absent,
so the specification of DESIGN.md section 7 is the definition and this file writes it out, one image at a time, with no tiles,
no lists and no chunks.  `dtype=np.float32` runs the same arithmetic in float32: the tests take their tolerance of the float
colour from the difference of the two.

Per image: meshes = [{"verts" (N, 3), "faces" (F, 3), "color" (3) in [0, 1], "metallic", "roughness" (1.0), "valid" (True)}],
K (3, 3), optional T (3, 4) applied to every vertex first, optional background image (3, S, S).
"""
import math

import numpy as np

K_EPS = 1e-8
LIGHT_INTENSITY = 3.0        # three DirectionalLights of intensity 1, all shining along the view axis (rend_utils.py:128-142)
AMBIENT = 0.5
W_UNSURE = 1e-5
GAP_UNSURE = 1e-6            # metres
NV_UNSURE = 1e-5


def uv_sphere(n_lat, n_lon, radius, centre):
    """A closed UV sphere, outward winding in a right-handed frame: 2 + (n_lat - 1) n_lon vertices, 2 n_lon (n_lat - 1) faces."""
    v = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * math.pi * j / n_lon
            v.append((math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)))
    v.append((0.0, 0.0, -1.0))
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    south = len(v) - 1
    f = []
    for j in range(n_lon):
        f.append((0, ring(1, j), ring(1, j + 1)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            f.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    for j in range(n_lon):
        f.append((south, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    verts = (np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64)).astype(np.float32)
    return verts, np.asarray(f, np.int32)


def transform(verts, T, dtype=np.float64):
    P = np.asarray(verts).astype(dtype)
    if T is None:
        return P
    T = np.asarray(T).astype(dtype)
    return (T[None, :, 0] * P[:, 0:1] + T[None, :, 1] * P[:, 1:2] + T[None, :, 2] * P[:, 2:3] + T[None, :, 3]).astype(dtype)


def usable_faces(P, faces):
    """Indices in range (and the vertices they name) -- the faces a normal can be summed over / a pixel can be covered by."""
    faces = np.asarray(faces)
    return ((faces >= 0) & (faces < P.shape[0])).all(axis=1)


def vertex_normals(P, faces, dtype=np.float64):
    """Step 1: area-weighted, summed face by face in ascending order; a face whose cross product is not finite adds nothing."""
    faces = np.asarray(faces)
    acc = np.zeros((P.shape[0], 3), dtype)
    ok = usable_faces(P, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in np.nonzero(ok)[0]:
            i0, i1, i2 = (int(t) for t in faces[f])
            cr = np.cross(P[i1] - P[i0], P[i2] - P[i0]).astype(dtype)
            if not np.isfinite(cr).all():
                continue
            for v in sorted({i0, i1, i2}):
                acc[v] += cr
        s2 = (acc * acc).sum(axis=1)
        good = s2 > dtype(1e-30)
        n = np.zeros_like(acc)
        n[good] = acc[good] / np.sqrt(s2[good])[:, None]
    return n


def vertex_normals_csr(P, faces, csr_off, csr_face, dtype=np.float64):
    """Step 1 through the CALLER's vertex -> face table, as hands_mesh_prepare_f32 gathers it: vertex v sums the faces
    csr_face[csr_off[v] : csr_off[v + 1]] in the order they are listed; an entry outside [0, F), a face with a vertex index out of
    range and a face whose cross product is not finite add nothing.  An empty row gives the zero vector."""
    faces, csr_off, csr_face = np.asarray(faces), np.asarray(csr_off), np.asarray(csr_face)
    acc = np.zeros((P.shape[0], 3), dtype)
    ok = usable_faces(P, faces) if faces.shape[0] else np.zeros(0, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(P.shape[0]):
            for f in csr_face[csr_off[v]:csr_off[v + 1]]:
                if f < 0 or f >= faces.shape[0] or not ok[f]:
                    continue
                i0, i1, i2 = (int(t) for t in faces[f])
                cr = np.cross(P[i1] - P[i0], P[i2] - P[i0]).astype(dtype)
                if np.isfinite(cr).all():
                    acc[v] += cr
        s2 = (acc * acc).sum(axis=1)
        good = s2 > dtype(1e-30)
        n = np.zeros_like(acc)
        n[good] = acc[good] / np.sqrt(s2[good])[:, None]
    return n


def project(P, K, S, dtype=np.float64):
    K = np.asarray(K).astype(dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2]
        v = K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
        return dtype(2) * u / dtype(S) - dtype(1), dtype(2) * v / dtype(S) - dtype(1)


def brdf(c, metallic, roughness, NdotL, NdotV, NdotH, VdotH, dtype=np.float64):
    """Step 5 for one channel value c (arrays broadcast)."""
    one, m = dtype(1), dtype(metallic)
    a = dtype(roughness) * dtype(roughness)
    a2 = a * a
    pi = dtype(math.pi)
    f0 = dtype(0.04) * (one - m) + c * m
    c_diff = dtype(0.96) * c * (one - m)
    t = one - VdotH
    F = f0 + (one - f0) * (t * t * t * t * t)
    dd = NdotH * NdotH * (a2 - one) + one
    D = a2 / (pi * dd * dd)
    g1 = lambda nd: dtype(2) * nd / (nd + np.sqrt(a2 + (one - a2) * nd * nd))
    G = g1(NdotL) * g1(NdotV)
    col = dtype(LIGHT_INTENSITY) * NdotL * ((one - F) * c_diff / pi + F * G * D / (dtype(4) * NdotL * NdotV)) + dtype(AMBIENT) * c
    return np.clip(col, 0, 1)


def render(meshes, K, S, T=None, image=None, dtype=np.float64, tile=None, tie_rel=0.0):
    """One image.  A mesh may carry "csr": (csr_off, csr_face), the caller's vertex -> face table; its normals are then gathered
    through it (vertex_normals_csr) instead of summed over all faces.  "n_draw": only the first n_draw faces are drawn (the
    normals still see them all; face_id counts them all).
    tie_rel = 0 (the default): a face wins a pixel when its computed depth is smaller, so depths that are equal in exact arithmetic
    but differ in the last bit are decided by that rounding.  tie_rel > 0 is the tie mode: a face wins only when it is nearer by
    more than tie_rel x depth; depths closer than that count as EQUAL and stay with the lower (mesh, face), are not `unsure`, and
    `gap` is the distance to the nearest covering depth that is not equal to the winner's.  Returns rgb (S, S, 3), image uint8, depth (0 = empty), face_id (-1 = empty; face index + the faces of the
    meshes before it, valid or not), covered, unsure (the pixels where a float32 implementation may legitimately decide
    otherwise), gap (distance of the two nearest covering depths) and, with tile=(w, h), tile_candidates (rows, cols): the faces
    whose box meets the tile's sample points."""
    one = dtype(1)
    rows, cols = np.arange(S), np.arange(S)
    px = ((2 * cols + 1).astype(dtype) / dtype(S) - one)[None, :]
    py = ((2 * rows + 1).astype(dtype) / dtype(S) - one)[:, None]
    best_z = np.full((S, S), np.inf, dtype)
    second_z = np.full((S, S), np.inf, dtype)
    best = np.full((S, S), -1, np.int64)
    bary = np.zeros((S, S, 3), dtype)
    unsure = np.zeros((S, S), bool)
    if tile is not None:
        tw, th = tile
        tcols, trows = -(-S // tw), -(-S // th)
        tile_cand = np.zeros((trows, tcols), np.int64)
    offset, prepared = 0, []
    for m, mesh in enumerate(meshes):
        faces = np.asarray(mesh["faces"])
        P = transform(mesh["verts"], T, dtype)
        prepared.append((P, faces, offset))
        F = faces.shape[0]
        if not mesh.get("valid", True):
            offset += F
            continue
        xn, yn = project(P, K, S, dtype)
        ok = usable_faces(P, faces)
        ok[mesh.get("n_draw", F):] = False
        for f in np.nonzero(ok)[0]:
            i0, i1, i2 = faces[f]
            x0, y0, z0, x1, y1, z1, x2, y2, z2 = xn[i0], yn[i0], P[i0, 2], xn[i1], yn[i1], P[i1, 2], xn[i2], yn[i2], P[i2, 2]
            if not (z0 > 0 and z1 > 0 and z2 > 0):
                continue
            area = (x2 - x0) * (y1 - y0) - (y2 - y0) * (x1 - x0)
            if not abs(area) > K_EPS:                    # also false for a NaN
                continue
            xlo, xhi, ylo, yhi = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
            if tile is not None:
                # the tile's first and last sample point (the last tile's may lie outside the image)
                cx0 = (2 * np.arange(tcols) * tw + 1) / S - 1
                cx1 = (2 * (np.arange(tcols) * tw + tw - 1) + 1) / S - 1
                cy0 = (2 * np.arange(trows) * th + 1) / S - 1
                cy1 = (2 * (np.arange(trows) * th + th - 1) + 1) / S - 1
                tile_cand += ((ylo <= cy1) & (yhi >= cy0))[:, None] & ((xlo <= cx1) & (xhi >= cx0))[None, :]
            # pixels of the box, grown by one
            c0 = max(int(math.floor((float(xlo) + 1) * S / 2 - 0.5)) - 1, 0)
            c1 = min(int(math.ceil((float(xhi) + 1) * S / 2 - 0.5)) + 1, S - 1)
            r0 = max(int(math.floor((float(ylo) + 1) * S / 2 - 0.5)) - 1, 0)
            r1 = min(int(math.ceil((float(yhi) + 1) * S / 2 - 0.5)) + 1, S - 1)
            if c0 > c1 or r0 > r1:
                continue
            sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
            qx, qy = px[:, c0:c1 + 1], py[r0:r1 + 1, :]
            den = area + dtype(K_EPS)
            w0 = ((qx - x1) * (y2 - y1) - (qy - y1) * (x2 - x1)) / den
            w1 = ((qx - x2) * (y0 - y2) - (qy - y2) * (x0 - x2)) / den
            w2 = ((qx - x0) * (y1 - y0) - (qy - y0) * (x1 - x0)) / den
            unsure[sl] |= np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2)) < W_UNSURE
            inside = (w0 > 0) & (w1 > 0) & (w2 > 0)
            if not inside.any():
                continue
            q0, q1, q2 = w0 / z0, w1 / z1, w2 / z2
            with np.errstate(divide="ignore", invalid="ignore"):
                z = one / (q0 + q1 + q2)
            z = np.where(inside, z, np.inf).astype(dtype)
            bz, sz, bb, bw = best_z[sl], second_z[sl], best[sl], bary[sl]
            if tie_rel > 0:
                with np.errstate(invalid="ignore"):
                    wins = z < np.where(np.isfinite(bz), bz - dtype(tie_rel) * np.abs(bz), bz)
                    tied = ~wins & (z <= bz + dtype(tie_rel) * np.abs(bz))
                second_z[sl] = np.where(wins, bz, np.where(tied, sz, np.minimum(sz, z)))
            else:
                wins = z < bz                             # strict: equal depths stay with the lower (mesh, face)
                second_z[sl] = np.where(wins, bz, np.minimum(sz, z))
            best_z[sl] = np.where(wins, z, bz)
            best[sl] = np.where(wins, offset + f, bb)
            with np.errstate(invalid="ignore"):             # 0 x inf outside the face: never selected
                nb = np.stack([q0 * z, q1 * z, q2 * z], axis=-1)
            bary[sl] = np.where(wins[..., None], nb, bw)
        offset += F

    covered = best >= 0
    rgb = np.ones((S, S, 3), dtype)
    if image is not None:
        rgb = np.ascontiguousarray(np.moveaxis(np.asarray(image).astype(dtype), 0, -1))
    rr, cc = np.nonzero(covered)
    if rr.size:
        gid = best[rr, cc]
        for m, mesh in enumerate(meshes):
            P, faces, off = prepared[m]
            sel = (gid >= off) & (gid < off + faces.shape[0])
            if not sel.any() or not mesh.get("valid", True):
                continue
            nrm = vertex_normals_csr(P, faces, *mesh["csr"], dtype) if "csr" in mesh else vertex_normals(P, faces, dtype)
            tri = faces[gid[sel] - off]
            b = bary[rr[sel], cc[sel]]
            Pp = (b[:, :, None] * P[tri]).sum(axis=1)
            n = (b[:, :, None] * nrm[tri]).sum(axis=1)
            v = -Pp / np.sqrt((Pp * Pp).sum(axis=1))[:, None]
            n2 = (n * n).sum(axis=1)
            zero = ~(n2 > dtype(1e-30))
            n = np.where(zero[:, None], v, n / np.sqrt(np.where(zero, one, n2))[:, None])
            ndv = (n * v).sum(axis=1)
            unsure[rr[sel], cc[sel]] |= np.abs(ndv) < NV_UNSURE
            n = np.where((ndv < 0)[:, None], -n, n)
            ndv = np.abs(ndv)
            l = np.array([0, 0, -1], dtype)
            h = v + l
            h = h / np.sqrt((h * h).sum(axis=1))[:, None]
            NdotL = np.clip((n * l).sum(axis=1), dtype(0.001), one)
            NdotV = np.clip(ndv, dtype(0.001), one)
            NdotH = np.clip((n * h).sum(axis=1), 0, one)
            VdotH = np.clip((v * h).sum(axis=1), 0, one)
            col = np.asarray(mesh["color"]).astype(dtype)
            for k in range(3):
                rgb[rr[sel], cc[sel], k] = brdf(col[k], mesh.get("metallic", 0.1), mesh.get("roughness", 1.0), NdotL, NdotV, NdotH,
                                                VdotH, dtype)
    with np.errstate(invalid="ignore"):
        gap = second_z - best_z
    gap[~covered] = np.inf
    gap[np.isnan(gap)] = np.inf
    unsure |= gap < GAP_UNSURE
    out = {"rgb": rgb, "image": to_uint8(rgb), "depth": np.where(covered, best_z, 0).astype(dtype), "face_id": best.astype(np.int32),
           "covered": covered, "unsure": unsure, "gap": gap}
    if tile is not None:
        out["tile_candidates"] = tile_cand
    return out


def to_uint8(x):
    """Step 6: floor(255 x) (rend_utils.py:100), on values clamped to [0, 1]."""
    x = np.asarray(x)
    return np.floor(np.clip(x.dtype.type(255) * x, 0, 255)).astype(np.uint8)


def sideview_T(anchor_verts, angle_deg, cam_transl=None):
    """rend_utils.py:62-78 after flip_meshes, in the camera frame: a rotation by -angle about +y around the anchor's vertex
    mean; the x-negation of cam_transl (:55) and the 180-degree flip cancel.  T = [R | c - R c + cam_transl], fp64."""
    c = np.asarray(anchor_verts, np.float64).mean(axis=0)
    a = -math.radians(angle_deg)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    t = c - R @ c + (0.0 if cam_transl is None else np.asarray(cam_transl, np.float64))
    return np.concatenate([R, t[:, None]], axis=1)
