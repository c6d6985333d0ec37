"""Exact ties, list boundaries, rejection rules and micro-scenes of the two mesh rasterisers -- csrc/render.hip
(hands_render_silhouette_f32), csrc/shade.hip (hands_mesh_prepare_f32, hands_render_shaded_f32) and the binning core under both,
csrc/raster_tile.h -- through the C ABI, against the tie mode of the float64 restatements (tests/render_ref.py, tests/shade_ref.py,
tie_rel = raster_scenes.TIE_REL).  Conventions as in tests/test_gpu_kernel_edges.py: every output inside a guarded buffer
(edge_util.Out / OutInt: NaN or a second sentinel where the kernel must write, sentinel bands on both sides), the padding of
ld_verts and the surroundings of the vertex block filled with NaN, `EDGE|kernel|case|error|bound` printed before each assert.

The scenes are tests/raster_scenes.py's.  On the dyadic ones every projected coordinate is exact in float32 and the depths of a
tie group are bit-equal in the kernels, so "ties to the lower index", "equal depths go to the lower (mesh, face)" and the
in-order append of the face list decide the picture.  Before a test looks at the GPU's output it asserts in numpy that its scene
has these properties and that the restatement's own excuse sets are EMPTY on it: no pixel whose 10th and 11th depth group lie
within 1e-6 m, no winner within 1e-6 m of another depth group or with a barycentric under 1e-5, no `unsure` pixel of shade_ref.

Bounds.  Indices and "bit-equal to the clean scene" are exact; zbuf / depth 1e-6 m (the project's); the workspace of mesh_prepare
WS_ROUNDINGS x 2^-24 x max(1, |ref|) or 4 x the restatement's float32 error, whichever is larger.  Mask and colour follow the
rule of tests/test_gpu_render.py: 4 x the largest float32-vs-float64 difference of the restatement on the same scene family,
measured on the CPU with these scenes' sigma = 2^-6 and blur_radius = 2^-4 (E32_MASK / E32_RGB below hold the measured figures,
docs/EXPERIMENTS.md the table), and never under a floor that is derived from the operation count alone:
  mask    a pixel blends at most 10 factors 1 - 1 / (1 + expf(d / sigma)).  A factor goes through one division, one expf, one
          add, one reciprocal and one subtract.  The factor lies in [0, 1]; its sensitivity to a relative error of the exponential
          e is e / (1 + e)^2 <= 1/4 and to one of the argument x = d / sigma |x| e / (1 + e)^2 <= 0.23, so each of the five steps
          (expf taken as 2 ulp) moves it by at most 2^-23: 5 x 2^-23 per factor, 50 x 2^-23 for ten factors that are all <= 1, plus
          nine products and the final subtraction of 2^-24 each: MASK_FLOOR = 55 x 2^-23 = 6.6e-6.
  colour  clamp(3 NdotL (diffuse + specular) + 0.5 c) from about 60 float32 operations on quantities of size <= 3 (two
          normalisations, four dot products, the Fresnel, D and G terms), each rounded to 2^-24 relative: RGB_FLOOR = 60 x 3 x 2^-24 =
          1.1e-5.
Neither floor is taken from the kernels' own error."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import raster_scenes as SC
import render_ref as RR
import shade_ref as SR
from edge_util import DEV, EINVAL, In, Out, OutInt, _close, _stream
from hands_amd import _lib
from hands_amd._lib import ShadeScene, check, ptr
from raster_scenes import BLUR, SIGMA, TIE_REL

pytestmark = pytest.mark.gpu

MASK_FLOOR = 55 * 2.0 ** -23
RGB_FLOOR = 60 * 3 * 2.0 ** -24
WS_ROUNDINGS = 16          # a workspace float: at most 7 roundings (transform), 3 + 2 per face + 8 (normal), 5 (projection)
DEPTH_TOL = 1e-6
# the largest |float32 restatement - float64 restatement| per scene family (CPU, tie mode, sigma 2^-6, blur 2^-4)
# (the dyadic families sit at 1-2 ulp of 1: the floors hold there; `sized` un-projects through three general K)
E32_MASK = {"tie12": 2.74e-7, "straddle": 2.74e-7, "stack": 1.67e-7, "tiny": 2.74e-7, "needle": 7.9e-8, "sized": 6.81e-6}
E32_RGB = {"ties": 1.36e-7, "sized": 1.74e-7, "prepare": 2.68e-7}


def mask_tol(family):
    return max(4 * E32_MASK[family], MASK_FLOOR)


def rgb_tol(family):
    return max(4 * E32_RGB[family], RGB_FLOOR)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _padded(verts, pad):
    """(B, N, 3) -> In over (B, 3 N + pad) floats, NaN in the padding, in front and behind; ld_verts."""
    B, N, _ = verts.shape
    flat = np.full((B, 3 * N + pad), np.nan, np.float32)
    flat[:, :3 * N] = verts.reshape(B, -1)
    return In(torch.from_numpy(flat)), 3 * N + pad


# ================================================================================================================================
# silhouette
# ================================================================================================================================
def _sil(verts, faces, K, S, fpp=10, sigma=SIGMA, blur=BLUR, n_faces=None, extras=True, pad=5):
    """hands_render_silhouette_f32 on guarded buffers -> mask (B, S, S), face_idx, zbuf (None without `extras`) as numpy."""
    verts = np.asarray(verts, np.float32)
    verts = verts[None] if verts.ndim == 2 else verts
    B, N, _ = verts.shape
    vin, ld = _padded(verts, pad)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    fd = _t(faces if faces.shape[0] else np.zeros((1, 3), np.int32))
    Kd = _t(np.asarray(K, np.float32).reshape(B, 3, 3))
    mask = Out(B, S, S)
    fi, zb = (OutInt(torch.int32, B, S, S), Out(B, S, S)) if extras else (None, None)
    check(_lib.lib().hands_render_silhouette_f32(vin.ptr(), ld, N, ptr(fd), faces.shape[0] if n_faces is None else n_faces, ptr(Kd),
                                                 B, S, sigma, blur, fpp, mask.ptr(), fi.ptr() if extras else None,
                                                 zb.ptr() if extras else None, _stream()), "render_silhouette")
    return mask.get().numpy(), (fi.get().numpy() if extras else None), (zb.get().numpy() if extras else None)


def sil_ref(verts, faces, K, S, fpp=10, sigma=SIGMA, blur=BLUR, dtype=np.float64):
    return RR.render(verts, faces, K, S, dtype=dtype, sigma=sigma, blur_radius=blur, faces_per_pixel=fpp, tie_rel=TIE_REL)


def assert_no_excuse(case, ref):
    """The restatement's excuse sets (tests/test_gpu_render.py excludes them) are empty: the cap here is 0 pixels."""
    assert not (ref["tie_gap"] < 1e-6).any(), case
    assert not (((ref["z_gap"] < 1e-6) | (ref["win_wmin"] < 1e-5)) & (ref["face_idx"] >= 0)).any(), case


def _check_sil(case, got, b, ref, tol):
    assert_no_excuse(case, ref)
    mask, fi, zb = got[0][b], got[1], got[2]
    assert (mask[ref["n_cand"] == 0] == 0.0).all(), case                        # exactly zero where nothing is in reach
    _close("render_silhouette", case + "/mask", torch.from_numpy(mask), torch.from_numpy(ref["mask"]), tol)
    if fi is not None:
        mism = int((fi[b] != ref["face_idx"]).sum())
        print(f"EDGE|render_silhouette|{case}/face_idx|{mism}|0")
        assert mism == 0, (case, list(zip(*np.nonzero(fi[b] != ref["face_idx"])))[:5])
        _close("render_silhouette", case + "/zbuf", torch.from_numpy(zb[b]), torch.from_numpy(ref["zbuf"]), DEPTH_TOL)
        assert (zb[b][fi[b] < 0] == 0.0).all(), case


@functools.lru_cache(maxsize=None)
def _tie12(rev, flip):
    v, f = SC.tie12(rev, flip)
    K = SC.dyadic_K(64)
    SC.assert_exact_projection(v, K[0], 64)
    SC.assert_tie_group(v, f, K[0], 64, np.arange(12))
    return v, f, K


@pytest.mark.parametrize("rev,flip", [(False, False), (True, False), (False, True), (True, True)])
def test_silhouette_top_k_ties_go_to_the_lower_index(rev, flip):
    """Case 1.  More than 10 candidates at one bit-equal depth: the blend must be that of the lowest-index ones (their dist
    differ, so it shows), face_idx the lowest containing index -- in both face orders and both windings."""
    v, f, K = _tie12(rev, flip)
    refs = {k: sil_ref(v, f, K[0], 64, fpp=k) for k in range(1, 11)}
    assert int((refs[10]["n_cand"] > 10).sum()) == 466
    # observable: blending the HIGHEST-index candidates instead (the tie mode on the reversed face list) differs visibly
    v2, f2 = SC.tie12(not rev, flip)
    other = sil_ref(v2, f2, K[0], 64)
    assert np.abs(other["mask"] - refs[10]["mask"]).max() > 1000 * mask_tol("tie12")
    assert (refs[10]["top"][refs[10]["n_cand"] == 12] == np.arange(10)).all()                     # faces 0..9 where all 12 tie
    for k, ref in refs.items():
        _check_sil(f"tie12 rev={rev} flip={flip} fpp={k}", _sil(v, f, K, 64, fpp=k), 0, ref, mask_tol("tie12"))


@pytest.mark.parametrize("rev", [False, True])
def test_silhouette_ties_across_waves_passes_and_chunks(rev):
    """Case 2.  The tied faces straddle two waves of a pass, two passes of a chunk and two chunks; the list's in-order append and
    the carry of the top 10 across a flush decide which ten are blended."""
    v, f, at = SC.straddle(rev)
    K = SC.dyadic_K(64)
    SC.assert_exact_projection(v, K[0], 64)
    SC.assert_tie_group(v, f, K[0], 64, at)
    ref = sil_ref(v, f, K[0], 64)
    assert int((ref["n_cand"] > 10).sum()) >= 466 and set(SC.TIED_AT) <= set(np.unique(ref["face_idx"]))
    seen = np.unique(ref["top"])
    assert all(i in seen for i in SC.DEEP_AT[-3:])                               # the nearest deep faces are blended somewhere
    _check_sil(f"straddle rev={rev}", _sil(v, f, K, 64), 0, ref, mask_tol("straddle"))
    for k in (1, 9):
        _check_sil(f"straddle rev={rev} fpp={k}", _sil(v, f, K, 64, fpp=k), 0, sil_ref(v, f, K[0], 64, fpp=k), mask_tol("straddle"))


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n", [128, 129, 256, 257, 384, 385, 513])
def test_silhouette_list_boundaries(n, desc):
    """Case 3.  A tile with exactly n surviving faces (a flush fires when the list holds more than 128; it holds 384): the top 10
    and face_idx come from the nearest faces wherever they sit in the list."""
    v, f = SC.stack(n, desc)
    K = SC.dyadic_K(32)
    SC.assert_exact_projection(v, K[0], 32)
    ref = sil_ref(v, f, K[0], 32)
    assert ref["n_cand"][:8].max() > 100 and len(np.unique(ref["face_idx"])) > 5
    near = set(range(n - 16, n)) if desc else set(range(16))
    assert set(np.unique(ref["face_idx"])) - {-1} <= near
    _check_sil(f"stack n={n} desc={desc}", _sil(v, f, K, 32), 0, ref, mask_tol("stack"))


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_silhouette_face_counts_with_only_the_last_face_visible(n):
    K = SC.dyadic_K(32)
    if n == 0:
        v, _ = SC.last_only(1)
        mask, fi, zb = _sil(v, np.zeros((0, 3), np.int32), K, 32)
        print(f"EDGE|render_silhouette|n_faces=0|{np.abs(mask).max():.3e}|0")
        assert (mask == 0.0).all() and (fi == -1).all() and (zb == 0.0).all()
        return
    v, f = SC.last_only(n)
    SC.assert_exact_projection(v, K[0], 32)
    ref = sil_ref(v, f, K[0], 32)
    assert set(np.unique(ref["face_idx"])) == {-1, n - 1}
    _check_sil(f"last_only n={n}", _sil(v, f, K, 32), 0, ref, mask_tol("stack"))


def _rejected():
    """name -> (extra vertices, extra face) appended to the scene of case 1 (36 vertices): each must change nothing."""
    big = [[-0.5, -0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.5, 0.5]]              # in front of everything: would show if drawn
    with_v = lambda i, p: [p if j == i else q for j, q in enumerate(big)]
    nv = 36
    own = [nv, nv + 1, nv + 2]
    return {
        "index -1": (big, [nv, -1, nv + 2]), "index n_verts": (big, [nv, nv + 1, nv + 3]),
        "index INT32_MAX": (big, [2 ** 31 - 1, nv + 1, nv + 2]),
        "Z = 0": (with_v(1, [0.5, -0.5, 0.0]), own), "Z = -0.0": (with_v(2, [0.0, 0.5, -0.0]), own),
        "Z = -1": (with_v(0, [-0.5, -0.5, -1.0]), own),
        "NaN vertex": (with_v(1, [np.nan, -0.5, 0.5]), own), "NaN depth": (with_v(1, [0.5, -0.5, np.nan]), own),
        "Inf vertex": (with_v(2, [np.inf, 0.5, 0.5]), own),
        "collinear": ([[-0.25, -0.25, 0.5], [0.0, 0.0, 0.5], [0.25, 0.25, 0.5]], own),
        "area 2^-27": (SC.tiny(-27).tolist(), own),
    }


def test_silhouette_rejected_faces_change_nothing():
    """Case 4.  An index out of range, a vertex at Z <= 0 (also -0.0), a NaN or Inf vertex, a collinear face and one of
    |area| = 2^-27 <= 1e-8: every output is bit-equal to the clean scene's.  |area| = 2^-26 > 1e-8 is drawn."""
    v, f, K = _tie12(False, False)
    pad3 = np.full((3, 3), 0.5, np.float32)                                     # the clean scene has the same vertex count
    clean = _sil(np.concatenate([v, pad3]), f, K, 64)
    _check_sil("rejected/clean", clean, 0, sil_ref(v, f, K[0], 64), mask_tol("tie12"))
    for name, (ev, ef) in _rejected().items():
        got = _sil(np.concatenate([v, np.asarray(ev, np.float32)]), np.concatenate([f, np.asarray([ef], np.int32)]), K, 64)
        same = all(np.array_equal(a, b) for a, b in zip(got, clean))
        print(f"EDGE|render_silhouette|rejected/{name}|{0 if same else 1}|0")
        assert same, name
    # |area| = 2^-27 really is under the threshold and 2^-26 over it, in float32
    for lg, kept in ((-27, False), (-26, True)):
        a = SC.areas(SC.tiny(lg).astype(np.float32), [[0, 1, 2]], K[0], 64, np.float32)
        assert (abs(a[0]) == 2.0 ** lg) and (abs(a[0]) > np.float32(1e-8)) == kept
    v2, f2 = np.concatenate([v, SC.tiny(-26).astype(np.float32)]), np.concatenate([f, np.asarray([[36, 37, 38]], np.int32)])
    SC.assert_exact_projection(v2, K[0], 64)
    ref = sil_ref(v2, f2, K[0], 64)
    assert (ref["top"] == 12).any() and np.abs(ref["mask"] - sil_ref(v, f, K[0], 64)["mask"]).max() > 0.01      # it is drawn
    _check_sil("kept/area 2^-26", _sil(v2, f2, K, 64), 0, ref, mask_tol("tiny"))


def test_silhouette_needle_edge_counts_as_its_end_point():
    """Case 5.  The shortest edge has squared length 2^-28 <= 1e-8: the `il < 0` path of seg_d2."""
    v, f = SC.needle()
    K = SC.dyadic_K(64)
    SC.assert_exact_projection(v, K[0], 64)
    e = SC.project(v, K[0], 64, np.float32)
    assert (e[0][1] - e[0][0]) ** 2 + (e[1][1] - e[1][0]) ** 2 == np.float32(2.0 ** -28) and abs(SC.areas(v, f, K[0], 64, np.float32)[0]) == 2.0 ** -14
    ref = sil_ref(v, f, K[0], 64)
    assert (ref["n_cand"] > 0).sum() > 100
    _check_sil("needle", _sil(v, f, K, 64), 0, ref, mask_tol("needle"))


@functools.lru_cache(maxsize=None)
def _sized_refs(S, blur):
    V, f, K = SC.sized(S)
    return V, f, K, [sil_ref(V[b], f, K[b], S, blur=blur) for b in range(3)]


@pytest.mark.parametrize("blur", [BLUR, 0.0])
@pytest.mark.parametrize("S", [1, 7, 8, 31, 32, 33])
def test_silhouette_image_sizes_per_image_K_and_optional_outputs(S, blur):
    """Case 6.  Sizes around the 32 x 8 tile, B = 3 with three K, ld_verts = 3 n_verts + 5 (NaN padding), a triangle far larger
    than the image and one across the last corner; blur_radius 0; face_idx / zbuf NULL or not: the same mask bit for bit."""
    V, f, K, refs = _sized_refs(S, blur)
    got = _sil(V, f, K, S, blur=blur)
    for b in range(3):
        _check_sil(f"sized S={S} blur={blur:g} image {b}", got, b, refs[b], mask_tol("sized"))
    assert any((r["face_idx"] == 1).any() for r in refs) or S == 1
    alone = _sil(V, f, K, S, blur=blur, extras=False)
    assert np.array_equal(alone[0], got[0]), S
    if blur == 0.0:
        assert all(((r["n_cand"] > 0) == (r["face_idx"] >= 0)).all() for r in refs)       # only containing faces are candidates


# ================================================================================================================================
# shaded
# ================================================================================================================================
def _prepare(verts, faces, K, S, T=None, csr=None, pad=5, n_faces=None):
    """hands_mesh_prepare_f32 -> the guarded workspace Out(B, N, 8) and what must stay alive with it."""
    from hands_amd.rend_utils import build_vertex_face_csr
    B, N, _ = verts.shape
    vin, ld = _padded(verts, pad)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    F = faces.shape[0] if n_faces is None else n_faces
    off, ids = build_vertex_face_csr(faces[:F], N) if csr is None else csr
    fd = _t(faces if faces.shape[0] else np.zeros((1, 3), np.int32))
    offd, idsd = _t(np.asarray(off, np.int32)), _t(np.asarray(ids, np.int32) if len(ids) else np.zeros(1, np.int32))
    Kd = _t(np.asarray(K, np.float32))
    Td = None if T is None else _t(np.asarray(T, np.float32))
    ws = Out(B, N, 8)
    check(_lib.lib().hands_mesh_prepare_f32(vin.ptr(), ld, N, ptr(fd), F, ptr(offd), ptr(idsd), ptr(Kd), ptr(Td), B, S, ws.ptr(),
                                            _stream()), "mesh_prepare")
    return ws, fd, (vin, offd, idsd, Kd, Td), F


OUTS = ("rgb", "rgb8", "depth", "face_id")


def _shade(meshes, K, S, image=None, outs=OUTS, n_meshes=None, T=None):
    """meshes: dicts with verts (B, N, 3), faces, and optionally color, metallic, roughness, valid (B), face_offset, csr,
    n_faces.  -> the requested outputs as numpy, and the workspaces (checked for their bands)."""
    B = meshes[0]["verts"].shape[0]
    sc, alive, wss = ShadeScene(), [], []
    for m, M in enumerate(meshes):
        ws, fd, keep, F = _prepare(M["verts"], M["faces"], K, S, T=T, csr=M.get("csr"), n_faces=M.get("n_faces"))
        vd = None if M.get("valid") is None else _t(np.asarray(M["valid"], np.float32))
        alive += [ws, fd, keep, vd]
        wss.append(ws)
        sm = sc.mesh[m]
        sm.workspace, sm.faces, sm.valid, sm.n_verts, sm.n_faces = ws.ptr(), ptr(fd), ptr(vd), M["verts"].shape[1], M.get("n_draw", F)
        sm.face_offset = M.get("face_offset", 0)
        sm.color = (C.c_float * 3)(*M.get("color", SC.COLORS[m]))
        sm.metallic, sm.roughness = M.get("metallic", 0.1), M.get("roughness", 1.0)
    sc.n_meshes = len(meshes) if n_meshes is None else n_meshes
    img = None if image is None else _t(np.asarray(image, np.float32))
    o = {"rgb": Out(B, S, S, 3), "rgb8": OutInt(torch.uint8, B, S, S, 3), "depth": Out(B, S, S), "face_id": OutInt(torch.int32, B, S, S)}
    check(_lib.lib().hands_render_shaded_f32(C.byref(sc), ptr(img), B, S, *[o[k].ptr() if k in outs else None for k in OUTS], _stream()),
          "render_shaded")
    got = {k: o[k].get().numpy() for k in outs}
    return got, [w.get().numpy() for w in wss]


def shade_ref(meshes, K, S, b, image=None, T=None, dtype=np.float64):
    ms = [dict(verts=M["verts"][b], faces=np.asarray(M["faces"]).reshape(-1, 3)[:M.get("n_faces")], color=M.get("color", SC.COLORS[m]),
               metallic=M.get("metallic", 0.1), roughness=M.get("roughness", 1.0),
               valid=True if M.get("valid") is None else bool(M["valid"][b] != 0), **{k: M[k] for k in ("csr", "n_draw") if k in M})
          for m, M in enumerate(meshes)]
    return SR.render(ms, K[b], S, T=None if T is None else T[b], image=None if image is None else image[b], dtype=dtype, tie_rel=TIE_REL)


def _face_ids(meshes, ref_face_id):
    """The restatement numbers the faces cumulatively; the kernel adds each mesh's face_offset."""
    want = np.full(ref_face_id.shape, -1, np.int64)
    at = 0
    for M in meshes:
        F = np.asarray(M["faces"]).reshape(-1, 3)[:M.get("n_faces")].shape[0]
        sel = (ref_face_id >= at) & (ref_face_id < at + F)
        want[sel] = ref_face_id[sel] - at + M.get("face_offset", 0)
        at += F
    return want


def _check_shade(case, got, b, ref, meshes, tol, image=None):
    assert not (ref["unsure"]).any(), case                                      # the cap is 0 pixels
    S = ref["rgb"].shape[0]
    if "face_id" in got:
        want = _face_ids(meshes, ref["face_id"])
        mism = int((got["face_id"][b] != want).sum())
        print(f"EDGE|render_shaded|{case}/face_id|{mism}|0")
        assert mism == 0, (case, list(zip(*np.nonzero(got["face_id"][b] != want)))[:5])
    if "depth" in got:
        _close("render_shaded", case + "/depth", torch.from_numpy(got["depth"][b]), torch.from_numpy(ref["depth"].astype(np.float64)), DEPTH_TOL)
    bg = np.ones((S, S, 3), np.float32) if image is None else np.moveaxis(np.asarray(image[b], np.float32), 0, -1)
    empty = ~ref["covered"]
    if "rgb" in got:
        _close("render_shaded", case + "/rgb", torch.from_numpy(got["rgb"][b]), torch.from_numpy(ref["rgb"].astype(np.float64)), tol)
        assert np.array_equal(got["rgb"][b][empty], bg[empty]), case           # the background bit for bit
    if "rgb8" in got:
        lerr = np.abs(got["rgb8"][b].astype(np.int64) - ref["image"].astype(np.int64))
        print(f"EDGE|render_shaded|{case}/rgb8|{int(lerr.max())}|1")
        assert lerr.max() <= 1, case
        assert np.array_equal(got["rgb8"][b][empty], SR.to_uint8(bg)[empty]), case
        if "rgb" in got:
            assert np.array_equal(got["rgb8"][b], SR.to_uint8(got["rgb"][b])), case              # floor(255 x) of the float colour


def _tie_meshes(valid, n_faces=None, offsets=(7, 1000, 2000, 3000)):
    K = SC.dyadic_K(64, 3)
    out = []
    for m, (v, f) in enumerate(SC.same_triangle_meshes(4)):
        SC.assert_exact_projection(v, K[0], 64)
        SC.assert_tie_group(v, f, K[0], 64, np.arange(2))
        M = dict(verts=np.stack([v] * 3), faces=f, face_offset=offsets[m])
        if valid is not None:
            M["valid"] = np.asarray(valid, np.float32)[:, m]
        if n_faces is not None:
            M["n_faces"] = n_faces
        out.append(M)
    return out, K


VALID = ((0, 0, 1, 1), (1, 1, 1, 1), (0, 1, 1, 0))          # per image: mesh 0 off and mesh 2 on; all on; the last mesh off


@pytest.mark.parametrize("n_meshes", [1, 2, 3, 4])
def test_shaded_equal_depths_go_to_the_lower_mesh_and_face(n_meshes):
    """Case 7.  The same triangle in every mesh (and twice in each): the lowest valid (mesh, face) wins, face_id carries the
    mesh's face_offset, the colour is that mesh's."""
    meshes, K = _tie_meshes(VALID)
    meshes = meshes[:n_meshes]
    got, _ = _shade(meshes, K, 64)
    winners = []
    for b in range(3):
        ref = shade_ref(meshes, K, 64, b)
        assert (ref["gap"][ref["covered"]] == np.inf).all()                     # every other covering depth is EQUAL to the winner's
        _check_shade(f"mesh ties M={n_meshes} image {b}", got, b, ref, meshes, rgb_tol("ties"))
        winners.append(set(np.unique(got["face_id"][b])) - {-1})
    on = [[m for m in range(n_meshes) if VALID[b][m]] for b in range(3)]
    assert winners == [({(7, 1000, 2000, 3000)[o[0]]} if o else set()) for o in on], winners
    if n_meshes == 4:
        free, _ = _shade([{k: v for k, v in M.items() if k != "valid"} for M in meshes], K, 64)        # valid = NULL: all present
        assert all(np.array_equal(free[k][0], got[k][1]) for k in OUTS)


@pytest.mark.parametrize("what", ["all off", "no faces"])
def test_shaded_nothing_to_draw_is_the_background(what):
    meshes, K = _tie_meshes(((0, 0, 0, 0),) * 3) if what == "all off" else _tie_meshes(None, n_faces=0)
    image = (np.arange(3 * 3 * 64 * 64) % 256).astype(np.float32).reshape(3, 3, 64, 64) / np.float32(255)
    got, _ = _shade(meshes, K, 64, image=image)
    for b in range(3):
        _check_shade(f"{what} image {b}", got, b, shade_ref(meshes, K, 64, b, image=image), meshes, 0.0, image=image)
    assert (got["face_id"] == -1).all() and (got["depth"] == 0).all()


def test_shaded_ties_across_waves_chunks_and_meshes():
    """Case 7, chunks.  The tied triangle at (mesh, face) positions that straddle two waves, a flush, and meshes that do not
    flush on their own; per image another set of meshes is valid."""
    K = SC.dyadic_K(64, 3)
    valid = ((1, 1, 1, 1), (0, 1, 1, 1), (0, 0, 1, 0))
    meshes = []
    for m, (v, f) in enumerate(SC.straddle_meshes()):
        SC.assert_exact_projection(v, K[0], 64)
        meshes.append(dict(verts=np.stack([v] * 3), faces=f, face_offset=1000 * m, valid=np.asarray(valid, np.float32)[:, m]))
    got, _ = _shade(meshes, K, 64)
    for b, want in enumerate((63, 1000, 2005)):
        ref = shade_ref(meshes, K, 64, b)
        _check_shade(f"straddle meshes image {b}", got, b, ref, meshes, rgb_tol("ties"))
        assert set(np.unique(got["face_id"][b])) == {-1, want}


def _sized_meshes(S):
    V, f, K = SC.sized(S)
    return [dict(verts=V[:, :3], faces=f[:1], color=SC.COLORS[0]), dict(verts=V[:, 3:], faces=f[:1], color=SC.COLORS[1], face_offset=50)], K


@pytest.mark.parametrize("S", [1, 7, 8, 31, 32, 33])
def test_shaded_image_sizes_and_optional_outputs(S):
    """Case 8.  The sizes of case 6 with guard bands on all four outputs; each output requested alone is bit-equal to the
    all-outputs call."""
    meshes, K = _sized_meshes(S)
    image = np.random.RandomState(S).rand(3, 3, S, S).astype(np.float32)
    got, _ = _shade(meshes, K, S, image=image)
    for b in range(3):
        _check_shade(f"sized S={S} image {b}", got, b, shade_ref(meshes, K, S, b, image=image), meshes, rgb_tol("sized"), image=image)
    for k in OUTS:
        alone, _ = _shade(meshes, K, S, image=image, outs=(k,))
        assert np.array_equal(alone[k], got[k]), (S, k)


def test_shaded_rgb8_of_every_level_is_the_float32_floor():
    """Case 8.  A background holding all 256 values k / 255.f: rgb8 == floor(255.f x) in float32, exactly."""
    S = 32
    meshes, K = _sized_meshes(S)
    meshes = meshes[1:]                                                         # the corner triangle alone: nearly all background
    levels = np.arange(256, dtype=np.float32) / np.float32(255)
    b, c, r, x = np.meshgrid(np.arange(3), np.arange(3), np.arange(S), np.arange(S), indexing="ij")
    image = levels[(r * S + x + 85 * c + 7 * b) % 256]
    assert image.dtype == np.float32 and len(np.unique(image[0, 0])) == 256
    got, _ = _shade(meshes, K, S, image=image, outs=("rgb8", "face_id"))
    want = SR.to_uint8(np.moveaxis(image, 1, -1))
    assert want.dtype == np.uint8 and want.shape == got["rgb8"].shape
    empty = got["face_id"] < 0
    bad = int((got["rgb8"][empty] != want[empty]).sum())
    print(f"EDGE|render_shaded|rgb8 levels|{bad}|0")
    assert bad == 0 and empty.sum() > 0.9 * empty.size and len(np.unique(want[empty])) == 256


def _ws_ref(verts, faces, csr, K, S, T, dtype):
    P = SR.transform(verts, T, dtype)
    n = SR.vertex_normals_csr(P, faces, csr[0], csr[1], dtype)
    xn, yn = SR.project(P, K, S, dtype)
    return np.concatenate([P, n, xn[:, None], yn[:, None]], axis=1)


def _check_ws(case, ws, verts, faces, csr, K, S, T):
    for b in range(verts.shape[0]):
        Tb = None if T is None else T[b]
        ref, f32 = _ws_ref(verts[b], faces, csr, K[b], S, Tb, np.float64), _ws_ref(verts[b], faces, csr, K[b], S, Tb, np.float32)
        bound = max(WS_ROUNDINGS * 2.0 ** -24 * max(1.0, np.abs(ref).max()), 4 * np.abs(f32.astype(np.float64) - ref).max())
        _close("mesh_prepare", f"{case} image {b}", torch.from_numpy(ws[b]), torch.from_numpy(ref), bound)
    return ref


def _prepare_scene():
    """Two opposite faces (0, 1, 2) and (0, 2, 1) -- the second is the LAST face: the normals sum it, the picture is drawn from
    the first three (its depth equals face 0's in exact arithmetic only) --, a neighbour (3, 1, 2), a fronto-parallel face
    (4, 5, 6), a vertex 7 that no face uses, and a per-image rigid transform."""
    v = np.array([[-0.5, -0.5, 1.0], [0.25, -0.5, 1.0], [-0.5, 0.375, 1.25], [0.0, 0.0, 1.0],
                  [0.0625, -0.25, 0.75], [0.5, -0.1875, 0.75], [0.125, 0.4375, 0.75], [0.3, 0.3, 2.0]], np.float32)
    v += np.array([0.0137, -0.0071, 0.0], np.float32)                          # off the sample grid: no pixel on an edge
    f = np.array([[0, 1, 2], [4, 5, 6], [3, 1, 2], [0, 2, 1]], np.int32)
    c, s = np.cos(0.3), np.sin(0.3)
    T = np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], [[0, -1, 0, 0.125], [1, 0, 0, -0.0625], [0, 0, 1, 0.5]],
                  [[c, 0, s, 0.02], [0, 1, 0, -0.01], [-s, 0, c, 0.3]]], np.float32)
    return np.stack([v] * 3), f, T


@pytest.mark.parametrize("table", ["built", "empty", "skipped entries"])
def test_mesh_prepare_tables_transform_and_fallback_normal(table):
    """Case 9.  The workspace element by element, through the caller's CSR: all rows empty (every normal zero, every covered
    pixel shaded with n = v), rows holding -1 and n_faces (skipped), two opposite faces at one vertex (the sum is exactly zero),
    a vertex no face uses, a per-image T, NaN in the ld_verts padding."""
    from hands_amd.rend_utils import build_vertex_face_csr
    S = 32
    V, f, T = _prepare_scene()
    K = SC.sized(S)[2]
    off, ids = build_vertex_face_csr(f, 8)
    if table == "empty":
        off, ids = np.zeros(9, np.int32), np.zeros(0, np.int32)
    elif table == "skipped entries":                                            # every row: -1, its faces, n_faces, INT32_MAX
        rows = [[-1] + ids[off[i]:off[i + 1]].tolist() + [f.shape[0], 2 ** 31 - 1] for i in range(8)]
        off, ids = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32), np.concatenate(rows).astype(np.int32)
    meshes = [dict(verts=V, faces=f, csr=(off, ids), color=SC.COLORS[2], n_draw=3)]
    got, wss = _shade(meshes, K, S, T=T)
    ref = _check_ws(f"csr {table}", wss[0], V, f, (off, ids), K, S, T)
    n = wss[0][:, :, 3:6]
    assert (n[:, 7] == 0).all() and (n[:, 0] == 0).all()                        # the unused vertex; the two opposite faces: exactly zero
    assert (n == 0).all() if table == "empty" else (np.abs((n[:, 4:7] ** 2).sum(-1) - 1) < 1e-6).all()
    for b in range(3):
        r = shade_ref(meshes, K, S, b, T=T)
        assert r["covered"].sum() > 20
        _check_shade(f"csr {table} image {b}", got, b, r, meshes, rgb_tol("prepare"))


def test_mesh_prepare_rejects_a_misaligned_workspace():
    V, f, T = _prepare_scene()
    K = SC.sized(32)[2]
    vin, ld = _padded(V, 5)
    fd, offd, idsd, Kd = _t(f), _t(np.zeros(9, np.int32)), _t(np.zeros(1, np.int32)), _t(K)
    ws = Out(3, 8, 8 + 1)
    rc = _lib.lib().hands_mesh_prepare_f32(vin.ptr(), ld, 8, ptr(fd), 4, ptr(offd), ptr(idsd), ptr(Kd), None, 3, 32, ws.ptr() + 4, _stream())
    assert rc == EINVAL
    assert torch.isnan(ws.get()).all()                                          # nothing was written, the bands are intact
