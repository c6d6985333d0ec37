"""Surface distances without a GPU: the fp64 restatement (tests/surface_ref.py) against closed forms with dyadic coordinates,
the host side of the two C-ABI entries and the three Python names, and a compile-only resource guard of csrc/mesh_distance.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import render_ref
import surface_ref as SR
from mesh_metrics_ref import similarity_transform

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
# query, distance, closest point on the triangle (0,0,0), (1,0,0), (0,1,0): above the interior, beside an edge, beyond a vertex
CLOSED_FORMS = (((0.25, 0.25, 0.5), 0.5, (0.25, 0.25, 0.0)),
                ((0.5, -0.5, 0.0), 0.5, (0.5, 0.0, 0.0)),
                ((-0.375, -0.5, 0.0), 0.625, (0.0, 0.0, 0.0)))
# degenerate faces over the vertices a = (0,0,0), b = (1,0,0), c = (0.5,0,0) (collinear with a, b), query (0.25, 0.5, 0):
# (a,a,b) is the segment a b, (a,a,a) the point a, (a,c,b) three collinear vertices = the segment a b again
DEGENERATE_VERTS = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0, 0]], np.float64)
DEGENERATE = (((0, 0, 1), (0.25, 0.5, 0.0), 0.5, (0.25, 0.0, 0.0)),
              ((0, 0, 0), (0.375, 0.5, 0.0), 0.625, (0.0, 0.0, 0.0)),
              ((0, 2, 1), (0.75, 0.5, 0.0), 0.5, (0.75, 0.0, 0.0)),
              ((0, 2, 1), (1.375, 0.5, 0.0), 0.625, (1.0, 0.0, 0.0)))


def test_point_triangle_closed_forms():
    for q, d, c in CLOSED_FORMS:
        dist, idx, cl = SR.closest_on_mesh_1(np.array([q]), TRI, [[0, 1, 2]])
        assert dist[0] == d and idx[0] == 0 and (cl[0] == c).all(), q
        dist2, _, cl2 = SR.closest_on_mesh_1(np.array([q]), TRI, [[2, 0, 1]])          # whatever the vertex order
        assert dist2[0] == d and (cl2[0] == c).all(), q


def test_degenerate_faces_are_segments_and_points():
    for face, q, d, c in DEGENERATE:
        dist, idx, cl = SR.closest_on_mesh_1(np.array([q]), DEGENERATE_VERTS, [face])
        assert dist[0] == d and idx[0] == 0 and (cl[0] == c).all(), face


def test_skipped_faces_ties_and_non_finite_queries():
    verts = np.concatenate([TRI, TRI + [0, 0, 1.0]])
    faces = [[0, 1, 6], [3, 4, 5], [0, 1, 2], [0, 1, 2], [-1, 1, 2]]                   # out of range, far, near, its copy, negative
    q = np.array([[0.25, 0.25, 0.25], [np.nan, 0, 0], [0.25, 0.25, np.inf]])
    dist, idx, cl = SR.closest_on_mesh_1(q, verts, faces)
    assert dist[0] == 0.25 and idx[0] == 2                                             # the lower of two equal faces
    assert np.isnan(dist[1:]).all() and (idx[1:] == -1).all() and np.isnan(cl[1:]).all()
    dist, idx, cl = SR.closest_on_mesh_1(q[:1], verts, [[0, 1, 6]])
    assert dist[0] == np.inf and idx[0] == -1 and np.isnan(cl).all()
    dist, idx, cl = SR.closest_on_mesh_1(q[:1], verts, np.zeros((0, 3), np.int64))
    assert dist[0] == np.inf and idx[0] == -1
    verts[4, 1] = np.nan                                                               # a face with a non-finite vertex is skipped
    dist, idx, _ = SR.closest_on_mesh_1(q[:1], verts, faces)
    assert dist[0] == 0.25 and idx[0] == 2
    d, i, c = SR.closest_on_mesh(q[None, :1].repeat(2, 0), verts[None].repeat(2, 0), faces, valid=[0.0, 1.0])
    assert np.isnan(d[0]).all() and i[0, 0] == -1 and d[1, 0] == 0.25


def test_culled_search_is_the_full_search():
    """The restatement skips the pairs that cannot hold the minimum; the answer is that of all pairs, ties included."""
    from hands_amd.mano import synthetic_mano_asset
    rng = np.random.RandomState(1)
    a = synthetic_mano_asset(True)
    grid_v, grid_f = render_ref.mano_sized_mesh()
    for v, f in ((a.v_template[:200], rng.randint(0, 200, (300, 3))), (grid_v, grid_f[::3])):
        f = np.concatenate([f, f[:40]])                                                # exact ties between a face and its copy
        q = np.concatenate([v[::7], v[::5] + 4e-3 * rng.randn(*v[::5].shape)])
        full, culled = SR.closest_on_mesh_1(q, v, f, cull=False), SR.closest_on_mesh_1(q, v, f, cull=True)
        for x, y in zip(full, culled):
            assert np.array_equal(x, y)


def _batch(pv, gv, pj, gj):
    one = lambda x: np.float32(x)[None]
    pred = {"mano.v3d.cam.r": one(pv), "mano.v3d.cam.l": one(pv), "mano.j3d.cam.r": one(pj), "mano.j3d.cam.l": one(pj)}
    targets = {"mano.v3d.cam.r": one(gv), "mano.v3d.cam.l": one(gv), "mano.j3d.cam.r": one(gj), "mano.j3d.cam.l": one(gj),
               "is_valid": np.ones(1, np.float32), "right_valid": np.ones(1, np.float32), "left_valid": np.zeros(1, np.float32)}
    return pred, targets


def _grid(n=9, step=2.0 ** -7):
    """A flat n x n grid in the plane z = 0.5 (dyadic coordinates), two triangles per cell."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i * step, j * step, np.full_like(i, 0.5, dtype=np.float64)], -1).reshape(-1, 3)
    f = [t for a in range(n - 1) for b in range(n - 1)
         for t in ((a * n + b, a * n + b + 1, (a + 1) * n + b), (a * n + b + 1, (a + 1) * n + b + 1, (a + 1) * n + b))]
    return v, np.asarray(f, np.int64)


def test_identical_meshes_have_zero_distance():
    v, f = render_ref.mano_sized_mesh()
    j = np.tile(v[:1], (21, 1))
    out = SR.evaluate_surface(*_batch(v, v, j, j), f, f)
    assert len(out) == 12
    for k in ("p2s/ra/r", "chamfer/ra/r", "p2s/ra/h", "chamfer/ra/h"):
        assert out[k][0] == 0.0, k
    assert out["p2s/pa/r"][0] < 1e-9 and out["chamfer/pa/r"][0] < 1e-9
    assert all(np.isnan(out[k][0]) for k in out if k.endswith("/l"))


def test_shifted_flat_grid_is_the_shift():
    v, f = _grid()
    d = 2.0 ** -8
    j = np.tile(v[:1], (21, 1))
    out = SR.evaluate_surface(*_batch(v + [0, 0, d], v, j, j), f, f)                   # equal root joints: ra keeps the shift
    assert out["p2s/ra/r"][0] == 1000.0 * d and out["chamfer/ra/r"][0] == 1000.0 * d
    assert out["p2s/pa/r"][0] < 1e-9 and out["chamfer/pa/r"][0] < 1e-9                 # pa undoes it


def test_similarity_transformed_copy_has_zero_pa_distance():
    v, f = render_ref.mano_sized_mesh()
    v = v.astype(np.float64)
    th = 0.6
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    X = 1.25 * v @ R.T + [0.01, -0.02, 0.03]
    Q = similarity_transform(X, v)                                                     # in fp64 end to end
    assert SR.closest_on_mesh_1(Q, v, f)[0].mean() * 1000.0 <= 1e-9 and SR.closest_on_mesh_1(v, Q, f)[0].mean() * 1000.0 <= 1e-9
    j = np.tile(v[:1], (21, 1))
    out = SR.evaluate_surface(*_batch(X, v, 1.25 * j @ R.T + [0.01, -0.02, 0.03], j), f, f)   # fp32 inputs leave 1e-8 m
    assert out["p2s/pa/r"][0] < 1e-4 and out["chamfer/pa/r"][0] < 1e-4 and out["chamfer/ra/r"][0] > 1.0


def test_p2s_is_at_most_chamfer_when_every_vertex_lies_in_a_face():
    v, f = render_ref.mano_sized_mesh()
    assert len(np.unique(f)) == len(v)
    rng = np.random.RandomState(0)
    j = np.tile(v[:1], (21, 1))
    for noise in (1e-4, 2e-3, 8e-3):
        out = SR.evaluate_surface(*_batch(v + noise * rng.randn(*v.shape), v, j, j), f, f)
        for a in ("ra", "pa"):
            assert 0 < out[f"p2s/{a}/r"][0] <= out[f"chamfer/{a}/r"][0], (noise, a)


def test_no_usable_face_leaves_chamfer():
    v, f = _grid(4)
    j = np.tile(v[:1], (21, 1))
    out = SR.evaluate_surface(*_batch(v + [0, 0, 0.25], v, j, j), f + 100, np.zeros((0, 3), np.int64))
    assert np.isnan(out["p2s/ra/r"][0]) and out["chamfer/ra/r"][0] == 250.0


def test_interhand_field_of_the_restatement():
    v, f = _grid(4)
    out = SR.interhand_field((v + [0, 0, 2.0 ** -9])[None], v[None], f, f, contact_bnd=3e-3, dist_min=2.0 ** -8, dist_max=1.0)
    assert (out["raw.rl"] == 2.0 ** -9).all() and (out["dist.rl"] == 2.0 ** -8).all() and (out["contact.rl"] == 0).all()
    out = SR.interhand_field((v + [0, 0, 2.0 ** -9])[None], v[None], f, f)
    assert (out["dist.lr"] == 2.0 ** -9).all() and (out["contact.lr"] == 1).all() and out["idx.lr"].min() >= 0


# ---- the API surface (these fail without the feature) ---------------------------------------------------------------------
def test_names_are_exported():
    import hands_amd
    for n in ("evaluate_surface_metrics", "closest_on_mesh", "interhand_field"):
        assert n in hands_amd.__all__ and callable(getattr(hands_amd, n)), n


def test_surface_functions_refuse_cpu_tensors():
    import hands_amd
    v, f = _grid(4)
    j = np.tile(v[:1], (21, 1))
    pred, targets = ({k: torch.from_numpy(x) for k, x in d.items()} for d in _batch(v, v, j, j))
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.evaluate_surface_metrics(pred, targets, faces=(f, f))
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.closest_on_mesh(pred["mano.v3d.cam.r"], pred["mano.v3d.cam.r"], f)
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.interhand_field(pred, faces=(f, f))


def test_header_and_binding_hold_the_entries():
    from hands_amd import _lib
    from hands_amd.metrics import SURF_KEYS
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    for name in ("hands_mesh_closest_f32", "hands_eval_surface_metrics_f32"):
        assert re.search(rf"^int\s+{name}\s*\(", header, flags=re.M) and name in _lib.SIGNATURES, name
    assert f"#define HANDS_SURF_MAX_F {_lib.SURF_MAX_F}" in header and _lib.SURF_MAX_F >= 4096
    assert f"#define HANDS_SURF_CHUNK {_lib.SURF_CHUNK}" in header and f"#define HANDS_SURF_NQ {_lib.SURF_NQ}" in header
    assert "#define HANDS_ABI_VERSION 5" in header
    assert ctypes.sizeof(_lib.SurfEvalOut) == 3 * _lib.SURF_NQ * ctypes.sizeof(ctypes.c_void_p) and len(SURF_KEYS) == _lib.SURF_NQ
    assert SURF_KEYS == SR.SURF_KEYS


def test_entries_reject_bad_arguments_without_a_gpu():
    from hands_amd import _lib
    L = _lib.lib()
    call = lambda *a: L.hands_mesh_closest_f32(*a, None)
    p = 16                                               # never dereferenced: every call below is refused
    for B, P, V, F in ((0, 1, 3, 1), (1, 0, 3, 1), (1, 1, 0, 1), (-1, 1, 3, 1), (1, 1, 3, -1), (1, 1, _lib.MESH_MAX_V + 1, 1),
                       (1, 1, 3, _lib.SURF_MAX_F + 1)):
        assert call(p, p, p, None, p, p, p, B, P, V, F) == 10001, (B, P, V, F)
    assert call(None, p, p, None, p, None, None, 1, 1, 3, 1) == 10001
    assert call(p, None, p, None, p, None, None, 1, 1, 3, 1) == 10001
    assert call(p, p, None, None, p, None, None, 1, 1, 3, 1) == 10001
    assert call(p, p, p, None, None, p, p, 1, 1, 3, 1) == 10001
    fin, fout = _lib.MeshEvalIn(*[16] * 11), _lib.SurfEvalOut(*[16] * 12)
    ev = lambda i, fr, fl, Fr, Fl, o, B, V: L.hands_eval_surface_metrics_f32(i, fr, fl, Fr, Fl, o, B, V, None)
    for B, V, Fr, Fl in ((0, 778, 1, 1), (1, 0, 1, 1), (1, 1025, 1, 1), (1, 778, -1, 1), (1, 778, 1, _lib.SURF_MAX_F + 1)):
        assert ev(ctypes.byref(fin), p, p, Fr, Fl, ctypes.byref(fout), B, V) == 10001, (B, V, Fr, Fl)
    assert ev(None, p, p, 1, 1, ctypes.byref(fout), 1, 778) == 10001 and ev(ctypes.byref(fin), p, p, 1, 1, None, 1, 778) == 10001
    assert ev(ctypes.byref(fin), None, p, 1, 1, ctypes.byref(fout), 1, 778) == 10001
    a = [16] * 12
    a[11] = None
    assert ev(ctypes.byref(fin), p, p, 1, 1, ctypes.byref(_lib.SurfEvalOut(*a)), 1, 778) == 10001
    a = [16] * 11
    a[3] = None
    assert ev(ctypes.byref(_lib.MeshEvalIn(*a)), p, p, 1, 1, ctypes.byref(fout), 1, 778) == 10001


def test_wrapper_metric_dict_is_still_the_reference_names(recipe_model):
    import inspect
    from hands_amd.wrapper import HandsWrapper
    assert HandsWrapper(model=recipe_model).metric_dict == ["mrrpe.rl", "mpjpe.ra", "mpjpe.pa.ra", "pix_err"]
    assert '"surface" in self.metric_dict' in inspect.getsource(HandsWrapper.forward)


# ---- compile-only resource guard ------------------------------------------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mesh_distance_kernel_resources(tmp_path):
    """csrc/mesh_distance.hip as the Makefile builds it: no kernel spills or uses scratch, static LDS stays under 64 KB (no
    attribute call in front of a launch)."""
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "hands_amd", "csrc", "mesh_distance.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)[1:]
    field = lambda b, pat: int(re.search(pat, b).group(1))
    names = [b.split()[0] for b in blocks]
    assert len(blocks) == 3 and any("mesh_closest_kernel" in n for n in names) and any("surface_metrics_kernel" in n for n in names)
    for b in blocks:
        assert field(b, r"ScratchSize \[bytes/lane\]: (\d+)") == 0 and field(b, r"VGPRs Spill: (\d+)") == 0, b.split()[0]
        assert field(b, r"SGPRs Spill: (\d+)") == 0, b.split()[0]
        assert field(b, r"LDS Size \[bytes/block\]: (\d+)") <= 65536, b.split()[0]
