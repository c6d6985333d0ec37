"""CPU tests of the shaded renderer's host side (hands_amd/rend_utils.py) and of the fp64 restatement the GPU tests compare
against (tests/shade_ref.py).  No GPU is needed: the kernels are checked in tests/test_gpu_shaded_render.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import shade_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_public_names_are_exported():
    import hands_amd
    for name in ("Renderer", "denormalize_images", "sideview_transform"):
        assert hasattr(hands_amd, name) and name in hands_amd.__all__, name
    from hands_amd import rend_utils
    assert hands_amd.Renderer is rend_utils.Renderer
    assert hands_amd.Renderer(64).img_res == 64


def test_module_constants_agree_with_the_header():
    from hands_amd import rend_utils, _lib
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    g = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))
    assert rend_utils.SHADE_TILE == (g("HANDS_SHADE_TILE_W"), g("HANDS_SHADE_TILE_H"))
    assert rend_utils.SHADE_LIST_CAP == g("HANDS_SHADE_LIST_CAP")
    assert rend_utils.SHADE_MAX_MESHES == _lib.SHADE_MAX_MESHES == g("HANDS_SHADE_MAX_MESHES")
    L = _lib.lib()                                   # loads without a GPU
    assert L.hands_mesh_workspace_floats(3, 778) == 3 * 778 * rend_utils.WORKSPACE_FLOATS_PER_VERTEX
    import ctypes
    assert ctypes.sizeof(_lib.ShadeMesh) == 56 and ctypes.sizeof(_lib.ShadeScene) == 4 * 56 + 8


def test_cpu_tensors_and_bad_shapes_raise():
    import hands_amd
    r = hands_amd.Renderer(32)
    v = torch.zeros(2, 5, 3)
    v[..., 2] = 0.5
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    K = torch.eye(3).expand(2, 3, 3).contiguous()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_meshes_pose([v], [f], K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.visualize_rend(v, v, K, torch.zeros(2, 3, 32, 32), faces_r=f, faces_l=f)
    bad = [dict(verts=[v[..., :2]], faces=[f], K=K),                                # vertices not (B, N, 3)
           dict(verts=[v, v[:1]], faces=[f, f], K=K),                               # two batch sizes
           dict(verts=[v], faces=[f.reshape(3, 1)], K=K),                           # faces not (F, 3)
           dict(verts=[v], faces=[f, f], K=K),                                      # one mesh, two face lists
           dict(verts=[v] * 5, faces=[f] * 5, K=K),                                 # more than four meshes
           dict(verts=[], faces=[], K=K),
           dict(verts=[v], faces=[f], K=K[:1]),                                     # K for another batch size
           dict(verts=[v], faces=[f], K=K, image=torch.zeros(2, 3, 16, 16)),        # image of another size
           dict(verts=[v], faces=[f], K=K, colors=[(1, 2)]),
           dict(verts=[v], faces=[f], K=K, metallic=[0.1, 0.2]),
           dict(verts=[v], faces=[f], K=K, valid=[torch.ones(3)])]
    for kw in bad:
        with pytest.raises(ValueError):
            r.render_meshes_pose(**kw)
    with pytest.raises(ValueError):
        hands_amd.sideview_transform(torch.zeros(4, 2), 30.0)
    with pytest.raises(ValueError):
        hands_amd.Renderer(0)


def test_face_cache_is_bounded_and_handles_an_empty_face_list(monkeypatch):
    """The table cache keeps the last FACE_CACHE_ENTRIES face lists; a (0, 3) face list gives a table and a non-null buffer."""
    import hands_amd
    r = hands_amd.Renderer(32)
    monkeypatch.setattr(torch.Tensor, "to", lambda self, *a, **k: self)          # stay on the host: no GPU here
    for i in range(r.FACE_CACHE_ENTRIES + 5):
        fd, off, ids, n = r._faces_on("cpu", np.array([[0, 1, 2], [i % 3, 3, 4]], np.int32) + i, 5 + i)
        assert n == 2 and fd.shape == (2, 3) and off.shape == (6 + i,)
    assert len(r._face_cache) == r.FACE_CACHE_ENTRIES
    first = r._faces_on("cpu", np.array([[0, 1, 2], [0, 3, 4]], np.int32) + 20, 25)
    assert r._faces_on("cpu", np.array([[0, 1, 2], [0, 3, 4]], np.int32) + 20, 25)[0] is first[0]        # a hit, by content
    fd, off, ids, n = r._faces_on("cpu", np.zeros((0, 3), np.int64), 7)
    assert n == 0 and fd.numel() == 3 and off.tolist() == [0] * 8 and ids.numel() == 1


def test_restatement_meets_the_known_answer():
    """A fronto-parallel triangle on the optical axis, metallic 0, roughness 1: n = v = l = h = (0, 0, -1), every clamped dot
    product is 1, so F = f0 = 0.04, c_diff = 0.96 c, D = 1 / pi (a = 1), G = (2 / (1 + 1))^2 = 1 and
    colour = 3 ((1 - 0.04) 0.96 c / pi + 0.04 / (4 pi)) + 0.5 c = (2.7648 / pi + 0.5) c + 0.03 / pi."""
    S = 9                                              # odd: pixel (4, 4) samples the principal point (4.5, 4.5)
    K = np.array([[20.0, 0, 4.5], [0, 20.0, 4.5], [0, 0, 1]])
    verts = np.array([[-0.1, -0.1, 0.5], [0.1, -0.1, 0.5], [0.0, 0.15, 0.5]], np.float32)
    slope, const = 3.0 * 0.96 * 0.96 / math.pi + 0.5, 3.0 * 0.04 / (4.0 * math.pi)
    assert abs(slope - 1.38006) < 1e-5 and abs(const - 0.0095493) < 1e-7           # the figures of the specification
    for faces in ([[0, 1, 2]], [[0, 2, 1]]):                                        # both windings: two-sided
        for c in ((0.2, 0.5, 0.7), (100 / 255, 100 / 255, 254 / 255)):
            out = R.render([dict(verts=verts, faces=np.array(faces), color=c, metallic=0.0)], K, S)
            # the barycentrics sum to area / (area + 1e-8), not 1: the depth of a flat face is off by that factor (|area| = 3.95)
            assert out["face_id"][4, 4] == 0 and abs(out["depth"][4, 4] - 0.5) < 0.5 * 1e-8 / 3.9
            want = np.clip(slope * np.array(c) + const, 0, 1)
            assert np.abs(out["rgb"][4, 4] - want).max() < 1e-12, (out["rgb"][4, 4], want)
    assert want[2] == 1.0                              # the blue channel of the hand colour saturates: the clamp is exercised


def test_sideview_transform_closed_forms():
    import hands_amd
    g = torch.Generator().manual_seed(3)
    V = torch.randn(4, 50, 3, generator=g, dtype=torch.float64) * 0.05 + torch.tensor([0.02, -0.01, 0.5], dtype=torch.float64)
    t = torch.tensor([0.03, -0.02, 0.1], dtype=torch.float64)
    T0, T360 = hands_amd.sideview_transform(V, 0.0, t), hands_amd.sideview_transform(V, 360.0, t)
    assert T0.shape == (4, 3, 4) and T0.dtype == torch.float64
    assert (T0 - T360).abs().max() < 1e-12
    assert (T0[:, :, :3] - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12 and (T0[:, :, 3] - t).abs().max() < 1e-12
    # 90 degrees: R_y(-90) maps (x, y, z) to (-z, y, x), about the centroid, then cam_transl
    T90 = hands_amd.sideview_transform(V, 90.0, t)
    c = V.mean(dim=1, keepdim=True)
    d = V - c
    want = torch.stack([-d[..., 2], d[..., 1], d[..., 0]], dim=-1) + c + t
    got = V @ T90[:, :, :3].transpose(1, 2) + T90[:, None, :, 3]
    assert (got - want).abs().max() < 1e-12
    # the restatement's own builder says the same, and an un-batched anchor gives (3, 4)
    for i in range(4):
        assert np.abs(R.sideview_T(V[i].numpy(), 172.5, t.numpy()) - hands_amd.sideview_transform(V[i], 172.5, t).numpy()).max() < 1e-12
    assert hands_amd.sideview_transform(V[0], 45.0).shape == (3, 4)


def test_csr_table_is_ascending_complete_and_gives_radial_normals():
    from hands_amd.rend_utils import build_vertex_face_csr
    verts, faces = R.uv_sphere(12, 16, 0.045, (0.013, -0.007, 0.40))
    assert faces.shape == (352, 3) and verts.shape == (2 + 11 * 16, 3)
    off, ids = build_vertex_face_csr(faces, verts.shape[0])
    assert off.dtype == np.int32 and ids.dtype == np.int32 and off[0] == 0 and off[-1] == ids.size == 3 * faces.shape[0]
    for v in range(verts.shape[0]):
        mine = ids[off[v]:off[v + 1]]
        assert (np.diff(mine) > 0).all()                                            # ascending, no face twice
        assert set(mine.tolist()) == set(np.nonzero((faces == v).any(axis=1))[0].tolist())      # complete
    # a face that names a vertex twice is listed once for it; a face with an index out of range is in no list
    odd = np.array([[0, 0, 1], [1, 2, 7], [2, 1, 0], [-1, 1, 2]], np.int32)
    off, ids = build_vertex_face_csr(odd, 3)
    assert off.tolist() == [0, 2, 4, 5] and ids.tolist() == [0, 2, 0, 2, 2]
    # normals gathered through the table, on the closed sphere: within 15 degrees of the radial direction
    off, ids = build_vertex_face_csr(faces, verts.shape[0])
    P = verts.astype(np.float64)
    cr = np.cross(P[faces[:, 1]] - P[faces[:, 0]], P[faces[:, 2]] - P[faces[:, 0]])
    n = np.stack([cr[ids[off[v]:off[v + 1]]].sum(axis=0) for v in range(P.shape[0])])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    radial = P - np.array([0.013, -0.007, 0.40])
    radial /= np.linalg.norm(radial, axis=1, keepdims=True)
    cosang = (n * radial).sum(axis=1)
    assert cosang.min() > math.cos(math.radians(15.0)), math.degrees(math.acos(cosang.min()))
    assert np.abs(n - R.vertex_normals(P, faces)).max() < 1e-12                     # the restatement sums face by face


def test_background_is_floored_to_eight_bits():
    S = 8
    rng = np.random.RandomState(0)
    img = rng.rand(3, S, S).astype(np.float32)
    img[0, 0, 0], img[1, 0, 0], img[2, 0, 0] = 1.0, 0.0, 254.999 / 255.0
    far = dict(verts=np.array([[5.0, 5.0, 1.0], [5.1, 5.0, 1.0], [5.0, 5.1, 1.0]], np.float32), faces=np.array([[0, 1, 2]]),
               color=(0.5, 0.5, 0.5), metallic=0.1)                                 # out of the frame: nothing is covered
    K = np.array([[10.0, 0, 4], [0, 10.0, 4], [0, 0, 1]])
    out = R.render([far], K, S, image=img, dtype=np.float32)
    assert not out["covered"].any() and (out["face_id"] == -1).all() and (out["depth"] == 0).all()
    want = np.floor(np.float32(255) * np.moveaxis(img, 0, -1)).astype(np.uint8)
    assert np.array_equal(out["image"], want)
    assert out["image"][0, 0].tolist() == [255, 0, 254]                             # floor, not round
    assert (R.render([far], K, S)["image"] == 255).all()                            # no image: white
    # denormalize_images undoes the ImageNet normalisation
    import hands_amd
    x = torch.from_numpy(rng.rand(2, 3, 4, 4).astype(np.float32))
    mean, std = torch.tensor([0.485, 0.456, 0.406]).reshape(1, 3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).reshape(1, 3, 1, 1)
    assert (hands_amd.denormalize_images((x - mean) / std) - x).abs().max() < 1e-6


def test_tie_mode_keeps_equal_depths_with_the_lower_mesh_and_takes_the_callers_table():
    """The same fronto-parallel triangle in three meshes (tests/raster_scenes.py): the tie mode gives every covered pixel to the
    first valid mesh and reports no unsure pixel; the default mode calls the same pixels unsure (gap 0 or rounding).  A mesh may
    carry the caller's CSR table: an empty one gives zero normals, i.e. the n = v fallback."""
    import raster_scenes as SC
    K = SC.dyadic_K(64)[0]
    meshes = [dict(verts=v, faces=f, color=SC.COLORS[m], valid=m > 0) for m, (v, f) in enumerate(SC.same_triangle_meshes(3))]
    for M in meshes:
        SC.assert_exact_projection(M["verts"], K, 64)
        SC.assert_tie_group(M["verts"], M["faces"], K, 64, np.arange(2))
    tie, plain = R.render(meshes, K, 64, tie_rel=SC.TIE_REL), R.render(meshes, K, 64)
    cov = tie["covered"]
    assert cov.sum() == 192 and (tie["face_id"][cov] == 2).all()              # mesh 0 is off: (mesh 1, face 0) = 2 + 0
    assert not tie["unsure"].any() and (tie["gap"][cov] == np.inf).all()
    assert plain["unsure"][cov].all() and (plain["gap"][cov] < 1e-12).all()   # the default cannot judge these pixels
    want = R.render(meshes[1:2], K, 64)
    assert np.array_equal(tie["rgb"], want["rgb"]) and np.array_equal(tie["depth"], want["depth"])
    # distinct depths: the tie mode changes nothing
    verts, faces = R.uv_sphere(6, 8, 0.045, (0.013, -0.007, 0.40))
    Ks = np.array([[165.0, 0, 22], [0, 165.0, 22], [0, 0, 1]])
    one = [dict(verts=verts, faces=faces, color=(0.2, 0.5, 0.7))]
    a, b = R.render(one, Ks, 44), R.render(one, Ks, 44, tie_rel=SC.TIE_REL)
    assert a["covered"].sum() > 100 and all(np.array_equal(a[k], b[k]) for k in a)
    # the caller's table
    from hands_amd.rend_utils import build_vertex_face_csr
    P = verts.astype(np.float64)
    off, ids = build_vertex_face_csr(faces, verts.shape[0])
    assert np.abs(R.vertex_normals_csr(P, faces, off, ids) - R.vertex_normals(P, faces)).max() < 1e-15
    junk = np.concatenate([[-1, faces.shape[0]], ids]).astype(np.int32)        # entries out of range add nothing
    assert np.array_equal(R.vertex_normals_csr(P, faces, off + 2 * (np.arange(off.size) > 0), junk),
                          R.vertex_normals_csr(P, faces, off, ids))
    empty = (np.zeros(verts.shape[0] + 1, np.int32), np.zeros(0, np.int32))
    assert (R.vertex_normals_csr(P, faces, *empty) == 0).all()
    c = R.render([dict(one[0], csr=empty)], Ks, 44)
    assert np.array_equal(c["face_id"], a["face_id"]) and np.abs(c["rgb"] - a["rgb"]).max() > 0.01
    centre = np.unravel_index(np.argmin(np.where(a["covered"], a["depth"], np.inf)), a["depth"].shape)
    assert np.abs(c["rgb"][centre] - a["rgb"][centre]).max() < 0.02           # n = v is the true normal where the sphere faces the eye
    d = R.render([dict(one[0], n_draw=10)], Ks, 44)
    assert 0 < d["covered"].sum() < a["covered"].sum() and d["face_id"].max() < 10
