"""The fp64 restatement of the signed distance (tests/penetration_ref.py) against closed forms, hands_amd.seal_mesh and
hands_amd.penetration_grid on the host, and the public surface of the penetration functions.  No device is needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import penetration_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = {"tetrahedron": PR.tetrahedron, "cube": PR.cube, "octahedron": PR.octahedron, "sphere": PR.uv_sphere}


# ---- 1. analytic pins of the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(MESHES))
def test_winding_number_of_closed_meshes(name):
    v, f = MESHES[name]()
    assert len(PR.seal_mesh(f, len(v))[1]) == 0                                # closed to begin with
    assert all(sorted(u) == sorted([u[0], u[0][::-1]]) and len(u) == 2 for u in PR.edge_uses(f).values())
    inside = np.array([[0.0, 0, 0], [0.1, -0.05, 0.02]])
    far = np.array([[5.0, 0, 0], [-3.0, 4, 2], [0.0, 0, 1.5]])
    np.testing.assert_allclose(PR.winding_number(inside, v, f), 1.0, atol=1e-12)
    np.testing.assert_allclose(PR.winding_number(far, v, f), 0.0, atol=1e-12)
    np.testing.assert_allclose(PR.winding_number(inside, v, f[:, ::-1]), -1.0, atol=1e-12)
    sdf, w, idx = PR.signed_distance(inside[None], v[None], f[:, ::-1])        # reversed faces: still inside
    assert (sdf < 0).all() and (w < -0.99).all() and (idx >= 0).all()


def test_tetrahedron_counts_and_a_single_face():
    v, f = PR.tetrahedron()
    assert v.shape == (4, 3) and f.shape == (4, 3)
    # one regular face, counter-clockwise about +z, seen from its axis: a spherical triangle with three equal sides t, whose
    # area is L'Huilier's 4 atan sqrt(tan(3t/4) tan(t/4)^3); the side the normal points to is the outside
    tri = np.array([[1.0, 0, 0], [-0.5, np.sqrt(0.75), 0], [-0.5, -np.sqrt(0.75), 0]])
    h = 0.7
    a, b = tri[0] - [0, 0, h], tri[1] - [0, 0, h]
    t = np.arccos(a @ b / (a @ a))
    omega = 4 * np.arctan(np.sqrt(np.tan(0.75 * t) * np.tan(0.25 * t) ** 3))
    w = PR.winding_number(np.array([[0, 0, h], [0, 0, -h]]), tri, [[0, 1, 2]])
    np.testing.assert_allclose(w, [-omega / (4 * np.pi), omega / (4 * np.pi)], atol=1e-12)
    # in the plane of the face: half the sphere inside the triangle, nothing outside it
    np.testing.assert_allclose(np.abs(PR.winding_number(np.array([[0.1, 0.1, 0], [3.0, 0, 0]]), tri, [[0, 1, 2]])), [0.5, 0.0], atol=1e-12)


def test_terms_that_count_as_zero():
    v, f = PR.cube()
    w = PR.winding_number(v[:3], v, f)                                         # queries ON vertices: the faces at the vertex add 0
    assert np.isfinite(w).all() and (np.abs(w) < 0.5).all()
    np.testing.assert_allclose(w, 0.125, atol=1e-12)                           # a cube's corner sees an eighth of the sphere
    extra = np.concatenate([f, [[0, 0, 0]], [[1, 1, 5]], [[0, 1, 8]], [[-1, 2, 3]]])     # a point, a segment, two out of range
    q = np.array([[0.2, 0.1, -0.3], [2.0, 2, 2]])
    np.testing.assert_allclose(PR.winding_number(q, v, extra), PR.winding_number(q, v, f), atol=1e-15)
    sdf, w, idx = PR.signed_distance(q[None], v[None], np.array([[0, 1, 8]]))  # no usable face
    assert np.isposinf(sdf).all() and (w == 0).all() and (idx == -1).all()
    sdf, w, idx = PR.signed_distance(np.array([[[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0]]] * 2), np.stack([v, v]), f, valid=[1, 0])
    assert np.isnan(sdf[0, :2]).all() and np.isnan(w[0, :2]).all() and (idx[0, :2] == -1).all() and sdf[0, 2] == -1.0
    assert np.isnan(sdf[1]).all() and np.isnan(w[1]).all() and (idx[1] == -1).all()


def test_sdf_against_a_sphere_mesh_has_the_right_sign():
    v, f = PR.uv_sphere(12, 8, r=0.05)
    rng = np.random.RandomState(0)
    d = rng.randn(200, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    radius = 0.05 * np.r_[rng.uniform(0.0, 0.85, 100), rng.uniform(1.05, 3.0, 100)]     # the mesh lies between 0.87 r and r
    sdf, w, _ = PR.signed_distance((d * radius[:, None])[None], v[None], f)
    assert (sdf[0, :100] < 0).all() and (sdf[0, 100:] > 0).all()
    np.testing.assert_allclose(w[0], np.r_[np.ones(100), np.zeros(100)], atol=1e-12)
    assert (np.abs(sdf[0]) <= np.abs(radius - 0.05) + 0.05 * 0.14).all()       # within the chord error of the sphere's own distance


# ---- 2. seal_mesh ----------------------------------------------------------------------------------------------------------
def _closed_and_consistent(faces):
    return all(len(u) == 2 and u[0] == u[1][::-1] for u in PR.edge_uses(faces).values())


@pytest.mark.parametrize("as_tensor", [False, True])
def test_seal_mesh_closes_an_open_cube(as_tensor):
    from hands_amd import apply_seal, seal_mesh
    v, f = PR.cube()
    open_ = f[:10]                                                             # without the +z side
    assert not _closed_and_consistent(open_)
    arg = torch.from_numpy(open_) if as_tensor else open_
    sealed, loops = seal_mesh(arg, 8)
    assert sealed.dtype == torch.int32 and sealed.shape == (14, 3) and len(loops) == 1 and loops[0].dtype == torch.int64
    assert torch.equal(sealed[:10], torch.from_numpy(open_).int()) and sorted(loops[0].tolist()) == [1, 3, 5, 7]
    assert (sealed[10:, 2] == 8).all() and _closed_and_consistent(sealed.numpy())
    ref_faces, ref_loops = PR.seal_mesh(open_, 8)
    assert np.array_equal(sealed.numpy(), ref_faces) and [l.tolist() for l in loops] == ref_loops
    again = seal_mesh(arg, 8)
    assert again[0] is sealed and again[1] is loops                            # kept per face-list object
    vs = apply_seal(torch.from_numpy(np.stack([v, 2 * v + 1])), loops)
    assert vs.shape == (2, 9, 3) and torch.equal(vs[:, :8], torch.from_numpy(np.stack([v, 2 * v + 1])))
    assert vs[0, 8].tolist() == [0.0, 0.0, 1.0] and vs[1, 8].tolist() == [1.0, 1.0, 3.0]
    np.testing.assert_array_equal(PR.apply_seal(np.stack([v, 2 * v + 1]), ref_loops), vs.numpy())
    np.testing.assert_allclose(PR.winding_number(np.zeros((1, 3)), vs[0].numpy(), sealed.numpy()), 1.0, atol=1e-12)
    # an inward-oriented open cube is sealed with inward fans
    sealed_in, _ = seal_mesh(open_[:, ::-1].copy(), 8)
    assert _closed_and_consistent(sealed_in.numpy())
    np.testing.assert_allclose(PR.winding_number(np.zeros((1, 3)), vs[0].numpy(), sealed_in.numpy()), -1.0, atol=1e-12)


def test_seal_mesh_two_holes_closed_mesh_and_errors():
    from hands_amd import apply_seal, seal_mesh, synthetic_mano_asset
    v, f = PR.cube()
    two = f[4:]                                                                # without the -x and the +x side: a tube
    sealed, loops = seal_mesh(two, 8)
    assert len(loops) == 2 and sealed.shape == (8 + 8, 3) and _closed_and_consistent(sealed.numpy())
    assert [sorted(l.tolist()) for l in loops] == [[0, 1, 2, 3], [4, 5, 6, 7]] and loops[0][0] == 0 and loops[1][0] == 4
    np.testing.assert_allclose(PR.winding_number(np.zeros((1, 3)), PR.apply_seal(v[None], [l.tolist() for l in loops])[0], sealed.numpy()),
                               1.0, atol=1e-12)
    assert set(sealed[8:12, 2].tolist()) == {8} and set(sealed[12:, 2].tolist()) == {9}
    assert apply_seal(torch.from_numpy(v)[None], loops).shape == (1, 10, 3)
    closed, none = seal_mesh(f, 8)
    assert len(none) == 0 and torch.equal(closed, torch.from_numpy(f).int())
    x = torch.from_numpy(v)[None]
    assert apply_seal(x, none) is x
    for bad, why in ((synthetic_mano_asset(True).faces, "random faces"),
                     (np.concatenate([f, [[0, 1, 7]]]), "an edge of three faces"),
                     (np.array([[0, 1, 2], [0, 3, 4]]), "two boundaries through one vertex"),
                     (np.array([[0, 1, 8]]), "out of range"), (np.array([[0, 1, 1]]), "repeated index")):
        with pytest.raises(ValueError):
            seal_mesh(bad, 8 if len(bad) < 100 else 778)
        with pytest.raises(ValueError):
            PR.seal_mesh(bad, 8 if len(bad) < 100 else 778)


# ---- 3. the grid -----------------------------------------------------------------------------------------------------------
def test_penetration_grid():
    from hands_amd import penetration_grid
    v, _ = PR.cube()
    v_r = np.float32(np.stack([v, v, 0.5 * v]))                                # [-1,1]^3, the same, [-.5,.5]^3
    v_l = np.float32(np.stack([v + [1.0, 0.5, 0.0], v + [2.0, 0, 0], v + [3.0, 0, 0]]))   # overlap, touching, apart
    pts, cell = penetration_grid(torch.from_numpy(v_r), torch.from_numpy(v_l), 4)
    assert pts.shape == (3, 64, 3) and cell.shape == (3,) and pts.dtype == cell.dtype == torch.float32
    # sample 0: the box [0,1] x [-.5,1] x [-1,1]
    assert cell.tolist() == [0.25 * 0.375 * 0.5, 0.0, 0.0]
    grid = pts[0].reshape(4, 4, 4, 3)
    assert grid[:, 0, 0, 0].tolist() == [0.125, 0.375, 0.625, 0.875]
    assert grid[0, :, 0, 1].tolist() == [-0.5 + 0.375 * (i + 0.5) for i in range(4)]
    assert grid[0, 0, :, 2].tolist() == [-0.75, -0.25, 0.25, 0.75]
    assert bool((grid[:, 2, 1, 0] == grid[:, 0, 0, 0]).all()) and bool((grid[3, 1, :, 2] == grid[0, 0, :, 2]).all())
    rp, rc = PR.penetration_grid(v_r, v_l, 4)
    np.testing.assert_allclose(pts.numpy(), rp, atol=1e-6)
    np.testing.assert_allclose(cell.numpy(), rc, atol=1e-7)
    assert PR.lens_volume(1.0, 1.0, 2.5) == 0 and abs(PR.lens_volume(1.0, 1.0, 0.0) - 4 / 3 * np.pi) < 1e-12
    assert abs(PR.lens_volume(1.0, 1.0, 1.0) - 5 * np.pi / 12) < 1e-12


# ---- 4. the public surface -------------------------------------------------------------------------------------------------
NAMES = ("signed_distance_to_mesh", "interhand_penetration", "penetration_grid", "intersection_volume", "seal_mesh", "apply_seal",
         "evaluate_penetration_metrics")


def test_exports_header_and_signature():
    import hands_amd
    from hands_amd import _lib
    for n in NAMES:
        assert n in hands_amd.__all__ and callable(getattr(hands_amd, n)), n
    assert hands_amd.evaluate_penetration_metrics is hands_amd.metrics.evaluate_penetration_metrics
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"^int\s+hands_mesh_signed_f32\s*\(", header, flags=re.M)
    assert len(_lib.SIGNATURES["hands_mesh_signed_f32"]) == 12
    assert f"#define HANDS_SIGNED_CHUNK {_lib.SIGNED_CHUNK}" in header


def test_no_cpu_fallback():
    import hands_amd
    v, f = PR.uv_sphere(12, 8, 0.05)
    vt = torch.from_numpy(np.float32(v))[None]
    d = {"mano.v3d.cam.r": vt, "mano.v3d.cam.l": vt + 0.05, "is_valid": torch.ones(1), "right_valid": torch.ones(1), "left_valid": torch.ones(1)}
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.signed_distance_to_mesh(vt, vt, f)
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.interhand_penetration(d, faces=(f, f))
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.intersection_volume(d, faces=(f, f), G=4)
    with pytest.raises(RuntimeError, match="HIP device"):
        hands_amd.evaluate_penetration_metrics(d, d, faces=(f, f))
    with pytest.raises(ValueError):
        hands_amd.intersection_volume(d, faces=(f, f), G=33)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_mesh_signed_kernel_resources(tmp_path):
    """csrc/mesh_signed.hip as the Makefile builds it: one kernel, no scratch (atan2f inlined, nothing spilled), the static LDS
    of the unsigned primitive and registers for the four waves per SIMD that LDS allows."""
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "hands_amd", "csrc", "mesh_signed.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)[1:]
    field = lambda b, pat: int(re.search(pat, b).group(1))
    assert len(blocks) == 1 and "mesh_signed_kernel" in blocks[0].split()[0]
    b = blocks[0]
    assert field(b, r"ScratchSize \[bytes/lane\]: (\d+)") == 0 and field(b, r"VGPRs Spill: (\d+)") == 0
    assert field(b, r"SGPRs Spill: (\d+)") == 0 and field(b, r"LDS Size \[bytes/block\]: (\d+)") == 36864
    assert field(b, r" VGPRs: (\d+)") <= 128


def test_wrapper_has_the_seal_switch():
    from hands_amd.wrapper import HandsWrapper
    import inspect
    assert "penetration_seal = True" in inspect.getsource(HandsWrapper.__init__)
