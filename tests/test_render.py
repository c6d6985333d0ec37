"""CPU tests of the soft-silhouette renderer: the fp64 restatement (tests/render_ref.py) on closed-form cases, the host side
of hands_amd.MANORenderer, and the code object's resources.  The kernel itself is tested on the GPU (tests/test_gpu_render.py)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import render_ref as R

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _K(S, f=None):
    f = float(S) if f is None else f
    return np.array([[f, 0, S / 2], [0, f, S / 2], [0, 0, 1]], np.float64)


def _unproject(u, v, z, K):
    return [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]


def test_restatement_one_large_triangle_is_closed_form():
    S = 32
    K = _K(S)
    # image-space triangle (4, 4), (28, 4), (4, 28) at depth 0.5: the pixel (r, c) samples the image point (c + .5, r + .5)
    verts = np.array([_unproject(4, 4, 0.5, K), _unproject(28, 4, 0.5, K), _unproject(4, 28, 0.5, K)])
    out = R.render(verts, np.array([[0, 1, 2]]), K, S)
    # interior pixel (r, c) = (6, 10): nearest edge is y = 4, at 2.5 px = 2.5 * 2 / S NDC units
    d = 2.5 * 2 / S
    assert out["mask"][6, 10] == pytest.approx(1 / (1 + math.exp(-d * d / R.SIGMA)), abs=1e-12)
    assert out["face_idx"][6, 10] == 0 and out["zbuf"][6, 10] == pytest.approx(0.5, abs=1e-8)   # area / (area + 1e-8) of 0.5
    # a pixel 0.05 px inside the edge x = 4 would need a sub-pixel sample; the nearest samples are 0.5 px away:
    d = 0.5 * 2 / S
    assert out["mask"][10, 4] == pytest.approx(1 / (1 + math.exp(-d * d / R.SIGMA)), abs=1e-12)       # inside
    assert out["mask"][10, 3] == pytest.approx(1 / (1 + math.exp(+d * d / R.SIGMA)), abs=1e-12)       # outside
    assert out["face_idx"][10, 3] == -1 and out["zbuf"][10, 3] == 0
    # far pixels: exactly zero, not a candidate
    assert out["mask"][30, 30] == 0.0 and out["n_cand"][30, 30] == 0
    assert out["mask"][10, 1] == 0.0            # 2.5 px outside: d2 = 0.0244 >> blur_radius
    assert (out["mask"] >= 0).all() and (out["mask"] <= 1).all()


def test_restatement_half_pixel_convention():
    S = 16
    K = _K(S, 20.0)
    r, c = 5, 9
    # a vertex projected to (c + 0.5, r + 0.5) lies exactly on the sample point of pixel (r, c): d2 = 0
    verts = np.array([_unproject(c + 0.5, r + 0.5, 0.4, K), _unproject(c + 4.5, r + 0.5, 0.4, K), _unproject(c + 0.5, r + 4.5, 0.4, K)])
    pix, face, pz, dist, wmin, inside = R.candidates(verts, np.array([[0, 1, 2]]), K, S)
    at = pix == r * S + c
    assert at.sum() == 1 and abs(dist[at][0]) < 1e-30 and not inside[at][0]
    assert R.render(verts, np.array([[0, 1, 2]]), K, S)["mask"][r, c] == pytest.approx(0.5, abs=1e-9)
    # the sample grid itself
    assert (2 * c + 1) / S - 1 == pytest.approx(2 * (c + 0.5) / S - 1)


def test_restatement_skips_faces_behind_the_camera_and_degenerate_faces():
    S = 16
    K = _K(S)
    front = [_unproject(3, 3, 0.5, K), _unproject(12, 3, 0.5, K), _unproject(3, 12, 0.5, K)]
    behind = [[-0.1, -0.1, 0.5], [0.1, -0.1, -0.2], [0.0, 0.1, 0.5]]        # one vertex at Z < 0
    sliver = [_unproject(3, 3, 0.3, K), _unproject(8, 8, 0.3, K), _unproject(13, 13, 0.3, K)]   # zero area
    verts = np.array(front + behind + sliver)
    both = R.render(verts, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]]), K, S)
    alone = R.render(verts, np.array([[0, 1, 2]]), K, S)
    assert np.array_equal(both["mask"], alone["mask"]) and alone["mask"].max() > 0.99
    assert R.render(verts, np.array([[3, 4, 5], [6, 7, 8]]), K, S)["mask"].max() == 0.0


def test_restatement_keeps_the_nearest_faces_per_pixel():
    """12 stacked copies of one triangle: faces_per_pixel = 10 drops the two farthest, and the z-buffer holds the nearest."""
    S = 16
    K = _K(S)
    verts, faces = [], []
    for k in range(12):
        z = 0.9 - 0.05 * k                      # later faces are nearer
        verts += [_unproject(3, 3, z, K), _unproject(12, 3, z, K), _unproject(3, 12, z, K)]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    out = R.render(np.array(verts), np.array(faces), K, S)
    assert out["n_cand"][5, 5] == 12 and out["face_idx"][5, 5] == 11 and out["zbuf"][5, 5] == pytest.approx(0.35)
    assert out["tie_gap"][5, 5] == pytest.approx(0.05)
    # on the outside rim every layer contributes the same probability p: top-10 gives 1 - (1-p)^10, all give 1 - (1-p)^12
    p = 1 / (1 + math.exp((0.5 * 2 / S) ** 2 / R.SIGMA))
    assert out["mask"][7, 2] == pytest.approx(1 - (1 - p) ** 10, rel=1e-9)
    assert out["mask_all"][7, 2] == pytest.approx(1 - (1 - p) ** 12, rel=1e-9)


def test_test_meshes_have_the_stated_counts():
    v, f = R.ellipsoid_mesh()
    assert v.shape == (722, 3) and f.shape == (1440, 3)
    v, f = R.mano_sized_mesh()
    assert v.shape == (778, 3) and f.shape == (1538, 3) and f.min() == 0 and f.max() == 777


def test_renderer_constants_are_the_reference_expressions():
    import hands_amd
    from hands_amd import render
    blend_sigma, dist_eps = 1e-5, 1e-6                  # renderer.py:116-117
    assert render.SIGMA == blend_sigma and render.FACES_PER_PIXEL == 10
    assert render.BLUR_RADIUS == math.log(1. / dist_eps - 1.) * blend_sigma        # renderer.py:120
    assert (R.SIGMA, R.BLUR_RADIUS, R.FACES_PER_PIXEL) == (render.SIGMA, render.BLUR_RADIUS, render.FACES_PER_PIXEL)
    r = hands_amd.MANORenderer(faces=(np.zeros((1, 3), np.int64), np.zeros((1, 3), np.int64)))
    assert (r.sigma, r.blur_radius, r.faces_per_pixel, r.img_res) == (render.SIGMA, render.BLUR_RADIUS, 10, 224)
    assert hands_amd.MANORenderer(hands_amd.DEFAULT_ARGS, faces=(np.zeros((1, 3)), np.zeros((1, 3)))).img_res == 224

    class A:
        img_res = 128
    assert hands_amd.MANORenderer(A(), faces=(np.zeros((1, 3)), np.zeros((1, 3)))).img_res == 128
    assert hands_amd.MANORenderer({"img_res": 96}, faces=(np.zeros((1, 3)), np.zeros((1, 3)))).img_res == 96


def test_renderer_is_exported_and_takes_its_faces_from_the_assets():
    import hands_amd
    assert "MANORenderer" in hands_amd.__all__ and hands_amd.MANORenderer is hands_amd.render.MANORenderer
    ar, al = hands_amd.synthetic_mano_asset(True), hands_amd.synthetic_mano_asset(False)
    r = hands_amd.MANORenderer()                        # build_mano_asset (the synthetic stand-in under the tests' opt-in)
    assert r.mano_faces_r.dtype == torch.int32 and r.mano_faces_r.shape == (1538, 3)
    assert np.array_equal(r.mano_faces_r.numpy(), ar.faces) and np.array_equal(r.mano_faces_l.numpy(), al.faces)
    assert not np.array_equal(ar.faces, al.faces)
    r = hands_amd.MANORenderer(mano_assets=(al, ar))    # explicit assets win over the default
    assert np.array_equal(r.mano_faces_r.numpy(), al.faces) and np.array_equal(r.mano_faces_l.numpy(), ar.faces)
    mine = (np.array([[0, 1, 2]]), np.array([[2, 1, 0], [0, 2, 3]]))
    r = hands_amd.MANORenderer(mano_assets=(ar, al), faces=mine)        # explicit faces win over assets
    assert r.mano_faces_r.tolist() == [[0, 1, 2]] and r.mano_faces_l.tolist() == [[2, 1, 0], [0, 2, 3]]
    assert not list(r.parameters())                     # nothing to train: inference only


def test_cpu_tensors_raise():
    import hands_amd
    r = hands_amd.MANORenderer()
    verts, K = torch.zeros(1, 778, 3), torch.eye(3)[None]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r({"mano.v3d.cam.r": verts}, {"intrinsics": K})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.render_masks({"mano.v3d.cam.r": verts, "mano.v3d.cam.l": verts}, {"intrinsics": K})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hands_amd.rasterize(verts, r.mano_faces_r, K, 224)
    with pytest.raises(KeyError):
        r({"mano.vertices.r": verts}, {"intrinsics": K})


def test_render_seg_loss_switch_still_raises_in_the_models():
    import hands_amd
    with pytest.raises(NotImplementedError):
        hands_amd.HandsLight(args=hands_amd.hands_light._Args(hands_amd.DEFAULT_ARGS, use_render_seg_loss=True))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_render_kernel_keeps_its_top_k_in_registers(tmp_path):
    """The per-pixel top-10 arrays must stay in VGPRs (a runtime-indexed register array goes to scratch), and two workgroups
    must fit in the 160 KiB of LDS of a CU beside the dynamic vertex block."""
    src = os.path.join(ROOT, "hands_amd", "csrc", "render.hip")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
                        str(tmp_path / "o.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", p.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", p.stderr)]
    spills = [int(v) for v in re.findall(r"VGPRs Spill: (\d+)", p.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", p.stderr)]
    assert names and any("render_silhouette_kernel" in n for n in names)
    assert len(names) == len(scratch) == len(spills) == len(lds)
    bad = [(n, s, v) for n, s, v in zip(names, scratch, spills) if s or v]
    assert not bad, bad
    # static LDS (the face list) + the dynamic vertex block of a MANO mesh (778 x 3 floats)
    assert all(v + 778 * 12 <= 81920 for v in lds), lds
    # the host wrapper refuses a launch that would ask for more than 64 KiB in all
    text = open(src).read()
    assert "RENDER_MAX_LDS = 64 * 1024" in text and "lds_verts + lds_static > (size_t)RENDER_MAX_LDS" in text


def test_tie_mode_orders_equal_depths_by_face_index():
    """12 congruent fronto-parallel triangles at Z = 1 (tests/raster_scenes.py): their depths are equal in exact arithmetic, and
    bit-equal in the kernel.  The float64 restatement gives them two or three values one ulp (2.2e-16) apart, so its default order among them is
    rounding noise; the tie mode (tie_rel) orders them by face index.  The default mode is unchanged."""
    import raster_scenes as SC
    v, f = SC.tie12()
    K = SC.dyadic_K(64)[0]
    SC.assert_exact_projection(v, K, 64)
    SC.assert_tie_group(v, f, K, 64, np.arange(12))
    pix, face, pz, dist, wmin, ins = R.candidates(v, f, K, 64, blur_radius=SC.BLUR)
    spread = pz.max() - pz.min()
    print(f"distinct depths {np.unique(pz).size}, spread {spread:.3e}")
    assert 2 <= np.unique(pz).size <= 3 and 2.2e-16 <= spread <= 4.5e-16      # equal depths, told apart by the last bit (1 ulp = 2.2e-16)
    kw = dict(sigma=SC.SIGMA, blur_radius=SC.BLUR)
    tie, plain = R.render(v, f, K, 64, tie_rel=SC.TIE_REL, **kw), R.render(v, f, K, 64, **kw)
    full = tie["n_cand"] == 12
    assert int((tie["n_cand"] > 10).sum()) == 466 and full.sum() > 300
    assert (tie["top"][full] == np.arange(10)).all()                          # faces 0..9, in that order
    assert (tie["tie_gap"] == np.inf).all() and (tie["z_gap"] == np.inf).all()    # one depth group: nothing is decided by a gap
    assert (plain["top"][full] != np.arange(10)).any()                        # the default order follows the rounding
    assert (plain["tie_gap"][full] <= 4.5e-16).all()
    assert np.abs(plain["mask"] - tie["mask"]).max() > 1e-3                   # and blends other faces
    assert tie["win_wmin"].min() == pytest.approx(0.0208, abs=1e-4)           # no winner near an edge
    # face_idx: the lowest containing index, whatever the face order
    v2, f2 = SC.tie12(rev=True)
    rev = R.render(v2, f2, K, 64, tie_rel=SC.TIE_REL, **kw)
    tri = lambda r, flip: np.where(r["face_idx"] >= 0, 11 - r["face_idx"] if flip else r["face_idx"], -1)
    covered = tie["face_idx"] >= 0
    assert (tri(rev, True)[covered] >= tri(tie, False)[covered]).all() and (tri(rev, True) != tri(tie, False)).any()
    # distinct depths: the tie mode changes nothing (the existing scenes' reference stays what it was)
    S = 16
    K16 = _K(S)
    verts = np.array([_unproject(*p, 0.9 - 0.05 * k, K16) for k in range(12) for p in ((3, 3), (12, 3), (3, 12))])
    faces = np.arange(36).reshape(12, 3)
    a, b = R.render(verts, faces, K16, S), R.render(verts, faces, K16, S, tie_rel=SC.TIE_REL)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert "top" in a and a["top"][5, 5].tolist() == list(range(11, 1, -1))
