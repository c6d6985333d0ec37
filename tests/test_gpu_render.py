"""GPU tests of the soft-silhouette rasteriser (csrc/render.hip, hands_amd/render.py) against the fp64 restatement of its
semantics (tests/render_ref.py).  pytorch3d, which the reference delegates to, is absent: nothing here is pinned to a
reference fixture ("parity unpinned by necessity").

Tolerances.  The restatement itself was run in float32 against float64 on the 36 structured inputs below (2 meshes x 3 sizes
x 6 poses, CPU).  Away from the algorithm's own discontinuities the largest difference of the mask was 2.8e-5 (1.1e-5 .. 2.8e-5
per input): the steepest slope of the sigmoid is 1 / (4 sigma) = 25 000 per squared NDC unit and a float32 vertex position is
good to 6e-8.  Two kinds of pixel differ by more, in any float32 implementation: *tie pixels* (more than 10 candidates, 10th
and 11th depth closer than 1e-6 m; excluded, at most 0.5 % of an input's touched pixels) and pixels at a discontinuity that
the tie rule does not name -- a gap of 1.4e-6 m just above the tie threshold (5.1e-4), an edge-on face whose extrapolated
depth crosses the pz >= 0 cut (9.3e-4; float64 says -0, float32 +4e-4).  The largest float32-vs-float64 difference over all
non-tie pixels was 9.4e-4.  Hence, with the factor 4 for a different order of the arithmetic and another expf:
    MASK_TOL      = 4 x 9.4e-4 -> 3.8e-3   every non-tie pixel
    MASK_TOL_BULK = 4 x 2.8e-5 -> 1.1e-4   all but at most 0.5 % of the touched pixels (the cap of the tie pixels)
S = 76 (added for the partial tiles: 2 x 32 + 12 pixels wide, 9 x 8 + 4 high) was checked in the same way, on both meshes
and six poses: 3.7e-5 off the ties.
The pose seeds were chosen on the restatement alone so that every input respects the tie cap (seed 4 at S = 64 gives an
input with 0.7 % tie pixels); the test checks the cap before it looks at the kernel's output.
"""
import functools

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu

MASK_TOL = 3.8e-3
MASK_TOL_BULK = 1.1e-4
CAP = 0.005                 # excluded pixels per input, as a share of its touched pixels
TIE_GAP = 1e-6              # metres
POSE_SEED = {64: 1, 76: 1, 224: 224, 256: 256}
MESHES = {"ellipsoid": R.ellipsoid_mesh, "mano_sized": R.mano_sized_mesh}


@functools.lru_cache(maxsize=None)
def _mesh(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def _case(name, S):
    v, f = _mesh(name)
    V, K = R.poses(v, S, 6, seed=POSE_SEED[S])
    return V, f, K, [R.render(V[i], f, K[i], S) for i in range(V.shape[0])]


def _gpu(V, f, K, S, **kw):
    import hands_amd
    dev = torch.device("cuda:0")
    out = hands_amd.rasterize(torch.from_numpy(np.ascontiguousarray(V)).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev),
                              torch.from_numpy(np.ascontiguousarray(K)).to(dev), S, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare_mask(tag, got, ref):
    touched = ref["n_cand"] > 0
    tie = ref["tie_gap"] < TIE_GAP
    n_touched = int(touched.sum())
    assert tie.sum() <= CAP * n_touched, (tag, int(tie.sum()), n_touched)           # a property of the input
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0, tag
    assert (got[~touched] == 0.0).all(), tag                                         # exactly zero where nothing is in reach
    d = np.abs(got.astype(np.float64) - ref["mask"])
    d[tie] = 0.0
    n_bulk = int((d > MASK_TOL_BULK).sum())
    print(f"{tag}: touched {n_touched}, tie pixels {int(tie.sum())}, max |mask - ref| off ties {d.max():.3e}, "
          f"pixels over {MASK_TOL_BULK:g}: {n_bulk}")
    assert d.max() <= MASK_TOL, (tag, float(d.max()), np.unravel_index(d.argmax(), d.shape))
    assert n_bulk <= CAP * n_touched, (tag, n_bulk, n_touched)


def _compare_zbuf(tag, got_idx, got_z, ref):
    touched = ref["n_cand"] > 0
    unsure = (ref["z_gap"] < TIE_GAP) | (ref["win_wmin"] < 1e-5)      # two depths within 1e-6 m, or the winner barely contains the pixel
    unsure &= ref["face_idx"] >= 0
    n_touched = int(touched.sum())
    assert unsure.sum() <= CAP * n_touched, (tag, int(unsure.sum()), n_touched)
    mism = (got_idx != ref["face_idx"]) & ~unsure
    zerr = np.where(mism | unsure, 0.0, np.abs(got_z.astype(np.float64) - ref["zbuf"]))
    print(f"{tag}: unsure {int(unsure.sum())}, face_idx mismatches off unsure {int(mism.sum())}, max |zbuf - ref| {zerr.max():.3e}")
    assert mism.sum() == 0, (tag, int(mism.sum()), list(zip(*np.nonzero(mism)))[:5])
    assert zerr.max() <= 1e-6, (tag, float(zerr.max()))
    assert (got_z[got_idx < 0] == 0.0).all() and (got_idx[~touched] == -1).all(), tag


@pytest.mark.parametrize("S", [64, 76, 224, 256])      # 76: partial tiles, 2 x 32 + 12 wide and 9 x 8 + 4 high
@pytest.mark.parametrize("name", ["ellipsoid", "mano_sized"])
def test_mask_and_zbuffer_match_the_fp64_restatement(name, S):
    V, f, K, refs = _case(name, S)
    assert V.shape[0] >= 6
    got = _gpu(V, f, K, S)
    assert got["mask"].shape == (V.shape[0], 1, S, S) and got["face_idx"].dtype == np.int32
    for i, ref in enumerate(refs):
        _compare_mask(f"{name} S={S} pose {i}", got["mask"][i, 0], ref)
        _compare_zbuf(f"{name} S={S} pose {i}", got["face_idx"][i], got["zbuf"][i], ref)
    # the last hand is partly out of frame, the others are not cut by more than a rim
    assert (refs[-1]["n_cand"][:, -1] > 0).any()


def test_inputs_exercise_the_top10_rule():
    """Without this a kernel that ignores faces_per_pixel would pass: the inputs contain pixels with more than 10 candidates,
    and blending ALL candidates differs visibly from blending the nearest 10."""
    for name in MESHES:
        V, f, K, refs = _case(name, 224)
        n_over = sum(int((r["n_cand"] > 10).sum()) for r in refs)
        worst = max(float(np.abs(r["mask_all"] - r["mask"]).max()) for r in refs)
        print(f"{name}: {n_over} pixels with more than 10 candidates, all-vs-top10 up to {worst:.3f}")
        assert n_over > 100 and worst > 0.01
        # and the kernel is on the top-10 side of that difference, where it is largest
        got = _gpu(V, f, K, 224, return_zbuf=False)["mask"][:, 0]
        for i, r in enumerate(refs):
            gap = np.abs(r["mask_all"] - r["mask"])
            gap[r["tie_gap"] < TIE_GAP] = 0.0
            if gap.max() > 0.01:
                p = np.unravel_index(gap.argmax(), gap.shape)
                assert abs(got[i][p] - r["mask"][p]) <= MASK_TOL < abs(got[i][p] - r["mask_all"][p]), (name, i, p)
    # faces_per_pixel is honoured below 10 too
    V, f, K, _ = _case("ellipsoid", 64)
    ref3 = R.render(V[2], f, K[2], 64, faces_per_pixel=3)
    got3 = _gpu(V[2:3], f, K[2:3], 64, return_zbuf=False, faces_per_pixel=3)["mask"][0, 0]
    ok = ~(ref3["tie_gap"] < TIE_GAP)
    assert np.abs(got3 - ref3["mask"])[ok].max() <= MASK_TOL
    assert np.abs(ref3["mask"] - R.render(V[2], f, K[2], 64)["mask"]).max() > 0.01


def test_triangle_soup():
    """The random faces of the synthetic MANO asset: triangles that span the whole blob, hundreds of layers deep (up to 426
    candidates at a pixel), every tile's face list overflows its LDS share and is processed in chunks.  The restatement's own
    float32-vs-float64 run stays inside the cap on it (12 and 20 tie pixels of 50 176, largest difference off them 2.7e-6), so
    the comparison is the same as on the structured meshes."""
    import hands_amd
    A = hands_amd.synthetic_mano_asset(True)
    f = A.faces.astype(np.int32)
    V, K = R.poses(A.v_template, 224, 2, seed=7)
    got = _gpu(V, f, K, 224)
    for i in range(2):
        ref = R.render(V[i], f, K[i], 224)
        assert ref["n_cand"].max() > 384                   # more candidates at one pixel than a chunk of the list holds
        _compare_mask(f"soup pose {i}", got["mask"][i, 0], ref)
        _compare_zbuf(f"soup pose {i}", got["face_idx"][i], got["zbuf"][i], ref)


def test_batch_independence_and_determinism():
    import hands_amd
    v, f = _mesh("mano_sized")
    V, K = R.poses(v, 224, 37, seed=11)
    V[5, :, 0] += 3.0                                      # this hand is fully outside the frame (3 m to the right)
    a = _gpu(V, f, K, 224)
    b = _gpu(V, f, K, 224)
    for k in ("mask", "face_idx", "zbuf"):
        assert np.array_equal(a[k], b[k]), k               # two runs
    dev = torch.device("cuda:0")
    Vd, fd, Kd = torch.from_numpy(V).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(K).to(dev)
    singles = [hands_amd.rasterize(Vd[i:i + 1], fd, Kd[i:i + 1], 224) for i in range(37)]
    torch.cuda.synchronize()
    for k in ("mask", "face_idx", "zbuf"):
        one = torch.cat([s[k] for s in singles]).cpu().numpy()
        assert np.array_equal(a[k], one), k                # one launch of 37 == 37 launches of one
    assert (a["mask"][5] == 0).all() and (a["face_idx"][5] == -1).all() and (a["zbuf"][5] == 0).all()
    assert all(a["mask"][i].max() > 0.99 for i in range(37) if i != 5)


def test_left_and_right_use_their_own_faces():
    import hands_amd
    v, f = _mesh("mano_sized")
    f_half = np.ascontiguousarray(f[: f.shape[0] // 2])
    V, K = R.poses(v, 224, 3, seed=5)
    dev = torch.device("cuda:0")
    Vd, Kd = torch.from_numpy(V).to(dev), torch.from_numpy(K).to(dev)
    r = hands_amd.MANORenderer(faces=(f, f_half))
    pred, meta = {"mano.v3d.cam.r": Vd, "mano.v3d.cam.l": Vd}, {"intrinsics": Kd}
    right, left = r(pred, meta, is_right=True), r(pred, meta, is_right=False)
    plain = r({"v3d.cam.r": Vd, "v3d.cam.l": Vd}, meta, is_right=False)      # the un-prefixed dictionary of one MANO head
    assert torch.equal(right["mask"], hands_amd.rasterize(Vd, torch.from_numpy(f).to(dev), Kd, 224)["mask"])
    assert torch.equal(left["mask"], hands_amd.rasterize(Vd, torch.from_numpy(f_half).to(dev), Kd, 224)["mask"])
    assert torch.equal(plain["mask"], left["mask"]) and not torch.equal(right["mask"], left["mask"])
    assert right["image"].shape == (3, 3, 224, 224) and bool((right["image"] == 1).all())
    assert right["mask"].shape == (3, 1, 224, 224) and not right["mask"].requires_grad
    assert len(r._dev_faces) == 2                          # uploaded once per device and side


def test_error_paths_return_einval_and_do_not_launch():
    from hands_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    S, big_n = 32, 4000                                    # 4000 vertices = 48 000 bytes: does not fit beside the face list
    verts = torch.zeros(1, big_n, 3, device=dev)
    verts[..., 2] = 0.5
    faces = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    K = torch.eye(3, device=dev)[None].contiguous()
    mask = torch.full((1, S, S), -7.0, device=dev)
    call = lambda n, fpp, sigma=1e-5: L.hands_render_silhouette_f32(
        verts.data_ptr(), 3 * big_n, n, faces.data_ptr(), 1, K.data_ptr(), 1, S, sigma, 1e-4, fpp, mask.data_ptr(), None, None,
        torch.cuda.current_stream(dev).cuda_stream)
    assert call(778, 11) == 10001 and call(778, 0) == 10001 and call(big_n, 10) == 10001 and call(778, 10, 0.0) == 10001
    assert L.hands_render_silhouette_f32(None, 3 * 778, 778, faces.data_ptr(), 1, K.data_ptr(), 1, S, 1e-5, 1e-4, 10,
                                         mask.data_ptr(), None, None, None) == 10001
    torch.cuda.synchronize()
    assert bool((mask == -7.0).all())                      # nothing ran
    assert call(3410, 10) == 0                             # the largest vertex block that fits
    torch.cuda.synchronize()
    assert bool((mask == 0.0).all())                       # the degenerate face covers nothing, every pixel was written
    with pytest.raises(RuntimeError, match="hands_render_silhouette_f32"):
        import hands_amd
        hands_amd.rasterize(verts[:, :778].contiguous(), faces, K, S, faces_per_pixel=11)


def test_end_to_end_masks_of_a_hands_light_forward():
    import hands_amd
    dev = torch.device("cuda:0")
    model = hands_amd.apply_recipe(hands_amd.HandsLight()).to(dev)
    inputs, meta = hands_amd.synthetic_inputs(3, 0)
    inputs, meta = {k: v.to(dev) for k, v in inputs.items()}, {k: v.to(dev) for k, v in meta.items()}
    pred = model(inputs, meta)
    renderer = hands_amd.MANORenderer(hands_amd.DEFAULT_ARGS)
    out = renderer.render_masks(pred, meta)
    torch.cuda.synchronize()
    assert list(out.keys()) == ["render.r", "render.l"]
    for side, is_right in (("r", True), ("l", False)):
        m = out[f"render.{side}"]
        assert m.shape == (3, 1, 224, 224) and m.dtype == torch.float32
        assert bool(torch.isfinite(m).all()) and float(m.min()) >= 0.0 and float(m.max()) <= 1.0
        faces = torch.from_numpy(hands_amd.synthetic_mano_asset(is_right).faces.astype(np.int32)).to(dev)
        direct = hands_amd.rasterize(pred[f"mano.v3d.cam.{side}"], faces, meta["intrinsics"], 224)
        assert torch.equal(m, direct["mask"])
        assert float(m.max()) > 0.5                        # the synthetic hand is in front of the camera and in the frame
    pred.merge(out)                                        # model.py:420
    assert "render.r" in pred and len(pred) == 24


def test_renderer_is_capturable_in_one_graph():
    import hands_amd
    v, f = _mesh("mano_sized")
    V, K = R.poses(v, 224, 4, seed=3)
    dev = torch.device("cuda:0")
    Vd, fd, Kd = torch.from_numpy(V).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(K).to(dev)
    eager = hands_amd.rasterize(Vd, fd, Kd, 224)           # also warms the code object up before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                              # one stream, no parallel branches
        captured = hands_amd.rasterize(Vd, fd, Kd, 224)
    for k in captured:
        captured[k].fill_(-3)
    g.replay()
    torch.cuda.synchronize()
    for k in ("mask", "face_idx", "zbuf"):
        assert torch.equal(captured[k], eager[k]), k
    # the graph reads its inputs at replay: new vertices, same graph
    V2, _ = R.poses(v, 224, 4, seed=4)
    Vd.copy_(torch.from_numpy(V2).to(dev))
    g.replay()
    torch.cuda.synchronize()
    again = hands_amd.rasterize(Vd, fd, Kd, 224)
    torch.cuda.synchronize()
    assert torch.equal(captured["mask"], again["mask"]) and not torch.equal(again["mask"], eager["mask"])
