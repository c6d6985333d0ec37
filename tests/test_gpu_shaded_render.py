"""GPU tests of the shaded renderer (csrc/shade.hip, hands_amd/rend_utils.py) against the fp64 restatement of its semantics
(tests/shade_ref.py).  pyrender, which the reference delegates to, is absent: nothing here is pinned to a reference fixture
("parity unpinned by necessity"); the specification of DESIGN.md section 7 is the definition.

Scenes: two interpenetrating UV spheres (704 faces at S = 44, f = 165 px; 1 824 faces at S = 76, f = 300 px: partial tiles in
both directions), three poses, sphere B invalid in image 1, and a fourth image with both meshes invalid.

Unsure pixels come from the fp64 restatement alone: some face has min |w_i| < 1e-5 there, two covering depths lie within
1e-6 m, or |n.v| < 1e-5 at the winner.  The restatement evaluates the first rule inside each face's pixel box grown by one
pixel, not over the whole image: a pixel on the extension of an edge far outside the face is decided by another barycentric
that is clearly negative and is not at risk, so fewer pixels are excused than a literal reading over all pixels would excuse
(a stricter test).  They are capped at 1 % of an input's covered pixels, asserted before the kernel's output
is looked at (these scenes: 0-1 of 935-1 464 at S = 44, 0-1 of 3 055-4 765 at S = 76, no depth ties).

Off unsure pixels: face_id equal, depth within 1e-6 m, the 8-bit picture within one level, and the float colour within RGB_TOL:
the restatement was run in float32 against float64 on these six inputs (CPU); where both pick the same face, off unsure pixels,
the largest difference of the colour was 1.7e-6, 1.9e-6, 1.2e-5 (S = 44) and 1.4e-6, 9.1e-6, 1.4e-6 (S = 76).  With the factor 4
for another order of the arithmetic and another rsqrt (the rule of tests/test_gpu_render.py):
    RGB_TOL = 4 x 1.165e-5 -> 4.7e-5
"""
import functools

import numpy as np
import pytest
import torch

import shade_ref as R

pytestmark = pytest.mark.gpu

RGB_TOL = 4.7e-5
DEPTH_TOL = 1e-6
CAP = 0.01
COLORS = ((100, 100, 254), (183, 100, 254), (144, 250, 100), (129, 159, 214))
LEVELS = {44: (12, 16, 165.0), 76: (20, 24, 300.0)}
CENTRE_A, CENTRE_B = (0.013, -0.007, 0.40), (-0.021, 0.011, 0.43)
OFFSETS = ((0.0, 0.0, 0.0), (0.004, -0.003, 0.02), (-0.006, 0.005, -0.03))


def _K(S, f):
    return np.array([[f, 0.0, S / 2.0], [0.0, f, S / 2.0], [0.0, 0.0, 1.0]], np.float32)


class Scene:
    """verts: list of (B, N_m, 3); faces: list of (F_m, 3); valid: list of (B,) float arrays; K (B, 3, 3); image (B, 3, S, S)."""

    def __init__(self, S, verts, faces, valid, K, image=None, metallic=0.1):
        self.S, self.verts, self.faces, self.valid, self.K, self.image, self.metallic = S, verts, faces, valid, K, image, metallic
        self.B = verts[0].shape[0]

    def meshes(self, b, T=None):
        return [dict(verts=v[b], faces=f, color=tuple(c / 255.0 for c in COLORS[m]), metallic=self.metallic,
                     valid=bool(self.valid[m][b] != 0)) for m, (v, f) in enumerate(zip(self.verts, self.faces))]

    def ref(self, b, T=None, image=True, tile=None):
        img = self.image[b] if (image and self.image is not None) else None
        return R.render(self.meshes(b), self.K[b], self.S, T=T, image=img, tile=tile)


def _posed(A, Bm, S, f, seed):
    """The three poses (mirrored x for sphere B) and a fourth image, a copy of the first, with both meshes invalid."""
    offs = [np.array(o, np.float32) for o in OFFSETS] + [np.zeros(3, np.float32)]
    vA = np.stack([A[0] + o for o in offs])
    vB = np.stack([Bm[0] + o * np.array([-1, 1, 1], np.float32) for o in offs])
    valid = [np.array([1, 1, 1, 0], np.float32), np.array([1, 0, 1, 0], np.float32)]
    image = np.random.RandomState(seed).rand(4, 3, S, S).astype(np.float32)
    image[:, :, 0, 0] = np.array([1.0, 0.0, 254.999 / 255.0], np.float32)       # the ends of the range, and floor against round
    return Scene(S, [vA, vB], [A[1], Bm[1]], valid, np.stack([_K(S, f)] * 4), image)


@functools.lru_cache(maxsize=None)
def _scene(S):
    n_lat, n_lon, f = LEVELS[S]
    return _posed(R.uv_sphere(n_lat, n_lon, 0.045, CENTRE_A), R.uv_sphere(n_lat, n_lon, 0.040, CENTRE_B), S, f, seed=S)


@functools.lru_cache(maxsize=None)
def _refs(S):
    sc = _scene(S)
    return [sc.ref(b) for b in range(sc.B)]


def _concentric(n_lat, n_lon, radii, centre):
    vs, fs, at = [], [], 0
    for r in radii:
        v, f = R.uv_sphere(n_lat, n_lon, r, centre)
        vs.append(v)
        fs.append(f + at)
        at += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


@functools.lru_cache(maxsize=None)
def _dense_scene():
    """Four meshes of four concentric 352-face spheres each, 5 632 faces in reach of a handful of tiles; every mesh shows."""
    S, f = 44, 165.0
    spec = [(CENTRE_A, (0.045, 0.0445, 0.044, 0.0435)), (CENTRE_B, (0.040, 0.0395, 0.039, 0.0385)),
            ((0.030, 0.021, 0.39), (0.030, 0.0295, 0.029, 0.0285)), ((-0.030, -0.025, 0.40), (0.028, 0.0275, 0.027, 0.0265))]
    meshes = [_concentric(12, 16, radii, c) for c, radii in spec]
    offs = [np.array(o, np.float32) for o in OFFSETS[:2]]
    verts = [np.stack([v + (o if m % 2 == 0 else o * np.array([-1, 1, 1], np.float32)) for o in offs]) for m, (v, _) in enumerate(meshes)]
    valid = [np.ones(2, np.float32) for _ in meshes]
    image = np.random.RandomState(5).rand(2, 3, S, S).astype(np.float32)
    return Scene(S, verts, [fc for _, fc in meshes], valid, np.stack([_K(S, f)] * 2), image)


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _gpu(sc, renderer=None, image=True, M=None, **kw):
    import hands_amd
    r = renderer or hands_amd.Renderer(sc.S)
    M = len(sc.verts) if M is None else M
    out = r.render_meshes_pose([_t(v) for v in sc.verts[:M]], [_t(f) for f in sc.faces[:M]], _t(sc.K),
                               image=_t(sc.image) if image else None, colors=list(COLORS[:M]), metallic=sc.metallic,
                               valid=[_t(v) for v in sc.valid[:M]], return_float=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_cap(tag, ref):
    n_cov, n_unsure = int(ref["covered"].sum()), int((ref["unsure"] & ref["covered"]).sum())
    print(f"{tag}: covered {n_cov}, unsure {n_unsure}, depth ties {int((ref['gap'] == 0).sum())}")
    assert n_unsure <= CAP * n_cov, (tag, n_unsure, n_cov)              # a property of the input


def _compare(tag, got, b, ref, background, rgb_tol=RGB_TOL, cap=True):
    """got: the batch's outputs; ref: the restatement of image b; background (3, S, S) float32 or None."""
    if cap:
        _check_cap(tag, ref)
    rgb, img, depth, fid = got["rgb"][b], got["image"][b], got["depth"][b], got["face_id"][b]
    ok = ~ref["unsure"]
    # every pixel
    assert np.isfinite(rgb).all() and rgb.min() >= 0.0 and rgb.max() <= 1.0 and np.isfinite(depth).all(), tag
    assert ((fid >= 0) == (depth > 0)).all(), tag
    empty = fid < 0
    bg = np.ones((ref["rgb"].shape[0],) * 2 + (3,), np.float32) if background is None else np.moveaxis(background, 0, -1)
    assert np.array_equal(rgb[empty], bg[empty]), tag                                              # bit for bit
    assert np.array_equal(img[empty], np.floor(np.float32(255) * bg).astype(np.uint8)[empty]), tag
    # off the unsure pixels
    mism = (fid != ref["face_id"]) & ok
    derr = np.where(ok, np.abs(depth.astype(np.float64) - ref["depth"]), 0.0)
    cerr = np.where(ok[..., None], np.abs(rgb.astype(np.float64) - ref["rgb"]), 0.0)
    lerr = np.where(ok[..., None], np.abs(img.astype(np.int64) - ref["image"].astype(np.int64)), 0)
    print(f"{tag}: face_id mismatches {int(mism.sum())}, max |depth - ref| {derr.max():.3e}, max |rgb - ref| {cerr.max():.3e}, "
          f"max 8-bit difference {int(lerr.max())}")
    assert mism.sum() == 0, (tag, int(mism.sum()), list(zip(*np.nonzero(mism)))[:5])
    assert derr.max() <= DEPTH_TOL, (tag, float(derr.max()))
    assert cerr.max() <= rgb_tol, (tag, float(cerr.max()), np.unravel_index(cerr.argmax(), cerr.shape))
    assert lerr.max() <= 1, (tag, int(lerr.max()))


@pytest.mark.parametrize("S", [44, 76])
def test_overlay_matches_the_fp64_restatement(S):
    sc, refs = _scene(S), _refs(S)
    assert sum(f.shape[0] for f in sc.faces) == {44: 704, 76: 1824}[S]
    for b, ref in enumerate(refs):
        _check_cap(f"S={S} image {b}", ref)                  # before the kernel runs
    got = _gpu(sc)
    assert got["image"].shape == (4, S, S, 3) and got["image"].dtype == np.uint8 and got["face_id"].dtype == np.int32
    assert got["rgb"].shape == (4, S, S, 3) and got["depth"].shape == (4, S, S)
    for b, ref in enumerate(refs):
        _compare(f"S={S} image {b}", got, b, ref, sc.image[b], cap=False)
    nA = sc.faces[0].shape[0]
    assert (refs[0]["face_id"] >= nA).any() and (refs[0]["face_id"][refs[0]["covered"]] < nA).any()      # both meshes are seen
    assert refs[1]["covered"].any() and (refs[1]["face_id"] < nA).all()                                    # image 1: B is absent
    assert not refs[3]["covered"].any() and (got["face_id"][3] == -1).all() and (got["depth"][3] == 0).all()
    # the plain call returns the 8-bit picture alone
    import hands_amd
    plain = hands_amd.Renderer(S).render_meshes_pose([_t(v) for v in sc.verts], [_t(f) for f in sc.faces], _t(sc.K), image=_t(sc.image),
                                                     colors=list(COLORS[:2]), valid=[_t(v) for v in sc.valid])
    assert plain.dtype == torch.uint8 and np.array_equal(plain.cpu().numpy(), got["image"])


def test_no_background_is_white():
    sc, refs = _scene(44), _refs(44)
    got = _gpu(sc, image=False)
    for b in (0, 3):
        ref = dict(refs[b])
        ref["rgb"] = np.where(ref["covered"][..., None], ref["rgb"], 1.0)
        ref["image"] = R.to_uint8(ref["rgb"])
        _compare(f"white image {b}", got, b, ref, None)
    assert (got["image"][3] == 255).all()


def test_a_mesh_without_faces_draws_nothing():
    sc = _scene(44)
    with_empty = Scene(sc.S, sc.verts + [sc.verts[0]], sc.faces + [np.zeros((0, 3), np.int32)], sc.valid + [np.ones(4, np.float32)],
                       sc.K, sc.image)
    got, plain = _gpu(with_empty), _gpu(sc)
    for k in ("rgb", "image", "depth", "face_id"):
        assert np.array_equal(got[k], plain[k]), k


def test_overfull_tile_lists_run_in_chunks():
    from hands_amd.rend_utils import SHADE_LIST_CAP, SHADE_TILE
    sc = _dense_scene()
    refs = [sc.ref(b, tile=SHADE_TILE) for b in range(sc.B)]
    for b, ref in enumerate(refs):
        print(f"dense image {b}: candidates per tile up to {int(ref['tile_candidates'].max())}")
        assert ref["tile_candidates"].max() > 2 * SHADE_LIST_CAP          # the list overflows at least twice
        _check_cap(f"dense image {b}", ref)
    got = _gpu(sc)
    for b, ref in enumerate(refs):
        _compare(f"dense image {b}", got, b, ref, sc.image[b], cap=False)
    assert all((refs[0]["face_id"] >= off).any() for off in np.cumsum([0] + [f.shape[0] for f in sc.faces[:3]]))


def test_rejected_faces_are_absent_and_change_nothing():
    """Three faces are appended to the last mesh: one on three new vertices of which one lies at Z <= 0, one that names a new
    NaN vertex, one with an index out of range.  None may be drawn, nothing may fault, and the picture is the clean one bit for
    bit (the normal sum skips a face whose cross product is not finite or whose index is out of range)."""
    sc = _scene(44)
    clean = _gpu(sc)
    vB, fB = sc.verts[1], sc.faces[1]
    n = vB.shape[1]
    extra = np.zeros((sc.B, 4, 3), np.float32)
    extra[:, 0] = (0.05, 0.05, -0.2)                        # behind the camera
    extra[:, 1] = (-0.05, 0.05, 0.3)
    extra[:, 2] = (0.0, -0.05, 0.3)                         # in front of everything: would hide the spheres if drawn
    extra[:, 3] = (np.nan, 0.0, 0.3)
    faces = np.concatenate([fB, np.array([[n, n + 1, n + 2], [5, n + 3, 9], [3, 7, n + 4], [3, -1, 7]], np.int32)])
    bad = Scene(sc.S, [sc.verts[0], np.concatenate([vB, extra], axis=1)], [sc.faces[0], faces], sc.valid, sc.K, sc.image)
    got = _gpu(bad)
    for k in ("rgb", "image", "depth", "face_id"):
        assert np.array_equal(got[k], clean[k]), k
    for b in range(3):
        _compare(f"rejected image {b}", got, b, bad.ref(b), sc.image[b])


def test_side_view_matches_the_restatement():
    import hands_amd
    sc = _scene(44)
    cam_transl = (0.004, -0.006, 0.03)
    r = hands_amd.Renderer(sc.S)
    got = _gpu(sc, renderer=r, image=False, sideview_angle=172.5, cam_transl=torch.tensor(cam_transl))
    front = _gpu(sc, renderer=r, image=False)
    assert not np.array_equal(got["face_id"][0], front["face_id"][0])
    for b in range(3):
        anchor = sc.verts[1][b] if sc.valid[1][b] else sc.verts[0][b]          # the last mesh that is valid for the image
        T64 = R.sideview_T(anchor, 172.5, cam_transl)
        T = hands_amd.sideview_transform(_t(anchor), 172.5, cam_transl).cpu().numpy()
        assert T.dtype == np.float32 and np.abs(T - T64).max() < 1e-6
        # the transform is an INPUT of the specification: the restatement gets the float32 one the renderer used
        _compare(f"side view image {b}", got, b, sc.ref(b, T=T, image=False), None)
    assert (got["image"][3] == 255).all()
    # cam_transl alone
    moved = _gpu(sc, renderer=r, image=False, cam_transl=cam_transl)
    Tt = np.concatenate([np.eye(3, dtype=np.float32), np.array(cam_transl, np.float32)[:, None]], axis=1)
    _compare("cam_transl image 0", moved, 0, sc.ref(0, T=Tt, image=False), None)


def test_visualize_rend_is_four_render_calls():
    import hands_amd
    sc = _scene(44)
    r = hands_amd.Renderer(sc.S)
    vr, vl, K, img = _t(sc.verts[0]), _t(sc.verts[1]), _t(sc.K), _t(sc.image)
    fr, fl, rv, lv = _t(sc.faces[0]), _t(sc.faces[1]), _t(sc.valid[0]), _t(sc.valid[1])
    stack = r.visualize_rend(vr, vl, K, img, faces_r=fr, faces_l=fl, right_valid=rv, left_valid=lv)
    assert stack.shape == (4, 4 * sc.S, sc.S, 3) and stack.dtype == torch.uint8
    kw = dict(colors=[COLORS[0], COLORS[1]], metallic=0.1, valid=[rv, lv])
    panels = [r.render_meshes_pose([vr, vl], [fr, fl], K, image=img, **kw)]
    panels += [r.render_meshes_pose([vr, vl], [fr, fl], K, sideview_angle=a, **kw) for a in (45.0, 172.5, 300.0)]
    torch.cuda.synchronize()
    for i, p in enumerate(panels):
        assert torch.equal(stack[:3, i * sc.S:(i + 1) * sc.S], p[:3]), i          # bit for bit
    assert not torch.equal(panels[1], panels[2]) and not torch.equal(panels[2], panels[3])
    # image 3 has no valid mesh: floor(255 image), four times
    want = torch.floor(255.0 * img[3]).to(torch.uint8).permute(1, 2, 0)
    for i in range(4):
        assert torch.equal(stack[3, i * sc.S:(i + 1) * sc.S], want), i


def test_coverage_equals_the_silhouette_rasteriser():
    import hands_amd
    sc = _scene(76)
    one = Scene(sc.S, sc.verts[:1], sc.faces[:1], [np.ones(sc.B, np.float32)], sc.K, None)
    got = _gpu(one, image=False)
    ras = hands_amd.rasterize(_t(one.verts[0]), _t(one.faces[0]), _t(one.K), sc.S)
    torch.cuda.synchronize()
    for b in range(3):
        ref = one.ref(b, image=False)
        _check_cap(f"single mesh image {b}", ref)
        ok = ~ref["unsure"]
        assert ref["covered"].sum() > 1000
        assert np.array_equal((got["face_id"][b] >= 0)[ok], (ras["face_idx"][b].cpu().numpy() >= 0)[ok]), b


def test_determinism_and_graph_capture():
    import hands_amd
    sc = _scene(76)
    r = hands_amd.Renderer(sc.S)
    a, b = _gpu(sc, renderer=r), _gpu(sc, renderer=r)
    for k in ("rgb", "image", "depth", "face_id"):
        assert np.array_equal(a[k], b[k]), k                   # two runs
    fresh = _gpu(sc)                                           # another renderer: its own caches and workspace
    for k in ("rgb", "image", "depth", "face_id"):
        assert np.array_equal(a[k], fresh[k]), k
    verts, faces, K, img = [_t(v) for v in sc.verts], [_t(f) for f in sc.faces], _t(sc.K), _t(sc.image)
    valid = [_t(v) for v in sc.valid]
    call = lambda: r.render_meshes_pose(verts, faces, K, image=img, colors=list(COLORS[:2]), valid=valid, return_float=True,
                                        sideview_angle=45.0, cam_transl=(0.0, 0.0, 0.02))
    eager = call()                                             # also fills the caches before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one stream, no parallel branches
        captured = call()
    for k in captured:
        captured[k].fill_(3)
    g.replay()
    torch.cuda.synchronize()
    for k in ("rgb", "image", "depth", "face_id"):
        assert torch.equal(captured[k], eager[k]), k


def test_real_path_hands_light_to_pictures():
    import hands_amd
    dev = _dev()
    model = hands_amd.apply_recipe(hands_amd.HandsLight()).to(dev)
    inputs, meta = hands_amd.synthetic_inputs(2, 0)
    inputs, meta = {k: v.to(dev) for k, v in inputs.items()}, {k: v.to(dev) for k, v in meta.items()}
    pred = model(inputs, meta)
    r = hands_amd.Renderer(224)
    pics = r.render_hands(pred, meta, images=inputs["img"])
    torch.cuda.synchronize()
    assert pics.shape == (2, 896, 224, 3) and pics.dtype == torch.uint8
    fr, fl = (hands_amd.synthetic_mano_asset(s).faces.astype(np.int32) for s in (True, False))
    img = hands_amd.denormalize_images(inputs["img"]).clamp(0.0, 1.0)
    direct = r.visualize_rend(pred["mano.v3d.cam.r"], pred["mano.v3d.cam.l"], meta["intrinsics"], img, faces_r=_t(fr), faces_l=_t(fl))
    assert torch.equal(pics, direct)
    # a wrapper `vis` dict gives the same pictures
    vis = {"pred.mano.v3d.cam.r": pred["mano.v3d.cam.r"], "pred.mano.v3d.cam.l": pred["mano.v3d.cam.l"],
           "meta_info.intrinsics": meta["intrinsics"], "meta_info.mano.faces.r": fr, "meta_info.mano.faces.l": fl,
           "inputs.img": inputs["img"]}
    assert torch.equal(r.render_hands(vis), pics)
    got = pics.cpu().numpy()
    vr, vl = pred["mano.v3d.cam.r"].cpu().numpy(), pred["mano.v3d.cam.l"].cpu().numpy()
    K, bg = meta["intrinsics"].cpu().numpy(), img.cpu().numpy()
    sc = Scene(224, [vr, vl], [fr, fl], [np.ones(2, np.float32)] * 2, K, bg)
    # the asset's faces are a random soup, hundreds of layers deep: more near-ties than on the spheres, so the cap on the unsure
    # pixels is 3 % of a panel's covered pixels here (the 1 % cap is set for the sphere scenes; the restatement gives 0.2-2.3 %)
    for b in range(2):
        for i, angle in enumerate((None, 45.0, 172.5, 300.0)):
            T = None if angle is None else hands_amd.sideview_transform(_t(vl[b]), angle).cpu().numpy()
            ref = sc.ref(b, T=T, image=angle is None)
            ok = ~ref["unsure"]
            lerr = np.abs(got[b, i * 224:(i + 1) * 224].astype(np.int64) - ref["image"].astype(np.int64))
            print(f"real path image {b} panel {i}: covered {int(ref['covered'].sum())}, unsure {int(ref['unsure'].sum())}, "
                  f"max 8-bit difference off unsure {int(lerr[ok].max())}")
            assert ref["covered"].sum() > 100 and (ref["unsure"] & ref["covered"]).sum() <= 0.03 * ref["covered"].sum(), (b, i)
            assert lerr[ok].max() <= 1, (b, i, int(lerr[ok].max()))
