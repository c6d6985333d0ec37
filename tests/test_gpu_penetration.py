"""hands_mesh_signed_f32 and the penetration functions built on it (hands_amd/penetration.py, evaluate_penetration_metrics,
HandsWrapper) on the device against the fp64 restatement (tests/penetration_ref.py).

Bars.  Every coordinate stays in |x| <= 0.6 m.  |sdf|: 5e-7 m, the bar of the closest_on_mesh tests (test_gpu_surface_metrics.BAR,
reasoned there).  face_idx: equal wherever the restatement's two nearest faces are more than that bar apart.  winding: F * 2^-20
absolute -- per face a few fp32 roundings of a term of size pi (the lengths, the two arguments, atan2f, the running sum), each
2^-24 * pi relative to the 2 pi the sum is divided by.  The sign of sdf: for every finite query whose fp64 |w| is more than
1e-3 away from 0.5, and at most 1 % of them may be that close.  NaN, +inf and -1 are exact, two runs give the same bits and the
guard bands around the outputs stay intact.
"""
import copy
import os

import numpy as np
import pytest
import torch

import penetration_ref as PR
import surface_ref as SR
from edge_util import EINVAL, In, Out, OutInt
from test_gpu_surface_metrics import BAR, CENTRE, _rot

pytestmark = pytest.mark.gpu

SIZE = 0.05              # metres: half the extent of a test mesh
W_MARGIN = 1e-3


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- the scenes (plain functions: a host-only script can check what the docstrings promise of the restatement) -------------
def mesh(name):
    """-> verts (V,3) in metres about CENTRE, faces (F,3)."""
    if name == "tetrahedron":
        v, f = PR.tetrahedron()
    elif name == "sphere":
        v, f = PR.uv_sphere(12, 8)
    else:
        v, f = PR.cube()
        if name == "cube_inward":
            f = f[:, ::-1].copy()
        elif name == "cube_plus":                  # a zero-area face, a face with an index out of range, a negative index
            f = np.concatenate([f[:5], [[2, 2, 5]], f[5:], [[0, 1, 8]], [[-1, 2, 3]]])
        else:
            assert name == "cube"
    return v @ _rot([1, 2, 3], 0.3).T * SIZE + CENTRE, f


MESHES = ("tetrahedron", "cube", "sphere", "cube_inward", "cube_plus")


def queries(verts, faces, B, P, seed):
    """(B,P,3) fp32: random points in and around the mesh and, as far as P leaves room, every vertex, the centre of every
    usable face moved by +-1e-3 of the mesh size along its normal, one NaN and one inf."""
    rng = np.random.RandomState(seed)
    ok = SR.usable_faces(verts, faces)
    T = verts[np.asarray(faces)[ok]]
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    keep = np.linalg.norm(n, axis=1) > 0
    c, n = T[keep].mean(1), n[keep] / np.linalg.norm(n[keep], axis=1, keepdims=True)
    special = np.concatenate([[[np.nan, 0.1, 0.5]], [[0.1, np.inf, 0.5]], verts, c + 1e-3 * SIZE * n, c - 1e-3 * SIZE * n])
    out = []
    for b in range(B):
        q = CENTRE + 1.6 * SIZE * (2 * rng.rand(P, 3) - 1)
        k = min(len(special), P - 1)               # one random point stays; the NaN and the inf come first
        q[P - k:] = special[np.r_[0, 1, 2 + rng.permutation(len(special) - 2)][:k]]
        out.append(q)
    return np.float32(out)


def reference(points, verts, faces, valid):
    """The restatement on the fp32 inputs, plus the gap (B,P) between its nearest and second nearest face."""
    sdf, w, idx = PR.signed_distance(points, verts, faces, valid)
    gap = np.full(sdf.shape, np.inf)
    for b in range(len(points)):
        okb = SR.usable_faces(verts[b], faces)
        fin = np.isfinite(sdf[b])
        if okb.sum() >= 2 and fin.any():
            T = np.float64(verts[b])[np.asarray(faces)[okb]]
            d = np.sqrt(np.sort(SR.point_triangle(np.float64(points[b][fin]), T[:, 0], T[:, 1], T[:, 2], False)[0], 1))
            gap[b, fin] = d[:, 1] - d[:, 0]
    return sdf, w, idx, gap


def near_half(w):
    """Mask of the finite queries whose |w| is within W_MARGIN of 0.5, and their share among the finite ones."""
    fin = np.isfinite(w)
    close = fin & (np.abs(np.abs(np.where(fin, w, 0.0)) - 0.5) <= W_MARGIN)
    return close, close.sum() / max(fin.sum(), 1)


# ---- 1. the primitive through the C ABI, guarded buffers -------------------------------------------------------------------
def run_signed(points, verts, faces, valid=None, F=None, with_optional=True):
    from hands_amd import _lib
    points, verts = np.float32(points), np.float32(verts)
    B, P, V = points.shape[0], points.shape[1], verts.shape[1]
    pin, vin = In(torch.from_numpy(points)), In(torch.from_numpy(verts))
    fc = _cuda(np.int32(faces).reshape(-1, 3)) if len(faces) else None
    vl = None if valid is None else In(torch.tensor(valid, dtype=torch.float32))
    sdf, w, idx = Out(B, P), Out(B, P), OutInt(torch.int32, B, P)
    rc = _lib.lib().hands_mesh_signed_f32(pin.ptr(), vin.ptr(), _lib.ptr(fc) if fc is not None else None, vl.ptr() if vl else None,
                                          sdf.ptr(), w.ptr() if with_optional else None, idx.ptr() if with_optional else None,
                                          B, P, V, len(faces) if F is None else F, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    if not with_optional:
        return sdf.get().numpy()
    return sdf.get().numpy(), w.get().numpy(), idx.get().numpy()                # get() checks the guard bands


def check_signed(points, verts, faces, valid=None, what=""):
    points, verts = np.float32(points), np.float32(verts)
    assert all(np.abs(x[np.isfinite(x)]).max(initial=0.0) <= 0.6 for x in (points, verts))
    sdf, w, idx = run_signed(points, verts, faces, valid)
    again = run_signed(points, verts, faces, valid)
    for x, y in zip((sdf, w, idx), again):
        assert x.tobytes() == y.tobytes(), what                                # bit-reproducible
    assert run_signed(points, verts, faces, valid, with_optional=False).tobytes() == sdf.tobytes()
    rs, rw, ri, gap = reference(points, verts, faces, valid)
    # special values: exact
    np.testing.assert_array_equal(np.isnan(sdf), np.isnan(rs), err_msg=what)
    np.testing.assert_array_equal(np.isnan(w), np.isnan(rw), err_msg=what)
    np.testing.assert_array_equal(np.isposinf(sdf), np.isposinf(rs), err_msg=what)
    assert not np.isneginf(sdf).any()
    np.testing.assert_array_equal(idx == -1, ri == -1, err_msg=what)
    assert ((idx >= -1) & (idx < max(len(faces), 1))).all()
    assert (w[np.isposinf(rs)] == 0).all()
    fin = np.isfinite(rs)
    F = max(len(faces), 1)
    e_d = np.abs(np.abs(sdf[fin].astype(np.float64)) - np.abs(rs[fin])).max(initial=0.0)
    e_w = np.abs(w[fin].astype(np.float64) - rw[fin]).max(initial=0.0)
    sure_face = fin & (gap > BAR)
    close, share = near_half(rw)
    sure_sign = fin & ~close
    print(f"SIGNED|{what}|d {e_d:.2e} / {BAR:.1e}|w {e_w:.2e} / {F * 2.0 ** -20:.2e}|faces compared {sure_face.sum()} of {fin.sum()}"
          f"|near 0.5: {close.sum()} of {fin.sum()}")
    assert e_d <= BAR, (what, e_d)
    assert e_w <= F * 2.0 ** -20, (what, e_w)
    np.testing.assert_array_equal(idx[sure_face], ri[sure_face], err_msg=what)
    assert share <= 0.01, (what, share)
    np.testing.assert_array_equal(np.signbit(sdf[sure_sign]), np.signbit(rs[sure_sign]), err_msg=what)
    np.testing.assert_array_equal(np.signbit(sdf[sure_sign]), np.abs(w[sure_sign]) >= 0.5, err_msg=what)
    return sdf, w, idx


def batch_of(name, B):
    """The mesh, and for B = 3 two more copies: rotated, and shrunk (a sample of its own each)."""
    v, f = mesh(name)
    if B == 1:
        return np.float32(v[None]), f
    return np.float32([v, (v - CENTRE) @ _rot([3, 1, 2], 0.7).T + CENTRE, 0.6 * (v - CENTRE) + CENTRE]), f


@pytest.mark.parametrize("B,P", [(1, 1), (1, 255), (1, 257), (3, 1), (3, 255), (3, 257)])
@pytest.mark.parametrize("name", MESHES)
def test_primitive_against_the_restatement(name, B, P):
    verts, faces = batch_of(name, B)
    points = queries(np.float64(verts[0]), faces, B, P, seed=7 * P + B)
    valid = [1.0, 0.0, 1.0] if B == 3 else None
    sdf, w, idx = check_signed(points, verts, faces, valid, what=f"{name} B={B} P={P}")
    if B == 3:
        assert np.isnan(sdf[1]).all() and np.isnan(w[1]).all() and (idx[1] == -1).all() and np.isfinite(sdf[0]).any()
    if P >= 255:
        assert (sdf[0][np.isfinite(sdf[0])] < 0).any() and (sdf[0] > 0).any()  # the scene has both sides
        assert np.isnan(sdf[0]).sum() == 2                                     # the NaN and the inf query


def test_invalid_sample_is_not_read():
    verts, faces = batch_of("cube", 3)
    points = queries(np.float64(verts[0]), faces, 3, 40, seed=1)
    verts[1], points[1] = np.nan, np.nan
    sdf, w, idx = check_signed(points, verts, faces, [2.0, 0.0, 1.0], what="middle sample invalid and NaN")
    assert np.isnan(sdf[1]).all() and np.isfinite(w[[0, 2]]).sum() >= 2 * 38


def test_no_face_and_one_vertex():
    v, f = mesh("cube")
    points = queries(v, f, 1, 20, seed=2)
    for none, what in ((np.zeros((0, 3), np.int64), "F=0"), (np.array([[0, 1, 8], [9, 9, 9]]), "no usable face")):
        sdf, w, idx = check_signed(points, np.float32(v[None]), none, what=what)
        fin = np.isfinite(points[0]).all(1)
        assert np.isposinf(sdf[0][fin]).all() and (w[0][fin] == 0).all() and (idx == -1).all() and np.isnan(sdf[0][~fin]).all()
    one = np.float32(v[None, :1])                                              # V = 1: the face collapses to the vertex
    points[0, 0] = one[0, 0]
    sdf, w, idx = check_signed(points, one, np.array([[0, 0, 0]]), what="V=1")
    assert sdf[0, 0] == 0 and (w[0][np.isfinite(w[0])] == 0).all() and (idx[0][np.isfinite(sdf[0])] == 0).all()
    bad = np.float32(v[None]).copy()
    bad[0, 7, 1] = np.nan                                                      # a NaN vertex: its faces are skipped, the cube is open
    check_signed(points, bad, f, what="NaN vertex")


def test_einval_leaves_the_outputs_untouched():
    from hands_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    pts, vt = torch.rand(2, 4, 3).cuda(), torch.rand(2, 5, 3).cuda()
    fc = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32).cuda()
    sdf, w, idx = torch.full((2, 4), -7.5).cuda(), torch.full((2, 4), -7.5).cuda(), torch.full((2, 4), -7, dtype=torch.int32).cuda()
    s = torch.cuda.current_stream().cuda_stream
    good = [p(pts), p(vt), p(fc), None, p(sdf), p(w), p(idx), 2, 4, 5, 2]
    for i, v in ((7, 0), (8, 0), (9, 0), (7, -1), (10, -1), (9, _lib.MESH_MAX_V + 1), (10, _lib.SURF_MAX_F + 1), (0, None), (1, None),
                 (2, None), (4, None)):
        a = list(good)
        a[i] = v
        assert L.hands_mesh_signed_f32(*a, s) == EINVAL, (i, v)
    torch.cuda.synchronize()
    assert bool((sdf == -7.5).all()) and bool((w == -7.5).all()) and bool((idx == -7).all())


def test_wrapper_of_the_entry():
    from hands_amd import signed_distance_to_mesh
    verts, faces = batch_of("sphere", 3)
    points = queries(np.float64(verts[0]), faces, 3, 300, seed=3)
    valid = [1.0, 0.0, 1.0]
    sdf, w, idx = signed_distance_to_mesh(_cuda(points), _cuda(verts), faces, _cuda(np.float32(valid)))
    torch.cuda.synchronize()
    assert sdf.dtype == w.dtype == torch.float32 and idx.dtype == torch.int64 and sdf.shape == w.shape == idx.shape == (3, 300)
    assert sdf.is_cuda and w.is_cuda and idx.is_cuda
    raw = run_signed(points, verts, faces, valid)
    assert sdf.cpu().numpy().tobytes() == raw[0].tobytes() and w.cpu().numpy().tobytes() == raw[1].tobytes()
    assert (idx.cpu().numpy() == raw[2]).all()
    for conv in (lambda f: torch.from_numpy(np.int64(f)), lambda f: np.int16(f), lambda f: _cuda(np.int32(f))):
        again = signed_distance_to_mesh(_cuda(points), _cuda(verts), conv(faces))[1]
        assert torch.equal(again[[0, 2]].view(torch.int32), w[[0, 2]].view(torch.int32))       # the bits: NaN queries included


# ---- 2. the two hands ------------------------------------------------------------------------------------------------------
R_HAND = 0.04


def sphere_hands():
    """Right: a 12 x 8 sphere of radius r about CENTRE; left: one of 0.8 r, turned, its centre 2.5 r, 1.5 r, 0 and 1.5 r away;
    the last sample is not valid."""
    vr, fr = PR.uv_sphere(12, 8, R_HAND)
    vl, fl = PR.uv_sphere(12, 8, 0.8 * R_HAND)
    vl = vl @ _rot([1, -2, 0.5], 0.4).T
    axis = np.array([0.6, 0.8, 0.0])
    dist = [2.5, 1.5, 0.0, 1.5]
    v_r = np.float32([vr + CENTRE for _ in dist])
    v_l = np.float32([vl + CENTRE + d * R_HAND * axis for d in dist])
    valid = {"right_valid": np.float32([1, 1, 1, 1]), "left_valid": np.float32([1, 1, 1, 0]), "is_valid": np.float32([1, 1, 1, 1])}
    return v_r, v_l, fr, fl, valid, dist


def cup_hands():
    """Right: the cube without its +z side; left: a small tetrahedron inside the cup, just under the opening."""
    vc, fc = PR.cube()
    vt, ft = PR.tetrahedron()
    v_r = np.float32([vc * SIZE + CENTRE])
    v_l = np.float32([vt * 0.1 * SIZE + CENTRE + [0.0, 0.0, 0.7 * SIZE]])
    return v_r, v_l, fc[:10], ft


def _dev(d):
    return {k: _cuda(v) if isinstance(v, np.ndarray) and v.dtype == np.float32 else v for k, v in d.items()}


def check_penetration(out, ref, live, what):
    for k in ("rl", "lr"):
        close, share = near_half(ref["winding." + k][live])
        assert share == 0, (what, k, "the scene has a vertex on the other hand's surface")
        sdf, inside = out["sdf." + k].cpu().numpy(), out["inside." + k].cpu().numpy()
        depth, count = out["pen.depth." + k].cpu().numpy(), out["pen.count." + k].cpu().numpy()
        assert inside.dtype == count.dtype == np.int64 and sdf.dtype == depth.dtype == np.float32
        assert sdf.shape == inside.shape == ref["sdf." + k].shape and depth.shape == count.shape == (len(sdf),)
        e = np.abs(sdf[live].astype(np.float64) - ref["sdf." + k][live]).max()
        e_depth = np.abs(depth[live].astype(np.float64) - ref["pen.depth." + k][live]).max()
        print(f"PEN|{what}|{k}|sdf {e:.2e}|depth {e_depth:.2e} / {BAR:.1e}|depth mm {1e3 * depth}|count {count}")
        assert e <= BAR and e_depth <= BAR
        np.testing.assert_array_equal(inside[live], ref["inside." + k][live])
        np.testing.assert_array_equal(count[live], ref["pen.count." + k][live])
        assert (depth[live] == np.maximum(0, -sdf[live].min(1))).all() and (count == inside.sum(1)).all()


def test_interhand_penetration_of_two_spheres():
    from hands_amd import interhand_penetration
    v_r, v_l, fr, fl, valid, dist = sphere_hands()
    ref = PR.interhand_penetration(v_r, v_l, fr, fl, True, valid=[1, 1, 1, 0])
    d = _dev({"mano.v3d.cam.r": v_r, "mano.v3d.cam.l": v_l, "mano.faces.r": fr, "mano.faces.l": fl, **valid})
    out = interhand_penetration(d)
    torch.cuda.synchronize()
    assert list(out) == [f"{q}.{k}" for k in ("rl", "lr") for q in ("sdf", "inside", "pen.depth", "pen.count")]
    check_penetration(out, ref, [0, 1, 2], "spheres")
    for k in ("rl", "lr"):
        depth, count = out["pen.depth." + k].cpu().numpy(), out["pen.count." + k].cpu().numpy()
        assert depth[0] == 0 and count[0] == 0 and depth[1] > 1e-3 and count[1] > 0       # apart; through each other
        assert np.isnan(depth[3]) and count[3] == 0 and np.isnan(out["sdf." + k][3].cpu().numpy()).all()
        assert (out["inside." + k][3] == 0).all()
    assert out["pen.count.lr"][2] == v_l.shape[1] and out["pen.count.rl"][2] == 0         # the small sphere inside the large one
    assert abs(float(out["pen.depth.lr"][2]) - 0.2 * R_HAND) < 0.14 * R_HAND              # 0.2 r, less the chords of the mesh
    same = interhand_penetration({k: v for k, v in d.items() if "faces" not in k}, faces=(fr, fl), seal=False)    # closed already
    for k in out:
        assert torch.equal(out[k].view(torch.int32) if out[k].dtype == torch.float32 else out[k],
                           same[k].view(torch.int32) if same[k].dtype == torch.float32 else same[k]), k


def test_interhand_penetration_seals_an_open_hand():
    from hands_amd import interhand_penetration
    v_r, v_l, fr, fl = cup_hands()
    d = _dev({"mano.v3d.cam.r": v_r, "mano.v3d.cam.l": v_l})
    got = {}
    for seal in (True, False):
        out = interhand_penetration(d, faces=(fr, fl), seal=seal)
        torch.cuda.synchronize()
        check_penetration(out, PR.interhand_penetration(v_r, v_l, fr, fl, seal), [0], f"cup seal={seal}")
        assert out["sdf.lr"].shape == (1, 4) and out["sdf.rl"].shape == (1, 8)            # the seal's vertex is no query
        got[seal] = float(out["pen.depth.lr"][0])
        assert out["pen.count.lr"][0] == 4
    # sealed, the lid is the nearest surface of the tetrahedron inside the cup (its lower vertices 0.4 below it); open, the
    # walls are (0.9 away)
    assert abs(got[True] - 0.4 * SIZE) < 1e-6 and abs(got[False] - 0.9 * SIZE) < 1e-6 and got[False] - got[True] > 1000 * BAR


@pytest.fixture(scope="module")
def sphere_volume():
    from hands_amd import intersection_volume
    v_r, v_l, fr, fl, valid, dist = sphere_hands()
    d = _dev({"mano.v3d.cam.r": v_r, "mano.v3d.cam.l": v_l, **valid})
    vol = intersection_volume(d, faces=(fr, fl), G=8)
    torch.cuda.synchronize()
    return d, vol


def test_intersection_volume_of_two_spheres(sphere_volume):
    from hands_amd import penetration_grid
    v_r, v_l, fr, fl, valid, dist = sphere_hands()
    d, vol = sphere_volume
    assert vol.shape == (4,) and vol.dtype == torch.float32 and vol.is_cuda
    points, cell = penetration_grid(d["mano.v3d.cam.r"], d["mano.v3d.cam.l"], 8)         # closed meshes: nothing is appended
    assert points.shape == (4, 512, 3) and points.is_cuda
    points, cell, vol = points.cpu().numpy(), cell.cpu().numpy(), vol.cpu().numpy()
    rp, rc = PR.penetration_grid(v_r, v_l, 8)
    assert np.abs(points - rp).max() <= 1e-7 and np.abs(cell - rc).max() <= 1e-6 * rc.max()
    w_r, w_l = PR.grid_windings(points, v_r, v_l, fr, fl, True, valid=[1, 1, 1, 0])
    live = [0, 1, 2]
    assert near_half(w_r[live])[1] == 0 and near_half(w_l[live])[1] == 0                  # no grid point on a surface
    count = ((np.abs(w_r[live]) >= 0.5) & (np.abs(w_l[live]) >= 0.5)).sum(1)
    for b in live:
        lens = PR.lens_volume(R_HAND, 0.8 * R_HAND, dist[b] * R_HAND)
        print(f"VOLUME|d = {dist[b]} r|{count[b]} of 512 cells|{1e6 * vol[b]:.3f} cm3|balls: {1e6 * lens:.3f} cm3")
        assert vol[b] == np.float32(count[b]) * cell[b]
    assert vol[0] == 0 and cell[0] == 0 and count[1] > 0 and count[2] > count[1] and np.isnan(vol[3])


def test_evaluate_penetration_metrics(sphere_volume):
    from hands_amd import evaluate_penetration_metrics, interhand_penetration
    v_r, v_l, fr, fl, valid, dist = sphere_hands()
    d, vol = sphere_volume
    pred = {k: v for k, v in d.items() if k.startswith("mano")}
    targets = {k: v for k, v in d.items() if not k.startswith("mano")}
    keys = [f"pen/{q}/{s}" for q in ("depth", "count") for s in "rlh"]
    out = evaluate_penetration_metrics(pred, targets, faces=(fr, fl))
    assert list(out) == keys
    full = evaluate_penetration_metrics(pred, targets, {"mano.faces.r": fr, "mano.faces.l": fl}, volume_grid=8)
    assert list(full) == keys + ["pen/volume/h"]
    torch.cuda.synchronize()
    pen = interhand_penetration(d, faces=(fr, fl))
    ref = PR.evaluate_penetration(v_r, v_l, fr, fl, [1, 1, 1, 0])
    for k in keys:
        v = out[k].cpu().numpy()
        assert out[k].is_cuda and v.dtype == np.float32 and v.shape == (4,) and np.isnan(v[3]) and np.isfinite(v[:3]).all(), k
        assert torch.equal(out[k].view(torch.int32), full[k].view(torch.int32))
        np.testing.assert_allclose(v[:3], ref[k][:3], rtol=0, atol=1e3 * BAR if "depth" in k else 0, err_msg=k)      # mm
    for s, k in (("r", "rl"), ("l", "lr")):
        assert torch.equal(out[f"pen/depth/{s}"][:3], 1000.0 * pen[f"pen.depth.{k}"][:3])                            # millimetres
        assert torch.equal(out[f"pen/count/{s}"][:3], pen[f"pen.count.{k}"][:3].float())
    for q in ("depth", "count"):
        assert torch.equal(out[f"pen/{q}/h"][:3], torch.maximum(out[f"pen/{q}/r"], out[f"pen/{q}/l"])[:3])
    assert float(out["pen/depth/h"][2]) > 1.0 and float(out["pen/depth/r"][2]) == 0                                  # 0.2 r = 8 mm
    assert torch.equal(full["pen/volume/h"][:3], 1e6 * vol[:3]) and bool(torch.isnan(full["pen/volume/h"][3]))       # cm^3
    with pytest.raises(ValueError):
        evaluate_penetration_metrics(pred, targets)


# ---- 3. the wrapper --------------------------------------------------------------------------------------------------------
def test_wrapper_penetration_metrics(golden_dir, recipe_model):
    from hands_amd import evaluate_penetration_metrics
    from hands_amd.weights import synthetic_inputs
    from hands_amd.wrapper import HandsWrapper
    d = np.load(os.path.join(golden_dir, "process_data.npz"))
    tin = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("in/")}
    K = tin.pop("intrinsics")
    B = K.shape[0]
    inputs, meta = synthetic_inputs(B, 4, device="cuda")
    meta["intrinsics"] = K.cuda()
    meta["imgname"] = [f"{i}.jpg" for i in range(B)]
    targets = {k: v.cuda() for k, v in tin.items()}
    g = torch.Generator().manual_seed(1)
    for h in "rl":
        targets[f"mano.j2d.norm.{h}"] = (0.5 * torch.randn(B, 21, 2, generator=g)).cuda()
        targets[f"joints_valid_{h}"] = torch.ones(B, 21).cuda()
    targets.update(is_valid=torch.ones(B).cuda(), right_valid=torch.ones(B).cuda(), left_valid=torch.tensor([1.0, 0, 1, 1, 1, 1]).cuda())
    w = HandsWrapper(model=copy.deepcopy(recipe_model).to("cuda"))
    assert w.penetration_seal is True
    today = ["imgname"] + ["metric." + k for k in ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l",
                                                   "pix_err/r", "pix_err/l", "pix_err/h")]
    out0, _ = w.forward(inputs, dict(targets), meta, "test")
    assert list(out0) == today                                                           # without the name: what it was
    w.metric_dict = w.metric_dict + ["penetration"]
    with pytest.raises(ValueError):                                                      # the synthetic asset's faces cannot be sealed
        w.forward(inputs, dict(targets), meta, "test")
    w.penetration_seal = False
    out1, _ = w.forward(inputs, dict(targets), meta, "test")
    keys = [f"metric.pen/{q}/{s}" for q in ("depth", "count") for s in "rlh"]
    assert list(out1) == today + keys
    for k in today[1:]:
        assert torch.equal(out0[k].view(torch.int32), out1[k].view(torch.int32)), k
    full = w.forward(inputs, dict(targets), meta, "extract")
    pred = {k[len("pred."):]: v.cuda() for k, v in full.items() if k.startswith("pred.") and torch.is_tensor(v)}
    tgt = {k[len("targets."):]: v.cuda() for k, v in full.items() if k.startswith("targets.") and torch.is_tensor(v)}
    direct = evaluate_penetration_metrics(pred, tgt, faces=(w.model.mano_r.faces, w.model.mano_l.faces), seal=False)
    for k in keys:
        a, b = out1[k], direct[k[len("metric."):]].cpu()
        assert a.device.type == "cpu" and a.shape == (B,) and torch.equal(a.view(torch.int32), b.view(torch.int32)), k
    assert bool(torch.isnan(out1["metric.pen/depth/h"][1])) and bool(torch.isfinite(out1["metric.pen/depth/h"][[0, 2, 3, 4, 5]]).all())
