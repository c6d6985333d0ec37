"""hands_mesh_closest_f32, hands_eval_surface_metrics_f32 and hands_amd.interhand_field on the device against the fp64
restatement (tests/surface_ref.py).

Bars.  Every coordinate stays in |x| <= 0.6 m.  Per-point distances: |d - d_fp64| <= 5e-7 m, the project's absolute bar for
continuous metric keys (5e-4 mm, tests/test_gpu_mesh_metrics.py) -- about ten times what fp32 needs: the kernel's arithmetic run
on the host stays within 6e-8 m of the restatement on the scenes of test_mano_counts.  face_idx: the fp64 distance from the query
to the reported face is at most the fp64 minimum + 5e-7 m (an equality check would be wrong: the closest point usually lies on
an edge or a vertex that several faces share, and fp32 and fp64 break such ties differently).  closest: | |p - c| - d | <= 5e-7
and the fp64 distance from c to the reported face is <= 5e-7; no query is excused.  Metric keys: rtol 2e-5 / atol 5e-4 mm and
equal NaN patterns, the mpvpe bar.
"""
import copy
import os

import numpy as np
import pytest
import torch

import render_ref
import surface_ref as SR
from test_surface_metrics import CLOSED_FORMS, DEGENERATE, DEGENERATE_VERTS, TRI

pytestmark = pytest.mark.gpu

BAR = 5e-7               # metres
CENTRE = np.array([0.05, -0.03, 0.5])


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _closest(points, verts, faces, valid=None):
    from hands_amd import closest_on_mesh
    dist, idx, cl = closest_on_mesh(_cuda(np.float32(points)), _cuda(np.float32(verts)), faces,
                                    None if valid is None else _cuda(np.float32(valid)), return_points=True)
    torch.cuda.synchronize()
    B, P = np.shape(points)[:2]
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and cl.dtype == torch.float32
    assert dist.shape == (B, P) and idx.shape == (B, P) and cl.shape == (B, P, 3) and dist.is_cuda and idx.is_cuda and cl.is_cuda
    return dist.cpu().numpy(), idx.cpu().numpy(), cl.cpu().numpy()


def check_closest(points, verts, faces, valid=None, what=""):
    """The three outputs of every query of the batch against the restatement, with the bars of the module docstring."""
    points, verts = np.float32(points), np.float32(verts)
    assert all(np.abs(x[np.isfinite(x)]).max(initial=0.0) <= 0.6 for x in (points, verts))
    dist, idx, cl = _closest(points, verts, faces, valid)
    rd, ri, _ = SR.closest_on_mesh(points, verts, faces, valid)
    np.testing.assert_array_equal(np.isnan(dist), np.isnan(rd), err_msg=what)
    np.testing.assert_array_equal(np.isinf(dist), np.isinf(rd), err_msg=what)
    np.testing.assert_array_equal(idx < 0, ri < 0, err_msg=what)
    assert ((idx >= -1) & (idx < max(len(faces), 1))).all()
    np.testing.assert_array_equal(np.isnan(cl).all(-1), ri < 0, err_msg=what)
    assert (np.isnan(cl).any(-1) == np.isnan(cl).all(-1)).all()
    worst = [0.0, 0.0, 0.0, 0.0]
    for b in range(len(points)):
        hit = ri[b] >= 0
        if not hit.any():
            continue
        p, d, c = points[b][hit].astype(np.float64), dist[b][hit].astype(np.float64), cl[b][hit].astype(np.float64)
        errs = (np.abs(d - rd[b][hit]), SR.distance_to_face(p, verts[b], faces, idx[b][hit]) - rd[b][hit],
                np.abs(np.sqrt(((p - c) ** 2).sum(-1)) - d), SR.distance_to_face(c, verts[b], faces, idx[b][hit]))
        worst = [max(w, float(e.max())) for w, e in zip(worst, errs)]
    print(f"{what}: |d - d64| {worst[0]:.2e}  face excess {worst[1]:.2e}  ||p - c| - d| {worst[2]:.2e}  c to face {worst[3]:.2e}"
          f"  other face than fp64 {(idx != ri).mean():.3f}")
    assert max(worst) <= BAR, (what, worst)
    return dist, idx, cl


def _soup(V, F, seed):
    """A hand-sized cloud of V vertices and F random faces over it."""
    rng = np.random.RandomState(seed)
    return CENTRE + 0.08 * (rng.rand(V, 3) - 0.5), rng.randint(0, V, (F, 3))


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------
def test_closed_forms_on_the_device():
    for q, d, c in CLOSED_FORMS:
        dist, idx, cl = _closest([[q]], [TRI], np.array([[0, 1, 2]]))
        assert dist[0, 0] == d and idx[0, 0] == 0 and (cl[0, 0] == c).all(), q
    for face, q, d, c in DEGENERATE:
        dist, idx, cl = _closest([[q]], [DEGENERATE_VERTS], np.array([face]))
        assert dist[0, 0] == d and idx[0, 0] == 0 and (cl[0, 0] == c).all(), (face, q)


# ---- 2. launch geometry ----------------------------------------------------------------------------------------------------
def _chunk():
    from hands_amd import _lib
    return _lib.SURF_CHUNK


@pytest.mark.parametrize("case", range(6))
def test_launch_geometry(case):
    """P around the queries of a workgroup, F around the stride of the face load (the kernel has no face chunk), the largest
    V with the largest F."""
    from hands_amd import _lib
    c = _chunk()
    P, V, F = ((1, 3, 1), (c - 1, 40, 255), (c, 41, 256), (c + 1, 42, 257), (2 * c + 3, 43, 31),
               (9, _lib.MESH_MAX_V, _lib.SURF_MAX_F))[case]
    verts, faces = _soup(V, F, case)
    rng = np.random.RandomState(100 + case)
    points = CENTRE + 0.1 * (rng.rand(2, P, 3) - 0.5)
    check_closest(points, np.stack([verts, verts[::-1]]), faces, what=f"P={P} V={V} F={F}")


def test_invalid_sample_is_not_read():
    verts, faces = _soup(30, 50, 7)
    rng = np.random.RandomState(7)
    points = np.float32(CENTRE + 0.1 * (rng.rand(3, 70, 3) - 0.5))
    verts = np.float32(np.stack([verts, verts, verts + 0.01]))
    points[1], verts[1] = np.nan, np.nan
    dist, idx, cl = check_closest(points, verts, faces, valid=[1.0, 0.0, 2.0], what="B=3, middle invalid")
    assert np.isnan(dist[1]).all() and (idx[1] == -1).all() and np.isnan(cl[1]).all() and np.isfinite(dist[[0, 2]]).all()


# ---- 3. MANO's counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["grid", "soup"])
def test_mano_counts(scene):
    """778 vertices / 1538 faces: the closed grid of render_ref and the synthetic asset's face soup (7 faces with a repeated
    index); the queries are the vertices plus noise of 0, 0.1, 2 and 8 mm, one level per vertex in turn."""
    from hands_amd.mano import synthetic_mano_asset
    if scene == "grid":
        v, f = render_ref.mano_sized_mesh()
    else:
        a = synthetic_mano_asset(True)
        v, f = a.v_template, a.faces
        assert ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum() == 7
    assert v.shape == (778, 3) and f.shape == (1538, 3)
    rng = np.random.RandomState(3)
    level = np.array([0.0, 1e-4, 2e-3, 8e-3])
    off = CENTRE * [1, 1, 0.9 if scene == "grid" else 0.3]         # the asset's template spans +-0.3 m: all in |x| <= 0.6
    verts = np.float32(np.stack([v + off, v @ _rot([1, 2, 3], 0.8).T + off * [-1, 1, 1]]))
    points = np.stack([verts[b] + level[(np.arange(778) + b) % 4][:, None] * rng.randn(778, 3) for b in range(2)])
    dist, _, _ = check_closest(points, verts, f, what=scene)
    if scene == "grid":
        assert (dist[0][::4] == 0).all()                 # a vertex that lies in a face, without noise: exactly 0


# ---- 4. edge semantics -----------------------------------------------------------------------------------------------------
def test_edge_semantics():
    verts = np.concatenate([TRI, TRI + [0, 0, 0.5]]) * 0.5
    q = np.array([[[0.125, 0.125, 0.0625], [0.1, 0.05, 0.2], [np.nan, 0, 0], [0.1, np.inf, 0]]])
    faces = np.array([[0, 1, 6], [3, 4, 5], [0, 1, 2], [0, 1, 2], [-1, 1, 2]])        # out of range, far, near, its copy, negative
    dist, idx, cl = check_closest(q, [verts], faces, what="skipped faces")
    assert dist[0, 0] == 0.0625 and idx[0, 0] == 2                                     # the lower of two equal faces
    assert np.isnan(dist[0, 2:]).all() and (idx[0, 2:] == -1).all()
    for none in (np.array([[0, 1, 6], [7, 7, 7]]), np.zeros((0, 3), np.int64)):        # no usable face, F = 0
        dist, idx, cl = check_closest(q, [verts], none, what=f"F={len(none)}")
        assert np.isinf(dist[0, :2]).all() and (dist[0, :2] > 0).all() and (idx == -1).all() and np.isnan(cl).all()
        assert np.isnan(dist[0, 2:]).all()
    bad = np.float32(verts).copy()
    bad[4, 1] = np.nan                                                                 # a NaN vertex: its face is skipped
    dist, idx, _ = check_closest(q, [bad], faces, what="NaN vertex")
    assert (idx[0, :2] == 2).all()
    dist, idx, _ = check_closest(q, [bad], faces[:2], what="NaN vertex, nothing left")
    assert np.isinf(dist[0, :2]).all()


def test_einval_through_ctypes_leaves_the_outputs_untouched():
    from hands_amd import _lib
    L = _lib.lib()
    pts, vt = torch.rand(2, 4, 3).cuda(), torch.rand(2, 5, 3).cuda()
    fc = torch.tensor([[0, 1, 2], [2, 3, 4]], dtype=torch.int32).cuda()
    dist, idx, cl = torch.full((2, 4), -7.5).cuda(), torch.full((2, 4), -7, dtype=torch.int32).cuda(), torch.full((2, 4, 3), -7.5).cuda()
    s = torch.cuda.current_stream().cuda_stream
    p = _lib.ptr
    call = lambda *a: L.hands_mesh_closest_f32(*a, s)
    good = [p(pts), p(vt), p(fc), None, p(dist), p(idx), p(cl), 2, 4, 5, 2]
    for i, v in ((7, 0), (8, 0), (9, 0), (7, -1), (10, -1), (9, _lib.MESH_MAX_V + 1), (10, _lib.SURF_MAX_F + 1), (0, None), (1, None),
                 (2, None), (4, None)):
        a = list(good)
        a[i] = v
        assert call(*a) == 10001, (i, v)
    torch.cuda.synchronize()
    assert bool((dist == -7.5).all()) and bool((idx == -7).all()) and bool((cl == -7.5).all())
    assert call(*good) == 0 and call(*(good[:5] + [None, None] + good[7:])) == 0       # the optional outputs
    torch.cuda.synchronize()
    assert bool((dist >= 0).all()) and bool((idx >= 0).all()) and bool((cl != -7.5).all())


# ---- 5. metrics ------------------------------------------------------------------------------------------------------------
def _faces():
    from hands_amd.mano import synthetic_mano_asset
    return render_ref.mano_sized_mesh()[1], synthetic_mano_asset(False).faces


def make_batch(B, seed=0, noise_mm=(2.0, 4.0, 8.0)):
    """As make_batch of tests/test_gpu_mesh_metrics.py -- ground truth = a hand-sized mesh + offset, prediction = a rotated copy
    scaled x 1.1 plus Gaussian noise of 2, 4, 8 mm (by sample) -- with a surface under each hand: the right hand is the closed
    grid of render_ref, the left the synthetic asset's template under its random face soup."""
    from hands_amd.mano import synthetic_mano_asset
    rng = np.random.RandomState(seed)
    meshes = {"r": render_ref.mano_sized_mesh()[0].astype(np.float64), "l": synthetic_mano_asset(False).v_template.astype(np.float64)}
    pred, targets = {}, {}
    for s in "rl":
        gv, gj, pv, pj = [], [], [], []
        for b in range(B):
            off = np.array([0.05 if s == "r" else -0.07, -0.03, 0.42 if s == "r" else 0.15]) + 0.02 * rng.randn(3)   # all in |x| <= 0.6
            v = meshes[s] + off
            j = v[rng.choice(778, 21, replace=False)] * [1, 1, 0.999]
            R, c, sig = _rot(rng.randn(3), 0.15 + 0.05 * b), v.mean(0), noise_mm[b % len(noise_mm)] * 1e-3
            f = lambda x: 1.1 * (x - c) @ R.T + c + sig * rng.randn(*x.shape)
            gv.append(v), gj.append(j), pv.append(f(v)), pj.append(f(j))
        targets[f"mano.v3d.cam.{s}"], targets[f"mano.j3d.cam.{s}"] = np.float32(gv), np.float32(gj)
        pred[f"mano.v3d.cam.{s}"], pred[f"mano.j3d.cam.{s}"] = np.float32(pv), np.float32(pj)
    assert max(np.abs(x).max() for d in (pred, targets) for x in d.values()) <= 0.6
    targets.update(is_valid=np.ones(B, np.float32), right_valid=np.ones(B, np.float32), left_valid=np.ones(B, np.float32))
    return pred, targets


def _dev(d):
    return {k: _cuda(v) for k, v in d.items()}


def _run(pred, targets, faces):
    from hands_amd import evaluate_surface_metrics
    out = evaluate_surface_metrics(_dev(pred), _dev(targets), faces=faces)
    torch.cuda.synchronize()
    B = len(targets["is_valid"])
    assert list(out) == [f"{q}/{a}/{s}" for q in ("p2s", "chamfer") for a in ("ra", "pa") for s in "rlh"]
    assert all(v.is_cuda and v.dtype == torch.float32 and v.shape == (B,) for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    return {k: np.asarray(v).view(np.int32).copy() for k, v in out.items()}


def check_metrics(got, ref, what=""):
    assert set(got) == set(ref)
    for k in ref:
        print(what, k, got[k], ref[k])
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
        np.testing.assert_allclose(got[k], ref[k], rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=k)
        if k.endswith("/h"):                             # h is the nanmean of the r and l the device itself gave
            np.testing.assert_allclose(got[k], SR.nanmean2(got[k[:-1] + "r"], got[k[:-1] + "l"]), rtol=3e-7, atol=1e-30, equal_nan=True)


@pytest.fixture(scope="module")
def metric_batch():
    """B = 3, V = 778: both hands, the right hand only, the left hand only."""
    pred, targets = make_batch(3)
    targets["left_valid"][1] = 0
    targets["right_valid"][2] = 0
    pred["mano.v3d.cam.l"][1, 5, 0] = np.nan               # in an invalid hand: not read
    faces = _faces()
    return pred, targets, faces, _run(pred, targets, faces)


def test_metrics_b3_v778(metric_batch):
    pred, targets, faces, got = metric_batch
    check_metrics(got, SR.evaluate_surface(pred, targets, *faces), "B=3")
    assert np.isnan(got["p2s/pa/l"][1]) and np.isnan(got["chamfer/ra/r"][2]) and got["p2s/ra/h"][1] == got["p2s/ra/r"][1]
    r = got["p2s/pa/r"]
    assert 0.5 < r[0] < r[1] < 16.0 and (got["p2s/pa/r"][:2] < got["chamfer/pa/r"][:2]).all()      # the noise shows, mm
    assert (got["chamfer/ra/r"][:2] > got["chamfer/pa/r"][:2]).all()


def test_metrics_small_hands_and_nan_rules():
    """V = 5 with F = 3; an invalid sample, the right hand alone, the left hand alone; a constant prediction; a non-finite
    coordinate; no usable face."""
    rng = np.random.RandomState(11)
    B, V = 6, 5
    pred, targets = {}, {}
    for s in "rl":
        g = CENTRE + 0.05 * (rng.rand(B, V, 3) - 0.5)
        gj = CENTRE + 0.05 * (rng.rand(B, 21, 3) - 0.5)
        targets[f"mano.v3d.cam.{s}"], targets[f"mano.j3d.cam.{s}"] = np.float32(g), np.float32(gj)
        pred[f"mano.v3d.cam.{s}"] = np.float32(1.05 * g + 0.004 * rng.randn(B, V, 3))
        pred[f"mano.j3d.cam.{s}"] = np.float32(1.05 * gj + 0.004 * rng.randn(B, 21, 3))
    targets.update(is_valid=np.float32([1, 0, 1, 1, 1, 1]), right_valid=np.float32([1, 1, 1, 1, 1, 0]), left_valid=np.float32([1, 1, 1, 1, 0, 1]))
    pred["mano.v3d.cam.r"][1] = np.nan                                                 # is_valid = 0: not read
    pred["mano.v3d.cam.r"][2] = pred["mano.v3d.cam.r"][2, :1]                          # a constant prediction: pa is NaN
    targets["mano.v3d.cam.l"][3, 4, 2] = np.inf                                        # a non-finite vertex: the hand is NaN
    pred["mano.j3d.cam.r"][3, 20, 1] = np.nan                                          # a non-finite joint: the hand is NaN
    faces = (np.array([[0, 1, 2], [2, 3, 4], [0, 0, 4]]), np.array([[4, 3, 1], [0, 5, 2], [1, 1, 1]]))
    got = _run(pred, targets, faces)
    check_metrics(got, SR.evaluate_surface(pred, targets, *faces), "V=5")
    assert all(np.isnan(got[k][1]) for k in got)
    assert all(np.isnan(got[k][5]) if k[-1] == "r" else np.isfinite(got[k][5]) for k in got if "ra" in k)
    assert np.isnan(got["p2s/pa/r"][2]) and np.isnan(got["chamfer/pa/r"][2]) and np.isfinite(got["p2s/ra/r"][2])
    assert np.isnan(got["chamfer/ra/l"][3]) and np.isnan(got["p2s/ra/r"][3]) and np.isfinite(got["p2s/ra/r"][4])
    none = (np.array([[0, 1, 5]]), np.zeros((0, 3), np.int32))                         # no usable face: p2s NaN, chamfer stays
    got2 = _run(pred, targets, none)
    check_metrics(got2, SR.evaluate_surface(pred, targets, *none), "no face")
    for k in got:
        if k.startswith("chamfer"):
            assert (_bits(got)[k] == _bits(got2)[k]).all(), k
        else:
            assert np.isnan(got2[k]).all(), k


def test_face_lists_of_any_integer_type(metric_batch):
    pred, targets, faces, got = metric_batch
    one = lambda d: {k: v[:1] for k, v in d.items()}
    for conv in (lambda f: torch.from_numpy(np.int64(f)), lambda f: np.int16(f), lambda f: _cuda(np.int32(f))):
        again = _run(one(pred), one(targets), tuple(conv(f) for f in faces))
        assert all(_bits(again)[k][0] == _bits(got)[k][0] for k in got)
    from hands_amd import evaluate_surface_metrics
    meta = {"mano.faces.r": faces[0], "mano.faces.l": faces[1]}
    again = _bits({k: v.cpu().numpy() for k, v in evaluate_surface_metrics(_dev(one(pred)), _dev(one(targets)), meta).items()})
    assert all(again[k][0] == _bits(got)[k][0] for k in got)


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_batch_independent(metric_batch):
    pred, targets, faces, got = metric_batch
    base = _bits(got)
    again = _bits(_run(pred, targets, faces))
    assert all((again[k] == base[k]).all() for k in base)
    one = _bits(_run({k: v[:1] for k, v in pred.items()}, {k: v[:1] for k, v in targets.items()}, faces))
    assert all(one[k][0] == base[k][0] for k in base)
    verts, fc = np.float32(targets["mano.v3d.cam.l"]), faces[1]
    points = np.float32(pred["mano.v3d.cam.r"])
    a, b = _closest(points, verts, fc), _closest(points, verts, fc)
    alone = _closest(points[2:], verts[2:], fc)
    for x, y, z in zip(a, b, alone):
        assert x.tobytes() == y.tobytes() and x[2:].tobytes() == z.tobytes()


def test_graph_replay_has_the_eager_bits(metric_batch):
    from hands_amd import evaluate_surface_metrics
    pred, targets, faces, got = metric_batch
    p, t = _dev(pred), _dev(targets)
    fdev = tuple(_cuda(np.int32(f)) for f in faces)        # on the device already: nothing is copied under capture
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = evaluate_surface_metrics(p, t, faces=fdev)
    for v in out.values():
        v.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for k in got:
        assert (out[k].cpu().numpy().view(np.int32) == _bits(got)[k]).all(), k


# ---- 7. the field between the hands ----------------------------------------------------------------------------------------
def test_interhand_field():
    from hands_amd import interhand_field
    vr, fr = render_ref.ellipsoid_mesh(9, 16, radii=(0.045, 0.03, 0.09))
    vl, fl = render_ref.ellipsoid_mesh(8, 14, radii=(0.04, 0.03, 0.08))
    pad = lambda v, n: np.concatenate([v, np.tile(v[-1:], (n - len(v), 1))])            # both hands with the same vertex count
    n = max(len(vr), len(vl))
    rng = np.random.RandomState(5)
    v_r = np.float32(np.stack([pad(vr, n) + CENTRE + [0.0, 0.002 * b, 0.0] for b in range(3)]))
    v_l = np.float32(np.stack([pad(vl, n) @ _rot(rng.randn(3), 0.4).T + CENTRE + [0.06, 0.01 * b, -0.02] for b in range(3)]))
    valid = {"right_valid": np.float32([1, 1, 1]), "left_valid": np.float32([1, 0, 1]), "is_valid": np.float32([1, 1, 1])}
    d = {"mano.v3d.cam.r": _cuda(v_r), "mano.v3d.cam.l": _cuda(v_l), "mano.faces.r": fr, "mano.faces.l": fl, **_dev(valid)}
    bnd = 3e-3
    ref = SR.interhand_field(v_r, v_l, fr, fl, bnd, valid=[1, 0, 1])
    out = interhand_field(d)
    torch.cuda.synchronize()
    assert list(out) == ["dist.rl", "idx.rl", "contact.rl", "dist.lr", "idx.lr", "contact.lr"]
    for k in ("rl", "lr"):
        dist, idx, con = (out[f"{x}.{k}"].cpu().numpy() for x in ("dist", "idx", "contact"))
        assert dist.shape == idx.shape == con.shape == (3, n) and idx.dtype == con.dtype == np.int64
        assert np.isnan(dist[1]).all() and (idx[1] == -1).all() and (con[1] == 0).all()
        live = [0, 2]
        assert np.abs(dist[live] - ref["dist." + k][live]).max() <= BAR
        q, t, f = (v_r, v_l, fl) if k == "rl" else (v_l, v_r, fr)
        for b in live:
            assert (SR.distance_to_face(q[b], t[b], f, idx[b]) - ref["dist." + k][b]).max() <= BAR
        unsure = np.abs(ref["dist." + k][live] - bnd) <= BAR
        assert unsure.mean() <= 0.01                                                   # the scene: few vertices sit on the bound
        assert (con[live] == ref["contact." + k][live])[~unsure].all()
        assert 0 < con[live].sum() < con[live].size                                    # the hands touch and part
    lo, hi = 2e-3, 0.05
    clamped = interhand_field({k: v for k, v in d.items() if not k.endswith("valid")}, faces=(fr, fl), contact_bnd=bnd, dist_min=lo, dist_max=hi)
    rc = SR.interhand_field(v_r, v_l, fr, fl, bnd, lo, hi)
    for k in ("rl", "lr"):
        dist = clamped["dist." + k].cpu().numpy()
        assert dist.min() == np.float32(lo) and dist.max() == np.float32(hi) and np.abs(dist - rc["dist." + k]).max() <= BAR
        raw = rc["raw." + k]
        assert ((raw < lo).any() and (raw > hi).any())
        assert torch.equal(clamped["idx." + k][[0, 2]], out["idx." + k][[0, 2]])
        unsure = np.abs(rc["dist." + k] - bnd) <= BAR
        assert (clamped["contact." + k].cpu().numpy() == rc["contact." + k])[~unsure].all()


# ---- 8. the wrapper --------------------------------------------------------------------------------------------------------
def test_wrapper_surface_metrics(golden_dir, recipe_model):
    from hands_amd import evaluate_surface_metrics
    from hands_amd.metrics import SURF_KEYS
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
    today = ["imgname"] + ["metric." + k for k in ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l",
                                                   "pix_err/r", "pix_err/l", "pix_err/h")]
    out0, _ = w.forward(inputs, dict(targets), meta, "test")
    assert list(out0) == today
    w.metric_dict = w.metric_dict + ["surface"]
    out1, _ = w.forward(inputs, dict(targets), meta, "test")
    surf = ["metric." + k + "/" + s for k in SURF_KEYS for s in "rlh"]
    assert list(out1) == today + surf and len(surf) == 12
    for k in today[1:]:
        assert torch.equal(out0[k].view(torch.int32), out1[k].view(torch.int32)), k
    full = w.forward(inputs, dict(targets), meta, "extract")                          # what the metrics were computed from
    pred = {k[len("pred."):]: v.cuda() for k, v in full.items() if k.startswith("pred.") and torch.is_tensor(v)}
    tgt = {k[len("targets."):]: v.cuda() for k, v in full.items() if k.startswith("targets.") and torch.is_tensor(v)}
    direct = evaluate_surface_metrics(pred, tgt, faces=(w.model.mano_r.faces, w.model.mano_l.faces))
    for k in SURF_KEYS:
        for s in "rlh":
            a, b = out1[f"metric.{k}/{s}"], direct[f"{k}/{s}"].cpu()
            assert a.device.type == "cpu" and a.shape == (B,) and torch.equal(a.view(torch.int32), b.view(torch.int32)), (k, s)
    assert torch.isnan(out1["metric.p2s/pa/l"][1]) and torch.equal(out1["metric.p2s/pa/h"][1], out1["metric.p2s/pa/r"][1])
    assert bool(torch.isfinite(out1["metric.chamfer/pa/h"]).all()) and bool(torch.isfinite(out1["metric.p2s/ra/r"]).all())
