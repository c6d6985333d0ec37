"""MANO fitting to surface correspondences and the ICP loop without a GPU: the fp64 restatement tests/fit_surf_ref.py of DESIGN.md
section 7 ("MANO fitting to surface correspondences and ICP registration") against central differences, against the vertex
fit's restatement and against its own closest points, its convergence on a tube hand (tests/surface_asset.py), and the host
side of hands_amd.fitting (names, ABI, the two configurations, the argument rules)."""
import os
import re

import numpy as np
import pytest
import torch

import fit_surf_ref as S
import fit_verts_ref as V
import hands_amd
import surface_ref as SR
from hands_amd import _lib
from hands_amd.mano import synthetic_mano_asset
from surface_asset import tube_hand_asset

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ASSETS = {"r": synthetic_mano_asset(True), "l": synthetic_mano_asset(False), "tube": tube_hand_asset(True)}
CONSTS = {h: V.consts_from_asset(a) for h, a in ASSETS.items()}
SEEDS = (0, 1, 2, 3)
# The restatement's loop on the tube hand, registration_case(seed, P = 512), 10 rounds of 3 iterations, seeds 0..3 (measured;
# DESIGN.md section 7 records them): rms cloud-to-surface distance 3.32 / 3.72 / 3.61 / 4.22 mm at the start;
# tangent_weight 1: 0.558 / 0.493 / 0.313 / 0.413 mm at the end; tangent_weight 0.1: 0.232 / 0.167 / 0.224 / 0.203 mm.
# The tests hold 4 x the largest, as the other fits' tests do.
END_MAX = {1.0: 4 * 0.558e-3, 0.1: 4 * 0.232e-3}
_RUNS = {}


def tube_run(seed, tau):
    """The loop on the tube hand, computed once per (seed, tangent_weight)."""
    if (seed, tau) not in _RUNS:
        C, faces = CONSTS["tube"], ASSETS["tube"].faces
        pts, start, truth = S.registration_case(C, faces, seed, 512)
        out = S.register(C, faces, pts, start, rounds=10, iters=3, tangent_weight=tau)
        _RUNS[(seed, tau)] = (pts, out, S.cloud_distance(pts, out["verts"].astype(np.float64), faces))
    return _RUNS[(seed, tau)]


@pytest.mark.parametrize("side", ["r", "tube"])
def test_row_jacobian_matches_central_differences(side):
    """d c_k / d theta of 50 rows against central differences (h = 1e-6) of the restatement's own surface points: 1e-9, the
    tolerance of tests/test_fit_verts.py (truncation h^2 / 6 = 1.7e-13 and rounding 1e-16 / h = 1e-10 for entries <= 1; a
    row is a convex combination of vertex rows)."""
    C, faces = CONSTS[side], np.asarray(ASSETS[side].faces)
    _, f, b, (R, beta, _) = S.surface_case(C, faces, 3, 50)
    tri, b = faces[f], b.astype(np.float64)
    D = S.row_jacobian(C, R, V.evaluate(C, R, beta), tri, b)
    h, num = 1e-6, np.zeros((50, 3, 61))
    for u in range(61):
        def at(sign):
            d = np.zeros(61)
            d[u] = sign * h
            R2 = np.stack([R[j] @ V.exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            return S.surface_points(V.vertices_of(C, R2, beta + d[48:58]), tri, b) + d[58:61]
        num[:, :, u] = (at(1.0) - at(-1.0)) / (2 * h)
    err = np.abs(D - num).max()
    print(f"FITS|jacobian|{side}|{err:.3e}|1e-9|largest entry {np.abs(D).max():.3f}")
    assert np.abs(D).max() <= 1.0 + 1e-12 and err <= 1e-9


def vertex_rows(faces):
    """Per vertex n a face that holds it and the unit coefficients that name it there; ``has`` (778): such a face exists."""
    faces = np.asarray(faces, np.int64)
    f, b, has = np.zeros(V.NV, np.int64), np.zeros((V.NV, 3), np.float32), np.zeros(V.NV, bool)
    for i in (2, 1, 0):                                                # the first place wins
        for k in range(len(faces) - 1, -1, -1):
            n = faces[k, i]
            f[n], b[n], has[n] = k, np.eye(3, dtype=np.float32)[i], True
    return f, b, has


@pytest.mark.parametrize("side", ["r", "tube"])
def test_unit_coefficients_are_the_vertex_fit(side):
    """Rows b = e_i on a face whose i-th vertex is n, one per vertex, tangent_weight 1: cost, gradient and the state after four
    iterations equal fit_verts_ref's to summation-order rounding (1e-12 of the largest entry; the state 1e-9).  The tube hand
    names all 778 vertices; the synthetic asset's random faces miss a few, which get weight 0 in both fits."""
    C, faces = CONSTS[side], np.asarray(ASSETS[side].faces)
    f, b, has = vertex_rows(faces)
    assert has.all() if side == "tube" else has.sum() >= 760
    y, _, (R, beta, t) = V.family_case(C, 5)
    w = has.astype(np.float32)
    cfg, cfgv = S.config(iters=4), V.config(iters=4)
    R0, beta0, t0 = V.near((R, beta, t), np.random.RandomState(1))
    rows = (faces[f[has]], b[has].astype(np.float64), y[has].astype(np.float64), w[has].astype(np.float64), S.row_matrices(None, 1.0, int(has.sum())))
    rs, Js = S.residual(C, R0, beta0, t0, rows, cfg), S.jacobian(C, R0, beta0, rows, cfg)
    yz = np.where(has[:, None], y.astype(np.float64), 0.0)
    rv, Jv = V.residual(C, R0, beta0, t0, yz, w.astype(np.float64), cfgv), V.jacobian(C, R0, beta0, w.astype(np.float64), cfgv)
    cs, cv, gs, gv = rs @ rs, rv @ rv, Js.T @ rs, Jv.T @ rv
    print(f"FITS|unit|{side}|cost {abs(cs - cv) / cv:.2e}|gradient {np.abs(gs - gv).max() / np.abs(gv).max():.2e}")
    assert abs(cs - cv) <= 1e-12 * cv and np.abs(gs - gv).max() <= 1e-12 * np.abs(gv).max()
    init = tuple(np.asarray(a, np.float32) for a in (R0, beta0, t0))
    a = S.fit(C, faces, y, f, b, w, None, None, init, cfg)
    v = V.fit(C, y, w, None, init, cfgv)
    assert a["steps"] == v["steps"] >= 3
    for k in ("pose", "beta", "transl", "rmse", "j3d"):
        assert np.abs(np.asarray(a["raw"][k]) - np.asarray(v["raw"][k])).max() <= 1e-9, k
    assert np.abs(a["raw"]["verts"] - (V.vertices_of(C, a["raw"]["pose"], a["raw"]["beta"]) + a["raw"]["transl"])).max() == 0.0


def test_normals_at_tangent_weight_one_change_no_bit():
    C, faces = CONSTS["r"], ASSETS["r"].faces
    y, f, b, _ = S.surface_case(C, faces, 11, 40)
    n = np.random.RandomState(2).randn(40, 3).astype(np.float32)
    n[7] = np.nan                                                      # not read
    a, c = S.fit(C, faces, y, f, b, cfg=S.config(iters=3)), S.fit(C, faces, y, f, b, normals=n, cfg=S.config(iters=3))
    for k in ("pose", "beta", "transl", "rmse", "j3d", "verts"):
        assert np.array_equal(np.asarray(a["raw"][k]), np.asarray(c["raw"][k])), k
    assert a["steps"] == c["steps"]
    n[7] = 0.0
    d = S.fit(C, faces, y, f, b, normals=n, cfg=S.config(iters=3, tangent_weight=0.25))
    assert np.abs(d["raw"]["pose"] - a["raw"]["pose"]).max() > 1e-6    # and below one they matter


def test_tangent_weight_zero_annihilates_tangential_displacement():
    rng = np.random.RandomState(4)
    n = rng.randn(20, 3)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[3] = 0.0                                                         # a zero normal: A = I
    A = S.row_matrices(n, 0.0, 20)
    e = rng.randn(20, 3)
    tang = e - n * (n * e).sum(1, keepdims=True)
    out = np.einsum("kab,kb->ka", A, tang)
    assert np.abs(np.delete(out, 3, 0)).max() <= 1e-15 and np.array_equal(out[3], tang[3])
    assert np.abs(np.einsum("kab,kb->ka", A, n) - n).max() <= 1e-15
    half = S.row_matrices(n, 0.25, 20)                                  # sqrt(tau) on the tangential part
    assert np.abs(np.delete(np.einsum("kab,kb->ka", half, tang) - 0.5 * tang, 3, 0)).max() <= 1e-15


@pytest.mark.parametrize("side", ["r", "tube"])
def test_coefficients_reproduce_the_closest_point(side):
    """sum_i b_i v_i of the restated coefficients is the restated closest point (1e-12 m: fp64 rounding at a hand's size); the
    coefficients of a point are non-negative and add up to one; the normal is a unit vector or zero."""
    asset = ASSETS[side]
    C = CONSTS[side]
    _, _, (R, beta, t) = V.family_case(C, 9)
    verts = V.vertices_of(C, R, beta) + t
    rng = np.random.RandomState(6)
    pts = verts[rng.randint(0, 778, 200)] + 0.01 * rng.randn(200, 3)
    w = np.ones(200)
    w[[5, 17]] = 0.0
    pts[5] = np.nan
    cor = S.correspond(pts, verts, asset.faces, w, max_dist=0.015)
    has = cor["face_idx"] >= 0
    assert has.sum() == 198 and not has[5] and cor["weights"][5] == 0 and np.isnan(cor["bary"][5]).all()
    tri = verts[np.asarray(asset.faces)[cor["face_idx"][has]]]
    back = np.einsum("ki,kic->kc", cor["bary"][has], tri)
    err = np.abs(back - cor["closest"][has]).max()
    print(f"FITS|bary|{side}|{err:.3e}|1e-12")
    assert err <= 1e-12
    assert (cor["bary"][has] >= -1e-12).all() and np.abs(cor["bary"][has].sum(1) - 1).max() <= 1e-12
    nn = np.linalg.norm(cor["normal"][has], axis=1)
    assert (np.isclose(nn, 1.0, atol=1e-12) | (nn == 0)).all()
    assert np.array_equal(cor["weights"] > 0, has & (cor["dist"] <= 0.015)) and (cor["weights"] > 0).sum() not in (0, 198)
    d, i, c = SR.closest_on_mesh_1(pts[has], verts, asset.faces)
    assert np.array_equal(d, cor["dist"][has]) and np.array_equal(i, cor["face_idx"][has])


def test_the_truth_is_a_fixed_point_of_the_loop():
    """A noise-free cloud sampled from the model's own surface, init = the truth, no priors: the loop stays where it is.  The
    cloud's fp32 rounding is 3e-8 m at 0.6 m; the bar on the vertices' movement and on the final distance is 1e-6 m."""
    C, faces = CONSTS["tube"], ASSETS["tube"].faces
    pts, _, (R, beta, t) = S.registration_case(C, faces, 5, 256)
    init = tuple(np.asarray(a, np.float32) for a in (R, beta, t))
    v0 = V.vertices_of(C, *(a.astype(np.float64) for a in init[:2])) + init[2].astype(np.float64)
    out = S.register(C, faces, pts, init, rounds=3, iters=3, lambda_beta=0.0, lambda_pose=0.0)
    move, end = np.abs(out["raw"]["verts"] - v0).max(), S.cloud_distance(pts, out["verts"].astype(np.float64), faces)
    print(f"FITS|fixed point|moved {move:.3e} m|distance {end:.3e} m|1e-6")
    assert out["rounds_done"] == 3 and move <= 1e-6 and end <= 1e-6


@pytest.mark.parametrize("tau", [1.0, 0.1])
@pytest.mark.parametrize("seed", SEEDS)
def test_the_loop_converges_on_the_tube_hand(seed, tau):
    """512 points uniform on the posed tube hand, the start 0.05 rad per joint, 0.1 in beta and 5 mm off: after 10 rounds of 3
    iterations the rms cloud-to-surface distance is below its start and below 4 x the largest value measured (END_MAX).  No
    vertex recovery is claimed: a round tube does not observe twist."""
    pts, out, end = tube_run(seed, tau)
    h = out["history"]
    print(f"FITS|converge|seed {seed}|tau {tau}|start {h[0] * 1e3:.3f} mm|end {end * 1e3:.4f} mm|bar {END_MAX[tau] * 1e3:.3f} mm")
    assert out["rounds_done"] == 10 and end < h[0] and end <= END_MAX[tau]
    assert all(b <= a for a, b in zip(h, h[1:]))                       # monotone from round to round


def test_names_are_exported_and_the_abi():
    for name in ("SurfaceFitConfig", "fit_mano_surface", "fit_mano_hands_surface", "correspond_on_mesh", "RegisterConfig",
                 "register_mano", "register_mano_hands", "register_predictions"):
        assert name in hands_amd.__all__ and hasattr(hands_amd, name)
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"\bint hands_mano_fit_surf_f32\(const hands_mano_fit_surf_side\* sides, int n_sides, const hands_fit_surf_cfg\* "
                     r"cfg, int B, int P,\s+hands_stream_t stream\);", header)
    assert re.search(r"\bint hands_mesh_correspond_f32\(", header) and "#define HANDS_FIT_SURF_MAX_P 16384" in header
    for struct in ("hands_mano_fit_surf_consts", "hands_mano_fit_surf_side", "hands_fit_surf_cfg", "hands_fit_cfg"):
        assert f"}} {struct};" in header
    assert len(_lib.SIGNATURES["hands_mano_fit_surf_f32"]) == 6 and len(_lib.SIGNATURES["hands_mesh_correspond_f32"]) == 17
    assert [n for n, _ in _lib.FitCfg._fields_] == ["iters", "lambda_beta", "lambda_pose", "mu0"]       # shared by three entries
    assert [n for n, _ in _lib.FitSurfCfg._fields_] == ["iters", "lambda_beta", "lambda_pose", "mu0", "tangent_weight"]
    assert [n for n, _ in _lib.ManoFitSurfSide._fields_] == [
        "consts", "points", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps",
        "j3d", "verts", "face_idx", "bary", "normals"]
    assert [n for n, _ in _lib.ManoFitSurfConsts._fields_][-1] == "faces"
    mk = open(os.path.join(ROOT, "hands_amd", "csrc", "Makefile")).read()
    assert "fit_surf.hip" in mk and "mesh_correspond.hip" in mk and "fit_mesh_device.h" in mk
    assert hands_amd.fitting.MAX_SURFACE_ROWS == 16384
    from hands_amd.packing import pack_mano
    p = pack_mano(ASSETS["tube"], "cpu")
    assert p["faces_i32"].dtype == torch.int32 and torch.equal(p["faces_i32"].long(), p["faces"])


def test_configurations_and_argument_rules():
    """A bad configuration is a ValueError before anything else is looked at; a good one gets as far as the device rule."""
    from hands_amd import RegisterConfig, SurfaceFitConfig
    assert SurfaceFitConfig() == SurfaceFitConfig(30, 1e-6, 1e-6, 1e-3, 1.0)
    assert RegisterConfig() == RegisterConfig(10, 3, 1e-6, 1e-6, 1e-3, 0.1, 0.0)
    y, f, b = torch.zeros(1, 8, 3), torch.zeros(1, 8, dtype=torch.int32), torch.zeros(1, 8, 3)
    init = (torch.eye(3).repeat(1, 16, 1, 1), torch.zeros(1, 10), torch.zeros(1, 3))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(iters=-1), dict(iters=2.5), dict(lambda_beta=-1e-9), dict(lambda_pose=nan), dict(mu0=inf),
                dict(tangent_weight=1.5), dict(tangent_weight=-0.1), dict(tangent_weight=nan)):
        with pytest.raises(ValueError):
            hands_amd.fit_mano_surface(y, f, b, None, config=SurfaceFitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_mano_hands_surface(y, f, b, y, f, b, None, config=SurfaceFitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.register_mano(y, None, init=init, config=RegisterConfig(**bad))
    for bad in (dict(rounds=-1), dict(rounds=1.5), dict(max_dist=nan)):
        with pytest.raises(ValueError):
            hands_amd.register_mano(y, None, init=init, config=RegisterConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.register_mano_hands(y, y, None, init, init, config=RegisterConfig(**bad))
    with pytest.raises(ValueError, match="ICP is local"):              # the registration needs a start
        hands_amd.register_mano(y, None)
    with pytest.raises(ValueError, match="ICP is local"):
        hands_amd.register_mano_hands(y, y, None, init_r=init)
    with pytest.raises(ValueError, match="max_dist"):
        RegisterConfig(max_dist=nan).fit_config()
    for call in (lambda: hands_amd.fit_mano_surface(y, f, b, None, config=SurfaceFitConfig(iters=0, tangent_weight=0.0)),
                 lambda: hands_amd.register_mano(y, None, init=init),
                 lambda: hands_amd.correspond_on_mesh(y, y, f)):
        with pytest.raises(RuntimeError, match="HIP device only"):
            call()
