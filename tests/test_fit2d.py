"""MANO fitting to 2-D keypoints without a GPU: the fp64 restatement tests/fit2d_ref.py of DESIGN.md section 7 ("MANO fitting to
2-D keypoints") against central differences and its own rules, and the host side of hands_amd.fitting (names, ABI, Fit2DConfig)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import fit2d_ref as G
import fit_ref as F
import hands_amd
from hands_amd import _lib
from hands_amd.fitting import Fit2DConfig
from hands_amd.mano import synthetic_mano_asset

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ASSETS = {"r": synthetic_mano_asset(True), "l": synthetic_mano_asset(False)}
CONSTS = {h: F.consts_from_asset(a) for h, a in ASSETS.items()}
K = G.K_TEST


def _perturbed(C, seed):
    y, w, (R, beta, t) = G.family_case(C, seed)
    rng = np.random.RandomState(seed)
    R = np.stack([R[j] @ F.exp_so3(0.1 * rng.randn(3)) for j in range(16)])
    y = np.where((w > 0)[:, None], y.astype(np.float64), 0.0) + rng.randn(21, 2)          # a residual of about a pixel
    return y, w.astype(np.float64), R, beta + 0.1 * rng.randn(10), t + 0.01 * rng.randn(3)


@pytest.mark.parametrize("sigma", [0.0, 30.0])
@pytest.mark.parametrize("side", ["r", "l"])
def test_jacobian_matches_central_differences(side, sigma):
    """The 42 data rows s_k P_k D_k against central differences of s_k e_k with s_k held (h = 1e-6), and J^T r against half the
    central-difference gradient of the data cost sum rho_k -- with sigma > 0 that is the property the row scaling is chosen
    for.  Bars, from the sizes involved: first derivatives of a pixel coordinate reach f / Z = 1.7e3 (per metre of translation),
    second ones 2 f / Z^2 = 5.6e3, third ones 6 f / Z^3 = 2.8e4, pixel values 3e2.  One difference of e carries a rounding of
    3e2 * 2^-52 / 2e-6 = 3e-8 and a truncation of h^2 / 6 * 2.8e4 = 5e-9: 1e-6 absolute on J.  The cost's third derivative is
    at most 6 sum_k |e_k'| |e_k''| = 6 * 42 * 1.7e3 * 5.6e3 = 2.4e9, so the gradient's difference carries a truncation of up to
    h^2 / 6 * 2.4e9 = 4e-4 (its rounding, 1e2 * 2^-52 / 2e-6 = 1e-8, is nothing beside it): 1e-3 absolute, at gradient entries
    of 1e3 to 1e4 -- a wrong factor or sign in the row scaling shows as an error of that size.  Measured: 1.0e-7 on J, 2.0e-4 on
    the gradient."""
    C = F.consts_from_asset(ASSETS[side], rounded=False)
    cfg = G.config(lambda_beta=0.0, lambda_pose=0.0, robust_sigma=sigma)
    prior = (np.zeros(10), C.M)
    for seed in (3, 8):                                   # seed 3 has five keypoints of weight 0
        y, w, R, beta, t = _perturbed(C, seed)
        S = G.state(C, R, beta, t, y, w, K, cfg, prior)
        Jm = G.data_jacobian(C, R, beta, w, K, S)

        def at(d):
            R2 = np.stack([R[j] @ F.exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            return G.state(C, R2, beta + d[48:58], t + d[58:61], y, w, K, cfg, prior)
        h, num, grad = 1e-6, np.zeros_like(Jm), np.zeros(G.NU)
        for i in range(G.NU):
            e = np.zeros(G.NU)
            e[i] = h
            a, b = at(e), at(-e)
            num[:, i] = (S["s"][:, None] * (a["e"] - b["e"])).reshape(42) / (2 * h)
            grad[i] = (a["c"] - b["c"]) / (2 * h)
        _, g = G.normal_equations(Jm, S, cfg, G.frozen(1, cfg))
        err, gerr = np.abs(Jm - num).max(), np.abs(g - 0.5 * grad).max()
        print(f"FIT2D|jacobian|{side}{seed} sigma {sigma}|{err:.3e}|1e-6|gradient {gerr:.3e}|1e-3|largest {np.abs(Jm).max():.3e} {np.abs(g).max():.3e}")
        assert err <= 1e-6 and gerr <= 1e-3 and np.abs(g).max() >= 1e2
        assert not Jm[np.repeat(w == 0, 2)].any()         # a keypoint of weight 0 has no rows
        if sigma > 0:
            assert (S["s"][w > 0] < np.sqrt(w[w > 0])).all()


def test_the_24_start_matrices():
    Gs = G.START
    assert len(Gs) == 24
    for M in Gs:
        assert np.array_equal(M @ M.T, np.eye(3)) and round(np.linalg.det(M)) == 1 and set(np.unique(M)) <= {-1.0, 0.0, 1.0}
    assert len({M.tobytes() for M in Gs}) == 24
    perms = [tuple(int(np.flatnonzero(M[i])[0]) for i in range(3)) for M in Gs]
    assert perms == [p for p in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)] for _ in range(4)]
    signs = [(M[0].sum(), M[1].sum()) for M in Gs]
    assert signs == [(1, 1), (1, -1), (-1, 1), (-1, -1)] * 6
    assert np.array_equal(Gs[0], np.eye(3)) and np.array_equal(Gs[7], np.array([[-1.0, 0, 0], [0, 0, -1], [0, -1, 0]]))


@pytest.mark.parametrize("side", ["r", "l"])
def test_the_start_rule_finds_the_rotation_the_hand_was_projected_from(side):
    """The rest hand under each G_c at 0.6 m: candidate c wins, R_0 = G_c, the other rotations are M_j, beta = 0, and the state
    re-projects within the weak-perspective error of a hand that reaches 0.1 m from its wrist at that depth: offsets of up to
    0.1 * 1000 / 0.6 = 167 px, each wrong by at most 0.1 / 0.6 of itself, 28 px -- the bar is 30 px."""
    C = CONSTS[side]
    w = np.ones(21)
    for c, Gc in enumerate(G.START):
        R = F.rest_pose(C)
        R[0] = Gc
        y = G.project(K, F.joints_of(C, R, np.zeros(10)) + np.array([0.03, -0.02, 0.6]))
        got = G.start_state(C, y, w, K)
        assert got is not None and got[0] == c, (c, got and got[0])
        assert np.array_equal(got[1][0], Gc) and np.array_equal(got[1][1:], C.M[1:]) and not got[2].any()
        r = G.fit(C, y.astype(np.float32), K, cfg=G.config(iters_rigid=0, iters=0))
        assert r["start"] == c and r["steps"] == 0 and float(r["rmse"]) < 30.0
        assert abs(r["raw"]["transl"][2] + C.J_template[0, 2] - 0.6) < 0.1
    few = np.zeros(21)
    few[[0, 4, 9, 18]] = 1.0
    assert G.start_state(C, np.tile(y[:1], (21, 1)), few, K) is None          # coincident keypoints: s = 0, no candidate
    assert np.isnan(G.fit(C, np.tile(y[:1], (21, 1)), K, few)["rmse"])


def test_frozen_unknowns_keep_their_bits():
    C = CONSTS["r"]
    y, w, init = G.step_parity_inputs(C, 100, True)
    r = G.fit(C, y[0], K, w[0], init=tuple(a[0] for a in init), cfg=G.config(iters_rigid=4, iters=0))
    assert r["steps"] >= 2 and len(r["trace"]) == 4
    assert np.array_equal(r["pose"][1:].view(np.int32), init[0][0][1:].view(np.int32))
    assert np.array_equal(r["beta"].view(np.int32), init[1][0].view(np.int32))
    assert not np.array_equal(r["pose"][0], init[0][0][0]) and not np.array_equal(r["transl"], init[2][0])
    r = G.fit(C, y[0], K, w[0], init=tuple(a[0] for a in init), cfg=G.config(iters_rigid=0, iters=4, fit_shape=False))
    assert r["steps"] >= 2 and np.array_equal(r["beta"].view(np.int32), init[1][0].view(np.int32))
    assert not np.array_equal(r["pose"][1:], init[0][0][1:])
    for stage, free in ((0, [0, 1, 2, 58, 59, 60]), (1, list(range(61)))):
        assert list(np.flatnonzero(~G.frozen(stage, G.config()))) == free
    assert list(np.flatnonzero(G.frozen(1, G.config(fit_shape=False)))) == list(range(48, 58))


def test_stages_restart_the_damping_and_count_every_iteration():
    C = CONSTS["l"]
    y, w, _ = G.family_case(C, 2)
    r = G.fit(C, y, K, w, cfg=G.config(iters_rigid=3, iters=5))
    assert len(r["trace"]) == 8 and r["steps"] == sum(1 for t in r["trace"] if t[3])
    cur = r["trace"][0][0]
    for c, c2, ok, acc in r["trace"]:
        assert c == cur
        if acc:
            assert ok and c2 < c
            cur = c2


def test_prior_to_init_changes_the_cost_as_specified():
    C = CONSTS["r"]
    y, w, init = G.step_parity_inputs(C, 100, True)
    i0 = tuple(a[0] for a in init)
    R, beta = i0[0].astype(np.float64), i0[1].astype(np.float64)
    mean = G.fit(C, y[0], K, w[0], init=i0, cfg=G.config(iters_rigid=0, iters=1))
    own = G.fit(C, y[0], K, w[0], init=i0, cfg=G.config(iters_rigid=0, iters=1, prior_to_init=True))
    lg = np.concatenate([F.log_so3(C.M[j].T @ R[j]) for j in range(1, 16)])
    prior = 1e-2 * float(beta @ beta) + 1e-2 * float(lg @ lg)
    assert prior > 1e-3 and abs(mean["trace"][0][0] - own["trace"][0][0] - prior) <= 1e-12 * mean["trace"][0][0]
    # without a caller's state the flag changes nothing
    a = G.fit(C, y[0], K, w[0], cfg=G.config(iters_rigid=1, iters=1))
    b = G.fit(C, y[0], K, w[0], cfg=G.config(iters_rigid=1, iters=1, prior_to_init=True))
    assert a["trace"] == b["trace"]


def test_the_depth_guard():
    C = CONSTS["r"]
    y, w, init = G.step_parity_inputs(C, 100, True)
    i0 = tuple(a[0] for a in init)
    zmin_state = float((F.joints_of(C, i0[0].astype(np.float64), i0[1].astype(np.float64)) + i0[2])[w[0] > 0, 2].min())
    S = G.state(C, i0[0].astype(np.float64), i0[1].astype(np.float64), i0[2].astype(np.float64),
                np.nan_to_num(y[0].astype(np.float64)), w[0].astype(np.float64), K, G.config(z_min=zmin_state), (np.zeros(10), C.M))
    assert math.isinf(S["c"]) and S["c"] > 0                               # Z == z_min is not in front of it
    assert np.isnan(G.fit(C, y[0], K, w[0], init=i0, cfg=G.config(z_min=zmin_state))["rmse"])       # as the initial state
    # as a candidate: the wrist is pulled towards a target behind z_min; every such candidate is a rejected step
    far = y[0].copy()
    far[w[0] > 0] = (far[w[0] > 0] - 112.0) * 3.0 + 112.0                    # three times as large: the fit wants a third of the depth
    r = G.fit(C, far, K, w[0], init=i0, cfg=G.config(iters_rigid=6, iters=0, z_min=zmin_state - 0.1))
    assert any(math.isinf(c2) for _, c2, _, _ in r["trace"])
    assert all(not acc for _, c2, _, acc in r["trace"] if math.isinf(c2))
    assert r["raw"]["j3d"][w[0] > 0, 2].min() > zmin_state - 0.1 and np.isfinite(r["rmse"])


def test_rows_that_are_not_fitted():
    C = CONSTS["r"]
    y, w, (R, beta, t) = G.family_case(C, 1)
    few = np.zeros(21, np.float32)
    few[:3] = 1.0
    nan_y = y.copy()
    nan_y[4, 1] = np.nan
    good_init = (R.astype(np.float32), beta.astype(np.float32), t.astype(np.float32))
    bad_init = (R.astype(np.float32), np.full(10, np.inf, np.float32), t.astype(np.float32))
    behind = (good_init[0], good_init[1], np.array([0.0, 0.0, 0.01], np.float32))
    Kn, K0, K1, Ki = K.copy(), K.copy(), K.copy(), K.copy()
    Kn[0, 1], K0[0, 0], K1[1, 1], Ki[1, 2] = np.nan, 0.0, -1000.0, np.inf
    K2 = K.copy()
    K2[2] = np.nan                                                         # row 2 is never read
    rows = [G.fit(C, y, K, w, valid=0.0), G.fit(C, y, K, few), G.fit(C, nan_y, K, w), G.fit(C, y, K, w, init=bad_init),
            G.fit(C, y, K, w, init=behind), G.fit(C, y, Kn, w), G.fit(C, y, K0, w), G.fit(C, y, K1, w), G.fit(C, y, Ki, w)]
    for r in rows:
        assert r["steps"] == 0 and r["start"] == -1 and np.isnan(r["rmse"]) and not r["beta"].any() and not r["transl"].any()
        assert np.array_equal(r["pose"], C.M.astype(np.float32)) and np.isnan(r["j3d"]).all() and np.isnan(r["j2d"]).all()
        assert r["j3d"].shape == (21, 3) and r["j2d"].shape == (21, 2)
    cfg = G.config(iters_rigid=2, iters=2)
    ok = G.fit(C, y, K2, w, cfg=cfg)
    assert np.isfinite(ok["rmse"]) and ok["start"] >= 0
    assert np.isfinite(G.fit(C, y, K, w, init=good_init, cfg=cfg)["rmse"])
    w0 = w.copy()
    w0[4] = 0.0
    a, b = G.fit(C, nan_y, K, w0, cfg=cfg), G.fit(C, y, K, w0, cfg=cfg)
    assert np.isfinite(a["rmse"]) and all(np.array_equal(a[k], b[k]) for k in ("pose", "beta", "transl", "rmse"))
    assert a["start"] == b["start"] and np.array_equal(a["j3d"], b["j3d"])  # all 21 joints are reported, the unweighted too


def test_no_tie_decides_a_branch_on_the_parity_inputs():
    """Every accept / reject decision of the restatement on the inputs of the GPU step-parity test has a margin above 1e-9 of
    the cost, every factorisation succeeds, and the start candidate wins by a clear margin."""
    for C, base, with_init in ((CONSTS["r"], 100, True), (CONSTS["l"], 200, False)):
        y, w, init = G.step_parity_inputs(C, base, with_init)
        Ks = np.repeat(K[None], 5, 0)
        for sigma, shape in ((0.0, True), (30.0, True), (0.0, False)):
            cfg = G.config(iters_rigid=2, iters=3, robust_sigma=sigma, fit_shape=shape, prior_to_init=with_init)
            rows = G.fit_rows(C, y, Ks, w, init=init, cfg=cfg)
            assert all(G.margins_ok(r) for r in rows)
            assert all((r["start"] >= 0) != with_init for r in rows)


def test_recorded_figures_of_the_family():
    """Seeds 0..15 at the default configuration: the figures DESIGN.md and Fit2DConfig state -- median 7.2e-3 px, maximum 2.0
    px, 3 of the 16 above 1 px, none above 2.5 px."""
    rm = sorted(float(r["rmse"]) for r in G.default_family(CONSTS["r"]))
    print("FIT2D|family rmse px|min %.3e|median %.3e|max %.3e|above 1 px: %d" % (rm[0], float(np.median(rm)), rm[-1],
                                                                                 sum(x > 1.0 for x in rm)))
    assert 1.0e-3 <= rm[0] <= 1.5e-3 and 6.5e-3 <= float(np.median(rm)) <= 8.0e-3 and 1.9 <= rm[-1] <= 2.1
    assert sum(x > 1.0 for x in rm) == 3
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "median 7.2e-3 px" in doc and "maximum 2.0 px" in doc and "3 of the 16" in doc


def test_the_full_run_seeds_qualify():
    """The 8 seeds of the GPU full-run test at 6 + 14 iterations: every decision above 1e-9 c, the twin takes the same steps on
    at least 7."""
    _, _, ref, twin = G.full_run_reference(CONSTS["r"])
    assert all(G.margins_ok(r) for r in ref)
    assert sum(a["steps"] == b["steps"] for a, b in zip(ref, twin)) >= 7


def test_names_are_exported_and_the_abi():
    for name in ("Fit2DConfig", "fit_mano_2d", "fit_mano_hands_2d", "fit_targets_2d", "refine_predictions"):
        assert name in hands_amd.__all__ and hasattr(hands_amd, name)
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"\bint hands_mano_fit2d_f32\(const hands_mano_fit2d_side\* sides, int n_sides, const float\* K, "
                     r"const hands_fit2d_cfg\* cfg, int B,\s+hands_stream_t stream\);", header)
    for struct in ("hands_mano_fit2d_side", "hands_fit2d_cfg"):
        assert f"}} {struct};" in header
    assert len(_lib.SIGNATURES["hands_mano_fit2d_f32"]) == 6
    assert [n for n, _ in _lib.ManoFit2DSide._fields_] == ["consts", "kp2d", "weights", "valid", "init_pose", "init_beta",
                                                           "init_transl", "pose", "beta", "transl", "rmse", "steps", "start",
                                                           "j3d", "j2d"]
    assert [n for n, _ in _lib.Fit2DCfg._fields_] == ["iters_rigid", "iters", "lambda_beta", "lambda_pose", "mu0", "robust_sigma",
                                                      "z_min", "fit_shape", "prior_to_init"]
    from hands_amd.wrapper import HandsWrapper
    assert "fit_gt_2d" in open(os.path.join(ROOT, "hands_amd", "wrapper.py")).read() and HandsWrapper is not None


def test_fit2d_config_validation():
    c = Fit2DConfig().c_struct()
    assert (c.iters_rigid, c.iters, c.lambda_beta, c.lambda_pose, c.mu0, c.robust_sigma, c.z_min, c.fit_shape, c.prior_to_init) == \
        (10, 30, 1e-2, 1e-2, 1e-3, 0.0, 0.05, 1, 0)
    z = Fit2DConfig(iters_rigid=0, iters=0, lambda_beta=0.0, lambda_pose=0.0, mu0=0.0, fit_shape=False, prior_to_init=True).c_struct()
    assert (z.iters_rigid, z.iters, z.fit_shape, z.prior_to_init) == (0, 0, 0, 1)
    for bad in (dict(iters=-1), dict(iters_rigid=-1), dict(iters=2.5), dict(iters_rigid=0.5), dict(lambda_beta=-1e-9),
                dict(lambda_pose=float("nan")), dict(mu0=float("inf")), dict(robust_sigma=-1.0), dict(robust_sigma=float("nan")),
                dict(robust_sigma=float("inf")), dict(z_min=0.0), dict(z_min=-0.1), dict(z_min=float("nan")), dict(z_min=float("inf"))):
        with pytest.raises(ValueError):
            Fit2DConfig(**bad).c_struct()
    with pytest.raises(Exception):
        Fit2DConfig().iters = 3                                            # frozen


def test_fitting_2d_refuses_cpu_tensors():
    K1 = torch.eye(3)[None]
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano_2d(torch.zeros(1, 21, 2), K1, None)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano_hands_2d(torch.zeros(1, 21, 2), torch.zeros(1, 21, 2), K1, None)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_targets_2d({"mano.j2d.norm.r": torch.zeros(1, 21, 2), "mano.j2d.norm.l": torch.zeros(1, 21, 2)}, None,
                                 {"intrinsics": K1})
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.refine_predictions({"mano.pose.r": torch.zeros(1, 16, 3, 3)}, torch.zeros(1, 21, 2), torch.zeros(1, 21, 2), None,
                                     {"intrinsics": K1})


def test_the_wrapper_refuses_both_fits():
    from hands_amd.wrapper import HandsWrapper
    w = HandsWrapper.__new__(HandsWrapper)
    torch.nn.Module.__init__(w)
    w.fit_gt, w.fit_gt_2d = hands_amd.FitConfig(), Fit2DConfig()
    with pytest.raises(ValueError, match="fit_gt and fit_gt_2d"):
        w.process_data({}, {"intrinsics": torch.eye(3)[None]})
    w.fit_gt = None
    with pytest.raises(RuntimeError, match="HIP device only"):
        w.process_data({}, {"intrinsics": torch.eye(3)[None]})
