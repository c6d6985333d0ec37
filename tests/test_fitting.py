"""MANO fitting without a GPU: the fp64 restatement tests/fit_ref.py of DESIGN.md section 7 ("MANO fitting") against central
differences, the oracle's LBS and its own rules, and the host side of hands_amd.fitting (names, ABI, FitConfig)."""
import os
import re

import numpy as np
import pytest
import torch

import fit_ref as F
import hands_amd
from hands_amd import _lib
from hands_amd.fitting import FitConfig
from hands_amd.mano import synthetic_mano_asset
from oracle.hands_oracle import batch_rodrigues, mano_lbs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ASSETS = {"r": synthetic_mano_asset(True), "l": synthetic_mano_asset(False)}
CONSTS = {h: F.consts_from_asset(a) for h, a in ASSETS.items()}


@pytest.mark.parametrize("side", ["r", "l"])
def test_analytic_jacobian_matches_central_differences(side):
    """Bar 1e-8 absolute at h = 1e-6 (entries are of size <= 1; 5.8e-11 measured).  The 45 pose-prior rows are left out: they
    use the Gauss-Newton approximation d Log / d delta = I on purpose."""
    C = F.consts_from_asset(ASSETS[side], rounded=False)
    cfg = F.config()
    for seed in (3, 8):                                   # seed 3 has five joints of weight 0
        y, w, (R, beta, t) = F.family_case(C, seed)
        y, w = y.astype(np.float64), w.astype(np.float64)
        R = np.stack([R[j] @ F.exp_so3(0.1 * np.random.RandomState(seed).randn(16, 3)[j]) for j in range(16)])
        Jm = F.jacobian(C, R, beta, w, cfg)

        def res(d):
            R2 = np.stack([R[j] @ F.exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            return F.residual(C, R2, beta + d[48:58], t + d[58:61], y, w, cfg)
        h, num = 1e-6, np.zeros_like(Jm)
        for i in range(F.NU):
            e = np.zeros(F.NU)
            e[i] = h
            num[:, i] = (res(e) - res(-e)) / (2 * h)
        err = np.abs(Jm[:73] - num[:73]).max()
        print(f"FIT|jacobian|{side}{seed}|{err:.3e}|1e-8")
        assert err <= 1e-8
        assert np.abs(Jm[:63]).max() <= 1.0 * np.sqrt(w.max()) + 1e-12
        assert not Jm[:63][np.repeat(w == 0, 3)].any()    # a joint of weight 0 has no rows


@pytest.mark.parametrize("side", ["r", "l"])
def test_joints_match_the_oracle_lbs(side):
    """Within 1e-8 m of oracle.hands_oracle.mano_lbs in fp64, fed Log R_j - pose_mean (its Rodrigues adds 1e-8 inside the norm)."""
    C = F.consts_from_asset(ASSETS[side], rounded=False)
    for seed in range(4):
        _, _, (R, beta, _) = F.family_case(C, seed)
        aa = F.pose_aa(C, R)
        _, j = mano_lbs(torch.tensor(beta)[None], torch.tensor(aa[:3])[None], torch.tensor(aa[3:])[None], ASSETS[side],
                        dtype=torch.float64)
        err = np.abs(j[0].numpy() - F.joints_of(C, R, beta)).max()
        print(f"FIT|oracle|{side}{seed}|{err:.3e}|1e-8")
        assert err <= 1e-8


def test_pose_aa_round_trips_through_the_convention_of_process_data():
    """process_data adds pose_mean to the (B,48) axis-angle target and takes Rodrigues of it: that gives the fitted rotations."""
    C = CONSTS["r"]
    _, _, (R, _, _) = F.family_case(C, 5)
    aa = F.pose_aa(C, R)
    back = batch_rodrigues(torch.tensor(aa + C.pose_mean).reshape(16, 3)).numpy()
    assert np.abs(back - R).max() <= 1e-7
    assert np.abs(F.pose_aa(C, F.rest_pose(C))).max() <= 1e-12          # the mean pose is the zero target


def test_cost_never_rises_and_steps_count_the_accepted():
    C = CONSTS["r"]
    y, w, _ = F.family_case(C, 2)
    r = F.fit(C, y, w)
    cur = r["trace"][0][0]
    for c, c2, ok, acc in r["trace"]:
        assert c == cur
        if acc:
            assert ok and c2 < c
            cur = c2
    assert r["steps"] == sum(1 for t in r["trace"] if t[3]) and len(r["trace"]) == 30


def test_zero_iterations_return_the_kabsch_state():
    C = CONSTS["l"]
    y, w, _ = F.family_case(C, 7)
    r = F.fit(C, y, w, cfg=F.config(iters=0))
    R = r["raw"]["pose"]
    assert r["steps"] == 0 and np.array_equal(R[1:], C.M[1:]) and not r["raw"]["beta"].any()
    assert abs(np.linalg.det(R[0]) - 1.0) < 1e-12 and np.abs(R[0] @ R[0].T - np.eye(3)).max() < 1e-12
    X = F.joints_of(C, F.rest_pose(C), np.zeros(10))
    Rk, tk = F.kabsch(X, y.astype(np.float64), w.astype(np.float64))
    posed = F.joints_of(C, R, np.zeros(10)) + r["raw"]["transl"]
    # the posed rest hand is the aligned one; 1e-8 m because the fp32 skinning weights of a tip sum to 1 within 2^-23 only,
    # so the published LBS is rigid in R_0 to that relative precision of a 0.1 m hand
    assert np.abs(posed[:16] - (X @ Rk.T + tk)[:16]).max() < 1e-12 and np.abs(posed - (X @ Rk.T + tk)).max() < 1e-8
    sel = w > 0
    rms = lambda P: np.sqrt((w[sel, None] * (P[sel] - y[sel]) ** 2).sum() / w[sel].sum())
    best = rms(X @ Rk.T + tk)
    assert abs(best - r["raw"]["rmse"]) < 1e-8
    for seed in range(3):                                              # no rigid motion nearby does better
        rng = np.random.RandomState(seed)
        assert rms(X @ (F.exp_so3(1e-3 * rng.randn(3)) @ Rk).T + tk + 1e-4 * rng.randn(3)) > best


def test_rows_that_are_not_fitted():
    C = CONSTS["r"]
    y, w, (R, beta, t) = F.family_case(C, 1)
    few = np.zeros(21, np.float32)
    few[:3] = 1.0
    nan_y = y.copy()
    nan_y[4, 1] = np.nan
    bad_init = (R.astype(np.float32), np.full(10, np.inf, np.float32), t.astype(np.float32))
    for r in (F.fit(C, y, w, valid=0.0), F.fit(C, y, few), F.fit(C, nan_y, w), F.fit(C, y, w, init=bad_init)):
        assert r["steps"] == 0 and np.isnan(r["rmse"]) and not r["beta"].any() and not r["transl"].any()
        assert np.array_equal(r["pose"], C.M.astype(np.float32)) and np.array_equal(r["pose"][0], np.eye(3, dtype=np.float32))
    w0 = w.copy()
    w0[4] = 0.0
    a, b = F.fit(C, nan_y, w0, cfg=F.config(iters=3)), F.fit(C, y, w0, cfg=F.config(iters=3))
    assert np.isfinite(a["rmse"]) and all(np.array_equal(a[k], b[k]) for k in ("pose", "beta", "transl", "rmse"))


def test_no_tie_decides_a_branch_on_the_parity_inputs():
    """Every accept / reject decision of the restatement on the inputs of the GPU parity tests has a margin |c' - c| > 1e-9 c,
    and every factorisation succeeds: a rounding-level difference cannot change a branch."""
    for C, base, with_init in ((CONSTS["r"], 100, True), (CONSTS["l"], 200, False)):
        y, w, init = F.step_parity_inputs(C, base, with_init)
        for r in F.fit_rows(C, y, w, init=init, cfg=F.config(iters=3)):
            assert all(ok and abs(c2 - c) > 1e-9 * c for c, c2, ok, _ in r["trace"])
    _, _, ref, _ = F.full_run_reference(CONSTS["r"])
    for r in ref:
        assert all(ok and abs(c2 - c) > 1e-9 * c for c, c2, ok, _ in r["trace"])


def test_the_family_converges_and_the_twin_agrees():
    """The 16 cases of DESIGN.md section 7 at the default configuration: rmse <= 2e-3 m in every case (the priors set a floor of
    about 1e-4 m), and the noise = 1e-15 twin takes the same number of steps on at least 14 of them."""
    _, _, ref, twin = F.full_run_reference(CONSTS["r"])
    rm = [float(r["rmse"]) for r in ref]
    print("FIT|family rmse|min %.3e|median %.3e|max %.3e" % (min(rm), float(np.median(rm)), max(rm)))
    assert max(rm) <= 2e-3
    assert sum(a["steps"] == b["steps"] for a, b in zip(ref, twin)) >= 14


def test_names_are_exported_and_the_abi_version_stays():
    for name in ("FitConfig", "fit_mano", "fit_mano_hands", "fit_targets"):
        assert name in hands_amd.__all__ and hasattr(hands_amd, name)
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"\bint hands_mano_fit_f32\(const hands_mano_fit_side\* sides, int n_sides, const hands_fit_cfg\* cfg, int B,"
                     r" hands_stream_t stream\);", header)
    for struct in ("hands_mano_fit_consts", "hands_mano_fit_side", "hands_fit_cfg"):
        assert f"}} {struct};" in header
    assert "hands_mano_fit_f32" in _lib.SIGNATURES and len(_lib.SIGNATURES["hands_mano_fit_f32"]) == 5
    assert re.search(r"#define HANDS_ABI_VERSION 5\b", header) and _lib.ABI_VERSION == 5
    assert [n for n, _ in _lib.ManoFitSide._fields_] == ["consts", "joints", "weights", "valid", "init_pose", "init_beta",
                                                         "init_transl", "pose", "beta", "transl", "rmse", "steps"]
    assert "fit.hip" in open(os.path.join(ROOT, "hands_amd", "csrc", "Makefile")).read()


def test_fit_config_validation():
    c = FitConfig().c_struct()
    assert (c.iters, c.lambda_beta, c.lambda_pose, c.mu0) == (30, 1e-6, 1e-6, 1e-3)
    assert FitConfig(iters=0, lambda_beta=0.0, lambda_pose=0.0, mu0=0.0).c_struct().iters == 0
    for bad in (dict(iters=-1), dict(iters=2.5), dict(lambda_beta=-1e-9), dict(lambda_pose=float("nan")), dict(mu0=float("inf"))):
        with pytest.raises(ValueError):
            FitConfig(**bad).c_struct()


def test_fitting_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano(torch.zeros(1, 21, 3), None)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_targets({"mano.j3d.full.r": torch.zeros(1, 21, 3), "mano.j3d.full.l": torch.zeros(1, 21, 3)}, None)


def test_the_three_fits_share_the_config_and_init_rules(monkeypatch):
    """One launch path: the joint and the 2-D fit refuse a bad configuration before they look at a tensor, as the vertex fit
    does (tests/test_fit_verts.py), and every fit refuses an ``init`` that is not three tensors with the same ValueError."""
    from hands_amd import Fit2DConfig, fitting
    y3, y2, K = torch.zeros(1, 21, 3), torch.zeros(1, 21, 2), torch.eye(3)[None]
    for bad in (dict(iters=-1), dict(lambda_pose=float("nan")), dict(mu0=float("inf"))):
        with pytest.raises(ValueError):
            hands_amd.fit_mano(y3, None, config=FitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_mano_hands(y3, y3, None, config=FitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_targets({"mano.j3d.full.r": y3, "mano.j3d.full.l": y3}, None, config=FitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_mano_2d(y2, K, None, config=Fit2DConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_mano_hands_2d(y2, y2, K, None, config=Fit2DConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_targets_2d({"mano.j2d.norm.r": y2, "mano.j2d.norm.l": y2}, None, {"intrinsics": K}, config=Fit2DConfig(**bad))
    monkeypatch.setattr(fitting, "_opt", lambda v, *a: v)                 # the device rule comes first on this machine
    a = torch.zeros(1)
    for fit, shared in ((fitting._FIT_JOINTS, ()), (fitting._FIT_2D, (K,)), (fitting._FIT_VERTS, ())):
        for init in ((a, a), (a, a, a, a), (a, None, a)):
            with pytest.raises(ValueError, match=r"init is \(pose"):
                fitting._launch(fit, [None], [a], [None], [None], [init], None, "cpu", shared)
