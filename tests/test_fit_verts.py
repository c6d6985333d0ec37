"""MANO fitting to 778 vertices without a GPU: the fp64 restatement tests/fit_verts_ref.py of DESIGN.md section 7 ("MANO fitting to
778 vertices") against central differences, the oracle's LBS and the joint fit's restatement, the conditions the seed tables of
tests/test_gpu_fit_verts.py rest on, and the host side of hands_amd.fitting (names, ABI, FitConfig, the pack)."""
import os
import re

import numpy as np
import pytest
import torch

import fit_ref as F
import fit_verts_ref as V
import hands_amd
from hands_amd import _lib
from hands_amd.fitting import FitConfig
from hands_amd.mano import synthetic_mano_asset
from oracle.hands_oracle import mano_lbs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ASSETS = {"r": synthetic_mano_asset(True), "l": synthetic_mano_asset(False)}
CONSTS = {h: V.consts_from_asset(a) for h, a in ASSETS.items()}
KEYS = ("pose", "beta", "transl", "rmse", "j3d")


@pytest.mark.parametrize("side", ["r", "l"])
def test_jacobian_matches_central_differences(side):
    """The analytic Jacobian of all 2334 data rows against central differences (h = 1e-6) of the restatement's own vertices:
    1e-9 at entries <= 1 (5.2e-11 and 7.0e-11 measured; the truncation error h^2 / 6 of a unit third derivative is 1.7e-13,
    the rounding error 1e-16 / h = 1e-10)."""
    C = CONSTS[side]
    _, _, (R, beta, _) = V.family_case(C, 3)
    D = V.vertex_jacobian(C, R, V.evaluate(C, R, beta))
    h, num = 1e-6, np.zeros((V.NV, 3, 61))
    for u in range(61):
        def at(sign):
            d = np.zeros(61)
            d[u] = sign * h
            R2 = np.stack([R[j] @ V.exp_so3(d[3 * j:3 * j + 3]) for j in range(16)])
            return V.vertices_of(C, R2, beta + d[48:58]) + d[58:61]
        num[:, :, u] = (at(1.0) - at(-1.0)) / (2 * h)
    err = np.abs(D - num).max()
    print(f"FITV|jacobian|{side}|{err:.3e}|1e-9|largest entry {np.abs(D).max():.3f}")
    assert np.abs(D).max() <= 1.0 + 1e-12 and err <= 1e-9


@pytest.mark.parametrize("side", ["r", "l"])
def test_vertices_match_the_oracle_lbs(side):
    """Within 1e-8 m of oracle.hands_oracle.mano_lbs in fp64, fed Log R_j - pose_mean (its Rodrigues adds 1e-8 inside the norm)."""
    C = V.consts_from_asset(ASSETS[side], rounded=False)
    for seed in range(4):
        _, _, (R, beta, _) = V.family_case(C, seed)
        aa = V.pose_aa(C, R)
        v, j = mano_lbs(torch.tensor(beta)[None], torch.tensor(aa[:3])[None], torch.tensor(aa[3:])[None], ASSETS[side],
                        dtype=torch.float64)
        E = V.evaluate(C, R, beta)
        err = max(np.abs(v[0].numpy() - E["v"]).max(), np.abs(j[0].numpy() - E["joints"]).max())
        print(f"FITV|oracle|{side}{seed}|{err:.3e}|1e-8")
        assert err <= 1e-8


@pytest.mark.parametrize("side", ["r", "l"])
def test_tip_rows_are_those_of_the_joint_fit(side):
    """The rows of vertices 744 / 320 / 443 / 554 / 671 are rows 16..20 of fit_ref.jacobian and fit_ref.evaluate: 1e-14, the
    order of a few fp64 sums."""
    C = CONSTS[side]
    Ct = V.tip_consts(C)
    _, _, (R, beta, _) = V.family_case(C, 6)
    E = V.evaluate(C, R, beta)
    D = V.vertex_jacobian(C, R, E)[list(V.TIP_IDS)].reshape(15, 61)
    Jt = F.jacobian(Ct, R, beta, np.ones(21), F.config())
    Et = F.evaluate(Ct, R, beta)
    assert np.abs(D - Jt[48:63]).max() <= 1e-14 and np.abs(E["joints"] - Et["joints"]).max() <= 1e-14
    assert np.abs(E["x"][list(V.TIP_IDS)] - Et["x"]).max() <= 1e-14 and np.abs(E["A"][list(V.TIP_IDS)] - Et["A"]).max() <= 1e-14


# what the restatement measures on the fully weighted family (8 seeds an asset, default configuration): the largest rmse, rotation,
# beta and translation error; the bars below are 4 x these
MEASURED = {"rmse": 9.5e-7, "rot": 1.8e-5, "beta": 8.6e-5, "t": 4.6e-7}


@pytest.mark.parametrize("side", ["r", "l"])
def test_the_family_converges_and_recovers_pose_and_shape(side):
    C = CONSTS[side]
    worst = {k: 0.0 for k in MEASURED}
    for seed in range(8):
        y, w, (R, beta, t) = V.family_case(C, seed)
        r = V.fit(C, y, w)
        raw = r["raw"]
        rot = max(float(np.linalg.norm(V.log_so3(R[j].T @ raw["pose"][j]))) for j in range(16))
        got = {"rmse": raw["rmse"], "rot": rot, "beta": float(np.abs(beta - raw["beta"]).max()), "t": float(np.abs(t - raw["transl"]).max())}
        worst = {k: max(worst[k], got[k]) for k in worst}
        real = sum(1 for c, c2, ok, acc in r["trace"] if acc and abs(c2 - c) > 1e-9 * c)
        assert 4 <= real <= 7, (seed, real)
        cur = r["trace"][0][0]
        for c, c2, ok, acc in r["trace"]:                               # the cost never rises; steps counts the accepted
            assert c == cur
            if acc:
                assert ok and c2 < c
                cur = c2
        assert r["steps"] == sum(1 for x in r["trace"] if x[3]) and len(r["trace"]) == 30
    print(f"FITV|family|{side}|" + "|".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 4 * MEASURED[k], (k, v)


def test_step_parity_rows_have_margins():
    """(a) Every accept / reject decision of iterations 1..4 on the rows of the GPU step-parity test has a margin above 1e-9 c
    and every factorisation succeeds."""
    for h, with_init in (("r", True), ("l", False)):
        y, w, init = V.step_parity_inputs(CONSTS[h], V.STEP_BASES[h], with_init)
        assert np.isnan(y[w == 0]).all() and [int((x > 0).sum()) for x in w] == [778, 778, 278, 736, 20, 4]
        for r in V.fit_rows(CONSTS[h], y, w, init=init, cfg=V.config(iters=4)):
            assert len(r["trace"]) == 4 and V.clear(r["trace"])


def test_full_run_rows_have_margins_and_a_quiet_twin():
    """(b) Every decision of all 30 iterations on the sparse full-run rows has a margin above 1e-9 c.  (c) For every full-run row,
    16 x the largest difference between the run and its noise = 1e-15 twin is <= 1e-6 on every float output."""
    y, w, ref, twin = V.full_run_reference(CONSTS["r"])
    nd = len(V.FULL_DENSE)
    assert nd == 4 and len(V.FULL_SPARSE) == 2 and [int((x > 0).sum()) for x in w] == [778] * 4 + [20] * 2
    for r in ref[nd:]:
        assert len(r["trace"]) == 30 and V.clear(r["trace"])
    for r in ref[:nd]:
        assert V.clear(r["trace"], 4)
    for k in KEYS:
        d = max(float(np.abs(np.asarray(a["raw"][k]) - np.asarray(b["raw"][k])).max()) for a, b in zip(ref, twin))
        print(f"FITV|twin|{k}|{d:.3e}")
        assert 16 * d <= 1e-6, (k, d)


def test_zero_iterations_return_the_kabsch_state_and_unfitted_rows():
    C = CONSTS["l"]
    y, w, (R, beta, t) = V.family_case(C, 7, keep=200)
    r = V.fit(C, y, w, cfg=V.config(iters=0))
    R0 = r["raw"]["pose"]
    assert r["steps"] == 0 and np.array_equal(R0[1:], C.M[1:]) and not r["raw"]["beta"].any()
    assert abs(np.linalg.det(R0[0]) - 1.0) < 1e-12 and np.abs(R0[0] @ R0[0].T - np.eye(3)).max() < 1e-12
    X = V.vertices_of(C, V.rest_pose(C), np.zeros(10))
    Rk, tk = V.kabsch(X, y.astype(np.float64), w.astype(np.float64))
    posed = V.vertices_of(C, R0, np.zeros(10)) + r["raw"]["transl"]
    assert np.abs(posed - (X @ Rk.T + tk)).max() < 1e-8                # fp32 skinning weights sum to 1 within 2^-23 only
    few = np.zeros(V.NV, np.float32)
    few[:3] = 1.0
    nan_y = y.copy()
    nan_y[np.flatnonzero(w)[0], 1] = np.nan
    bad_init = (R.astype(np.float32), np.full(10, np.inf, np.float32), t.astype(np.float32))
    for u in (V.fit(C, y, w, valid=0.0), V.fit(C, y, few), V.fit(C, nan_y, w), V.fit(C, y, w, init=bad_init)):
        assert u["steps"] == 0 and np.isnan(u["rmse"]) and not u["beta"].any() and not u["transl"].any() and np.isnan(u["j3d"]).all()
        assert np.array_equal(u["pose"], C.M.astype(np.float32))
    hidden = y.copy()
    hidden[w == 0] = np.nan
    a, b = V.fit(C, hidden, w, cfg=V.config(iters=3)), V.fit(C, y, w, cfg=V.config(iters=3))
    assert np.isfinite(a["rmse"]) and all(np.array_equal(a[k], b[k]) for k in KEYS)


def test_names_are_exported_and_the_abi():
    for name in ("fit_mano_verts", "fit_mano_hands_verts", "fit_targets_verts"):
        assert name in hands_amd.__all__ and hasattr(hands_amd, name)
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"\bint hands_mano_fit_verts_f32\(const hands_mano_fit_verts_side\* sides, int n_sides, const hands_fit_cfg\* "
                     r"cfg, int B,\s+hands_stream_t stream\);", header)
    for struct in ("hands_mano_fit_verts_consts", "hands_mano_fit_verts_side"):
        assert f"}} {struct};" in header
    assert len(_lib.SIGNATURES["hands_mano_fit_verts_f32"]) == 5
    assert [n for n, _ in _lib.ManoFitVertsConsts._fields_] == ["pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs",
                                                                "lbs_weights", "posedirs_vm"]
    assert [n for n, _ in _lib.ManoFitVertsSide._fields_] == ["consts", "verts", "weights", "valid", "init_pose", "init_beta",
                                                              "init_transl", "pose", "beta", "transl", "rmse", "steps", "j3d"]
    mk = open(os.path.join(ROOT, "hands_amd", "csrc", "Makefile")).read()
    assert "fit_verts.hip" in mk and "fit_device.h" in mk
    from hands_amd.wrapper import HandsWrapper
    assert HandsWrapper.fit_gt_verts is None


def test_fit_config_validation_through_the_new_entry_points():
    """The same FitConfig, the same validation: a bad configuration is a ValueError before anything else is looked at."""
    y = torch.zeros(1, 778, 3)
    t = {"mano.v3d.full.r": y, "mano.v3d.full.l": y}
    for bad in (dict(iters=-1), dict(iters=2.5), dict(lambda_beta=-1e-9), dict(lambda_pose=float("nan")), dict(mu0=float("inf"))):
        with pytest.raises(ValueError):
            hands_amd.fit_mano_verts(y, None, config=FitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_mano_hands_verts(y, y, None, config=FitConfig(**bad))
        with pytest.raises(ValueError):
            hands_amd.fit_targets_verts(t, None, config=FitConfig(**bad))
    with pytest.raises(RuntimeError, match="HIP device only"):           # a good one gets as far as the device rule
        hands_amd.fit_mano_verts(y, None, config=FitConfig(iters=0, lambda_beta=0.0, lambda_pose=0.0, mu0=0.0))
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_targets_verts(t, None)


@pytest.mark.parametrize("side", ["r", "l"])
def test_pack_layout(side):
    """The new keys of pack_mano against the asset: v_template (778,3), shapedirs (778,3,10) and posedirs with the vertex first,
    posedirs_vm[n, f, c] = posedirs[f, 3 n + c]; the existing keys keep their values."""
    from hands_amd.packing import pack_mano
    asset = ASSETS[side]
    p = pack_mano(asset, "cpu")
    pd = np.asarray(asset.posedirs, np.float32).reshape(135, 778 * 3)
    vm = p["posedirs_vm"]
    assert vm.dtype == torch.float32 and tuple(vm.shape) == (778, 135, 3) and vm.is_contiguous()
    flat = vm.numpy().reshape(-1)
    for n, f, c in ((0, 0, 0), (777, 134, 2), (320, 17, 1), (15, 133, 0)):
        assert flat[(n * 135 + f) * 3 + c] == pd[f, 3 * n + c]
    assert np.array_equal(vm.numpy(), pd.reshape(135, 778, 3).transpose(1, 0, 2))
    assert np.array_equal(p["v_template"].numpy(), np.asarray(asset.v_template, np.float32).reshape(778, 3))
    assert np.array_equal(p["shapedirs"].numpy(), np.asarray(asset.shapedirs, np.float32).reshape(778, 3, 10))
    assert p["shapedirs"].is_contiguous() and p["v_template"].is_contiguous()
    tips = list(V.TIP_IDS)
    assert np.array_equal(p["tip_v_template"].numpy(), p["v_template"].numpy()[tips])
    assert np.array_equal(p["tip_posedirs"].numpy(), vm.numpy()[tips].transpose(1, 0, 2).reshape(135, 15))
    C, Cp = CONSTS[side], V.consts_from_pack(p)
    for k in ("pose_mean", "v_template", "shapedirs", "lbs_weights", "posedirs"):
        assert np.array_equal(getattr(C, k), getattr(Cp, k)), k
    for k in ("J_template", "J_shapedirs"):                             # the pack regresses them in its own order of sums
        assert np.abs(getattr(C, k) - getattr(Cp, k)).max() <= 1e-6, k
