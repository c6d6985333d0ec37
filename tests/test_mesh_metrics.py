"""Mesh metrics and the masked (egoexo) joint metrics without a GPU: closed forms of the fp64 restatement
(tests/mesh_metrics_ref.py), the restatement of the masked branch against the reference's own function, and the host side of
the two new C-ABI entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_metrics_ref as MR

MASKED_KEYS = tuple(f"mpjpe/pa/{k}/{s}" for k in ("rao", "abs", "ra") for s in "rlh")


def _hand(seed=0, V=60):
    rng = np.random.RandomState(seed)
    gv = (0.05 * rng.randn(V, 3) + [0.1, -0.05, 0.6]).astype(np.float32)
    gj = (0.05 * rng.randn(21, 3) + [0.1, -0.05, 0.6]).astype(np.float32)
    return gv, gj


def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def test_identical_clouds_are_perfect():
    gv, gj = _hand()
    vals, _ = MR.hand_mesh_metrics(gv, gv, gj, gj)
    # ra: mpvpe 0, F@5 = F@15 = 1, both AUCs 1 -- exactly
    assert vals[:5] == [0.0, 1.0, 1.0, 1.0, 1.0]
    # pa: the fitted transform is the identity up to rounding; an error of 1e-17 m is past t_0 = 0, which costs half a bin
    assert vals[5] < 1e-9 and vals[6] == 1.0 and vals[7] == 1.0 and vals[8] >= 98.5 / 99 and vals[9] >= 98.5 / 99


def test_similarity_transformed_copy_has_zero_pa_error():
    gv, gj = _hand(1)
    R, s, t = _rot([1, 2, 3], 0.7), 1.3, np.array([0.02, -0.01, 0.03])
    root = gj[0].astype(np.float64)
    f = lambda x: ((s * (x.astype(np.float64) - root) @ R.T) + root + t)
    pv, pj = f(gv), f(gj)
    # in fp64 end to end (the fp32 cast of the inputs would leave 1e-8 m): call the pieces on the root-aligned clouds
    g0, p0 = gv.astype(np.float64) - root, pv - pj[0]
    q = MR.similarity_transform(p0, g0)
    ev = np.sqrt(((g0 - q) ** 2).sum(-1))
    assert ev.max() * 1000.0 < 1e-9
    d1, d2 = MR.nn_distances(g0, q)
    assert MR.fscore(d1, d2, 0.005) == 1.0 and MR.pck_auc(ev) >= 98.5 / 99
    vals, _ = MR.hand_mesh_metrics(pv.astype(np.float32), gv, pj.astype(np.float32), gj)
    assert vals[0] > 1.0 and vals[1] < 1.0 and vals[3] < 1.0 and vals[4] < 1.0          # ra sees the transform ...
    assert vals[5] < 1e-4 and vals[6] == 1.0 and vals[8] >= 98.5 / 99 and vals[9] >= 98.5 / 99   # ... pa undoes it (fp32 inputs)


def test_mirrored_copy_keeps_a_pa_error():
    gv, gj = _hand(2)
    m = np.array([1.0, 1.0, -1.0], np.float32)
    vals, _ = MR.hand_mesh_metrics(gv * m, gv, gj * m, gj)
    assert vals[5] > 1.0 and vals[8] < 1.0 and vals[9] < 1.0          # the best ROTATION, not a reflection


def test_two_point_fscore_by_hand():
    gt = np.array([[0, 0, 0], [0.1, 0, 0]], np.float64)
    pr = np.array([[0.003, 0, 0], [0.004, 0, 0]], np.float64)
    d1, d2 = MR.nn_distances(gt, pr)
    np.testing.assert_allclose(d1, [0.003, 0.096], atol=1e-15)
    np.testing.assert_allclose(d2, [0.003, 0.004], atol=1e-15)
    assert MR.fscore(d1, d2, 0.005) == pytest.approx(2 * 0.5 * 1.0 / 1.5, abs=1e-15)      # P = 1/2, R = 1
    assert MR.fscore(d1, d2, 0.0035) == pytest.approx(0.5, abs=1e-15)                      # P = R = 1/2
    assert MR.fscore(d1, d2, 0.003) == 0.0                                                 # strict <: P + R = 0
    assert MR.fscore(d1, d2, 0.1) == 1.0


def test_auc_closed_form_per_point():
    """A point whose error first passes at threshold k0 adds 1 (k0 = 0), (99.5 - k0) / 99 (1 <= k0 <= 99) or 0."""
    t = MR.PCK_THRESHOLDS
    assert MR.pck_auc([0.0]) == pytest.approx(1.0, abs=1e-12)
    assert MR.pck_auc([1e-12]) == pytest.approx(98.5 / 99, abs=1e-12)
    assert MR.pck_auc([t[37]]) == pytest.approx((99.5 - 37) / 99, abs=1e-12)
    assert MR.pck_auc([np.nextafter(t[37], 1.0)]) == pytest.approx((99.5 - 38) / 99, abs=1e-12)
    assert MR.pck_auc([0.05]) == pytest.approx(0.5 / 99, abs=1e-12) and MR.pck_auc([0.0501]) == 0.0
    e = np.random.RandomState(0).rand(500) * 0.06
    k0 = np.array([np.argmax(x <= t) if (x <= t).any() else 100 for x in e])
    w = np.where(k0 == 0, 1.0, np.where(k0 <= 99, (99.5 - k0) / 99, 0.0))
    assert MR.pck_auc(e) == pytest.approx(w.mean(), abs=1e-12)


def test_degenerate_and_invalid_hands_in_the_restatement():
    gv, gj = _hand(3)
    const = np.tile(gv[:1], (len(gv), 1))
    vals, _ = MR.hand_mesh_metrics(const, gv, gj, gj)           # constant prediction: no similarity transform
    assert np.isfinite(vals[:5]).all() and np.isnan(vals[5:9]).all() and np.isfinite(vals[9])
    vals, _ = MR.hand_mesh_metrics(gv, const, gj, gj)           # constant ground truth: the scale is 0
    assert vals[5] < 1e-9 and vals[6] == 1.0
    bad = gv.copy()
    bad[5, 1] = np.nan
    pred = {"mano.v3d.cam.r": np.stack([gv, bad]), "mano.v3d.cam.l": np.stack([gv, gv]),
            "mano.j3d.cam.r": np.stack([gj, gj]), "mano.j3d.cam.l": np.stack([gj, gj])}
    targets = dict(pred, is_valid=np.ones(2), right_valid=np.ones(2), left_valid=np.array([0.0, 1.0]))
    out = MR.evaluate_mesh(pred, targets)
    assert len(out) == 30 and all(v.shape == (2,) for v in out.values())
    assert np.isnan(out["mpvpe/ra/l"][0]) and out["mpvpe/ra/h"][0] == out["mpvpe/ra/r"][0] == 0.0
    assert np.isnan(out["fscore/pa/5/r"][1]) and out["fscore/pa/5/h"][1] == out["fscore/pa/5/l"][1] == 1.0


def test_masked_restatement_matches_reference(golden_dir):
    d = np.load(os.path.join(golden_dir, "eval_metrics_egoexo.npz"))
    pred = {k[len("in/pred."):]: d[k] for k in d.files if k.startswith("in/pred.")}
    targets = {k[len("in/targets."):]: d[k] for k in d.files if k.startswith("in/targets.")}
    nflag = np.concatenate([targets["joints3d_valid_r"].sum(1), targets["joints3d_valid_l"].sum(1)])
    assert len(pred["mano.j3d.cam.r"]) == 24 and {0, 1, 2, 3, 21} <= set(nflag.astype(int))
    assert (targets["joints3d_valid_r"][:, 0] == 0).any() and (targets["right_valid"] * targets["is_valid"] == 0).any()
    out = MR.evaluate_masked(pred, targets)
    assert set(out) == set(MASKED_KEYS) == {k[4:] for k in d.files if k.startswith("out/")}
    for k in MASKED_KEYS:
        ref = d["out/" + k]
        assert out[k].shape == ref.shape == (24,), k
        np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref), err_msg=k)
        np.testing.assert_allclose(out[k], ref, rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=k)     # mm
    assert np.isnan(d["out/mpjpe/pa/ra/r"]).any() and (d["out/mpjpe/pa/ra/r"] == 0).any()


def test_mesh_metrics_refuse_cpu_tensors():
    import hands_amd
    assert hands_amd.evaluate_mesh_metrics is hands_amd.metrics.evaluate_mesh_metrics and "evaluate_mesh_metrics" in hands_amd.__all__
    gv, gj = _hand()
    pred = {"mano.v3d.cam.r": torch.from_numpy(gv)[None], "mano.v3d.cam.l": torch.from_numpy(gv)[None],
            "mano.j3d.cam.r": torch.from_numpy(gj)[None], "mano.j3d.cam.l": torch.from_numpy(gj)[None]}
    targets = dict(pred, is_valid=torch.ones(1), right_valid=torch.ones(1), left_valid=torch.ones(1))
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.evaluate_mesh_metrics(pred, targets)


def test_wrapper_metric_dict_defaults_to_the_reference_names(recipe_model):
    from hands_amd.wrapper import HandsWrapper
    assert HandsWrapper(model=recipe_model).metric_dict == ["mrrpe.rl", "mpjpe.ra", "mpjpe.pa.ra", "pix_err"]


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from hands_amd import _lib
    from hands_amd.metrics import MESH_KEYS
    L = _lib.lib()
    assert ctypes.sizeof(_lib.MeshEvalOut) == 3 * _lib.MESH_NQ * ctypes.sizeof(ctypes.c_void_p) and len(MESH_KEYS) == _lib.MESH_NQ
    assert ctypes.sizeof(_lib.MeshEvalIn) == 11 * 8 and ctypes.sizeof(_lib.EvalMaskedOut) == 9 * 8
    header = open(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "..", "include", "hands_hip.h")).read()
    assert f"#define HANDS_MESH_MAX_V {_lib.MESH_MAX_V}" in header and f"#define HANDS_MESH_NQ {_lib.MESH_NQ}" in header
    fin, fout = _lib.MeshEvalIn(*[16] * 11), _lib.MeshEvalOut(*[16] * 30)      # never dereferenced: every call below is refused
    for B, V in ((1, 0), (1, 1025), (0, 778), (-1, 778)):
        assert L.hands_eval_mesh_metrics_f32(ctypes.byref(fin), ctypes.byref(fout), B, V, None) == 10001, (B, V)
    assert L.hands_eval_mesh_metrics_f32(None, ctypes.byref(fout), 1, 778, None) == 10001
    assert L.hands_eval_mesh_metrics_f32(ctypes.byref(fin), None, 1, 778, None) == 10001
    for i in (0, 7, 10):
        a = [16] * 11
        a[i] = None
        assert L.hands_eval_mesh_metrics_f32(ctypes.byref(_lib.MeshEvalIn(*a)), ctypes.byref(fout), 1, 778, None) == 10001
    a = [16] * 30
    a[29] = None
    assert L.hands_eval_mesh_metrics_f32(ctypes.byref(fin), ctypes.byref(_lib.MeshEvalOut(*a)), 1, 778, None) == 10001
    ein, mout = _lib.EvalIn(*[16] * 13), _lib.EvalMaskedOut(*[16] * 9)
    assert L.hands_eval_metrics_masked_f32(ctypes.byref(ein), 16, 16, ctypes.byref(mout), 0, None) == 10001
    assert L.hands_eval_metrics_masked_f32(ctypes.byref(ein), None, 16, ctypes.byref(mout), 4, None) == 10001
    assert L.hands_eval_metrics_masked_f32(ctypes.byref(ein), 16, 16, None, 4, None) == 10001
    a = [16] * 9
    a[4] = None
    assert L.hands_eval_metrics_masked_f32(ctypes.byref(ein), 16, 16, ctypes.byref(_lib.EvalMaskedOut(*a)), 4, None) == 10001
