"""hands_eval_mesh_metrics_f32 and hands_eval_metrics_masked_f32 on the device against the fp64 restatement
(tests/mesh_metrics_ref.py) and the reference fixture (tests/golden/eval_metrics_egoexo.npz).

Bars.  Continuous keys (mpvpe, the masked mpjpe): rtol 2e-5 / atol 5e-4 mm, the bar of tests/test_metrics.py against the
reference.  F-score and AUC are counts of points under a threshold: a point is *unsure* when its fp64 distance lies within
1e-6 m of a threshold -- about 5 x the fp32 rounding of coordinates <= 0.6 m through one subtraction and one norm -- and only
unsure points may fall on the other side on the device.  So precision P and recall R may each move by (unsure points of that
direction) / V, and F, which grows with both, must lie between F(P - dP, R - dR) and F(P + dP, R + dR); the AUC may move by
(unsure points) / (99 V), a point changing bin being worth 1 / 99 at most.  FP32_SLACK covers the fp32 rounding of the stored
value itself.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_metrics_ref as MR

pytestmark = pytest.mark.gpu

MARGIN = 1e-6            # metres
FP32_SLACK = 2e-7
ALIGN = ("ra", "pa")
MASKED_KEYS = tuple(f"mpjpe/pa/{k}/{s}" for k in ("rao", "abs", "ra") for s in "rlh")


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _rot(ax, ang):
    ax = np.asarray(ax, np.float64) / np.linalg.norm(ax)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def _cloud(V, seed):
    """V vertices and 21 joints of a hand-sized cloud: the synthetic asset's template (cut or tiled to V) plus an offset."""
    from hands_amd.mano import synthetic_mano_asset
    tpl = synthetic_mano_asset(True).v_template.astype(np.float64)
    rng = np.random.RandomState(seed)
    v = np.concatenate([tpl, tpl[::-1] * 0.9 + 0.003])[:V] if V > len(tpl) else tpl[:V]
    j = np.concatenate([tpl[rng.choice(len(tpl), 16, replace=False)], 0.5 * tpl[rng.choice(len(tpl), 5, replace=False)]])
    off = np.array([0.05, -0.03, 0.5]) + 0.02 * rng.randn(3)
    return v + off, j + off


def make_batch(B, V, seed=0, noise_mm=(2.0, 4.0, 8.0)):
    """Ground truth = template + offset; prediction = rotated copy scaled x 1.1 plus Gaussian noise of 2, 4, 8 mm (by sample)."""
    rng = np.random.RandomState(seed)
    pred, targets = {}, {}
    for s in "rl":
        gv, gj, pv, pj = [], [], [], []
        for b in range(B):
            v, j = _cloud(V, seed * 100 + b * 2 + (s == "l"))
            R, c, sig = _rot(rng.randn(3), 0.15 + 0.05 * b), v.mean(0), noise_mm[b % len(noise_mm)] * 1e-3
            f = lambda x: 1.1 * (x - c) @ R.T + c + sig * rng.randn(*x.shape)
            gv.append(v), gj.append(j), pv.append(f(v)), pj.append(f(j))
        targets[f"mano.v3d.cam.{s}"], targets[f"mano.j3d.cam.{s}"] = np.float32(gv), np.float32(gj)
        pred[f"mano.v3d.cam.{s}"], pred[f"mano.j3d.cam.{s}"] = np.float32(pv), np.float32(pj)
    targets.update(is_valid=np.ones(B, np.float32), right_valid=np.ones(B, np.float32), left_valid=np.ones(B, np.float32))
    return pred, targets


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _run(pred, targets):
    from hands_amd.metrics import evaluate_mesh_metrics
    out = evaluate_mesh_metrics(_dev(pred), _dev(targets))
    torch.cuda.synchronize()
    assert len(out) == 30 and all(v.is_cuda and v.dtype == torch.float32 and v.shape == (len(targets["is_valid"]),) for v in out.values())
    return {k: v.cpu().numpy() for k, v in out.items()}


def _bits(out):
    return {k: np.asarray(v).view(np.int32).copy() for k, v in out.items()}


# ---- the comparison ------------------------------------------------------------------------------------------------------
def _f(P, R):
    return 2.0 * P * R / (P + R) if P + R > 0 else 0.0


def _near(x, th):
    return int((np.abs(np.asarray(x)[..., None] - np.atleast_1d(th)) < MARGIN).any(-1).sum())


def check_against_restatement(got, pred, targets, caps=False):
    """Every key of every sample against the restatement, with the bars of the module docstring; returns the largest counts of
    unsure points met (F direction, AUC) for the caller's caps."""
    ref, dists = MR.evaluate_mesh(pred, targets, return_dist=True)
    B, V = pred["mano.v3d.cam.r"].shape[:2]
    assert set(got) == set(ref)
    worst_f = worst_auc = 0
    for k in ref:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(ref[k]), err_msg=k)
    for a in ALIGN:
        for s in "rl":
            k = f"mpvpe/{a}/{s}"
            np.testing.assert_allclose(got[k], ref[k], rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=k)
            for b in range(B):
                if not dists[s][b]:                       # an invalid or non-finite hand: NaN everywhere, checked above
                    continue
                ev, d1, d2, ej = dists[s][b][a]
                for th, name in zip(MR.F_THRESHOLDS, ("5", "15")):
                    kk = f"fscore/{a}/{name}/{s}"
                    if np.isnan(ref[kk][b]):
                        continue
                    u1, u2 = _near(d1, th), _near(d2, th)
                    worst_f = max(worst_f, u1, u2)
                    P, R = float((d1 < th).mean()), float((d2 < th).mean())
                    lo = _f(max(P - u1 / V, 0.0), max(R - u2 / V, 0.0)) - FP32_SLACK
                    hi = _f(min(P + u1 / V, 1.0), min(R + u2 / V, 1.0)) + FP32_SLACK
                    assert lo <= got[kk][b] <= hi, (kk, b, got[kk][b], ref[kk][b], u1, u2)
                for kind, e, n in (("v", ev, V), ("j", ej, 21)):
                    kk = f"auc/{a}/{kind}/{s}"
                    if np.isnan(ref[kk][b]):
                        continue
                    u = _near(e, MR.PCK_THRESHOLDS)
                    if kind == "v":
                        worst_auc = max(worst_auc, u)
                    assert abs(got[kk][b] - ref[kk][b]) <= u / (99.0 * n) + FP32_SLACK, (kk, b, got[kk][b], ref[kk][b], u)
    for k in ref:                                         # h is the nanmean of the r and l the device itself gave
        if k.endswith("/h"):
            r, l = got[k[:-1] + "r"], got[k[:-1] + "l"]
            np.testing.assert_allclose(got[k], MR.nanmean2(r, l), rtol=3e-7, atol=1e-30, equal_nan=True, err_msg=k)
    if caps:
        print(f"unsure points: {worst_f} of {V} per F direction, {worst_auc} of {V} for the vertex AUC")
        assert worst_f <= 0.01 * V and worst_auc <= 0.02 * V
    return worst_f, worst_auc


# ---- parity --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity_batch():
    pred, targets = make_batch(8, 778)
    return pred, targets, _run(pred, targets)


def test_parity_b8_v778(parity_batch):
    pred, targets, got = parity_batch
    check_against_restatement(got, pred, targets, caps=True)
    f5 = np.concatenate([got["fscore/pa/5/r"], got["fscore/pa/5/l"], got["fscore/ra/5/r"], got["fscore/ra/5/l"]])
    print("F@5 range", f5.min(), f5.max(), "mpvpe/pa", got["mpvpe/pa/h"])
    assert f5.min() < 0.5 < f5.max()                      # the thresholds bite: neither all under nor all over
    assert 1.5 < got["mpvpe/pa/r"].min() and got["mpvpe/pa/r"].max() < 16.0 and (got["mpvpe/ra/r"] > got["mpvpe/pa/r"]).all()


@pytest.mark.parametrize("V", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 778, 1024])
def test_edge_vertex_counts(V):
    pred, targets = make_batch(2, V, seed=V)
    check_against_restatement(_run(pred, targets), pred, targets)


def test_single_sample_batch():
    pred, targets = make_batch(1, 778, seed=3)
    check_against_restatement(_run(pred, targets), pred, targets)


def test_bad_arguments_leave_the_outputs_untouched():
    from hands_amd import _lib
    L = _lib.lib()
    pred, targets = make_batch(2, 8)
    p, t = _dev(pred), _dev(targets)
    keep = [p["mano.v3d.cam.r"], p["mano.v3d.cam.l"], t["mano.v3d.cam.r"], t["mano.v3d.cam.l"], p["mano.j3d.cam.r"],
            p["mano.j3d.cam.l"], t["mano.j3d.cam.r"], t["mano.j3d.cam.l"], t["is_valid"], t["right_valid"], t["left_valid"]]
    buf = torch.full((30, 2), -7.5, device="cuda")
    mout = _lib.MeshEvalOut(*[_lib.ptr(buf[i]) for i in range(30)])
    fin = _lib.MeshEvalIn(*[_lib.ptr(x) for x in keep])
    stream = torch.cuda.current_stream().cuda_stream
    for B, V in ((2, 1025), (2, 0), (0, 8)):
        assert L.hands_eval_mesh_metrics_f32(ctypes.byref(fin), ctypes.byref(mout), B, V, stream) == 10001
    args = [_lib.ptr(x) for x in keep]
    args[2] = None
    assert L.hands_eval_mesh_metrics_f32(ctypes.byref(_lib.MeshEvalIn(*args)), ctypes.byref(mout), 2, 8, stream) == 10001
    torch.cuda.synchronize()
    assert bool((buf == -7.5).all())
    assert L.hands_eval_mesh_metrics_f32(ctypes.byref(fin), ctypes.byref(mout), 2, 8, stream) == 0
    torch.cuda.synchronize()
    assert bool((buf != -7.5).all())


# ---- degenerate clouds ---------------------------------------------------------------------------------------------------
def test_degenerate_clouds():
    pred, targets = make_batch(6, 200, seed=5)
    gv, pv = targets["mano.v3d.cam.r"], pred["mano.v3d.cam.r"]
    t = np.linspace(-1, 1, 200, dtype=np.float32)[:, None]
    root = targets["mano.j3d.cam.r"][:, 0]
    gv[0] = root[0] + t * np.float32([0.05, 0.02, -0.03])                               # collinear ground truth and prediction
    pv[0] = pred["mano.j3d.cam.r"][0, 0] + t * np.float32([0.01, 0.06, 0.02]) * (1 + 0.1 * t)
    gv[1, :, 2] = root[1, 2]                                                            # planar, both
    pv[1, :, 2] = pred["mano.j3d.cam.r"][1, 0, 2] + 0.01
    pv[2] = pv[2, :1]                                                                   # constant prediction: pa is NaN
    gv[3] = gv[3, :1]                                                                   # constant ground truth: pa error 0
    for k in ("mano.v3d.cam.r", "mano.j3d.cam.r"):                                      # an exact copy
        pred[k][4] = targets[k][4]
    pv[5] = root[5] + t * np.float32([0.03, 0.0, 0.0])                                  # a line against a full cloud (rank 1)
    got = _run(pred, targets)
    check_against_restatement(got, pred, targets)
    assert all(np.isnan(got[k][2]) for k in ("mpvpe/pa/r", "fscore/pa/5/r", "fscore/pa/15/r", "auc/pa/v/r"))
    assert np.isfinite(got["mpvpe/ra/r"][2]) and np.isfinite(got["auc/pa/j/r"][2])
    assert got["mpvpe/pa/r"][3] < 5e-4 and got["fscore/pa/5/r"][3] == 1.0
    for k in ("mpvpe/ra/r", "fscore/ra/5/r", "fscore/ra/15/r", "auc/ra/v/r", "auc/ra/j/r"):
        assert got[k][4] == (0.0 if k.startswith("mpvpe") else 1.0), k                  # exactly
    assert got["mpvpe/pa/r"][4] < 5e-4 and got["fscore/pa/5/r"][4] == 1.0


# ---- validity ------------------------------------------------------------------------------------------------------------
def test_validity_and_non_finite_coordinates(parity_batch):
    pred, targets, base = parity_batch
    pred, targets = copy.deepcopy(pred), copy.deepcopy(targets)
    targets["left_valid"][1] = 0
    targets["is_valid"][2] = 0
    targets["right_valid"][3] = 0
    pred["mano.v3d.cam.l"][1, 17, 2] = np.nan             # in an invalid hand: changes nothing
    targets["mano.v3d.cam.r"][3, 700, 0] = np.inf
    got = _run(pred, targets)
    gb, bb = _bits(got), _bits(base)
    for k in got:
        s = k[-1]
        if s == "l":
            assert np.isnan(got[k][[1, 2]]).all() and (np.delete(gb[k], [1, 2]) == np.delete(bb[k], [1, 2])).all(), k
        elif s == "r":
            assert np.isnan(got[k][[2, 3]]).all() and (np.delete(gb[k], [2, 3]) == np.delete(bb[k], [2, 3])).all(), k
        else:
            assert np.isnan(got[k][2]) and gb[k][1] == gb[k[:-1] + "r"][1] and gb[k][3] == gb[k[:-1] + "l"][3], k
            assert (np.delete(gb[k], [1, 2, 3]) == np.delete(bb[k], [1, 2, 3])).all(), k
    # a non-finite coordinate in a VALID hand: that hand is NaN in every output, nothing else moves
    for key, idx in (("mano.v3d.cam.r", (5, 777, 1)), ("mano.j3d.cam.r", (5, 20, 0))):
        for where, val in ((pred, np.nan), (targets, -np.inf)):
            p2, t2 = copy.deepcopy(pred), copy.deepcopy(targets)
            (p2 if where is pred else t2)[key][idx] = val
            g2 = _bits(_run(p2, t2))
            for k in got:
                if k[-1] == "r":
                    assert np.isnan(g2[k].view(np.float32)[5]), k
                elif k[-1] == "h":
                    assert g2[k][5] == g2[k[:-1] + "l"][5], k
                assert (np.delete(g2[k], 5) == np.delete(gb[k], 5)).all(), k


# ---- reproducibility -----------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_batch_independent(parity_batch):
    pred, targets, base = parity_batch
    bb = _bits(base)
    again = _bits(_run(pred, targets))
    assert all((again[k] == bb[k]).all() for k in bb)
    for i in (0, 5, 7):
        one = _bits(_run({k: v[i:i + 1] for k, v in pred.items()}, {k: v[i:i + 1] for k, v in targets.items()}))
        assert all(one[k][0] == bb[k][i] for k in bb), i


def test_graph_replay_has_the_eager_bits(parity_batch):
    from hands_amd.metrics import evaluate_mesh_metrics
    pred, targets, base = parity_batch
    p, t = _dev({k: v[:2] for k, v in pred.items()}), _dev({k: v[:2] for k, v in targets.items()})
    eager = {k: v.clone() for k, v in evaluate_mesh_metrics(p, t).items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                             # one stream, one kernel node
        out = evaluate_mesh_metrics(p, t)
    for v in out.values():
        v.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert (out[k].cpu().numpy().view(np.int32) == eager[k].cpu().numpy().view(np.int32)).all(), k
        assert (out[k].cpu().numpy().view(np.int32) == _bits(base)[k][:2]).all(), k


# ---- the masked (egoexo) branch ------------------------------------------------------------------------------------------
def _masked_fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, "eval_metrics_egoexo.npz"))
    pred = {k[len("in/pred."):]: d[k] for k in d.files if k.startswith("in/pred.")}
    targets = {k[len("in/targets."):]: d[k] for k in d.files if k.startswith("in/targets.")}
    B = len(targets["is_valid"])
    rng = np.random.RandomState(0)
    for s in "rl":                                        # the keys the 21-joint entry needs beside
        pred[f"mano.j2d.{s}"] = np.float32(224 * rng.rand(B, 21, 2))
        targets[f"mano.j2d.{s}"] = np.float32(224 * rng.rand(B, 21, 2))
        targets[f"joints_valid_{s}"] = np.float32(rng.rand(B, 21) > 0.2)
    return pred, targets, {k[4:]: d[k] for k in d.files if k.startswith("out/")}


def test_masked_branch_matches_the_reference(golden_dir):
    from hands_amd.metrics import evaluate_metrics
    pred, targets, ref = _masked_fixture(golden_dir)
    B = len(targets["is_valid"])
    p, t = _dev(pred), _dev(targets)
    out = evaluate_metrics(p, t, {"dataset": ["egoexo"] * B})
    plain = evaluate_metrics(p, t, {"dataset": ["arctic"] * B})
    none = evaluate_metrics(p, t)
    torch.cuda.synchronize()
    assert set(out) == set(plain) | set(MASKED_KEYS) and set(ref) == set(MASKED_KEYS)
    for k in MASKED_KEYS:
        got = out[k].cpu().numpy()
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref[k]), err_msg=k)
        np.testing.assert_allclose(got, ref[k], rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=k)        # mm
    # a batch of another dataset: today's keys and values, bit for bit -- and the keys the two branches share do not move
    assert list(plain) == list(none) == ["mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l",
                                         "pix_err/r", "pix_err/l", "pix_err/h"]
    for k in plain:
        a, b = plain[k].cpu().numpy().view(np.int32), none[k].cpu().numpy().view(np.int32)
        assert (a == b).all(), k
        if k not in MASKED_KEYS:
            assert (out[k].cpu().numpy().view(np.int32) == a).all(), k
    # all 21 joints flagged: pa/ra is the 21-joint branch's
    t21 = dict(t, joints3d_valid_r=torch.ones(B, 21).cuda(), joints3d_valid_l=torch.ones(B, 21).cuda())
    full = evaluate_metrics(p, t21, {"dataset": "egoexo_val"})           # a string: 'egoexo' in it, as the reference tests
    for s in "rlh":
        np.testing.assert_allclose(full[f"mpjpe/pa/ra/{s}"].cpu().numpy(), plain[f"mpjpe/pa/ra/{s}"].cpu().numpy(),
                                   rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=s)
    ref21 = MR.evaluate_masked(pred, {k: v.cpu().numpy() for k, v in t21.items()})
    for k in MASKED_KEYS:
        np.testing.assert_allclose(full[k].cpu().numpy(), ref21[k], rtol=2e-5, atol=5e-4, equal_nan=True, err_msg=k)


# ---- the wrapper ---------------------------------------------------------------------------------------------------------
def test_wrapper_mesh_metrics(golden_dir, recipe_model):
    from hands_amd import losses
    from hands_amd.metrics import MESH_KEYS
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
    w.metric_dict = w.metric_dict + ["mesh"]
    out1, _ = w.forward(inputs, dict(targets), meta, "test")
    mesh = ["metric." + k + "/" + s for k in MESH_KEYS for s in "rlh"]
    assert list(out1) == today + mesh
    for k in today[1:]:
        assert torch.equal(out0[k].view(torch.int32), out1[k].view(torch.int32)), k
    for k in mesh:
        assert out1[k].device.type == "cpu" and out1[k].shape == (B,), k
    assert torch.isnan(out1["metric.mpvpe/pa/l"][1]) and torch.equal(out1["metric.mpvpe/pa/h"][1], out1["metric.mpvpe/pa/r"][1])
    assert bool(torch.isfinite(out1["metric.fscore/pa/5/h"]).all())
    ep = losses.epoch_end([{"out_dict": out1, "loss": {}}, {"out_dict": out1, "loss": {}}])
    assert ep["metric.fscore/pa/5/h__val"] == pytest.approx(float(out1["metric.fscore/pa/5/h"].double().mean()), rel=1e-6)
    assert "metric.auc/pa/v/h__val" in ep and "metric.mpvpe/ra/r__val" in ep
