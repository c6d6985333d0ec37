"""Temporal metrics without a GPU: the fp64 restatement (tests/accel_ref.py) against the reference's fixture and closed forms
with dyadic coordinates, the streaming bookkeeping of AccelMetrics on the restatement, the host side of the two C-ABI entries
and the three Python names, and a compile-only resource guard of csrc/accel.hip."""
import ctypes
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import accel_ref as AR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
KEYS9 = tuple(f"{k}/{s}" for k in AR.ACCEL_KEYS for s in "rlh")
BATCHES = (1, 4, 2, 3, 1)
# a change of sequence inside the second batch (frame 3) and one exactly at the border in front of the fourth (frame 7)
STREAM_IDS = ["a"] * 3 + ["b"] * 4 + ["c"] * 4


def load_fixture():
    z = np.load(os.path.join(ROOT, "tests", "golden", "eval_acc_pose.npz"))
    pred = {k[len("in/pred."):]: z[k] for k in z.files if k.startswith("in/pred.")}
    targets = {k[len("in/targets."):]: z[k] for k in z.files if k.startswith("in/targets.")}
    return z, pred, targets, json.loads(str(z["meta"]))


def dyadic_sequence(T, V, seed=0):
    """Inputs whose coordinates are multiples of 2^-10 in [0.5, 1.5): every difference of them is exact."""
    rng = np.random.RandomState(seed)
    pred, targets = AR.sequence(T, V, seed)
    for h in "rl":
        for k, n in ((f"mano.v3d.cam.{h}", V), (f"mano.j3d.cam.{h}", 21)):
            targets[k] = (0.5 + rng.randint(0, 1024, (T, n, 3)) / 1024.0).astype(np.float32)
            pred[k] = targets[k].copy()
    return pred, targets


def drifted(pred, T):
    """``pred`` moved by a drift linear in t, dyadic: its second difference is exactly zero."""
    t = np.arange(T, dtype=np.float32)[:, None, None]
    a, b = np.float32([2.0 ** -6, -2.0 ** -5, 2.0 ** -4]), np.float32([2.0 ** -8, 2.0 ** -7, -2.0 ** -9])
    return {k: v + a + b * t for k, v in pred.items()}


def quadratic(pred, T, c=2.0 ** -10):
    """``pred`` of a static scene moved by x = c t^2 along the first axis."""
    t = np.arange(T, dtype=np.float32)[:, None, None]
    return {k: v[:1] + np.float32([c, 0, 0]) * t * t for k, v in pred.items()}


def stream_case(T=sum(BATCHES), V=5, seed=3):
    pred, targets = AR.sequence(T, V, seed)
    targets["left_valid"][8] = 0
    targets["is_valid"][5] = 0
    return pred, targets


def run_stream(metric, pred, targets, ids, dev="cpu"):
    """Feed the stream in BATCHES as tensors on ``dev`` -> the nine keys over the whole stream, as numpy."""
    conv = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    rows, at = [], 0
    for p, t in zip(AR.split(pred, BATCHES), AR.split(targets, BATCHES)):
        B = len(t["is_valid"])
        sid = None if ids is None else ids[at:at + B]
        out = metric.update(conv(p), conv(t), seq_id=sid)
        assert set(out) == set(KEYS9) and all(len(v) == B for v in out.values())
        rows.append({k: v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for k, v in out.items()})
        at += B
    return {k: np.concatenate([r[k] for r in rows]) for k in KEYS9}


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_fixture():
    z, pred, targets, meta = load_fixture()
    tol = meta["ref_vs_f64_max_rel"]
    assert 0 < tol < 1e-6
    out = AR.evaluate_accel(pred, targets)
    full = AR.evaluate_accel(pred, AR.all_valid(targets))             # acc_r, acc_l of the fixture: before the masking
    pairs = [("acc/h", z["out/acc/h"], out["acc/h"]),
             ("acc_r", z["out/acc_r"], full["acc/r"][1:-1]),
             ("acc_l", z["out/acc_l"], full["acc/l"][1:-1]),
             ("d1", z["d1/out"], AR.accel_error(z["d1/gt"], z["d1/pred"])[1:-1])]
    for name, ref, mine in pairs:
        assert np.array_equal(np.isnan(ref), np.isnan(mine)), name
        m = ~np.isnan(mine)
        assert m.any() and (np.abs(ref[m].astype(np.float64) - mine[m]) / np.abs(mine[m])).max() <= tol, name   # as the fixture's script
    # the flags of the fixture: what is NaN in acc/r and acc/l is what the validity window says
    for h, bad in (("r", {3, 9, 12}), ("l", {6, 7, 9, 12})):
        want = np.array([t in (0, 15) or any(t + k in bad for k in (-1, 0, 1)) for t in range(16)])
        assert np.array_equal(np.isnan(out[f"acc/{h}"]), want), h
    assert np.isnan(z["out/acc/h"][[0, -1]]).all()


def test_equal_prediction_and_linear_drift_give_exact_zero():
    T = 7
    pred, targets = dyadic_sequence(T, 9)
    for p in (pred, drifted(pred, T)):
        out = AR.evaluate_accel(p, targets)
        for k in KEYS9:
            assert np.isnan(out[k][[0, -1]]).all() and (out[k][1:-1] == 0.0).all(), k
    x = targets["mano.v3d.cam.r"]
    assert (AR.accel_error(x, x)[1:-1] == 0.0).all() and (AR.accel_error(x[..., :1], x[..., :1] + np.float32(0.25))[1:-1] == 0.0).all()


def test_quadratic_motion_is_twice_c_fps_squared():
    T, c = 6, 2.0 ** -10
    _, targets = dyadic_sequence(T, 4)
    static = {k: np.repeat(v[:1], T, 0) for k, v in targets.items() if k.startswith("mano.")}
    targets.update(static)
    for fps in (30.0, 60.0):
        out = AR.evaluate_accel(quadratic(static, T, c), targets, fps=fps)
        for s in "rlh":
            assert (out[f"acc/abs/{s}"][1:-1] == 2 * c * fps * fps).all()
            assert (out[f"acc/{s}"][1:-1] == 0.0).all() and (out[f"acc/j/{s}"][1:-1] == 0.0).all()
        x = static["mano.v3d.cam.r"]
        moved = quadratic({"x": x}, T, c)["x"]
        assert (AR.accel_error(x, moved, fps=fps)[1:-1] == 2 * c * fps * fps).all()
        assert (AR.accel_error(x[..., :1], moved[..., :1], fps=fps)[1:-1] == 2 * c * fps * fps).all()


def test_window_and_sequence_rules():
    x = np.zeros((6, 2, 3), np.float32)
    nan = lambda **kw: np.isnan(AR.accel_error(x, x, **kw)).tolist()
    assert nan() == [True, False, False, False, False, True]
    assert nan(valid=[1, 1, 0, 1, 1, 1]) == [True, True, True, True, False, True]
    assert nan(seq_id=[0, 0, 0, 1, 1, 1]) == [True, False, True, True, False, True]
    assert nan(valid=[1, 1, 1, 1, 1, 0], seq_id=[5, 5, 5, 5, 5, 5]) == [True, False, False, False, True, True]
    for T in (1, 2):
        assert np.isnan(AR.accel_error(x[:T], x[:T])).all()
    poisoned = x.copy()
    poisoned[2] = np.nan                                      # an invalid frame is not looked at
    assert (AR.accel_error(poisoned, poisoned, valid=[1, 1, 0, 1, 1, 1])[4] == 0.0)


# ---- the streaming bookkeeping, on the restatement --------------------------------------------------------------------------
def test_stream_in_batches_is_the_one_shot_call_moved_by_a_row():
    from hands_amd import AccelMetrics
    pred, targets = stream_case()
    T = sum(BATCHES)
    ints = np.array([{"a": 7, "b": 3, "c": 11}[s] for s in STREAM_IDS])
    one = AR.evaluate_accel(pred, targets, seq_id=ints)
    assert sum(~np.isnan(one["acc/h"])) >= 3 and np.isnan(one["acc/h"][[3, 6, 7]]).all()
    metric = AccelMetrics(evaluate=AR.evaluate_accel)
    by_name = run_stream(metric, pred, targets, STREAM_IDS)
    for k in KEYS9:
        assert np.isnan(by_name[k][:2]).all(), k
        assert np.array_equal(by_name[k][2:], one[k][1:T - 1], equal_nan=True), k       # rows 2..T-1 against rows 1..T-2
        assert np.array_equal(by_name[k], AR.stream([(pred, targets, ints)])[k], equal_nan=True), k
    # without reset() the stream goes on: the first two rows now see the kept frames, which are of sequence "c"
    again = run_stream(metric, pred, targets, ["c"] * T)
    assert not np.isnan(again["acc/r"][:2]).any()
    metric.reset()
    fresh = run_stream(metric, pred, targets, STREAM_IDS)
    metric.reset()
    by_int = run_stream(metric, pred, targets, torch.from_numpy(ints))
    for k in KEYS9:
        assert np.array_equal(fresh[k], by_name[k], equal_nan=True), k
        assert np.array_equal(by_int[k], by_name[k], equal_nan=True), k
    # no ids: one sequence
    metric.reset()
    plain = run_stream(metric, pred, targets, None)
    assert np.array_equal(plain["acc/h"][2:], AR.evaluate_accel(pred, targets)["acc/h"][1:T - 1], equal_nan=True)
    # the ids may come through meta_info
    metric.reset()
    conv = lambda d: {k: torch.from_numpy(v) for k, v in d.items()}
    out = metric.update(conv(pred), conv(targets), {"seq_id": STREAM_IDS})
    assert np.array_equal(np.asarray(out["acc/h"]), by_name["acc/h"], equal_nan=True)


# ---- the API surface --------------------------------------------------------------------------------------------------------
def test_names_are_exported():
    import hands_amd
    for n in ("accel_error", "evaluate_accel_metrics", "AccelMetrics"):
        assert n in hands_amd.__all__ and callable(getattr(hands_amd, n)), n
    assert "dist.rl" in hands_amd.accel_error.__doc__                # the distance-field example
    from hands_amd.temporal import ACCEL_KEYS
    assert ACCEL_KEYS == AR.ACCEL_KEYS


def test_accel_functions_refuse_cpu_tensors():
    import hands_amd
    pred, targets = (({k: torch.from_numpy(v) for k, v in d.items()}) for d in AR.sequence(4, 3))
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.evaluate_accel_metrics(pred, targets)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.accel_error(targets["mano.v3d.cam.r"], pred["mano.v3d.cam.r"])
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.AccelMetrics().update(pred, targets)


def test_header_and_binding_hold_the_entries():
    from hands_amd import _lib
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    for name in ("hands_accel_error_f32", "hands_eval_accel_metrics_f32"):
        assert re.search(rf"^int\s+{name}\s*\(", header, flags=re.M) and name in _lib.SIGNATURES, name
    assert f"#define HANDS_ACCEL_NQ {_lib.ACCEL_NQ}" in header and _lib.ACCEL_NQ == 3
    assert "#define HANDS_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5
    assert ctypes.sizeof(_lib.AccelEvalOut) == 3 * _lib.ACCEL_NQ * ctypes.sizeof(ctypes.c_void_p)
    members = re.search(r"typedef struct hands_accel_eval_out \{[^\n]*\n\s*float ([^;]*);", header).group(1)
    assert [m.strip(" *") for m in members.split(",")] == [n for n, _ in _lib.AccelEvalOut._fields_]
    assert "accel.hip" in open(os.path.join(ROOT, "hands_amd", "csrc", "Makefile")).read()


def test_entries_reject_bad_arguments_without_a_gpu():
    from hands_amd import _lib
    L = _lib.lib()
    p, E = 16, 10001                                     # never dereferenced: every call below is refused
    call = lambda gt, pred, valid, seq, out, T, N, D, fps: L.hands_accel_error_f32(gt, pred, valid, seq, out, T, N, D, fps, None)
    assert call(None, p, p, p, p, 3, 1, 3, 30.0) == E and call(p, None, p, p, p, 3, 1, 3, 30.0) == E
    assert call(p, p, p, p, None, 3, 1, 3, 30.0) == E
    for T, N, D, fps in ((0, 1, 3, 30.0), (-1, 1, 3, 30.0), (3, 0, 3, 30.0), (3, -5, 3, 30.0), (3, 1, 0, 30.0), (3, 1, 4, 30.0),
                         (3, 1, -1, 30.0), (3, 1, 3, 0.0), (3, 1, 3, -30.0), (3, 1, 3, float("inf")), (3, 1, 3, float("nan"))):
        assert call(p, p, p, p, p, T, N, D, fps) == E, (T, N, D, fps)
        assert call(p, p, None, None, p, T, N, D, fps) == E, (T, N, D, fps)
    fin, fout = _lib.MeshEvalIn(*[p] * 11), _lib.AccelEvalOut(*[p] * 9)
    ev = lambda i, s, o, T, V, fps: L.hands_eval_accel_metrics_f32(i, s, o, T, V, fps, None)
    for T, V, fps in ((0, 778, 30.0), (-2, 778, 30.0), (3, 0, 30.0), (3, -1, 30.0), (3, 778, 0.0), (3, 778, -1.0),
                      (3, 778, float("inf")), (3, 778, float("-inf")), (3, 778, float("nan"))):
        assert ev(ctypes.byref(fin), p, ctypes.byref(fout), T, V, fps) == E, (T, V, fps)
        assert ev(ctypes.byref(fin), None, ctypes.byref(fout), T, V, fps) == E, (T, V, fps)
    assert ev(None, p, ctypes.byref(fout), 3, 778, 30.0) == E and ev(ctypes.byref(fin), p, None, 3, 778, 30.0) == E
    for i in range(11):
        a = [p] * 11
        a[i] = None
        assert ev(ctypes.byref(_lib.MeshEvalIn(*a)), p, ctypes.byref(fout), 3, 778, 30.0) == E, i
    for i in range(9):
        a = [p] * 9
        a[i] = None
        assert ev(ctypes.byref(fin), p, ctypes.byref(_lib.AccelEvalOut(*a)), 3, 778, 30.0) == E, i


def test_wrapper_metric_dict_is_still_the_reference_names(recipe_model):
    from hands_amd.wrapper import HandsWrapper
    w = HandsWrapper(model=recipe_model)
    assert w.metric_dict == ["mrrpe.rl", "mpjpe.ra", "mpjpe.pa.ra", "pix_err"] and w.accel_fps == 30.0
    assert '"accel" in self.metric_dict' in inspect.getsource(HandsWrapper.forward)
    w.accel_fps = 60.0
    assert w._accel_metrics().fps == 60.0 and w._accel_metrics() is w._accel_metrics()
    first = w._accel_metrics()
    w.reset_accel()
    assert w._accel_metrics() is not first


# ---- compile-only resource guard ----------------------------------------------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_accel_kernel_resources(tmp_path):
    """csrc/accel.hip as the Makefile builds it: neither kernel spills or uses scratch, static LDS stays under 64 KB."""
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "hands_amd", "csrc", "accel.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)[1:]
    field = lambda b, pat: int(re.search(pat, b).group(1))
    names = [b.split()[0] for b in blocks]
    assert len(blocks) == 2 and any("accel_error_kernel" in n for n in names) and any("accel_metrics_kernel" in n for n in names)
    for b in blocks:
        assert field(b, r"ScratchSize \[bytes/lane\]: (\d+)") == 0 and field(b, r"VGPRs Spill: (\d+)") == 0, b.split()[0]
        assert field(b, r"SGPRs Spill: (\d+)") == 0, b.split()[0]
        assert field(b, r"LDS Size \[bytes/block\]: (\d+)") <= 65536, b.split()[0]
