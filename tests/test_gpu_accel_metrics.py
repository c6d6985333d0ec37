"""hands_accel_error_f32, hands_eval_accel_metrics_f32 and what stands on them (hands_amd/temporal.py, "accel" in HandsWrapper)
on the device against the fp64 restatement (tests/accel_ref.py) and the reference's fixture (tests/golden/eval_acc_pose.npz).

Bars.  Against the restatement: 4 * 2^-24 relative plus 1e-10 (fps / 30)^2 absolute.  The kernel computes in fp64 what the
restatement computes, in another summation order (a change below N * 2^-53 relative), and rounds once to fp32: 2^-24 relative, taken
four times.  The absolute term is the fp64 cancellation of coordinates of about 1 m, 2^-53 * fps^2 * a few operations.  Against
the fixture: its own recorded deviation from the restatement, ``ref_vs_f64_max_rel``, plus 4 * 2^-24, by the triangle inequality.
NaN patterns are identical everywhere, exact zeros are exact, equal windows give equal bits wherever they stand.

A non-finite coordinate goes through the arithmetic as IEEE has it, with no special case: a NaN gives NaN in the three rows whose
window holds it; an infinity gives +inf there (inf - 2 x + y is inf, and so are its norm and the mean), and the nanmean of +inf and
the other hand is +inf -- that is what the restatement says and what test_non_finite_coordinates holds the kernel to.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import accel_ref as AR
from edge_util import In, Out
from hands_amd._lib import ptr
from test_accel_metrics import (BATCHES, KEYS9, STREAM_IDS, drifted, dyadic_sequence, load_fixture, quadratic, run_stream,
                                stream_case)

pytestmark = pytest.mark.gpu

UNWRITTEN = 123.0
MESH_IN = ("pred:mano.v3d.cam.r", "pred:mano.v3d.cam.l", "targets:mano.v3d.cam.r", "targets:mano.v3d.cam.l",
           "pred:mano.j3d.cam.r", "pred:mano.j3d.cam.l", "targets:mano.j3d.cam.r", "targets:mano.j3d.cam.l",
           "targets:is_valid", "targets:right_valid", "targets:left_valid")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def bound(ref, fps=30.0):
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return 4 * 2.0 ** -24 * torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0) + 1e-10 * (fps / 30.0) ** 2


def close(what, got, ref, fps=30.0, rel_extra=0.0):
    """NaN exactly where the restatement has it, +-inf equal, the rest inside the bar; prints the narrowest margin."""
    got, ref = torch.as_tensor(got).cpu(), torch.as_tensor(ref, dtype=torch.float64)
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), (what, "NaN positions differ", got, ref)
    inf = torch.isinf(ref)
    assert torch.equal(got[inf].double(), ref[inf]), (what, "infinities differ")
    fin = torch.isfinite(ref)
    err = (got[fin].double() - ref[fin]).abs()
    bnd = bound(ref[fin], fps) + rel_extra * ref[fin].abs()
    if err.numel():
        i = (err / bnd).argmax()
        print(f"ACCEL|{what}|{err[i].item():.3e}|{bnd[i].item():.3e}")
    assert torch.all(err <= bnd), (what, err.max().item())


def c_accel(gt, pred, valid, seq, fps):
    """hands_accel_error_f32 on guarded buffers -> (T) on the CPU."""
    from hands_amd import _lib
    T, N, D = gt.shape
    g, p = In(torch.from_numpy(gt)), In(torch.from_numpy(pred), lead=12)
    v = None if valid is None else In(torch.from_numpy(np.float32(valid)))
    s = None if seq is None else torch.tensor(seq, dtype=torch.int32).cuda()
    o = Out(T, init=torch.full((T,), UNWRITTEN))
    rc = _lib.lib().hands_accel_error_f32(g.ptr(), p.ptr(), None if v is None else v.ptr(), ptr(s), o.ptr(), T, N, D, fps, _stream())
    assert rc == 0, rc
    out = o.get()
    assert not bool((out == UNWRITTEN).any()), "a row was left unwritten"
    return out


def c_eval(pred, targets, seq, fps):
    """hands_eval_accel_metrics_f32 on guarded buffers -> the nine keys on the CPU."""
    from hands_amd import _lib
    src = {"pred": pred, "targets": targets}
    ins = [In(torch.from_numpy(np.float32(src[k.split(":")[0]][k.split(":")[1]]))) for k in MESH_IN]
    T, V = pred["mano.v3d.cam.r"].shape[:2]
    outs = [Out(T, init=torch.full((T,), UNWRITTEN)) for _ in KEYS9]
    s = None if seq is None else torch.tensor(seq, dtype=torch.int32).cuda()
    fin, fout = _lib.MeshEvalIn(*[i.ptr() for i in ins]), _lib.AccelEvalOut(*[o.ptr() for o in outs])
    rc = _lib.lib().hands_eval_accel_metrics_f32(ctypes.byref(fin), ptr(s), ctypes.byref(fout), T, V, fps, _stream())
    assert rc == 0, rc
    res = {k: o.get() for k, o in zip(KEYS9, outs)}
    assert not any(bool((v == UNWRITTEN).any()) for v in res.values()), "a row was left unwritten"
    return res


def flags_for(T, N):
    """valid and seq_id of a primitive case: an invalid frame and a change of sequence that leave a row alive where T allows."""
    valid, seq = np.ones(T, np.float32), np.full(T, 2 ** 31 - 1, np.int64)
    if T >= 4:
        valid[T - 1] = 0
        seq[0] = -2 ** 31 if T == 9 else seq[0]
    if T == 9:
        valid[4] = 0
    if T == 3 and N % 2:
        valid[0] = 0
    if T == 3 and N == 64:
        seq[2] = 7
    return valid, seq


# ---- 1. the primitive through the C ABI --------------------------------------------------------------------------------------
PRIMITIVE = ((1, 1, 3), (2, 65, 3), (3, 1, 1), (3, 63, 2), (3, 64, 3), (3, 257, 3), (3, 1500, 2), (4, 65, 1), (4, 255, 2),
             (4, 778, 3), (9, 256, 3), (9, 257, 1), (9, 1500, 3))


@pytest.mark.parametrize("T,N,D", PRIMITIVE)
def test_primitive_against_the_restatement(T, N, D):
    rng = np.random.RandomState(T * 10000 + N * 10 + D)
    gt = (0.6 + 0.1 * rng.randn(T, N, D)).astype(np.float32)
    pred = (gt + 3e-3 * rng.randn(T, N, D)).astype(np.float32)
    valid, seq = flags_for(T, N)
    alive = 0
    for i, (v, s) in enumerate(((None, None), (valid, None), (None, seq), (valid, seq))):
        fps = (30.0, 60.0)[(i + N) % 2]
        got = c_accel(gt, pred, v, s, fps)
        ref = AR.accel_error(gt, pred, v, s, fps)
        assert bool(torch.isnan(got[0])) and bool(torch.isnan(got[-1]))
        close(f"primitive T{T} N{N} D{D} case{i}", got, ref, fps)
        alive += int((~np.isnan(ref)).sum())
    assert alive >= (4 if T >= 4 else (1 if T == 3 else 0))


# ---- 2. the fused entry ------------------------------------------------------------------------------------------------------
FUSED = ((1, 1), (2, 257), (3, 1), (3, 778), (3, 1500), (7, 257), (7, 1024), (7, 1500))


@pytest.mark.parametrize("T,V", FUSED)
def test_fused_against_the_restatement(T, V):
    pred, targets = AR.sequence(T, V, seed=T * 2000 + V)
    if T == 7:
        targets["right_valid"][1] = 0
        targets["left_valid"][5] = 0
    for fps, seq in ((30.0, None), (60.0, [4] * (T - 1) + [9])):
        got = c_eval(pred, targets, seq, fps)
        ref = AR.evaluate_accel(pred, targets, fps=fps, seq_id=seq)
        for k in KEYS9:
            close(f"fused T{T} V{V} {k}", got[k], ref[k], fps)
    if T >= 3:
        assert np.isfinite(ref["acc/h"]).sum() >= 1 - (T == 3)


def test_every_invalid_hand_in_a_window():
    from hands_amd import evaluate_accel_metrics
    pred, targets = AR.sequence(3, 257, seed=5)
    dp = _cuda(pred)
    combos = [(r, l, None) for r in (None, 0, 1, 2) for l in (None, 0, 1, 2)] + [(None, None, i) for i in range(3)] + [(1, None, 2)]
    for r, l, i in combos:
        t = {k: v.copy() for k, v in targets.items()}
        for key, at in (("right_valid", r), ("left_valid", l), ("is_valid", i)):
            if at is not None:
                t[key][at] = 0
        got = evaluate_accel_metrics(dp, _cuda(t))
        ref = AR.evaluate_accel(pred, t)
        assert list(got) == list(KEYS9)
        for k in KEYS9:
            close(f"invalid r{r} l{l} i{i} {k}", got[k], ref[k])
        assert np.isnan(ref["acc/r"][1]) == (r is not None or i is not None)
        assert np.isnan(ref["acc/h"][1]) == (i is not None or (r is not None and l is not None))


def test_a_sequence_change_at_every_position():
    from hands_amd import evaluate_accel_metrics
    pred, targets = AR.sequence(7, 257, seed=6)
    dp, dt = _cuda(pred), _cuda(targets)
    for c in range(0, 7):
        ids = [3] * c + [-8] * (7 - c)
        ref = AR.evaluate_accel(pred, targets, seq_id=ids)
        for how, got in (("keyword", evaluate_accel_metrics(dp, dt, seq_id=torch.tensor(ids))),
                         ("meta_info", evaluate_accel_metrics(dp, dt, {"seq_id": torch.tensor(ids).cuda()})),
                         ("wide ids", evaluate_accel_metrics(dp, dt, seq_id=[i * 2 ** 40 for i in ids]))):
            for k in KEYS9:
                close(f"change at {c} {how} {k}", got[k], ref[k])
        want = [t in (0, 6) or (c > 0 and t in (c - 1, c)) for t in range(7)]
        assert np.isnan(ref["acc/h"]).tolist() == want, c


# ---- 3. the reference's fixture ------------------------------------------------------------------------------------------------
def test_reference_fixture():
    from hands_amd import accel_error, evaluate_accel_metrics
    z, pred, targets, meta = load_fixture()
    extra = meta["ref_vs_f64_max_rel"]
    T = len(targets["is_valid"])

    def against(what, got, ref):
        got, ref = got.cpu(), torch.from_numpy(np.asarray(ref, np.float64))
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
        m = ~torch.isnan(ref)
        err, bnd = (got[m].double() - ref[m]).abs(), (extra + 4 * 2.0 ** -24) * ref[m].abs()
        print(f"ACCEL|fixture {what}|{(err / bnd).max().item():.3f} of the bar")
        assert bool(m.any()) and torch.all(err <= bnd), (what, (err / bnd).max().item())
    got = evaluate_accel_metrics(_cuda(pred), _cuda(targets))
    against("acc/h", got["acc/h"], z["out/acc/h"])
    pad = lambda x: np.concatenate([[np.nan], x, [np.nan]])
    for h in "rl":                                                   # the fixture holds acc_r, acc_l before the masking
        mask = np.isnan(AR.evaluate_accel(pred, targets)[f"acc/{h}"])
        against(f"acc/{h}", got[f"acc/{h}"], np.where(mask, np.nan, pad(z[f"out/acc_{h}"])))
    ones = dict(targets, **{k: np.ones(T, np.float32) for k in ("is_valid", "right_valid", "left_valid")})
    free = evaluate_accel_metrics(_cuda(pred), _cuda(ones))
    for h in "rl":
        against(f"acc/{h} all valid", free[f"acc/{h}"], pad(z[f"out/acc_{h}"]))
    against("D = 1", accel_error(torch.from_numpy(z["d1/gt"]).cuda(), torch.from_numpy(z["d1/pred"]).cuda()), pad(z["d1/out"]))


# ---- 4. exact zeros ----------------------------------------------------------------------------------------------------------
def test_exact_zeros_and_the_quadratic():
    from hands_amd import accel_error, evaluate_accel_metrics
    T = 7
    pred, targets = dyadic_sequence(T, 300)
    zero = torch.zeros(T - 2)
    for p in (pred, drifted(pred, T)):
        out = evaluate_accel_metrics(_cuda(p), _cuda(targets), fps=60.0)
        for k in KEYS9:
            assert bool(torch.isnan(out[k][[0, -1]]).all()) and torch.equal(out[k][1:-1].cpu(), zero), k
        x, y = torch.from_numpy(targets["mano.v3d.cam.l"]).cuda(), torch.from_numpy(p["mano.v3d.cam.l"]).cuda()
        for D in (1, 2, 3):
            assert torch.equal(accel_error(x[..., :D].contiguous(), y[..., :D].contiguous())[1:-1].cpu(), zero), D
    c = 2.0 ** -10
    static = {k: np.repeat(v[:1], T, 0) for k, v in targets.items() if k.startswith("mano.")}
    for fps in (30.0, 60.0):
        out = evaluate_accel_metrics(_cuda(quadratic(static, T, c)), _cuda(dict(targets, **static)), fps=fps)
        for s in "rlh":
            assert torch.equal(out[f"acc/abs/{s}"][1:-1].cpu(), torch.full((T - 2,), 2 * c * fps * fps)), (fps, s)
            assert torch.equal(out[f"acc/{s}"][1:-1].cpu(), zero) and torch.equal(out[f"acc/j/{s}"][1:-1].cpu(), zero)


# ---- 5. non-finite input -----------------------------------------------------------------------------------------------------
def _bits(d):
    return {k: v.cpu().view(torch.int32) for k, v in d.items()}


@pytest.mark.parametrize("poison", (float("nan"), float("inf"), float("-inf")))
def test_non_finite_coordinates(poison):
    """One non-finite vertex coordinate of the right hand in frame k touches acc/r in the rows k-1..k+1 and nothing else: a NaN
    gives NaN there and acc/h falls back to acc/l; an infinity gives +inf in acc/r and in acc/h (see the module docstring)."""
    from hands_amd import evaluate_accel_metrics
    T, V, k = 7, 257, 3
    pred, targets = AR.sequence(T, V, seed=8)
    base = evaluate_accel_metrics(_cuda(pred), _cuda(targets))
    bad = {key: v.copy() for key, v in pred.items()}
    bad["mano.v3d.cam.r"][k, 100, 1] = poison
    got = evaluate_accel_metrics(_cuda(bad), _cuda(targets))
    ref = AR.evaluate_accel(bad, targets)
    rows = torch.zeros(T, dtype=torch.bool)
    rows[k - 1:k + 2] = True
    b, g = _bits(base), _bits(got)
    for key in KEYS9:
        close(f"poison {poison} {key}", got[key], ref[key])
        if key in ("acc/r", "acc/h"):
            assert torch.equal(g[key][~rows], b[key][~rows]), key
        else:
            assert torch.equal(g[key], b[key]), key
    if np.isnan(poison):
        assert bool(torch.isnan(got["acc/r"][rows]).all()) and torch.equal(g["acc/h"][rows], b["acc/l"][rows])
    else:
        assert bool((got["acc/r"][rows] == float("inf")).all()) and bool((got["acc/h"][rows] == float("inf")).all())
    assert not bool(torch.isfinite(got["acc/r"][rows]).any()) and bool(torch.isfinite(got["acc/r"][1:-1][~rows[1:-1]]).all())


def test_an_invalid_frame_is_not_looked_at():
    from hands_amd import accel_error, evaluate_accel_metrics
    T, V, k = 7, 257, 3
    pred, targets = AR.sequence(T, V, seed=9)
    targets["right_valid"][k] = 0
    base = _bits(evaluate_accel_metrics(_cuda(pred), _cuda(targets)))
    bad_p, bad_t = ({key: v.copy() for key, v in d.items()} for d in (pred, targets))
    for d in (bad_p, bad_t):
        d["mano.v3d.cam.r"][k] = np.nan
        d["mano.j3d.cam.r"][k] = np.nan
    got = _bits(evaluate_accel_metrics(_cuda(bad_p), _cuda(bad_t)))
    for key in KEYS9:
        assert torch.equal(got[key], base[key]), key
    x, y = (torch.from_numpy(d["mano.v3d.cam.l"]).cuda() for d in (targets, pred))
    valid = torch.ones(T)
    valid[k] = 0
    first = accel_error(x, y, valid=valid)
    x[k], y[k] = float("nan"), float("nan")
    assert torch.equal(accel_error(x, y, valid=valid).view(torch.int32), first.view(torch.int32))
    assert bool(torch.isnan(first[k - 1:k + 2]).all()) and bool(torch.isfinite(first[[1, 5]]).all())


# ---- 6. position independence ------------------------------------------------------------------------------------------------
def test_a_window_gives_the_same_bits_wherever_it_stands():
    from hands_amd import accel_error, evaluate_accel_metrics
    V = 778
    three = AR.sequence(3, V, seed=10)
    seen, seen_prim = [], []
    for T, at in ((3, 0), (5, 0), (9, 5), (9, 5), (4, 1)):
        pred, targets = AR.sequence(T, V, seed=20 + T)
        for d, w in ((pred, three[0]), (targets, three[1])):
            for key in d:
                d[key][at:at + 3] = w[key]
        out = evaluate_accel_metrics(_cuda(pred), _cuda(targets))
        seen.append(torch.stack([out[key][at + 1] for key in KEYS9]).cpu().view(torch.int32))
        prim = accel_error(torch.from_numpy(targets["mano.v3d.cam.r"]).cuda(), torch.from_numpy(pred["mano.v3d.cam.r"]).cuda())
        seen_prim.append(prim[at + 1].cpu().view(torch.int32))
    assert bool(torch.isfinite(seen[0].view(torch.float32)).all())
    for s, p in zip(seen[1:], seen_prim[1:]):
        assert torch.equal(s, seen[0]) and torch.equal(p, seen_prim[0])


# ---- 7. streaming ------------------------------------------------------------------------------------------------------------
def test_stream_in_batches_on_the_device():
    from hands_amd import AccelMetrics, evaluate_accel_metrics
    pred, targets = stream_case(V=300)
    T = sum(BATCHES)
    ints = torch.tensor([{"a": 7, "b": 3, "c": 11}[s] for s in STREAM_IDS])
    one = {k: v.cpu().numpy() for k, v in evaluate_accel_metrics(_cuda(pred), _cuda(targets), seq_id=ints).items()}
    metric = AccelMetrics()
    runs = [run_stream(metric, pred, targets, STREAM_IDS, dev="cuda")]
    metric.reset()
    runs.append(run_stream(metric, pred, targets, ints, dev="cuda"))
    assert np.isfinite(one["acc/h"]).sum() >= 3
    for got in runs:
        for k in KEYS9:
            assert got[k].dtype == np.float32 and np.isnan(got[k][:2]).all(), k
            nan = np.isnan(one[k][1:T - 1])
            assert np.array_equal(np.isnan(got[k][2:]), nan), k
            assert np.array_equal(got[k][2:][~nan], one[k][1:T - 1][~nan]), k            # rows 2..T-1 against rows 1..T-2
    ref = AR.stream([(pred, targets, ints.numpy())])
    for k in KEYS9:
        close(f"stream {k}", torch.from_numpy(runs[0][k]), ref[k])


# ---- 8. the wrapper ----------------------------------------------------------------------------------------------------------
def test_wrapper_accel_metrics(golden_dir, recipe_model):
    from hands_amd import evaluate_accel_metrics
    from hands_amd.weights import synthetic_inputs
    from hands_amd.wrapper import HandsWrapper
    B = 3
    d = np.load(os.path.join(golden_dir, "process_data.npz"))
    tin = {k[3:]: torch.from_numpy(d[k])[:B] for k in d.files if k.startswith("in/")}
    K = tin.pop("intrinsics")
    assert K.shape[0] == B
    targets = {k: v.cuda() for k, v in tin.items()}
    g = torch.Generator().manual_seed(1)
    for h in "rl":
        targets[f"mano.j2d.norm.{h}"] = (0.5 * torch.randn(B, 21, 2, generator=g)).cuda()
        targets[f"joints_valid_{h}"] = torch.ones(B, 21).cuda()
    targets.update(is_valid=torch.ones(B).cuda(), right_valid=torch.ones(B).cuda(), left_valid=torch.ones(B).cuda())
    calls = []
    for seed in (4, 5):
        inputs, meta = synthetic_inputs(B, seed, device="cuda")
        meta["intrinsics"] = K.cuda()
        meta["imgname"] = [f"{seed}/{i}.jpg" for i in range(B)]
        calls.append((inputs, meta))
    w = HandsWrapper(model=copy.deepcopy(recipe_model).to("cuda"))
    today = ["imgname"] + ["metric." + k for k in ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l",
                                                   "pix_err/r", "pix_err/l", "pix_err/h")]
    out0, _ = w.forward(*calls[0][:1], dict(targets), calls[0][1], "test")
    assert list(out0) == today                                                           # without the name: what it was
    w.metric_dict = w.metric_dict + ["accel"]
    keys = ["metric." + k for k in KEYS9]
    outs = [w.forward(inputs, dict(targets), meta, "test")[0] for inputs, meta in calls]
    assert list(outs[0]) == today + keys and list(outs[1]) == today + keys
    for k in today[1:]:
        assert torch.equal(outs[0][k].view(torch.int32), out0[k].view(torch.int32)), k
    first, second = outs[0]["metric.acc/h"], outs[1]["metric.acc/h"]
    assert first.device.type == "cpu" and first.shape == (B,)
    assert torch.isnan(first).tolist() == [True, True, False] and not bool(torch.isnan(second).any())      # the carry works
    # "extract" is no frame of the stream: the object still holds the last two frames of the second call
    full = [w.forward(inputs, dict(targets), meta, "extract") for inputs, meta in calls]
    need = [f"mano.{q}.cam.{h}" for q in ("v3d", "j3d") for h in "rl"]
    cat = lambda prefix, names: {k: torch.cat([f[prefix + k] for f in full]).cuda() for k in names}
    one = evaluate_accel_metrics(cat("pred.", need), cat("targets.", need + ["is_valid", "right_valid", "left_valid"]),
                                 fps=w.accel_fps)
    for k in KEYS9:
        got = torch.cat([outs[0]["metric." + k], outs[1]["metric." + k]])
        assert bool(torch.isnan(got[:2]).all()) and not bool(torch.isnan(got[2:]).any()), k
        assert torch.equal(got[2:], one[k][1:2 * B - 1].cpu()), k                        # rows 2..5 against rows 1..4
    third = w.forward(*calls[0][:1], dict(targets), calls[0][1], "test")[0]
    assert not bool(torch.isnan(third["metric.acc/h"]).any())
    w.reset_accel()
    again = w.forward(*calls[0][:1], dict(targets), calls[0][1], "test")[0]
    for k in keys:
        assert torch.equal(again[k].view(torch.int32), outs[0][k].view(torch.int32)), k
