#!/usr/bin/env python3
"""Device time of the acceleration metrics (hands_eval_accel_metrics_f32, csrc/accel.hip: one launch) at T = 256, V = 778.

Times ``hands_amd.evaluate_accel_metrics`` -- the Python function with its allocation -- against the same nine keys composed with
torch ops on the same device, in fp64 like the kernel (the reference's fp32 form misses the parity bar through cancellation).
The two are checked against each other, with the bar of tests/test_gpu_accel_metrics.py, before either is timed.  Device events
around ``calls`` back-to-back calls, the number chosen so that a timed window is well over a tenth of a second; the two versions
alternate in one process, the median over ``--runs`` windows each; a third entry in the rotation is the launch alone, through the
C ABI with pre-bound structs.  ``--forward-ms`` is the time of a HandsLight forward at
bz = 256 the share is taken of (docs/EXPERIMENTS.md records it; this tool does not run the model).  No profiler.  Prints one
JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")


def make_case(torch, T, V, seed):
    """Two hands on smooth paths around z = 0.6 / 0.7 m, 3 mm of noise on the prediction, a tenth of the left hands invalid and a
    change of sequence every 64 frames."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    t = torch.arange(T, device="cuda", dtype=torch.float32)[:, None, None] / 30.0
    pred, targets = {}, {}
    for h, centre in (("r", (-0.1, 0.0, 0.6)), ("l", (0.1, 0.02, 0.7))):
        path = torch.cat([0.05 * torch.sin(3.0 * t), 0.03 * torch.cos(2.0 * t), 0.02 * torch.sin(t)], -1)
        gt = 0.04 * r(1, V + 21, 3) * (1.0 + 0.2 * torch.sin(2.0 * t)) + path + torch.tensor(centre, device="cuda")
        pr = gt + 0.003 * r(T, V + 21, 3)
        targets[f"mano.v3d.cam.{h}"], targets[f"mano.j3d.cam.{h}"] = gt[:, :V].contiguous(), gt[:, V:].contiguous()
        pred[f"mano.v3d.cam.{h}"], pred[f"mano.j3d.cam.{h}"] = pr[:, :V].contiguous(), pr[:, V:].contiguous()
    targets.update(is_valid=torch.ones(T, device="cuda"), right_valid=torch.ones(T, device="cuda"),
                   left_valid=(torch.rand(T, device="cuda", generator=g) > 0.1).float())
    return pred, targets, torch.arange(T, device="cuda") // 64


def torch_accel_metrics(torch, pred, targets, seq, fps):
    """The nine keys with torch ops on the device, fp64 from the first subtraction on."""
    nan = float("nan")
    same = (seq[:-2] == seq[1:-1]) & (seq[1:-1] == seq[2:])

    def err(g, p):
        ag = (g[:-2] - 2.0 * g[1:-1] + g[2:]) * (fps * fps)
        ap = (p[:-2] - 2.0 * p[1:-1] + p[2:]) * (fps * fps)
        return (ap - ag).norm(dim=2).mean(dim=1)

    out = {}
    for h, hv in (("r", "right_valid"), ("l", "left_valid")):
        v = targets[hv] * targets["is_valid"] != 0
        ok = v[:-2] & v[1:-1] & v[2:] & same
        pv, gv = pred[f"mano.v3d.cam.{h}"].double(), targets[f"mano.v3d.cam.{h}"].double()
        pj, gj = pred[f"mano.j3d.cam.{h}"].double(), targets[f"mano.j3d.cam.{h}"].double()
        for k, e in (("acc", err(gv - gj[:, :1], pv - pj[:, :1])), ("acc/j", err(gj - gj[:, :1], pj - pj[:, :1])),
                     ("acc/abs", err(gj, pj))):
            e = torch.where(ok, e, torch.full_like(e, nan)).float()
            out[f"{k}/{h}"] = torch.nn.functional.pad(e, (1, 1), value=nan)
    for k in ("acc", "acc/j", "acc/abs"):
        out[k + "/h"] = torch.stack([out[k + "/r"], out[k + "/l"]], 1).nanmean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--verts", type=int, default=778)
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    ap.add_argument("--forward-ms", type=float, default=45.10, help="HandsLight forward at bz = 256 (docs/EXPERIMENTS.md)")
    a = ap.parse_args()
    import torch
    from hands_amd import _lib, evaluate_accel_metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_accel_metrics.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    T, V = a.frames, a.verts
    pred, targets, seq = make_case(torch, T, V, seed=7)
    hip = lambda: evaluate_accel_metrics(pred, targets, fps=a.fps, seq_id=seq)
    ops = lambda: torch_accel_metrics(torch, pred, targets, seq, a.fps)
    # the launch alone, through the C ABI with pre-bound structs: what is left of `hip` without the Python around it
    keep = [pred["mano.v3d.cam.r"], pred["mano.v3d.cam.l"], targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"],
            pred["mano.j3d.cam.r"], pred["mano.j3d.cam.l"], targets["mano.j3d.cam.r"], targets["mano.j3d.cam.l"],
            targets["is_valid"], targets["right_valid"], targets["left_valid"]]
    buf, seq32 = torch.empty(9, T, device="cuda"), seq.to(torch.int32)
    fin, fout = _lib.MeshEvalIn(*[_lib.ptr(x) for x in keep]), _lib.AccelEvalOut(*[_lib.ptr(buf[i]) for i in range(9)])
    L = _lib.lib()
    abi = lambda: _lib.check(L.hands_eval_accel_metrics_f32(C.byref(fin), _lib.ptr(seq32), C.byref(fout), T, V, a.fps, st.cuda_stream),
                             "hands_eval_accel_metrics_f32")

    got, ref = hip(), ops()                                # the two agree before either is timed
    worst = 0.0
    for k in got:
        assert torch.equal(got[k].isnan(), ref[k].isnan()), k
        m = ~ref[k].isnan()
        d = (got[k][m].double() - ref[k][m].double()).abs()
        bar = 4 * 2.0 ** -24 * ref[k][m].double().abs() + 1e-10 * (a.fps / 30.0) ** 2
        worst = max(worst, float((d / bar).max()))         # two roundings of nearly one fp64 value to fp32: one ulp = 2 * 2^-24
    if worst > 1.0:
        raise SystemExit(f"kernel and torch ops disagree: {worst:.2f} of the bar")

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    calls = {}
    for name, fn in (("hip", hip), ("ops", ops), ("abi", abi)):
        for _ in range(10):                                # warm-up: code objects, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        per_call = window_us(fn, 50) / 50
        calls[name] = max(50, math.ceil(1e3 * a.window_ms / per_call))
    t = {"hip": [], "ops": [], "abi": []}
    for _ in range(a.runs):                                # alternating
        for name, fn in (("hip", hip), ("ops", ops), ("abi", abi)):
            t[name].append(window_us(fn, calls[name]) / calls[name])
    us = {k: statistics.median(v) for k, v in t.items()}
    live = int((~got["acc/r"].isnan()).sum() + (~got["acc/l"].isnan()).sum())
    print(json.dumps({"tool": "bench_accel_metrics", "frames": T, "verts": V, "fps": a.fps, "runs": a.runs,
                      "calls_per_window": calls, "window_ms": {k: round(us[k] * calls[k] / 1e3, 1) for k in us},
                      "scored_hand_rows": live, "worst_diff_over_bar": round(worst, 3),
                      "hip_us": round(us["hip"], 2), "hip_us_min_max": [round(min(t["hip"]), 2), round(max(t["hip"]), 2)],
                      "torch_ops_us": round(us["ops"], 2), "torch_ops_us_min_max": [round(min(t["ops"]), 2), round(max(t["ops"]), 2)],
                      "torch_ops_over_hip": round(us["ops"] / us["hip"], 2),
                      "launch_alone_us": round(us["abi"], 2), "launch_alone_us_min_max": [round(min(t["abi"]), 2), round(max(t["abi"]), 2)],
                      "forward_ms": a.forward_ms, "share_of_forward": round(us["hip"] / (1e3 * a.forward_ms), 5)}))


if __name__ == "__main__":
    main()
