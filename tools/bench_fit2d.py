#!/usr/bin/env python3
"""Device time of MANO fitting to 2-D keypoints (hands_mano_fit2d_f32, csrc/fit.hip) for 256 hand pairs at the default
``Fit2DConfig`` (10 rigid + 30 full iterations), beside the 3-D fit (hands_mano_fit_f32) at the same total iteration count on
the 3-D joints the keypoints were projected from.  Both launches go through the C ABI with pre-bound structs, alternate in one
process, and are timed with device events around ``calls`` back-to-back launches in a window at least ``--window-ms`` long; the
median over ``--runs`` windows each and the spread (min, max) are reported, per launch and per iteration.  No threshold is fixed in
advance: docs/EXPERIMENTS.md records the two per-iteration times and explains a difference beyond the 3-D kernel's own spread
from the resource report.  The targets are those of tools/bench_fit.py (the family of DESIGN.md section 7), projected with
f = 1000 px, c = 112 px.  No profiler.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")

KEYS = ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs", "tip_lbs_weights", "tip_posedirs")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=256, help="hand pairs (B)")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hands_amd
    from bench_fit import TorchFit, exp_so3
    from hands_amd import _lib
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit2d.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    L, B = _lib.lib(), a.hands
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], dev)
    tf = TorchFit(torch, packs, B)                          # only its forward kinematics, for the targets

    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.float64)
    aa = tf.pm + torch.cat([2.0 * rn(2 * B, 1, 3), 0.5 * rn(2 * B, 15, 3)], 1)
    y3 = tf.evaluate(exp_so3(torch, aa), rn(2 * B, 10))[5] + torch.tensor([0.05, -0.03, 0.6], device=dev) + 0.1 * rn(2 * B, 1, 3)
    y2 = (1000.0 * y3[..., :2] / y3[..., 2:] + 112.0).float()
    y3 = y3.float()
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]], device=dev).repeat(B, 1, 1).contiguous()

    cfg2 = hands_amd.Fit2DConfig()
    total = cfg2.iters_rigid + cfg2.iters
    c2, c3 = cfg2.c_struct(), hands_amd.FitConfig(iters=total).c_struct()
    new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)
    o2 = [(new(B, 16, 3, 3), new(B, 10), new(B, 3), new(B), new(B, dt=torch.int32), new(B, dt=torch.int32), new(B, 21, 3), new(B, 21, 2))
          for _ in range(2)]
    o3 = [o[:5] for o in o2]
    s2, s3 = (_lib.ManoFit2DSide * 2)(), (_lib.ManoFitSide * 2)()
    ins2, ins3 = [y2[:B].contiguous(), y2[B:].contiguous()], [y3[:B].contiguous(), y3[B:].contiguous()]
    for i in range(2):
        consts = _lib.ManoFitConsts(*[_lib.ptr(packs[i][k]) for k in KEYS])
        s2[i] = _lib.ManoFit2DSide(consts, _lib.ptr(ins2[i]), None, None, None, None, None, *[_lib.ptr(o) for o in o2[i]])
        s3[i] = _lib.ManoFitSide(consts, _lib.ptr(ins3[i]), None, None, None, None, None, *[_lib.ptr(o) for o in o3[i]])
    fit2d = lambda: _lib.check(L.hands_mano_fit2d_f32(s2, 2, _lib.ptr(K), C.byref(c2), B, st.cuda_stream), "hands_mano_fit2d_f32")
    fit3d = lambda: _lib.check(L.hands_mano_fit_f32(s3, 2, C.byref(c3), B, st.cuda_stream), "hands_mano_fit_f32")

    fit2d()
    torch.cuda.synchronize()
    rm = np.sort(torch.cat([o2[0][3], o2[1][3]]).cpu().numpy())
    steps = torch.cat([o2[0][4], o2[1][4]]).cpu().numpy()
    if not np.isfinite(rm).all():
        raise SystemExit("a hand of the benchmark was not fitted")

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    fns = (("fit2d", fit2d), ("fit3d", fit3d))
    calls = {}
    for name, fn in fns:
        for _ in range(2):                                 # warm-up: code objects
            fn()
        torch.cuda.synchronize()
        calls[name] = max(2, math.ceil(1e3 * a.window_ms / (window_us(fn, 2) / 2)))
    t = {name: [] for name, _ in fns}
    for _ in range(a.runs):                                # alternating
        for name, fn in fns:
            t[name].append(window_us(fn, calls[name]) / calls[name])
    us = {k: statistics.median(v) for k, v in t.items()}
    per = lambda k, v: round(v / total, 2)
    print(json.dumps({"tool": "bench_fit2d", "hands": B, "sides": 2, "iters_rigid": cfg2.iters_rigid, "iters": cfg2.iters,
                      "runs": a.runs, "calls_per_window": calls,
                      "rmse_px_min_median_max": [float(f"{rm[0]:.3e}"), float(f"{rm[len(rm) // 2]:.3e}"), float(f"{rm[-1]:.3e}")],
                      "hands_above_1_px": int((rm > 1.0).sum()), "accepted_steps_median": float(np.median(steps)),
                      "fit2d_us": round(us["fit2d"], 1), "fit2d_us_min_max": [round(min(t["fit2d"]), 1), round(max(t["fit2d"]), 1)],
                      "fit3d_us": round(us["fit3d"], 1), "fit3d_us_min_max": [round(min(t["fit3d"]), 1), round(max(t["fit3d"]), 1)],
                      "fit2d_us_per_iteration": per("fit2d", us["fit2d"]),
                      "fit2d_us_per_iteration_min_max": [per("fit2d", min(t["fit2d"])), per("fit2d", max(t["fit2d"]))],
                      "fit3d_us_per_iteration": per("fit3d", us["fit3d"]),
                      "fit3d_us_per_iteration_min_max": [per("fit3d", min(t["fit3d"])), per("fit3d", max(t["fit3d"]))],
                      "fit2d_over_fit3d": round(us["fit2d"] / us["fit3d"], 3)}), flush=True)


if __name__ == "__main__":
    main()
