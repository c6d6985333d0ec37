#!/usr/bin/env python3
"""Device time of temporal smoothing (hands_smooth_mano_f32, csrc/smooth.hip, then the fused MANO head) for 256 hand pairs, as
(T, S) = (256, 1) -- consecutive frames of one video -- and (1, 256) -- one frame of each of 256 cameras, the state carried.

Times ``hands_amd.smooth_predictions`` -- the Python function with its allocations: one filter launch, one MANO launch -- against
the same filter written with torch ops on the same device (fp64, batched over hands, streams and channels, a Python loop over
time) followed by the same MANO launch.  The two are checked against each other, with the bar of tests/test_gpu_smoothing.py,
before either is timed.  Two more entries in the rotation: the filter launch alone through the C ABI with pre-bound structs, and
the filter-free re-pose (``run_mano_heads`` on the raw parameters) it feeds.  Device events around ``calls`` back-to-back calls,
a timed window at least ``--window-ms`` long; the versions alternate in one process, the median over ``--runs`` windows each.
``--forward-ms`` is the time of a HandsLight forward at bz = 256 the share is taken of (docs/EXPERIMENTS.md records it; this
tool does not run the trunks).  The inputs stay away from the half-turn branch of Log, which the torch version leaves out.  No
profiler.  Prints one JSON line per layout."""
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


def hat(torch, w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).view(w.shape[:-1] + (3, 3))


def exp_so3(torch, w):
    th = w.norm(dim=-1)[..., None, None]
    K = hat(torch, w)
    small = th < 1e-6
    safe = torch.where(small, torch.ones_like(th), th)
    a = torch.where(small, torch.ones_like(th), torch.sin(safe) / safe)
    b = torch.where(small, torch.full_like(th, 0.5), (1.0 - torch.cos(safe)) / (safe * safe))
    return torch.eye(3, dtype=w.dtype, device=w.device) + a * K + b * (K @ K)


def log_so3(torch, D):
    v = 0.5 * torch.stack([D[..., 2, 1] - D[..., 1, 2], D[..., 0, 2] - D[..., 2, 0], D[..., 1, 0] - D[..., 0, 1]], -1)
    s = v.norm(dim=-1, keepdim=True)
    c = 0.5 * (D[..., 0, 0] + D[..., 1, 1] + D[..., 2, 2] - 1.0)[..., None]
    big = s >= 1e-9
    return torch.where(big, v * (torch.atan2(s, c) / torch.where(big, s, torch.ones_like(s))), v)


def make_params(torch, T, S, seed):
    """pose (2, T*S, 16, 3, 3), beta (2, T*S, 10), cam (2, T*S, 3) fp32, rows t * S + s: every channel on a smooth path of its own
    with 0.03 rad / 0.03 / 0.01 of noise a frame."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g, dtype=torch.float64)
    t = torch.arange(T, device="cuda", dtype=torch.float64).view(1, T, 1, 1, 1) / 30.0
    w = 0.4 * r(2, 1, S, 16, 3) + 0.3 * torch.sin(3.0 * t + r(2, 1, S, 16, 3)) + 0.03 * r(2, T, S, 16, 3)
    pose = exp_so3(torch, w).view(2, T * S, 16, 3, 3)
    t = t.view(1, T, 1, 1)
    beta = (r(2, 1, S, 10) + 0.03 * r(2, T, S, 10)).view(2, T * S, 10)
    cam = (torch.tensor([0.9, 0.0, 0.0], device="cuda") + 0.05 * torch.sin(2.0 * t + r(2, 1, S, 3)) + 0.01 * r(2, T, S, 3)).view(2, T * S, 3)
    return pose.float().contiguous(), beta.float().contiguous(), cam.float().contiguous()


class TorchFilter:
    """The filter of DESIGN.md section 7 with torch ops, every frame usable and of one sequence, ``shape_mode="filter"``: the state
    is carried between calls as the kernel's is."""

    def __init__(self, torch, fps, mc=1.5, beta=0.5, dc=1.0):
        self.torch, self.dt, self.mc, self.beta, self.dc, self.st = torch, 1.0 / fps, mc, beta, dc, None

    def alpha(self, f):
        r = 2.0 * math.pi * f * self.dt
        return r / (r + 1.0)

    def vector(self, st, x):
        d = (x - st["raw"]) / self.dt
        st["d"] = st["d"] + self.alpha(self.dc) * (d - st["d"])
        st["hat"] = st["hat"] + self.alpha(self.mc + self.beta * st["d"].norm(dim=-1, keepdim=True)) * (x - st["hat"])
        st["raw"] = x
        return st["hat"]

    def __call__(self, pose, beta, cam, T, S):
        torch = self.torch
        P, Bv, Cv = pose.double().view(2, T, S, 16, 3, 3), beta.double().view(2, T, S, 10), cam.double().view(2, T, S, 3)
        out = [], [], []
        for t in range(T):
            R, b, c = P[:, t], Bv[:, t], Cv[:, t]
            if self.st is None:
                self.st = {"raw": R, "hat": R, "w": torch.zeros_like(R[..., 0]), "shape": {"raw": b, "hat": b, "d": torch.zeros_like(b)},
                           "cam": {"raw": c, "hat": c, "d": torch.zeros_like(c)}}
                res = R, b, c
            else:
                st = self.st
                w = log_so3(torch, st["raw"].transpose(-1, -2) @ R) / self.dt
                st["w"] = st["w"] + self.alpha(self.dc) * (w - st["w"])
                a = self.alpha(self.mc + self.beta * st["w"].norm(dim=-1, keepdim=True))
                st["hat"] = st["hat"] @ exp_so3(torch, a * log_so3(torch, st["hat"].transpose(-1, -2) @ R))
                st["raw"] = R
                res = st["hat"], self.vector(st["shape"], b), self.vector(st["cam"], c)
            for o, v in zip(out, res):
                o.append(v)
        return tuple(torch.stack(o, 1).float().reshape((2 * T * S,) + o[0].shape[2:]) for o in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=256, help="rows per hand: T of the 'time' case, S of the 'streams' case")
    ap.add_argument("--fps", type=float, default=30.0)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    ap.add_argument("--forward-ms", type=float, default=45.10, help="HandsLight forward at bz = 256 (docs/EXPERIMENTS.md)")
    a = ap.parse_args()
    import torch
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import run_mano_heads
    from hands_amd.smoothing import smooth_state
    if not torch.cuda.is_available():
        raise SystemExit("bench_smoothing.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    B = a.hands
    model = hands_amd.HandsLight().to(dev)
    P = model.packed(dev)
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]], device=dev).repeat(B, 1, 1)
    meta = {"intrinsics": K}
    repose = lambda rot, shape, cam: run_mano_heads(L, P["mano_r"], P["mano_l"], rot, shape, cam, cam, K, float(model.img_res), B,
                                                    st.cuda_stream, None)

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    for layout, T, S in (("time", B, 1), ("streams", 1, B)):
        flat = lambda x: x.reshape((2 * B,) + x.shape[2:])
        if layout == "time":
            frames, state = [make_params(torch, T, S, seed=7)], None
        else:
            # three consecutive frames of the S streams: the first starts them, the timed calls take the other two in turn with
            # the state carried, so that the filter keeps moving (a constant input would converge onto the cheap branch of Log)
            three = make_params(torch, 3, S, seed=7)
            frames = [tuple(x[:, i * S:(i + 1) * S].contiguous() for x in three) for i in range(3)]
            state = smooth_state(2, S, dev)
        preds = [repose(*(flat(x) for x in f)) for f in frames]
        tf = TorchFilter(torch, a.fps)
        if layout == "streams":
            hands_amd.smooth_predictions(preds[0], model, meta, fps=a.fps, layout=layout, state=state)
            tf(*frames[0], T, S)
            frames, preds = frames[1:], preds[1:]
        turn = {"hip": 0, "ops": 0, "abi": 0, "raw": 0}

        def nxt(name):
            turn[name] = (turn[name] + 1) % len(frames)
            return turn[name]

        hip = lambda: hands_amd.smooth_predictions(preds[nxt("hip")], model, meta, fps=a.fps, layout=layout, state=state)

        def ops():
            if layout == "time":
                tf.st = None
            return repose(*tf(*frames[nxt("ops")], T, S))
        raw = lambda: repose(*(flat(x) for x in frames[nxt("raw")]))
        outs = [torch.empty_like(flat(x)) for x in frames[0]]
        bound = []
        for pose, beta, cam in frames:
            sides = (_lib.SmoothSide * 2)()
            for i in range(2):
                sides[i] = _lib.SmoothSide(_lib.ptr(pose[i]), _lib.ptr(beta[i]), _lib.ptr(cam[i]), None, _lib.ptr(outs[0][i * B:]),
                                           _lib.ptr(outs[1][i * B:]), _lib.ptr(outs[2][i * B:]), None if state is None else _lib.ptr(state[i]))
            bound.append(sides)
        cfg = hands_amd.SmoothConfig().c_struct()
        abi = lambda: _lib.check(L.hands_smooth_mano_f32(bound[nxt("abi")], 2, None, T, S, a.fps, C.byref(cfg), st.cuda_stream),
                                 "hands_smooth_mano_f32")

        # the two agree before either is timed (from the same state: snapshot and restore it around the check)
        keep = None if state is None else state.clone()
        keep_tf = None if tf.st is None else {k: (dict(v) if isinstance(v, dict) else v) for k, v in tf.st.items()}
        got, ref = hip(), ops()
        if state is not None:
            state.copy_(keep)
            tf.st = keep_tf
        worst = 0.0
        for h, sl in (("r", slice(0, B)), ("l", slice(B, 2 * B))):
            for k, absolute in (("pose", True), ("beta", False), ("cam_t.wp", False)):
                g, r = got[f"mano.{k}.{h}"].double(), ref[f"mano.{k}.{h}"].double()
                bar = 4 * 2.0 ** -24 * (torch.ones_like(r) if absolute else r.abs()) + 1e-12
                worst = max(worst, float(((g - r).abs() / bar).max()))
        if worst > 1.0:
            raise SystemExit(f"{layout}: kernel and torch ops disagree: {worst:.2f} of the bar")
        turn.update(hip=0, ops=0)
        moved = float((got["mano.pose.r"] - preds[1 % len(frames)]["mano.pose.r"]).abs().max())

        fns = (("hip", hip), ("ops", ops), ("abi", abi), ("raw", raw))
        calls = {}
        for name, fn in fns:
            for _ in range(3):                             # warm-up: code objects, the allocator's blocks
                fn()
            torch.cuda.synchronize()
            per_call = window_us(fn, 5) / 5
            calls[name] = max(5, math.ceil(1e3 * a.window_ms / per_call))
        t = {name: [] for name, _ in fns}
        for _ in range(a.runs):                            # alternating
            for name, fn in fns:
                t[name].append(window_us(fn, calls[name]) / calls[name])
        us = {k: statistics.median(v) for k, v in t.items()}
        mm = lambda k: [round(min(t[k]), 2), round(max(t[k]), 2)]
        print(json.dumps({"tool": "bench_smoothing", "layout": layout, "T": T, "S": S, "fps": a.fps, "runs": a.runs,
                          "calls_per_window": calls, "worst_diff_over_bar": round(worst, 3), "largest_pose_change": round(moved, 4),
                          "hip_us": round(us["hip"], 2), "hip_us_min_max": mm("hip"),
                          "torch_ops_us": round(us["ops"], 2), "torch_ops_us_min_max": mm("ops"),
                          "torch_ops_over_hip": round(us["ops"] / us["hip"], 2),
                          "filter_launch_alone_us": round(us["abi"], 2), "filter_launch_alone_us_min_max": mm("abi"),
                          "repose_alone_us": round(us["raw"], 2), "repose_alone_us_min_max": mm("raw"),
                          "filter_over_repose": round(us["abi"] / us["raw"], 2),
                          "forward_ms": a.forward_ms, "share_of_forward": round(us["hip"] / (1e3 * a.forward_ms), 5)}), flush=True)


if __name__ == "__main__":
    main()
