#!/usr/bin/env python3
"""Device time of MANO fitting to 778 vertices (hands_mano_fit_verts_f32, csrc/fit_verts.hip) for 256 hand pairs at the default
configuration, for fully weighted targets and for targets with 20 weighted vertices, beside the fit to 21 joints
(hands_mano_fit_f32) at the same B and iters in the same process, and against the same algorithm -- DESIGN.md section 7 "MANO
fitting to 778 vertices" -- written with batched torch ops in fp64 on the same device (a Python loop over the iterations; the
Jacobian of all hands is one (N, 2334, 61) tensor).

Times ``hands_amd.fit_mano_hands_verts`` (the Python function with its allocations) and the fit launch alone through the C ABI
with pre-bound structs, at ``--iters`` and at 0 iterations: the difference over ``--iters`` is the time of an iteration.  Before
anything is timed, the kernel's rmse is checked against its own outputs (recomputed with the torch forward) and the two versions
are compared hand by hand: 99 % of the hands have to agree within 1e-6 m, or the tool refuses to report.  Device events around
back-to-back calls, a timed window at least ``--window-ms`` long; the versions alternate in one process, the median over
``--runs`` windows each.  ``--forward-ms`` is the time of a HandsLight forward at bz = 256 the share is taken of
(docs/EXPERIMENTS.md records it; this tool does not run the trunks).  ``--only kernel`` times nothing but the vertex fit's launch
(for a counter run under a profiler).  Prints one JSON line."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")

from bench_fit import KEYS as JOINT_KEYS, PARENTS, exp_so3, hat, log_so3  # noqa: E402

KEYS = ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights", "posedirs_vm")
NV = 778


class TorchFitVerts:
    """The fit over N hands at once (every row fitted, the half-turn branch of Log left out).  Constants carry a leading hand
    dimension, so both sides go through one batch."""

    def __init__(self, torch, packs, B, iters=30, lb=1e-6, lp=1e-6, mu0=1e-3):
        self.t, self.iters, self.lb, self.lp, self.mu0, self.retried = torch, iters, lb, lp, mu0, 0
        rep = lambda k, *s: torch.cat([p[k].double().view(1, *s).expand(B, *s) for p in packs]).contiguous()
        self.pm, self.Jt, self.Js = rep("pose_mean", 16, 3), rep("J_template", 16, 3), rep("J_shapedirs", 16, 3, 10)
        self.vt, self.sd, self.W = rep("v_template", NV, 3), rep("shapedirs", NV, 3, 10), rep("lbs_weights", NV, 16)
        self.pd = rep("posedirs_vm", NV, 15, 9, 3)
        self.M = exp_so3(torch, self.pm)
        dev = self.M.device
        below = [[j == 0 or (i >= j and (i - 1) // 3 == (j - 1) // 3) for i in range(16)] for j in range(16)]
        self.below = torch.tensor(below, dtype=torch.float64, device=dev)                  # [j, i]: i at or below j
        self.E = hat(torch, torch.eye(3, dtype=torch.float64, device=dev))                 # [e_a]x
        prior = torch.zeros(61, dtype=torch.float64, device=dev)
        prior[3:48], prior[48:58] = lp, lb
        self.prior = prior

    def factor(self, Ad):
        """As bench_fit.TorchFit.factor: a batched cholesky_ex that reports failures is repeated, up to twice."""
        t = self.t
        for _ in range(3):
            L, info = t.linalg.cholesky_ex(Ad)
            if not bool((info != 0).any()):
                break
            self.retried += 1
        return L, info == 0

    def evaluate(self, R, beta):
        t = self.t
        J = self.Jt + t.einsum("njcl,nl->njc", self.Js, beta)
        Q, p = [R[:, 0]], [J[:, 0]]
        for i in range(1, 16):
            a = PARENTS[i]
            Q.append(Q[a] @ R[:, i])
            p.append(p[a] + (Q[a] @ (J[:, i] - J[:, a])[..., None])[..., 0])
        Q, p = t.stack(Q, 1), t.stack(p, 1)
        pf = (R[:, 1:] - t.eye(3, dtype=R.dtype, device=R.device)).reshape(-1, 15, 9)
        vt = self.vt + t.einsum("nvcl,nl->nvc", self.sd, beta) + t.einsum("njf,nvjfc->nvc", pf, self.pd)
        x = t.einsum("niab,nvib->nvia", Q, vt[:, :, None] - J[:, None]) + p[:, None]
        A = t.einsum("nvi,niab->nvab", self.W, Q)
        v = t.einsum("nvi,nvic->nvc", self.W, x)
        return J, Q, p, x, A, v

    def residual(self, R, beta, tr, y, sw):
        ev = self.evaluate(R, beta)
        r = (sw[..., None] * (ev[5] + tr[:, None] - y)).reshape(-1, 3 * NV)
        lg = log_so3(self.t, self.M[:, 1:].transpose(-1, -2) @ R[:, 1:]).reshape(-1, 45)
        c = (r * r).sum(1) + self.lb * (beta * beta).sum(1) + self.lp * (lg * lg).sum(1)
        return ev, r, lg, c

    def jacobian(self, R, ev, sw):
        t = self.t
        _, Q, p, x, A, _ = ev
        N = R.shape[0]
        D = t.empty(N, NV, 3, 61, dtype=R.dtype, device=R.device)
        s = t.einsum("ji,nvic->nvjc", self.below, self.W[..., None] * x) - t.einsum("ji,nvi->nvj", self.below, self.W)[..., None] * p[:, None]
        blk = -hat(t, s) @ Q[:, None]                                                      # [n, v, j, 3, 3]
        dR = (R[:, 1:, None] @ self.E).reshape(N, 15, 3, 9)                                # [n, j - 1, a, f]
        u = t.einsum("njaf,nvjfc->nvjca", dR, self.pd)
        blk[:, :, 1:] += t.einsum("nvrc,nvjca->nvjra", A, u)
        D[..., :48] = blk.permute(0, 1, 3, 2, 4).reshape(N, NV, 3, 48)
        dp = [self.Js[:, 0]]
        for i in range(1, 16):
            a = PARENTS[i]
            dp.append(dp[a] + Q[:, a] @ (self.Js[:, i] - self.Js[:, a]))
        dp = t.stack(dp, 1)
        D[..., 48:58] = A @ self.sd + t.einsum("nvi,nicl->nvcl", self.W, dp - Q @ self.Js)
        D[..., 58:] = t.eye(3, dtype=R.dtype, device=R.device)
        return (sw[..., None, None] * D).reshape(N, 3 * NV, 61)

    def __call__(self, y, w):
        t = self.t
        y, w = y.double(), w.double()
        y = t.where(w[..., None] > 0, y, t.zeros_like(y))
        sw = w.sqrt()
        N = y.shape[0]
        R, beta = self.M.clone(), t.zeros(N, 10, dtype=t.float64, device=y.device)
        J, _, _, _, _, X = self.evaluate(R, beta)
        ws = w.sum(1, keepdim=True)
        mx, my = (w[..., None] * X).sum(1) / ws, (w[..., None] * y).sum(1) / ws
        K = (w[..., None] * (X - mx[:, None])).transpose(1, 2) @ (y - my[:, None])
        U, _, Vh = t.linalg.svd(K)
        V = Vh.transpose(1, 2)
        d = t.ones(N, 3, dtype=t.float64, device=y.device)
        d[:, 2] = t.linalg.det(V @ U.transpose(1, 2))
        R0 = (V * d[:, None]) @ U.transpose(1, 2)
        R[:, 0] = R0
        tr = my - (R0 @ (mx - J[:, 0])[..., None])[..., 0] - J[:, 0]
        mu = t.full((N,), self.mu0, dtype=t.float64, device=y.device)
        steps = t.zeros(N, dtype=t.int32, device=y.device)
        ev, r, lg, c = self.residual(R, beta, tr, y, sw)
        for _ in range(self.iters):
            Jm = self.jacobian(R, ev, sw)
            H = Jm.transpose(1, 2) @ Jm + t.diag_embed(self.prior.expand(N, -1))
            g = (Jm.transpose(1, 2) @ r[..., None])[..., 0]
            g[:, 3:48] += self.lp * lg
            g[:, 48:58] += self.lb * beta
            Ad = H + t.diag_embed(mu[:, None] * t.diagonal(H, dim1=1, dim2=2))
            L, ok = self.factor(Ad)
            dl = t.cholesky_solve(-g[..., None], L)[..., 0]
            R2 = R @ exp_so3(t, dl[:, :48].reshape(N, 16, 3))
            beta2, tr2 = beta + dl[:, 48:58], tr + dl[:, 58:]
            ev2, r2, lg2, c2 = self.residual(R2, beta2, tr2, y, sw)
            acc = ok & (c2 < c)
            pick = lambda a, b: t.where(acc.view((-1,) + (1,) * (a.dim() - 1)), a, b)
            R, beta, tr, r, lg, c = pick(R2, R), pick(beta2, beta), pick(tr2, tr), pick(r2, r), pick(lg2, lg), pick(c2, c)
            ev = tuple(pick(a, b) for a, b in zip(ev2, ev))
            mu = t.where(acc, (mu / 3.0).clamp_min(1e-9), (5.0 * mu).clamp_max(1e6))
            steps += acc.to(t.int32)
        return R.float(), beta.float(), tr.float(), ((r * r).sum(1) / w.sum(1)).sqrt().float(), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=256, help="hand pairs (B)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    ap.add_argument("--keep", type=int, default=20, help="weighted vertices of the sparse targets")
    ap.add_argument("--only", default="", choices=("", "kernel"), help="kernel: launch the vertex fit alone, 3 calls, no torch version")
    ap.add_argument("--forward-ms", type=float, default=45.10, help="HandsLight forward at bz = 256 (docs/EXPERIMENTS.md)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_verts.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    L, B = _lib.lib(), a.hands
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], dev)
    pair = type("Pair", (), {"packed": lambda self, d: {"mano_r": packs[0], "mano_l": packs[1]}})()
    tf = TorchFitVerts(torch, packs, B, a.iters)

    # targets the model generates itself: global rotation 2 randn, fingers hands_mean + 0.5 randn, beta = randn, rounded to fp32
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.float64)
    aa = tf.pm + torch.cat([2.0 * rn(2 * B, 1, 3), 0.5 * rn(2 * B, 15, 3)], 1)
    truth = tf.evaluate(exp_so3(torch, aa), rn(2 * B, 10))
    shift = torch.tensor([0.05, -0.03, 0.6], device=dev) + 0.1 * rn(2 * B, 1, 3)
    y = (truth[5] + shift).float()
    yj = (torch.cat([truth[2], truth[5][:, [744, 320, 443, 554, 671]]], 1) + shift).float()          # the 21 joints of the same hands
    order = torch.rand(2 * B, NV, device=dev, generator=g).argsort(1)
    weights = {"full": torch.ones(2 * B, NV, device=dev), "sparse": torch.zeros(2 * B, NV, device=dev).scatter_(1, order[:, :a.keep], 1.0)}
    yr, yl = y[:B].contiguous(), y[B:].contiguous()
    cfg = hands_amd.FitConfig(iters=a.iters)

    def bound(w, iters):
        """the vertex fit's launch alone through the C ABI"""
        outs = [(torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
                 torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 21, 3, device=dev)) for _ in range(2)]
        ws = (w[:B].contiguous(), w[B:].contiguous())
        sides = (_lib.ManoFitVertsSide * 2)()
        for i, yy in enumerate((yr, yl)):
            sides[i] = _lib.ManoFitVertsSide(_lib.ManoFitVertsConsts(*[_lib.ptr(packs[i][k]) for k in KEYS]), _lib.ptr(yy), _lib.ptr(ws[i]),
                                             None, None, None, None, *[_lib.ptr(o) for o in outs[i]])
        c = hands_amd.FitConfig(iters=iters).c_struct()
        keep = (outs, ws, sides, c)
        return lambda: (_lib.check(L.hands_mano_fit_verts_f32(sides, 2, C.byref(c), B, st.cuda_stream), "hands_mano_fit_verts_f32"), keep)[0]

    if a.only == "kernel":
        fn = bound(weights["full"], a.iters)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        print(json.dumps({"tool": "bench_fit_verts", "only": "kernel", "hands": B, "iters": a.iters, "calls": 3}), flush=True)
        return

    def joints_bound(iters):
        """hands_mano_fit_f32 on the 21 joints of the same hands"""
        outs = [(torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
                 torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(2)]
        js = (yj[:B].contiguous(), yj[B:].contiguous())
        sides = (_lib.ManoFitSide * 2)()
        for i in range(2):
            sides[i] = _lib.ManoFitSide(_lib.ManoFitConsts(*[_lib.ptr(packs[i][k]) for k in JOINT_KEYS]), _lib.ptr(js[i]), None,
                                        None, None, None, None, *[_lib.ptr(o) for o in outs[i]])
        c = hands_amd.FitConfig(iters=iters).c_struct()
        keep = (outs, js, sides, c)
        return lambda: (_lib.check(L.hands_mano_fit_f32(sides, 2, C.byref(c), B, st.cuda_stream), "hands_mano_fit_f32"), keep)[0]

    # before anything is timed: the kernel's rmse is the one of its own outputs, and the two versions agree hand by hand
    checks = {}
    for name, w in weights.items():
        fr, fl = hands_amd.fit_mano_hands_verts(yr, yl, pair, weights_r=w[:B].contiguous(), weights_l=w[B:].contiguous(), config=cfg)
        ref = tf(y, w)
        got_rmse, got_steps = torch.cat([fr["rmse"], fl["rmse"]]), torch.cat([fr["steps"], fl["steps"]])
        full = torch.cat([fr["pose"], fl["pose"]]).double()
        own = tf.evaluate(full, torch.cat([fr["beta"], fl["beta"]]).double())[5] + torch.cat([fr["transl"], fl["transl"]]).double()[:, None]
        own = ((w.double() * (own - y.double()).pow(2).sum(2)).sum(1) / w.double().sum(1)).sqrt()
        if not float((own - got_rmse).abs().max()) <= 1e-6:
            raise SystemExit(f"{name}: the kernel's rmse is not the one of its outputs: {float((own - got_rmse).abs().max()):.3e} m")
        diff = (got_rmse - ref[3]).abs()
        worst, agree = float(diff.max()), float((diff <= 1e-6).float().mean())
        if not agree >= 0.99:
            raise SystemExit(f"{name}: kernel and torch ops disagree on {100 * (1 - agree):.1f} % of the hands (worst {worst:.3e} m; "
                             f"{tf.retried} factorisations repeated)")
        rm = np.sort(got_rmse.cpu().numpy())
        checks[name] = {"rmse_m_min_median_max": [float(f"{rm[0]:.3e}"), float(f"{rm[len(rm) // 2]:.3e}"), float(f"{rm[-1]:.3e}")],
                        "rows_within_1e-6_m_of_torch_ops": round(agree, 4), "worst_rmse_diff_m": float(f"{worst:.3e}"),
                        "rows_with_equal_steps": round(float((got_steps == ref[4]).float().mean()), 4),
                        "steps_min_median_max": [int(got_steps.min()), int(got_steps.median()), int(got_steps.max())]}
    retried_in_check, tf.retried = tf.retried, 0

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    wf, wsp = weights["full"], weights["sparse"]
    fns = [("hip_full", lambda: hands_amd.fit_mano_hands_verts(yr, yl, pair, config=cfg)),
           ("abi_full", bound(wf, a.iters)), ("abi_full_0", bound(wf, 0)),
           ("abi_sparse", bound(wsp, a.iters)), ("abi_sparse_0", bound(wsp, 0)),
           ("joints", joints_bound(a.iters)), ("joints_0", joints_bound(0)),
           ("ops_full", lambda: tf(y, wf))]
    calls = {}
    for name, fn in fns:
        for _ in range(2):                                 # warm-up: code objects, the allocator's blocks
            fn()
        torch.cuda.synchronize()
        per_call = window_us(fn, 2) / 2
        calls[name] = max(2, math.ceil(1e3 * a.window_ms / per_call))
    t = {name: [] for name, _ in fns}
    for _ in range(a.runs):                                # alternating
        for name, fn in fns:
            t[name].append(window_us(fn, calls[name]) / calls[name])
    us = {k: statistics.median(v) for k, v in t.items()}
    mm = lambda k: [round(min(t[k]), 1), round(max(t[k]), 1)]
    it = max(a.iters, 1)
    print(json.dumps({"tool": "bench_fit_verts", "hands": B, "sides": 2, "iters": a.iters, "runs": a.runs, "calls_per_window": calls,
                      "checks": checks, "torch_factorisations_repeated": [retried_in_check, tf.retried],
                      "hip_us": round(us["hip_full"], 1), "hip_us_min_max": mm("hip_full"),
                      "fit_launch_alone_us": round(us["abi_full"], 1), "fit_launch_alone_us_min_max": mm("abi_full"),
                      "fit_launch_0_iters_us": round(us["abi_full_0"], 1),
                      "us_per_iteration": round((us["abi_full"] - us["abi_full_0"]) / it, 1),
                      "sparse_launch_alone_us": round(us["abi_sparse"], 1), "sparse_launch_alone_us_min_max": mm("abi_sparse"),
                      "sparse_us_per_iteration": round((us["abi_sparse"] - us["abi_sparse_0"]) / it, 1),
                      "joint_fit_launch_alone_us": round(us["joints"], 1), "joint_fit_launch_alone_us_min_max": mm("joints"),
                      "joint_fit_us_per_iteration": round((us["joints"] - us["joints_0"]) / it, 1),
                      "torch_ops_us": round(us["ops_full"], 1), "torch_ops_us_min_max": mm("ops_full"),
                      "torch_ops_over_hip": round(us["ops_full"] / us["hip_full"], 2),
                      "forward_ms": a.forward_ms, "share_of_forward": round(us["hip_full"] / (1e3 * a.forward_ms), 4)}), flush=True)


if __name__ == "__main__":
    main()
