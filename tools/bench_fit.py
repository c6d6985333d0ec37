#!/usr/bin/env python3
"""Device time of MANO fitting (hands_mano_fit_f32, csrc/fit.hip) for 256 hand pairs at 30 iterations, against the same algorithm
-- DESIGN.md section 7 "MANO fitting": analytic Jacobian, H = J^T J, (H + mu diag H) d = -g by Cholesky, accept / reject per hand
-- written with batched torch ops in fp64 on the same device (``torch.linalg.cholesky_ex`` / ``torch.cholesky_solve``, a Python
loop over the iterations and over the 16 joints of the chain).

Times ``hands_amd.fit_mano_hands`` (the Python function with its allocations: one fit launch, two axis-angle launches) and the
fit launch alone through the C ABI with pre-bound structs.  Before either is timed, the kernel's rmse is checked against its own
outputs (recomputed with the torch forward) and the two versions are compared hand by hand: 99 % of the hands have to agree
within 1e-6 m.  Device events around ``calls`` back-to-back calls, a timed window at least ``--window-ms`` long; the versions
alternate in one process, the median over ``--runs`` windows each.  ``--forward-ms`` is the time of a HandsLight forward
at bz = 256 the share is taken of (docs/EXPERIMENTS.md records it; this tool does not run the trunks).  The targets are joints
the synthetic assets generate themselves (the family of DESIGN.md section 7).  No profiler.  Prints one JSON line."""
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

PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
KEYS = ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs", "tip_lbs_weights", "tip_posedirs")


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


class TorchFit:
    """The fit over N hands at once (all weights 1, every row fitted, the half-turn branch of Log left out).  Constants carry a
    leading hand dimension, so both sides go through one batch."""

    def __init__(self, torch, packs, B, iters=30, lb=1e-6, lp=1e-6, mu0=1e-3, factorisation="cholesky_ex"):
        self.t, self.iters, self.lb, self.lp, self.mu0 = torch, iters, lb, lp, mu0
        self.factorisation, self.retried = factorisation, 0
        rep = lambda k, *s: torch.cat([p[k].double().view(1, *s).expand(B, *s) for p in packs]).contiguous()
        self.pm, self.Jt, self.Js = rep("pose_mean", 16, 3), rep("J_template", 16, 3), rep("J_shapedirs", 16, 3, 10)
        self.tv, self.tsd, self.W = rep("tip_v_template", 5, 3), rep("tip_shapedirs", 5, 3, 10), rep("tip_lbs_weights", 5, 16)
        self.pd = rep("tip_posedirs", 15, 9, 5, 3)
        self.M = exp_so3(torch, self.pm)
        dev = self.M.device
        below = [[j == 0 or (i >= j and (i - 1) // 3 == (j - 1) // 3) for i in range(16)] for j in range(16)]
        self.below = torch.tensor(below, dtype=torch.float64, device=dev)                  # [j, i]: i at or below j
        self.strict = self.below * (1.0 - torch.eye(16, dtype=torch.float64, device=dev))
        self.E = hat(torch, torch.eye(3, dtype=torch.float64, device=dev))                 # [e_a]x
        prior = torch.zeros(61, dtype=torch.float64, device=dev)
        prior[3:48], prior[48:58] = lp, lb
        self.prior = prior

    def factor(self, Ad):
        """The lower Cholesky factor per hand and whether it exists.  ``cholesky_ex``: the batched factorisation; on an MI355X
        with torch 2.10 / ROCm 7.0 it now and then reports failure for (nearly) the whole batch on matrices that factorise --
        the host, the kernel and a second call agree on that -- so a call with failures is repeated, up to twice, which costs a
        host synchronisation.  ``loop``: 61 column steps written with torch ops."""
        t = self.t
        if self.factorisation == "loop":
            L, ok = Ad.clone(), t.ones(Ad.shape[0], dtype=t.bool, device=Ad.device)
            for k in range(61):
                piv = L[:, k, k]
                ok &= piv > 0
                L[:, k:, k] /= t.where(piv > 0, piv, t.ones_like(piv)).sqrt()[:, None]
                L[:, k + 1:, k + 1:] -= L[:, k + 1:, k, None] * L[:, None, k + 1:, k]
            return L.tril(), ok
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
        vp = self.tv + t.einsum("nmcl,nl->nmc", self.tsd, beta) + t.einsum("njf,njfmc->nmc", pf, self.pd)
        x = t.einsum("niab,nmib->nmia", Q, vp[:, :, None] - J[:, None]) + p[:, None]
        A = t.einsum("nmi,niab->nmab", self.W, Q)
        joints = t.cat([p, t.einsum("nmi,nmic->nmc", self.W, x)], 1)
        return J, Q, p, x, A, joints

    def residual(self, R, beta, tr, y):
        ev = self.evaluate(R, beta)
        r = (ev[5] + tr[:, None] - y).reshape(-1, 63)
        lg = log_so3(self.t, self.M[:, 1:].transpose(-1, -2) @ R[:, 1:]).reshape(-1, 45)
        c = (r * r).sum(1) + self.lb * (beta * beta).sum(1) + self.lp * (lg * lg).sum(1)
        return ev, r, lg, c

    def jacobian(self, R, ev):
        t = self.t
        _, Q, p, x, A, _ = ev
        N = R.shape[0]
        D = t.zeros(N, 21, 3, 61, dtype=R.dtype, device=R.device)
        v = (p[:, None] - p[:, :, None]) * self.strict[None, :, :, None]                   # [n, j, k]
        kin = -hat(t, v) @ Q[:, :, None]                                                   # [n, j, k, 3, 3]
        D[:, :16, :, :48] = kin.permute(0, 2, 3, 1, 4).reshape(N, 16, 3, 48)
        s = t.einsum("ji,nmi,nmic->njmc", self.below, self.W, x) - t.einsum("ji,nmi->njm", self.below, self.W)[..., None] * p[:, :, None]
        tip = -hat(t, s) @ Q[:, :, None]                                                   # [n, j, m, 3, 3]
        dR = (R[:, 1:, None] @ self.E).reshape(N, 15, 3, 9)                                # [n, j - 1, a, f]
        u = t.einsum("njaf,njfmc->njmca", dR, self.pd)
        tip[:, 1:] += t.einsum("nmrc,njmca->njmra", A, u)
        D[:, 16:, :, :48] = tip.permute(0, 2, 3, 1, 4).reshape(N, 5, 3, 48)
        dp = [self.Js[:, 0]]
        for i in range(1, 16):
            a = PARENTS[i]
            dp.append(dp[a] + Q[:, a] @ (self.Js[:, i] - self.Js[:, a]))
        dp = t.stack(dp, 1)
        D[:, :16, :, 48:58] = dp
        D[:, 16:, :, 48:58] = t.einsum("nmi,nmicl->nmcl", self.W, t.einsum("nicb,nmibl->nmicl", Q, self.tsd[:, :, None] - self.Js[:, None]) + dp[:, None])
        D[:, :, :, 58:] = t.eye(3, dtype=R.dtype, device=R.device)
        return D.reshape(N, 63, 61)

    def __call__(self, y):
        t = self.t
        y = y.double()
        N = y.shape[0]
        R, beta = self.M.clone(), t.zeros(N, 10, dtype=t.float64, device=y.device)
        X = self.evaluate(R, beta)[5]
        mx, my = X.mean(1), y.mean(1)
        K = (X - mx[:, None]).transpose(1, 2) @ (y - my[:, None])
        U, _, Vh = t.linalg.svd(K)
        V = Vh.transpose(1, 2)
        d = t.ones(N, 3, dtype=t.float64, device=y.device)
        d[:, 2] = t.linalg.det(V @ U.transpose(1, 2))
        R0 = (V * d[:, None]) @ U.transpose(1, 2)
        R[:, 0] = R0
        tr = my - (R0 @ (mx - X[:, 0])[..., None])[..., 0] - X[:, 0]
        mu = t.full((N,), self.mu0, dtype=t.float64, device=y.device)
        steps = t.zeros(N, dtype=t.int32, device=y.device)
        ev, r, lg, c = self.residual(R, beta, tr, y)
        for _ in range(self.iters):
            Jm = self.jacobian(R, ev)
            H = Jm.transpose(1, 2) @ Jm + t.diag_embed(self.prior.expand(N, -1))
            g = (Jm.transpose(1, 2) @ r[..., None])[..., 0]
            g[:, 3:48] += self.lp * lg
            g[:, 48:58] += self.lb * beta
            Ad = H + t.diag_embed(mu[:, None] * t.diagonal(H, dim1=1, dim2=2))
            L, ok = self.factor(Ad)
            dl = t.cholesky_solve(-g[..., None], L)[..., 0]
            R2 = R @ exp_so3(t, dl[:, :48].reshape(N, 16, 3))
            beta2, tr2 = beta + dl[:, 48:58], tr + dl[:, 58:]
            ev2, r2, lg2, c2 = self.residual(R2, beta2, tr2, y)
            acc = ok & (c2 < c)
            pick = lambda a, b: t.where(acc.view((-1,) + (1,) * (a.dim() - 1)), a, b)
            R, beta, tr, r, lg, c = pick(R2, R), pick(beta2, beta), pick(tr2, tr), pick(r2, r), pick(lg2, lg), pick(c2, c)
            ev = tuple(pick(a, b) for a, b in zip(ev2, ev))
            mu = t.where(acc, (mu / 3.0).clamp_min(1e-9), (5.0 * mu).clamp_max(1e6))
            steps += acc.to(t.int32)
        return R.float(), beta.float(), tr.float(), (r * r).sum(1).div(21.0).sqrt().float(), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=256, help="hand pairs (B)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    ap.add_argument("--factorisation", default="cholesky_ex", choices=("cholesky_ex", "loop"), help="of the torch version")
    ap.add_argument("--dump", default="", help="write targets and both versions' rmse / steps to this .npz")
    ap.add_argument("--forward-ms", type=float, default=45.10, help="HandsLight forward at bz = 256 (docs/EXPERIMENTS.md)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    L, B = _lib.lib(), a.hands
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], dev)
    pair = type("Pair", (), {"packed": lambda self, d: {"mano_r": packs[0], "mano_l": packs[1]}})()
    tf = TorchFit(torch, packs, B, a.iters, factorisation=a.factorisation)

    # targets the model generates itself: global rotation 2 randn, fingers hands_mean + 0.5 randn, beta = randn, rounded to fp32
    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.float64)
    aa = tf.pm + torch.cat([2.0 * rn(2 * B, 1, 3), 0.5 * rn(2 * B, 15, 3)], 1)
    y = (tf.evaluate(exp_so3(torch, aa), rn(2 * B, 10))[5] + torch.tensor([0.05, -0.03, 0.6], device=dev) + 0.1 * rn(2 * B, 1, 3)).float()
    yr, yl = y[:B].contiguous(), y[B:].contiguous()
    cfg = hands_amd.FitConfig(iters=a.iters)

    hip = lambda: hands_amd.fit_mano_hands(yr, yl, pair, config=cfg)
    ops = lambda: tf(y)
    outs = [(torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
             torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev)) for _ in range(2)]
    sides = (_lib.ManoFitSide * 2)()
    for i, yy in enumerate((yr, yl)):
        sides[i] = _lib.ManoFitSide(_lib.ManoFitConsts(*[_lib.ptr(packs[i][k]) for k in KEYS]), _lib.ptr(yy), None, None, None, None,
                                    None, *[_lib.ptr(o) for o in outs[i]])
    ccfg = cfg.c_struct()
    abi = lambda: _lib.check(L.hands_mano_fit_f32(sides, 2, C.byref(ccfg), B, st.cuda_stream), "hands_mano_fit_f32")

    # before either is timed: the kernel's rmse is the one of its own outputs (recomputed with the torch forward), and the two
    # versions agree hand by hand -- on the host, the torch version reproduces the kernel's rmse of all 512 hands of these
    # targets within 1.5e-8 m, the hands that have not converged after 30 iterations included
    fr, fl = hip()
    ref = ops()
    got_rmse, got_steps = torch.cat([fr["rmse"], fl["rmse"]]), torch.cat([fr["steps"], fl["steps"]])
    full = torch.cat([fr["pose"], fl["pose"]]).double()
    own = tf.evaluate(full, torch.cat([fr["beta"], fl["beta"]]).double())[5] + torch.cat([fr["transl"], fl["transl"]]).double()[:, None]
    own = (own - y.double()).pow(2).sum(2).mean(1).sqrt()
    if not float((own - got_rmse).abs().max()) <= 1e-6:
        raise SystemExit(f"the kernel's rmse is not the one of its outputs: {float((own - got_rmse).abs().max()):.3e} m")
    diff = (got_rmse - ref[3]).abs()
    worst, agree = float(diff.max()), float((diff <= 1e-6).float().mean())
    same_steps = float((got_steps == ref[4]).float().mean())
    if a.dump:
        np.savez(a.dump, y=y.cpu().numpy(), hip_rmse=got_rmse.cpu().numpy(), ops_rmse=ref[3].cpu().numpy(),
                 hip_steps=got_steps.cpu().numpy(), ops_steps=ref[4].cpu().numpy())
    if not agree >= 0.99:
        raise SystemExit(f"kernel and torch ops disagree on {100 * (1 - agree):.1f} % of the hands (worst {worst:.3e} m; "
                         f"{tf.retried} factorisations repeated)")
    retried_in_check, tf.retried = tf.retried, 0

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    fns = (("hip", hip), ("ops", ops), ("abi", abi))
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
    rm = np.sort(got_rmse.cpu().numpy())
    print(json.dumps({"tool": "bench_fit", "hands": B, "sides": 2, "iters": a.iters, "runs": a.runs, "calls_per_window": calls,
                      "rmse_m_min_median_max": [float(f"{rm[0]:.3e}"), float(f"{rm[len(rm) // 2]:.3e}"), float(f"{rm[-1]:.3e}")],
                      "rows_within_1e-6_m_of_torch_ops": round(agree, 4), "worst_rmse_diff_m": float(f"{worst:.3e}"),
                      "rows_with_equal_steps": round(same_steps, 4), "torch_factorisation": a.factorisation,
                      "torch_factorisations_repeated": [retried_in_check, tf.retried],
                      "hip_us": round(us["hip"], 1), "hip_us_min_max": mm("hip"),
                      "fit_launch_alone_us": round(us["abi"], 1), "fit_launch_alone_us_min_max": mm("abi"),
                      "torch_ops_us": round(us["ops"], 1), "torch_ops_us_min_max": mm("ops"),
                      "torch_ops_over_hip": round(us["ops"] / us["hip"], 2),
                      "forward_ms": a.forward_ms, "share_of_forward": round(us["hip"] / (1e3 * a.forward_ms), 4),
                      "torch_ops_share_of_forward": round(us["ops"] / (1e3 * a.forward_ms), 3)}), flush=True)


if __name__ == "__main__":
    main()
