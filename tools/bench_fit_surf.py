#!/usr/bin/env python3
"""Device time of MANO fitting to surface correspondences (hands_mano_fit_surf_f32, csrc/fit_surf.hip) and of the ICP loop on it
(hands_amd.register_mano_hands) for 256 hand pairs, modelled on tools/bench_fit_verts.py:

* P = 778 rows that name the vertices (b = (1, 0, 0) on a face whose first vertex is n; a vertex no face starts with has weight
  0 in both) against hands_mano_fit_verts_f32 on the same problem in the same process;
* P = 512 and P = 2048 rows at random places of the surface;
* a full ``register_mano_hands`` at the default ``RegisterConfig`` on clouds of ``--cloud`` points;
* the same algorithms -- DESIGN.md section 7 "MANO fitting to surface correspondences and ICP registration" -- written with
  batched torch ops in fp64 on the same device (tools/bench_fit_verts.py's TorchFitVerts with the rows combined from its vertex
  quantities; the correspondences by brute force over all faces, ``--chunk`` hands at a time).

The launch alone goes through the C ABI with pre-bound structs at ``--iters`` and at 0 iterations: the difference over ``--iters``
is the time of an iteration.  Before anything is timed the kernel and the torch version are compared hand by hand on the P = 512
problem (99 % of the hands within 1e-6 m of rmse, or the tool refuses to report).  Device events around back-to-back calls, a
timed window at least ``--window-ms`` long, the versions alternating in one process, the median over ``--runs`` windows each.
Prints one JSON line."""
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

from bench_fit import exp_so3, log_so3  # noqa: E402
from bench_fit_verts import KEYS, NV, TorchFitVerts  # noqa: E402

SURF_KEYS = KEYS + ("faces_i32",)


class TorchFitSurf(TorchFitVerts):
    """TorchFitVerts with rows on faces: tri (N,P,3) vertex indices, b (N,P,3), y (N,P,3), w (N,P), A (N,P,3,3) or None."""

    def rows(self, v, tri, b):
        t = self.t
        N, P = tri.shape[:2]
        g = t.gather(v, 1, tri.reshape(N, 3 * P, 1).expand(-1, -1, v.shape[2])).view(N, P, 3, -1)
        return (b[..., None] * g).sum(2)

    def res(self, R, beta, tr, tri, b, y, sw, A):
        ev = self.evaluate(R, beta)
        e = sw[..., None] * (self.rows(ev[5], tri, b) + tr[:, None] - y)
        r = e if A is None else (A @ e[..., None])[..., 0]
        lg = log_so3(self.t, self.M[:, 1:].transpose(-1, -2) @ R[:, 1:]).reshape(-1, 45)
        c = (r * r).sum((1, 2)) + self.lb * (beta * beta).sum(1) + self.lp * (lg * lg).sum(1)
        return ev, r.reshape(r.shape[0], -1), lg, c, (e * e).sum((1, 2))

    def jac(self, R, ev, tri, b, sw, A):
        N, P = tri.shape[:2]
        ones = self.t.ones(N, NV, dtype=R.dtype, device=R.device)
        D = self.jacobian(R, ev, ones).view(N, NV, 3 * 61)
        Jr = self.rows(D, tri, b).view(N, P, 3, 61)
        Jr[..., 58:] = self.t.eye(3, dtype=R.dtype, device=R.device)
        if A is not None:
            Jr = A @ Jr
        return (sw[..., None, None] * Jr).reshape(N, 3 * P, 61)

    def fit(self, tri, b, y, w, R, beta, tr, iters, A=None):
        """LM from the state (R, beta, tr) -> R, beta, tr, rmse, steps, vertices + tr."""
        t = self.t
        sw, N = w.sqrt(), y.shape[0]
        mu = t.full((N,), self.mu0, dtype=t.float64, device=y.device)
        steps = t.zeros(N, dtype=t.int32, device=y.device)
        ev, r, lg, c, d = self.res(R, beta, tr, tri, b, y, sw, A)
        for _ in range(iters):
            Jm = self.jac(R, ev, tri, b, sw, A)
            H = Jm.transpose(1, 2) @ Jm + t.diag_embed(self.prior.expand(N, -1))
            g = (Jm.transpose(1, 2) @ r[..., None])[..., 0]
            g[:, 3:48] += self.lp * lg
            g[:, 48:58] += self.lb * beta
            L, ok = self.factor(H + t.diag_embed(mu[:, None] * t.diagonal(H, dim1=1, dim2=2)))
            dl = t.cholesky_solve(-g[..., None], L)[..., 0]
            R2, beta2, tr2 = R @ exp_so3(t, dl[:, :48].reshape(N, 16, 3)), beta + dl[:, 48:58], tr + dl[:, 58:]
            ev2, r2, lg2, c2, d2 = self.res(R2, beta2, tr2, tri, b, y, sw, A)
            acc = ok & (c2 < c)
            pick = lambda a, o: t.where(acc.view((-1,) + (1,) * (a.dim() - 1)), a, o)
            R, beta, tr, r, lg, c, d = pick(R2, R), pick(beta2, beta), pick(tr2, tr), pick(r2, r), pick(lg2, lg), pick(c2, c), pick(d2, d)
            ev = tuple(pick(a, o) for a, o in zip(ev2, ev))
            mu = t.where(acc, (mu / 3.0).clamp_min(1e-9), (5.0 * mu).clamp_max(1e6))
            steps += acc.to(t.int32)
        return R, beta, tr, (d / w.sum(1)).sqrt(), steps, ev[5] + tr[:, None]

    def kabsch_fit(self, tri, b, y, w, iters):
        t = self.t
        N = y.shape[0]
        R, beta = self.M.clone(), t.zeros(N, 10, dtype=t.float64, device=y.device)
        J, _, _, _, _, V0 = self.evaluate(R, beta)
        X = self.rows(V0, tri, b)
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
        return self.fit(tri, b, y, w, R, beta, tr, iters)

    def correspond(self, p, verts, faces, chunk):
        """Closest point of every p (N,P,3) on its hand's mesh by brute force: coefficients (N,P,3), the vertex triples (N,P,3) and
        the unit normals (N,P,3) of the closest faces; ``faces`` (N,F,3) per hand."""
        t = self.t
        outs = []
        for s in range(0, p.shape[0], chunk):
            q, T = p[s:s + chunk, :, None], t.gather(verts[s:s + chunk], 1, faces[s:s + chunk].reshape(-1, faces.shape[1] * 3, 1).expand(-1, -1, 3))
            T = T.view(T.shape[0], 1, -1, 3, 3)
            a, bb, cc = T[..., 0, :], T[..., 1, :], T[..., 2, :]

            def seg(u, v):
                e = v - u
                L = (e * e).sum(-1)
                tt = t.where(L > 0, ((q - u) * e).sum(-1) / L.clamp_min(1e-300), t.zeros_like(L)).clamp(0.0, 1.0)
                c = u + tt[..., None] * e
                return ((q - c) ** 2).sum(-1), tt
            d1, t1 = seg(a, bb)
            d2, t2 = seg(a, cc)
            d3, t3 = seg(bb, cc)
            n = t.linalg.cross(bb - a, cc - a)
            nn = (n * n).sum(-1)
            wa = (n * t.linalg.cross(bb - q, cc - q)).sum(-1)
            wb = (n * t.linalg.cross(cc - q, a - q)).sum(-1)
            wc = (n * t.linalg.cross(a - q, bb - q)).sum(-1)
            inside = (nn > 0) & (wa >= 0) & (wb >= 0) & (wc >= 0)
            sdn = ((q - a) * n).sum(-1)
            dp = t.where(inside, sdn * sdn / nn.clamp_min(1e-300), t.full_like(nn, float("inf")))
            best, f = t.stack([d1, d2, d3, dp], -1).min(-1)[0].min(-1)
            pickf = lambda x: t.gather(x.expand(f.shape[0], f.shape[1], -1), 2, f[..., None]).squeeze(-1)
            z = t.zeros_like(pickf(t1))
            cand = t.stack([t.stack([1 - pickf(t1), pickf(t1), z], -1), t.stack([1 - pickf(t2), z, pickf(t2)], -1),
                            t.stack([z, 1 - pickf(t3), pickf(t3)], -1),
                            t.stack([pickf(wa), pickf(wb), pickf(wc)], -1) / pickf(nn).clamp_min(1e-300)[..., None]], -2)
            which = t.stack([pickf(d1), pickf(d2), pickf(d3), pickf(dp)], -1).argmin(-1)
            coef = t.gather(cand, 2, which[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
            nf = t.gather(n.expand(q.shape[0], q.shape[1], -1, 3), 2, f[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
            nf = nf / nf.norm(dim=-1, keepdim=True).clamp_min(1e-300)
            tri = t.gather(faces[s:s + chunk], 1, f[..., None].expand(-1, -1, 3))
            outs.append((coef, tri, nf, best.sqrt()))
        return tuple(t.cat(x) for x in zip(*outs))

    def register(self, p, faces, R, beta, tr, rounds, iters, tau, chunk):
        t = self.t
        eye = t.eye(3, dtype=t.float64, device=p.device)
        w = t.ones(p.shape[:2], dtype=t.float64, device=p.device)
        verts = self.evaluate(R, beta)[5] + tr[:, None]
        for _ in range(rounds):
            coef, tri, nf, dist = self.correspond(p, verts, faces, chunk)
            nnT = nf[..., :, None] * nf[..., None, :]
            A = nnT + math.sqrt(tau) * (eye - nnT)
            R, beta, tr, rmse, _, verts = self.fit(tri, coef, p, w, R, beta, tr, iters, A)
        return R, beta, tr, rmse, dist


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hands", type=int, default=256, help="hand pairs (B)")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0, help="least length of a timed window")
    ap.add_argument("--cloud", type=int, default=512, help="points of a registration cloud")
    ap.add_argument("--chunk", type=int, default=16, help="hands per brute-force step of the torch correspondences")
    ap.add_argument("--no-torch-register", action="store_true", help="leave the torch version of the ICP loop out")
    a = ap.parse_args()
    import torch
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit_surf.py needs a HIP device: a CPU run cannot give a time")
    st = torch.cuda.current_stream()
    dev = torch.device("cuda", torch.cuda.current_device())
    L, B = _lib.lib(), a.hands
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], dev)
    pair = type("Pair", (), {"packed": lambda self, d: {"mano_r": packs[0], "mano_l": packs[1]}})()
    tf = TorchFitSurf(torch, packs, B, a.iters)
    faces = torch.cat([p["faces_i32"].long().view(1, -1, 3).expand(B, -1, -1) for p in packs]).contiguous()      # (2B, 1538, 3)

    g = torch.Generator(device="cuda").manual_seed(3)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g, dtype=torch.float64)
    aa = tf.pm + torch.cat([2.0 * rn(2 * B, 1, 3), 0.5 * rn(2 * B, 15, 3)], 1)
    Rt, bt = exp_so3(torch, aa), rn(2 * B, 10)
    vt = tf.evaluate(Rt, bt)[5]
    shift = torch.tensor([0.05, -0.03, 0.6], device=dev) + 0.1 * rn(2 * B, 1, 3)

    def problem(P, vertex_rows=False):
        """rows on the truth's surface: face (2B,P) int32, b (2B,P,3) fp32, y (2B,P,3) fp32, w (2B,P) fp32"""
        if vertex_rows:
            f = torch.zeros(2 * B, NV, dtype=torch.long, device=dev)
            w = torch.zeros(2 * B, NV, device=dev)
            for i in range(2):
                first = packs[i]["faces_i32"][:, 0].long()
                idx = torch.arange(first.numel(), device=dev)
                f[i * B:(i + 1) * B].scatter_(1, first.view(1, -1).expand(B, -1), idx.view(1, -1).expand(B, -1))
                w[i * B:(i + 1) * B, first] = 1.0
            b = torch.tensor([1.0, 0.0, 0.0], device=dev).expand(2 * B, NV, 3).contiguous()
        else:
            f = torch.randint(0, 1538, (2 * B, P), device=dev, generator=g)
            e = -torch.rand(2 * B, P, 3, device=dev, generator=g).clamp_min(1e-9).log()
            b, w = (e / e.sum(-1, keepdim=True)).contiguous(), torch.ones(2 * B, P, device=dev)
        tri = torch.gather(faces, 1, f[..., None].expand(-1, -1, 3))
        y = (tf.rows(vt, tri, b.double()) + shift).float()
        return dict(f=f.int().contiguous(), b=b, y=y, w=w, tri=tri)

    def bound(pr, iters):
        """the surface fit's launch alone through the C ABI"""
        P = pr["y"].shape[1]
        outs = [(torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
                 torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 21, 3, device=dev),
                 torch.empty(B, NV, 3, device=dev)) for _ in range(2)]
        ins = [tuple(pr[k][i * B:(i + 1) * B].contiguous() for k in ("y", "w", "f", "b")) for i in range(2)]
        sides = (_lib.ManoFitSurfSide * 2)()
        for i in range(2):
            yy, ww, ff, bb = ins[i]
            sides[i] = _lib.ManoFitSurfSide(_lib.ManoFitSurfConsts(*[_lib.ptr(packs[i][k]) for k in SURF_KEYS]), _lib.ptr(yy), _lib.ptr(ww),
                                            None, None, None, None, *[_lib.ptr(o) for o in outs[i]], _lib.ptr(ff), _lib.ptr(bb), None)
        c = hands_amd.SurfaceFitConfig(iters=iters).c_struct()
        keep = (outs, ins, sides, c)
        fn = lambda: (_lib.check(L.hands_mano_fit_surf_f32(sides, 2, C.byref(c), B, P, st.cuda_stream), "hands_mano_fit_surf_f32"), keep)[0]
        fn.outs = outs
        return fn

    def verts_bound(pr, iters):
        """hands_mano_fit_verts_f32 on the same vertices"""
        outs = [(torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
                 torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 21, 3, device=dev)) for _ in range(2)]
        y = (vt + shift).float()
        ins = [(y[i * B:(i + 1) * B].contiguous(), pr["w"][i * B:(i + 1) * B].contiguous()) for i in range(2)]
        sides = (_lib.ManoFitVertsSide * 2)()
        for i in range(2):
            sides[i] = _lib.ManoFitVertsSide(_lib.ManoFitVertsConsts(*[_lib.ptr(packs[i][k]) for k in KEYS]), _lib.ptr(ins[i][0]),
                                             _lib.ptr(ins[i][1]), None, None, None, None, *[_lib.ptr(o) for o in outs[i]])
        c = hands_amd.FitConfig(iters=iters).c_struct()
        keep = (outs, ins, sides, c)
        fn = lambda: (_lib.check(L.hands_mano_fit_verts_f32(sides, 2, C.byref(c), B, st.cuda_stream), "hands_mano_fit_verts_f32"), keep)[0]
        fn.outs = outs
        return fn

    pv, p512, p2048 = problem(NV, True), problem(512), problem(2048)
    # before anything is timed: the two versions agree hand by hand on the P = 512 problem, and the vertex rows give the vertex fit
    k512 = bound(p512, a.iters)
    k512()
    ref = tf.kabsch_fit(p512["tri"], p512["b"].double(), p512["y"].double(), p512["w"].double(), a.iters)
    got = torch.cat([k512.outs[0][3], k512.outs[1][3]]).double()
    diff = (got - ref[3]).abs()
    agree = float((diff <= 1e-6).float().mean())
    if not agree >= 0.99:
        raise SystemExit(f"kernel and torch ops disagree on {100 * (1 - agree):.1f} % of the hands (worst {float(diff.max()):.3e} m)")
    kv, vv = bound(pv, a.iters), verts_bound(pv, a.iters)
    kv(), vv()
    same = float((torch.cat([kv.outs[0][3], kv.outs[1][3]]) - torch.cat([vv.outs[0][3], vv.outs[1][3]])).abs().max())
    checks = {"rows_within_1e-6_m_of_torch_ops": round(agree, 4), "worst_rmse_diff_m": float(f"{float(diff.max()):.3e}"),
              "vertex_rows_rmse_diff_to_vertex_fit_m": float(f"{same:.3e}"),
              "vertex_rows_weighted": int(pv["w"][0].sum()), "rmse_m_median": float(f"{float(got.median()):.3e}")}

    # registration: clouds on the truth's surface, the start 0.05 rad per joint, 0.1 in beta and 5 mm off
    pc = problem(a.cloud)
    unit = lambda *s: torch.nn.functional.normalize(rn(*s), dim=-1)
    R0 = (Rt @ exp_so3(torch, 0.05 * unit(2 * B, 16, 3))).float()
    b0, t0 = (bt + 0.1 * rn(2 * B, 10)).float(), (shift[:, 0] + 0.005 * unit(2 * B, 3)).float()
    init = [tuple(x[i * B:(i + 1) * B].contiguous() for x in (R0, b0, t0)) for i in range(2)]
    cl = [pc["y"][i * B:(i + 1) * B].contiguous() for i in range(2)]
    rc = hands_amd.RegisterConfig()
    reg = lambda: hands_amd.register_mano_hands(cl[0], cl[1], pair, init[0], init[1], config=rc)
    out = reg()
    dist_end = torch.cat([hands_amd.correspond_on_mesh(cl[i], out[i]["verts"], packs[i]["faces_i32"])["dist"] for i in range(2)])
    dist_start = torch.cat([hands_amd.correspond_on_mesh(cl[i], hands_amd.fit_mano_surface(
        cl[i], pc["f"][i * B:(i + 1) * B], pc["b"][i * B:(i + 1) * B], pair, "rl"[i], init=init[i],
        config=hands_amd.SurfaceFitConfig(iters=0))["verts"], packs[i]["faces_i32"])["dist"] for i in range(2)])
    rms = lambda d: d.double().pow(2).mean(1).sqrt()
    checks["register_rms_mm_start_median"] = round(1e3 * float(rms(dist_start).median()), 4)
    checks["register_rms_mm_end_median"] = round(1e3 * float(rms(dist_end).median()), 4)
    checks["register_rounds_done_min"] = int(torch.cat([o["rounds_done"] for o in out]).min())
    reg_ops = lambda: tf.register(pc["y"].double(), faces, R0.double(), b0.double(), t0.double(), rc.rounds, rc.iters, rc.tangent_weight, a.chunk)
    if not a.no_torch_register:
        ro = reg_ops()
        checks["register_torch_rms_mm_last_round_median"] = round(1e3 * float(rms(ro[4]).median()), 4)

    def window_us(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(calls):
            fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    fns = [("surf_778", kv), ("surf_778_0", bound(pv, 0)), ("verts_778", vv), ("verts_778_0", verts_bound(pv, 0)),
           ("surf_512", k512), ("surf_512_0", bound(p512, 0)), ("surf_2048", bound(p2048, a.iters)), ("surf_2048_0", bound(p2048, 0)),
           ("register", reg),
           ("ops_512", lambda: tf.kabsch_fit(p512["tri"], p512["b"].double(), p512["y"].double(), p512["w"].double(), a.iters))]
    if not a.no_torch_register:
        fns.append(("ops_register", reg_ops))
    calls = {}
    for name, fn in fns:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        calls[name] = max(2, math.ceil(1e3 * a.window_ms / (window_us(fn, 2) / 2)))
    t = {name: [] for name, _ in fns}
    for _ in range(a.runs):
        for name, fn in fns:
            t[name].append(window_us(fn, calls[name]) / calls[name])
    us = {k: statistics.median(v) for k, v in t.items()}
    mm = lambda k: [round(min(t[k]), 1), round(max(t[k]), 1)]
    it = max(a.iters, 1)
    per = lambda k: round((us[k] - us[k + "_0"]) / it, 1)
    res = {"tool": "bench_fit_surf", "hands": B, "sides": 2, "iters": a.iters, "runs": a.runs, "calls_per_window": calls, "checks": checks,
           "surf_778_us": round(us["surf_778"], 1), "surf_778_us_min_max": mm("surf_778"), "surf_778_us_per_iteration": per("surf_778"),
           "verts_778_us": round(us["verts_778"], 1), "verts_778_us_min_max": mm("verts_778"), "verts_778_us_per_iteration": per("verts_778"),
           "surf_over_verts_per_iteration": round(per("surf_778") / per("verts_778"), 2),
           "surf_512_us": round(us["surf_512"], 1), "surf_512_us_per_iteration": per("surf_512"),
           "surf_2048_us": round(us["surf_2048"], 1), "surf_2048_us_per_iteration": per("surf_2048"),
           "register_us": round(us["register"], 1), "register_us_min_max": mm("register"), "register_cloud": a.cloud,
           "register_rounds_iters": [rc.rounds, rc.iters],
           "torch_ops_512_us": round(us["ops_512"], 1), "torch_ops_512_over_hip": round(us["ops_512"] / us["surf_512"], 2)}
    if not a.no_torch_register:
        res.update(torch_ops_register_us=round(us["ops_register"], 1), torch_ops_register_over_hip=round(us["ops_register"] / us["register"], 2))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
