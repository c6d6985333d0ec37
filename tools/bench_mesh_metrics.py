#!/usr/bin/env python3
"""Device time of the mesh metrics (hands_eval_mesh_metrics_f32, csrc/mesh_metrics.hip: one launch) at V = 778.

Per batch size (default 256): the median over `--runs` event-timed runs of `--calls` back-to-back launches through the C ABI
with pre-bound structs; the distance evaluations the definition needs (4 V^2 per hand: two directions, two alignments) and the
rate they are done at; the same thirty quantities computed with torch ops on the same device (`torch.cdist` over 16 samples at a
time, batched `torch.linalg.svd` -- what a user would write instead of the host loop), wall clock ending in a synchronise; both
checked against each other before timing (a disagreement prints the fp64 restatement's value of the worst sample beside
them); and the share of a HandsLight forward at that batch size.  No profiler.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")


def make_case(torch, B, V, seed):
    """Ground truth: a hand-sized cloud; prediction: rotated, scaled x 1.1, 2-8 mm of noise (what the parity tests use)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    pred, targets = {}, {}
    for h in "rl":
        gv = 0.08 * r(B, V, 3) + torch.tensor([0.05, -0.03, 0.5], device="cuda")
        gj = torch.cat([gv[:, :16], 0.5 * gv[:, 16:21] + torch.tensor([0.025, -0.015, 0.25], device="cuda")], 1)
        ang = 0.15 + 0.4 * torch.rand(B, device="cuda", generator=g)
        R = torch.zeros(B, 3, 3, device="cuda")
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = ang.cos(), -ang.sin(), ang.sin(), ang.cos(), 1.0
        c = gv.mean(1, keepdim=True)
        sig = (0.002 * 2 ** torch.randint(0, 3, (B, 1, 1), device="cuda", generator=g)).float()
        f = lambda x: 1.1 * (x - c) @ R.transpose(1, 2) + c + sig * r(*x.shape)
        targets[f"mano.v3d.cam.{h}"], targets[f"mano.j3d.cam.{h}"] = gv.contiguous(), gj.contiguous()
        pred[f"mano.v3d.cam.{h}"], pred[f"mano.j3d.cam.{h}"] = f(gv).contiguous(), f(gj).contiguous()
    targets.update(is_valid=torch.ones(B, device="cuda"), right_valid=torch.ones(B, device="cuda"),
                   left_valid=(torch.rand(B, device="cuda", generator=g) > 0.1).float())
    return pred, targets


def torch_mesh_metrics(torch, pred, targets):
    """The same quantities with torch ops on the device, fp32 (fp64 for the 3x3 SVD), all hands batched."""
    th = torch.arange(100, device="cuda", dtype=torch.float32) * (0.05 / 99.0)

    def fit(p, g):
        mu1, mu2 = p.mean(1, keepdim=True), g.mean(1, keepdim=True)
        x1, x2 = (p - mu1).double(), (g - mu2).double()
        K = x1.transpose(1, 2) @ x2
        U, _, Vh = torch.linalg.svd(K)
        Z = torch.eye(3, device="cuda", dtype=torch.float64).repeat(len(p), 1, 1)
        Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ Vh))
        R = Vh.transpose(1, 2) @ Z @ U.transpose(1, 2)
        scale = (R @ K).diagonal(dim1=1, dim2=2).sum(1) / (x1 ** 2).sum((1, 2))
        return ((scale[:, None, None] * (x1 @ R.transpose(1, 2))) + mu2.double()).float()

    def auc(e):
        pck = (e[:, None, :] <= th[None, :, None]).float().mean(2)
        return ((pck[:, 1:] + pck[:, :-1]) * 0.5).sum(1) / 99.0

    out = {}
    for h, hv in (("r", "right_valid"), ("l", "left_valid")):
        valid = targets[hv] * targets["is_valid"] != 0
        pj, gj = pred[f"mano.j3d.cam.{h}"], targets[f"mano.j3d.cam.{h}"]
        pv, gv = pred[f"mano.v3d.cam.{h}"] - pj[:, :1], targets[f"mano.v3d.cam.{h}"] - gj[:, :1]
        pj, gj = pj - pj[:, :1], gj - gj[:, :1]
        for a in ("ra", "pa"):
            qv, qj = (pv, pj) if a == "ra" else (fit(pv, gv), fit(pj, gj))
            # 16 samples per call: one cdist launch takes a thread block per distance, and 256 x 778^2 of them are more than a
            # launch can hold
            D = torch.cat([torch.cdist(gv[i:i + 16], qv[i:i + 16], compute_mode="donot_use_mm_for_euclid_dist")
                           for i in range(0, len(gv), 16)])
            d1, d2 = D.min(2).values, D.min(1).values
            ev, ej = (gv - qv).norm(dim=2), (gj - qj).norm(dim=2)
            vals = {f"mpvpe/{a}": ev.mean(1) * 1000.0, f"auc/{a}/v": auc(ev), f"auc/{a}/j": auc(ej)}
            for t, name in ((0.005, "5"), (0.015, "15")):
                P, R = (d1 < t).float().mean(1), (d2 < t).float().mean(1)
                vals[f"fscore/{a}/{name}"] = torch.where(P + R > 0, 2 * P * R / (P + R).clamp_min(1e-30), torch.zeros_like(P))
            for k, v in vals.items():
                out[f"{k}/{h}"] = torch.where(valid, v, torch.full_like(v, float("nan")))
    for k in [k[:-2] for k in out if k.endswith("/r")]:
        out[k + "/h"] = torch.stack([out[k + "/r"], out[k + "/l"]], 1).nanmean(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256])
    ap.add_argument("--verts", type=int, default=778)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward the share is taken of")
    a = ap.parse_args()
    assert a.runs >= 20
    import torch
    import hands_amd
    from hands_amd import _lib
    from hands_amd.metrics import MESH_KEYS, evaluate_mesh_metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_metrics.py needs a HIP device: a CPU run cannot give a time")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    V = a.verts

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    out = {"tool": "bench_mesh_metrics", "verts": V, "runs": a.runs, "calls_per_run": a.calls, "batches": {}}
    for B in a.batches:
        pred, targets = make_case(torch, B, V, seed=7)
        keep = [pred["mano.v3d.cam.r"], pred["mano.v3d.cam.l"], targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"],
                pred["mano.j3d.cam.r"], pred["mano.j3d.cam.l"], targets["mano.j3d.cam.r"], targets["mano.j3d.cam.l"],
                targets["is_valid"], targets["right_valid"], targets["left_valid"]]
        buf = torch.empty(3 * len(MESH_KEYS), B, device=dev)
        fin = _lib.MeshEvalIn(*[_lib.ptr(t) for t in keep])
        fout = _lib.MeshEvalOut(*[_lib.ptr(buf[i]) for i in range(buf.shape[0])])

        def hip_calls():
            for _ in range(a.calls):
                _lib.check(L.hands_eval_mesh_metrics_f32(C.byref(fin), C.byref(fout), B, V, st.cuda_stream), "mesh metrics")
        # the two agree before either is timed: continuous keys to 1e-3 mm, counted keys to a few points of V
        got, ref = evaluate_mesh_metrics(pred, targets), torch_mesh_metrics(torch, pred, targets)
        worst, where = {}, {}
        for k in got:
            assert torch.equal(got[k].isnan(), ref[k].isnan()), k
            d = (got[k] - ref[k]).abs().nan_to_num()
            if float(d.max()) >= worst.get(k.split("/")[0], -1.0):
                worst[k.split("/")[0]], where[k.split("/")[0]] = float(d.max()), (k, int(d.argmax()))
        if not (worst["mpvpe"] < 1e-3 and worst["fscore"] < 8.0 / V and worst["auc"] < 8.0 / (99 * min(V, 21))):
            import mesh_metrics_ref
            for k, i in where.values():                   # the fp64 restatement's opinion on the worst sample of each kind
                one = mesh_metrics_ref.evaluate_mesh({n: t[i:i + 1].cpu().numpy() for n, t in pred.items()},
                                                     {n: t[i:i + 1].cpu().numpy() for n, t in targets.items()})
                print(f"{k}[{i}]: kernel {float(got[k][i])!r} torch ops {float(ref[k][i])!r} fp64 restatement {float(one[k][0])!r}",
                      file=sys.stderr)
            raise SystemExit(f"kernel and torch ops disagree: {worst}")
        for _ in range(a.warmup):
            hip_calls()
        torch.cuda.synchronize()
        us = statistics.median(event_us(hip_calls) / a.calls for _ in range(a.runs))

        def torch_once():
            d = torch_mesh_metrics(torch, pred, targets)
            torch.cuda.synchronize()
            return d
        for _ in range(3):
            torch_once()
        tt = []
        for _ in range(max(20, a.runs)):
            t0 = time.perf_counter()
            torch_once()
            tt.append(1e6 * (time.perf_counter() - t0))
        live = int((targets["is_valid"] * targets["right_valid"] != 0).sum() + (targets["is_valid"] * targets["left_valid"] != 0).sum())
        dist = 4 * V * V * 2 * B                          # both halves of a workgroup walk their loops whatever the flags
        row = {"valid_hands": live, "distance_evals": dist, "hip_us": round(us, 2),
               "hip_gdist_per_s": round(dist / (us * 1e-6) / 1e9, 1), "hip_gflops": round(8 * dist / (us * 1e-6) / 1e9, 1),
               "torch_ops_us": round(statistics.median(tt), 1), "max_abs_diff_vs_torch": {k: float(f"{v:.3g}") for k, v in worst.items()}}
        row["torch_ops_over_hip"] = round(row["torch_ops_us"] / us, 1)
        if not a.no_forward:
            model = hands_amd.apply_recipe(hands_amd.HandsLight()).to(dev)
            inputs, meta = hands_amd.synthetic_inputs(B, 0)
            inputs, meta = {k: t.to(dev) for k, t in inputs.items()}, {k: t.to(dev) for k, t in meta.items()}

            def fwd():
                len(model(inputs, meta))               # len() joins the forward's tail stream
            for _ in range(3):
                fwd()
            torch.cuda.synchronize()
            f_us = statistics.median(event_us(fwd) for _ in range(10))
            row["forward_us"] = round(f_us, 1)
            row["share_of_forward"] = round(us / f_us, 4)
            del model
            torch.cuda.empty_cache()
        out["batches"][str(B)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
