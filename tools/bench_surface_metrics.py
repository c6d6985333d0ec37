#!/usr/bin/env python3
"""Device time of the surface metrics (hands_eval_surface_metrics_f32, csrc/mesh_distance.hip: two launches) and of
hands_amd.interhand_field (two launches of hands_mesh_closest_f32) with MANO's counts, V = 778 and F = 1538.

Per batch size (default 256): the median over `--runs` event-timed runs of `--calls` back-to-back calls after warm-up -- the
metrics through the C ABI with pre-bound structs, the field through its Python function; the point-triangle and point-point
evaluations the definitions need and the rate they are done at; the same numbers composed from torch ops on the same device
(a (b, 778, 1538) broadcast per direction, `--torch-chunk` samples at a time; `torch.cdist`; a batched fp64 `torch.linalg.svd`),
wall clock ending in a synchronise; both checked against each other before timing; and the share of a HandsLight forward at
that batch size.  No profiler.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")


def torch_point_to_surface(torch, q, v, faces, chunk):
    """Distance of q (B,P,3) to the triangles `faces` (F,3) over v (B,V,3): the three clamped segments and the in-plane
    projection where it falls inside, fp32 torch ops, `chunk` samples at a time."""
    dot = lambda a, b: (a * b).sum(-1)
    out = []
    for i in range(0, len(q), chunk):
        p = q[i:i + chunk, :, None, :]
        a, b, c = (v[i:i + chunk][:, faces[:, k]][:, None] for k in range(3))

        def seg(a, b):
            ab = b - a
            L = dot(ab, ab)
            t = torch.where(L > 0, dot(p - a, ab) / L.clamp_min(1e-38), torch.zeros_like(L)).clamp(0.0, 1.0)
            d = p - (a + t[..., None] * ab)
            return dot(d, d)
        d2 = torch.minimum(torch.minimum(seg(a, b), seg(a, c)), seg(b, c))
        ab, ac, ap = b - a, c - a, p - a
        n = torch.linalg.cross(ab, ac)
        nn = dot(n, n)
        d00, d01, d11, d1, d2_ = dot(ab, ab), dot(ab, ac), dot(ac, ac), dot(ap, ab), dot(ap, ac)
        nv, nw = d11 * d1 - d01 * d2_, d00 * d2_ - d01 * d1
        # a fused multiply-add leaves rounding noise in the normal of a face with a repeated index: a relative threshold
        inside = (nn > 1e-12 * d00 * d11) & (nv >= 0) & (nw >= 0) & (nv + nw <= d00 * d11 - d01 * d01)
        pl = dot(ap, n) ** 2 / nn.clamp_min(1e-38)
        out.append(torch.where(inside, torch.minimum(pl, d2), d2).min(2).values.sqrt())
    return torch.cat(out)


def torch_surface_metrics(torch, pred, targets, faces, chunk):
    """The twelve quantities with torch ops on the device, fp32 (fp64 for the 3x3 SVD), all hands batched."""
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

    out = {}
    for (h, hv), fc in zip((("r", "right_valid"), ("l", "left_valid")), faces):
        valid = targets[hv] * targets["is_valid"] != 0
        X = pred[f"mano.v3d.cam.{h}"] - pred[f"mano.j3d.cam.{h}"][:, :1]
        Y = targets[f"mano.v3d.cam.{h}"] - targets[f"mano.j3d.cam.{h}"][:, :1]
        for a in ("ra", "pa"):
            Q = X if a == "ra" else fit(X, Y)
            D = torch.cat([torch.cdist(Y[i:i + 16], Q[i:i + 16], compute_mode="donot_use_mm_for_euclid_dist")
                           for i in range(0, len(Y), 16)])
            vals = {f"chamfer/{a}": 500.0 * (D.min(1).values.mean(1) + D.min(2).values.mean(1)),
                    f"p2s/{a}": 500.0 * (torch_point_to_surface(torch, Q, Y, fc, chunk).mean(1) +
                                         torch_point_to_surface(torch, Y, Q, fc, chunk).mean(1))}
            for k, v in vals.items():
                out[f"{k}/{h}"] = torch.where(valid, v, torch.full_like(v, float("nan")))
    for k in [k[:-2] for k in out if k.endswith("/r")]:
        out[k + "/h"] = torch.stack([out[k + "/r"], out[k + "/l"]], 1).nanmean(1)
    return out


def torch_interhand(torch, v_r, v_l, faces, chunk, bnd=3e-3):
    d_rl, d_lr = torch_point_to_surface(torch, v_r, v_l, faces[1], chunk), torch_point_to_surface(torch, v_l, v_r, faces[0], chunk)
    return d_rl, d_lr, (d_rl < bnd).long(), (d_lr < bnd).long()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-runs", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=8)
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward the share is taken of")
    a = ap.parse_args()
    import torch
    import hands_amd
    from bench_mesh_metrics import make_case
    from hands_amd import _lib
    from hands_amd.metrics import SURF_KEYS, evaluate_surface_metrics
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_metrics.py needs a HIP device: a CPU run cannot give a time")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    V = 778
    faces = tuple(torch.from_numpy(hands_amd.synthetic_mano_asset(r).faces).to(dev, torch.int32).contiguous() for r in (True, False))
    F = faces[0].shape[0]

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    def wall_us(fn, runs):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        tt = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tt.append(1e6 * (time.perf_counter() - t0))
        return statistics.median(tt)

    out = {"tool": "bench_surface_metrics", "verts": V, "faces": F, "runs": a.runs, "calls_per_run": a.calls, "batches": {}}
    for B in a.batches:
        pred, targets = make_case(torch, B, V, seed=7)
        keep = [pred["mano.v3d.cam.r"], pred["mano.v3d.cam.l"], targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"],
                pred["mano.j3d.cam.r"], pred["mano.j3d.cam.l"], targets["mano.j3d.cam.r"], targets["mano.j3d.cam.l"],
                targets["is_valid"], targets["right_valid"], targets["left_valid"]]
        buf = torch.empty(3 * len(SURF_KEYS), B, device=dev)
        fin = _lib.MeshEvalIn(*[_lib.ptr(t) for t in keep])
        fout = _lib.SurfEvalOut(*[_lib.ptr(buf[i]) for i in range(buf.shape[0])])

        def hip_metrics():
            for _ in range(a.calls):
                _lib.check(L.hands_eval_surface_metrics_f32(C.byref(fin), _lib.ptr(faces[0]), _lib.ptr(faces[1]), F, F, C.byref(fout),
                                                            B, V, st.cuda_stream), "surface metrics")
        hands = {"mano.v3d.cam.r": targets["mano.v3d.cam.r"], "mano.v3d.cam.l": targets["mano.v3d.cam.l"] + 0.03}

        def hip_field():
            for _ in range(a.calls):
                hands_amd.interhand_field(hands, faces=faces)
        # the two agree before either is timed: to 1e-3 mm, and the contact flags but for vertices within 1e-6 m of the bound
        got, ref = evaluate_surface_metrics(pred, targets, faces=faces), torch_surface_metrics(torch, pred, targets, faces, a.torch_chunk)
        worst = 0.0
        for k in got:
            assert torch.equal(got[k].isnan(), ref[k].isnan()), k
            worst = max(worst, float((got[k] - ref[k]).abs().nan_to_num().max()))
        field = hands_amd.interhand_field(hands, faces=faces)
        t_rl, t_lr, c_rl, c_lr = torch_interhand(torch, hands["mano.v3d.cam.r"], hands["mano.v3d.cam.l"], faces, a.torch_chunk)
        worst_d = max(float((field["dist.rl"] - t_rl).abs().max()), float((field["dist.lr"] - t_lr).abs().max()))
        flips = int(((field["contact.rl"] != c_rl) & ((t_rl - 3e-3).abs() > 1e-6)).sum() +
                    ((field["contact.lr"] != c_lr) & ((t_lr - 3e-3).abs() > 1e-6)).sum())
        if not (worst < 1e-3 and worst_d < 1e-6 and flips == 0):
            raise SystemExit(f"kernel and torch ops disagree: metrics {worst} mm, field {worst_d} m, contact flips {flips}")
        row = {"max_abs_diff_vs_torch": {"metrics_mm": float(f"{worst:.3g}"), "field_m": float(f"{worst_d:.3g}")}}
        for name, fn in (("metrics", hip_metrics), ("field", hip_field)):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            row[f"hip_{name}_us"] = round(statistics.median(event_us(fn) / a.calls for _ in range(a.runs)), 1)
        row["torch_ops_metrics_us"] = round(wall_us(lambda: torch_surface_metrics(torch, pred, targets, faces, a.torch_chunk), a.torch_runs), 1)
        row["torch_ops_field_us"] = round(wall_us(lambda: torch_interhand(torch, hands["mano.v3d.cam.r"], hands["mano.v3d.cam.l"], faces,
                                                                          a.torch_chunk), a.torch_runs), 1)
        tri = 2 * 2 * 2 * V * F * B                       # point-triangle evaluations: hands x alignments x directions
        row.update(valid_hands=int((targets["is_valid"] * targets["right_valid"] != 0).sum() + (targets["is_valid"] * targets["left_valid"] != 0).sum()),
                   tri_evals_metrics=tri, hip_metrics_gtri_per_s=round(tri / row["hip_metrics_us"] / 1e3, 1),
                   tri_evals_field=2 * V * F * B, hip_field_gtri_per_s=round(2 * V * F * B / row["hip_field_us"] / 1e3, 1),
                   torch_ops_over_hip_metrics=round(row["torch_ops_metrics_us"] / row["hip_metrics_us"], 1),
                   torch_ops_over_hip_field=round(row["torch_ops_field_us"] / row["hip_field_us"], 1))
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
            row.update(forward_us=round(f_us, 1), metrics_share_of_forward=round(row["hip_metrics_us"] / f_us, 4),
                       field_share_of_forward=round(row["hip_field_us"] / f_us, 4))
            del model
            torch.cuda.empty_cache()
        out["batches"][str(B)] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
