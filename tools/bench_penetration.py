#!/usr/bin/env python3
"""Device time of hands_amd.interhand_penetration (two launches of hands_mesh_signed_f32, V = 778 queries each) and of
hands_amd.intersection_volume (two launches with G^3 queries each) on two closed, MANO-sized hands: 778 vertices, 1552 faces.

Per quantity: the median over `--runs` event-timed runs of `--calls` back-to-back calls of the Python function after warm-up
(allocations included); the point-triangle pairs the definition needs and the rate they are done at; the same numbers composed
from torch ops on the same device (a (b, P, F) broadcast per direction, `--torch-chunk` samples at a time, fp32), wall clock
ending in a synchronise; both checked against each other before timing; and the share of a HandsLight forward at that batch
size.  No profiler.  Prints one JSON line per quantity."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")


def closed_hand(torch, n_lon=97, n_lat=9, radii=(0.045, 0.03, 0.09)):
    """A closed, outward ellipsoid with MANO's vertex count: 2 + n_lon (n_lat - 1) = 778 vertices, 2 n_lon (n_lat - 1) = 1552
    faces (MANO sealed at the wrist has 779 and 1554)."""
    v = [[0.0, 0.0, 1.0]]
    for i in range(1, n_lat):
        t = math.pi * i / n_lat
        v += [[math.sin(t) * math.cos(2 * math.pi * j / n_lon), math.sin(t) * math.sin(2 * math.pi * j / n_lon), math.cos(t)]
              for j in range(n_lon)]
    v.append([0.0, 0.0, -1.0])
    ring = lambda i, j: 1 + (i - 1) * n_lon + j % n_lon
    f = [[0, ring(1, j), ring(1, j + 1)] for j in range(n_lon)]
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            f += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    f += [[len(v) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)] for j in range(n_lon)]
    return torch.tensor(v) * torch.tensor(radii), torch.tensor(f, dtype=torch.int32)


def torch_winding(torch, q, v, faces, chunk):
    """Generalised winding number of q (B,P,3) about the triangles `faces` (F,3) over v (B,V,3): fp32 torch ops."""
    dot = lambda a, b: (a * b).sum(-1)
    out = []
    for i in range(0, len(q), chunk):
        p = q[i:i + chunk, :, None, :]
        a, b, c = (v[i:i + chunk][:, faces[:, k]][:, None] - p for k in range(3))
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        num = dot(a, torch.linalg.cross(b, c))
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        out.append(torch.atan2(num, den).sum(2) / (2 * math.pi))
    return torch.cat(out)


def torch_penetration(torch, v_r, v_l, faces, chunk):
    from bench_surface_metrics import torch_point_to_surface
    out = {}
    for k, q, t, fc in (("rl", v_r, v_l, faces[1]), ("lr", v_l, v_r, faces[0])):
        inside = torch_winding(torch, q, t, fc, chunk).abs() >= 0.5
        dist = torch_point_to_surface(torch, q, t, fc, chunk)
        out["sdf." + k] = torch.where(inside, -dist, dist)
        out["pen.depth." + k] = (-out["sdf." + k].min(1).values).clamp_min(0.0)
        out["pen.count." + k] = inside.sum(1)
    return out


def torch_volume(torch, v_r, v_l, faces, G, chunk):
    import hands_amd
    points, cell = hands_amd.penetration_grid(v_r, v_l, G)
    both = (torch_winding(torch, points, v_r, faces[0], chunk).abs() >= 0.5) & (torch_winding(torch, points, v_l, faces[1], chunk).abs() >= 0.5)
    return both.sum(1).float() * cell


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--grid", type=int, default=24)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--torch-runs", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=8, help="samples per broadcast of the torch-ops penetration (the volume takes 1)")
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward the share is taken of")
    a = ap.parse_args()
    import torch
    import hands_amd
    if not torch.cuda.is_available():
        raise SystemExit("bench_penetration.py needs a HIP device: a CPU run cannot give a time")
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    B, G = a.batch, a.grid
    v, f = closed_hand(torch)
    V, F = v.shape[0], f.shape[0]
    g = torch.Generator().manual_seed(7)
    # the left hand 3 cm beside the right one (they overlap), each sample moved and stretched a little
    jit = lambda: (1.0 + 0.05 * torch.randn(B, 1, 3, generator=g)) * v[None] + 0.004 * torch.randn(B, 1, 3, generator=g)
    centre = torch.tensor([0.05, -0.03, 0.5])
    v_r, v_l = (jit() + centre).to(dev), (jit() + centre + torch.tensor([0.03, 0.01, 0.0])).to(dev)
    faces = (f.to(dev), f.to(dev))
    hands = {"mano.v3d.cam.r": v_r, "mano.v3d.cam.l": v_l}

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    def wall_us(fn, runs):
        fn()
        torch.cuda.synchronize()
        tt = []
        for _ in range(runs):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            tt.append(1e6 * (time.perf_counter() - t0))
        return statistics.median(tt)

    # the two agree before either is timed: distances to 1e-6 m, flags and counts but for points within 1e-4 of |w| = 0.5
    pen, ref = hands_amd.interhand_penetration(hands, faces=faces), torch_penetration(torch, v_r, v_l, faces, a.torch_chunk)
    worst_d, flips = 0.0, 0
    for k in ("rl", "lr"):
        w = hands_amd.signed_distance_to_mesh(*((v_r, v_l, faces[1]) if k == "rl" else (v_l, v_r, faces[0])))[1]
        sure = (w.abs() - 0.5).abs() > 1e-4
        worst_d = max(worst_d, float((pen["sdf." + k].abs() - ref["sdf." + k].abs()).abs().max()))
        flips += int(((pen["sdf." + k] < 0) != (ref["sdf." + k] < 0))[sure].sum())
    vol, vref = hands_amd.intersection_volume(hands, faces=faces, G=G), torch_volume(torch, v_r, v_l, faces, G, 1)
    points, cell = hands_amd.penetration_grid(v_r, v_l, G)
    cells_off = float(((vol - vref).abs() / cell).max())
    if not (worst_d < 1e-6 and flips == 0 and cells_off <= 2):
        raise SystemExit(f"kernel and torch ops disagree: distance {worst_d} m, sign flips {flips}, volume {cells_off} cells")
    f_us = None
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
        del model
        torch.cuda.empty_cache()
    jobs = (("interhand_penetration", lambda: hands_amd.interhand_penetration(hands, faces=faces),
             lambda: torch_penetration(torch, v_r, v_l, faces, a.torch_chunk), 2 * V * F * B,
             {"vertices_inside_mean": float(pen["pen.count.rl"].float().mean() + pen["pen.count.lr"].float().mean()) / 2,
              "depth_mm_mean": 1e3 * float(pen["pen.depth.rl"].mean() + pen["pen.depth.lr"].mean()) / 2,
              "max_abs_diff_vs_torch_m": float(f"{worst_d:.3g}")}),
            ("intersection_volume", lambda: hands_amd.intersection_volume(hands, faces=faces, G=G),
             lambda: torch_volume(torch, v_r, v_l, faces, G, 1), 2 * G ** 3 * F * B,
             {"grid": G, "volume_cm3_mean": 1e6 * float(vol.mean()), "max_cells_off_vs_torch": cells_off}))
    for name, hip, tch, pairs, extra in jobs:
        def run():
            for _ in range(a.calls):
                hip()
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        us = statistics.median(event_us(run) / a.calls for _ in range(a.runs))
        t_us = wall_us(tch, a.torch_runs)
        row = {"tool": "bench_penetration", "quantity": name, "batch": B, "verts": V, "faces": F, "hip_us": round(us, 1),
               "pairs": pairs, "hip_gpairs_per_s": round(pairs / us / 1e3, 1), "torch_ops_us": round(t_us, 1),
               "torch_ops_over_hip": round(t_us / us, 1), **extra}
        if f_us is not None:
            row.update(forward_us=round(f_us, 1), share_of_forward=round(us / f_us, 4))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
