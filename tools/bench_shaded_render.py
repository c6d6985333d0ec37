#!/usr/bin/env python3
"""Device time of the shaded renderer (hands_mesh_prepare_f32 + hands_render_shaded_f32, csrc/shade.hip) per image.

Workload: `--images` (256) images x two MANO-sized hands at `--img-res` (224): the 778-vertex / 1538-face closed grid of
tests/render_ref.py in random poses (depth 0.35-0.8 m), the left hand a second pose of the same mesh.  Timed:
  overlay        one `Renderer.render_meshes_pose` over the batch (two pre-passes, one rasterise-and-shade launch);
  four_panel     `Renderer.visualize_rend`: the overlay plus the three side views, the whole (B, 4 S, S, 3) stack;
and, in the same run, for scale:
  silhouette     `hands_amd.rasterize` (csrc/render.hip) on the same 2 x images hands;
  forward        one `HandsLight` forward at bz = images (recipe weights, synthetic inputs).
Events around `--iters` calls after `--warmup`; no profiler.  `--resources` cross-compiles shade.hip with the resource remarks
on and prints the VGPR / LDS / scratch figures of both kernels.  For the kernel trace run this tool under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_shaded_render.py --iters 20` (a run of its own).
Prints one JSON line."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "hands_amd", "csrc", "shade.hip"), "-o", os.devnull],
                       capture_output=True, text=True, timeout=600, check=True)
    out = {}
    for blk in re.split(r"Function Name: ", p.stderr)[1:]:
        name = "prepare" if "mesh_prepare" in blk.split()[0] else "render_shaded"
        g = lambda pat: int(re.search(pat, blk).group(1))
        out[name] = {"vgprs": g(r"VGPRs: (\d+)"), "sgprs": g(r"TotalSGPRs: (\d+)"),
                     "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]: (\d+)"), "vgpr_spill": g(r"VGPRs Spill: (\d+)"),
                     "lds_bytes_per_workgroup": g(r"LDS Size \[bytes/block\]: (\d+)"),
                     "waves_per_simd": g(r"Occupancy \[waves/SIMD\]: (\d+)")}
    return out


def time_us(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--img-res", type=int, default=224)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward")
    a = ap.parse_args()
    out = {"tool": "bench_shaded_render", "images": a.images, "img_res": a.img_res, "iters": a.iters}
    if a.resources:
        out["resources"] = resources()
    import torch
    import hands_amd
    import render_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_shaded_render.py needs a HIP device: a CPU run cannot give a time")
    dev, B, S = torch.device("cuda:0"), a.images, a.img_res
    v, f = R.mano_sized_mesh()
    V, K = R.poses(v, S, 2 * B, seed=0)
    Vd, fd, Kd = torch.from_numpy(V).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(K).to(dev)
    vr, vl, Kb = Vd[:B].contiguous(), Vd[B:].contiguous(), Kd[:B].contiguous()
    vl = vl + (vr.mean(dim=1, keepdim=True) - vl.mean(dim=1, keepdim=True)) + torch.tensor([0.06, 0.0, 0.02], device=dev)   # beside the right hand
    img = torch.rand(B, 3, S, S, device=dev)
    r = hands_amd.Renderer(S)
    kw = dict(colors=[(100, 100, 254), (183, 100, 254)])
    out["overlay_us_per_image"] = round(time_us(lambda: r.render_meshes_pose([vr, vl], [fd, fd], Kb, image=img, **kw), a.warmup, a.iters) / B, 3)
    out["overlay_with_float_outputs_us_per_image"] = round(time_us(
        lambda: r.render_meshes_pose([vr, vl], [fd, fd], Kb, image=img, return_float=True, **kw), a.warmup, a.iters) / B, 3)
    out["four_panel_us_per_image"] = round(time_us(lambda: r.visualize_rend(vr, vl, Kb, img, faces_r=fd, faces_l=fd), a.warmup, a.iters) / B, 3)
    pic = r.render_meshes_pose([vr, vl], [fd, fd], Kb, image=img, return_float=True, **kw)
    out["overlay_mean_coverage"] = round(float((pic["face_id"] >= 0).float().mean()), 4)
    both = torch.cat([vr, vl]).contiguous()
    K2 = torch.cat([Kb, Kb]).contiguous()
    sil = time_us(lambda: hands_amd.rasterize(both, fd, K2, S, return_zbuf=False), a.warmup, a.iters)
    out["silhouette_us_per_image"] = round(sil / B, 3)                   # two hands
    out["silhouette_us_per_hand"] = round(sil / (2 * B), 3)
    if not a.no_forward:
        model = hands_amd.apply_recipe(hands_amd.HandsLight()).to(dev)
        inputs, meta = hands_amd.synthetic_inputs(B, 0)
        inputs, meta = {k: t.to(dev) for k, t in inputs.items()}, {k: t.to(dev) for k, t in meta.items()}
        fwd = time_us(lambda: model(inputs, meta), 3, max(5, a.iters // 10))
        out["forward_us_per_image"] = round(fwd / B, 3)
        out["four_panel_over_forward"] = round(out["four_panel_us_per_image"] / out["forward_us_per_image"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
