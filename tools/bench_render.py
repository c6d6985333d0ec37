#!/usr/bin/env python3
"""Device time of the soft-silhouette rasteriser (hands_render_silhouette_f32, csrc/render.hip) per hand.

Two inputs at B = 512 hands (the two hands of bz = 256), S = 224:
  structured   the 778-vertex / 1538-face closed grid of tests/render_ref.py in 512 random poses (depth 0.35-0.8 m): a mesh
               shaped like a hand's, a few tens of faces per 32 x 8 pixel tile;
  forward      `mano.v3d.cam.{r,l}` of a real HandsLight forward (recipe weights, synthetic MANO asset) with the asset's own
               random faces: a triangle soup hundreds of layers deep, every tile's face list overflows and runs in chunks --
               the worst case, not a hand.
Events around `--iters` launches after `--warmup`; no profiler.  `--resources` cross-compiles the kernel with the resource
remarks on and prints its VGPR / LDS / scratch figures.  For the kernel trace run this tool under
`rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_render.py --iters 20` (a run of its own).
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
                        os.path.join(ROOT, "hands_amd", "csrc", "render.hip"), "-o", os.devnull],
                       capture_output=True, text=True, timeout=600, check=True)
    g = lambda pat: int(re.search(pat, p.stderr).group(1))
    return {"vgprs": g(r"VGPRs: (\d+)"), "sgprs": g(r"TotalSGPRs: (\d+)"), "scratch_bytes_per_lane": g(r"ScratchSize \[bytes/lane\]: (\d+)"),
            "vgpr_spill": g(r"VGPRs Spill: (\d+)"), "lds_static_bytes": g(r"LDS Size \[bytes/block\]: (\d+)"),
            "lds_dynamic_bytes_778_verts": 778 * 12, "waves_per_simd_by_registers": g(r"Occupancy \[waves/SIMD\]: (\d+)")}


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
    ap.add_argument("--hands", type=int, default=512)
    ap.add_argument("--img-res", type=int, default=224)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--resources", action="store_true")
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward input")
    a = ap.parse_args()
    out = {"tool": "bench_render", "hands": a.hands, "img_res": a.img_res, "iters": a.iters}
    if a.resources:
        out["resources"] = resources()
    import numpy as np
    import torch
    import hands_amd
    import render_ref as R
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs a HIP device: a CPU run cannot give a time")
    dev, B, S = torch.device("cuda:0"), a.hands, a.img_res
    v, f = R.mano_sized_mesh()
    V, K = R.poses(v, S, B, seed=0)
    Vd, fd, Kd = torch.from_numpy(V).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(K).to(dev)
    for name, zb in (("structured_us_per_hand", False), ("structured_with_zbuf_us_per_hand", True)):
        out[name] = round(time_us(lambda: hands_amd.rasterize(Vd, fd, Kd, S, return_zbuf=zb), a.warmup, a.iters) / B, 3)
    m = hands_amd.rasterize(Vd, fd, Kd, S, return_zbuf=False)["mask"]
    out["structured_mean_coverage"] = round(float((m > 0.5).float().mean()), 4)
    if not a.no_forward:
        bz = B // 2
        model = hands_amd.apply_recipe(hands_amd.HandsLight()).to(dev)
        inputs, meta = hands_amd.synthetic_inputs(bz, 0)
        pred = model({k: t.to(dev) for k, t in inputs.items()}, {k: t.to(dev) for k, t in meta.items()})
        verts = torch.cat([pred["mano.v3d.cam.r"], pred["mano.v3d.cam.l"]]).contiguous()
        Kf = meta["intrinsics"].to(dev).repeat(2, 1, 1).contiguous()
        faces = torch.from_numpy(hands_amd.synthetic_mano_asset(True).faces.astype(np.int32)).to(dev)
        del model
        iters = max(3, a.iters // 20)                      # two orders of magnitude more work per hand
        out["forward_soup_us_per_hand"] = round(time_us(lambda: hands_amd.rasterize(verts, faces, Kf, S, return_zbuf=False),
                                                        2, iters) / verts.shape[0], 3)
        m = hands_amd.rasterize(verts, faces, Kf, S, return_zbuf=False)["mask"]
        out["forward_soup_mean_coverage"] = round(float((m > 0.5).float().mean()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
