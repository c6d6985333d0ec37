#!/usr/bin/env python3
"""Throughput of ``HandsLight(backbone='vit_b_16')`` and where its time goes.

  1. shipped mode (trunk jobs on side streams, asynchronous tail): `--warmup` forwards, then `--steps` timed forwards at `--bz`
     between two synchronisations -> hands/s (2 hands per sample, as bench.py counts);
  2. one-stream pass (``overlap_trunks = False``) with every GEMM / convolution launch and every attention call bracketed by
     events: the GEMMs' algorithmic FLOP rate as a fraction of the fp32-MFMA peak (157.3 TFLOP/s), the attention kernel's time
     per call and its share of the forward;
  3. the attention kernels alone, same box, same run: attention_kernel<13,64,197> (ViT-B/16: 197 tokens, 12 heads x 64, one
     call of the hand job = 2 bz crops) next to attention_kernel<12,80,192> (ViT-H/16 of hamer_light: 192 tokens, 16 heads x 80, 128
     crops = its bz 64 test shape), each as algorithmic GFLOP/s (4 T^2 D per head and crop).

Recipe weights, synthetic inputs; events only, no profiler.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("HANDS_SYNTHETIC_MANO", "1")
FP32_MFMA_PEAK_TFLOPS = 157.3


def attention_rate(L, torch, B, T, heads, D, iters=20, warmup=3):
    from hands_amd._lib import check, ptr
    qkv = torch.randn(B, T, 3 * heads * D, device="cuda")
    out = torch.empty(B, T, heads * D, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    run = lambda: check(L.hands_attention_f32(ptr(qkv), ptr(out), B, T, heads, D, float(D ** -0.5), st), "attention")
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        run()
    t1.record()
    torch.cuda.synchronize()
    us = 1e3 * t0.elapsed_time(t1) / iters
    flop = 4.0 * T * T * D * heads * B
    return {"crops": B, "tokens": T, "heads": heads, "head_dim": D, "us_per_call": round(us, 1),
            "algorithmic_tflops": round(flop / (us * 1e-6) / 1e12, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bz", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--attention-only", action="store_true", help="part 3 only: the two attention kernels alone")
    a = ap.parse_args()
    import torch
    import hands_amd
    from hands_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_vit_backbone.py needs a HIP device: a CPU run cannot give a time")
    dev, bz = torch.device("cuda:0"), a.bz
    L = _lib.lib()
    out = {"tool": "bench_vit_backbone", "device": torch.cuda.get_device_name(0), "bz": bz, "steps": a.steps, "warmup": a.warmup}
    if a.attention_only:
        out["attention_vit_b"] = attention_rate(L, torch, 2 * bz, 197, 12, 64)
        out["attention_vit_h"] = attention_rate(L, torch, 128, 192, 16, 80)
        print(json.dumps(out))
        return
    model = hands_amd.apply_recipe(hands_amd.HandsLight(backbone="vit_b_16")).eval().to(dev)
    inputs, meta = hands_amd.synthetic_inputs(bz, 0)
    inputs, meta = {k: v.to(dev) for k, v in inputs.items()}, {k: v.to(dev) for k, v in meta.items()}

    # ---- 1. shipped mode --------------------------------------------------------------------------------------------------------
    for _ in range(a.warmup):
        model(inputs, meta)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        res = model(inputs, meta)
    dict(res.items())                      # joins the asynchronous tail of the last forward
    torch.cuda.synchronize(dev)
    el = time.perf_counter() - t0
    out["hands_per_s"] = round(2 * bz * a.steps / el, 1)
    out["ms_per_step"] = round(el / a.steps * 1e3, 2)

    # ---- 2. one-stream pass with per-launch events ------------------------------------------------------------------------------
    model.overlap_trunks = False
    model(inputs, meta)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    model(inputs, meta)
    torch.cuda.synchronize(dev)
    ser_ms = (time.perf_counter() - t0) * 1e3
    main_stream = torch.cuda.current_stream(dev)
    gemm_ev, gemm_info, att_ev = [], [], []

    def mark(lst):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record(main_stream)
        lst.append(ev)

    def hook(phase, pc, npix, stream_handle, has_res, kernel):
        assert stream_handle == main_stream.cuda_stream
        mark(gemm_ev)
        if phase == "begin":
            gemm_info.append((kernel, pc.KH, 2.0 * pc.macs_per_pixel * npix))

    real = L.hands_attention_f32

    def timed_attention(*args):
        mark(att_ev)
        rc = real(*args)
        mark(att_ev)
        return rc

    model.conv_hook, L.hands_attention_f32 = hook, timed_attention
    try:
        model(inputs, meta)
        torch.cuda.synchronize(dev)
    finally:
        model.conv_hook, L.hands_attention_f32 = None, real
        model.overlap_trunks = True
    cal = [torch.cuda.Event(enable_timing=True) for _ in range(202)]
    for ev in cal:
        ev.record(main_stream)
    torch.cuda.synchronize(dev)
    gaps = sorted(cal[i].elapsed_time(cal[i + 1]) for i in range(0, 202, 2))
    ovh = gaps[len(gaps) // 2]                      # an empty event pair still reads a few microseconds
    dur = lambda evs: [max(evs[i].elapsed_time(evs[i + 1]) - ovh, 0.0) for i in range(0, len(evs), 2)]
    g_ms, a_ms = dur(gemm_ev), dur(att_ev)
    # the trunks' GEMMs: the pointwise launches with >= 197 rows per image (qkv, proj, fc1, fc2) + the patch embedding; vit_conv apart
    trunk = [(ms, fl) for ms, (k, kh, fl) in zip(g_ms, gemm_info) if fl >= 2.0 * 768 * 768 * 197 * bz]
    t_ms, t_fl = sum(m for m, _ in trunk), sum(f for _, f in trunk)
    all_ms, all_fl = sum(g_ms), sum(f for _, _, f in gemm_info)
    out["one_stream"] = {
        "ms_per_step": round(ser_ms, 2), "hands_per_s": round(2 * bz / (ser_ms * 1e-3), 1),
        "trunk_gemm_launches": len(trunk), "trunk_gemm_ms": round(t_ms, 2), "trunk_gemm_tflops": round(t_fl / (t_ms * 1e-3) / 1e12, 2),
        "trunk_gemm_frac_of_fp32_mfma_peak": round(t_fl / (t_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
        "all_mfma_launches": len(g_ms), "all_mfma_ms": round(all_ms, 2),
        "all_mfma_frac_of_fp32_mfma_peak": round(all_fl / (all_ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
        "algorithmic_gflop_per_image": round(all_fl / (3 * bz) / 1e9, 2),
        "attention_calls": len(a_ms), "attention_ms_total": round(sum(a_ms), 2),
        "attention_us_per_call": {"global_job": round(1e3 * sorted(a_ms[:12])[6], 1), "hand_job": round(1e3 * sorted(a_ms[12:])[6], 1)},
        "attention_share_of_forward": round(sum(a_ms) / ser_ms, 4),
        "event_pair_overhead_us": round(1e3 * ovh, 2)}
    del model
    torch.cuda.empty_cache()

    # ---- 3. the two attention kernels, alone ------------------------------------------------------------------------------------
    out["attention_vit_b"] = attention_rate(L, torch, 2 * bz, 197, 12, 64)
    out["attention_vit_h"] = attention_rate(L, torch, 128, 192, 16, 80)
    out["attention_rate_ratio_b_over_h"] = round(out["attention_vit_b"]["algorithmic_tflops"] / out["attention_vit_h"]["algorithmic_tflops"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
