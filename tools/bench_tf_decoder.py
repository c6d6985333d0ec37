#!/usr/bin/env python3
"""What ``HandsLight(tf_decoder=True)`` costs and where the transformer head's time goes.

  1. shipped mode (trunk jobs on side streams, asynchronous tail): `--warmup` forwards, then `--steps` timed forwards at `--bz`
     between two synchronisations, with the switch off and on -> ms per step and hands/s (2 hands per sample, as bench.py counts);
  2. one-stream pass of the tf_decoder model (``overlap_trunks = False``) with the two ``tf_head`` calls bracketed by events:
     the head's share of the forward;
  3. hands_wide_attention_f32 alone at the head's two shapes -- 109 tokens x 109 tokens reading a packed (bz, 109, 3072) in_proj
     output, 109 tokens x 49 pixels reading a (bz, 49, 2048) k | v buffer, D = 1024, one hand's batch -- as time per call and
     algorithmic TFLOP/s (4 Tq Tk D per batch element).

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


def attention_rate(L, torch, B, Tq, Tk, D=1024, iters=20, warmup=3):
    from hands_amd._lib import check, ptr
    if Tq == Tk:       # self-attention: q | k | v packed
        buf = torch.randn(B, Tq, 3 * D, device="cuda")
        q, ldq, k, v, ldk = ptr(buf), 3 * D, ptr(buf, D), ptr(buf, 2 * D), 3 * D
    else:              # cross-attention: q alone, k | v packed
        qb, buf = torch.randn(B, Tq, D, device="cuda"), torch.randn(B, Tk, 2 * D, device="cuda")
        q, ldq, k, v, ldk = ptr(qb), D, ptr(buf), ptr(buf, D), 2 * D
    out = torch.empty(B, Tq, D, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    run = lambda: check(L.hands_wide_attention_f32(q, Tq * ldq, ldq, k, Tk * ldk, ldk, v, Tk * ldk, ldk, ptr(out), Tq * D, D, B, Tq, Tk, D,
                                                   float(D ** -0.5), st), "wide_attention")
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
    tflops = 4.0 * Tq * Tk * D * B / (us * 1e-6) / 1e12
    return {"batch": B, "Tq": Tq, "Tk": Tk, "D": D, "us_per_call": round(us, 1), "algorithmic_tflops": round(tflops, 2),
            "frac_of_fp32_mfma_peak": round(tflops / FP32_MFMA_PEAK_TFLOPS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bz", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--attention-only", action="store_true", help="part 3 only")
    a = ap.parse_args()
    import torch
    import hands_amd
    from hands_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_tf_decoder.py needs a HIP device: a CPU run cannot give a time")
    dev, bz = torch.device("cuda:0"), a.bz
    L = _lib.lib()
    out = {"tool": "bench_tf_decoder", "device": torch.cuda.get_device_name(0), "bz": bz, "steps": a.steps, "warmup": a.warmup}
    if not a.attention_only:
        inputs, meta = hands_amd.synthetic_inputs(bz, 0)
        inputs, meta = {k: v.to(dev) for k, v in inputs.items()}, {k: v.to(dev) for k, v in meta.items()}
        for tf in (False, True):
            model = hands_amd.apply_recipe(hands_amd.HandsLight(tf_decoder=tf)).eval().to(dev)
            for _ in range(a.warmup):
                model(inputs, meta)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                res = model(inputs, meta)
            dict(res.items())                      # joins the asynchronous tail of the last forward
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
            rec = {"ms_per_step": round(el / a.steps * 1e3, 2), "hands_per_s": round(2 * bz * a.steps / el, 1)}
            if tf:
                # one stream, the two heads one after the other, each between two events
                model.overlap_trunks = False
                model(inputs, meta)
                torch.cuda.synchronize(dev)
                from hands_amd import hands_light as HL
                evs, real = [], HL.tf_head

                def mark():
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(torch.cuda.current_stream(dev))
                    evs.append(ev)

                def timed_head(*args, **kw):
                    mark()
                    real(*args, **kw)
                    mark()

                HL.tf_head = timed_head
                t0 = time.perf_counter()
                model(inputs, meta)
                torch.cuda.synchronize(dev)
                ser_ms = (time.perf_counter() - t0) * 1e3
                HL.tf_head = real
                head_ms = sum(evs[i].elapsed_time(evs[i + 1]) for i in range(0, len(evs), 2))
                rec["one_stream"] = {"ms_per_step": round(ser_ms, 2), "tf_head_ms_both_hands": round(head_ms, 2),
                                     "tf_head_share_of_forward": round(head_ms / ser_ms, 4)}
            out["tf_decoder_on" if tf else "tf_decoder_off"] = rec
            del model
            torch.cuda.empty_cache()
        out["slowdown_on_over_off"] = round(out["tf_decoder_on"]["ms_per_step"] / out["tf_decoder_off"]["ms_per_step"], 3)
    out["attention_self_109x109"] = attention_rate(L, torch, bz, 109, 109)
    out["attention_cross_109x49"] = attention_rate(L, torch, bz, 109, 49)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
