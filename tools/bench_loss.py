#!/usr/bin/env python3
"""Device time of the validation loss dict (hands_loss_light_f32, csrc/loss.hip: two launches) with every switch on, S = 224.

Per batch size (256 and 32): the median over `--runs` event-timed runs of `--calls` back-to-back evaluations, the inputs
rotating over enough sets to exceed the 256 MB Infinity Cache (so every tensor comes from HBM); the bytes read and the achieved
GB/s against the streaming-read ceiling measured in this process (hands_ceiling_hbm_read_f32, 2 GiB, best of 3) and the 8 TB/s
datasheet figure; the same dict evaluated with torch ops on the same device (tests/loss_ref.py -- what a user had to do before),
wall clock with a synchronise per evaluation since it synchronises anyway; and the share of a HandsLight forward at that
batch size.  No profiler.  Prints one JSON line."""
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


def device_case(torch, loss_ref, B, S, seed):
    """random_case's small tensors from the host, the eight large ones generated on the device."""
    pred, gt, meta, args = loss_ref.random_case(B, 1, 1, seed=seed, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for h in "rl":
        pred[f"render.{h}"] = torch.rand(B, 1, S, S, device="cuda", generator=g)
        gt[f"render.{h}"] = (torch.rand(B, 1, S, S, device="cuda", generator=g) < 0.3).float()
        pred[f"depth.{h}"] = 0.6 + 0.2 * torch.randn(B, S, S, device="cuda", generator=g)
        gt[f"depth.{h}"] = 0.6 + 0.2 * torch.randn(B, S, S, device="cuda", generator=g)
    return pred, gt, meta, args


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--img-res", type=int, default=224)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--calls", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-forward", action="store_true", help="skip the HandsLight forward the share is taken of")
    a = ap.parse_args()
    assert a.runs >= 20
    import torch
    import hands_amd
    import loss_ref
    from hands_amd import _lib, losses
    if not torch.cuda.is_available():
        raise SystemExit("bench_loss.py needs a HIP device: a CPU run cannot give a time")
    L = _lib.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev)
    S = a.img_res

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)

    # the streaming-read ceiling, same process
    buf = torch.ones((2 << 30) // 4, device=dev)
    sink = torch.empty(512 * 256, device=dev)
    read = lambda: _lib.check(L.hands_ceiling_hbm_read_f32(_lib.ptr(buf), buf.numel(), _lib.ptr(sink), st.cuda_stream), "ceiling")
    event_us(read)
    ceiling = max(buf.numel() * 4 / (event_us(read) * 1e-6) for _ in range(3)) / 1e9
    del buf
    torch.cuda.empty_cache()
    out = {"tool": "bench_loss", "img_res": S, "runs": a.runs, "calls_per_run": a.calls, "hbm_read_ceiling_gbs": round(ceiling, 1),
           "datasheet_gbs": 8000.0, "batches": {}}
    for B in a.batches:
        nbytes = 8 * B * S * S * 4 + 2 * B * 4 * (144 + 48 + 2 * (10 + 63 + 42 + 3 + 2 + 8) + 3 + 9 + 21 + 8)
        nsets = max(2, -(-(512 << 20) // nbytes))
        sets = [device_case(torch, loss_ref, B, S, seed=100 + i) for i in range(nsets)]
        bound = [losses.bind_loss_inputs(*c) for c in sets]
        ws = torch.empty(L.hands_loss_workspace_bytes(B, S, S) // 8, dtype=torch.float64, device=dev)
        res = torch.empty(43, device=dev)
        turn = [0]

        def hip_calls():
            for _ in range(a.calls):
                b = bound[turn[0] % nsets]
                turn[0] += 1
                _lib.check(L.hands_loss_light_f32(C.byref(b[0]), B, S, S, _lib.ptr(ws), _lib.ptr(res), _lib.ptr(res, 21),
                                                  _lib.ptr(res, 42), st.cuda_stream), "hands_loss_light_f32")
        for _ in range(a.warmup):
            hip_calls()
        torch.cuda.synchronize()
        us = statistics.median(event_us(hip_calls) / a.calls for _ in range(a.runs))

        def torch_once():
            c = sets[turn[0] % nsets]
            turn[0] += 1
            d = loss_ref.finish(loss_ref.compute_loss_light(*c))
            torch.cuda.synchronize()
            return d
        for _ in range(3):
            torch_once()
        tt = []
        for _ in range(max(20, a.runs)):
            t0 = time.perf_counter()
            torch_once()
            tt.append(1e6 * (time.perf_counter() - t0))
        row = {"bytes_read_mb": round(nbytes / 1e6, 1), "input_sets": nsets, "hip_us": round(us, 2),
               "hip_gbs": round(nbytes / (us * 1e-6) / 1e9, 1), "of_measured_ceiling": round(nbytes / (us * 1e-6) / 1e9 / ceiling, 3),
               "of_datasheet": round(nbytes / (us * 1e-6) / 1e9 / 8000.0, 3), "torch_ops_us": round(statistics.median(tt), 1)}
        row["torch_ops_over_hip"] = round(row["torch_ops_us"] / us, 1)
        del sets, bound
        torch.cuda.empty_cache()
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
