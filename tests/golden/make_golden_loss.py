#!/usr/bin/env python3
"""Generate tests/golden/loss_light.npz with the REAL reference loss code: compute_loss_light
(src/callbacks/loss/loss_arctic_sf.py:20-206, src/utils/loss_modules.py:97-152) and the epoch aggregation
pl_utils.reform_outputs (common/pl_utils.py:46-63) + np.nanmean (common/abstract_pl.py:134-137).  Dev container only.

Layout of the file (tests/loss_ref.py:load_fixture reads it):
  base/{pred,gt,meta}.<key>          the inputs of case a (B = 5, S = 16, every switch on)
  case/<c>/{pred,gt,meta}.<key>      the arrays case <c> replaces
  case/<c>/out/<i>                   the reference's value of the i-th key (fp32, shape (1,))
  epoch/...                          step records and what reform_outputs made of them
  meta                               JSON: per case the batch slice, the switches, keys, weights, and
                                       d_ref      max_k |ref_fp32 - ref_fp64| / |ref_fp64|  (the reference's own fp32 error)
                                       d_threads  the same distance between the fp32 run at 1 and at 8 ATen threads
`--check` regenerates in memory and compares every array with the committed file bit for bit.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from _ref_shims import *  # noqa: F401,F403
from _ref_shims import META, Args
import numpy as np
import torch

import common.pl_utils as pl_utils  # noqa: E402  (real reference code)
from src.callbacks.loss.loss_arctic_sf import compute_loss_light  # noqa: E402  (real reference code)
import loss_ref  # noqa: E402  (inputs only: random_case)

ALL = dict(use_grasp_loss=True, use_render_seg_loss=True, use_depth_loss=True, regress_center_corner=True)
BASE_ONLY = dict(use_grasp_loss=False, use_render_seg_loss=False, use_depth_loss=False, regress_center_corner=False)


def run_ref(pred, gt, meta, args, dtype=torch.float32):
    c = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in d.items()}
    out = compute_loss_light(c(pred), c(gt), c(meta), Args(args))
    return [(k, v[0].detach().clone(), float(v[1])) for k, v in out.items()]


def rel_dist(a, b):
    """max_k |a_k - b_k| / |b_k| over the keys where b is finite and non-zero."""
    worst = 0.0
    for (_, x, _), (_, y, _) in zip(a, b):
        x, y = float(x.double()), float(y.double())
        if np.isfinite(y) and y != 0.0 and np.isfinite(x):
            worst = max(worst, abs(x - y) / abs(y))
    return worst


def cases():
    pred, gt, meta, _ = loss_ref.random_case(5, 16, 16, seed=3)
    gt["right_valid"] = torch.tensor([1.0, 0, 1, 1, 0])
    gt["left_valid"] = torch.tensor([1.0, 1, 0, 1, 1])
    base = (pred, gt, meta)
    out = {"a": ({}, {}, {}, ALL, None)}
    pb, gb, _, _ = loss_ref.random_case(5, 31, 31, seed=4)
    out["b"] = ({k: pb[k] for k in pb if k.startswith(("render.", "depth."))},
                {k: gb[k] for k in gb if k.startswith(("render.", "depth."))}, {}, ALL, None)
    out["c"] = ({}, {"right_valid": torch.zeros(5), "grasp_valid_r": torch.zeros(5)}, {}, ALL, None)
    out["d"] = ({}, {}, {k: torch.zeros(5) for k in meta}, ALL, None)
    nan_cam = pred["mano.cam_t.wp.r"].clone()
    nan_cam[1, 0] = float("nan")                       # sample 1: right hand invalid
    out["e"] = ({"mano.cam_t.wp.r": nan_cam}, {}, {k: torch.ones(5) for k in meta}, ALL, None)
    out["f"] = ({"mano.cam_t.wp.r": nan_cam}, {"right_valid": torch.zeros(5)}, {k: torch.ones(5) for k in meta}, ALL, None)
    out["g"] = ({}, {}, {}, ALL, 1)
    out["h"] = ({}, {}, {}, BASE_ONLY, None)
    return base, out


def epoch_records():
    g = torch.Generator().manual_seed(9)
    steps = []
    for i, n in enumerate((3, 2, 4)):                  # uneven step sizes
        m1, m2 = torch.rand(n, generator=g) * 20, torch.rand(n, 42, generator=g) * 5
        if i == 1:
            m1[0] = float("nan")
            m2[1, 5] = float("nan")
        steps.append({"out_dict": {"imgname": [f"s{i}_{j}.jpg" for j in range(n)], "metric.mpjpe/ra/h": m1, "metric.pix_err/h": m2},
                      "loss": {"loss/mano/kp2d/r": torch.rand((), generator=g), "loss/mano/pose/l": torch.rand((), generator=g),
                               "loss": torch.rand((), generator=g) * 3}})
    return steps


def build():
    base, cs = cases()
    rec = {}
    for grp, d in zip(("pred", "gt", "meta"), base):
        rec.update({f"base/{grp}.{k}": v.numpy() for k, v in d.items()})
    info = {}
    for name, (po, go, mo, args, sl) in cs.items():
        full = []
        for d, o in zip(base, (po, go, mo)):
            m = dict(d)
            m.update(o)
            full.append({k: (v[:sl] if sl else v) for k, v in m.items()})
        for grp, o in zip(("pred", "gt", "meta"), (po, go, mo)):
            rec.update({f"case/{name}/{grp}.{k}": v.numpy() for k, v in o.items()})
        torch.set_num_threads(8)
        r32 = run_ref(*full, args)
        r64 = run_ref(*full, args, dtype=torch.float64)
        torch.set_num_threads(1)
        r32_1 = run_ref(*full, args)
        torch.set_num_threads(8)
        for i, (_, v, _) in enumerate(r32):
            assert v.dtype == torch.float32 and v.shape == (1,)
            rec[f"case/{name}/out/{i}"] = v.numpy()
        info[name] = {"slice": sl, "args": args, "keys": [k for k, _, _ in r32], "weights": [w for _, _, w in r32],
                      "d_ref": rel_dist(r32, r64), "d_threads": rel_dist(r32_1, r32)}
        print(name, len(r32), "keys  d_ref %.3g  d_threads %.3g" % (info[name]["d_ref"], info[name]["d_threads"]))
    steps = epoch_records()
    outputs, loss_dict = pl_utils.reform_outputs(steps)
    for i, s in enumerate(steps):
        for k, v in s["out_dict"].items():
            if torch.is_tensor(v):
                rec[f"epoch/step{i}/out_dict/{k}"] = v.numpy()
        for k, v in s["loss"].items():
            rec[f"epoch/step{i}/loss/{k}"] = v.numpy()
    for k, v in outputs.items():
        if "metric." in k:
            rec[f"epoch/out/{k}"] = np.asarray(np.nanmean(np.array(v)))
    for k, v in loss_dict.items():
        rec[f"epoch/out/{k}"] = np.asarray(v, dtype=np.float64)
    meta = dict(META, what="loss_arctic_sf.py compute_loss_light; pl_utils.reform_outputs", cases=info,
                epoch={"steps": len(steps), "imgnames": [s["out_dict"]["imgname"] for s in steps],
                       "all_imgnames": list(outputs["imgname"])})
    meta.pop("torch", None)                            # the arrays, not the torch build, are what --check compares
    rec["meta"] = np.array(json.dumps(meta, sort_keys=True))
    return rec


def main():
    path = os.path.join(HERE, "loss_light.npz")
    rec = build()
    if "--check" in sys.argv:
        old = np.load(path)
        assert sorted(old.files) == sorted(rec), set(old.files) ^ set(rec)
        for k in rec:
            a, b = np.asarray(rec[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k
        print("loss_light.npz regenerates bit-equal:", len(rec), "arrays")
        return
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
