#!/usr/bin/env python3
"""Generate tests/golden/eval_acc_pose.npz with the REAL reference ``eval_acc_pose`` and ``compute_error_accel``
(src/utils/eval_modules.py:508-622).  Dev container only.

T = 16 frames of two hands with V = 96 vertices on smooth trajectories around z = 0.6 / 0.7 m, a few millimetres of noise on the
prediction; the flags hold a right-only, a left-only and a both-hands invalid frame, an ``is_valid = 0`` frame and two adjacent
invalid frames.  ``eval_acc_pose`` demands an object: it gets four vertices at the origin in prediction and ground truth, and
only ``acc/h`` is recorded.  Also recorded: ``compute_error_accel`` on the root-relative vertices of each hand before any
masking (T - 2 rows) and on one (T, N, 1) field.  ``meta["ref_vs_f64_max_rel"]`` is the largest relative deviation of the
reference's fp32 results from the fp64 restatement (tests/accel_ref.py) on these inputs: the error of the reference itself.
The module's import-time NameError is handled as in make_golden_metrics.py.
"""
import builtins
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _ref_shims import *  # noqa: F401,F403
from _ref_shims import META, _mod
import numpy as np
import torch

_mod("pytorch3d.ops", knn_points=None)
sys.modules["pytorch3d"].ops = sys.modules["pytorch3d.ops"]
builtins.eval_mpjpe_mano = None
import src.utils.eval_modules as em  # noqa: E402  (real reference code)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import accel_ref as AR  # noqa: E402

T, V = 16, 96


def trajectory(g, n, centre, phase):
    """(T, n, 3): a cloud of n points of a few centimetres that swings and turns smoothly about ``centre``."""
    t = torch.arange(T, dtype=torch.float32) / 30.0
    shape = 0.04 * torch.randn(n, 3, generator=g)
    ang = 0.8 * torch.sin(2.0 * t + phase)
    c, s, o, z = torch.cos(ang), torch.sin(ang), torch.ones(T), torch.zeros(T)
    R = torch.stack([torch.stack([c, -s, z], -1), torch.stack([s, c, z], -1), torch.stack([z, z, o], -1)], -2)    # (T,3,3)
    path = torch.stack([0.05 * torch.sin(3.0 * t + phase), 0.03 * torch.cos(2.0 * t), 0.04 * t * t], -1)        # (T,3)
    return torch.einsum("tij,nj->tni", R, shape) + path[:, None, :] + torch.tensor(centre)


def main():
    g = torch.Generator().manual_seed(41)
    gt = {"r": trajectory(g, V + 21, (-0.1, 0.0, 0.6), 0.0), "l": trajectory(g, V + 21, (0.1, 0.02, 0.7), 1.0)}
    pred, targets = {}, {}
    for h in "rl":
        noisy = gt[h] + 0.003 * torch.randn(gt[h].shape, generator=g)
        targets[f"mano.v3d.cam.{h}"], targets[f"mano.j3d.cam.{h}"] = gt[h][:, :V].contiguous(), gt[h][:, V:].contiguous()
        pred[f"mano.v3d.cam.{h}"], pred[f"mano.j3d.cam.{h}"] = noisy[:, :V].contiguous(), noisy[:, V:].contiguous()
    is_valid, right_valid, left_valid = torch.ones(T), torch.ones(T), torch.ones(T)
    right_valid[3] = 0                     # right only
    left_valid[[6, 7]] = 0                 # left only, two adjacent frames
    right_valid[9] = left_valid[9] = 0     # both hands
    is_valid[12] = 0
    targets.update(is_valid=is_valid, right_valid=right_valid, left_valid=left_valid)
    obj = {"object.v.cam": torch.zeros(T, 4, 3)}
    with np.errstate(all="ignore"):
        out = em.eval_acc_pose({**pred, **obj}, {**targets, **obj, "object.parts_ids": torch.full((T, 4), 2)}, {})
    acc_h = np.asarray(out["acc/h"])
    assert acc_h.shape == (T,) and np.isnan(acc_h[[0, -1]]).all()
    rel = lambda d, h: d[f"mano.v3d.cam.{h}"] - d[f"mano.j3d.cam.{h}"][:, :1]
    acc = {h: em.compute_error_accel(rel(targets, h), rel(pred, h)).numpy() for h in "rl"}
    d1_gt = 0.05 + 0.02 * torch.sin(torch.arange(T)[:, None, None] / 5.0 + torch.rand(1, 40, 1, generator=g))
    d1_pred = d1_gt + 0.002 * torch.randn(T, 40, 1, generator=g)
    d1 = em.compute_error_accel(d1_gt, d1_pred).numpy()

    # the reference's own error: its fp32 results against the fp64 restatement on the same inputs
    f64 = AR.evaluate_accel(pred, targets)
    full = AR.evaluate_accel(pred, AR.all_valid(targets))
    pairs = [(acc_h, f64["acc/h"]), (acc["r"], full["acc/r"][1:-1]), (acc["l"], full["acc/l"][1:-1]),
             (d1, AR.accel_error(d1_gt, d1_pred)[1:-1])]
    dev = 0.0
    for got, ref in pairs:
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        m = ~np.isnan(ref)
        dev = max(dev, float((np.abs(got[m].astype(np.float64) - ref[m]) / np.abs(ref[m])).max()))

    rec = {"in/" + k: v.numpy() for k, v in {**{"pred." + k: v for k, v in pred.items()},
                                             **{"targets." + k: v for k, v in targets.items()}}.items()}
    rec.update({"out/acc/h": acc_h, "out/acc_r": acc["r"], "out/acc_l": acc["l"],
                "d1/gt": d1_gt.numpy(), "d1/pred": d1_pred.numpy(), "d1/out": d1})
    rec["meta"] = np.array(json.dumps(dict(META, what="eval_modules.py eval_acc_pose (acc/h) and compute_error_accel, fps 30",
                                           ref_vs_f64_max_rel=dev)))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_acc_pose.npz"), **rec)
    print("acc/h", acc_h)
    print("ref_vs_f64_max_rel", dev)


if __name__ == "__main__":
    main()
