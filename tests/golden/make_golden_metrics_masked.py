#!/usr/bin/env python3
"""Generate tests/golden/eval_metrics_egoexo.npz with the REAL reference ``eval_mpjpe_pa_ra`` on a batch whose dataset is
'egoexo' (src/utils/eval_modules.py:231-317): only the joints flagged in ``joints3d_valid_{r,l}`` count.  Dev container only.

B = 24 with masks of 0, 1, 2, 3 and 21 flagged joints, masks whose joint 0 is not flagged (the root is then the first flagged
joint) and invalid hands.  The module's import-time NameError is handled as in make_golden_metrics.py.
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


def main():
    g = torch.Generator().manual_seed(23)
    B = 24
    gt_r, gt_l = 0.1 * torch.randn(B, 21, 3, generator=g), 0.1 * torch.randn(B, 21, 3, generator=g)
    gt_r[..., 2] += 0.6
    gt_l[..., 2] += 0.7
    gt_l[..., 0] += 0.2

    def perturb(x, i):
        ang = torch.tensor(0.2 + 0.05 * i)
        Rz = torch.tensor([[torch.cos(ang), -torch.sin(ang), 0], [torch.sin(ang), torch.cos(ang), 0], [0, 0, 1.0]])
        return (1.1 * (x - x.mean(1, keepdim=True)) @ Rz.T) + x.mean(1, keepdim=True) + 0.01 * torch.randn(x.shape, generator=g)
    pr_r, pr_l = perturb(gt_r, 1), perturb(gt_l, 2)
    jv_r = (torch.rand(B, 21, generator=g) > 0.35).float()
    jv_l = (torch.rand(B, 21, generator=g) > 0.35).float()
    # the fixed masks: none, one, two and all 21 joints flagged; joint 0 not flagged
    jv_r[0] = 0
    jv_l[0] = 1
    jv_r[1] = 0
    jv_r[1, 7] = 1
    jv_l[1] = 0
    jv_l[1, 0] = 1
    jv_r[2] = 0
    jv_r[2, [4, 15]] = 1
    jv_l[2] = 0
    jv_r[3] = 1
    jv_l[3] = 1
    jv_r[4:8, 0] = 0
    jv_l[6:10, 0] = 0
    jv_l[5] = 0
    jv_l[5, [0, 20]] = 1
    jv_l[4] = 0
    jv_l[4, [2, 9, 14]] = 1                # two and three joints: the reference reads a 2 x 3 / 3 x 3 array as (dim, points)
    jv_r[12] = 0
    jv_r[12, [0, 5, 6]] = 1
    is_valid = torch.ones(B)
    right_valid = torch.ones(B)
    left_valid = torch.ones(B)
    is_valid[[9, 17]] = 0
    right_valid[[3, 10, 11]] = 0           # row 3: all 21 flagged in an invalid right hand -> 0, not NaN
    left_valid[[2, 11, 12]] = 0            # row 2: no joint flagged in an invalid left hand -> NaN
    pred = {"mano.j3d.cam.r": pr_r, "mano.j3d.cam.l": pr_l}
    targets = {"mano.j3d.cam.r": gt_r, "mano.j3d.cam.l": gt_l, "is_valid": is_valid, "right_valid": right_valid,
               "left_valid": left_valid, "joints3d_valid_r": jv_r, "joints3d_valid_l": jv_l}
    meta_info = {"dataset": ["egoexo"] * B}
    with np.errstate(all="ignore"):
        out = em.eval_mpjpe_pa_ra(pred, targets, meta_info)
    assert set(out) == {f"mpjpe/pa/{k}/{s}" for k in ("rao", "abs", "ra") for s in "rlh"}, sorted(out)
    rec = {"in/" + k: v.numpy() for k, v in {**{"pred." + k: v for k, v in pred.items()},
                                             **{"targets." + k: v for k, v in targets.items()}}.items()}
    rec.update({"out/" + k: np.asarray(v) for k, v in out.items()})
    rec["meta"] = np.array(json.dumps(dict(META, what="eval_modules.py eval_mpjpe_pa_ra, branch 'egoexo' in meta_info['dataset']")))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "eval_metrics_egoexo.npz"), **rec)
    for k, v in out.items():
        print(k, np.asarray(v).shape, np.asarray(v).reshape(-1)[:6])


if __name__ == "__main__":
    main()
