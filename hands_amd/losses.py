"""The reference's validation loss dict on device (csrc/loss.hip), forward only.

``compute_loss_light(pred, gt, meta_info, args)`` mirrors ``compute_loss_light`` of the reference
(src/callbacks/loss/loss_arctic_sf.py:20-206): same signature, same keys in the same order, values ``(tensor of shape (1,),
weight)``.  ``mul_loss_dict`` / ``total_loss`` are the weighting and the total of ``GenericWrapper.forward``
(src/models/generic/wrapper.py:19-23,100-115) and ``epoch_end`` is the aggregation that turns the per-step records into
``loss__val`` (common/pl_utils.py:46-63, common/abstract_pl.py:134-142) -- the number the reference selects checkpoints by.

One evaluation is two kernel launches on the current stream whatever switches are on, with no host synchronisation (the
reference's ``is_valid.sum() == 0`` branches are a select on the device), so it can be captured into a graph.  Gradients and
train mode are out of scope.  No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LossIn, check, ptr
from .xdict import xdict

BASE_KEYS = ("loss/mano/cam_t/r", "loss/mano/cam_t/l", "loss/mano/kp2d/r", "loss/mano/kp3d/r", "loss/mano/pose/r",
             "loss/mano/beta/r", "loss/mano/kp2d/l", "loss/mano/kp3d/l", "loss/mano/pose/l", "loss/mano/transl/l",
             "loss/mano/beta/l")
# the kernel's output order (HANDS_LOSS_NKEYS) and the reference's weights
LOSS_KEYS = BASE_KEYS + ("loss/grasp/r", "loss/grasp/l", "loss/mask/r", "loss/mask/l", "loss/depth/r", "loss/depth/l",
                         "loss/center/r", "loss/center/l", "loss/corner/r", "loss/corner/l")
LOSS_WEIGHTS = (1.0, 1.0, 5.0, 5.0, 10.0, 0.001, 5.0, 5.0, 10.0, 1.0, 0.001, 0.1, 0.1, 10.0, 10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0)
assert len(LOSS_KEYS) == len(LOSS_WEIGHTS) == _lib.LOSS_NKEYS


class LossDict(dict):
    """The dict ``compute_loss_light`` returns; it keeps the kernel's weighted values and total for ``mul_loss_dict`` /
    ``total_loss``."""
    weighted = None     # (21,) fp32 on the device, kernel order
    total = None        # (1,)


def _get(args, k, d=None):
    return args.get(k, d) if hasattr(args, "get") else getattr(args, k, d)


def loss_keys(args):
    """The keys ``compute_loss_light`` returns for ``args``, in order."""
    keys = list(BASE_KEYS)
    for switch, name in (("use_grasp_loss", "grasp"), ("use_render_seg_loss", "mask"), ("use_depth_loss", "depth")):
        if _get(args, switch, False):
            keys += [f"loss/{name}/r", f"loss/{name}/l"]
    if _get(args, "regress_center_corner", False):
        keys += ["loss/center/r", "loss/center/l", "loss/corner/r", "loss/corner/l"]
    return keys


def _square_side(t, B, what):
    n = t.numel() // B
    S = int(round(n ** 0.5))
    if t.shape[0] != B or S * S != n or t.shape[-1] != S:
        raise ValueError(f"compute_loss_light: {what} must hold one S x S map per sample, got {tuple(t.shape)}")
    return S


def bind_loss_inputs(pred, gt, meta_info, args):
    """-> (hands_loss_in, the fp32 / contiguous tensors it points to, device, B, S_mask, S_depth)."""
    head = pred["mano.beta.r"]
    if not (torch.is_tensor(head) and head.device.type == "cuda"):
        raise RuntimeError("hands_amd.compute_loss_light runs on a HIP device only (no CPU fallback)")
    dev = head.device
    B = head.shape[0]
    keep = []                                   # keeps the converted tensors alive until the launches are enqueued

    def f32(t, shape):
        t = t.detach().to(device=dev, dtype=torch.float32).contiguous()
        if t.numel() != B * int(np.prod(shape)):
            raise ValueError(f"compute_loss_light: expected {(B,) + tuple(shape)}, got {tuple(t.shape)}")
        keep.append(t)
        return ptr(t)

    a = LossIn()
    for h in "rl":
        for field, src, key, shape in (
                ("pred_pose", pred, "mano.pose", (16, 3, 3)), ("pred_beta", pred, "mano.beta", (10,)),
                ("pred_j3d", pred, "mano.j3d.cam", (21, 3)), ("pred_j2d", pred, "mano.j2d.norm", (21, 2)),
                ("pred_cam_wp", pred, "mano.cam_t.wp", (3,)), ("pred_cam_wp_init", pred, "mano.cam_t.wp.init", (3,)),
                ("gt_pose", gt, "mano.pose", (48,)), ("gt_beta", gt, "mano.beta", (10,)), ("gt_j3d", gt, "mano.j3d.cam", (21, 3)),
                ("gt_j2d", gt, "mano.j2d.norm", (21, 2)), ("gt_cam_wp", gt, "mano.cam_t.wp", (3,))):
            setattr(a, f"{field}_{h}", f32(src[f"{key}.{h}"], shape))
        setattr(a, f"joints_valid_{h}", f32(gt[f"joints_valid_{h}"], (21,)))
    a.right_valid, a.left_valid = f32(gt["right_valid"], ()), f32(gt["left_valid"], ())
    for k in ("cam", "j2d", "j3d", "pose", "beta"):
        setattr(a, f"is_{k}_loss", f32(meta_info[f"is_{k}_loss"], ()))
    S_mask = S_depth = 0
    if _get(args, "use_grasp_loss", False):
        for h in "rl":
            setattr(a, f"pred_grasp_{h}", f32(pred[f"grasp.{h}"], (9,)))
            lab = gt[f"grasp.{h}"].to(device=dev, dtype=torch.int64).contiguous()
            assert lab.numel() == B
            keep.append(lab)
            setattr(a, f"gt_grasp_{h}", ptr(lab))
            setattr(a, f"grasp_valid_{h}", f32(gt[f"grasp_valid_{h}"], ()))
        a.is_grasp_loss = f32(meta_info["is_grasp_loss"], ())
    if _get(args, "use_render_seg_loss", False):
        S_mask = _square_side(pred["render.r"], B, "render.r")
        for h in "rl":
            setattr(a, f"pred_mask_{h}", f32(pred[f"render.{h}"], (S_mask, S_mask)))
            setattr(a, f"gt_mask_{h}", f32(gt[f"render.{h}"], (S_mask, S_mask)))
            setattr(a, f"render_valid_{h}", f32(gt[f"render_valid_{h}"], ()))
        a.is_mask_loss = f32(meta_info["is_mask_loss"], ())
    if _get(args, "use_depth_loss", False):
        S_depth = _square_side(pred["depth.r"], B, "depth.r")
        for h in "rl":
            setattr(a, f"pred_depth_{h}", f32(pred[f"depth.{h}"], (S_depth, S_depth)))
            setattr(a, f"gt_depth_{h}", f32(gt[f"depth.{h}"], (S_depth, S_depth)))
        a.is_depth_loss = f32(meta_info["is_depth_loss"], ())
    if _get(args, "regress_center_corner", False):
        for h in "rl":
            for nm, n in (("center", 2), ("corner", 8)):
                setattr(a, f"pred_{nm}_{h}", f32(pred[f"{nm}.{h}"], (n,)))
                setattr(a, f"gt_{nm}_{h}", f32(gt[f"{nm}.{h}"], (n,)))
    return a, keep, dev, B, S_mask, S_depth


def loss_light_raw(pred, gt, meta_info, args):
    """-> (present keys, out) with out (43,) fp32 on the device: 21 unweighted means, 21 weighted values, the total."""
    L = _lib.lib()
    a, keep, dev, B, S_mask, S_depth = bind_loss_inputs(pred, gt, meta_info, args)
    nbytes = L.hands_loss_workspace_bytes(B, S_mask, S_depth)
    if nbytes <= 0:
        raise ValueError(f"compute_loss_light: bad shape B={B}, S_mask={S_mask}, S_depth={S_depth}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(2 * _lib.LOSS_NKEYS + 1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(L.hands_loss_light_f32(C.byref(a), B, S_mask, S_depth, ptr(ws), ptr(out), ptr(out, _lib.LOSS_NKEYS),
                                     ptr(out, 2 * _lib.LOSS_NKEYS), torch.cuda.current_stream(dev).cuda_stream),
              "hands_loss_light_f32")
    del keep                                    # stream-ordered: the allocator hands them out again after the launches
    return loss_keys(args), out


def compute_loss_light(pred, gt, meta_info, args):
    """{key: (tensor of shape (1,) fp32 on the device, weight)} -- the reference's ``compute_loss_light``."""
    keys, out = loss_light_raw(pred, gt, meta_info, args)
    d = LossDict()
    for k in keys:
        i = LOSS_KEYS.index(k)
        d[k] = (out[i:i + 1], LOSS_WEIGHTS[i])
    d.weighted = out[_lib.LOSS_NKEYS:2 * _lib.LOSS_NKEYS]
    d.total = out[2 * _lib.LOSS_NKEYS:]
    return d


def mul_loss_dict(loss_dict):
    """generic/wrapper.py:19-23,100: every key's weighted value, 0-dim -- read from the kernel's outputs."""
    if not isinstance(loss_dict, LossDict) or loss_dict.weighted is None:
        raise TypeError("hands_amd.mul_loss_dict takes the dict hands_amd.compute_loss_light returned")
    out = LossDict({k: loss_dict.weighted[LOSS_KEYS.index(k)] for k in loss_dict if k != "loss"})
    out.weighted, out.total = loss_dict.weighted, loss_dict.total
    return out


def total_loss(loss_dict):
    """generic/wrapper.py:111-115: adds ``'loss'``, the sum of the weighted values in key order (the kernel's total)."""
    if not isinstance(loss_dict, LossDict) or loss_dict.total is None:
        raise TypeError("hands_amd.total_loss takes the dict hands_amd.mul_loss_dict returned")
    loss_dict["loss"] = loss_dict.total[0]
    return loss_dict


def epoch_end(step_outputs, postfix="__val"):
    """The reference's epoch aggregation over the ``{"out_dict": ..., "loss": ...}`` records of ``inference_step``: every
    ``metric.*`` is the ``np.nanmean`` over all images, every loss key the mean over the steps, all keys postfixed (so the
    result holds ``loss__val``).  Host code."""
    assert isinstance(step_outputs, list) and isinstance(step_outputs[0], dict)
    outs = [s["out_dict"] for s in step_outputs]
    losses = [s["loss"] for s in step_outputs]
    res = {}
    for k in outs[0]:
        if "metric." not in k:
            continue
        v = torch.cat([torch.as_tensor(o[k]).detach().cpu() for o in outs]).numpy()
        res[k] = np.nanmean(np.array(v))
    for k in losses[0]:
        v = torch.cat([torch.as_tensor(l[k]).detach().cpu().view(-1) for l in losses])
        res[k] = v.mean().item()
    return xdict(res).postfix(postfix)
