"""Evaluation metrics on device: the consumer of the gathered predictions.

``evaluate_metrics(pred, targets)`` mirrors the reference's metric functions for the `*_light`
models -- ``eval_mpjpe_ra``, ``eval_mpjpe_pa_ra`` (21-joint branch), ``eval_mrrpe_hand``,
``eval_pixel_error`` (src/utils/eval_modules.py:97-134,221-343,386-428) -- with one kernel launch for
the whole batch instead of a per-sample numpy loop with a LAPACK SVD per hand.  Same keys, same units
(mm / px), same NaN conventions; tensors stay on the device.  With ``'egoexo' in meta_info['dataset']`` the reference
takes the other branch of ``eval_mpjpe_pa_ra`` (:231-317, joints flagged in ``joints3d_valid_{r,l}`` only) and so does this.

``evaluate_mesh_metrics(pred, targets)`` adds what mesh papers report and the reference does not compute: MPVPE, F@5mm /
F@15mm and the AUC of the PCK curve, root-aligned and Procrustes-aligned, for the 778 vertices of each hand.

``evaluate_surface_metrics(pred, targets, faces=...)`` measures to the triangle surface instead of the vertices: the
point-to-surface error scan-based benchmarks report, and the Chamfer distance, under the same two alignments.

``evaluate_penetration_metrics(pred, targets, faces=...)`` scores the prediction alone: how deep, with how many vertices and
-- on request -- with what volume the two predicted hands pass through each other (hands_amd/penetration.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import EvalIn, EvalMaskedOut, EvalOut, MeshEvalIn, MeshEvalOut, SurfEvalOut, check, ptr
from .xdict import xdict

# keys of evaluate_mesh_metrics without the hand suffix, in the order of hands_mesh_eval_out (_lib.MESH_QUANTITIES)
MESH_KEYS = tuple(k.format(a) for a in ("ra", "pa")
                  for k in ("mpvpe/{}", "fscore/{}/5", "fscore/{}/15", "auc/{}/v", "auc/{}/j"))
MASKED_KEYS = ("mpjpe/pa/rao", "mpjpe/pa/abs", "mpjpe/pa/ra")
# keys of evaluate_surface_metrics without the hand suffix, in the order of hands_surf_eval_out (_lib.SURF_QUANTITIES)
SURF_KEYS = tuple(f"{q}/{a}" for q in ("p2s", "chamfer") for a in ("ra", "pa"))


def _is_egoexo(meta_info) -> bool:
    """The reference's own test (src/utils/eval_modules.py:231): ``'egoexo' in meta_info['dataset']``."""
    if meta_info is None:
        return False
    try:
        dataset = meta_info["dataset"]
    except KeyError:
        return False
    return "egoexo" in dataset


def evaluate_metrics(pred: dict, targets: dict, meta_info: dict | None = None) -> xdict:
    L = _lib.lib()
    dev = pred["mano.j3d.cam.r"].device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.evaluate_metrics runs on a HIP device only (no CPU fallback)")
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    B = pred["mano.j3d.cam.r"].shape[0]
    keep = [f(pred["mano.j3d.cam.r"]), f(pred["mano.j3d.cam.l"]), f(targets["mano.j3d.cam.r"]), f(targets["mano.j3d.cam.l"]),
            f(pred["mano.j2d.r"]), f(pred["mano.j2d.l"]), f(targets["mano.j2d.r"]), f(targets["mano.j2d.l"]),
            f(targets["is_valid"]), f(targets["right_valid"]), f(targets["left_valid"]),
            f(targets["joints_valid_r"]), f(targets["joints_valid_l"])]
    assert keep[0].shape == (B, 21, 3) and keep[4].shape == (B, 21, 2) and keep[11].shape == (B, 21)
    o = {k: torch.empty(B, device=dev) for k in ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l")}
    o["pix_err/r"], o["pix_err/l"] = torch.empty(B, 21, device=dev), torch.empty(B, 21, device=dev)
    ein = EvalIn(*[ptr(t) for t in keep])
    eout = EvalOut(ptr(o["mpjpe/ra/h"]), ptr(o["mpjpe/pa/ra/r"]), ptr(o["mpjpe/pa/ra/l"]), ptr(o["mpjpe/pa/ra/h"]),
                   ptr(o["mrrpe/r/l"]), ptr(o["pix_err/r"]), ptr(o["pix_err/l"]))
    stream = torch.cuda.current_stream(dev).cuda_stream
    check(L.hands_eval_metrics_f32(C.byref(ein), C.byref(eout), B, stream), "hands_eval_metrics_f32")
    if _is_egoexo(meta_info):
        # the other branch of eval_mpjpe_pa_ra (eval_modules.py:231-317): its nine keys replace the three mpjpe/pa/ra/*
        jv3d = [f(targets["joints3d_valid_r"]), f(targets["joints3d_valid_l"])]
        assert jv3d[0].shape == (B, 21) and jv3d[1].shape == (B, 21)
        for k in MASKED_KEYS:
            for s in "rlh":
                o[f"{k}/{s}"] = torch.empty(B, device=dev)
        mout = EvalMaskedOut(*[ptr(o[f"{k}/{s}"]) for k in MASKED_KEYS for s in "rlh"])
        check(L.hands_eval_metrics_masked_f32(C.byref(ein), ptr(jv3d[0]), ptr(jv3d[1]), C.byref(mout), B, stream),
              "hands_eval_metrics_masked_f32")
    out = xdict(o)
    out["pix_err/h"] = torch.cat((o["pix_err/r"], o["pix_err/l"]), dim=1)
    return out


def evaluate_mesh_metrics(pred: dict, targets: dict, meta_info: dict | None = None) -> xdict:
    """Mesh metrics of both hands in one launch (hands_eval_mesh_metrics_f32): ``mpvpe/{ra,pa}/*`` (mm),
    ``fscore/{ra,pa}/{5,15}/*``, ``auc/{ra,pa}/{v,j}/*`` for ``* = r, l, h``, each a (B) tensor on the device of the inputs.
    Needs ``mano.v3d.cam.{r,l}`` (B,V,3) and ``mano.j3d.cam.{r,l}`` (B,21,3) in ``pred`` and ``targets`` and
    ``is_valid`` / ``right_valid`` / ``left_valid`` (B) in ``targets``.  Invalid hands are NaN, as ``mpjpe/ra``."""
    dev = pred["mano.v3d.cam.r"].device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.evaluate_mesh_metrics runs on a HIP device only (no CPU fallback)")
    L = _lib.lib()
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    B, V = pred["mano.v3d.cam.r"].shape[:2]
    keep = [f(pred["mano.v3d.cam.r"]), f(pred["mano.v3d.cam.l"]), f(targets["mano.v3d.cam.r"]), f(targets["mano.v3d.cam.l"]),
            f(pred["mano.j3d.cam.r"]), f(pred["mano.j3d.cam.l"]), f(targets["mano.j3d.cam.r"]), f(targets["mano.j3d.cam.l"]),
            f(targets["is_valid"]), f(targets["right_valid"]), f(targets["left_valid"])]
    assert all(t.shape == (B, V, 3) for t in keep[:4]) and all(t.shape == (B, 21, 3) for t in keep[4:8])
    assert all(t.shape == (B,) for t in keep[8:])
    buf = torch.empty(len(MESH_KEYS) * 3, B, device=dev)
    mout = MeshEvalOut(*[ptr(buf[i]) for i in range(buf.shape[0])])
    check(L.hands_eval_mesh_metrics_f32(C.byref(MeshEvalIn(*[ptr(t) for t in keep])), C.byref(mout), B, V,
                                        torch.cuda.current_stream(dev).cuda_stream), "hands_eval_mesh_metrics_f32")
    return xdict({f"{k}/{s}": buf[3 * i + j] for i, k in enumerate(MESH_KEYS) for j, s in enumerate("rlh")})


def faces_on_device(faces, dev) -> torch.Tensor:
    """A face list (tensor or numpy array of any integer type, (F,3)) as a contiguous int32 tensor on ``dev``."""
    t = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    if t.is_floating_point() or t.dtype == torch.bool or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"hands_amd: a face list is an (F, 3) integer array, got {tuple(t.shape)} {t.dtype}")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def evaluate_surface_metrics(pred: dict, targets: dict, meta_info: dict | None = None, faces=None) -> xdict:
    """Point-to-surface error and Chamfer distance of both hands (hands_eval_surface_metrics_f32, two launches):
    ``p2s/{ra,pa}/*`` and ``chamfer/{ra,pa}/*`` for ``* = r, l, h``, millimetres, each a (B) tensor on the device of the inputs.
    With X the aligned prediction, Y the ground truth and T the faces of the hand,
    ``p2s = 1000 * 1/2 [mean_i d(X_i, surface(Y,T)) + mean_j d(Y_j, surface(X,T))]`` and
    ``chamfer = 1000 * 1/2 [mean_i min_j |X_i - Y_j| + mean_j min_i |Y_j - X_i|]``; alignments, inputs and NaN rules are those of
    :func:`evaluate_mesh_metrics`.  The face lists come from ``faces=(faces_r, faces_l)`` or from
    ``meta_info["mano.faces.{r,l}"]``."""
    dev = pred["mano.v3d.cam.r"].device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.evaluate_surface_metrics runs on a HIP device only (no CPU fallback)")
    if faces is None:
        if meta_info is None or "mano.faces.r" not in meta_info or "mano.faces.l" not in meta_info:
            raise ValueError("hands_amd.evaluate_surface_metrics needs faces=(faces_r, faces_l) or meta_info['mano.faces.{r,l}']")
        faces = (meta_info["mano.faces.r"], meta_info["mano.faces.l"])
    L = _lib.lib()
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    B, V = pred["mano.v3d.cam.r"].shape[:2]
    keep = [f(pred["mano.v3d.cam.r"]), f(pred["mano.v3d.cam.l"]), f(targets["mano.v3d.cam.r"]), f(targets["mano.v3d.cam.l"]),
            f(pred["mano.j3d.cam.r"]), f(pred["mano.j3d.cam.l"]), f(targets["mano.j3d.cam.r"]), f(targets["mano.j3d.cam.l"]),
            f(targets["is_valid"]), f(targets["right_valid"]), f(targets["left_valid"])]
    assert all(t.shape == (B, V, 3) for t in keep[:4]) and all(t.shape == (B, 21, 3) for t in keep[4:8])
    assert all(t.shape == (B,) for t in keep[8:])
    fr, fl = (faces_on_device(x, dev) for x in faces)
    buf = torch.empty(len(SURF_KEYS) * 3, B, device=dev)
    sout = SurfEvalOut(*[ptr(buf[i]) for i in range(buf.shape[0])])
    check(L.hands_eval_surface_metrics_f32(C.byref(MeshEvalIn(*[ptr(t) for t in keep])), ptr(fr) or None, ptr(fl) or None,
                                           fr.shape[0], fl.shape[0], C.byref(sout), B, V,
                                           torch.cuda.current_stream(dev).cuda_stream), "hands_eval_surface_metrics_f32")
    return xdict({f"{k}/{s}": buf[3 * i + j] for i, k in enumerate(SURF_KEYS) for j, s in enumerate("rlh")})


PEN_KEYS = ("pen/depth", "pen/count")


def evaluate_penetration_metrics(pred: dict, targets: dict, meta_info: dict | None = None, faces=None, seal=True,
                                 volume_grid=0) -> xdict:
    """How far the two PREDICTED hands pass through each other (hands_mesh_signed_f32, two launches; the ground truth gives
    the validity flags only): ``pen/depth/*`` the deepest vertex below the other hand's surface in millimetres and
    ``pen/count/*`` the number of vertices inside it, for ``* = r`` (the right hand's vertices in the left hand), ``l`` and
    ``h``, the larger of the two; with ``volume_grid = G > 0`` also ``pen/volume/h``, the volume both hands occupy in cubic
    centimetres on a ``G^3`` grid (:func:`hands_amd.intersection_volume`, two more launches).  Each a (B) fp32 tensor on the
    device of the inputs; a sample with ``is_valid * right_valid * left_valid == 0`` is NaN, as is one with a non-finite vertex.
    ``seal`` closes each hand's open boundary first (:func:`hands_amd.seal_mesh`).  The face lists come from
    ``faces=(faces_r, faces_l)`` or from ``meta_info["mano.faces.{r,l}"]``."""
    from .penetration import interhand_penetration, intersection_volume
    dev = pred["mano.v3d.cam.r"].device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.evaluate_penetration_metrics runs on a HIP device only (no CPU fallback)")
    if faces is None:
        if meta_info is None or "mano.faces.r" not in meta_info or "mano.faces.l" not in meta_info:
            raise ValueError("hands_amd.evaluate_penetration_metrics needs faces=(faces_r, faces_l) or meta_info['mano.faces.{r,l}']")
        faces = (meta_info["mano.faces.r"], meta_info["mano.faces.l"])
    d = {"mano.v3d.cam.r": pred["mano.v3d.cam.r"], "mano.v3d.cam.l": pred["mano.v3d.cam.l"]}
    for k in ("is_valid", "right_valid", "left_valid"):
        d[k] = targets[k].to(dev)
    pen = interhand_penetration(d, faces=faces, seal=seal)
    nan = torch.isnan(pen["pen.depth.rl"]) | torch.isnan(pen["pen.depth.lr"])        # not valid, or a non-finite vertex
    out = xdict()
    for key, name, scale in (("pen/depth", "pen.depth", 1000.0), ("pen/count", "pen.count", 1.0)):
        r, l = (torch.where(nan, torch.full_like(nan, float("nan"), dtype=torch.float32), pen[f"{name}.{k}"].float() * scale)
                for k in ("rl", "lr"))
        out[key + "/r"], out[key + "/l"], out[key + "/h"] = r, l, torch.maximum(r, l)
    if volume_grid:
        vol = intersection_volume(d, faces=faces, seal=seal, G=int(volume_grid)) * 1e6
        out["pen/volume/h"] = torch.where(nan, torch.full_like(vol, float("nan")), vol)
    return out
