"""MANO fitting on device (csrc/fit.hip): a Levenberg-Marquardt fit of MANO -- the 16 rotations of the full pose, the shape and a
translation -- to 21 3-D joints per hand, the inverse of the forward kinematics everything else here runs.  It turns a
keypoint-only annotation (``mano.j3d.full.{r,l}``) into MANO parameters, so that the mesh, surface, penetration and temporal
metrics, the overlays and the pose and shape terms of the loss have a ground-truth mesh that belongs to the annotation.

The reference has no fitter: DESIGN.md section 7 "MANO fitting" is the specification and tests/fit_ref.py its fp64 restatement.
The fit reproduces the JOINTS.  It does not recover a unique mesh: with joints alone, the twist of a finger segment about its
own bone is observed only through the tips and the pose prior.  One launch fits both hands of a batch, one workgroup a hand;
nothing here synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import FitCfg, ManoFitConsts, ManoFitSide, check, ptr
from .packing import pack_mano
from .xdict import xdict

_CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs", "tip_lbs_weights", "tip_posedirs")


@dataclass(frozen=True)
class FitConfig:
    """``iters`` Levenberg-Marquardt iterations (exactly that many: no data-dependent exit), the weights ``lambda_beta`` and
    ``lambda_pose`` of the priors ``|beta|^2`` and ``|Log(M_j^T R_j)|^2`` (towards the mean pose), and the first damping ``mu0``.

    The defaults (30, 1e-6, 1e-6, 1e-3) are starting values and NOT tuned on data.  On the 16 cases of the tests
    (``fit_ref.FULL_SEEDS``: joints the synthetic right asset generates itself -- global rotation 2 randn, fingers hands_mean +
    0.5 randn, beta = randn, rounded to fp32) the fp64 restatement reaches an rmse of 9.4e-5 to 4.2e-4 m, median 1.6e-4 m -- the
    priors set that floor."""
    iters: int = 30
    lambda_beta: float = 1e-6
    lambda_pose: float = 1e-6
    mu0: float = 1e-3

    def c_struct(self) -> FitCfg:
        if int(self.iters) != self.iters or self.iters < 0:
            raise ValueError(f"hands_amd: iters is a non-negative integer, got {self.iters!r}")
        for name in ("lambda_beta", "lambda_pose", "mu0"):
            v = float(getattr(self, name))
            if not (v >= 0.0 and v != float("inf")):
                raise ValueError(f"hands_amd: {name} is finite and not negative, got {v!r}")
        return FitCfg(int(self.iters), float(self.lambda_beta), float(self.lambda_pose), float(self.mu0))


def _device_of(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError(f"hands_amd.{what} runs on a HIP device only (no CPU fallback)")
    return t.device


def _mano_pack(model_or_layer, side, dev):
    """The packed constants of one hand: from a model (``packed(dev)``), a ``MANOHead`` or a ``ManoLayer`` (packed once per
    device and kept on the layer)."""
    if side not in ("r", "l"):
        raise ValueError(f"hands_amd: side is 'r' or 'l', got {side!r}")
    if hasattr(model_or_layer, "packed"):
        return model_or_layer.packed(dev)[f"mano_{side}"]
    layer = getattr(model_or_layer, "mano", model_or_layer)
    kept = layer.__dict__.get("_fit_pack")
    if kept is None or kept[0] != dev:
        kept = (dev, pack_mano(layer.asset(), dev))
        layer.__dict__["_fit_pack"] = kept
    return kept[1]


def _opt(v, shape, dev, what):
    """An optional input as a contiguous fp32 tensor: it has to be on the device already (nothing here copies from the host)."""
    if v is None:
        return None
    if _device_of(v, f"fit_mano ({what})") != dev:
        raise RuntimeError(f"hands_amd: {what} is on {v.device}, the joints on {dev}")
    v = v.to(dtype=torch.float32).contiguous()
    if tuple(v.shape) != shape:
        raise ValueError(f"hands_amd: {what} has shape {shape}, got {tuple(v.shape)}")
    return v


def _launch(packs, joints, weights, valids, inits, config, dev):
    """One hands_mano_fit_f32 launch over len(packs) sides of B rows; -> per side (pose, beta, transl, rmse, steps)."""
    n, B = len(packs), joints[0].shape[0]
    sides, outs, keep = (ManoFitSide * n)(), [], []
    for i in range(n):
        j = _opt(joints[i], (B, 21, 3), dev, "joints")
        w, v = _opt(weights[i], (B, 21), dev, "weights"), _opt(valids[i], (B,), dev, "valid")
        init = (None, None, None)
        if inits[i] is not None:
            init = tuple(_opt(a, s, dev, "init " + k) for a, s, k in zip(inits[i], ((B, 16, 3, 3), (B, 10), (B, 3)),
                                                                         ("pose", "beta", "transl")))
            if any(a is None for a in init):
                raise ValueError("hands_amd: init is (pose (B,16,3,3), beta (B,10), transl (B,3)), all three")
        o = (torch.empty(B, 16, 3, 3, device=dev), torch.empty(B, 10, device=dev), torch.empty(B, 3, device=dev),
             torch.empty(B, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        consts = ManoFitConsts(*[ptr(packs[i][k]) for k in _CONST_KEYS])
        sides[i] = ManoFitSide(consts, ptr(j), ptr(w), ptr(v), ptr(init[0]), ptr(init[1]), ptr(init[2]), *[ptr(t) for t in o])
        outs.append(o)
        keep.append((j, w, v, init))           # converted copies stay alive until the launch is queued
    cfg = (config or FitConfig()).c_struct()
    check(_lib.lib().hands_mano_fit_f32(sides, n, C.byref(cfg), B, torch.cuda.current_stream(dev).cuda_stream), "hands_mano_fit_f32")
    return outs


def _result(pack, out):
    """pose, beta, transl, rmse, steps and pose_aa (B,48) = [Log R_0, Log R_j - hands_mean_j], the axis-angle form
    HandsWrapper.process_data and the reference's targets use."""
    pose = out[0]
    aa = torch.empty(pose.shape[0], 48, device=pose.device)
    check(_lib.lib().hands_matrix_to_axis_angle_f32(ptr(pose), ptr(aa), pose.shape[0] * 16,
                                                    torch.cuda.current_stream(pose.device).cuda_stream), "matrix_to_axis_angle")
    return xdict({"pose": pose, "beta": out[1], "transl": out[2], "rmse": out[3], "steps": out[4],
                  "pose_aa": aa - pack["pose_mean"]})


def fit_mano(joints, model_or_layer, side="r", weights=None, valid=None, init=None, config=None) -> xdict:
    """Fit ONE hand of a batch: ``joints`` (B,21,3) in metres, in this package's joint order (16 + the five tips), on the device, as every
    other tensor argument has to be (RuntimeError otherwise).  ``model_or_layer``: a model (HandsLight, HAMER, HandOccNet), a ``MANOHead`` or a ``ManoLayer``.  ``weights`` (B,21) >= 0
    (default 1; a joint of weight 0 is never read and may be NaN), ``valid`` (B) (a row with 0 is not fitted), ``init``
    (pose (B,16,3,3), beta (B,10), transl (B,3)) instead of the rest pose aligned rigidly to the joints, ``config`` a
    :class:`FitConfig` (its defaults are untuned starting values).

    Returns an xdict: ``pose`` (B,16,3,3) rotations of the FULL pose, pose_mean included (a prediction's ``mano.pose.{r,l}`` is
    the rotation BEFORE the MANO head adds pose_mean to its axis-angle: hand ``pose_aa`` on, not ``pose``), ``beta`` (B,10),
    ``transl`` (B,3) -- the model's joints plus ``transl`` approximate ``joints`` --, ``rmse`` (B) in metres without the priors, ``steps`` (B) int32 accepted steps and ``pose_aa`` (B,48).  A row that is not fitted (``valid`` 0, fewer
    than four weighted joints, a non-finite weighted joint or initial value) has the mean pose, zeros, ``rmse`` NaN, 0 steps."""
    dev = _device_of(joints, "fit_mano")
    pack = _mano_pack(model_or_layer, side, dev)
    return _result(pack, _launch([pack], [joints], [weights], [valid], [init], config, dev)[0])


def fit_mano_hands(joints_r, joints_l, model, weights_r=None, weights_l=None, valid_r=None, valid_l=None, init_r=None,
                   init_l=None, config=None):
    """Both hands of a batch in ONE launch: -> (right, left), each what :func:`fit_mano` returns."""
    dev = _device_of(joints_r, "fit_mano_hands")
    packs = [_mano_pack(model, "r", dev), _mano_pack(model, "l", dev)]
    outs = _launch(packs, [joints_r, joints_l], [weights_r, weights_l], [valid_r, valid_l], [init_r, init_l], config, dev)
    return _result(packs[0], outs[0]), _result(packs[1], outs[1])


def fit_targets(targets, model, meta_info=None, config=None) -> xdict:
    """Ground-truth MANO parameters for a keypoint-only batch: fits both hands to ``targets["mano.j3d.full.{r,l}"]`` (camera
    space, metres, on the device) in one launch and returns a NEW xdict with the entries of ``targets`` in which
    ``mano.pose.{r,l}`` (B,48) axis-angle and ``mano.beta.{r,l}`` (B,10) are the fit -- the two keys
    ``HandsWrapper.process_data`` builds the ground-truth mesh from -- and ``mano.fit.rmse.{r,l}`` (B) and
    ``mano.fit.transl.{r,l}`` (B,3) are added; ``targets`` itself is left as it was.  ``meta_info["right_valid"]`` /
    ``["left_valid"]`` (B, on the device), where present, say which rows are fitted."""
    dev = _device_of(targets["mano.j3d.full.r"], "fit_targets")
    flag = lambda k: meta_info[k] if meta_info is not None and k in meta_info else None
    fits = fit_mano_hands(targets["mano.j3d.full.r"], targets["mano.j3d.full.l"], model, valid_r=flag("right_valid"),
                          valid_l=flag("left_valid"), config=config)
    out = xdict(targets)
    for h, f in zip("rl", fits):
        out.overwrite(f"mano.pose.{h}", f["pose_aa"])
        out.overwrite(f"mano.beta.{h}", f["beta"])
        out.overwrite(f"mano.fit.rmse.{h}", f["rmse"])
        out.overwrite(f"mano.fit.transl.{h}", f["transl"])
    return out
