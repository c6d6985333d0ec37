"""MANO fitting on device (csrc/fit.hip): a Levenberg-Marquardt fit of MANO -- the 16 rotations of the full pose, the shape and a
translation -- to 21 3-D joints per hand, the inverse of the forward kinematics everything else here runs.  It turns a
keypoint-only annotation (``mano.j3d.full.{r,l}``) into MANO parameters, so that the mesh, surface, penetration and temporal
metrics, the overlays and the pose and shape terms of the loss have a ground-truth mesh that belongs to the annotation.

The reference has no fitter: DESIGN.md section 7 "MANO fitting" is the specification and tests/fit_ref.py its fp64 restatement.
The fit reproduces the JOINTS.  It does not recover a unique mesh: with joints alone, the twist of a finger segment about its
own bone is observed only through the tips and the pose prior.  One launch fits both hands of a batch, one workgroup a hand;
nothing here synchronises with the host.

The ``*_2d`` functions fit the same unknowns to 21 2-D keypoints in pixels under the perspective projection of the intrinsics
(hands_mano_fit2d_f32; DESIGN.md section 7 "MANO fitting to 2-D keypoints", tests/fit2d_ref.py): for 2-D-only annotations
(``fit_targets_2d``, ``HandsWrapper.fit_gt_2d``) and for moving a prediction onto detected keypoints (``refine_predictions``).
That fit reproduces the KEYPOINTS.  It does not recover depth, scale or a unique 3-D hand from one view.

The ``*_verts`` functions fit the same unknowns to the 778 vertices of a mesh in MANO topology (hands_mano_fit_verts_f32,
csrc/fit_verts.hip; DESIGN.md section 7 "MANO fitting to 778 vertices", tests/fit_verts_ref.py): for mesh-only annotations
(``fit_targets_verts``, ``HandsWrapper.fit_gt_verts``) and for turning any MANO-topology mesh into ``mano.pose`` /
``mano.beta``.  That fit reproduces the VERTICES: where the mesh is a MANO mesh it recovers pose and shape.  It does no
correspondence-free registration (vertex n of the target is vertex n of the model) and fits no scale.

``fit_mano_surface`` fits the same unknowns to P points whose places ON the model's surface are named: row k is a face of the
asset's face list and three coefficients (hands_mano_fit_surf_f32, csrc/fit_surf.hip; DESIGN.md section 7 "MANO fitting to
surface correspondences and ICP registration", tests/fit_surf_ref.py) -- mocap markers at known places, or the correspondences
of one ICP round.  ``correspond_on_mesh`` (hands_mesh_correspond_f32) derives such rows from a point cloud and a posed mesh, and
``register_mano`` alternates the two: data-to-model ICP from a caller's initial state.  That loop lowers the cloud's distance
to the surface; it is local, fits no scale, and observes no twist of a round finger.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import (Fit2DCfg, FitCfg, FitSurfCfg, ManoFit2DSide, ManoFitConsts, ManoFitSide, ManoFitSurfConsts, ManoFitSurfSide,
                   ManoFitVertsConsts, ManoFitVertsSide, check, ptr)
from .metrics import faces_on_device
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
    priors set that floor.

    The fit to 778 vertices (``fit_mano_verts``) takes the same four numbers.  There the restatement
    (``fit_verts_ref.family_case``, both synthetic assets, 16 fully weighted cases) takes 5 or 6 real steps, reaches an rmse of
    at most 9.5e-7 m and recovers the rotations to 1.8e-5 rad, beta to 8.6e-5 and the translation to 4.6e-7 m: on a fully
    weighted, noise-free mesh the iterations after about the sixth change nothing and cost time.  Sparse targets (20 of the
    778 vertices weighted) are what need the thirty: they take 15 to 30 iterations with rejections on the way.  Once the cost
    has stalled, an accept / reject decision is a tie at rounding level (|c' - c| <= 4e-16 c, often exactly 0), so ``steps``
    past convergence carries no information; there is no stall rule and no tolerance in the accept test."""
    iters: int = 30
    lambda_beta: float = 1e-6
    lambda_pose: float = 1e-6
    mu0: float = 1e-3

    def c_struct(self) -> FitCfg:
        _check_config(self, ("iters",), ("lambda_beta", "lambda_pose", "mu0"))
        return FitCfg(int(self.iters), float(self.lambda_beta), float(self.lambda_pose), float(self.mu0))


def _check_config(config, counts, reals):
    """ValueError unless the fields ``counts`` are non-negative integers and the fields ``reals`` finite and not negative."""
    for name in counts:
        v = getattr(config, name)
        if int(v) != v or v < 0:
            raise ValueError(f"hands_amd: {name} is a non-negative integer, got {v!r}")
    for name in reals:
        v = float(getattr(config, name))
        if not (v >= 0.0 and v != float("inf")):
            raise ValueError(f"hands_amd: {name} is finite and not negative, got {v!r}")


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


def _opt(v, shape, dev, what, dtype=torch.float32):
    """An optional input as a contiguous fp32 (or ``dtype``) tensor: it has to be on the device already (nothing here copies
    from the host)."""
    if v is None:
        return None
    if _device_of(v, f"fit_mano ({what})") != dev:
        raise RuntimeError(f"hands_amd: {what} is on {v.device}, the joints on {dev}")
    v = v.to(dtype=dtype).contiguous()
    if tuple(v.shape) != shape:
        raise ValueError(f"hands_amd: {what} has shape {shape}, got {tuple(v.shape)}")
    return v


_Fit = namedtuple("_Fit", "entry side consts const_keys data data_shape n_weights extras config shared more", defaults=((), ()))
"""What tells one fit from another on the way to its C entry: the entry's name, the ctypes side and consts structs, the keys of
the pack the consts are, name and per-row shape of the data tensor, the number of weights of a row, the outputs behind pose,
beta, transl, rmse and steps as (name, per-row shape, dtype), the configuration class, the tensors the entry takes once for
all sides as (name, per-row shape), and the data tensors a side takes beside the first, behind its outputs, as (name, per-row
shape, dtype, required).  ``n_weights`` -1: the rows of a hand are as many as the data tensor has (a -1 in a shape stands for
that number), and the entry takes the number behind B."""

_OUTPUTS = (("pose", (16, 3, 3), torch.float32), ("beta", (10,), torch.float32), ("transl", (3,), torch.float32),
            ("rmse", (), torch.float32), ("steps", (), torch.int32))
_FIT_JOINTS = _Fit("hands_mano_fit_f32", ManoFitSide, ManoFitConsts, _CONST_KEYS, "joints", (21, 3), 21, (), FitConfig)


def _launch(fit, packs, data, weights, valids, inits, cfg, dev, shared=(), more=None):
    """One launch of ``fit.entry`` over len(packs) sides of B rows; -> per side the outputs, _OUTPUTS then ``fit.extras``."""
    n, B = len(packs), data[0].shape[0]
    rows = fit.n_weights if fit.n_weights >= 0 else (int(data[0].shape[1]) if data[0].dim() > 1 else 0)
    dims = lambda s: tuple(rows if d < 0 else d for d in s)
    if fit.n_weights < 0 and not 1 <= rows <= MAX_SURFACE_ROWS:
        raise ValueError(f"hands_amd: {fit.data} has 1 to {MAX_SURFACE_ROWS} rows per hand, got {rows}")
    shared = [_opt(t, (B,) + s, dev, k) for t, (k, s) in zip(shared, fit.shared)]
    sides, outs, keep = (fit.side * n)(), [], []
    for i in range(n):
        y = _opt(data[i], (B,) + dims(fit.data_shape), dev, fit.data)
        w, v = _opt(weights[i], (B, rows), dev, "weights"), _opt(valids[i], (B,), dev, "valid")
        extra = [_opt(t, (B,) + dims(s), dev, k, dt) for t, (k, s, dt, _) in zip(more[i] if more else (), fit.more)]
        for t, (k, _, _, required) in zip(extra, fit.more):
            if required and t is None:
                raise ValueError(f"hands_amd: {k} is required")
        init = (None, None, None)
        if inits[i] is not None:
            if len(inits[i]) == 3:
                init = tuple(_opt(a, (B,) + s, dev, "init " + k) for a, (k, s, _) in zip(inits[i], _OUTPUTS))
            if any(a is None for a in init):
                raise ValueError("hands_amd: init is (pose (B,16,3,3), beta (B,10), transl (B,3)), all three")
        o = [torch.empty((B,) + s, dtype=t, device=dev) for _, s, t in _OUTPUTS + fit.extras]
        consts = fit.consts(*[ptr(packs[i][k]) for k in fit.const_keys])
        sides[i] = fit.side(consts, ptr(y), ptr(w), ptr(v), *[ptr(t) for t in init], *[ptr(t) for t in o], *[ptr(t) for t in extra])
        outs.append(o)
        keep.append((y, w, v, init, extra))    # converted copies stay alive until the launch is queued
    check(getattr(_lib.lib(), fit.entry)(sides, n, *[ptr(t) for t in shared], C.byref(cfg), B, *([rows] if fit.n_weights < 0 else []),
                                         torch.cuda.current_stream(dev).cuda_stream), fit.entry)
    return outs


def _matrix_to_aa(rot):
    """(B,16,3,3) -> (B,48) axis-angle through hands_matrix_to_axis_angle_f32."""
    aa = torch.empty(rot.shape[0], 48, device=rot.device)
    check(_lib.lib().hands_matrix_to_axis_angle_f32(ptr(rot), ptr(aa), rot.shape[0] * 16,
                                                    torch.cuda.current_stream(rot.device).cuda_stream), "matrix_to_axis_angle")
    return aa


def _result(fit, pack, out):
    """The outputs by name, in the order of the launch, then pose_aa (B,48) = [Log R_0, Log R_j - hands_mean_j], the axis-angle
    form HandsWrapper.process_data and the reference's targets use."""
    r = xdict({name: t for (name, _, _), t in zip(_OUTPUTS + fit.extras, out)})
    r["pose_aa"] = _matrix_to_aa(out[0]) - pack["pose_mean"]
    return r


def _fit(fit, what, hands, model_or_layer, data, weights, valids, inits, config, shared=(), more=None):
    """The fit of the sides ``hands`` (("r",), ("l",) or "rl") in one launch; -> per side what the public functions return."""
    cfg = (config or fit.config()).c_struct()      # a bad configuration is refused before anything else is looked at
    dev = _device_of(data[0], what)
    packs = [_mano_pack(model_or_layer, h, dev) for h in hands]
    outs = _launch(fit, packs, data, weights, valids, inits, cfg, dev, shared, more)
    return tuple(_result(fit, p, o) for p, o in zip(packs, outs))


_TARGET_KEYS = (("mano.pose", "pose_aa"), ("mano.beta", "beta"), ("mano.fit.rmse", "rmse"), ("mano.fit.transl", "transl"))


def _valid_flags(meta_info):
    """[right_valid, left_valid] of ``meta_info``, None where it has none."""
    return [meta_info[k] if meta_info is not None and k in meta_info else None for k in ("right_valid", "left_valid")]


def _with_fits(targets, fits, keys, keep=()):
    """A NEW xdict with the entries of ``targets`` in which, for hand h and every (key, name) of ``keys``, ``key.h`` is ``name``
    of that hand's fit; a key of ``keep`` that ``targets`` has is left alone."""
    out = xdict(targets)
    for h, f in zip("rl", fits):
        for key, name in keys:
            if not (key in keep and f"{key}.{h}" in targets):
                out.overwrite(f"{key}.{h}", f[name])
    return out


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
    return _fit(_FIT_JOINTS, "fit_mano", (side,), model_or_layer, [joints], [weights], [valid], [init], config)[0]


def fit_mano_hands(joints_r, joints_l, model, weights_r=None, weights_l=None, valid_r=None, valid_l=None, init_r=None,
                   init_l=None, config=None):
    """Both hands of a batch in ONE launch: -> (right, left), each what :func:`fit_mano` returns."""
    return _fit(_FIT_JOINTS, "fit_mano_hands", "rl", model, [joints_r, joints_l], [weights_r, weights_l], [valid_r, valid_l],
                [init_r, init_l], config)


def fit_targets(targets, model, meta_info=None, config=None) -> xdict:
    """Ground-truth MANO parameters for a keypoint-only batch: fits both hands to ``targets["mano.j3d.full.{r,l}"]`` (camera
    space, metres, on the device) in one launch and returns a NEW xdict with the entries of ``targets`` in which
    ``mano.pose.{r,l}`` (B,48) axis-angle and ``mano.beta.{r,l}`` (B,10) are the fit -- the two keys
    ``HandsWrapper.process_data`` builds the ground-truth mesh from -- and ``mano.fit.rmse.{r,l}`` (B) and
    ``mano.fit.transl.{r,l}`` (B,3) are added; ``targets`` itself is left as it was.  ``meta_info["right_valid"]`` /
    ``["left_valid"]`` (B, on the device), where present, say which rows are fitted."""
    fits = _fit(_FIT_JOINTS, "fit_targets", "rl", model, [targets["mano.j3d.full.r"], targets["mano.j3d.full.l"]], [None, None],
                _valid_flags(meta_info), [None, None], config)
    return _with_fits(targets, fits, _TARGET_KEYS)


# ---- fitting to 2-D keypoints ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fit2DConfig:
    """``iters_rigid`` iterations that free only the global rotation and the translation, then ``iters`` that free everything
    (all but the shape with ``fit_shape=False``) -- exactly that many, no data-dependent exit; the weights ``lambda_beta`` and
    ``lambda_pose`` of the priors; the first damping ``mu0`` (it restarts with the second stage); ``robust_sigma`` > 0 in pixels
    switches the Geman-McClure kernel on; a state with a weighted joint at Z <= ``z_min`` metres is never accepted;
    ``prior_to_init``: with a caller's initial state, both priors pull towards that state instead of the mean pose and beta = 0.

    The defaults are UNTUNED starting values.  On the 16 cases of the tests (seeds 0..15 of ``fit2d_ref.family_case``: the
    synthetic right asset's own joints projected with f = 1000 px, c = 112 px and rounded to fp32) the fp64 restatement reaches a
    reprojection rmse of 1.2e-3 to 2.0 px, median 7.2e-3 px; 3 of the 16 stay above 1 px."""
    iters_rigid: int = 10
    iters: int = 30
    lambda_beta: float = 1e-2
    lambda_pose: float = 1e-2
    mu0: float = 1e-3
    robust_sigma: float = 0.0
    z_min: float = 0.05
    fit_shape: bool = True
    prior_to_init: bool = False

    def c_struct(self) -> Fit2DCfg:
        _check_config(self, ("iters_rigid", "iters"), ("lambda_beta", "lambda_pose", "mu0", "robust_sigma"))
        z = float(self.z_min)
        if not (z > 0.0 and z != float("inf")):
            raise ValueError(f"hands_amd: z_min is finite and positive, got {z!r}")
        return Fit2DCfg(int(self.iters_rigid), int(self.iters), float(self.lambda_beta), float(self.lambda_pose), float(self.mu0),
                        float(self.robust_sigma), z, int(bool(self.fit_shape)), int(bool(self.prior_to_init)))


_FIT_2D = _Fit("hands_mano_fit2d_f32", ManoFit2DSide, ManoFitConsts, _CONST_KEYS, "kp2d", (21, 2), 21,
               (("start", (), torch.int32), ("j3d", (21, 3), torch.float32), ("j2d", (21, 2), torch.float32)), Fit2DConfig,
               (("intrinsics", (3, 3)),))


def fit_mano_2d(kp2d, intrinsics, model_or_layer, side="r", weights=None, valid=None, init=None, config=None) -> xdict:
    """Fit ONE hand of a batch to 2-D keypoints: ``kp2d`` (B,21,2) in PIXELS of the image ``intrinsics`` (B,3,3) belongs to (rows 0
    and 1 are read), in this package's joint order, on the device, as every other tensor argument has to be (RuntimeError
    otherwise).  ``weights`` (B,21) >= 0 (default 1; a keypoint of weight 0 is never read and may be NaN), ``valid`` (B),
    ``init`` (pose (B,16,3,3), beta (B,10), transl (B,3)) instead of the state generated from the keypoints (the rest hand under
    the best of the 24 axis-aligned rotations, placed by weak perspective), ``config`` a :class:`Fit2DConfig` (untuned defaults).

    Returns an xdict: ``pose``, ``beta``, ``transl``, ``rmse`` (B) in pixels without the robust kernel and the priors, ``steps``
    (B) int32, ``start`` (B) int32 -- the index of the generated start, -1 with ``init`` --, ``j3d`` (B,21,3) = joints + transl
    in camera space, ``j2d`` (B,21,2) their projection in pixels, and ``pose_aa`` (B,48) as :func:`fit_mano` returns it.
    The fit reproduces the KEYPOINTS: one view fixes neither depth nor scale nor a unique 3-D hand, and ``j3d`` may differ from
    the true joints by centimetres at a sub-pixel ``rmse``.  A row that is not fitted (``valid`` 0, fewer than four weighted
    keypoints, a non-finite weighted keypoint, intrinsic or initial value, K00 <= 0 or K11 <= 0, an initial state with a
    weighted joint at Z <= z_min, no start candidate) has the mean pose, zeros, ``rmse`` NaN, 0 steps, ``start`` -1 and NaN in
    ``j3d`` and ``j2d``."""
    return _fit(_FIT_2D, "fit_mano_2d", (side,), model_or_layer, [kp2d], [weights], [valid], [init], config, [intrinsics])[0]


def fit_mano_hands_2d(kp2d_r, kp2d_l, intrinsics, model, weights_r=None, weights_l=None, valid_r=None, valid_l=None, init_r=None,
                      init_l=None, config=None):
    """Both hands of a batch in ONE launch, sharing ``intrinsics``: -> (right, left), each what :func:`fit_mano_2d` returns."""
    return _fit(_FIT_2D, "fit_mano_hands_2d", "rl", model, [kp2d_r, kp2d_l], [weights_r, weights_l], [valid_r, valid_l],
                [init_r, init_l], config, [intrinsics])


def _unnormalize(t, img_res):
    """hands_unnormalize_kp2d_f32: 0.5 * img_res * (x + 1), the inverse of normalize_kp2d."""
    t = t.to(dtype=torch.float32).contiguous()
    out = torch.empty_like(t)
    check(_lib.lib().hands_unnormalize_kp2d_f32(ptr(t), ptr(out), t.numel(), float(img_res),
                                                torch.cuda.current_stream(t.device).cuda_stream), "unnormalize_kp2d")
    return out


def fit_targets_2d(targets, model, meta_info, weights_r=None, weights_l=None, config=None) -> xdict:
    """Ground-truth MANO parameters for a 2-D-only batch: fits both hands to ``targets["mano.j2d.norm.{r,l}"]`` (un-normalised
    with the model's ``img_res``) under ``meta_info["intrinsics"]`` in one launch and returns a NEW xdict with the entries of
    ``targets`` in which ``mano.pose.{r,l}`` (B,48), ``mano.beta.{r,l}`` (B,10) and ``mano.j3d.full.{r,l}`` (B,21,3; the fit's
    ``j3d``) are the fit, and ``mano.fit.rmse_px.{r,l}`` (B) and ``mano.fit.transl.{r,l}`` (B,3) are added; ``targets`` itself
    is left as it was.  ``meta_info["right_valid"]`` / ``["left_valid"]``, where present, say which rows are fitted.  The 3-D
    entries reproduce the keypoints, not the depth or scale of the true hand."""
    (config or Fit2DConfig()).c_struct()
    _device_of(targets["mano.j2d.norm.r"], "fit_targets_2d")
    res = float(getattr(model, "img_res", 224))
    fits = _fit(_FIT_2D, "fit_targets_2d", "rl", model, [_unnormalize(targets[f"mano.j2d.norm.{h}"], res) for h in "rl"],
                [weights_r, weights_l], _valid_flags(meta_info), [None, None], config, [meta_info["intrinsics"]])
    return _with_fits(targets, fits, (("mano.pose", "pose_aa"), ("mano.beta", "beta"), ("mano.j3d.full", "j3d"),
                                      ("mano.fit.rmse_px", "rmse"), ("mano.fit.transl", "transl")))


_HEAD_KEYS = ("cam_t.wp", "cam_t", "joints3d", "vertices", "j3d.cam", "v3d.cam", "j2d.norm", "beta", "pose")
MIN_WP_SCALE = 0.1           # the clamp of the MANO head's weak-perspective scale (hands_mano_heads_f32's min_s)


def _aa_to_matrix(aa):
    """(B,48) axis-angle -> (B,16,3,3) through hands_axis_angle_to_matrix_f32."""
    aa = aa.contiguous()
    rot = torch.empty(aa.shape[0], 16, 3, 3, device=aa.device)
    check(_lib.lib().hands_axis_angle_to_matrix_f32(ptr(aa), ptr(rot), aa.shape[0] * 16,
                                                    torch.cuda.current_stream(aa.device).cuda_stream), "axis_angle_to_matrix")
    return rot


def refine_predictions(pred, kp2d_r, kp2d_l, model, meta_info, weights_r=None, weights_l=None, valid_r=None, valid_l=None,
                       config=None) -> xdict:
    """Test-time refinement: move a model's prediction so that it re-projects onto detected keypoints ``kp2d_{r,l}`` (B,21,2) in
    pixels of the image ``meta_info["intrinsics"]`` belongs to.  The fit starts from the prediction -- the full pose
    Exp(Log(``mano.pose``_j) + hands_mean_j), ``mano.beta`` and ``mano.cam_t`` as the translation --; the default ``config`` is
    ``Fit2DConfig(iters_rigid=0, prior_to_init=True)``: no rigid stage, the priors pull towards the prediction.  The nine MANO-head
    keys per hand are then recomputed by one ``hands_mano_heads_f32`` launch (as ``smooth_predictions`` does) from the rotations
    before the mean, the fitted beta and the weak-perspective camera that gives the fitted translation back; every other key of
    ``pred`` is handed through, in the order of ``pred``.  Added: ``refined.{r,l}`` (B) bool, the rows that moved.

    A row that is not fitted keeps the prediction's tensors bit for bit.  So does a row whose fitted depth cannot be represented:
    the head clamps the weak-perspective scale at 0.1, so a depth beyond 2 f / (0.1 img_res) -- 89 m at f = 1000, img_res = 224
    -- is not refined.  The translation goes through the head's fp32 camera conversion, so the refined ``mano.cam_t`` is the
    fitted one to fp32 rounding of its depth."""
    dev = _device_of(pred["mano.pose.r"], "refine_predictions")
    P = model.packed(dev)
    K = meta_info["intrinsics"].to(device=dev, dtype=torch.float32).contiguous()
    inits = _prediction_state(pred, P, dev)
    config = config or Fit2DConfig(iters_rigid=0, prior_to_init=True)
    fits = fit_mano_hands_2d(kp2d_r, kp2d_l, K, model, weights_r, weights_l, valid_r, valid_l, inits[0], inits[1], config)
    return _with_refits(pred, fits, model, P, K, dev)


def _prediction_state(pred, P, dev):
    """Per hand the state a prediction is: (Exp(Log(mano.pose_j) + hands_mean_j), mano.beta, mano.cam_t), fp32 on ``dev``."""
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    inits = []
    for h in "rl":
        aa = _matrix_to_aa(f32(pred[f"mano.pose.{h}"]))
        inits.append((_aa_to_matrix(aa + P[f"mano_{h}"]["pose_mean"]), f32(pred[f"mano.beta.{h}"]), f32(pred[f"mano.cam_t.{h}"])))
    return inits


def _with_refits(pred, fits, model, P, K, dev):
    """What ``refine_predictions`` and ``register_predictions`` do after their fit: the nine MANO-head keys per hand recomputed by
    one ``hands_mano_heads_f32`` launch from the fitted state, on the rows that were fitted and whose depth the head's
    weak-perspective camera can represent; every other key and row of ``pred`` handed through; ``refined.{r,l}`` added."""
    from .mano_head import run_mano_heads
    L, stream = _lib.lib(), torch.cuda.current_stream(dev).cuda_stream
    f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    B = pred["mano.pose.r"].shape[0]
    res = float(getattr(model, "img_res", 224))
    focal = 0.5 * (K[:, 0, 0] + K[:, 1, 1])
    rot, shape, cam = torch.empty(2 * B, 16, 3, 3, device=dev), torch.empty(2 * B, 10, device=dev), torch.empty(2 * B, 3, device=dev)
    moved = []
    for i, (h, f) in enumerate(zip("rl", fits)):
        t = f["transl"]
        s = (2.0 * focal / t[:, 2] - 1e-9) / res       # the inverse of weak_perspective_to_perspective: t_z = 2 f / (res s + 1e-9)
        ok = torch.isfinite(f["rmse"]) & (s >= MIN_WP_SCALE)
        wp = torch.stack([s, t[:, 0], t[:, 1]], 1)
        sl = slice(i * B, (i + 1) * B)
        rot[sl] = torch.where(ok[:, None, None, None], _aa_to_matrix(f["pose_aa"]), f32(pred[f"mano.pose.{h}"]))
        shape[sl] = torch.where(ok[:, None], f["beta"], f32(pred[f"mano.beta.{h}"]))
        cam[sl] = torch.where(ok[:, None], wp, f32(pred[f"mano.cam_t.wp.{h}"]))
        moved.append(ok)
    new = run_mano_heads(L, P["mano_r"], P["mano_l"], rot, shape, cam, cam, K, res, B, stream, None)
    out = xdict()
    for k, v in pred.items():
        parts = k.rsplit(".", 1)
        if len(parts) == 2 and parts[1] in ("r", "l") and parts[0].startswith("mano.") and parts[0][5:] in _HEAD_KEYS:
            ok = moved["rl".index(parts[1])]
            v = torch.where(ok.view((-1,) + (1,) * (v.dim() - 1)), new[k].to(v.dtype), v)
        out[k] = v
    out["refined.r"], out["refined.l"] = moved
    return out


# ---- fitting to 778 vertices -------------------------------------------------------------------------------------------------
_VERTS_CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights", "posedirs_vm")


_FIT_VERTS = _Fit("hands_mano_fit_verts_f32", ManoFitVertsSide, ManoFitVertsConsts, _VERTS_CONST_KEYS, "verts", (778, 3), 778,
                  (("j3d", (21, 3), torch.float32),), FitConfig)


def fit_mano_verts(verts, model_or_layer, side="r", weights=None, valid=None, init=None, config=None) -> xdict:
    """Fit ONE hand of a batch to the vertices of a mesh in MANO topology: ``verts`` (B,778,3) in metres, vertex n the model's
    vertex n, on the device, as every other tensor argument has to be (RuntimeError otherwise).  ``weights`` (B,778) >= 0
    (default 1; a vertex of weight 0 is never read and may be NaN: that is how a partial or occluded mesh is fitted), ``valid``
    (B), ``init`` (pose (B,16,3,3), beta (B,10), transl (B,3)) instead of the rest hand aligned rigidly to the weighted vertices,
    ``config`` a :class:`FitConfig` (untuned defaults; see there what the thirty iterations are for).

    Returns an xdict: ``pose``, ``beta``, ``transl``, ``rmse`` (B) in metres without the priors, ``steps`` (B) int32 accepted
    steps -- past convergence a decision is a tie at rounding level and ``steps`` carries no information --, ``j3d`` (B,21,3) =
    the fitted joints + transl, and ``pose_aa`` (B,48) as :func:`fit_mano` returns it.  The fit reproduces the VERTICES and, where
    the mesh is a MANO mesh, recovers pose and shape; it does not register a surface or a point cloud without correspondences
    and fits no scale.  A row that is not fitted (``valid`` 0, fewer than four weighted vertices, a non-finite weighted vertex
    or initial value) has the mean pose, zeros, ``rmse`` NaN, 0 steps and NaN in ``j3d``."""
    return _fit(_FIT_VERTS, "fit_mano_verts", (side,), model_or_layer, [verts], [weights], [valid], [init], config)[0]


def fit_mano_hands_verts(verts_r, verts_l, model, weights_r=None, weights_l=None, valid_r=None, valid_l=None, init_r=None,
                         init_l=None, config=None):
    """Both hands of a batch in ONE launch: -> (right, left), each what :func:`fit_mano_verts` returns."""
    return _fit(_FIT_VERTS, "fit_mano_hands_verts", "rl", model, [verts_r, verts_l], [weights_r, weights_l], [valid_r, valid_l],
                [init_r, init_l], config)


def fit_targets_verts(targets, model, meta_info=None, config=None) -> xdict:
    """Ground-truth MANO parameters for a mesh-only batch: fits both hands to ``targets["mano.v3d.full.{r,l}"]`` (B,778,3; camera
    space, metres, on the device: the vertex counterpart of ``mano.j3d.full``) in one launch and returns a NEW xdict with the
    entries of ``targets`` in which ``mano.pose.{r,l}`` (B,48) and ``mano.beta.{r,l}`` (B,10) are the fit, ``mano.fit.rmse.{r,l}``
    (B) and ``mano.fit.transl.{r,l}`` (B,3) are added, and ``mano.j3d.full.{r,l}`` is the fit's ``j3d`` where ``targets`` has no
    such key (a present one is left alone); ``targets`` itself is left as it was.  ``meta_info["right_valid"]`` /
    ``["left_valid"]`` (B, on the device), where present, say which rows are fitted."""
    fits = _fit(_FIT_VERTS, "fit_targets_verts", "rl", model, [targets["mano.v3d.full.r"], targets["mano.v3d.full.l"]],
                [None, None], _valid_flags(meta_info), [None, None], config)
    return _with_fits(targets, fits, _TARGET_KEYS + (("mano.j3d.full", "j3d"),), keep=("mano.j3d.full",))


# ---- fitting to surface correspondences; ICP registration -----------------------------------------------------------------------
MAX_SURFACE_ROWS = 16384     # HANDS_FIT_SURF_MAX_P of include/hands_hip.h: it bounds time, not memory


@dataclass(frozen=True)
class SurfaceFitConfig:
    """The four numbers of :class:`FitConfig` and ``tangent_weight`` in [0, 1]: with ``normals``, the part of a residual along
    the normal counts fully and the part across it ``tangent_weight`` times (point-to-plane at 0, point-to-point at 1, where
    the normals are not read).  The defaults are UNTUNED starting values, as FitConfig's are."""
    iters: int = 30
    lambda_beta: float = 1e-6
    lambda_pose: float = 1e-6
    mu0: float = 1e-3
    tangent_weight: float = 1.0

    def c_struct(self) -> FitSurfCfg:
        _check_config(self, ("iters",), ("lambda_beta", "lambda_pose", "mu0"))
        tau = float(self.tangent_weight)
        if not 0.0 <= tau <= 1.0:
            raise ValueError(f"hands_amd: tangent_weight is in [0, 1], got {tau!r}")
        return FitSurfCfg(int(self.iters), float(self.lambda_beta), float(self.lambda_pose), float(self.mu0), tau)


_FIT_SURF = _Fit("hands_mano_fit_surf_f32", ManoFitSurfSide, ManoFitSurfConsts, _VERTS_CONST_KEYS + ("faces_i32",), "points", (-1, 3),
                 -1, (("j3d", (21, 3), torch.float32), ("verts", (778, 3), torch.float32)), SurfaceFitConfig, (),
                 (("face_idx", (-1,), torch.int32, True), ("bary", (-1, 3), torch.float32, True),
                  ("normals", (-1, 3), torch.float32, False)))


def fit_mano_surface(points, face_idx, bary, model_or_layer, side="r", weights=None, normals=None, valid=None, init=None,
                     config=None) -> xdict:
    """Fit ONE hand of a batch to points whose places on the model's surface are known: ``points`` (B,P,3) in metres, row k
    belonging to face ``face_idx`` (B,P) of the asset's face list (0..1537) at the coefficients ``bary`` (B,P,3), finite, neither
    clamped nor normalised: the model's point is sum_i bary_i * vertex faces[face_idx][i].  P is 1 to 16384, the same for the
    batch.  Every tensor is on the device (RuntimeError otherwise).  ``weights`` (B,P) >= 0 (default 1; a row of weight 0 is
    never read -- its point, coefficients and normal may be NaN, its face -1: that is how hands with fewer rows are padded),
    ``normals`` (B,P,3) with ``config.tangent_weight`` < 1 weigh a residual's part across the normal down (a zero normal: no
    such weighting for the row), ``valid`` (B), ``init`` (pose, beta, transl) instead of the rest hand aligned rigidly to the
    points, ``config`` a :class:`SurfaceFitConfig` (untuned defaults).

    Returns an xdict: ``pose``, ``beta``, ``transl``, ``rmse`` (B) -- always the Euclidean sqrt(sum w |c + t - y|^2 / sum w),
    without the normals' weighting and the priors --, ``steps``, ``j3d`` (B,21,3), ``verts`` (B,778,3) = the fitted vertices +
    transl, and ``pose_aa`` (B,48).  A hand that is not fitted (``valid`` 0, fewer than four weighted rows, a weighted row with a
    non-finite value, a weight of +inf or a face outside 0..1537, a non-finite initial value) has the mean pose, zeros, ``rmse``
    NaN, 0 steps and NaN in ``j3d`` and ``verts``."""
    return _fit(_FIT_SURF, "fit_mano_surface", (side,), model_or_layer, [points], [weights], [valid], [init], config,
                more=[(face_idx, bary, normals)])[0]


def fit_mano_hands_surface(points_r, face_idx_r, bary_r, points_l, face_idx_l, bary_l, model, weights_r=None, weights_l=None,
                           normals_r=None, normals_l=None, valid_r=None, valid_l=None, init_r=None, init_l=None, config=None):
    """Both hands of a batch in ONE launch (the same P for both): -> (right, left), each what :func:`fit_mano_surface` returns."""
    return _fit(_FIT_SURF, "fit_mano_hands_surface", "rl", model, [points_r, points_l], [weights_r, weights_l], [valid_r, valid_l],
                [init_r, init_l], config, more=[(face_idx_r, bary_r, normals_r), (face_idx_l, bary_l, normals_l)])


def correspond_on_mesh(points, verts, faces, weights=None, max_dist=0.0) -> xdict:
    """Per query point the closest point of a triangle mesh with what a fit needs, one launch of hands_mesh_correspond_f32:
    ``points`` (B,P,3), ``verts`` (B,V,3) with V <= 1024, ``faces`` (F,3) integers shared by the batch (F <= 4096), ``weights``
    (B,P) or None (all 1), on the device.  Returns an xdict of new tensors: ``dist`` (B,P), ``face_idx`` (B,P) int32 and
    ``closest`` (B,P,3) -- the bits ``closest_on_mesh`` gives --, ``bary`` (B,P,3) the coefficients of ``closest`` on its face,
    ``normal`` (B,P,3) that face's unit normal (zero for a face without one) and ``weights`` (B,P): the input weight where
    ``max_dist`` <= 0 or ``dist`` <= ``max_dist``, else 0.  A query of weight 0 is not read: NaN / -1 / NaN / NaN / 0 / 0."""
    dev = _device_of(points, "correspond_on_mesh")
    max_dist = float(max_dist)
    if max_dist != max_dist:
        raise ValueError("hands_amd: max_dist is a number")
    points = _opt(points, tuple(points.shape), dev, "points")
    if points.dim() != 3 or points.shape[2] != 3 or not isinstance(verts, torch.Tensor) or verts.dim() != 3:
        raise ValueError("hands_amd: points is (B,P,3) and verts (B,V,3)")
    B, P = points.shape[:2]
    verts = _opt(verts, (B, verts.shape[1], 3), dev, "verts")
    w = _opt(weights, (B, P), dev, "weights")
    fc = faces_on_device(faces, dev)
    out = xdict(dict(dist=torch.empty(B, P, device=dev), face_idx=torch.empty(B, P, dtype=torch.int32, device=dev),
                     closest=torch.empty(B, P, 3, device=dev), bary=torch.empty(B, P, 3, device=dev),
                     normal=torch.empty(B, P, 3, device=dev), weights=torch.empty(B, P, device=dev)))
    check(_lib.lib().hands_mesh_correspond_f32(ptr(points), ptr(verts), ptr(fc) or None, None, ptr(w), max_dist, *[ptr(t) for t in out.values()],
                                               B, P, verts.shape[1], fc.shape[0], torch.cuda.current_stream(dev).cuda_stream),
          "hands_mesh_correspond_f32")
    return out


@dataclass(frozen=True)
class RegisterConfig:
    """``rounds`` ICP rounds of ``iters`` Levenberg-Marquardt iterations each (the damping restarts at ``mu0`` every round), the
    priors' weights, ``tangent_weight`` of the rounds' fits (the normals are those of the closest faces) and ``max_dist`` in
    metres: a point farther than that from the current surface has weight 0 in its round (<= 0: no such trim).

    The defaults (10, 3, 1e-6, 1e-6, 1e-3, 0.1, 0) are UNTUNED starting points, not tuned on data; DESIGN.md section 7 records
    what the fp64 restatement reaches with them on a synthetic tube hand."""
    rounds: int = 10
    iters: int = 3
    lambda_beta: float = 1e-6
    lambda_pose: float = 1e-6
    mu0: float = 1e-3
    tangent_weight: float = 0.1
    max_dist: float = 0.0

    def fit_config(self, iters=None) -> SurfaceFitConfig:
        """The configuration of a round's fit, checked; ValueError for a bad field."""
        _check_config(self, ("rounds",), ())
        if float(self.max_dist) != float(self.max_dist):
            raise ValueError("hands_amd: max_dist is a number")
        cfg = SurfaceFitConfig(self.iters if iters is None else iters, self.lambda_beta, self.lambda_pose, self.mu0, self.tangent_weight)
        cfg.c_struct()
        return cfg


_STATE_KEYS = ("pose", "beta", "transl")


def _register(what, hands, model_or_layer, points, inits, weights, valids, config):
    config = config or RegisterConfig()
    fit_cfg, start_cfg = config.fit_config(), config.fit_config(iters=0)
    if any(i is None for i in inits):
        raise ValueError(f"hands_amd: {what} needs init = (pose (B,16,3,3), beta (B,10), transl (B,3)) for every hand: ICP is local")
    dev = _device_of(points[0], what)
    packs = [_mano_pack(model_or_layer, h, dev) for h in hands]
    points = [_opt(p, tuple(p.shape), dev, "points") for p in points]
    B, P = points[0].shape[:2]
    # round 0: no iteration, any four rows will do -- it turns init into vertices (and refuses what a fit refuses)
    face0 = torch.zeros(B, P, dtype=torch.int32, device=dev)
    bary0 = torch.zeros(B, P, 3, device=dev)
    bary0[..., 0] = 1.0
    n = len(hands)
    state = list(_fit(_FIT_SURF, what, hands, model_or_layer, points, weights, valids, inits, start_cfg,
                      more=[(face0, bary0, None)] * n))
    done = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in hands]
    dist = [torch.full((B, P), float("nan"), device=dev) for _ in hands]
    for r in range(int(config.rounds)):
        cor = [correspond_on_mesh(points[i], state[i]["verts"], packs[i]["faces_i32"], weights[i], config.max_dist) for i in range(n)]
        new = _fit(_FIT_SURF, what, hands, model_or_layer, points, [c["weights"] for c in cor], valids,
                   [tuple(s[k] for k in _STATE_KEYS) for s in state], fit_cfg,
                   more=[(c["face_idx"], c["bary"], c["normal"]) for c in cor])
        for i in range(n):
            ok = torch.isfinite(new[i]["rmse"])        # a hand whose round is not fitted keeps its state
            state[i] = xdict({k: torch.where(ok.view((-1,) + (1,) * (v.dim() - 1)), new[i][k], v) for k, v in state[i].items()})
            done[i] = torch.where(ok, torch.full_like(done[i], r + 1), done[i])
            dist[i] = cor[i]["dist"]
    for i in range(n):                                 # round 0's rmse is about its stand-in rows: it says nothing
        state[i].overwrite("rmse", torch.where(done[i] > 0, state[i]["rmse"], torch.full_like(state[i]["rmse"], float("nan"))))
        state[i]["dist"], state[i]["rounds_done"] = dist[i], done[i]
    return tuple(state)


def register_mano(points, model_or_layer, side="r", init=None, weights=None, valid=None, config=None) -> xdict:
    """Register ONE hand of a batch to a point cloud WITHOUT correspondences (data-to-model ICP): ``points`` (B,P,3) in metres
    on the device, P up to 16384.  ``init`` = (pose (B,16,3,3), beta (B,10), transl (B,3)) is REQUIRED (ValueError without it):
    ICP is local -- every round pairs a point with the closest point of the CURRENT surface --, so the global rotation and a
    rough pose have to come from somewhere else: a model's prediction (``register_predictions``) or :func:`fit_mano` /
    :func:`fit_mano_2d` on keypoints.  ``weights`` (B,P) >= 0 (a point of weight 0 is never read), ``valid`` (B), ``config`` a
    :class:`RegisterConfig` (untuned defaults).

    Round 0 is a launch without iterations that turns ``init`` into vertices; each of the ``rounds`` is one
    :func:`correspond_on_mesh` launch and one :func:`fit_mano_surface` launch from the previous state with that round's
    coefficients, normals and (``max_dist``) trimmed weights.  Nothing synchronises with the host.  A hand whose round comes back
    not fitted (``max_dist`` left fewer than four points, say) keeps its previous state.

    Returns what :func:`fit_mano_surface` returns for the last fitted round, plus ``dist`` (B,P) of the last correspondence --
    measured BEFORE the last fit -- and ``rounds_done`` (B) int32, the number of the last round that was fitted (0: none; the
    outputs are then those of round 0 -- ``init`` and its vertices, or the unfitted outputs for a hand no fit accepts -- and
    ``rmse`` is NaN).  The loop lowers
    the cloud's distance to the surface; it does not recover what the cloud does not observe."""
    return _register("register_mano", (side,), model_or_layer, [points], [init], [weights], [valid], config)[0]


def register_mano_hands(points_r, points_l, model, init_r=None, init_l=None, weights_r=None, weights_l=None, valid_r=None,
                        valid_l=None, config=None):
    """Both hands of a batch, one fit launch per round for the two (and one correspondence launch per hand): -> (right, left),
    each what :func:`register_mano` returns.  The two clouds have the same number of points (pad with weight 0)."""
    return _register("register_mano_hands", "rl", model, [points_r, points_l], [init_r, init_l], [weights_r, weights_l],
                     [valid_r, valid_l], config)


def register_predictions(pred, cloud_r, cloud_l, model, meta_info, weights_r=None, weights_l=None, valid_r=None, valid_l=None,
                         config=None) -> xdict:
    """The point-cloud counterpart of :func:`refine_predictions`: move a model's prediction onto ``cloud_{r,l}`` (B,P,3), camera
    space, metres (a depth camera's back-projected pixels of each hand, say).  The registration starts from the prediction as
    ``refine_predictions`` does, runs :func:`register_mano_hands` with ``config`` (a :class:`RegisterConfig`), and recomputes the
    nine MANO-head keys per hand exactly as ``refine_predictions`` does; ``refined.{r,l}`` (B) bool are the rows that moved.  A
    row that is not registered keeps the prediction's tensors bit for bit."""
    dev = _device_of(pred["mano.pose.r"], "register_predictions")
    (config or RegisterConfig()).fit_config()
    P = model.packed(dev)
    K = meta_info["intrinsics"].to(device=dev, dtype=torch.float32).contiguous()
    inits = _prediction_state(pred, P, dev)
    fits = register_mano_hands(cloud_r, cloud_l, model, inits[0], inits[1], weights_r, weights_l, valid_r, valid_l, config)
    return _with_refits(pred, fits, model, P, K, dev)
