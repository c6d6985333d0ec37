"""``HandsWrapper`` -- the inference-side shell of the reference's wrapper around ``HandsLight``.

The reference's ``HandsWrapper(GenericWrapper(AbstractPL(LightningModule)))``
(src/models/hands_light/wrapper.py:11-25, src/models/generic/wrapper.py:27-75) is a training
harness; ``inference`` / ``inference_pose`` and the validation call ``forward(..., "test")`` are what this
class reproduces: run the model, merge ``inputs.*`` + ``pred.*`` + ``meta_info.*`` into one strict
dict and move every tensor to the CPU (generic/wrapper.py:68-75); in ``forward``, GT preprocessing, the
metrics and -- on request -- the loss dict ``loss__val`` is averaged from (hands_amd/losses.py), all on
device.  Like the reference it does not switch the module to eval mode; the HIP path has no train-mode
behaviour anyway: gradients, optimisers and ``mode="train"`` stay out of scope.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import ManoOut, ManoSide, check, ptr
from .engine import DEFAULT_ENGINE
from .hands_light import DEFAULT_ARGS, HandsLight
from .xdict import xdict


class HandsWrapper(nn.Module):
    # a hands_amd.FitConfig here makes process_data fit MANO to the annotated vertices mano.v3d.full.{r,l} (B,778,3) first
    # (hands_amd.fit_targets_verts): a mesh-only batch then yields the full target dict, mano.j3d.full from the fit where the
    # batch has none; more than one of the three fits set raises; None: nothing changes
    fit_gt_verts = None

    def __init__(self, args=None, push_images_fn=None, model: HandsLight | None = None):
        super().__init__()
        args = args if args is not None else DEFAULT_ARGS
        self.args = args
        get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
        self.model = model if model is not None else HandsLight(
            backbone=get("backbone", "resnet50"), focal_length=get("focal_length", 1000.0),
            img_res=get("img_res", 224), args=args)
        # the reference wrapper owns its own MANO layers for GT processing (generic/wrapper.py:36-39)
        self.mano_r = self.model.mano_r.mano
        self.mano_l = self.model.mano_l.mano
        # generic/wrapper.py:44-54.  The four reference names are always evaluated (one launch gives them all); the extra
        # name "mesh" adds evaluate_mesh_metrics' MPVPE / F-score / AUC keys to what forward(..., "test") returns, the extra
        # name "surface" evaluate_surface_metrics' point-to-surface and Chamfer keys, the extra name "penetration"
        # evaluate_penetration_metrics' depth and count keys (penetration_seal is handed on as its `seal`: a model whose face
        # lists cannot be sealed, such as the synthetic asset's, sets it to False), the extra name "accel" the acceleration
        # errors acc/*, acc/j/*, acc/abs/* of hands_amd.AccelMetrics: consecutive calls are read as consecutive frames at
        # accel_fps, sequences told apart by meta_info["seq_id"] where it is given; reset_accel() starts a new stream
        self.metric_dict = ["mrrpe.rl", "mpjpe.ra", "mpjpe.pa.ra", "pix_err"]
        self.penetration_seal = True
        self.accel_fps = 30.0
        # a hands_amd.TemporalSmoother here makes forward(..., "test") smooth the predictions over consecutive calls (One-Euro
        # filter over the MANO parameters, re-posed) before the loss, the de-normalisation and the metrics; None: nothing changes
        self.smoother = None
        # a hands_amd.FitConfig here makes process_data fit MANO to the annotated joints mano.j3d.full.{r,l} first
        # (hands_amd.fit_targets): a keypoint-only batch, whose mano.pose / mano.beta are missing or dummies, then yields the
        # full target dict and every metric family; None: nothing changes
        self.fit_gt = None
        # a hands_amd.Fit2DConfig here makes process_data fit MANO to the annotated 2-D keypoints mano.j2d.norm.{r,l} first
        # (hands_amd.fit_targets_2d): a 2-D-only batch, whose mano.j3d.full are zeros, then yields a full target dict that
        # re-projects onto the annotation (depth and scale are not recovered); setting both fits raises; None: nothing changes
        self.fit_gt_2d = None

    def inference_pose(self, inputs, meta_info):
        pred = self.model(inputs, meta_info)
        mydict = xdict()
        mydict.merge(xdict(inputs).prefix("inputs."))
        mydict.merge(pred.prefix("pred."))
        mydict.merge(xdict(meta_info).prefix("meta_info."))
        return mydict.detach()

    def inference(self, inputs, meta_info):
        return self.inference_pose(inputs, meta_info)

    # ---- GT preprocessing on device (src/callbacks/process/process_arctic.py:4-75) ----------------
    @torch.no_grad()
    def process_data(self, targets, meta_info):
        """Adds mano.{joints3d,vertices,cam_t,cam_t.wp,v3d.cam,j3d.cam}.{r,l} to ``targets`` from the GT
        MANO parameters (axis-angle pose (B,48), betas (B,10)) and the annotated camera-space joints
        ``mano.j3d.full.{r,l}``; MANO runs on the same LBS kernels as the prediction path."""
        if self.fit_gt is not None and self.fit_gt_2d is not None:
            raise ValueError("hands_amd.HandsWrapper: fit_gt and fit_gt_2d are both set; a batch is fitted to 3-D joints or to "
                             "2-D keypoints, not both")
        if self.fit_gt_verts is not None and (self.fit_gt is not None or self.fit_gt_2d is not None):
            raise ValueError("hands_amd.HandsWrapper: fit_gt_verts is set beside fit_gt or fit_gt_2d; a batch is fitted to 3-D "
                             "joints, to 2-D keypoints or to vertices, to one of them")
        L = _lib.lib()
        K = meta_info["intrinsics"]
        dev = K.device
        if dev.type != "cuda":
            raise RuntimeError("hands_amd.HandsWrapper runs on a HIP device only (no CPU fallback)")
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        if self.fit_gt_verts is not None:           # as everything below: what arrives on the host is moved here
            from .fitting import fit_targets_verts
            moved, flags = xdict(targets), dict(meta_info)
            for h in "rl":
                moved.overwrite(f"mano.v3d.full.{h}", f32(targets[f"mano.v3d.full.{h}"]))
            for k in ("right_valid", "left_valid"):
                if k in flags:
                    flags[k] = f32(flags[k])
            targets = fit_targets_verts(moved, self.model, flags, self.fit_gt_verts)
        if self.fit_gt_2d is not None:
            from .fitting import fit_targets_2d
            moved, flags = xdict(targets), dict(meta_info)
            for h in "rl":
                moved.overwrite(f"mano.j2d.norm.{h}", f32(targets[f"mano.j2d.norm.{h}"]))
            flags["intrinsics"] = f32(K)
            for k in ("right_valid", "left_valid"):
                if k in flags:
                    flags[k] = f32(flags[k])
            targets = fit_targets_2d(moved, self.model, flags, config=self.fit_gt_2d)
        if self.fit_gt is not None:                 # as everything below: what arrives on the host is moved here
            from .fitting import fit_targets
            moved, flags = xdict(targets), dict(meta_info)
            for h in "rl":
                moved.overwrite(f"mano.j3d.full.{h}", f32(targets[f"mano.j3d.full.{h}"]))
            for k in ("right_valid", "left_valid"):
                if k in flags:
                    flags[k] = f32(flags[k])
            targets = fit_targets(moved, self.model, flags, self.fit_gt)
        K = f32(K)
        P = self.model.packed(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        img_res = float(getattr(self.model, "img_res", 224))
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        for h, mp in (("r", P["mano_r"]), ("l", P["mano_l"])):
            pose, beta, full = f32(targets[f"mano.pose.{h}"]), f32(targets[f"mano.beta.{h}"]), f32(targets[f"mano.j3d.full.{h}"])
            B = pose.shape[0]
            assert pose.shape == (B, 48) and beta.shape == (B, 10) and full.shape == (B, 21, 3)
            o = {k: new(B, n, 3) for k, n in (("vertices", 778), ("joints3d", 21), ("v3d", 778), ("j3d", 21))}
            j2d, cam_t_unused, one_cam = new(B, 21, 2), new(B, 3), torch.ones(B, 3, device=dev)
            mo = ManoOut(ptr(o["vertices"]), ptr(o["joints3d"]), ptr(o["v3d"]), ptr(o["j3d"]), ptr(j2d), ptr(cam_t_unused))
            side = (ManoSide * 1)(ManoSide(mp["consts"], ptr(mp["blend"].w), ptr(mp["blend"].bias), ptr(pose), ptr(beta),
                                           ptr(one_cam), mo))
            check(L.hands_mano_heads_f32(side, 1, ptr(K), 10, img_res, 0.1, B, 1, stream), "mano_heads (axis-angle)")
            v3d_cam, cam_t, cam_wp = new(B, 778, 3), new(B, 3), new(B, 3)
            check(L.hands_gt_targets_f32(ptr(o["joints3d"]), ptr(o["vertices"]), ptr(full), ptr(K), img_res, ptr(v3d_cam),
                                         ptr(cam_t), ptr(cam_wp), B, 778, stream), "gt_targets")
            for key, val in ((f"mano.joints3d.{h}", o["joints3d"]), (f"mano.vertices.{h}", o["vertices"]),
                             (f"mano.cam_t.{h}", cam_t), (f"mano.cam_t.wp.{h}", cam_wp), (f"mano.v3d.cam.{h}", v3d_cam),
                             (f"mano.j3d.cam.{h}", full)):
                targets.overwrite(key, val)
        return targets

    def _unnormalize(self, t):
        L = _lib.lib()
        t = t.to(dtype=torch.float32).contiguous()
        out = torch.empty_like(t)
        check(L.hands_unnormalize_kp2d_f32(ptr(t), ptr(out), t.numel(), float(getattr(self.model, "img_res", 224)),
                                           torch.cuda.current_stream(t.device).cuda_stream), "unnormalize_kp2d")
        return out

    def _mask_renderer(self):
        """The soft-silhouette renderer of the mask loss, built on first use from the model's MANO face lists."""
        r = self.__dict__.get("_mask_renderer_obj")
        if r is None:
            from .render import MANORenderer
            r = MANORenderer({"img_res": int(getattr(self.model, "img_res", 224))},
                             faces=(self.model.mano_r.faces, self.model.mano_l.faces))
            self.__dict__["_mask_renderer_obj"] = r
        return r

    def _accel_metrics(self):
        """The streaming acceleration metrics, built on first use with ``accel_fps``."""
        a = self.__dict__.get("_accel_metrics_obj")
        if a is None:
            from .temporal import AccelMetrics
            a = AccelMetrics(self.accel_fps)
            self.__dict__["_accel_metrics_obj"] = a
        return a

    def reset_accel(self):
        """Forget the frames the "accel" metrics carry from one ``forward`` to the next (a new stream; ``accel_fps`` is read again)."""
        self.__dict__.pop("_accel_metrics_obj", None)

    def reset_smoother(self):
        """Start a new stream for ``smoother``, if there is one (its filter state and id dict are forgotten)."""
        if self.smoother is not None:
            self.smoother.reset()

    def forward(self, inputs, targets=None, meta_info=None, mode="test", compute_loss=False, loss_args=None):
        """GenericWrapper.forward without the training parts (src/models/generic/wrapper.py:77-164):
        GT preprocessing -> model -> [loss dict] -> 2-D de-normalisation -> metrics (``test``) / merged dict
        (``vis``, ``extract``).

        By default the loss dict is returned empty.  With ``compute_loss=True`` the reference's
        ``compute_loss_light(pred, targets, meta_info, loss_args or self.args)`` is evaluated on device where the
        reference calls it (generic/wrapper.py:97-115) and ``test`` returns the weighted 0-dim values plus their sum
        under ``'loss'``; forward evaluation only -- ``mode="train"`` raises.  If the loss args switch
        ``use_render_seg_loss`` on and the model gave no ``render.r``, ``MANORenderer.render_masks`` fills
        ``render.{r,l}`` into the predictions first.

        With a ``TemporalSmoother`` in ``self.smoother``, a ``test`` call is a frame batch of its stream: the predictions are
        replaced by ``smoother.update(...)`` right after the model call, a hand's frame being valid where
        ``{right,left}_valid * is_valid`` of the targets is non-zero (every frame where the targets have no flags); loss,
        masks and metrics -- "accel" among them -- then see the smoothed stream.  ``vis`` and ``extract`` are left alone."""
        if mode not in ("test", "extract", "vis"):
            raise NotImplementedError("hands_amd.HandsWrapper: the training mode (gradients, optimiser) is out of scope")
        inputs, targets, meta_info = xdict(inputs), xdict(targets or {}), xdict(meta_info)
        targets = self.process_data(targets, meta_info)
        meta_info.overwrite("mano.faces.r", self.model.mano_r.faces)      # generic/wrapper.py:93-94
        meta_info.overwrite("mano.faces.l", self.model.mano_l.faces)
        pred = self.model(inputs, meta_info)
        if self.smoother is not None and mode == "test":
            flag = lambda k: targets[k] * targets["is_valid"] if k in targets and "is_valid" in targets else targets.get(k)
            pred = self.smoother.update(pred, meta_info, valid_r=flag("right_valid"), valid_l=flag("left_valid"))
        loss_dict = {}
        if compute_loss:                                                   # generic/wrapper.py:97-115
            from .losses import compute_loss_light, mul_loss_dict, total_loss
            largs = loss_args if loss_args is not None else self.args
            lget = largs.get if hasattr(largs, "get") else (lambda k, d=None: getattr(largs, k, d))
            if lget("use_render_seg_loss", False) and "render.r" not in pred:
                pred.merge(self._mask_renderer().render_masks(pred, meta_info))
            loss_dict = dict(total_loss(mul_loss_dict(compute_loss_light(pred, targets, meta_info, largs))))
        for key in list(pred.keys()):                                      # generic/wrapper.py:118-134
            if "2d.norm" in key:
                assert key in targets.keys(), f"Do not have key {key}"
                dk = key.replace(".norm", "")
                dev = pred[key].device
                pred[dk] = self._unnormalize(pred[key])
                targets[dk] = self._unnormalize(targets[key].to(dev))
        merged = lambda: xdict({**inputs.prefix("inputs."), **pred.prefix("pred."), **targets.prefix("targets."),
                                **meta_info.prefix("meta_info.")}).detach()
        if mode == "vis":
            return merged()
        from .metrics import evaluate_mesh_metrics, evaluate_metrics, evaluate_surface_metrics
        metrics_all = evaluate_metrics(pred, targets, meta_info).detach()
        if "mesh" in self.metric_dict:
            metrics_all.merge(evaluate_mesh_metrics(pred, targets, meta_info).detach())
        if "surface" in self.metric_dict:
            faces = (self.model.mano_r.faces, self.model.mano_l.faces)
            metrics_all.merge(evaluate_surface_metrics(pred, targets, meta_info, faces=faces).detach())
        if "penetration" in self.metric_dict:
            from .metrics import evaluate_penetration_metrics
            faces = (self.model.mano_r.faces, self.model.mano_l.faces)
            metrics_all.merge(evaluate_penetration_metrics(pred, targets, meta_info, faces=faces, seal=self.penetration_seal).detach())
        if "accel" in self.metric_dict and mode == "test":                 # "extract" returns no metric: it is no frame of the stream
            metrics_all.merge(self._accel_metrics().update(pred, targets, meta_info).detach())
        out_dict = xdict()
        out_dict["imgname"] = meta_info.get("imgname")
        out_dict.merge({"metric." + k: v for k, v in metrics_all.items()})
        if mode == "extract":
            return merged()
        return out_dict, loss_dict


class HaMeRWrapper(HandsWrapper):
    """src/models/hamer_light/wrapper.py:5-19: the same shell around ``HAMER``."""

    def __init__(self, args=None, push_images_fn=None, model=None):
        from .hamer import HAMER, HAMER_DEFAULT_ARGS
        args = args if args is not None else HAMER_DEFAULT_ARGS
        get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
        if model is None:
            model = HAMER(focal_length=get("focal_length", 1000.0), img_res=get("img_res", 224), args=args)
        super().__init__(args, push_images_fn, model=model)


class HandOccNetWrapper(HandsWrapper):
    """src/models/handoccnet_light/wrapper.py:5-19: the same shell around ``HandOccNet``."""

    def __init__(self, args=None, push_images_fn=None, model=None):
        from .handoccnet import HANDOCC_DEFAULT_ARGS, HandOccNet
        args = args if args is not None else HANDOCC_DEFAULT_ARGS
        get = args.get if hasattr(args, "get") else (lambda k, d=None: getattr(args, k, d))
        if model is None:
            model = HandOccNet(focal_length=get("focal_length", 1000.0), img_res=get("img_res", 224), args=args)
        super().__init__(args, push_images_fn, model=model)
