"""Soft-silhouette renderer of the predicted MANO meshes, on device (csrc/render.hip).

Mirror of the reference's ``MANORenderer(args)`` (src/models/hands_light/renderer.py:161-200), which the three models call on
``mano.v3d.cam.{r,l}`` to get the per-hand masks ``render.r`` / ``render.l`` (hands_light/model.py:413-420,
hamer_light/model.py:143-148).  The reference builds pytorch3d ``Meshes`` / ``PerspectiveCameras`` and runs ``MeshRasterizer`` +
``SoftSilhouetteShader`` with the settings of ``DiffRenderer`` (renderer.py:116-123); here one kernel launch rasterises the
whole batch from the vertex tensor the MANO heads wrote.  pytorch3d is third party and absent from the reference checkout: the
kernel restates its published algorithm ("parity unpinned").

Inference only: the outputs carry no gradient (the reference uses the masks in a training loss; training is out of scope).
No CPU fallback: CPU tensors raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr
from .mano import mano_face_lists
from .xdict import xdict

# renderer.py:116-123: BlendParams(sigma=1e-5), dist_eps = 1e-6, RasterizationSettings(blur_radius=log(1/dist_eps - 1) * sigma,
# faces_per_pixel=10, perspective_correct=False)
SIGMA = 1e-5
DIST_EPS = 1e-6
BLUR_RADIUS = math.log(1. / DIST_EPS - 1.) * SIGMA
FACES_PER_PIXEL = 10


def rasterize(verts, faces, K, img_res, return_zbuf=True, sigma=SIGMA, blur_radius=BLUR_RADIUS,
              faces_per_pixel=FACES_PER_PIXEL):
    """The low-level call.  verts (B, N, 3) fp32 in the camera frame, faces (F, 3) int32 shared by the batch, K (B, 3, 3) in
    pixels of the img_res x img_res image.  Returns ``{"mask": (B, 1, S, S)}`` and, with ``return_zbuf``, ``"face_idx"``
    (B, S, S) int32 (-1 = empty) and ``"zbuf"`` (B, S, S) of the nearest face that contains each pixel.  Fresh tensors, ordered
    on the current stream."""
    if not (torch.is_tensor(verts) and verts.device.type == "cuda"):
        raise RuntimeError("hands_amd.render.rasterize runs on a HIP device only (no CPU fallback)")
    dev = verts.device
    if faces.device != dev or K.device != dev:
        raise RuntimeError("hands_amd.render.rasterize: verts, faces and K must be on the same HIP device")
    if verts.dim() != 3 or verts.shape[2] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or K.shape != (verts.shape[0], 3, 3):
        raise ValueError(f"rasterize: verts (B, N, 3), faces (F, 3), K (B, 3, 3) expected, got {tuple(verts.shape)}, "
                         f"{tuple(faces.shape)}, {tuple(K.shape)}")
    verts = verts.detach().to(torch.float32).contiguous()
    faces = faces.to(torch.int32).contiguous()
    K = K.detach().to(torch.float32).contiguous()
    B, N, S = verts.shape[0], verts.shape[1], int(img_res)
    mask = torch.empty(B, 1, S, S, device=dev)
    out = {"mask": mask}
    if return_zbuf:
        out["face_idx"] = torch.empty(B, S, S, device=dev, dtype=torch.int32)
        out["zbuf"] = torch.empty(B, S, S, device=dev)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        check(_lib.lib().hands_render_silhouette_f32(
            ptr(verts), 3 * N, N, ptr(faces), faces.shape[0], ptr(K), B, S, float(sigma), float(blur_radius),
            int(faces_per_pixel), ptr(mask), ptr(out.get("face_idx")), ptr(out.get("zbuf")),
            torch.cuda.current_stream(dev).cuda_stream), "hands_render_silhouette_f32")
    return out


class MANORenderer(nn.Module):
    """``MANORenderer(args)(mano_output, meta_info, is_right)`` -> ``{"image", "mask"}`` like the reference's.

    The reference reads the face lists from ``default_mano_faces.pkl`` in the working directory (a file its checkout does not
    have).  Here they come from ``faces=(right, left)`` arrays, else from ``mano_assets=(right, left)`` (``ManoAsset.faces``),
    else from :func:`hands_amd.build_mano_asset`; they are uploaded once per device."""

    sigma = SIGMA
    blur_radius = BLUR_RADIUS
    faces_per_pixel = FACES_PER_PIXEL

    def __init__(self, args=None, mano_assets=None, faces=None):
        super().__init__()
        self.args = args
        get = (lambda k, d=None: args.get(k, d)) if isinstance(args, dict) else (lambda k, d=None: getattr(args, k, d))
        self.img_res = int(get("img_res", None) or 224)
        if faces is None:
            faces = mano_face_lists(mano_assets)
        f_r, f_l = (torch.as_tensor(np.asarray(f.cpu() if torch.is_tensor(f) else f).astype(np.int32)) for f in faces)
        assert f_r.dim() == 2 and f_r.shape[1] == 3 and f_l.dim() == 2 and f_l.shape[1] == 3
        self.mano_faces_r, self.mano_faces_l = f_r.contiguous(), f_l.contiguous()
        self._dev_faces = {}

    def _faces_on(self, dev, is_right):
        key = (str(dev), bool(is_right))
        if key not in self._dev_faces:
            self._dev_faces[key] = (self.mano_faces_r if is_right else self.mano_faces_l).to(dev)
        return self._dev_faces[key]

    @staticmethod
    def _verts(mano_output, post):
        for key in ("mano.v3d.cam" + post, "v3d.cam" + post):
            if key in mano_output:
                return mano_output[key]
        raise KeyError("mano.v3d.cam" + post)

    def _rasterize(self, verts, K, is_right=True, return_zbuf=True):
        if not (torch.is_tensor(verts) and verts.device.type == "cuda"):
            raise RuntimeError("hands_amd.MANORenderer runs on a HIP device only (no CPU fallback)")
        return rasterize(verts, self._faces_on(verts.device, is_right), K.to(verts.device), self.img_res, return_zbuf,
                         self.sigma, self.blur_radius, self.faces_per_pixel)

    @torch.no_grad()
    def forward(self, mano_output, meta_info, is_right=True):
        verts = self._verts(mano_output, ".r" if is_right else ".l")        # renderer.py:180-185
        mask = self._rasterize(verts, meta_info["intrinsics"], is_right, return_zbuf=False)["mask"]
        # SoftSilhouetteShader returns RGB = 1 everywhere (renderer.py:153: "all 1s ... only care about mask")
        return {"image": torch.ones(mask.shape[0], 3, self.img_res, self.img_res, device=mask.device), "mask": mask}

    @torch.no_grad()
    def render_masks(self, pred, meta_info):
        """model.py:413-420: the ``render.r`` / ``render.l`` entries a model built with ``use_render_seg_loss`` adds to its output."""
        out = xdict()
        out["render.r"] = self.forward(pred, meta_info, is_right=True)["mask"]
        out["render.l"] = self.forward(pred, meta_info, is_right=False)["mask"]
        return out
