"""Closest point on a triangle mesh and the distance field between the two hands, on device (csrc/mesh_distance.hip).

``closest_on_mesh`` is the thin wrapper of ``hands_mesh_closest_f32``.  ``interhand_field`` is what the reference's lineage
computes with ``pytorch3d.ops.knn_points`` (src/utils/interfield.py: distance clamped to ``[dist_min, dist_max]``, index of
the neighbour; ``dist2contact``: ``(dist < contact_bnd).long()`` with ``contact_dist`` = 3 mm, src/utils/loss_modules.py:48) --
with one deviation: the distance goes to the other hand's triangle SURFACE and the index names a face, where the reference
takes the nearest vertex.  pytorch3d is absent, so nothing here is pinned to it; tests/surface_ref.py restates the definition.
"""
from __future__ import annotations

import torch

from . import _lib
from ._lib import check, ptr
from .metrics import faces_on_device
from .xdict import xdict


def closest_on_mesh(points, verts, faces, valid=None, return_points=False):
    """Per query point the closest point of a triangle mesh.  ``points`` (B,P,3), ``verts`` (B,V,3) with V <= 1024, ``faces``
    (F,3) integers shared by the batch (F <= 4096), ``valid`` (B) or None.  Returns new tensors on the inputs' device, queued
    on the current stream: ``dist`` (B,P) fp32, ``face_idx`` (B,P) int64 and, with ``return_points``, ``closest`` (B,P,3).
    No usable face: +inf / -1 / NaN; a non-finite query or ``valid[b] == 0``: NaN / -1 / NaN (include/hands_hip.h)."""
    dev = points.device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.closest_on_mesh runs on a HIP device only (no CPU fallback)")
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    points, verts = f(points), f(verts)
    B, P = points.shape[:2]
    V = verts.shape[1]
    assert points.shape == (B, P, 3) and verts.shape == (B, V, 3)
    fc = faces_on_device(faces, dev)
    valid = None if valid is None else f(valid)
    assert valid is None or valid.shape == (B,)
    dist = torch.empty(B, P, device=dev)
    idx = torch.empty(B, P, dtype=torch.int32, device=dev)
    closest = torch.empty(B, P, 3, device=dev) if return_points else None
    check(_lib.lib().hands_mesh_closest_f32(ptr(points), ptr(verts), ptr(fc) or None, ptr(valid), ptr(dist), ptr(idx), ptr(closest),
                                            B, P, V, fc.shape[0], torch.cuda.current_stream(dev).cuda_stream),
          "hands_mesh_closest_f32")
    return (dist, idx.long(), closest) if return_points else (dist, idx.long())


def interhand_field(d, faces=None, contact_bnd=3e-3, dist_min=None, dist_max=None) -> xdict:
    """The distance field between the two hands of ``d`` (a model output or a targets dict with ``mano.v3d.cam.{r,l}``), two
    launches of the primitive: ``dist.rl`` (B,V) the distance in metres from the right hand's vertices to the left hand's
    surface, clamped to ``[dist_min, dist_max]`` where given, ``idx.rl`` its closest face, ``contact.rl = (dist.rl <
    contact_bnd).long()``; ``*.lr`` the other way round.  ``faces=(faces_r, faces_l)``, else ``d["mano.faces.{r,l}"]``.  Where
    ``d`` has ``right_valid``, ``left_valid`` and ``is_valid``, a sample whose product of the three is 0 gives NaN / -1 / 0."""
    v_r, v_l = d["mano.v3d.cam.r"], d["mano.v3d.cam.l"]
    if faces is None:
        faces = (d["mano.faces.r"], d["mano.faces.l"])
    valid = None
    if all(k in d for k in ("right_valid", "left_valid", "is_valid")):
        valid = d["right_valid"].float() * d["left_valid"].float() * d["is_valid"].float()
    out = xdict()
    for k, (q, t, fc) in (("rl", (v_r, v_l, faces[1])), ("lr", (v_l, v_r, faces[0]))):
        dist, idx = closest_on_mesh(q, t, fc, valid)
        if dist_min is not None or dist_max is not None:
            dist = torch.clamp(dist, dist_min, dist_max)
        out["dist." + k], out["idx." + k], out["contact." + k] = dist, idx, (dist < contact_bnd).long()
    return out
