"""Signed distance between the two hands, penetration depth and intersection volume, on device (csrc/mesh_distance.hip).

``signed_distance_to_mesh`` is the thin wrapper of ``hands_mesh_signed_f32``: the closest-face walk of ``closest_on_mesh`` with
the generalised winding number ``w`` summed beside it; a query is inside where ``|w| >= 0.5``.  That needs a closed surface and
MANO's hand is open at the wrist, so ``seal_mesh`` closes every boundary loop of a face list with a fan about one new vertex --
what the reference's lineage does with fixed index lists (``seal_mano_mesh``, common/body_models.py:60-72), here derived from the
faces themselves -- and ``apply_seal`` appends those vertices, the mean of each loop, as ``seal_mano_mesh`` does.  The reference
leaves the inside test to libraries that are absent, so nothing here is pinned to it; tests/penetration_ref.py restates the
definitions in fp64.
"""
from __future__ import annotations

import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .metrics import faces_on_device
from .xdict import xdict

MAX_GRID = 32                                   # intersection_volume: G^3 queries per sample at the most

_SEALS: dict = {}                               # id(face list) -> (weak reference, version, n_verts, result)


def _seal(faces: np.ndarray, n_verts: int):
    """seal_mesh on an (F,3) int64 array -> (the fan faces (K,3), the loops as lists of vertex indices)."""
    if faces.size and (faces.min() < 0 or faces.max() >= n_verts):
        raise ValueError(f"hands_amd.seal_mesh: a face index outside [0, {n_verts})")
    src, dst = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)             # the half-edges i -> j, face by face
    if (src == dst).any():
        raise ValueError("hands_amd.seal_mesh: a face with a repeated vertex index")
    key = np.minimum(src, dst) * n_verts + np.maximum(src, dst)
    _, inverse, count = np.unique(key, return_inverse=True, return_counts=True)
    if (count > 2).any():
        raise ValueError("hands_amd.seal_mesh: an edge used by more than two faces")
    open_ = count[inverse] == 1                                                # the boundary: edges of exactly one face
    bs, bd = src[open_], dst[open_]
    if len(np.unique(bs)) != len(bs) or len(np.unique(bd)) != len(bd) or set(bs.tolist()) != set(bd.tolist()):
        raise ValueError("hands_amd.seal_mesh: the boundary edges do not form simple closed loops")
    nxt = dict(zip(bs.tolist(), bd.tolist()))
    loops, seen = [], set()
    for start in sorted(nxt):                                                  # loop k begins at its lowest vertex
        if start in seen:
            continue
        loop, v = [], start
        while v not in seen:
            seen.add(v)
            loop.append(v)
            v = nxt[v]
        loops.append(loop)
    # a fan face runs against the boundary half-edge i -> j it closes: (j, i, centre), the orientation of the face next to it
    fan = [(nxt[i], i, n_verts + k) for k, loop in enumerate(loops) for i in loop]
    return np.asarray(fan, np.int64).reshape(-1, 3), loops


def seal_mesh(faces, n_verts: int):
    """Close the open boundaries of a triangle mesh.  ``faces`` (F,3) integers over ``n_verts`` vertices.  Boundary edges -- the
    edges used by exactly one face -- must form simple closed loops; loop ``k`` (ordered by lowest vertex) gets the new vertex
    ``n_verts + k`` and one fan face per boundary edge, oriented as the face on the other side of that edge.  Returns
    ``(faces_sealed, loops)``: an int32 tensor (F + sum of the loop lengths, 3) and a tuple of int64 index tensors, both on the
    device of ``faces`` (the CPU for a numpy array); a closed mesh comes back with no loop and its own faces.  ``ValueError``: an
    index outside ``[0, n_verts)``, a repeated index in a face, an edge of more than two faces, a boundary that is no set of
    simple loops.  The result is kept per face-list object, so a model's face tensor is sealed once."""
    hit = _SEALS.get(id(faces))
    version = getattr(faces, "_version", 0)
    if hit is not None and hit[0]() is faces and hit[1] == version and hit[2] == n_verts:
        return hit[3]
    dev = faces.device if isinstance(faces, torch.Tensor) else torch.device("cpu")
    host = faces_on_device(faces, torch.device("cpu"))
    fan, loops = _seal(host.numpy().astype(np.int64), int(n_verts))
    sealed = torch.cat([host, torch.from_numpy(fan).to(torch.int32)]).to(dev) if len(fan) else host.to(dev)
    result = (sealed, tuple(torch.tensor(loop, dtype=torch.int64, device=dev) for loop in loops))
    try:
        key = id(faces)
        _SEALS[key] = (weakref.ref(faces, lambda _, key=key: _SEALS.pop(key, None)), version, n_verts, result)
    except TypeError:                                                          # a list of lists: nothing to hang the entry on
        pass
    return result


def apply_seal(verts: torch.Tensor, loops) -> torch.Tensor:
    """``verts`` (B,V,3) with the mean of each loop's vertices appended: (B, V + len(loops), 3)."""
    if len(loops) == 0:
        return verts
    centres = [verts[:, loop.to(verts.device)].mean(dim=1, keepdim=True) for loop in loops]
    return torch.cat([verts] + centres, dim=1)


def signed_distance_to_mesh(points, verts, faces, valid=None):
    """Per query point the signed distance to a closed triangle mesh.  Arguments and limits as :func:`closest_on_mesh`.  Returns
    new tensors on the inputs' device, queued on the current stream: ``sdf`` (B,P) fp32, negative inside, ``winding`` (B,P) fp32
    the generalised winding number, ``face_idx`` (B,P) int64 the closest face.  Inside is ``|winding| >= 0.5``, so an
    inward-oriented mesh works too.  No usable face: +inf / 0 / -1; a non-finite query or ``valid[b] == 0``: NaN / NaN / -1."""
    dev = points.device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.signed_distance_to_mesh runs on a HIP device only (no CPU fallback)")
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    points, verts = f(points), f(verts)
    B, P = points.shape[:2]
    V = verts.shape[1]
    assert points.shape == (B, P, 3) and verts.shape == (B, V, 3)
    fc = faces_on_device(faces, dev)
    valid = None if valid is None else f(valid)
    assert valid is None or valid.shape == (B,)
    sdf, winding = torch.empty(B, P, device=dev), torch.empty(B, P, device=dev)
    idx = torch.empty(B, P, dtype=torch.int32, device=dev)
    check(_lib.lib().hands_mesh_signed_f32(ptr(points), ptr(verts), ptr(fc) or None, ptr(valid), ptr(sdf), ptr(winding), ptr(idx),
                                           B, P, V, fc.shape[0], torch.cuda.current_stream(dev).cuda_stream),
          "hands_mesh_signed_f32")
    return sdf, winding, idx.long()


def _hands(d, faces, seal, who):
    """The two hands of ``d`` as the signed primitive wants them: (v_r, v_l) as given, the (sealed) surfaces and ``valid``."""
    v_r, v_l = d["mano.v3d.cam.r"], d["mano.v3d.cam.l"]
    if v_r.device.type != "cuda":
        raise RuntimeError(f"hands_amd.{who} runs on a HIP device only (no CPU fallback)")
    if faces is None:
        faces = (d["mano.faces.r"], d["mano.faces.l"])
    valid = None
    if all(k in d for k in ("right_valid", "left_valid", "is_valid")):
        valid = d["right_valid"].float() * d["left_valid"].float() * d["is_valid"].float()
    surf = []
    for v, fc in zip((v_r, v_l), faces):
        if seal:
            fc, loops = seal_mesh(fc, v.shape[1])
            v = apply_seal(v, loops)
        surf.append((v, fc))
    return v_r, v_l, surf[0], surf[1], valid


def interhand_penetration(d, faces=None, seal=True) -> xdict:
    """How far the two hands of ``d`` (as :func:`interhand_field` takes it) pass through each other, two launches of the signed
    primitive: ``sdf.rl`` (B,V) metres from the right hand's vertices to the left hand's surface, negative inside it,
    ``inside.rl`` (B,V) int64, ``pen.depth.rl`` (B) ``= max(0, -min_v sdf.rl)`` and ``pen.count.rl`` (B) int64 the number of
    vertices inside; ``*.lr`` the other way round.  With ``seal`` each surface is closed first (:func:`seal_mesh`; the queries stay
    the hand's own vertices); ``seal=False`` takes the face lists as they are, for meshes that are closed already or cannot be
    sealed.  A sample that is not valid (``interhand_field``'s rule) gives NaN in the float outputs and 0 in the integer ones."""
    v_r, v_l, surf_r, surf_l, valid = _hands(d, faces, seal, "interhand_penetration")
    out = xdict()
    for k, q, (t, fc) in (("rl", v_r, surf_l), ("lr", v_l, surf_r)):
        sdf, w, _ = signed_distance_to_mesh(q, t, fc, valid)
        inside = w.abs() >= 0.5                                                # NaN compares false
        out["sdf." + k], out["inside." + k] = sdf, inside.long()
        out["pen.depth." + k] = (-sdf.min(dim=1).values).clamp_min(0.0)       # min and clamp keep a NaN
        out["pen.count." + k] = inside.sum(dim=1)
    return out


def penetration_grid(v_r: torch.Tensor, v_l: torch.Tensor, G: int):
    """The ``G^3`` cell centres of a regular grid over the intersection of the two hands' axis-aligned bounding boxes:
    ``points`` (B, G^3, 3) ``= lo + (i + 0.5) (hi - lo) / G`` with the x index slowest, and the volume of a cell (B), 0 where the
    boxes do not overlap.  fp32 torch ops on the device of the inputs."""
    v_r, v_l = v_r.float(), v_l.float()
    lo = torch.maximum(v_r.min(dim=1).values, v_l.min(dim=1).values)
    hi = torch.minimum(v_r.max(dim=1).values, v_l.max(dim=1).values)
    step = (hi - lo) / G                                                       # (B,3)
    i = torch.arange(G, device=v_r.device, dtype=torch.float32) + 0.5
    axis = lo[:, None, :] + i[None, :, None] * step[:, None, :]               # (B,G,3)
    B = v_r.shape[0]
    points = torch.stack([axis[:, :, None, None, 0].expand(B, G, G, G), axis[:, None, :, None, 1].expand(B, G, G, G),
                          axis[:, None, None, :, 2].expand(B, G, G, G)], dim=-1).reshape(B, G ** 3, 3)
    cell = torch.where((step > 0).all(dim=1), step.prod(dim=1), torch.zeros_like(step[:, 0]))
    return points, cell


def intersection_volume(d, faces=None, seal=True, G=24) -> torch.Tensor:
    """The volume (B) in cubic metres both hands of ``d`` occupy: the number of points of :func:`penetration_grid` with
    ``|winding| >= 0.5`` against both (sealed) hands, times the cell volume; two launches of the signed primitive with ``G^3``
    queries each, ``G <= 32``.  Exactly 0 where the bounding boxes do not overlap, NaN for a sample that is not valid."""
    if not 1 <= G <= MAX_GRID:
        raise ValueError(f"hands_amd.intersection_volume: G must be in [1, {MAX_GRID}], got {G}")
    _, _, surf_r, surf_l, valid = _hands(d, faces, seal, "intersection_volume")
    points, cell = penetration_grid(surf_r[0], surf_l[0], G)
    both = None
    for t, fc in (surf_r, surf_l):
        w = signed_distance_to_mesh(points, t, fc, valid)[1]
        both = (w.abs() >= 0.5) if both is None else both & (w.abs() >= 0.5)
    vol = both.sum(dim=1).float() * cell
    return vol if valid is None else torch.where(valid != 0, vol, torch.full_like(vol, float("nan")))
