"""Shaded pictures of the predicted meshes, on device (csrc/shade.hip): the overlay on the input image and the rotated side views.

Mirror of the reference's ``Renderer(img_res)`` (common/rend_utils.py:34-190, built at src/models/generic/wrapper.py:40, driven
by ``visualize_rend`` of src/callbacks/vis/visualize_arctic.py:199-271).  The reference hands trimesh objects to pyrender
(OpenGL / EGL, one image at a time); here two kernels draw the whole batch: ``hands_mesh_prepare_f32`` (rigid transform,
area-weighted vertex normals, projection) once per mesh and ``hands_render_shaded_f32`` (hard z-buffer, glTF 2.0
metallic-roughness shading, composite).  pyrender is third party and absent: the semantics are specified in DESIGN.md section 7
and restated in fp64 in tests/shade_ref.py ("parity unpinned"); no pixel parity with pyrender is claimed.

Inference only.  No CPU fallback: CPU vertex tensors raise.
"""
from __future__ import annotations

import collections
import math

import numpy as np
import torch
import torch.nn.functional as F_

from . import _lib
from ._lib import check, ptr
from .mano import mano_face_lists

# include/hands_hip.h: HANDS_SHADE_TILE_W / _H, HANDS_SHADE_LIST_CAP, HANDS_SHADE_MAX_MESHES (tests/test_shaded_render.py
# holds these against the header)
SHADE_TILE = (32, 8)                 # pixels (width, height) of one workgroup's tile
SHADE_LIST_CAP = 384                 # face records of one chunk of a tile's list
SHADE_MAX_MESHES = _lib.SHADE_MAX_MESHES
WORKSPACE_FLOATS_PER_VERTEX = 8

# visualize_arctic.py:15-21 (mesh_color_dict), 0-255
COLOR_RIGHT = (100, 100, 254)
COLOR_LEFT = (183, 100, 254)
DEFAULT_COLORS = (COLOR_RIGHT, COLOR_LEFT, (144, 250, 100), (129, 159, 214))
SIDEVIEW_ANGLES = (45.0, 172.5, 300.0)          # np.linspace(45, 300, 3), visualize_arctic.py:256


def denormalize_images(images):
    """common/data_utils.py:322-329: undo the ImageNet mean / std normalisation of ``inputs.img`` (B, 3, H, W)."""
    images = images * torch.tensor([0.229, 0.224, 0.225], device=images.device, dtype=images.dtype).reshape(1, 3, 1, 1)
    return images + torch.tensor([0.485, 0.456, 0.406], device=images.device, dtype=images.dtype).reshape(1, 3, 1, 1)


def build_vertex_face_csr(faces, n_verts):
    """The vertex -> face table the pre-pass gathers normals through: ``offsets`` (n_verts + 1) and ``face_ids`` int32, the
    faces that hold each vertex in ascending order, each face once per vertex.  A face with an index outside [0, n_verts) is
    in no list.  Host side, numpy."""
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    ok = ((faces >= 0) & (faces < n_verts)).all(axis=1)
    fid = np.repeat(np.arange(faces.shape[0], dtype=np.int64), 3)
    vid = faces.reshape(-1)
    keep = np.repeat(ok, 3)
    pairs = np.unique(np.stack([vid[keep], fid[keep]], axis=1), axis=0)      # sorted by (vertex, face), duplicates dropped
    counts = np.bincount(pairs[:, 0], minlength=n_verts) if pairs.size else np.zeros(n_verts, np.int64)
    offsets = np.zeros(n_verts + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    return offsets, np.ascontiguousarray(pairs[:, 1].astype(np.int32))


def _rotation_values(angle_deg):
    """Row-major R_y(-angle)."""
    a = -math.radians(float(angle_deg))
    return (math.cos(a), 0.0, math.sin(a), 0.0, 1.0, 0.0, -math.sin(a), 0.0, math.cos(a))


def _rigid_about(center, R, cam_transl):
    """T = [R | c - R c + cam_transl]; center (..., 3), R (3, 3), cam_transl broadcastable to center or None."""
    t = center - center @ R.T
    if cam_transl is not None:
        t = t + cam_transl
    return torch.cat([R.expand(*center.shape[:-1], 3, 3), t.unsqueeze(-1)], dim=-1)


def sideview_transform(anchor_verts, angle_deg, cam_transl=None):
    """The side view of rend_utils.py:62-78 as a rigid transform of the camera frame: a rotation by **-angle** about +y around
    the anchor's vertex mean (the reference rotates by +angle after ``flip_meshes``' 180-degree turn about x), then
    ``cam_transl`` (its x-negation at :55 and the flip cancel).  anchor_verts (B, N, 3) or (N, 3) -> T (B, 3, 4) or (3, 4),
    P' = T[:, :3] P + T[:, 3].  Plain torch: works on CPU tensors, in the dtype of ``anchor_verts``."""
    if not torch.is_tensor(anchor_verts) or anchor_verts.dim() not in (2, 3) or anchor_verts.shape[-1] != 3:
        raise ValueError("sideview_transform: anchor_verts (B, N, 3) or (N, 3) expected")
    kw = dict(dtype=anchor_verts.dtype, device=anchor_verts.device)
    R = torch.tensor(_rotation_values(angle_deg), **kw).reshape(3, 3)
    return _rigid_about(anchor_verts.mean(dim=-2), R, None if cam_transl is None else torch.as_tensor(cam_transl, **kw))


class Renderer:
    """``Renderer(img_res)`` like the reference's; the meshes are batched device tensors instead of trimesh objects.

    Face lists and their CSR tables are cached per device (as ``MANORenderer._faces_on`` does), the last ``FACE_CACHE_ENTRIES``
    of them: the first call with a new face list reads it back to the host once to build the table, so keep the face tensors
    (or pass host arrays, which are keyed by content) and warm a renderer up before a graph capture.  The vertex workspace is
    a fresh tensor per call, so captured graphs and several streams can share one renderer."""

    FACE_CACHE_ENTRIES = 16

    def __init__(self, img_res: int = 224, mano_assets=None) -> None:
        self.img_res = int(img_res)
        if self.img_res < 1:
            raise ValueError("Renderer: img_res >= 1 expected")
        self._mano_assets = mano_assets
        self._mano_faces = None
        self._face_cache = collections.OrderedDict()
        self._consts = {}

    # ---- caches
    def _const(self, dev, values):
        """A small float32 constant on the device, uploaded once (a replayed graph must not copy from the host)."""
        key = (str(dev), tuple(float(x) for x in values))
        if key not in self._consts:
            self._consts[key] = torch.tensor(key[1], dtype=torch.float32, device=dev)
        return self._consts[key]

    def _faces_on(self, dev, faces, n_verts):
        """(faces int32 on dev, csr offsets, csr face ids, n_faces) of one face list for meshes of n_verts vertices."""
        if torch.is_tensor(faces) and faces.device.type == "cuda":
            key = (str(dev), "dev", faces.data_ptr(), tuple(faces.shape), faces.dtype, faces._version, int(n_verts))
            hit = self._cached(key)
            if hit is not None:
                return hit[:4]
            host = faces.detach().cpu().numpy()
            keep = faces                                   # held: its storage cannot be recycled under this key
        else:
            host = faces.detach().numpy() if torch.is_tensor(faces) else np.asarray(faces)
            key = (str(dev), "host", host.shape, hash(np.ascontiguousarray(host).tobytes()), int(n_verts))
            hit = self._cached(key)
            if hit is not None:
                return hit[:4]
            keep = None
        off, ids = build_vertex_face_csr(host, n_verts)
        n_faces = host.shape[0]
        host = np.ascontiguousarray(host.astype(np.int32)) if n_faces else np.zeros((1, 3), np.int32)   # never a null pointer
        entry = (torch.from_numpy(host).to(dev), torch.from_numpy(off).to(dev),
                 torch.from_numpy(ids if ids.size else np.zeros(1, np.int32)).to(dev), n_faces, keep)
        self._face_cache[key] = entry
        while len(self._face_cache) > self.FACE_CACHE_ENTRIES:
            self._face_cache.popitem(last=False)           # the least recently used; its pinned tensor is released
        return entry[:4]

    def _cached(self, key):
        hit = self._face_cache.get(key)
        if hit is not None:
            self._face_cache.move_to_end(key)
        return hit

    def mano_faces(self):
        if self._mano_faces is None:
            self._mano_faces = mano_face_lists(self._mano_assets)
        return self._mano_faces

    # ---- the call
    @torch.no_grad()
    def render_meshes_pose(self, verts, faces, K, image=None, colors=None, metallic=0.1, cam_transl=None,
                           sideview_angle=None, valid=None, return_float=False):
        """rend_utils.py:41-101 for a batch.  verts: list of M <= 4 tensors (B, N_m, 3) fp32 in the camera frame; faces: list of
        (F_m, 3) integer tensors / arrays shared by the batch; K (B, 3, 3) or (3, 3) in pixels of the img_res image; image
        (B, 3, S, S) in [0, 1] or None (white); colors: one 0-255 RGB triple per mesh; metallic: a number or one per mesh;
        cam_transl (3,) or (B, 3), added to the vertices; sideview_angle in degrees (see :func:`sideview_transform`; the anchor
        is the last mesh that is valid for the image); valid: list of (B,) tensors or None entries, 0 = the mesh is absent.
        Returns uint8 (B, S, S, 3); with ``return_float`` a dict of ``rgb`` (B, S, S, 3) float, ``image`` uint8, ``depth``
        (B, S, S), 0 where empty, and ``face_id`` (B, S, S) int32, -1 where empty, else the face index plus the face counts of
        the meshes before it.  Fresh tensors, ordered on the current stream."""
        if torch.is_tensor(verts):
            verts, faces = [verts], [faces]
        verts, faces = list(verts), list(faces)
        M, S = len(verts), self.img_res
        if not 1 <= M <= SHADE_MAX_MESHES or len(faces) != M:
            raise ValueError(f"render_meshes_pose: 1..{SHADE_MAX_MESHES} meshes with one face list each expected, got {M} / {len(faces)}")
        for v in verts:
            if not torch.is_tensor(v) or v.dim() != 3 or v.shape[2] != 3 or v.shape[1] < 1 or v.shape[0] != verts[0].shape[0]:
                raise ValueError("render_meshes_pose: every verts entry must be a (B, N, 3) tensor with the same B")
        for f in faces:
            if tuple(f.shape)[1:] != (3,) or len(f.shape) != 2:
                raise ValueError(f"render_meshes_pose: faces (F, 3) expected, got {tuple(f.shape)}")
        B = verts[0].shape[0]
        if not torch.is_tensor(K) or K.shape not in ((B, 3, 3), (3, 3)):
            raise ValueError(f"render_meshes_pose: K (B, 3, 3) or (3, 3) expected, got {tuple(getattr(K, 'shape', ()))}")
        if image is not None and (not torch.is_tensor(image) or image.shape != (B, 3, S, S)):
            raise ValueError(f"render_meshes_pose: image ({B}, 3, {S}, {S}) expected, got {tuple(getattr(image, 'shape', ()))}")
        colors = list(DEFAULT_COLORS[:M]) if colors is None else list(colors)
        metallic = [float(metallic)] * M if not isinstance(metallic, (list, tuple)) else [float(x) for x in metallic]
        valid = [None] * M if valid is None else list(valid)
        if len(colors) != M or len(metallic) != M or len(valid) != M or any(len(c) != 3 for c in colors):
            raise ValueError("render_meshes_pose: one RGB colour, one metallic factor and one valid entry per mesh expected")
        for vl in valid:
            if vl is not None and (not torch.is_tensor(vl) or vl.shape != (B,)):
                raise ValueError(f"render_meshes_pose: valid entries must be ({B},) tensors or None")
        if any(v.device.type != "cuda" for v in verts):
            raise RuntimeError("hands_amd.Renderer runs on a HIP device only (no CPU fallback)")
        dev = verts[0].device
        others = [K, image] + verts + [vl for vl in valid if vl is not None]
        if any(t is not None and t.device != dev for t in others):
            raise RuntimeError("hands_amd.Renderer: verts, K, image and valid must be on the same HIP device")

        verts = [v.detach().to(torch.float32).contiguous() for v in verts]
        valid = [None if vl is None else vl.detach().to(torch.float32).contiguous() for vl in valid]
        K = K.detach().to(torch.float32).expand(B, 3, 3).contiguous()
        image = None if image is None else image.detach().to(torch.float32).contiguous()
        T = None
        if cam_transl is not None:
            if torch.is_tensor(cam_transl):
                cam_transl = cam_transl.detach().to(dev, torch.float32)
            else:
                cam_transl = self._const(dev, np.asarray(cam_transl, np.float64).reshape(-1))
            if cam_transl.shape not in ((3,), (B, 3)):
                raise ValueError(f"render_meshes_pose: cam_transl (3,) or ({B}, 3) expected, got {tuple(cam_transl.shape)}")
        if sideview_angle is not None:
            center = verts[0].mean(dim=1)
            for v, vl in zip(verts[1:], valid[1:]):        # the last valid mesh is the anchor; no host sync
                c = v.mean(dim=1)
                center = c if vl is None else torch.where(vl[:, None] != 0, c, center)
            T = _rigid_about(center, self._const(dev, _rotation_values(sideview_angle)).reshape(3, 3), cam_transl).contiguous()
        elif cam_transl is not None:
            eye = self._const(dev, (1, 0, 0, 0, 1, 0, 0, 0, 1)).reshape(3, 3)
            T = torch.cat([eye.expand(B, 3, 3), cam_transl.expand(B, 3).unsqueeze(-1)], dim=-1).contiguous()

        out = {"rgb": torch.empty(B, S, S, 3, device=dev) if return_float else None,
               "image": torch.empty(B, S, S, 3, device=dev, dtype=torch.uint8),
               "depth": torch.empty(B, S, S, device=dev) if return_float else None,
               "face_id": torch.empty(B, S, S, device=dev, dtype=torch.int32) if return_float else None}
        if B == 0:
            return out if return_float else out["image"]
        L = _lib.lib()
        tables = [self._faces_on(dev, f, v.shape[1]) for f, v in zip(faces, verts)]
        sizes = [int(L.hands_mesh_workspace_floats(B, v.shape[1])) for v in verts]
        ws = torch.empty(max(sum(sizes), 1), dtype=torch.float32, device=dev)
        scene = _lib.ShadeScene()
        scene.n_meshes = M
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            at = face_offset = 0
            for m, (v, (fd, off, ids, Fm)) in enumerate(zip(verts, tables)):
                N = v.shape[1]
                check(L.hands_mesh_prepare_f32(ptr(v), 3 * N, N, ptr(fd), Fm, ptr(off), ptr(ids), ptr(K), ptr(T), B, S,
                                               ptr(ws, at), stream), "hands_mesh_prepare_f32")
                sm = scene.mesh[m]
                sm.workspace, sm.faces, sm.valid = ptr(ws, at), ptr(fd), ptr(valid[m])
                sm.n_verts, sm.n_faces, sm.face_offset = N, Fm, face_offset
                sm.color[0], sm.color[1], sm.color[2] = (float(x) / 255.0 for x in colors[m])
                sm.metallic, sm.roughness = metallic[m], 1.0
                at += sizes[m]
                face_offset += Fm
            check(L.hands_render_shaded_f32(scene, ptr(image), B, S, ptr(out["rgb"]), ptr(out["image"]), ptr(out["depth"]),
                                            ptr(out["face_id"]), stream), "hands_render_shaded_f32")
        return out if return_float else out["image"]

    @torch.no_grad()
    def visualize_rend(self, verts_r, verts_l, K, images, faces_r=None, faces_l=None, right_valid=None, left_valid=None):
        """visualize_arctic.py:199-271 with ``only_hands``: the overlay on ``images`` (B, 3, S, S in [0, 1]), then the side views
        at 45, 172.5 and 300 degrees without a background, stacked to (B, 4 S, S, 3) uint8.  An image with no valid mesh gives
        floor(255 image) four times."""
        fr, fl = self.mano_faces() if faces_r is None or faces_l is None else (None, None)
        faces = [faces_r if faces_r is not None else fr, faces_l if faces_l is not None else fl]
        kw = dict(colors=[COLOR_RIGHT, COLOR_LEFT], metallic=0.1, valid=[right_valid, left_valid])
        panels = [self.render_meshes_pose([verts_r, verts_l], faces, K, image=images, **kw)]
        for angle in SIDEVIEW_ANGLES:
            panels.append(self.render_meshes_pose([verts_r, verts_l], faces, K, image=None, sideview_angle=angle, **kw))
        if right_valid is not None and left_valid is not None:
            none = ((right_valid == 0) & (left_valid == 0)).to(panels[0].device)[:, None, None, None]
            panels = panels[:1] + [torch.where(none, panels[0], p) for p in panels[1:]]
        return torch.cat(panels, dim=1)

    @torch.no_grad()
    def render_hands(self, pred, meta_info=None, images=None, flag=None, right_valid=None, left_valid=None):
        """From a model output -- or the merged dict of ``HandsWrapper(mode="vis")``, whose keys start with ``pred.`` /
        ``targets.`` (``flag`` picks which, "pred" by default) -- to the four-panel pictures of :meth:`visualize_rend`.
        ``images``: normalised ``inputs.img`` (taken from the vis dict when not given); it goes through
        :func:`denormalize_images` and is resized bilinearly (align_corners=True) when its size differs from img_res.  The face
        lists come from ``meta_info["mano.faces.{r,l}"]``, else from the MANO assets."""
        def find(d, names):
            for n in names:
                if d is not None and n in d:
                    return d[n]
            return None
        flags = [flag] if flag is not None else ["pred", "targets"]
        pre = [f"{fl}." for fl in flags] + [""]
        v_r = find(pred, [p + "mano.v3d.cam.r" for p in pre] + ["v3d.cam.r"])
        v_l = find(pred, [p + "mano.v3d.cam.l" for p in pre] + ["v3d.cam.l"])
        if v_r is None or v_l is None:
            raise KeyError("mano.v3d.cam.r / mano.v3d.cam.l")
        K = find(meta_info, ["intrinsics"])
        K = K if K is not None else find(pred, ["meta_info.intrinsics"])
        if K is None:
            raise KeyError("intrinsics")
        f_r = find(meta_info, ["mano.faces.r"])
        f_r = f_r if f_r is not None else find(pred, ["meta_info.mano.faces.r"])
        f_l = find(meta_info, ["mano.faces.l"])
        f_l = f_l if f_l is not None else find(pred, ["meta_info.mano.faces.l"])
        images = images if images is not None else find(pred, ["inputs.img"])
        if images is None:
            raise KeyError("inputs.img")
        S = self.img_res
        images = denormalize_images(images.to(v_r.device, torch.float32))
        if tuple(images.shape[-2:]) != (S, S):
            images = F_.interpolate(images, size=(S, S), mode="bilinear", align_corners=True)
        return self.visualize_rend(v_r, v_l, K.to(v_r.device), images.clamp(0.0, 1.0), f_r, f_l, right_valid, left_valid)
