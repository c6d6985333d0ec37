"""The MANO head the three models share (src/nets/hand_heads/mano_head.py:12-65): parameter container, packing of both hands'
assets, the output buffers / dict, and the launch of ``hands_mano_heads_f32`` per call (``run_mano_heads``) or pre-bound
(``ManoHeadsPlan``).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ._lib import ManoConsts, ManoOut, ManoSide, check, ptr
from .engine import DEFAULT_ENGINE
from .mano import ManoLayer, build_mano_asset
from .packing import pack_mano
from .xdict import prefix_dict, xdict


class MANOHead(nn.Module):
    """mano_head.py:12-19: holds the MANO layer as ``.mano``."""

    def __init__(self, is_rhand, focal_length, img_res, asset=None):
        super().__init__()
        self.mano = ManoLayer(asset if asset is not None else build_mano_asset(is_rhand))
        self.focal_length, self.img_res, self.is_rhand = focal_length, img_res, is_rhand

    @property
    def faces(self):
        return self.mano.faces


def mano_consts(m):
    return ManoConsts(ptr(m["pose_mean"]), ptr(m["J_template"]), ptr(m["J_shapedirs"]), ptr(m["lbs_weights"]),
                      ptr(m["tip_ids"]))


def pack_mano_pair(mano_r, mano_l, dev):
    """The packed constants of the right and the left ``MANOHead``, each with its ``consts`` descriptor."""
    pair = []
    for head in (mano_r, mano_l):
        m = pack_mano(head.mano.asset(), dev)
        m["consts"] = mano_consts(m)
        pair.append(m)
    return pair


_MANO_OUT_SHAPES = (("vertices", (778, 3)), ("v3d.cam", (778, 3)), ("joints3d", (21, 3)), ("j3d.cam", (21, 3)),
                    ("j2d.norm", (21, 2)), ("cam_t", (3,)))


def _mano_out_buffers(bz, dev):
    """The twelve output tensors of the two MANO heads as contiguous views of ONE allocation (one allocator call per
    forward); the two vertex arrays come first in each side's 16-byte aligned block (the kernel stores them 8 bytes wide)."""
    side_floats = (bz * 4839 + 3) // 4 * 4
    flat = torch.empty(2 * side_floats, device=dev)
    outs = []
    for side in range(2):
        o, off = {}, side * side_floats
        for name, shp in _MANO_OUT_SHAPES:
            n = bz
            for d_ in shp:
                n *= d_
            o[name] = flat[off:off + n].view((bz,) + shp)
            off += n
        outs.append(o)
    return outs


def _mano_out(o):
    return ManoOut(ptr(o["vertices"]), ptr(o["joints3d"]), ptr(o["v3d.cam"]), ptr(o["j3d.cam"]), ptr(o["j2d.norm"]),
                   ptr(o["cam_t"]))


def _mano_sides(mano_r, mano_l, rot, per, shape, cam, outs, bz):
    """The descriptor array of ``hands_mano_heads_f32``: rows [0, bz) of rot (``per`` floats a row) / shape / cam are the right
    hand's, rows [bz, 2 bz) the left hand's."""
    sides = (ManoSide * 2)()
    for side, mp in enumerate((mano_r, mano_l)):
        ro = side * bz
        sides[side] = ManoSide(mp["consts"], ptr(mp["blend"].w), ptr(mp["blend"].bias), ptr(rot, ro * per),
                               ptr(shape, ro * 10), ptr(cam, ro * 3), _mano_out(outs[side]))
    return sides


def _mano_output_dict(outs, rot, shape, cam, cam_init, bz):
    """Key order of mano_head.py:53-61 + the `cam_t.wp.init` / `mano.` prefixing of model.py:392-399."""
    output = xdict()
    for side, post in enumerate((".r", ".l")):
        ro = side * bz
        o = outs[side]
        md = xdict()
        md["cam_t.wp"] = cam[ro:ro + bz]
        md["cam_t"] = o["cam_t"]
        md["joints3d"] = o["joints3d"]
        md["vertices"] = o["vertices"]
        md["j3d.cam"] = o["j3d.cam"]
        md["v3d.cam"] = o["v3d.cam"]
        md["j2d.norm"] = o["j2d.norm"]
        md["beta"] = shape[ro:ro + bz]
        md["pose"] = rot[ro:ro + bz]
        md = md.postfix(post)
        md["cam_t.wp.init" + post] = cam_init[ro:ro + bz]       # model.py:392-393
        output.merge(prefix_dict(md, "mano."))                  # model.py:395-399
    return output


class ManoHeadsPlan:
    """``MANOHead.forward`` of both hands as ONE pre-bound C-ABI call (BASELINE configs[4], a serving loop over fixed
    buffers): the descriptor array of ``hands_mano_heads_f32`` -- input pointers, the twelve output views, both assets'
    constants -- is built once; ``launch(stream)`` is the single ctypes call per step and ``outputs`` the (fixed) result
    dict.  The caller owns ``rot`` (2bz,16,3,3) [or (2bz,48) axis-angle with ``aa_input``], ``shape`` (2bz,10),
    ``cam`` (2bz,3), ``K`` (bz,3,3) and rewrites them in place between steps."""

    def __init__(self, L, mano_r, mano_l, rot, shape, cam, K, img_res, bz, aa_input=False, cam_init=None):
        per = 48 if aa_input else 144
        assert rot.is_contiguous() and shape.is_contiguous() and cam.is_contiguous() and K.is_contiguous()
        assert rot.numel() == 2 * bz * per and shape.numel() == 2 * bz * 10 and cam.numel() == 2 * bz * 3 and K.numel() == bz * 9
        self.L, self.bz, self.img_res, self.aa = L, bz, float(img_res), int(bool(aa_input))
        self._keep = (mano_r, mano_l, rot, shape, cam, K)
        self._outs = _mano_out_buffers(bz, rot.device)
        self._sides = _mano_sides(mano_r, mano_l, rot, per, shape, cam, self._outs, bz)
        self._K = ptr(K)
        self.outputs = _mano_output_dict(self._outs, rot, shape, cam, cam if cam_init is None else cam_init, bz)

    def launch(self, stream):
        check(self.L.hands_mano_heads_f32(self._sides, 2, self._K, 10, self.img_res, 0.1, self.bz, self.aa, stream), "mano_heads")
        return self.outputs


def run_mano_heads(L, mano_r, mano_l, rot, shape, cam, cam_init, K, img_res, bz, stream, buf, engine=None):
    """MANOHead.forward for the right (rows [0,bz)) and left (rows [bz,2bz)) hands
    (src/nets/hand_heads/mano_head.py:21-65) + the `cam_t.wp.init` / `mano.` prefixing of
    model.py:392-399.  rot (2bz,16,3,3), shape (2bz,10), cam / cam_init (2bz,3), K (bz,3,3).
    One launch for both hands (hands_mano_heads_f32); ``engine.fuse_mano = False`` keeps the three-launch
    chain per side (pose -> blend GEMM -> skin), which the tests compare it with."""
    engine = engine or DEFAULT_ENGINE
    outs = _mano_out_buffers(bz, rot.device)
    if getattr(engine, "fuse_mano", True):
        sides = _mano_sides(mano_r, mano_l, rot, 144, shape, cam, outs, bz)
        check(L.hands_mano_heads_f32(sides, 2, ptr(K), 10, img_res, 0.1, bz, 0, stream), "mano_heads")
    else:
        blend_in = buf("blend_in", bz * 160)
        Abuf, j16 = buf("mano_A", bz * 192), buf("mano_j16", bz * 48)
        vposed = buf("vposed", bz * 2336)
        for side, mp in enumerate((mano_r, mano_l)):
            ro = side * bz
            check(L.hands_mano_pose_f32(C.byref(mp["consts"]), ptr(rot, ro * 144), ptr(shape, ro * 10), 10,
                                        ptr(blend_in), 160, ptr(Abuf), ptr(j16), bz, stream), "mano_pose")
            engine.conv(L, mp["blend"], blend_in, bz, 1, 1, vposed, False, stream)
            check(L.hands_mano_skin_f32(C.byref(mp["consts"]), ptr(vposed), 2336, ptr(Abuf), ptr(j16),
                                        ptr(cam, ro * 3), ptr(K), img_res, 0.1, C.byref(_mano_out(outs[side])), bz, stream),
                  "mano_skin")
    return _mano_output_dict(outs, rot, shape, cam, cam_init, bz)


run_mano_heads.launches_per_step = 1


def run_mano_heads_from_pred(L, mano_r, mano_l, pred, K, img_res, bz, stream, buf, engine=None):
    """The regressor tail of hamer_light / handoccnet_light: ``pred`` (2bz, 112) rows [pose_6d 96 | shape 10 | 2 pad | cam 3 |
    1 pad] -> rotation matrices (rot6d read by columns, geometry.py:47-62), shape and cam slices -> ``run_mano_heads`` (cam is
    its own `cam_t.wp.init`).  Returns (output, rot, shape): the grasp head reads the last two."""
    rot = torch.empty(2 * bz, 16, 3, 3, dtype=torch.float32, device=pred.device)
    check(L.hands_rot6d_to_matrix_cols_f32(ptr(pred), 112, ptr(rot), 2 * bz, stream), "rot6d_cols")
    shape = pred[:, 96:106].contiguous()
    cam = pred[:, 108:111].contiguous()
    return run_mano_heads(L, mano_r, mano_l, rot, shape, cam, cam, K, img_res, bz, stream, buf, engine), rot, shape
