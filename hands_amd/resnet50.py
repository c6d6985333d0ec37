"""The ResNet-50 trunk of hands_light (src/nets/backbone/resnet.py:99-280): parameter containers, packing (BatchNorm folded)
and the runner on the kernels of ``libhands_hip.so``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import check, ptr
from .packing import fold_bn, pack_conv, pack_conv1x1_dual, pack_linear

RESNET50_LAYERS = (3, 4, 6, 3)


# parameter containers (names = the reference's state_dict keys; never called)
class _Bottleneck(nn.Module):
    """resnet.py:99-154 parameter layout (conv1/bn1/conv2/bn2/conv3/bn3/downsample.{0,1})."""

    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.stride = stride
        if downsample:
            self.downsample = nn.Sequential(nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                            nn.BatchNorm2d(planes * 4))
        else:
            self.downsample = None


class ResNet50Params(nn.Module):
    """resnet.py:157-280 parameter layout of the ResNet-50 trunk (no avgpool/fc)."""

    def __init__(self, in_ch=3):
        super().__init__()
        self.conv1 = nn.Conv2d(in_ch, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        inplanes = 64
        for li, (planes, n) in enumerate(zip((64, 128, 256, 512), RESNET50_LAYERS), start=1):
            blocks = []
            for bi in range(n):
                stride = 2 if (bi == 0 and li > 1) else 1
                blocks.append(_Bottleneck(inplanes, planes, stride, downsample=(bi == 0)))
                inplanes = planes * 4
            setattr(self, f"layer{li}", nn.Sequential(*blocks))


@torch.no_grad()
def pack_resnet50_trunk(net: ResNet50Params, dev, winograd4_stages):
    """The trunk in kernel layout; the stride-1 3x3 layers of ``winograd4_stages`` also get their Winograd F(4x4,3x3) form."""
    cpu = lambda t: t.detach().cpu()
    bnp = lambda bn: (cpu(bn.weight), cpu(bn.bias), cpu(bn.running_mean), cpu(bn.running_var))
    P = {}
    w, b = fold_bn(cpu(net.conv1.weight), *bnp(net.bn1))
    if w.shape[1] == 3:
        P["stem"] = pack_conv(w, b, 2, 3, dev, cin_pad_to=4)
        # planar form for hands_stem_conv_maxpool_nchw_f32: k = plane * 52 + tap (49 taps + 3 zero columns per plane)
        col = [c * 52 + t for c in range(3) for t in range(49)]
        P["stem_planar"] = pack_linear(w.reshape(64, 147), b, dev, col_index=col, k_total=160)
        P["stem_planar"].macs_per_pixel = 64 * 147
    else:
        # widened conv1 (image-level encodings): the general implicit-GEMM route on an NHWC input whose channel count is
        # padded to a multiple of 16 (hands_image_posenc_nhwc_f32 writes the zeros)
        P["stem_wide"] = pack_conv(w, b, 2, 3, dev, cin_pad_to=(w.shape[1] + 15) // 16 * 16)
    blocks = []
    for li in range(1, 5):
        for blk in getattr(net, f"layer{li}"):
            e = {}
            w, b = fold_bn(cpu(blk.conv1.weight), *bnp(blk.bn1)); e["c1"] = pack_conv(w, b, 1, 0, dev)
            w, b = fold_bn(cpu(blk.conv2.weight), *bnp(blk.bn2))
            e["c2"] = pack_conv(w, b, blk.stride, 1, dev, winograd4=li in winograd4_stages)
            w, b = fold_bn(cpu(blk.conv3.weight), *bnp(blk.bn3)); e["c3"] = pack_conv(w, b, 1, 0, dev)
            if blk.downsample is not None:
                w, b = fold_bn(cpu(blk.downsample[0].weight), *bnp(blk.downsample[1]))
                e["ds"] = pack_conv(w, b, blk.stride, 0, dev)
                # conv3 + downsample as ONE GEMM over K = planes + inplanes (hands_conv1x1_dual_nhwc_f32)
                w3, b3 = fold_bn(cpu(blk.conv3.weight), *bnp(blk.bn3))
                e["c3ds"] = pack_conv1x1_dual(w3, b3, w, b, dev)
                e["c3ds_split"] = (w3.shape[1], w.shape[1], blk.stride)
            blocks.append(e)
    P["blocks"] = blocks
    return P


def _blocks(engine, L, blocks, cur, nxt, t1, t2, ds, B, H, W, stream, final_dst, final_off):
    """A run of bottlenecks (resnet.py:134-154) on ping-pong buffers; the last one writes ``final_dst``
    at float offset ``final_off``.  Returns (H, W) of the output map."""
    n = len(blocks)
    for i, e in enumerate(blocks):
        engine.conv(L, e["c1"], cur, B, H, W, t1, True, stream)
        last = i + 1 == n
        dst, off = (final_dst, final_off) if last else (nxt, 0)
        H2, W2 = engine.conv(L, e["c2"], t1, B, H, W, t2, True, stream)
        if "ds" in e and engine.fuse_downsample:
            engine.conv_dual(L, e["c3ds"], e["c3ds_split"], t2, cur, B, H2, W2, H, W, dst, stream, out_off=off)
        else:
            if "ds" in e:
                engine.conv(L, e["ds"], cur, B, H, W, ds, False, stream)
                ident = ds
            else:
                ident = cur
            engine.conv(L, e["c3"], t2, B, H2, W2, dst, True, stream, res=ident, out_off=off)
        H, W = H2, W2
        cur, nxt = dst, cur
    return H, W


def resnet50_trunk(engine, buf, L, P, segs, B, res_in, stream, tag, cap_B, out=None, out_off=0):
    """ResNet-50 trunk on B images given as NCHW segments ``[(tensor, first image, n images), ...]`` (the
    reference's input layout, read in place); returns (B,7,7,2048) features (flat tensor).  ``buf(name, numel)`` is the
    model's workspace allocator.
    (Running stem + layer1 + layer2 per sub-batch of 32-128 images, to keep their HBM-bound 1x1 layers'
    tensors inside the 256 MB Infinity Cache, was measured 1-18 % SLOWER than whole-job launches.)"""
    per = 112 * 112 * 64 * (res_in * res_in) // (224 * 224) + 64      # floats per image of the largest map
    cap = cap_B * per
    a = buf("trunk_a_" + tag, cap); b = buf("trunk_b_" + tag, cap)
    t1 = buf("trunk_t1_" + tag, cap); t2 = buf("trunk_t2_" + tag, cap)
    ds = buf("trunk_ds_" + tag, cap)
    Hs, Ws = (res_in - 1) // 2 + 1, (res_in - 1) // 2 + 1                # stem conv map
    Hp, Wp = (Hs + 2 - 3) // 2 + 1, (Ws + 2 - 3) // 2 + 1                # after the max-pool
    img_floats = 3 * res_in * res_in
    done = 0
    for src, first, n in segs:
        if "stem_wide" in P:
            # widened conv1 (image-level encodings): `src` is the NHWC (.., res, res, Cpad) tensor hands_image_posenc_nhwc_f32
            # wrote; general implicit GEMM + the max-pool kernel
            Cp = P["stem_wide"].Cin
            engine.conv(L, P["stem_wide"], src, n, res_in, res_in, a, True, stream, x_off=first * res_in * res_in * Cp)
            check(L.hands_maxpool3x3s2_nhwc_f32(ptr(a), ptr(b, done * Hp * Wp * 64), n, Hs, Ws, 64, stream), "maxpool")
        elif engine.fuse_stem_pool:
            # conv1 + bn1 + relu + maxpool in one kernel straight from the NCHW image: neither the NHWC copy
            # of the input nor the 112x112x64 map ever reaches HBM
            engine.stem_pool_nchw(L, P["stem_planar"], src, first * img_floats, b, done * Hp * Wp * 64, n,
                                  res_in, res_in, 1, stream)
        else:
            x4 = buf("trunk_x4_" + tag, cap_B * res_in * res_in * 4)
            check(L.hands_nchw3_to_nhwc4_f32(ptr(src, first * img_floats), ptr(x4), n, res_in, res_in, stream), "nchw->nhwc4")
            engine.conv(L, P["stem"], x4, n, res_in, res_in, a, True, stream)
            check(L.hands_maxpool3x3s2_nhwc_f32(ptr(a), ptr(b, done * Hp * Wp * 64), n, Hs, Ws, 64, stream), "maxpool")
        done += n
    assert done == B
    feat = out if out is not None else buf("feat_" + tag, B * 49 * P["blocks"][-1]["c3"].Cout)
    H, W = _blocks(engine, L, P["blocks"], b, a, t1, t2, ds, B, Hp, Wp, stream, feat, out_off)
    return feat, H, W
