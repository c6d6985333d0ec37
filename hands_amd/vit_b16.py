"""The ViT-B/16 backbone of hands_light (``HandsLight(backbone='vit_b_16')``): parameter containers, packing and runner.

The reference builds ``torchvision.models.vit_b_16`` (src/models/hands_light/model.py:25-29, 45-58) and ``vit_conv()``
(src/nets/backbone/utils.py:27-34).  These classes carry the same ``state_dict`` names and shapes -- torchvision's published
module layout: ``class_token``, ``conv_proj``, ``encoder.pos_embedding``, ``encoder.layers.encoder_layer_{i}.{ln_1,
self_attention, ln_2, mlp.0, mlp.3}``, ``encoder.ln``, ``heads.head`` -- and are never called: the forward is
``vit_b16_trunk`` on the kernels of ``libhands_hip.so``.  No weights are fetched (the reference's
``weights='DEFAULT'`` is a download): the containers are filled by ``load_state_dict`` or ``apply_recipe``.
"""
from __future__ import annotations

import types
from collections import OrderedDict

import torch
import torch.nn as nn

from ._lib import check, ptr
from .packing import BN_EPS, pack_conv, pack_linear
from .vit_encoder import vit_encoder_blocks

VITB_DIM, VITB_HEADS, VITB_HDIM, VITB_DEPTH, VITB_MLP = 768, 12, 64, 12, 3072
VITB_PATCH, VITB_RES = 16, 224
VITB_GRID = VITB_RES // VITB_PATCH            # 14 x 14 patches
VITB_TOKENS = 1 + VITB_GRID * VITB_GRID       # 197 with the class token
VITB_LN_EPS = 1e-6


class _EncoderBlockParams(nn.Module):
    """EncoderBlock: ln_1 -> self_attention (nn.MultiheadAttention, batch_first) -> + ; ln_2 -> mlp (Linear, GELU, Dropout,
    Linear, Dropout) -> +."""

    def __init__(self):
        super().__init__()
        self.ln_1 = nn.LayerNorm(VITB_DIM, eps=VITB_LN_EPS)
        self.self_attention = nn.MultiheadAttention(VITB_DIM, VITB_HEADS, dropout=0.0, batch_first=True)
        self.dropout = nn.Dropout(0.0)
        self.ln_2 = nn.LayerNorm(VITB_DIM, eps=VITB_LN_EPS)
        self.mlp = nn.Sequential(nn.Linear(VITB_DIM, VITB_MLP), nn.GELU(), nn.Dropout(0.0), nn.Linear(VITB_MLP, VITB_DIM),
                                 nn.Dropout(0.0))


class _EncoderParams(nn.Module):
    def __init__(self):
        super().__init__()
        self.pos_embedding = nn.Parameter(torch.empty(1, VITB_TOKENS, VITB_DIM).normal_(std=0.02))
        self.dropout = nn.Dropout(0.0)
        self.layers = nn.Sequential(OrderedDict((f"encoder_layer_{i}", _EncoderBlockParams()) for i in range(VITB_DEPTH)))
        self.ln = nn.LayerNorm(VITB_DIM, eps=VITB_LN_EPS)


class ViTB16Params(nn.Module):
    """VisionTransformer(image 224, patch 16, 12 layers, 12 heads, hidden 768, mlp 3072) parameter layout.  ``in_ch`` > 3: the
    widened ``conv_proj`` of the image-level encodings (model.py:60-78).  ``heads.head`` (768 -> 1000) is part of the
    ``state_dict`` and never run (vit_forward stops at the encoder)."""

    def __init__(self, in_ch=3):
        super().__init__()
        self.image_size, self.patch_size, self.hidden_dim = VITB_RES, VITB_PATCH, VITB_DIM
        self.conv_proj = nn.Conv2d(in_ch, VITB_DIM, VITB_PATCH, stride=VITB_PATCH)
        self.class_token = nn.Parameter(torch.zeros(1, 1, VITB_DIM))
        self.encoder = _EncoderParams()
        self.heads = nn.Sequential(OrderedDict(head=nn.Linear(VITB_DIM, 1000)))


def vit_conv_params():
    """utils.py:27-34: AvgPool2d(2) -> Conv2d(768, 2048, 3, padding 1, bias) -> BatchNorm2d -> ReLU (keys ``1.*``, ``2.*``)."""
    return nn.Sequential(nn.AvgPool2d(kernel_size=2, stride=2), nn.Conv2d(VITB_DIM, 2048, 3, stride=1, padding=1),
                         nn.BatchNorm2d(2048), nn.ReLU(inplace=True))


@torch.no_grad()
def pack_vit_b16_trunk(net: ViTB16Params, tail: nn.Sequential, dev):
    """ViT-B/16 + vit_conv in kernel layout (once per load_state_dict, like the ResNet trunk): the patch embedding as a
    16x16 / stride 16 convolution on NHWC4 (or on the padded NHWC map of the widened form), the four linears of every block
    through pack_linear, and vit_conv's Conv2d bias + eval BatchNorm2d folded in fp64 into one 3x3 / pad 1 layer."""
    cpu = lambda t: t.detach().cpu()
    lin = lambda w, b: pack_linear(cpu(w), cpu(b), dev)
    ln = lambda m: (cpu(m.weight).float().contiguous().to(dev), cpu(m.bias).float().contiguous().to(dev))
    P = {"vit": True}
    w, b = cpu(net.conv_proj.weight), cpu(net.conv_proj.bias)
    if w.shape[1] == 3:
        P["patch"] = pack_conv(w, b, 16, 0, dev, cin_pad_to=4)
    else:
        # widened conv_proj (image-level encodings) on the padded NHWC map.  The general implicit GEMM takes kernels of at most
        # 15 x 15 taps when Cin != 4, so the 16 x 16 / stride 16 layer runs as TWO launches on a strip view of the same memory:
        # 16 image rows x 224 pixels x Cp channels are 16 rows x 14 patches x (16 Cp) channels, i.e. every strip of 16 rows is an
        # "image" (H 16, W 14, C 16 Cp) on which the patch embedding is a KH 16 x KW 1 kernel with one output row.  Its upper
        # and lower 8 rows are one launch each (k order (kh, kw, c) is the same in both views); the second adds the first
        # through the residual epilogue.  No copy of the map is made.
        Cp = (w.shape[1] + 15) // 16 * 16
        P["stem_wide"] = types.SimpleNamespace(Cin=Cp)       # what the callers ask: the padded channel count of the map
        P["patch_halves"] = []
        for h0 in (0, 8):
            pc = pack_conv(w[:, :, h0:h0 + 8, :], b if h0 == 0 else None, 1, 0, dev, cin_pad_to=Cp)
            pc.Cin, pc.KH, pc.KW = 16 * Cp, 8, 1             # the strip view of the same packed weight
            P["patch_halves"].append(pc)
    P["cls"] = cpu(net.class_token).float().reshape(VITB_DIM).contiguous().to(dev)
    P["pos"] = cpu(net.encoder.pos_embedding).float().reshape(VITB_TOKENS, VITB_DIM).contiguous().to(dev)
    P["blocks"] = []
    for blk in net.encoder.layers:
        at = blk.self_attention
        P["blocks"].append({"n1": ln(blk.ln_1), "qkv": lin(at.in_proj_weight, at.in_proj_bias),
                            "proj": lin(at.out_proj.weight, at.out_proj.bias), "n2": ln(blk.ln_2),
                            "fc1": lin(blk.mlp[0].weight, blk.mlp[0].bias), "fc2": lin(blk.mlp[3].weight, blk.mlp[3].bias)})
    P["last"] = ln(net.encoder.ln)
    # vit_conv (utils.py:27-34): y = relu(bn(conv(x) + cb)) = relu(conv'(x) + b'), w' = w g / sqrt(var + eps),
    # b' = (cb - mean) g / sqrt(var + eps) + beta, all in fp64 and rounded to fp32 once by pack_conv.  Winograd F(2x2,3x3)
    # weights only: at 1.4 of the trunk's 36 GFLOP the F(4x4) form has nothing to win and its larger rounding error to lose.
    conv, bn = tail[1], tail[2]
    sc = cpu(bn.weight).double() / torch.sqrt(cpu(bn.running_var).double() + BN_EPS)
    wf = cpu(conv.weight).double() * sc[:, None, None, None]
    bf = (cpu(conv.bias).double() - cpu(bn.running_mean).double()) * sc + cpu(bn.bias).double()
    P["vit_conv"] = pack_conv(wf, bf, 1, 1, dev)
    return P


def vit_b16_trunk(engine, buf, L, P, segs, B, res_in, stream, tag, cap_B, out=None, out_off=0):
    """``vit_forward`` (model.py:483-493) on B images given as the segments of ``resnet50_trunk``: same contract, writes
    (B,7,7,2048) NHWC features at float offset ``out_off``.  conv_proj as a 16x16 / stride 16 GEMM -> class token + position
    embedding (hands_vit_tokens_f32) -> 12 encoder blocks (``vit_encoder_blocks``: 197 tokens, 12 heads x 64) -> encoder.ln on
    the patch tokens + 2x2 average (hands_vit_tail_f32) -> vit_conv (3x3, BatchNorm folded, ReLU).  Token-major rows are NHWC
    already: the reference's permute + reshape to (B,768,14,14) never happens.  Workspaces are sized for M = cap_B * 197 rows
    and kept."""
    if res_in != VITB_RES:
        raise ValueError(f"hands_amd.HandsLight: the ViT-B/16 backbone takes {VITB_RES}x{VITB_RES} images, not {res_in}")
    T, Cd, G = VITB_TOKENS, VITB_DIM, VITB_GRID
    capM = cap_B * T
    x = buf("vit_x_" + tag, capM * Cd); y = buf("vit_y_" + tag, capM * Cd)
    att = buf("vit_att_" + tag, capM * Cd)
    qkv = buf("vit_qkv_" + tag, capM * 3 * Cd); hid = buf("vit_h_" + tag, capM * VITB_MLP)
    # -- conv_proj (`_process_input`): patch rows (B,196,768) into `y`, which the first LayerNorm overwrites afterwards
    done = 0
    for src, first, n in segs:
        if "stem_wide" in P:       # NHWC (.., 224, 224, Cpad) map of the image-level encodings: two launches on its strip view
            Cp = P["stem_wide"].Cin
            top, bottom = P["patch_halves"]
            img = res_in * res_in * Cp
            step = max(1, (1 << 31) // img - 1)            # the library indexes one launch's input with 31 bits
            for c0 in range(0, n, step):
                nc = min(step, n - c0)
                xo, oo = (first + c0) * img, (done + c0) * G * G * Cd
                engine.conv(L, top, src, nc * G, 16, G, y, False, stream, x_off=xo, out_off=oo, out_hw=(1, G))
                engine.conv(L, bottom, src, nc * G, 16, G, y, False, stream, x_off=xo + 8 * res_in * Cp, out_off=oo,
                            res=y, res_off=oo, out_hw=(1, G))
            hw = (G, G)
        else:
            x4 = buf("vit_x4_" + tag, cap_B * res_in * res_in * 4)
            check(L.hands_nchw3_to_nhwc4_f32(ptr(src, first * 3 * res_in * res_in), ptr(x4), n, res_in, res_in, stream), "nchw->nhwc4")
            hw = engine.conv(L, P["patch"], x4, n, res_in, res_in, y, False, stream, out_off=done * G * G * Cd)
        assert hw == (G, G)
        done += n
    assert done == B
    check(L.hands_vit_tokens_f32(ptr(y), ptr(P["cls"]), ptr(P["pos"]), ptr(x), B, T, Cd, stream), "vit_tokens")
    vit_encoder_blocks(engine, L, P["blocks"], x, y, qkv, att, hid, B, T, VITB_HEADS, VITB_HDIM, VITB_LN_EPS,
                       float(VITB_HDIM) ** -0.5, stream)
    # -- encoder.ln on tokens 1..196 + AvgPool2d(2) -> (B,7,7,768) in `att`; vit_conv -> the caller's feature rows
    check(L.hands_vit_tail_f32(ptr(x), ptr(P["last"][0]), ptr(P["last"][1]), ptr(att), B, G, Cd, VITB_LN_EPS, stream), "vit_tail")
    feat = out if out is not None else buf("feat_" + tag, B * 49 * P["vit_conv"].Cout)
    H, W = engine.conv(L, P["vit_conv"], att, B, G // 2, G // 2, feat, True, stream, out_off=out_off)
    return feat, H, W
