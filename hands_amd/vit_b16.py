"""Parameter containers of the ViT-B/16 backbone of hands_light (``HandsLight(backbone='vit_b_16')``).

The reference builds ``torchvision.models.vit_b_16`` (src/models/hands_light/model.py:25-29, 45-58) and ``vit_conv()``
(src/nets/backbone/utils.py:27-34).  These classes carry the same ``state_dict`` names and shapes -- torchvision's published
module layout: ``class_token``, ``conv_proj``, ``encoder.pos_embedding``, ``encoder.layers.encoder_layer_{i}.{ln_1,
self_attention, ln_2, mlp.0, mlp.3}``, ``encoder.ln``, ``heads.head`` -- and are never called: the forward is
``HandsLight._trunk_vit`` on the kernels of ``libhands_hip.so``.  No weights are fetched (the reference's
``weights='DEFAULT'`` is a download): the containers are filled by ``load_state_dict`` or ``apply_recipe``.
"""
from __future__ import annotations

from collections import OrderedDict

import torch
import torch.nn as nn

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
