"""The pre-norm ViT encoder block both ViTs run: ViT-H/16 of hamer_light (vit.py:128-151) and torchvision's ViT-B/16 of
hands_light (``backbone='vit_b_16'``)."""
from __future__ import annotations

from ._lib import ACT_GELU, check, ptr


def vit_encoder_blocks(engine, L, blocks, x, y, qkv, att, hid, B, T, heads, hdim, eps, scale, stream):
    """``x`` (B T, heads hdim) through ``blocks`` in place, seven launches a block: LayerNorm -> qkv GEMM ->
    hands_attention_f32 -> out_proj GEMM + residual -> LayerNorm -> fc1 GEMM + exact GELU -> fc2 GEMM + residual.
    A block is ``{"n1", "n2": (gamma, beta); "qkv", "proj", "fc1", "fc2": PackedConv}``; ``y`` (like x), ``qkv`` (3 x wide),
    ``att`` (like x) and ``hid`` (the MLP width) are the caller's workspaces."""
    M, Cd = B * T, heads * hdim
    conv, layernorm, attention = engine.conv, L.hands_layernorm_f32, L.hands_attention_f32
    px, py = ptr(x), ptr(y)
    for blk in blocks:
        g, b = blk["n1"]
        check(layernorm(px, ptr(g), ptr(b), py, None, 1, M, Cd, eps, stream), "layernorm")
        conv(L, blk["qkv"], y, M, 1, 1, qkv, 0, stream)
        check(attention(ptr(qkv), ptr(att), B, T, heads, hdim, scale, stream), "attention")
        conv(L, blk["proj"], att, M, 1, 1, x, 0, stream, res=x)
        g, b = blk["n2"]
        check(layernorm(px, ptr(g), ptr(b), py, None, 1, M, Cd, eps, stream), "layernorm")
        conv(L, blk["fc1"], y, M, 1, 1, hid, ACT_GELU, stream)
        conv(L, blk["fc2"], hid, M, 1, 1, x, 0, stream, res=x)
