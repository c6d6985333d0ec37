"""The grasp classifier the three models share (src/models/hands_light/model.py:113-125, 401-411; hamer_light/model.py:59-72,
136-143; handoccnet_light/model.py:103-120): a four-layer MLP on ``cat([shape 10, rot 144(, feat_vec)])`` of both hands.
"""
from __future__ import annotations

import torch

from ._lib import ACT_NONE, ACT_RELU, check, ptr
from .engine import linear_chain
from .packing import pack_linear
from .xdict import xdict

# Which of the four layers each model marks ``splitk`` (rows per sample: the library may cut K by its layer-only policy).  The
# differences are historical and DELIBERATELY kept: g4 has K = 512, which the policy cuts in two when the layer is marked, so
# HandOccNet sums g4 in another order than the other two models -- marking or unmarking a layer changes output bits.
GRASP_SPLITK = {               # g0     g2     g4     g6
    "hands_light":              (True,  True,  True,  False),
    "hamer":                    (True,  True,  True,  True),
    "handoccnet":               (True,  True,  False, False),
}


def pack_grasp_head(linears, dev, feat=0, lin=None):
    """The four Linear layers of ``grasp_classifier`` -> packed layers [g0, g2, g4, g6].  The reference's input row
    cat([shape 10, rot 144(, feat_vec ``feat``)]) becomes the packed row [feat_vec | rot 144 | shape 10] (16-byte aligned
    segments), and the 9 logits are stored 12 wide.  ``lin(layer, **kw)`` packs one element of ``linears`` (default: an
    ``nn.Linear`` through ``pack_linear``); a model with per-stage layer flags passes its own."""
    if lin is None:
        lin = lambda m, **kw: pack_linear(m.weight.detach().cpu(), m.bias.detach().cpu(), dev, **kw)
    gcol = [feat + 144 + i for i in range(10)] + [feat + i for i in range(144)] + list(range(feat))
    g0, g2, g4, g6 = linears
    return [lin(g0, col_index=gcol, k_total=feat + 154), lin(g2), lin(g4), lin(g6, n_total=12)]


def run_grasp_head(engine, L, G, splitk, shape, rot, bz, stream, buf, shape_ld=10, shape_off=0, feat=None, feat_dim=0):
    """``grasp_classifier`` on the 2 bz rows of ``shape`` (row length ``shape_ld``, first column ``shape_off``), ``rot``
    (2bz, 144) and, with ``feat_dim`` > 0, the bz rows of ``feat`` (both hands of a sample read the same row): the input row
    (hands_grasp_input_f32), the four layers ``G`` of :func:`pack_grasp_head` with the flags ``splitk`` (a row of
    ``GRASP_SPLITK``), and the xdict {grasp.r, grasp.l} of (bz, 9) logits."""
    B2, gld = 2 * bz, G[0].Cin
    gin = buf("grasp_in", B2 * gld)
    check(L.hands_grasp_input_f32(ptr(shape, shape_off), shape_ld, ptr(rot), ptr(shape if feat is None else feat), ptr(gin), B2, bz,
                                  feat_dim, gld, stream), "grasp_input")
    g4 = torch.empty(B2, 12, dtype=torch.float32, device=gin.device)
    acts = (ACT_RELU, ACT_RELU, ACT_RELU, ACT_NONE)
    linear_chain(engine, L, list(zip(G, acts, splitk)), gin, B2, stream, buf, ("g1", "g2", "g3"), out=g4)
    grasp = xdict()
    grasp["grasp.r"] = g4[:bz, :9].contiguous()
    grasp["grasp.l"] = g4[bz:, :9].contiguous()
    return grasp
