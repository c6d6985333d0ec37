"""The heads of hands_light that read the 7x7 feature map: ``HandHMR`` (src/nets/hand_heads/hand_hmr.py:9-92,
src/nets/hmr_layer.py:7-86) -- parameter containers, packing, the iterative head ``iter_head`` and the transformer head ``tf_head``
(tf_decoder=True), both per hand on one stream -- and the depth head
(src/models/hands_light/model.py:133-155, 177-185).  The runners take the model's ``engine`` and its workspace allocator
``buf(name, numel)``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ._lib import check, ptr
from .engine import linear_chain
from .packing import HMR_VEC, hmr_state_columns, pack_hmr_decoders, pack_linear


# parameter containers (names = the reference's state_dict keys; never called)
class _HMRLayerParams(nn.Module):
    """hmr_layer.py:7-62 (tf_decoder=False)."""

    def __init__(self, feat_dim, mid_dim, specs):
        super().__init__()
        hmr_dim = feat_dim + sum(specs.values())
        self.refine = nn.Sequential(nn.Linear(hmr_dim, mid_dim), nn.ReLU(), nn.Dropout(),
                                    nn.Linear(mid_dim, mid_dim), nn.ReLU(), nn.Dropout())
        self.decoders = nn.ModuleDict({k: nn.Linear(mid_dim, v) for k, v in specs.items()})


class _MHAParams(nn.Module):
    """nn.MultiheadAttention's parameter layout (packed in_proj rows [q | k | v], out_proj as a Linear)."""

    def __init__(self, dim):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * dim, dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * dim))
        self.out_proj = nn.Linear(dim, dim)
        nn.init.xavier_uniform_(self.in_proj_weight)


class _TFLayerParams(nn.Module):
    """hands_light/transformer.py:398-415 (encoder layer) / :601-622 (decoder layer: + multihead_attn, norm3).  The norms are
    never applied (the head runs both layers with no_norm=True) but stay in the state_dict, as in the reference."""

    def __init__(self, dim, cross):
        super().__init__()
        self.self_attn = _MHAParams(dim)
        if cross:
            self.multihead_attn = _MHAParams(dim)
        self.linear1 = nn.Linear(dim, dim)
        self.linear2 = nn.Linear(dim, dim)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        if cross:
            self.norm3 = nn.LayerNorm(dim)


class _TFStack(nn.Module):
    """TransformerDecoder / TransformerEncoder with num_layers=1: ``layers.0``."""

    def __init__(self, dim, cross):
        super().__init__()
        self.layers = nn.ModuleList([_TFLayerParams(dim, cross)])


class _HMRLayerTFParams(nn.Module):
    """hmr_layer.py:7-62 with tf_decoder=True: ``refine`` is replaced by the token embeddings, one decoder layer over the
    feature pixels and one encoder layer; ``in_dim`` is the channel count of the map the head reads."""

    def __init__(self, in_dim, mid_dim, specs):
        super().__init__()
        self.vector_mlp = nn.Sequential(nn.Linear(1, mid_dim), nn.ReLU())
        self.feat_mlp = nn.Sequential(nn.Linear(in_dim, mid_dim), nn.ReLU())
        self.refine_decoder = _TFStack(mid_dim, cross=True)
        self.self_attn = _TFStack(mid_dim, cross=False)
        self.decoders = nn.ModuleDict({k: nn.Linear(mid_dim, v) for k, v in specs.items()})


TF_TOKENS = 109      # one token per scalar of the vectors, in `init_vector_dict` order: pose_6d 96, shape 10, cam_t/wp 3
TF_DIM = 1024        # d_model of the head's layers = its single head's dimension
TF_PASS = 256        # samples per pass of the transformer head (the (109 n, 3072) in_proj output of 256 samples is 343 MB)


class HandHMR(nn.Module):
    """hand_hmr.py:9-44 parameter layout.  ``tf_in``: tf_decoder=True, the head reads a (tf_in, 7, 7) map."""

    def __init__(self, feat_dim, is_rhand, n_iter, tf_in=None):
        super().__init__()
        self.is_rhand, self.n_iter = is_rhand, n_iter
        self.hand_specs = {"pose_6d": 96, "cam_t/wp": 3, "shape": 10}
        if tf_in is None:
            self.hmr_layer = _HMRLayerParams(feat_dim, 1024, self.hand_specs)
        else:
            self.hmr_layer = _HMRLayerTFParams(tf_in, TF_DIM, self.hand_specs)
            self.cam_init_precursor = nn.Sequential(nn.Linear(tf_in, feat_dim), nn.ReLU())
        self.cam_init = nn.Sequential(nn.Linear(feat_dim, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU(),
                                      nn.Linear(512, 3))


@torch.no_grad()
def pack_hmr_head(head: HandHMR, dev, feat_dim, tf_decoder):
    cpu = lambda t: t.detach().cpu()
    F = feat_dim
    P = {}
    ci = head.cam_init
    P["ci0"] = pack_linear(cpu(ci[0].weight), cpu(ci[0].bias), dev)
    P["ci2"] = pack_linear(cpu(ci[2].weight), cpu(ci[2].bias), dev)
    P["ci4"] = pack_linear(cpu(ci[4].weight), cpu(ci[4].bias), dev, n_total=4)
    hl = head.hmr_layer
    if tf_decoder:
        # every Linear of the transformer head as a pointwise GEMM; the cross-attention in_proj is cut into its query rows
        # (applied to the tokens, every iteration) and its key | value rows (applied to `memory`, once per forward)
        lin = lambda m: pack_linear(cpu(m.weight), cpu(m.bias), dev)
        E = TF_DIM
        dl, el = hl.refine_decoder.layers[0], hl.self_attn.layers[0]
        xw, xb = cpu(dl.multihead_attn.in_proj_weight), cpu(dl.multihead_attn.in_proj_bias)
        P["tf"] = {
            "pre": lin(head.cam_init_precursor[0]), "feat_mlp": lin(hl.feat_mlp[0]),
            "vec_w": cpu(hl.vector_mlp[0].weight).float().reshape(E).contiguous().to(dev),
            "vec_b": cpu(hl.vector_mlp[0].bias).float().contiguous().to(dev),
            "d_qkv": pack_linear(cpu(dl.self_attn.in_proj_weight), cpu(dl.self_attn.in_proj_bias), dev),
            "d_proj": lin(dl.self_attn.out_proj),
            "x_q": pack_linear(xw[:E], xb[:E], dev), "x_kv": pack_linear(xw[E:], xb[E:], dev),
            "x_proj": lin(dl.multihead_attn.out_proj), "d_l1": lin(dl.linear1), "d_l2": lin(dl.linear2),
            "e_qkv": pack_linear(cpu(el.self_attn.in_proj_weight), cpu(el.self_attn.in_proj_bias), dev),
            "e_proj": lin(el.self_attn.out_proj), "e_l1": lin(el.linear1), "e_l2": lin(el.linear2)}
        # cam_t.wp.init = 1 + an O(0.1) read-out: its error is the final rounding plus what the four layers in front of it
        # pass on.  The reference's fp32 value is within 0.3-0.8 ulp of its fp64 run, so the layers are accumulated in fp64
        # (HANDS_ACC_F64: correctly rounded fp32 outputs; the precursor is 4 % of the head's work at half the matrix rate)
        for pc in (P["tf"]["pre"], P["ci0"], P["ci2"], P["ci4"]):
            pc.acc64 = True
    else:
        rf = hl.refine
        P["r0"] = pack_linear(cpu(rf[0].weight), cpu(rf[0].bias), dev, col_index=hmr_state_columns(F),
                              k_total=F + HMR_VEC)
        P["r3"] = pack_linear(cpu(rf[3].weight), cpu(rf[3].bias), dev)
    P["dec"] = pack_hmr_decoders(*[(hl.decoders[k].weight, hl.decoders[k].bias) for k in ("pose_6d", "shape", "cam_t/wp")], dev)
    return P


def depth_head(engine, buf, L, P, dev, stream, cat, B2, bz, fh, fw, Cr, lda, ldd):
    """`predict_depth` (model.py:177-185, 438-441) on the map feature_conv reads (``Cr`` channels in rows of ``lda`` floats):
    (x, y) grid channels appended (rows of ``ldd``), eight 3x3 / pad 1 convolutions, three align_corners upsamplings
    (7 -> 28 -> 112 -> 224).  Returns (depth.r, depth.l), each (bz, 224, 224)."""
    d = P["depth"]
    out = torch.empty(B2, 16 * fh * 2, 16 * fw * 2, device=dev)
    step = 256                       # images per pass: the 224 x 224 x 32 map of 256 crops is 1.6 GB (and < 2^31 floats)
    for lo in range(0, B2, step):
        n = min(step, B2 - lo)
        din = buf("depth_in", n * fh * fw * ldd)
        check(L.hands_concat_nhwc_f32(ptr(cat, lo * fh * fw * lda), lda, Cr, None, 0, ptr(P["depth_grid"]), 0, 2, ptr(din), ldd,
                                      n, n, fh * fw, stream), "depth_in")
        h, w = fh, fw
        x = din
        for i, pc in enumerate(d):
            y = buf(f"depth_c{i}", n * h * w * pc.Cout)
            engine.conv(L, pc, x, n, h, w, y, i < 7, stream)
            x = y
            if i in (1, 3, 5):                            # nn.Upsample(x4, x4, x2; bilinear, align_corners=True)
                k = 2 if i == 5 else 4
                u = buf(f"depth_u{i}", n * h * k * w * k * pc.Cout)
                check(L.hands_upsample_bilinear_ac_f32(ptr(x), ptr(u), n, h, w, h * k, w * k, pc.Cout, stream), "upsample_ac")
                x, h, w = u, h * k, w * k
        out[lo:lo + n] = x[: n * h * w * 4].view(n, h, w, 4)[..., 0]      # Cout = 1 stored with a pixel stride of 4 floats
    return out[:bz], out[bz:]


def cam_init(engine, buf, names, L, hp, stream, x, rows, caminit4, out_off, in_ps=None, x_off=0):
    """The ``cam_init`` MLP (hand_hmr.py:34-40, 512 -> 512 -> 3 stored 4 wide) on ``rows`` feature rows of ``x`` -> rows of
    ``caminit4`` from float ``out_off``; ``names``: the two hidden buffers."""
    linear_chain(engine, L, [(hp["ci0"], True, True), (hp["ci2"], True, True), (hp["ci4"], False, False)], x, rows, stream, buf, names,
                 out=caminit4, in_ps=in_ps, x_off=x_off, out_off=out_off)


def iter_head(engine, buf, L, hp, stream, side, bz, state, caminit4, feat_dim):
    """``HandHMR.forward`` with tf_decoder=False (hand_hmr.py:73-92, hmr_layer.py:67-86) for one hand: its ``state`` rows
    [side bz, (side + 1) bz) hold [feat F | vectors 112] with the feat segment filled in -> cam_init, hands_hmr_init_f32, then
    3 x [refine MLP -> decoders GEMM + residual on the vector columns]; its ``caminit4`` rows."""
    F, ld = feat_dim, feat_dim + HMR_VEC
    so, co = side * bz * ld, side * bz * 4
    cam_init(engine, buf, (f"h512a{side}", f"h512b{side}"), L, hp, stream, state, bz, caminit4, co, in_ps=ld, x_off=so)
    check(L.hands_hmr_init_f32(ptr(state, so), ptr(caminit4, co), bz, ld, F, stream), "hmr_init")
    for _ in range(3):
        x2 = linear_chain(engine, L, [(hp["r0"], True, True), (hp["r3"], True, True)], state, bz, stream, buf,
                          (f"x1024a{side}", f"x1024b{side}"), in_ps=ld, x_off=so)
        engine.conv(L, hp["dec"], x2, bz, 1, 1, state, False, stream, res=state, out_ps=ld, res_ps=ld, out_off=so + F, res_off=so + F,
                    splitk=True)


def tf_head(engine, buf, L, hp, stream, side, bz, HW, cat, state, caminit4, feat_dim, Cc, tf_pass=TF_PASS):
    """``HandHMR.forward(features, use_pool=False)`` with tf_decoder=True (hand_hmr.py:57-62, 73-92; hmr_layer.py:67-86) for one
    hand: rows [side bz, (side + 1) bz) of the concatenated map ``cat`` (B2, HW, Cc) -> the vector columns of its ``state``
    rows (ld 112) and its ``caminit4`` rows.

      cam_init_precursor per pixel (GEMM + ReLU) -> average pool -> cam_init MLP -> hands_hmr_init_f32
      memory = feat_mlp(pixels) and the cross-attention k | v = in_proj[E:](memory): ONCE, they do not change between iterations
      3 x [ hands_vector_tokens_f32 (109 tokens) -> decoder layer: self-attention, cross-attention, FFN -> encoder layer:
            self-attention, FFN -> hands_token_mean_f32 -> decoders GEMM + residual on the vectors ]

    Every residual is the GEMM's epilogue (x = x + f(x), no norm: no_norm=True); attention is hands_wide_attention_f32 reading
    the packed in_proj output in place.  Samples are walked in passes of ``tf_pass`` (256) so that the workspaces
    (``tf_{name}{side}``) stop growing at bz = 256; every kernel's rows are per sample, so a sample's result does not depend on
    the pass it falls in."""
    T, E, F = TF_TOKENS, TF_DIM, feat_dim
    tf = hp["tf"]
    assert tf["feat_mlp"].Cin == Cc and tf["pre"].Cin == Cc
    cap = min(bz, tf_pass)
    tbuf = lambda nm, numel: buf(f"tf_{nm}{side}", numel)
    mem, kv, pre, pooled = tbuf("mem", cap * HW * E), tbuf("kv", cap * HW * 2 * E), tbuf("pre", cap * HW * F), tbuf("pool", cap * F)
    x, att, q, hid = tbuf("x", cap * T * E), tbuf("att", cap * T * E), tbuf("q", cap * T * E), tbuf("hid", cap * T * E)
    qkv, xc = tbuf("qkv", cap * T * 3 * E), tbuf("xc", cap * E)
    scale = float(E) ** -0.5
    conv = engine.conv

    def attention(qb, kb, koff, ldk, Tk, n):
        """softmax(scale q k^T) v: q rows of ``qb`` (ld of its own width), k | v side by side in ``kb`` from column ``koff``"""
        ldq = 3 * E if qb is kb else E
        check(L.hands_wide_attention_f32(ptr(qb), T * ldq, ldq, ptr(kb, koff), Tk * ldk, ldk, ptr(kb, koff + E), Tk * ldk, ldk,
                                         ptr(att), T * E, E, n, T, Tk, E, scale, stream), "wide_attention")

    for lo in range(0, bz, tf_pass):
        n = min(tf_pass, bz - lo)
        r0 = side * bz + lo                       # first row of the pass in the (B2, ..) buffers
        so, co, M = r0 * HMR_VEC, r0 * 4, n * T
        # -- init_vector_dict (hand_hmr.py:46-71): cam_init_precursor per pixel BEFORE the average pool
        conv(L, tf["pre"], cat, n * HW, 1, 1, pre, True, stream, x_off=r0 * HW * Cc)
        check(L.hands_avgpool_nhwc_f32(ptr(pre), ptr(pooled), n, HW, F, F, stream), "avgpool")
        cam_init(engine, tbuf, ("h512a", "h512b"), L, hp, stream, pooled, n, caminit4, co)
        check(L.hands_hmr_init_f32(ptr(state, so), ptr(caminit4, co), n, HMR_VEC, 0, stream), "hmr_init")
        # -- memory and the cross-attention keys | values
        conv(L, tf["feat_mlp"], cat, n * HW, 1, 1, mem, True, stream, x_off=r0 * HW * Cc)
        conv(L, tf["x_kv"], mem, n * HW, 1, 1, kv, False, stream)
        for _ in range(3):
            # tokens in `init_vector_dict` order: pose_6d 96, shape 10 (state columns 0..105), cam_t/wp 3 (columns 108..110)
            check(L.hands_vector_tokens_f32(ptr(state, so), HMR_VEC, 106, 2, ptr(tf["vec_w"]), ptr(tf["vec_b"]), ptr(x), n, T, E,
                                            stream), "vector_tokens")
            # decoder layer (transformer.py:652-658): self-attention, cross-attention over the pixels, FFN
            conv(L, tf["d_qkv"], x, M, 1, 1, qkv, False, stream)
            attention(qkv, qkv, E, 3 * E, T, n)
            conv(L, tf["d_proj"], att, M, 1, 1, x, False, stream, res=x)
            conv(L, tf["x_q"], x, M, 1, 1, q, False, stream)
            attention(q, kv, 0, 2 * E, HW, n)
            conv(L, tf["x_proj"], att, M, 1, 1, x, False, stream, res=x)
            conv(L, tf["d_l1"], x, M, 1, 1, hid, True, stream)
            conv(L, tf["d_l2"], hid, M, 1, 1, x, False, stream, res=x)
            # encoder layer (transformer.py:533-539): self-attention, FFN
            conv(L, tf["e_qkv"], x, M, 1, 1, qkv, False, stream)
            attention(qkv, qkv, E, 3 * E, T, n)
            conv(L, tf["e_proj"], att, M, 1, 1, x, False, stream, res=x)
            conv(L, tf["e_l1"], x, M, 1, 1, hid, True, stream)
            conv(L, tf["e_l2"], hid, M, 1, 1, x, False, stream, res=x)
            # token mean, then the three decoders' residual update of the vectors (hmr_layer.py:78, 82-83)
            check(L.hands_token_mean_f32(ptr(x), ptr(xc), n, T, E, stream), "token_mean")
            conv(L, hp["dec"], xc, n, 1, 1, state, False, stream, res=state, out_ps=HMR_VEC, res_ps=HMR_VEC, out_off=so,
                 res_off=so, splitk=True)
