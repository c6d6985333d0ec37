"""Plain float64 restatements of the non-convolution kernels of csrc/handocc.hip, csrc/transformer.hip, csrc/vit_b.hip and of
the layout / pool kernels of csrc/elementwise.hip, for tests/test_gpu_kernel_edges.py.

One function per C entry point of include/hands_hip.h, named after it without ``hands_`` and ``_f32``.  Each takes the entry
point's arguments in its order -- CPU tensors where the C function takes pointers, with the same layouts (NHWC maps, token rows,
row strides), ``None`` for an optional pointer, no output pointers and no stream -- evaluates in float64 whatever the inputs'
dtype (or, inside ``precision(torch.float32)``, in float32), and returns the output tensor(s) in the layout the kernel writes.  Where a row stride leaves padding, the documented
fill is part of the result (the 4th channel of NHWC4, the heat-map columns J..ld_out-1, the KPE pad: all zero); undocumented gaps
(``out_stride > C`` of the pools, ``ld6 > 96``) are not part of it.  A ``scale`` / ``eps`` argument is taken as the float32 the C
function receives.  Where oracle/ already states an operation (the gated attention, pos_enc, the 6-D rotation) it is called,
not re-derived.  tests/test_kernel_refs.py pins every function here to the ATen operator or oracle function it restates;
nothing here is imported by the package.
"""
import torch

from oracle import hamer_oracle as H
from oracle import handoccnet_oracle as HO
from oracle import hands_oracle as O


_DT = torch.float64


class precision:
    """``with precision(torch.float32):`` evaluates the functions below with ATen in that dtype instead of float64 -- the
    yardstick tests/test_gpu_kernel_edges.py measures a float32 kernel against on inputs nobody has measured before."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        global _DT
        self.saved, _DT = _DT, self.dtype

    def __exit__(self, *exc):
        global _DT
        _DT = self.saved


def _d(t):
    return None if t is None else t.detach().cpu().to(_DT)


def _zeros(*shape):
    return torch.zeros(*shape, dtype=_DT)


def _f32(x):
    """The value a C `float` argument holds."""
    return float(torch.tensor(x, dtype=torch.float32).double())


def _lerp_axis(n_in, n_total, dst):
    """Source taps of bilinear interpolation, align_corners=False: for destination indices `dst` (int64) of a resize from n_in to
    n_total samples, src = max(0, (dst + 0.5) * n_in / n_total - 0.5); returns (i0, i1, w1) with i1 = min(i0 + 1, n_in - 1)."""
    s = ((dst.to(_DT) + 0.5) * (float(n_in) / float(n_total)) - 0.5).clamp_min(0.0)
    i0 = s.floor().long().clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, s - i0.to(_DT)


def _bilinear_nhwc(x, H, W, col0=0, Wc=None):
    """x (B,h,w,C) float64 -> (B,H,Wc,C): columns [col0, col0+Wc) of the bilinear resize to (H,W)."""
    _, h, w, _ = x.shape
    Wc = W if Wc is None else Wc
    y0, y1, ly = _lerp_axis(h, H, torch.arange(H))
    x0, x1, lx = _lerp_axis(w, W, torch.arange(col0, col0 + Wc))
    ly, lx = ly.view(1, H, 1, 1), lx.view(1, 1, Wc, 1)
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


# ---- csrc/handocc.hip -------------------------------------------------------------------------------------------------------
def upsample_bilinear_add(x, y, B, h, w, H, W, C):
    return _bilinear_nhwc(_d(x).view(B, h, w, C), H, W) + _d(y).view(B, H, W, C)


def pool2x2_nhwc(x, B, H, W, C, mode):
    win = _d(x).view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    return win.mean(-1) if mode == 0 else win.max(-1)[0]


def channel_pool(x, npix, C):
    x = _d(x).view(npix, C)
    return torch.stack([x.max(1)[0], x.mean(1), _zeros(npix), _zeros(npix)], 1)


def gate_apply(x, logit, logit_stride, npix, C):
    """-> (primary, secondary); logit is the flat buffer, one logit every logit_stride floats."""
    x = _d(x).view(npix, C)
    s = torch.sigmoid(_d(logit).reshape(-1)[: (npix - 1) * logit_stride + 1: logit_stride]).view(npix, 1)
    return x * s, x * (1 - s)


def add_embed2(query, key, q_emb, k_emb, kpe, B, N, C):
    """-> (out_q, out_k)"""
    kp = _d(kpe).view(B, 1, C)
    return (_d(query).view(B, N, C) + _d(q_emb).view(1, N, C)) + kp, (_d(key).view(B, N, C) + _d(k_emb).view(1, N, C)) + kp


def add_rowvec(x, vec, B, N, C):
    return _d(x).view(B, N, C) + _d(vec).view(B, 1, C)


def token_sum(x, B, N, C):
    return _d(x).view(B, N, C).sum(1)


def bn_leaky(x, scale, shift, npix, C):
    y = _d(x).view(npix, C) * _d(scale) + _d(shift)
    return torch.where(y > 0, y, 0.01 * y)


def upsample_nearest2x_add(low, up1, B, h, w, C):
    low = _d(low).view(B, h, w, C)
    return _d(up1).view(B, 2 * h, 2 * w, C) + low[:, torch.arange(2 * h) // 2][:, :, torch.arange(2 * w) // 2]


def spatial_softmax(latents, ld_in, betas, ld_out, B, N, J):
    """-> (B, N, ld_out): softmax over the N positions of latents[b,:,j] * betas[j] for j < J, zeros in the columns J..ld_out-1."""
    z = _d(latents).view(B, N, ld_in)[:, :, :J] * _d(betas)[:J]
    out = _zeros(B, N, ld_out)
    out[:, :, :J] = torch.softmax(z, dim=1)
    return out


def flash_attention(q, k, v, q2, k2sum, resid, B, N, heads, head_dim, scale):
    """oracle.handoccnet_oracle.attention, which fixes scale = head_dim ** -0.5 and takes the gate's keys k2 (B,N,C): another
    `scale` goes in through q (and q2), and a k2 whose only non-zero token is k2sum has the key sum the entry point is given."""
    C = heads * head_dim
    f = _f32(scale) / head_dim ** -0.5
    q, k, v = (_d(t).view(B, N, C) for t in (q, k, v))
    if q2 is not None:
        k2 = _zeros(B, N, C)
        k2[:, 0] = _d(k2sum).view(B, C)
        out = HO.attention(q * f, k, v, _d(q2).view(B, N, C) * f, k2, heads, True)
    else:
        out = HO.attention(q * f, k, v, None, None, heads, False)
    return out if resid is None else _d(resid).view(B, N, C) + out


# ---- csrc/transformer.hip ---------------------------------------------------------------------------------------------------
def resize_crop_nchw3_to_nhwc4(x, B, Hin, Win, S, col0, Wc):
    """-> (B, S, Wc, 4), 4th channel zero."""
    img = _bilinear_nhwc(_d(x).view(B, 3, Hin, Win).permute(0, 2, 3, 1), S, S, col0, Wc)
    return torch.cat([img, _zeros(B, S, Wc, 1)], -1)


def layernorm(x, gamma, beta, addvec, rows_per_vec, M, C, eps):
    x = _d(x).view(M, C)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + _f32(eps)) * _d(gamma) + _d(beta)
    if addvec is not None:
        y = y + _d(addvec).view(-1, C)[torch.arange(M) // rows_per_vec]
    return y


def add_pos(x, pos, vec, B, T, C):
    pos = _d(pos).view(-1, C)
    y = (_d(x).view(B, T, C) + pos[None, 1:1 + T]) + pos[None, :1]
    return y if vec is None else y + _d(vec).view(B, 1, C)


def kpe_encode(center_angle, corner_angle, B, ld, n_freq):
    """-> (B, ld): [pos_enc(center) 4 n_freq | pos_enc(corner) 16 n_freq | zeros].  oracle.hands_oracle.pos_enc evaluates in the
    dtype it is given (float64 here) and returns float32: the rounding of its result, 6e-8, is part of this reference."""
    out = _zeros(B, ld)
    enc = torch.cat([O.pos_enc(_d(center_angle).view(B, 2), n_freq), O.pos_enc(_d(corner_angle).view(B, 8), n_freq)], 1)
    out[:, :20 * n_freq] = enc.to(_DT)
    return out


def attention(qkv, B, T, heads, head_dim, scale):
    """softmax((scale q) k^T) v per (batch, head); qkv rows [q | k | v] -> (B, T, heads * head_dim)."""
    q, k, v = _d(qkv).view(B, T, 3, heads, head_dim).permute(2, 0, 3, 1, 4)
    p = torch.softmax((q * _f32(scale)) @ k.transpose(-2, -1), dim=-1)
    return (p @ v).transpose(1, 2).reshape(B, T, heads * head_dim)


def cross_attention_1q(q, kv, B, T, heads, head_dim, scale):
    inner = heads * head_dim
    k, v = _d(kv).view(B, T, 2 * inner).split(inner, dim=-1)
    sp = lambda z: z.reshape(B, -1, heads, head_dim).transpose(1, 2)
    p = torch.softmax(sp(_d(q).view(B, 1, inner)) @ sp(k).transpose(-1, -2) * _f32(scale), dim=-1)
    return (p @ sp(v)).transpose(1, 2).reshape(B, inner)


def rot6d_to_matrix_cols(pose6d, ld6, B):
    """-> (B, 16, 3, 3); oracle.hamer_oracle.rot6d_to_rotmat_columns on the first 96 floats of each row (F.normalize clamps
    both norms at 1e-12, as the kernel does)."""
    return H.rot6d_to_rotmat_columns(_d(pose6d).view(B, ld6)[:, :96].reshape(-1, 6)).view(B, 16, 3, 3)


# ---- csrc/vit_b.hip ---------------------------------------------------------------------------------------------------------
def vit_tokens(patch, class_token, pos, B, T, C):
    x = torch.cat([_d(class_token).view(1, 1, C).expand(B, 1, C), _d(patch).view(B, T - 1, C)], 1)
    return x + _d(pos).view(1, T, C)


def vit_tail(x, gamma, beta, B, grid, C, eps):
    """-> (B, grid/2, grid/2, C)"""
    T = 1 + grid * grid
    y = layernorm(_d(x).view(B, T, C)[:, 1:].reshape(-1, C), gamma, beta, None, 1, B * grid * grid, C, eps)
    return pool2x2_nhwc(y, B, grid, grid, C, 0)


# ---- csrc/elementwise.hip ---------------------------------------------------------------------------------------------------
def nchw3_to_nhwc4(x, B, H, W):
    return torch.cat([_d(x).view(B, 3, H, W).permute(0, 2, 3, 1), _zeros(B, H, W, 1)], -1)


def maxpool3x3s2_nhwc(x, B, H, W, C):
    """MaxPool2d(3, 2, 1): -> (B, Ho, Wo, C), Ho = (H - 1) // 2 + 1; taps outside the map do not take part."""
    x = _d(x).view(B, H, W, C)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = torch.full((B, 2 * Ho + 1, 2 * Wo + 1, C), float("-inf"), dtype=_DT)
    pad[:, 1:H + 1, 1:W + 1] = x
    out = torch.full((B, Ho, Wo, C), float("-inf"), dtype=_DT)
    for dh in range(3):
        for dw in range(3):
            out = torch.maximum(out, pad[:, dh:dh + 2 * Ho:2, dw:dw + 2 * Wo:2])
    return out


def sumpool_nhwc(feat, B, HW, C, out_stride):
    """-> (B, C): the columns the kernel writes of its (B, out_stride) output."""
    return _d(feat).view(B, HW, C).sum(1)


def avgpool_nhwc(feat, B, HW, C, out_stride):
    return _d(feat).view(B, HW, C).sum(1) / HW
