"""Plain float64 restatements of the non-convolution kernels of csrc/handocc.hip, csrc/transformer.hip, csrc/vit_b.hip,
csrc/metrics.hip and csrc/elementwise.hip, for tests/test_gpu_kernel_edges.py and tests/test_gpu_io_edges.py (csrc/frontend.hip
has its restatement in oracle/frontend_oracle.py), ``mano_head_ref`` (the MANO head of csrc/mano_lbs.hip with a general K, free
tip vertices and min_s, for tests/test_gpu_mano_edges.py), and -- last in the file -- ``conv_ref``, the one restatement of the
convolution entry points of csrc/conv_igemm.hip on flat, strided buffers for tests/test_gpu_conv_edges.py (and of the same layer
on the Winograd routes), with ``stem_pool_ref``, the fused stems of csrc/stem_pool.hip, for tests/test_gpu_wino_stem_edges.py.

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
import numpy as np
import torch
import torch.nn.functional as F

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


# ---- csrc/elementwise.hip: the glue kernels ---------------------------------------------------------------------------------
def _pos_enc(angle, n_freq):
    """oracle.hands_oracle.pos_enc without its final rounding to float32: (bz, c) -> (bz, n_freq * c * 2), element
    (k c + ci) 2 + {0: sin, 1: cos} of 2^k angle[ci].  2^k times a float32 angle is exact in float32 and in float64."""
    bz, c = angle.shape
    a = (2.0 ** torch.arange(n_freq, dtype=_DT)).view(1, n_freq, 1) * angle.view(bz, 1, c)
    return torch.stack([torch.sin(a), torch.cos(a)], -1).reshape(bz, -1)


def image_posenc_nhwc(img_nchw, center_angle, corner_angle, B, H, W, n_freq, mode, Cpad):
    """-> (B, H, W, Cpad): [r g b | center encoding if mode & 1 | corner encoding if mode & 2 | zeros]."""
    parts = [_d(img_nchw).view(B, 3, H, W).permute(0, 2, 3, 1)]
    if mode & 1:
        parts.append(_pos_enc(_d(center_angle).view(B, 2), n_freq).view(B, 1, 1, -1).expand(B, H, W, -1))
    if mode & 2:
        parts.append(_pos_enc(_d(corner_angle).view(B, 8), n_freq).view(B, 1, 1, -1).expand(B, H, W, -1))
    out = _zeros(B, H, W, Cpad)
    cat = torch.cat(parts, -1)
    out[..., :cat.shape[-1]] = cat
    return out


def kpe_concat(crop, glb, center_angle, corner_angle, B2, Bg, HW, C, n_freq):
    """-> (B2, HW, C + 20 n_freq): [crop (+ glb of sample b2 % Bg) | center encoding | corner encoding]."""
    feat = _d(crop).view(B2, HW, C)
    if glb is not None:
        feat = feat + _d(glb).view(Bg, HW, C)[torch.arange(B2) % Bg]
    enc = torch.cat([_pos_enc(_d(center_angle).view(B2, 2), n_freq), _pos_enc(_d(corner_angle).view(B2, 8), n_freq)], 1)
    return torch.cat([feat, enc.view(B2, 1, -1).expand(B2, HW, -1)], -1)


def dense_posenc(angle, mask, img_nchw, B, Ca, Hs, Ws, n_freq, R, Ho, Wo, ld, c_off):
    """-> with img (B, Ho, Wo, ld): [r g b | encoding | zeros]; without (B, Ho, Wo, Cenc): the columns c_off.. the kernel writes.
    The masked encoding (n_freq 0: the masked maps themselves) resized to (R, R) and then to (Ho, Wo), both times as
    F.interpolate(mode='bilinear', align_corners=True) does."""
    ang, msk = _d(angle).view(B, Ca, Hs, Ws), _d(mask).view(B, 1, Hs, Ws)
    if n_freq:
        a = (2.0 ** torch.arange(n_freq, dtype=_DT)).view(1, n_freq, 1, 1, 1) * ang.view(B, 1, Ca, Hs, Ws)
        enc = torch.stack([torch.sin(a), torch.cos(a)], 3).reshape(B, 2 * n_freq * Ca, Hs, Ws)      # channel (k Ca + ci) 2 + sc
    else:
        enc = ang
    enc = F.interpolate(enc * msk, size=(R, R), mode="bilinear", align_corners=True)
    enc = F.interpolate(enc, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    if img_nchw is None:
        return enc.contiguous()
    out = _zeros(B, Ho, Wo, ld)
    out[..., :3] = _d(img_nchw).view(B, 3, Ho, Wo).permute(0, 2, 3, 1)
    out[..., 3:3 + enc.shape[-1]] = enc
    return out


def concat_nhwc(a, lda, Ca, add, ld_add, extra, extra_batch_stride, Cb, ld, B, Bg, HW):
    """-> (B, HW, ld): [a[:, :, :Ca] (+ add of sample b % Bg) | extra (B, HW, Cb), or one (HW, Cb) map for all when the batch
    stride is 0 | zeros]."""
    out = _zeros(B, HW, ld)
    out[..., :Ca] = _d(a).view(B, HW, lda)[..., :Ca]
    if add is not None:
        out[..., :Ca] += _d(add).view(Bg, HW, ld_add)[torch.arange(B) % Bg][..., :Ca]
    if Cb:
        ex = _d(extra).reshape(-1)
        idx = (torch.arange(B) * extra_batch_stride).view(B, 1, 1) + torch.arange(HW * Cb).view(1, HW, Cb)
        out[..., Ca:Ca + Cb] = ex[idx]
    return out


def upsample_bilinear_ac(x, B, h, w, H, W, C):
    y = F.interpolate(_d(x).view(B, h, w, C).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)
    return y.permute(0, 2, 3, 1).contiguous()


def rot_leftmul(rotmat, rot, B):
    """-> (B, 16, 3, 3): joint 0 left-multiplied by rot (B, 3, 3), the other fifteen as they were."""
    out = _d(rotmat).view(B, 16, 3, 3).clone()
    out[:, 0] = _d(rot).view(B, 3, 3) @ out[:, 0]
    return out


def perspective_correction(rot_swapped, rotmat, center_angle, is_flipped, Bg):
    """-> (rot_swapped, rotmat) afterwards, (2 Bg, 16, 3, 3) each: joint 0 of rot_swapped left-multiplied by
    oracle.hands_oracle.euler_angles_to_matrix_xyz(-center_x, -center_y, 0); rotmat receives the same matrix only when no sample
    is flipped."""
    c = _d(center_angle).view(2 * Bg, 2)
    e = O.euler_angles_to_matrix_xyz(torch.cat([-c, torch.zeros(2 * Bg, 1, dtype=_DT)], -1))
    sw, un = _d(rot_swapped).view(2 * Bg, 16, 3, 3).clone(), _d(rotmat).view(2 * Bg, 16, 3, 3).clone()
    sw[:, 0] = e @ sw[:, 0]
    if not bool((is_flipped != 0).any()):
        un[:, 0] = sw[:, 0]
    return sw, un


def hmr_init(state, cam_init, B, ld, F_):
    """-> state (B, ld) afterwards: columns F.. = [identity 6-D x 16 | zeros 10 | 0 0 | cam_init[:, :3] | 0]; the rest untouched."""
    out = _d(state).view(B, ld).clone()
    vec = _zeros(B, 112)
    vec[:, 0:96:6] = 1.0
    vec[:, 4:96:6] = 1.0
    vec[:, 108:111] = _d(cam_init).view(B, 4)[:, :3]
    out[:, F_:F_ + 112] = vec
    return out


def rot6d_to_matrix(pose6d, ld6, B):
    """-> (B, 16, 3, 3); oracle.hands_oracle.rotation_6d_to_matrix (rows) on the first 96 floats of each row."""
    return O.rotation_6d_to_matrix(_d(pose6d).view(B, ld6)[:, :96].reshape(-1, 6)).view(B, 16, 3, 3)


def grasp_input(shape, ld_shape, rotmat, feat_vec, B2, Bg, F_, ld_out):
    """-> (B2, ld_out): [feat_vec of sample b % Bg (F) | rotmat 144 | shape 10 | zeros]."""
    out = _zeros(B2, ld_out)
    if F_:
        out[:, :F_] = _d(feat_vec).view(-1)[:Bg * F_].view(Bg, F_)[torch.arange(B2) % Bg]
    out[:, F_:F_ + 144] = _d(rotmat).view(B2, 144)
    out[:, F_ + 144:F_ + 154] = _d(shape).view(B2, ld_shape)[:, :10]
    return out


# ---- csrc/metrics.hip -------------------------------------------------------------------------------------------------------
def _procrustes_mean_error(gt, pr):
    """eval_modules.py:136-219 on root-aligned (B, 21, 3) joints: mean_j |gt_j - (s R pr_j + t)| with the similarity transform of
    the reference, LAPACK SVD and its Z[-1, -1] *= sign(det(U V^T))."""
    mu1, mu2 = pr.mean(1, keepdim=True), gt.mean(1, keepdim=True)
    X1, X2 = pr - mu1, gt - mu2
    var1 = (X1 ** 2).sum((1, 2))
    K = X1.transpose(1, 2) @ X2
    U, _, Vh = torch.linalg.svd(K)
    V = Vh.transpose(1, 2)
    Z = torch.eye(3, dtype=K.dtype).repeat(K.shape[0], 1, 1)
    Z[:, 2, 2] = torch.sign(torch.linalg.det(U @ V.transpose(1, 2)))
    Rm = V @ Z @ U.transpose(1, 2)
    scale = (Rm @ K).diagonal(dim1=1, dim2=2).sum(1) / var1                  # 0 / 0 = NaN for a constant prediction
    t = mu2.transpose(1, 2) - scale.view(-1, 1, 1) * (Rm @ mu1.transpose(1, 2))
    hat = scale.view(-1, 1, 1) * (Rm @ pr.transpose(1, 2)) + t
    return (gt - hat.transpose(1, 2)).norm(dim=2).mean(1)


def _nanmean2(a, b):
    st = torch.stack([a, b], 1)
    nan = torch.isnan(st)
    return torch.where(nan, torch.zeros_like(st), st).sum(1) / (~nan).sum(1).to(st.dtype)


def eval_metrics(pred_j3d_r, pred_j3d_l, gt_j3d_r, gt_j3d_l, pred_j2d_r, pred_j2d_l, gt_j2d_r, gt_j2d_l, is_valid, right_valid,
                 left_valid, joints_valid_r, joints_valid_l, B):
    """The members of hands_eval_in in their order -> those of hands_eval_out in theirs: (mpjpe_ra_h, mpjpe_pa_ra_r, mpjpe_pa_ra_l,
    mpjpe_pa_ra_h, mrrpe_rl) (B) each in mm, (pix_err_r, pix_err_l) (B, 21) in px.  The root alignment is done in float32, as by
    the reference and the kernel (the inputs are float32 and that subtraction is part of the definition); everything after it in
    float64."""
    f32 = lambda t, *s: t.detach().cpu().to(torch.float32).view(B, *s)
    nan = float("nan")
    iv = f32(is_valid)
    rv, lv = _d(f32(right_valid) * iv), _d(f32(left_valid) * iv)
    pr, pl, gr, gl = (f32(t, 21, 3) for t in (pred_j3d_r, pred_j3d_l, gt_j3d_r, gt_j3d_l))
    ra = lambda x: _d(x - x[:, :1])
    ra_err = lambda g, p, v: torch.where(v != 0, (ra(g) - ra(p)).norm(dim=2).mean(1), torch.full_like(v, nan))
    mpjpe_ra_h = _nanmean2(ra_err(gr, pr, rv), ra_err(gl, pl, lv)) * 1000.0
    pa_r, pa_l = _procrustes_mean_error(ra(gr), ra(pr)) * rv, _procrustes_mean_error(ra(gl), ra(pl)) * lv
    rel = ((_d(pl[:, 0]) - _d(pr[:, 0])) - (_d(gl[:, 0]) - _d(gr[:, 0]))).norm(dim=1)
    mrrpe = torch.where(lv * rv != 0, rel * 1000.0, torch.full_like(rel, nan))
    pix = []
    for g2, p2, jv, v in ((gt_j2d_r, pred_j2d_r, joints_valid_r, rv), (gt_j2d_l, pred_j2d_l, joints_valid_l, lv)):
        d = (_d(f32(g2, 21, 2)) - _d(f32(p2, 21, 2))).norm(dim=2)
        pix.append(torch.where(_d(f32(jv, 21)) * v.view(B, 1) != 0, d, torch.full_like(d, nan)))
    return mpjpe_ra_h, pa_r * 1000.0, pa_l * 1000.0, _nanmean2(pa_r, pa_l) * 1000.0, mrrpe, pix[0], pix[1]


def gt_targets(joints, verts, j3d_full, K, img_res, B, NV):
    """-> (v3d_cam (B, NV, 3), cam_t (B, 3), cam_t_wp (B, 3)): process_data_light as oracle.wrapper_oracle states it."""
    jc, jf, Km = _d(joints).view(B, 21, 3), _d(j3d_full).view(B, 21, 3), _d(K).view(B, 3, 3)
    cam_t = jf[:, 0] - jc[:, 0]
    f = (Km[:, 0, 0] + Km[:, 1, 1]) / 2.0
    wp = torch.stack([2 * f / (_f32(img_res) * cam_t[:, 2] + 1e-9), cam_t[:, 0], cam_t[:, 1]], -1)
    return _d(verts).view(B, NV, 3) + (jf - jc).mean(1)[:, None, :], cam_t, wp


def unnormalize_kp2d(x, n, img_res):
    return 0.5 * _f32(img_res) * (_d(x).reshape(-1)[:n] + 1)


# ---- csrc/mano_lbs.hip ------------------------------------------------------------------------------------------------------
def mano_head_ref(rot_or_aa, betas, cam, K, asset, img_res, min_s, tip_ids=O.TIP_IDS, aa_input=False):
    """hands_mano_heads_f32 / the chain hands_mano_pose[_aa]_f32 -> blend GEMM -> hands_mano_skin_f32 for one side:
    oracle.hands_oracle.mano_head and mano_lbs restated statement for statement (the same ATen calls in the same order, so the
    float32 evaluation has the oracle's bits) with the three things the oracle fixes made free: a general (B, 3, 3) K -- the
    projection is (K X)_xy / (K X)_z --, any five ``tip_ids``, any ``min_s``.  ``rot_or_aa``: (B, 16, 3, 3) rotation matrices, or
    (B, 48) axis-angle with ``aa_input``.  ``img_res`` and ``min_s`` are used as given: pass the float32 values the C function
    receives.  -> dict of the six outputs under the head's names plus the intermediates of the three-launch chain:
    ``blend_row`` (B, 145) = [beta | R - I of joints 1..15], ``A`` (B, 16, 12) skinning transforms (3 x 4, row-major),
    ``joints16`` (B, 16, 3) posed joints, and ``hz`` (B, 21), the third row of K X the projection divides by."""
    dt = _DT
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dt)
    betas, cam, K = _d(betas), _d(cam), _d(K)
    B = betas.shape[0]
    if aa_input:
        aa = _d(rot_or_aa).reshape(B, 48)
    else:
        aa = O.matrix_to_axis_angle(_d(rot_or_aa).reshape(-1, 3, 3)).reshape(-1, 48)
    global_orient, hand_pose = aa[:, :3], aa[:, 3:]
    # smplx.MANO.forward as oracle.hands_oracle.mano_lbs states it
    v_template, shapedirs, posedirs = t(asset.v_template), t(asset.shapedirs), t(asset.posedirs)
    J_regressor, lbs_weights = t(asset.J_regressor), t(asset.lbs_weights)
    pose_mean = torch.cat([torch.zeros(3, dtype=dt), t(asset.hands_mean)])
    full_pose = torch.cat([global_orient, hand_pose], dim=1) + pose_mean
    v_shaped = v_template + torch.einsum("bl,mkl->bmk", betas, shapedirs)
    J = torch.einsum("bik,ji->bjk", v_shaped, J_regressor)
    rot_mats = O.batch_rodrigues(full_pose.reshape(-1, 3)).view(B, 16, 3, 3)
    pose_feature = (rot_mats[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(pose_feature, posedirs).view(B, -1, 3)
    rel_J = J.clone()
    parents = list(O.PARENTS)
    rel_J[:, 1:] = J[:, 1:] - J[:, parents[1:]]
    T = torch.zeros(B, 16, 4, 4, dtype=dt)
    T[:, :, :3, :3] = rot_mats
    T[:, :, :3, 3] = rel_J
    T[:, :, 3, 3] = 1
    chain = [T[:, 0]]
    for i in range(1, 16):
        chain.append(torch.matmul(chain[parents[i]], T[:, i]))
    G = torch.stack(chain, dim=1)
    posed_joints = G[:, :, :3, 3]
    J_h = torch.cat([J, torch.zeros(B, 16, 1, dtype=dt)], dim=2)[..., None]
    A = G.clone()
    A[:, :, :, 3] = G[:, :, :, 3] - torch.matmul(G, J_h)[..., 0]
    Tv = torch.matmul(lbs_weights[None].expand(B, -1, -1), A.view(B, 16, 16)).view(B, -1, 4, 4)
    v_h = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=dt)], dim=2)
    verts = torch.matmul(Tv, v_h[..., None])[:, :, :3, 0]
    joints = torch.cat([posed_joints, verts[:, list(tip_ids)]], dim=1)
    # MANOHead.forward as oracle.hands_oracle.mano_head states it
    avg_f = (K[:, 0, 0] + K[:, 1, 1]) / 2.0
    cam_t = O.weak_perspective_to_perspective(cam, avg_f, img_res, min_s)
    j3d_cam = joints + cam_t[:, None, :]
    v3d_cam = verts + cam_t[:, None, :]
    homo = torch.bmm(K, j3d_cam.permute(0, 2, 1)).permute(0, 2, 1)
    j2d = O.normalize_kp2d(homo[:, :, :2] / homo[:, :, 2:3], img_res)
    return {"vertices": verts, "joints3d": joints, "v3d.cam": v3d_cam, "j3d.cam": j3d_cam, "j2d.norm": j2d, "cam_t": cam_t,
            "blend_row": torch.cat([betas, pose_feature], dim=1), "A": A[:, :, :3, :].reshape(B, 16, 12).clone(),
            "joints16": posed_joints.clone(), "hz": homo[:, :, 2].clone()}


# ---- csrc/conv_igemm.hip ----------------------------------------------------------------------------------------------------
def _pixels(buf, n, ps, C):
    """(n, C): channels [0, C) of n pixels that sit `ps` floats apart in the flat buffer `buf` (ps == 0: one row for all)."""
    idx = torch.arange(n).view(n, 1) * ps + torch.arange(C).view(1, C)
    return buf.detach().cpu().reshape(-1)[idx]


def conv_act(y, act):
    """The epilogue activation HANDS_ACT_* (low byte of desc.act) in y's dtype."""
    act &= 0xff
    if act == 1:
        return y.clamp_min(0)
    if act == 2:
        return y * 0.5 * (1 + torch.erf(y * 0.70710678118654752440))
    if act == 3:
        return torch.where(y > 0, y, 0.01 * y)
    assert act == 0, act
    return y


def conv_ref(d, x, w, bias, res, out, pre=None, dual=None, round_sum=False):
    """The convolution entry points of include/hands_hip.h (hands_conv2d_nhwc_f32 and its split-K / fused / stream-K / grouped
    forms, hands_conv2d_nhwc_pre_f32 with ``pre`` = (scale, shift), hands_conv1x1_dual_nhwc_f32 with ``dual`` = (in2, Cin2, H2,
    W2, stride2, in2_pix_stride)) on FLAT buffers as the C function sees them: ``x``, ``res`` (or None), ``out`` start at the
    pointers the call gets, ``out`` holding what the buffer held before the call (pass it as ``res`` too for an in-place
    residual); ``d`` carries the fields of hands_conv_desc; ``w`` is the packed weight [Cout_pad][Kpad], k = (kh, kw, cin), for
    the dual form [W0 (Cin) | W1 (Cin2)]; columns beyond KH*KW*Cin of a plain layer are zero by contract and not read here.

    -> (expected, A), both of out's shape: the whole buffer after the call -- pixel m = (b, ho, wo) of the (Ho, Wo) top-left
    corner of the geometry's map at [m * out_pix_stride, + Cout), everything else as it was -- and the magnitude
    A = conv(|x|, |w|) + |bias| + |res| of every written element (0 elsewhere).  ``pre``: the operand is
    leaky_relu(x * scale + shift, 0.01) evaluated in float32, as the kernel stages it (bit-identical to hands_bn_leaky_f32 by the
    header's contract), whatever the precision.  ``round_sum`` (HANDS_ACC_F64): sum + bias is rounded to float32 once, residual
    and activation follow in float32."""
    B, H, W, Cin, Ho, Wo, Cout = d.B, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout
    KH, KW, K, M = d.KH, d.KW, d.KH * d.KW * d.Cin, d.B * d.Ho * d.Wo
    xs = _pixels(x, B * H * W, d.in_pix_stride, Cin)
    if pre is not None:
        xs = xs.float() * pre[0].detach().cpu().float().view(1, Cin) + pre[1].detach().cpu().float().view(1, Cin)
        xs = torch.where(xs > 0, xs, 0.01 * xs)
    xs = _d(xs).view(B, H, W, Cin).permute(0, 3, 1, 2)
    wt = _d(w).reshape(-1, d.Kpad)[:Cout]
    w0 = wt[:, :K].reshape(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    y = F.conv2d(xs, w0, None, d.stride, d.pad)[:, :, :Ho, :Wo]
    a = F.conv2d(xs.abs(), w0.abs(), None, d.stride, d.pad)[:, :, :Ho, :Wo]
    assert y.shape[2:] == (Ho, Wo), "the output map is larger than the geometry's"
    y, a = y.permute(0, 2, 3, 1).reshape(M, Cout), a.permute(0, 2, 3, 1).reshape(M, Cout)
    if dual is not None:
        x2, Cin2, H2, W2, s2, ps2 = dual
        x2 = _d(_pixels(x2, B * H2 * W2, ps2, Cin2)).view(B, H2, W2, Cin2)[:, :(Ho - 1) * s2 + 1:s2, :(Wo - 1) * s2 + 1:s2]
        x2, w1 = x2.reshape(M, Cin2), wt[:, K:K + Cin2]
        y, a = y + x2 @ w1.t(), a + x2.abs() @ w1.abs().t()
    bv = _d(bias).reshape(-1)[:Cout]
    y, a = y + bv, a + bv.abs()
    if round_sum:
        y = y.float()
    if res is not None:
        r = _pixels(res, M, d.res_pix_stride, Cout).to(y.dtype)
        y, a = y + r, a + r.abs().to(a.dtype)
    y = conv_act(y, d.act).to(_DT)
    idx = (torch.arange(M).view(M, 1) * d.out_pix_stride + torch.arange(Cout).view(1, Cout)).reshape(-1)
    exp, mag = _d(out).reshape(-1).clone(), _zeros(out.numel())
    exp[idx], mag[idx] = y.reshape(-1), a.reshape(-1)
    return exp.view(out.shape), mag.view(out.shape)


# ---- csrc/stem_pool.hip -----------------------------------------------------------------------------------------------------
class _StemDesc:
    """The hands_conv_desc of the stem convolution (7x7 / stride 2 / pad 3, 64 channels, no activation) on contiguous pixels."""

    def __init__(self, B, H, W, Cin, Kpad):
        self.B, self.H, self.W, self.Cin, self.Cout, self.KH, self.KW, self.stride, self.pad = B, H, W, Cin, 64, 7, 7, 2, 3
        self.Ho, self.Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        self.in_pix_stride, self.out_pix_stride, self.res_pix_stride, self.Kpad, self.act = Cin, 64, 0, Kpad, 0


def stem_pool_ref(x, w, bias, B, H, W, act, planar=False):
    """hands_stem_conv_maxpool_nhwc_f32 (``x`` = the RGB0 image (B, H, W, 4), ``w`` = [>= 64][208], k = (kh, kw, rgb0)) and, with
    ``planar``, hands_stem_conv_maxpool_nchw_f32 (``x`` = (B, 3, H, W), ``w`` = [>= 64][160], k = plane * 52 + kh * 7 + kw): conv_ref
    of the 7x7 / 2 / 3 layer on 4 resp. 3 input channels, conv_act, maxpool3x3s2_nhwc, in that order (the kernels add the bias and
    activate after the maximum: the same value, both being monotone).

    -> (expected, A_pool), both (B, Hp, Wp, 64): A_pool is the window maximum of conv_ref's magnitude A = conv(|x|, |w|) + |bias|,
    which bounds the pooled error through |max a - max b| <= max |a - b|."""
    if planar:
        xs = _d(x).reshape(B, 3, H, W).permute(0, 2, 3, 1).reshape(-1)
        wp = _d(w).reshape(-1, 160)[:64, :156].reshape(64, 3, 52)[:, :, :49].reshape(64, 3, 7, 7)
        wk = _zeros(64, 160)
        wk[:, :147] = wp.permute(0, 2, 3, 1).reshape(64, 147)
        d = _StemDesc(B, H, W, 3, 160)
    else:
        xs, wk, d = _d(x).reshape(-1), _d(w).reshape(-1, 208)[:64], _StemDesc(B, H, W, 4, 208)
    y, a = conv_ref(d, xs, wk, bias, None, _zeros(B * d.Ho * d.Wo * 64))
    y = conv_act(y, act)
    return maxpool3x3s2_nhwc(y, B, d.Ho, d.Wo, 64), maxpool3x3s2_nhwc(a, B, d.Ho, d.Wo, 64)
