"""tests/kernel_refs.py against the ATen operators and oracle functions it restates, on the CPU, at ragged shapes of
tests/test_gpu_kernel_edges.py: a restatement that is wrong at an odd size would hide a kernel bug there, or invent one."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
from oracle import hamer_oracle as H
from oracle import handoccnet_oracle as HO
from oracle import hands_oracle as O
from oracle import metrics_oracle as MO
from oracle import wrapper_oracle as WO

F64 = 1e-12          # two float64 evaluations of one formula in different orders


def _rand(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("B,h,w,H,W,C", [(2, 5, 3, 7, 8, 8), (2, 8, 8, 5, 3, 4), (1, 1, 1, 4, 4, 4), (2, 6, 6, 6, 6, 8), (1, 8, 8, 16, 16, 4)])
def test_bilinear_upsample_add(B, h, w, H, W, C):
    x, y = _rand(0, B, h, w, C), _rand(1, B, H, W, C)
    ref = F.interpolate(_nchw(x), size=(H, W), mode="bilinear", align_corners=False) + _nchw(y)
    assert (_nchw(R.upsample_bilinear_add(x, y, B, h, w, H, W, C)) - ref).abs().max().item() < F64


@pytest.mark.parametrize("B,Hin,Win,S,col0,Wc", [(2, 100, 180, 64, 0, 64), (1, 300, 200, 96, 10, 70), (1, 1, 1, 8, 2, 3), (2, 224, 224, 256, 32, 192)])
def test_resize_crop(B, Hin, Win, S, col0, Wc):
    x = _rand(2, B, 3, Hin, Win)
    ref = F.interpolate(x, size=S, mode="bilinear", align_corners=False)[:, :, :, col0:col0 + Wc]
    got = R.resize_crop_nchw3_to_nhwc4(x, B, Hin, Win, S, col0, Wc)
    assert got.shape == (B, S, Wc, 4) and torch.all(got[..., 3] == 0)
    assert (_nchw(got[..., :3]) - ref).abs().max().item() < F64


@pytest.mark.parametrize("M,C,rpv,eps", [(5, 256, 1, 1e-5), (37, 768, 4, 1e-6), (4, 1280, 4, 1e-6)])
def test_layernorm(M, C, rpv, eps):
    x, gam, bet = 1000 + _rand(3, M, C), _rand(4, C), _rand(5, C)
    vec = _rand(6, (M + rpv - 1) // rpv, C)
    e32 = R._f32(eps)
    ref = F.layer_norm(x, (C,), gam, bet, e32)
    assert (R.layernorm(x, gam, bet, None, 1, M, C, eps) - ref).abs().max().item() < 1e-9       # rstd of a 1000 + randn row
    ref = ref + vec[torch.arange(M) // rpv]
    assert (R.layernorm(x, gam, bet, vec, rpv, M, C, eps) - ref).abs().max().item() < 1e-9
    const = torch.full((2, C), 3.25, dtype=torch.float64)
    assert torch.equal(R.layernorm(const, gam, bet, None, 1, 2, C, eps), bet.expand(2, C))


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (2, 6, 14, 8)])
def test_pool2x2(B, H, W, C):
    x = _rand(7, B, H, W, C)
    assert (_nchw(R.pool2x2_nhwc(x, B, H, W, C, 0)) - F.avg_pool2d(_nchw(x), 2, 2)).abs().max().item() < F64
    assert torch.equal(_nchw(R.pool2x2_nhwc(x, B, H, W, C, 1)), F.max_pool2d(_nchw(x), 2, 2))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 2, 5, 8), (2, 17, 14, 64)])
def test_maxpool3x3s2(B, H, W, C):
    x = _rand(8, B, H, W, C)
    assert torch.equal(_nchw(R.maxpool3x3s2_nhwc(x, B, H, W, C)), F.max_pool2d(_nchw(x), 3, 2, 1))


@pytest.mark.parametrize("B,h,w,C", [(1, 1, 3, 4), (2, 5, 7, 8)])
def test_nearest_upsample_add(B, h, w, C):
    low, up1 = _rand(9, B, h, w, C), _rand(10, B, 2 * h, 2 * w, C)
    ref = _nchw(up1) + F.interpolate(_nchw(low), scale_factor=2, mode="nearest")
    assert torch.equal(_nchw(R.upsample_nearest2x_add(low, up1, B, h, w, C)), ref)


def _explicit_attention(q, k, v, scale):
    """(B, heads, T, D) each: softmax(q k^T scale) v, one row at a time with exp and a sum -- no torch.softmax."""
    s = torch.einsum("bhqd,bhkd->bhqk", q, k) * scale
    e = torch.exp(s - s.max(-1, keepdim=True)[0])
    return torch.einsum("bhqk,bhkd->bhqd", e / e.sum(-1, keepdim=True), v)


@pytest.mark.parametrize("B,T,heads,D", [(1, 197, 1, 64), (2, 192, 3, 80)])
def test_attention(B, T, heads, D):
    qkv = _rand(11, B, T, 3 * heads * D)
    scale = D ** -0.5
    q, k, v = qkv.view(B, T, 3, heads, D).permute(2, 0, 3, 1, 4)
    ref = _explicit_attention(q, k, v, R._f32(scale)).transpose(1, 2).reshape(B, T, heads * D)
    assert (R.attention(qkv, B, T, heads, D, scale) - ref).abs().max().item() < F64


@pytest.mark.parametrize("B,T,heads", [(1, 1, 1), (3, 65, 8)])
def test_cross_attention_1q(B, T, heads):
    D = 64
    q, kv = _rand(12, B, heads * D), _rand(13, B, T, 2 * heads * D)
    k, v = kv[..., :heads * D], kv[..., heads * D:]
    sp = lambda z: z.reshape(B, -1, heads, D).transpose(1, 2)
    ref = _explicit_attention(sp(q[:, None]), sp(k), sp(v), R._f32(0.1)).transpose(1, 2).reshape(B, heads * D)
    assert (R.cross_attention_1q(q, kv, B, T, heads, D, 0.1) - ref).abs().max().item() < F64


@pytest.mark.parametrize("scale", [0.125, 0.1])
def test_flash_attention(scale):
    """Against the explicit product with the gate sigmoid((q2 . sum_j k2_j) scale) and the residual written out; at scale 0.125
    also against the oracle's attention given the full k2, which the restatement replaces by its token sum."""
    B, N, heads, D = 2, 128, 3, 64
    C = heads * D
    q, k, v, q2, k2, res = (_rand(20 + i, B, N, C) for i in range(6))
    k2 = 0.05 * k2
    k2sum = k2.sum(1)
    sp = lambda z: z.reshape(B, -1, heads, D).transpose(1, 2)
    s32 = R._f32(scale)
    plain = _explicit_attention(sp(q), sp(k), sp(v), s32)
    gate = torch.sigmoid((sp(q2) * sp(k2sum[:, None])).sum(-1, keepdim=True) * s32)
    un = lambda z: z.transpose(1, 2).reshape(B, N, C)
    assert (R.flash_attention(q, k, v, None, None, None, B, N, heads, D, scale) - un(plain)).abs().max().item() < F64
    assert (R.flash_attention(q, k, v, q2, k2sum, None, B, N, heads, D, scale) - un(plain * gate)).abs().max().item() < F64
    assert (R.flash_attention(q, k, v, None, None, res, B, N, heads, D, scale) - (res + un(plain))).abs().max().item() < F64
    assert (R.flash_attention(q, k, v, q2, k2sum, res, B, N, heads, D, scale) - (res + un(plain * gate))).abs().max().item() < F64
    if scale == 0.125:
        ref = HO.attention(q, k, v, q2, k2, heads, True)
        assert (R.flash_attention(q, k, v, q2, k2sum, None, B, N, heads, D, scale) - ref).abs().max().item() < F64


def test_spatial_softmax():
    B, N, J, ld_in, ld_out = 2, 100, 21, 24, 32
    lat, betas = 20 * _rand(30, B, N, ld_in), 1 + 0.2 * _rand(31, J)
    got = R.spatial_softmax(lat, ld_in, betas, ld_out, B, N, J)
    assert got.shape == (B, N, ld_out) and torch.all(got[:, :, J:] == 0)
    assert (got[:, :, :J] - F.softmax(lat[:, :, :J] * betas, dim=1)).abs().max().item() < F64
    assert (got[:, :, :J].sum(1) - 1).abs().max().item() < F64
    assert torch.equal(R.spatial_softmax(lat[:, :1], ld_in, betas, J, B, 1, J), torch.ones(B, 1, J, dtype=torch.float64))


def test_streaming_and_reduction_restatements():
    B, N, C = 3, 17, 128
    x, key = _rand(40, B, N, C), _rand(41, B, N, C)
    qe, ke, kp = _rand(42, N, C), _rand(43, N, C), _rand(44, B, C)
    oq, ok = R.add_embed2(x, key, qe, ke, kp, B, N, C)
    assert torch.equal(oq, (x + qe) + kp[:, None]) and torch.equal(ok, (key + ke) + kp[:, None])
    assert torch.equal(R.add_rowvec(x, kp, B, N, C), x + kp[:, None])
    assert (R.token_sum(x, B, N, C) - torch.einsum("bnc->bc", x)).abs().max().item() < F64
    pos = _rand(45, N + 1, C)
    assert torch.equal(R.add_pos(x, pos, kp, B, N, C), ((x + pos[1:]) + pos[:1]) + kp[:, None])
    assert torch.equal(R.add_pos(x, pos, None, B, N, C), (x + pos[1:]) + pos[:1])
    cls = _rand(46, C)
    tok = R.vit_tokens(x, cls, pos, B, N + 1, C)
    assert torch.equal(tok[:, 0], (cls + pos[0]).expand(B, C)) and torch.equal(tok[:, 1:], x + pos[1:])
    sc, sh = _rand(47, C).abs() + 0.5, _rand(48, C)
    xs = x.clone()
    xs.view(-1)[::7] = 0.0
    assert (R.bn_leaky(xs, sc, sh, B * N, C) - F.leaky_relu(xs.view(-1, C) * sc + sh, 0.01)).abs().max().item() < F64
    for stride in (1, 4):
        logit = _rand(49, B * N * stride)
        s = torch.sigmoid(logit[::stride])[:, None]
        pr, se = R.gate_apply(x, logit, stride, B * N, C)
        assert (pr - x.view(-1, C) * s).abs().max().item() < F64 and (se - x.view(-1, C) * (1 - s)).abs().max().item() < F64
    img = _rand(50, 2, 3, 5, 7)
    out = R.nchw3_to_nhwc4(img, 2, 5, 7)
    assert torch.equal(out[..., :3], img.permute(0, 2, 3, 1)) and torch.all(out[..., 3] == 0)
    feat = _rand(51, 2, 49, 8)
    assert (R.sumpool_nhwc(feat, 2, 49, 8, 12) - feat.sum(1)).abs().max().item() < F64
    assert (R.avgpool_nhwc(feat, 2, 49, 8, 12) - F.adaptive_avg_pool2d(feat.permute(0, 2, 1).reshape(2, 8, 7, 7), 1).view(2, 8)).abs().max().item() < F64
    xc = _rand(52, 5, 256)
    cp = R.channel_pool(xc, 5, 256)
    assert torch.equal(cp[:, 0], xc.max(1)[0]) and (cp[:, 1] - xc.mean(1)).abs().max().item() < F64 and torch.all(cp[:, 2:] == 0)


@pytest.mark.parametrize("ld,n_freq", [(84, 4), (20, 1), (320, 16)])
def test_kpe_encode(ld, n_freq):
    B = 3
    ce, co = 1e-3 * _rand(60, B, 2), 1e-3 * _rand(61, B, 8)
    got = R.kpe_encode(ce, co, B, ld, n_freq)
    assert torch.equal(got[:, :20 * n_freq].float(), torch.cat([O.pos_enc(ce, n_freq), O.pos_enc(co, n_freq)], 1))
    assert torch.all(got[:, 20 * n_freq:] == 0)
    # the layout written out: element ((k * nc + c) * 2 + {0: sin, 1: cos}) of an nc-component block
    k, c = n_freq - 1, 1
    assert abs(got[2, (k * 2 + c) * 2 + 1].item() - torch.cos(2.0 ** k * ce[2, c]).item()) < 1e-7
    assert abs(got[1, 4 * n_freq + (k * 8 + 5) * 2].item() - torch.sin(2.0 ** k * co[1, 5]).item()) < 1e-7


def test_rot6d_columns():
    d6 = _rand(70, 4, 112)
    d6[1, :6] = torch.tensor([3.0, 0, 0, 5.0, 0, 0])           # parallel: b2 = 0 / 1e-12 = 0
    d6[2, 6:12] = 0.0
    got = R.rot6d_to_matrix_cols(d6, 112, 4)
    assert torch.equal(got, H.rot6d_to_rotmat_columns(d6[:, :96].reshape(-1, 6)).view(4, 16, 3, 3))
    assert torch.isfinite(got).all()
    assert torch.equal(got[1, 0], torch.tensor([[1.0, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.float64))
    assert torch.all(got[2, 1] == 0)
    good = got[0]
    assert (good.transpose(-1, -2) @ good - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-12
    a1 = d6[0, :3]
    assert (good[0, :, 0] - a1 / a1.norm()).abs().max().item() < 1e-15       # b1 is the first COLUMN


@pytest.mark.parametrize("B,G", [(1, 2), (2, 6)])
def test_vit_tail(B, G):
    C, eps = 768, 1e-6
    x, gam, bet = _rand(80, B, 1 + G * G, C), _rand(81, C), _rand(82, C)
    y = F.layer_norm(x[:, 1:], (C,), gam, bet, R._f32(eps))
    ref = F.avg_pool2d(y.permute(0, 2, 1).reshape(B, C, G, G), 2).permute(0, 2, 3, 1)
    assert (R.vit_tail(x, gam, bet, B, G, C, eps) - ref).abs().max().item() < 1e-11


# ---- the glue kernels of csrc/elementwise.hip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_freq", [1, 4, 16])
def test_pos_enc_and_its_two_concatenations(n_freq):
    B2, Bg, HW, C = 4, 2, 3, 8
    ce, co = 1e-3 * _rand(100, B2, 2).float().double(), 1e-3 * _rand(101, B2, 8).float().double()
    assert torch.equal(R._pos_enc(ce, n_freq).float(), O.pos_enc(ce, n_freq))
    crop, glb = _rand(102, B2, HW, C), _rand(103, Bg, HW, C)
    nchw = lambda t: t.permute(0, 2, 1).reshape(t.shape[0], C, HW, 1)
    ref = O.assemble_features(nchw(crop), nchw(glb).repeat(2, 1, 1, 1), ce, co, n_freq)[..., 0].permute(0, 2, 1)
    got = R.kpe_concat(crop, glb, ce, co, B2, Bg, HW, C, n_freq)
    assert got.shape == (B2, HW, C + 20 * n_freq) and torch.equal(got[..., :C], ref[..., :C])
    assert torch.equal(got[..., C:].float().double(), ref[..., C:])             # the oracle rounds its encodings to float32
    assert torch.equal(R.kpe_concat(crop, None, ce, co, B2, Bg, HW, C, n_freq)[..., :C], crop)
    img = _rand(104, B2, 3, 2, 3)
    for mode, Cpad in ((1, 3 + 4 * n_freq + 5), (2, 3 + 16 * n_freq + 1), (3, 3 + 20 * n_freq + 1)):
        Cpad = (Cpad + 3) // 4 * 4
        out = R.image_posenc_nhwc(img, ce, co, B2, 2, 3, n_freq, mode, Cpad)
        enc = torch.cat(([R._pos_enc(ce, n_freq)] if mode & 1 else []) + ([R._pos_enc(co, n_freq)] if mode & 2 else []), 1)
        assert out.shape == (B2, 2, 3, Cpad) and torch.equal(out[..., :3], img.permute(0, 2, 3, 1))
        assert torch.equal(out[:, 1, 2, 3:3 + enc.shape[1]], enc) and torch.all(out[..., 3 + enc.shape[1]:] == 0)


@pytest.mark.parametrize("Hs,Ws,R_,Ho,Wo", [(5, 9, 12, 7, 10), (5, 9, 1, 1, 1), (6, 6, 6, 6, 6), (5, 9, 5, 3, 4)])
def test_dense_posenc(Hs, Ws, R_, Ho, Wo):
    """Against the oracle's dense_pos_enc / cam_conv_pos_enc (first resize, square) followed by ATen's second resize."""
    B, Ca, nf = 2, 2, 3
    ang = _rand(110, B, Ca, Hs, Ws).float().double()
    msk = (_rand(111, B, Hs, Ws) > -0.5).double()
    two = lambda t: F.interpolate(t, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    got = R.dense_posenc(ang, msk, None, B, Ca, Hs, Ws, nf, R_, Ho, Wo, 16, 4)
    # the oracle rounds sin / cos to float32 before the mask and the resize: 6e-8 per tap, weights sum to 1
    assert got.shape == (B, Ho, Wo, 2 * nf * Ca) and (got - two(O.dense_pos_enc(ang, msk, nf, R_).double())).abs().max().item() < 1.2e-7
    raw = R.dense_posenc(ang, msk, None, B, Ca, Hs, Ws, 0, R_, Ho, Wo, 8, 0)
    assert (raw - two(O.cam_conv_pos_enc(ang, msk, R_))).abs().max().item() < F64
    img = _rand(112, B, 3, Ho, Wo)
    full = R.dense_posenc(ang, msk, img, B, Ca, Hs, Ws, nf, R_, Ho, Wo, 16, 3)
    assert full.shape == (B, Ho, Wo, 16) and torch.equal(full[..., :3], img.permute(0, 2, 3, 1))
    assert torch.equal(full[..., 3:15], got) and torch.all(full[..., 15:] == 0)


def test_concat_upsample_and_row_assemblies():
    B, Bg, HW, Ca, lda, Cb, ld, ld_add = 4, 2, 5, 6, 9, 3, 12, 7
    a, add, ex = _rand(120, B, HW, lda), _rand(121, Bg, HW, ld_add), _rand(122, B, HW, Cb)
    ref = torch.cat([a[..., :Ca] + add.repeat(2, 1, 1)[..., :Ca], ex, torch.zeros(B, HW, ld - Ca - Cb, dtype=torch.float64)], -1)
    assert torch.equal(R.concat_nhwc(a, lda, Ca, add, ld_add, ex, HW * Cb, Cb, ld, B, Bg, HW), ref)
    ref = torch.cat([a[..., :Ca], ex[:1].repeat(B, 1, 1), torch.zeros(B, HW, ld - Ca - Cb, dtype=torch.float64)], -1)
    assert torch.equal(R.concat_nhwc(a, lda, Ca, None, 0, ex, 0, Cb, ld, B, Bg, HW), ref)
    assert torch.equal(R.concat_nhwc(a, lda, Ca, None, 0, None, 0, 0, ld, B, Bg, HW)[..., Ca:], torch.zeros(B, HW, ld - Ca, dtype=torch.float64))
    x = _rand(123, 2, 5, 7, 4)
    for H_, W_ in ((11, 13), (1, 9), (5, 3)):
        ref = F.interpolate(_nchw(x), size=(H_, W_), mode="bilinear", align_corners=True)
        assert torch.equal(_nchw(R.upsample_bilinear_ac(x, 2, 5, 7, H_, W_, 4)), ref)
    # align_corners written out at one pixel: src = dst (in - 1) / (out - 1)
    sy, sx = 3 * 4 / 10, 8 * 6 / 12
    y0, x0 = int(sy), int(sx)
    ly, lx = sy - y0, sx - x0
    want = (1 - ly) * ((1 - lx) * x[1, y0, x0] + lx * x[1, y0, min(x0 + 1, 6)]) + ly * ((1 - lx) * x[1, y0 + 1, x0] + lx * x[1, y0 + 1, min(x0 + 1, 6)])
    assert (R.upsample_bilinear_ac(x, 2, 5, 7, 11, 13, 4)[1, 3, 8] - want).abs().max().item() < F64
    B2, F_, ldo, lds = 6, 5, 170, 12
    shape, rot, fv = _rand(124, B2, lds), _rand(125, B2, 16, 3, 3), _rand(126, 3, F_)
    gi = R.grasp_input(shape, lds, rot, fv, B2, 3, F_, ldo)
    assert torch.equal(gi, torch.cat([fv.repeat(2, 1), rot.view(B2, 144), shape[:, :10], torch.zeros(B2, ldo - F_ - 154, dtype=torch.float64)], 1))
    assert torch.equal(R.grasp_input(shape, lds, rot, fv, B2, 3, 0, 154), torch.cat([rot.view(B2, 144), shape[:, :10]], 1))
    state, cam = _rand(127, 3, 120), _rand(128, 3, 4)
    st = R.hmr_init(state, cam, 3, 120, 4)
    ident = O.matrix_to_rotation_6d(torch.eye(3, dtype=torch.float64)).repeat(16)
    assert torch.equal(st[:, :4], state[:, :4]) and torch.equal(st[:, 116:], state[:, 116:])
    assert torch.equal(st[:, 4:100], ident.expand(3, 96)) and torch.all(st[:, 100:112] == 0) and torch.equal(st[:, 112:115], cam[:, :3])
    assert torch.all(st[:, 115] == 0)


def test_rotation_restatements():
    B = 3
    d6 = _rand(130, B, 100)
    got = R.rot6d_to_matrix(d6, 100, B)
    assert torch.equal(got, O.rotation_6d_to_matrix(d6[:, :96].reshape(-1, 6)).view(B, 16, 3, 3))
    assert (got[0, 0] @ got[0, 0].T - torch.eye(3, dtype=torch.float64)).abs().max().item() < 1e-12
    assert (got[0, 0, 0] - d6[0, :3] / d6[0, :3].norm()).abs().max().item() < 1e-15      # b1 is the first ROW
    rot = O.axis_angle_to_matrix(_rand(131, 2 * B, 16, 3))
    fix = O.axis_angle_to_matrix(_rand(132, 2 * B, 3))
    lm = R.rot_leftmul(rot, fix, 2 * B)
    assert (lm[:, 0] - torch.bmm(fix, rot[:, 0])).abs().max().item() < F64 and torch.equal(lm[:, 1:], rot[:, 1:])
    center = 0.4 * _rand(133, 2 * B, 2)
    from scipy.spatial.transform import Rotation
    e = torch.from_numpy(Rotation.from_euler("XYZ", torch.cat([-center, torch.zeros(2 * B, 1, dtype=torch.float64)], -1).numpy()).as_matrix())
    for flips in ([0, 0, 0], [0, 1, 0]):
        sw, un = R.perspective_correction(rot, rot, center, torch.tensor(flips), B)
        assert (sw[:, 0] - e @ rot[:, 0]).abs().max().item() < F64 and torch.equal(sw[:, 1:], rot[:, 1:])
        assert torch.equal(un, rot if any(flips) else sw)


# ---- csrc/metrics.hip ---------------------------------------------------------------------------------------------------------
_EVAL_IN = ("pred.mano.j3d.cam.r", "pred.mano.j3d.cam.l", "targets.mano.j3d.cam.r", "targets.mano.j3d.cam.l", "pred.mano.j2d.r",
            "pred.mano.j2d.l", "targets.mano.j2d.r", "targets.mano.j2d.l", "targets.is_valid", "targets.right_valid",
            "targets.left_valid", "targets.joints_valid_r", "targets.joints_valid_l")
_EVAL_OUT = ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l", "pix_err/r", "pix_err/l")


def test_eval_metrics_on_the_reference_fixture(golden_dir):
    """Against oracle.metrics_oracle.evaluate, which evaluates in float32 where the reference does: its own distance to the
    fixture is rtol 1e-5 + atol 2e-4 (tests/test_metrics.py); NaN in the same places."""
    d = np.load(os.path.join(golden_dir, "eval_metrics.npz"))
    pred = {k[len("in/pred."):]: d[k] for k in d.files if k.startswith("in/pred.")}
    targets = {k[len("in/targets."):]: d[k] for k in d.files if k.startswith("in/targets.")}
    ref = MO.evaluate(pred, targets)
    B = len(d["in/targets.is_valid"])
    got = R.eval_metrics(*[torch.from_numpy(d["in/" + k]) for k in _EVAL_IN], B)
    for k, g in zip(_EVAL_OUT, got):
        assert g.dtype == torch.float64 and g.shape == ref[k].shape, k
        np.testing.assert_array_equal(np.isnan(g.numpy()), np.isnan(ref[k]), err_msg=k)
        np.testing.assert_allclose(g.numpy(), ref[k], rtol=1e-5, atol=2e-4, equal_nan=True, err_msg=k)
        np.testing.assert_allclose(g.numpy(), d["out/" + k], rtol=1e-5, atol=2e-4, equal_nan=True, err_msg=k)


def test_procrustes_restatement_on_rank_deficient_hands():
    """oracle.metrics_oracle.similarity_transform (np.linalg.svd) on joints on a line, both ways round: the error is unique there
    (it does not depend on how LAPACK completes the singular frame), 128.566 mm for the prediction on a line in any direction."""
    rng = np.random.default_rng(1)
    gt = (0.1 * rng.standard_normal((1, 21, 3))).astype(np.float32)
    a = rng.integers(-64, 64, (1, 21, 1)) / 512
    a[0, 0] = 0
    for dvec in ((1, 0, 0), (1, 2, 0), (1, 1, 1), (3, 5, 7)):
        line = (a * np.array(dvec, np.float64)).astype(np.float32)
        for g, p in ((gt, line), (line, gt)):
            g0, p0 = (g - g[:, :1]).astype(np.float64)[0], (p - p[:, :1]).astype(np.float64)[0]
            want = np.mean(np.sqrt(np.sum((g0 - MO.similarity_transform(p0, g0)) ** 2, axis=1))) * 1000
            got = R._procrustes_mean_error(torch.from_numpy(g0)[None], torch.from_numpy(p0)[None]).item() * 1000
            assert abs(got - want) < 1e-9, (dvec, got, want)
            if p is line:
                assert abs(got - 128.566210) < 1e-5
    const = torch.zeros(1, 21, 3, dtype=torch.float64)
    g0 = torch.from_numpy((gt - gt[:, :1]).astype(np.float64))
    assert torch.isnan(R._procrustes_mean_error(g0, const)).all() and R._procrustes_mean_error(const, g0).item() == 0.0


def test_gt_targets_and_unnormalize():
    B, NV = 3, 257
    jc, jf, verts = 0.1 * _rand(140, B, 21, 3), 0.1 * _rand(141, B, 21, 3) + torch.tensor([0.0, 0.0, 0.8]), 0.1 * _rand(142, B, NV, 3)
    K = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 900.0, 1100.0
    v3d, cam_t, wp = R.gt_targets(jc, verts, jf, K, 224.0, B, NV)
    assert (v3d - (verts + (jf - jc).mean(1)[:, None])).abs().max().item() < F64 and torch.equal(cam_t, jf[:, 0] - jc[:, 0])
    assert (wp - WO.perspective_to_weak_perspective(cam_t, torch.full((B,), 1000.0, dtype=torch.float64), 224)).abs().max().item() < F64
    x = _rand(143, 50)
    assert torch.equal(R.unnormalize_kp2d(x, 50, 57.0), WO.unnormalize_kp2d(x, 57))


# ---- conv_ref: the convolution entry points (tests/test_gpu_conv_edges.py) ---------------------------------------------------
class _Desc:
    """The fields of hands_conv_desc; strides default to the channel counts, the output map to the geometry's, Kpad to K."""

    def __init__(self, B, H, W, Cin, Cout, KH, KW, stride, pad, act=0, Ho=None, Wo=None, in_ps=None, out_ps=None, res_ps=None, Kpad=None):
        self.B, self.H, self.W, self.Cin, self.Cout, self.KH, self.KW, self.stride, self.pad, self.act = B, H, W, Cin, Cout, KH, KW, stride, pad, act
        self.Ho = Ho or (H + 2 * pad - KH) // stride + 1
        self.Wo = Wo or (W + 2 * pad - KW) // stride + 1
        self.in_pix_stride, self.out_pix_stride = in_ps or Cin, out_ps or Cout
        self.res_pix_stride = Cout if res_ps is None else res_ps
        self.Kpad = Kpad or KH * KW * Cin


def _conv_bufs(d, seed, res=True, dual=None):
    """Random flat buffers for `d`: x, packed w [Cout][Kpad] (zero beyond K, or W1 of the dual form), bias, res, out."""
    K = d.KH * d.KW * d.Cin
    x = _rand(seed, d.B * d.H * d.W * d.in_pix_stride)
    w = _rand(seed + 1, d.Cout, d.Kpad)
    w[:, K + (dual[1] if dual else 0):] = 0
    bias = _rand(seed + 2, d.Cout)
    M = d.B * d.Ho * d.Wo
    r = _rand(seed + 3, max(1, M if d.res_pix_stride else 1) * max(d.res_pix_stride, d.Cout)) if res else None
    out = _rand(seed + 4, M * d.out_pix_stride)
    return x, w, bias, r, out


def _conv_loops(d, x, w, bias, res, out, pre=None, dual=None):
    """The header's formula as a loop nest over Python floats: out[m, n] = act(bias[n] + sum_k patch(m, k) w[n, k] (+ res[m, n]))."""
    x, w, bias, out = x.tolist(), w.tolist(), bias.tolist(), out.clone().tolist()
    res = None if res is None else res.tolist()
    leaky = lambda v: v if v > 0 else 0.01 * v
    for b in range(d.B):
        for ho in range(d.Ho):
            for wo in range(d.Wo):
                m = (b * d.Ho + ho) * d.Wo + wo
                for n in range(d.Cout):
                    acc = bias[n]
                    for kh in range(d.KH):
                        for kw in range(d.KW):
                            hi, wi = ho * d.stride - d.pad + kh, wo * d.stride - d.pad + kw
                            if not (0 <= hi < d.H and 0 <= wi < d.W):
                                continue
                            for c in range(d.Cin):
                                v = x[((b * d.H + hi) * d.W + wi) * d.in_pix_stride + c]
                                if pre is not None:
                                    v = leaky(v * pre[0][c].item() + pre[1][c].item())
                                acc += v * w[n][(kh * d.KW + kw) * d.Cin + c]
                    if dual is not None:
                        x2, Cin2, H2, W2, s2, ps2 = dual
                        for c in range(Cin2):
                            acc += x2[((b * H2 + ho * s2) * W2 + wo * s2) * ps2 + c].item() * w[n][d.Cin + c]
                    if res is not None:
                        acc += res[m * d.res_pix_stride + n]
                    act = d.act & 0xff
                    if act == 1:
                        acc = max(acc, 0.0)
                    elif act == 2:
                        acc = acc * 0.5 * (1 + math.erf(acc / math.sqrt(2)))
                    elif act == 3:
                        acc = leaky(acc)
                    out[m * d.out_pix_stride + n] = acc
    return torch.tensor(out, dtype=torch.float64)


CONV_REF_FEATURES = {
    "plain": dict(),
    "in_ps": dict(in_ps=7),
    "out_ps": dict(out_ps=6),
    "res_ps": dict(res_ps=9),
    "res_row": dict(res_ps=0),
    "all_strides": dict(in_ps=8, out_ps=8, res_ps=12),
    "crop_corner": dict(Ho=2, Wo=3),
    "crop_row": dict(Ho=1),
    "crop_pixel": dict(Ho=1, Wo=1),
    "crop_strided": dict(Ho=2, Wo=2, out_ps=5, in_ps=6),
    "k1x3": dict(KH=1, KW=3, pad=0),
    "k3x1": dict(KH=3, KW=1, pad=0),
    "k5x3": dict(KH=5, KW=3, pad=1, H=6, W=5),
    "patch_half": dict(KH=2, KW=4, stride=4, pad=0, H=4, W=8, Ho=1),
    "kpad16": dict(Kpad=36 + 16),
    "kpad48": dict(Kpad=36 + 48),
    "stride2_odd": dict(stride=2, H=5, W=7),
    "pointwise_s2": dict(KH=1, KW=1, pad=0, stride=2, H=5, W=3),
    "relu": dict(act=1),
    "gelu": dict(act=2),
    "leaky": dict(act=3),
    "flags_ignored": dict(act=3 | 0x400),
}


@pytest.mark.parametrize("name", sorted(CONV_REF_FEATURES))
@pytest.mark.parametrize("use_res", [False, True])
def test_conv_ref_against_the_loop_nest(name, use_res):
    kw = dict(B=2, H=4, W=5, Cin=4, Cout=4, KH=3, KW=3, stride=1, pad=1)
    kw.update(CONV_REF_FEATURES[name])
    d = _Desc(**kw)
    x, w, bias, r, out = _conv_bufs(d, 100, res=use_res)
    exp, mag = R.conv_ref(d, x, w, bias, r, out)
    ref = _conv_loops(d, x, w, bias, r, out)
    assert exp.shape == out.shape and (exp - ref).abs().max().item() < F64
    written = torch.zeros(out.numel(), dtype=torch.bool)
    for m in range(d.B * d.Ho * d.Wo):
        written[m * d.out_pix_stride: m * d.out_pix_stride + d.Cout] = True
    assert torch.equal(exp[~written], out[~written]) and torch.all(mag[~written] == 0)      # gaps as they were
    assert torch.all(mag[written] >= exp[written].abs() * (1 - 1e-12))                      # |act(y)| <= |y| <= A
    ones = R.conv_ref(d, x.abs(), w.abs(), bias.abs(), None if r is None else r.abs(), out)[0 if (d.act & 0xff) != 2 else 1]
    if (d.act & 0xff) != 2:
        assert (mag[written] - ones[written]).abs().max().item() < F64                      # A is the result on magnitudes


def test_conv_ref_in_place_residual_and_pre_and_dual():
    d = _Desc(2, 3, 4, 4, 4, 1, 1, 1, 0, act=1, out_ps=6, res_ps=6)
    x, w, bias, _, out = _conv_bufs(d, 200, res=False)
    exp, _ = R.conv_ref(d, x, w, bias, out, out)                                            # the residual IS the output buffer
    assert (exp - _conv_loops(d, x, w, bias, out, out)).abs().max().item() < F64
    d = _Desc(2, 3, 4, 4, 8, 1, 1, 1, 0, act=3, in_ps=5)
    x, w, bias, r, out = _conv_bufs(d, 210)
    pre = (_rand(5, 4).float() + 1.5, _rand(6, 4).float())
    x = x.float().double()                                                                  # fp32 data: the operand is staged in fp32
    exp, _ = R.conv_ref(d, x, w, bias, r, out, pre=pre)
    assert (exp - _conv_loops(d, x, w, bias, r, out, pre=pre)).abs().max().item() < 1e-5    # fp32 operand against fp64 loops
    op = F.leaky_relu(R._pixels(x, 24, 5, 4).float() * pre[0] + pre[1], 0.01)
    d2 = _Desc(2, 3, 4, 4, 8, 1, 1, 1, 0, act=3)
    assert torch.equal(R.conv_ref(d2, op.reshape(-1), w, bias, r, out)[0], exp)             # = hands_bn_leaky_f32, then the layer
    for s2, H2, W2 in ((1, 3, 4), (2, 5, 7), (2, 6, 8)):
        d = _Desc(2, 3, 4, 4, 4, 1, 1, 1, 0, act=1, Kpad=4 + 8, in_ps=6, out_ps=5)
        dual = (_rand(220, 2 * H2 * W2 * 10), 8, H2, W2, s2, 10)
        x, w, bias, _, out = _conv_bufs(d, 230, res=False, dual=dual)
        exp, mag = R.conv_ref(d, x, w, bias, None, out, dual=dual)
        assert (exp - _conv_loops(d, x, w, bias, None, out, dual=dual)).abs().max().item() < F64
        assert torch.all(mag >= exp.abs() * (1 - 1e-12) * (mag > 0))


@pytest.mark.parametrize("B,Cin,H,W,Cout,KH,KW,stride,pad,act", [
    (3, 16, 5, 11, 140, 3, 3, 1, 1, 1), (2, 32, 9, 7, 20, 1, 1, 2, 0, 3), (2, 4, 9, 11, 64, 7, 7, 2, 3, 1), (1, 48, 6, 8, 12, 5, 3, 1, 2, 2),
    (2, 16, 8, 16, 8, 8, 16, 16, 0, 0)])
def test_conv_ref_against_aten(B, Cin, H, W, Cout, KH, KW, stride, pad, act):
    d = _Desc(B, H, W, Cin, Cout, KH, KW, stride, pad, act=act)
    x, w, bias, r, out = _conv_bufs(d, 300)
    wt = w.view(Cout, KH, KW, Cin).permute(0, 3, 1, 2)
    ref = F.conv2d(_nchw(x.view(B, H, W, Cin)), wt, bias, stride, pad) + _nchw(r.view(B, d.Ho, d.Wo, Cout))
    ref = {0: lambda t: t, 1: F.relu, 2: F.gelu, 3: lambda t: F.leaky_relu(t, 0.01)}[act](ref)
    exp, mag = R.conv_ref(d, x, w, bias, r, out)
    assert (_nchw(exp.view(B, d.Ho, d.Wo, Cout)) - ref).abs().max().item() < F64
    with R.precision(torch.float32):
        e32, _ = R.conv_ref(d, x, w, bias, r, out)
    assert e32.dtype == torch.float32 and (e32.double() - exp).abs().max().item() < 1e-4
    # HANDS_ACC_F64: one rounding of sum + bias, then residual and activation in float32
    if act != 2:
        rs, _ = R.conv_ref(d, x.float(), w.float(), bias.float(), r.float(), out.float(), round_sum=True)
        s = F.conv2d(_nchw(x.float().double().view(B, H, W, Cin)), wt.float().double(), bias.float().double(), stride, pad).float()
        s = s + _nchw(r.float().view(B, d.Ho, d.Wo, Cout))
        s = {0: lambda t: t, 1: F.relu, 3: lambda t: F.leaky_relu(t, 0.01)}[act](s)
        assert (_nchw(rs.view(B, d.Ho, d.Wo, Cout)) != s.double()).float().mean().item() < 1e-3      # ties of the fp64 sum's order only


# ---- stem_pool_ref: the fused stem entries (tests/test_gpu_wino_stem_edges.py) -------------------------------------------------
@pytest.mark.parametrize("B,H,W,act,negative", [
    (1, 25, 29, 1, False), (1, 25, 29, 3, False),          # Hc = 13, Wc = 15: the last pool windows have two taps per axis
    (2, 7, 7, 0, True), (2, 29, 33, 3, True)])             # every convolution output negative: a 0 as pool padding would win
def test_stem_pool_ref_against_aten(B, H, W, act, negative):
    x, w, bias = _rand(400, B, 3, H, W), _rand(401, 64, 3, 7, 7) / 147 ** 0.5, _rand(402, 64)
    if negative:                       # the construction of test_stem_all_negative: negative with and without the bias
        x, w, bias = x.abs() + 0.1, -0.25 * w.abs(), torch.full((64,), -8.0, dtype=torch.float64)
    t = F.conv2d(x, w, bias, 2, 3)
    assert t.shape[2:] == ((H - 1) // 2 + 1, (W - 1) // 2 + 1) and (not negative or t.max().item() < -8)
    fn = {0: lambda v: v, 1: F.relu, 3: lambda v: F.leaky_relu(v, 0.01)}[act]
    ref = F.max_pool2d(fn(t), 3, 2, 1).permute(0, 2, 3, 1)
    amag = F.max_pool2d(F.conv2d(x.abs(), w.abs(), bias.abs(), 2, 3), 3, 2, 1).permute(0, 2, 3, 1)
    if negative and act != 1:
        assert ref.max().item() < 0                                                          # ... and nothing here is one
    x4 = torch.cat([x.permute(0, 2, 3, 1), torch.zeros(B, H, W, 1, dtype=torch.float64)], -1)
    w4 = torch.zeros(128, 208, dtype=torch.float64)
    w4[:64, :196] = torch.cat([w.permute(0, 2, 3, 1), torch.zeros(64, 7, 7, 1, dtype=torch.float64)], -1).reshape(64, 196)
    wpl = torch.zeros(64, 3, 52, dtype=torch.float64)
    wpl[:, :, :49] = w.reshape(64, 3, 49)
    wpl = torch.cat([wpl.reshape(64, 156), torch.zeros(64, 4, dtype=torch.float64)], 1)
    for got, mag in (R.stem_pool_ref(x4, w4, bias, B, H, W, act), R.stem_pool_ref(x, wpl, bias, B, H, W, act, planar=True)):
        assert got.shape == ref.shape == mag.shape and got.dtype == torch.float64
        assert (got - ref).abs().max().item() < F64 and (mag - amag).abs().max().item() < F64
        assert torch.all(mag >= got.abs() * (1 - 1e-12))
    with R.precision(torch.float32):
        g32, _ = R.stem_pool_ref(x4, w4, bias, B, H, W, act)
    assert g32.dtype == torch.float32 and (g32.double() - ref).abs().max().item() < 1e-4


# ---- mano_head_ref ----------------------------------------------------------------------------------------------------------
def _mano_assets():
    import fake_mano
    import hands_amd
    import mano_cases as MC
    return [hands_amd.synthetic_mano_asset(True), hands_amd.synthetic_mano_asset(False), fake_mano.realistic_mano_asset(True),
            MC.dense_weight_asset(False)]


@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_mano_head_ref_is_the_oracle_at_the_oracles_parameters(which):
    """Default tips, K = diag(f, f, 1) with a principal point, min_s = 0.1: the oracle's numbers exactly in float64, and the
    oracle's bits at the float32 switch (the same ATen calls in the same order)."""
    import mano_cases as MC
    asset = _mano_assets()[which]
    rot, aa, betas, cam, _ = MC.inputs(7, 40 + which, sigma=1.0 + which)
    cam[2, 0] = -0.5                                                       # the clamp
    g = torch.Generator().manual_seed(which)
    K = torch.tensor([[1000.0, 0, 112], [0, 1000.0, 112], [0, 0, 1]])[None].repeat(7, 1, 1)
    K[:, 0, 0] += 20 * torch.randn(7, generator=g)
    keys = ("vertices", "joints3d", "v3d.cam", "j3d.cam", "j2d.norm", "cam_t")
    want64 = O.mano_head(rot.double(), betas.double(), cam.double(), K.double(), asset, 224, "")
    got64 = R.mano_head_ref(rot, betas, cam, K, asset, 224, 0.1)
    for k in keys:
        assert got64[k].dtype == torch.float64 and torch.equal(got64[k], want64[k]), k
    want32 = O.mano_head(rot, betas, cam, K, asset, 224, "")
    with R.precision(torch.float32):
        got32 = R.mano_head_ref(rot, betas, cam, K, asset, 224, 0.1)
    for k in keys:
        assert got32[k].dtype == torch.float32 and torch.equal(got32[k], want32[k]), k
    v64, j64 = O.mano_lbs(betas, aa[:, :3], aa[:, 3:], asset, dtype=torch.float64)
    via_aa = R.mano_head_ref(aa, betas, cam, K, asset, 224, 0.1, aa_input=True)
    assert torch.equal(via_aa["vertices"], v64) and torch.equal(via_aa["joints3d"], j64)
    # the intermediates: joints16 are the first 16 joints; A applied through the weights gives the vertices back
    assert torch.equal(got64["joints16"], got64["joints3d"][:, :16]) and got64["A"].shape == (7, 16, 12)
    assert got64["blend_row"].shape == (7, 145) and torch.equal(got64["blend_row"][:, :10], betas.double())
    vp = torch.from_numpy(asset.v_template).double() + torch.cat([got64["blend_row"][:, :10] @ torch.from_numpy(
        asset.shapedirs).double().reshape(-1, 10).t()], 1).view(7, 778, 3) + (got64["blend_row"][:, 10:] @ torch.from_numpy(
            asset.posedirs).double()).view(7, 778, 3)
    Tv = torch.einsum("vj,bje->bve", torch.from_numpy(asset.lbs_weights).double(), got64["A"]).view(7, 778, 3, 4)
    again = torch.einsum("bvij,bvj->bvi", Tv[..., :3], vp) + Tv[..., 3]
    assert (again - got64["vertices"]).abs().max().item() < F64


@pytest.mark.parametrize("which,min_s,img_res", [(0, 0.25, 256.0), (2, 0.1, 192.5), (3, 0.25, 224.0)])
def test_mano_head_ref_general_K_and_tips_against_per_vertex_loops(which, min_s, img_res):
    """The parameters tests/test_gpu_mano_edges.py frees -- a general K, tips at chunk edges, min_s -- against the loop-written
    evaluation of mano_cases.mano_head_loops: vertices[tips], K @ X, the division by row 2, element by element."""
    import mano_cases as MC
    asset = _mano_assets()[which]
    rot, aa, betas, cam, K = MC.inputs(5, 50 + which, sigma=3.0)
    cam[0, 0], cam[1, 0], cam[4, 0] = min_s, -0.5, 3.0
    got = R.mano_head_ref(aa, betas, cam, K, asset, img_res, min_s, tip_ids=MC.EDGE_TIPS, aa_input=True)
    want = MC.mano_head_loops(aa, betas, cam, K, asset, img_res, min_s, MC.EDGE_TIPS)
    assert got["hz"].min().item() > 1.0 and (K[:, 2, :2].abs() > 5e-4).all() and (K[:, 0, 1] != K[:, 1, 0]).all()
    for k, tol in (("vertices", 1e-13), ("joints3d", 1e-13), ("j3d.cam", 1e-12), ("cam_t", 1e-12), ("j2d.norm", 1e-11)):
        err = (got[k] - want[k]).abs().max().item()
        assert err < tol, (k, err)
    assert torch.equal(got["joints3d"][:, 16:], got["vertices"][:, list(MC.EDGE_TIPS)])
    # matrix input: the loops on the axis-angle rows the reference's conversion makes of the matrices (a quaternion that is not
    # standardised: an angle above pi where a vector component outweighs w, so NOT the rows the matrices were made from)
    via_rot = R.mano_head_ref(rot, betas, cam, K, asset, img_res, min_s, tip_ids=MC.EDGE_TIPS)
    aa2 = O.matrix_to_axis_angle(rot.double().reshape(-1, 3, 3)).reshape(5, 48)
    want2 = MC.mano_head_loops(aa2, betas, cam, K, asset, img_res, min_s, MC.EDGE_TIPS)
    assert (via_rot["vertices"] - want2["vertices"]).abs().max().item() < 1e-13
    assert (via_rot["j2d.norm"] - want2["j2d.norm"]).abs().max().item() < 1e-11
    # a projection that ignored the last row, or the skew, would be far off
    naive = (got["j3d.cam"][..., :2] * torch.stack([K[:, 0, 0], K[:, 1, 1]], -1).double()[:, None] / got["j3d.cam"][..., 2:]
             + K[:, :2, 2].double()[:, None])
    assert (2 * naive / img_res - 1 - got["j2d.norm"]).abs().max().item() > 1e-3
