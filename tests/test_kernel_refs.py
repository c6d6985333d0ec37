"""tests/kernel_refs.py against the ATen operators and oracle functions it restates, on the CPU, at ragged shapes of
tests/test_gpu_kernel_edges.py: a restatement that is wrong at an odd size would hide a kernel bug there, or invent one."""
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
from oracle import hamer_oracle as H
from oracle import handoccnet_oracle as HO
from oracle import hands_oracle as O

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
