"""Edge shapes of the non-convolution kernels (csrc/handocc.hip, csrc/transformer.hip, csrc/vit_b.hip, csrc/elementwise.hip: its
layout and pool kernels first, its glue kernels at the end) through the C ABI, every output element against the float64 restatements of tests/kernel_refs.py.

The model-shape tests of these kernels (test_gpu_handoccnet.py, test_gpu_hamer.py, test_gpu_vit_backbone.py, test_gpu_parity.py)
stay below every launch cap and on every tile boundary.  The cases here are the smallest that reach what those leave out: a
second, partial grid-stride pass (hands_grid_1d caps a launch at 2048 blocks x 256 threads = 524 288 items, 4096 blocks for the
3x3 max-pool, 2048 x 64 threads for the sum / average pool), the smallest legal size, sizes that are no multiple of a tile or a
wave, both instantiations of the flash attention, and softmax arguments far outside randn.

Every output lives inside a larger buffer: NaN where the kernel has to write, a sentinel band before and after and in every padded
row or column it must leave alone.  Bounds: a kernel that only moves, adds or takes a maximum is bit-equal to the float32 torch
expression; on inputs of the scale of a kernel's model-shape test that test's bound holds unchanged (the reductions here are no
longer); on inputs of another scale (wide logits, 1000 + randn rows, softmax arguments of +-60) the bound is
max(that bound, 4 x the error of ATen's float32 evaluation of the same restatement): 4 for a different summation order of the same
length and the ~1 ulp exp_nonpos.  Each comparison prints `EDGE|kernel|case|error|bound` before it asserts."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R
from edge_util import BAND, DEV, EINVAL, SENT, Out, _close, _dev, _exact, _gen, _rule
from hands_amd import _lib
from hands_amd._lib import check, ptr
from oracle import hands_oracle as O

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- streaming kernels: one case past the grid cap by a partial pass, one at the smallest legal size -------------------------------
@pytest.mark.parametrize("B,N,C", [(7, 1001, 300), (1, 1, 4)])
def test_add_embed2_and_add_rowvec(B, N, C):
    L = _lib.lib()
    g = _gen(1, B, N, C)
    q, k = torch.randn(B, N, C, generator=g), torch.randn(B, N, C, generator=g)
    qe, ke, kp = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g), torch.randn(B, C, generator=g)
    d = _dev(q, k, qe, ke, kp)
    oq, ok = Out(B, N, C), Out(B, N, C)
    check(L.hands_add_embed2_f32(*[ptr(t) for t in d], oq.ptr(), ok.ptr(), B, N, C, _stream()), "add_embed2")
    rq, rk = R.add_embed2(q, k, qe, ke, kp, B, N, C)
    _exact("add_embed2", f"q {B}x{N}x{C}", oq.get(), (q + qe) + kp[:, None], rq)
    _exact("add_embed2", f"k {B}x{N}x{C}", ok.get(), (k + ke) + kp[:, None], rk)
    o = Out(B, N, C)
    check(L.hands_add_rowvec_f32(ptr(d[0]), ptr(d[4]), o.ptr(), B, N, C, _stream()), "add_rowvec")
    _exact("add_rowvec", f"{B}x{N}x{C}", o.get(), q + kp[:, None], R.add_rowvec(q, kp, B, N, C))


@pytest.mark.parametrize("with_vec", [True, False])
@pytest.mark.parametrize("B,T,C", [(7, 1001, 300), (1, 1, 4)])
def test_add_pos(B, T, C, with_vec):
    L = _lib.lib()
    g = _gen(2, B, T, C)
    x, pos, vec = torch.randn(B, T, C, generator=g), torch.randn(T + 1, C, generator=g), torch.randn(B, C, generator=g)
    xo = Out(B, T, C, init=x)
    dp, dv = _dev(pos, vec)
    check(L.hands_add_pos_f32(xo.ptr(), ptr(dp), ptr(dv) if with_vec else None, B, T, C, _stream()), "add_pos")
    e32 = (x + pos[None, 1:]) + pos[None, :1]
    if with_vec:
        e32 = e32 + vec[:, None]
    _exact("add_pos", f"{B}x{T}x{C} vec={with_vec}", xo.get(), e32, R.add_pos(x, pos, vec if with_vec else None, B, T, C))


@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("npix,C", [(7007, 300), (1, 4)])
def test_gate_apply(npix, C, stride):
    L = _lib.lib()
    g = _gen(3, npix, C, stride)
    x, logit = torch.randn(npix, C, generator=g), torch.randn(npix * stride, generator=g)
    dx, dl = _dev(x, logit)
    pr, se = Out(npix, C), Out(npix, C)
    check(L.hands_gate_apply_f32(ptr(dx), ptr(dl), stride, pr.ptr(), se.ptr(), npix, C, _stream()), "gate_apply")
    rp, rs = R.gate_apply(x, logit, stride, npix, C)
    _close("gate_apply", f"primary {npix}x{C} stride {stride}", pr.get(), rp, 1e-6)
    _close("gate_apply", f"secondary {npix}x{C} stride {stride}", se.get(), rs, 1e-6)


@pytest.mark.parametrize("npix,C", [(7007, 300), (1, 4)])
def test_bn_leaky_both_signs_and_exact_zeros(npix, C):
    L = _lib.lib()
    g = _gen(4, npix, C)
    x = torch.randn(npix, C, generator=g)
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    sh[::4] = 0.0
    x[::3, ::4] = 0.0                         # x * scale + 0 == 0 exactly: neither branch may turn it into anything else
    x[0, 0] = 0.0
    dx, ds, dh = _dev(x, sc, sh)
    o = Out(npix, C)
    check(L.hands_bn_leaky_f32(ptr(dx), ptr(ds), ptr(dh), o.ptr(), npix, C, _stream()), "bn_leaky")
    got, ref = o.get(), R.bn_leaky(x, sc, sh, npix, C)
    assert (ref == 0).any() and (npix == 1 or ((ref > 0).any() and (ref < 0).any()))
    _close("bn_leaky", f"{npix}x{C}", got, ref, 1e-6)
    assert torch.all(got[ref == 0] == 0)


@pytest.mark.parametrize("B,T,C", [(7, 1001, 300), (1, 2, 4)])
def test_vit_tokens(B, T, C):
    L = _lib.lib()
    g = _gen(5, B, T, C)
    patch, cls, pos = torch.randn(B, T - 1, C, generator=g), torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    d = _dev(patch, cls, pos)
    o = Out(B, T, C)
    check(L.hands_vit_tokens_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), o.ptr(), B, T, C, _stream()), "vit_tokens")
    e32 = torch.cat([cls.view(1, 1, C).expand(B, -1, -1), patch], 1) + pos
    _exact("vit_tokens", f"{B}x{T}x{C}", o.get(), e32, R.vit_tokens(patch, cls, pos, B, T, C))


@pytest.mark.parametrize("B,h,w,H,W,C", [(3, 37, 41, 74, 82, 116), (2, 5, 3, 7, 8, 8), (2, 8, 8, 5, 3, 4), (1, 1, 1, 4, 4, 4),
                                         (2, 6, 6, 6, 6, 8)])
def test_upsample_bilinear_add(B, h, w, H, W, C):
    """Past the cap at an exact 2x ratio (527 916 float4), then ratios that are not: up by 7/5 and 8/3, DOWN by 5/8 and 3/8, from a
    single pixel, and the identity."""
    L = _lib.lib()
    g = _gen(6, B, h, w, H, W, C)
    x, y = torch.randn(B, h, w, C, generator=g), torch.randn(B, H, W, C, generator=g)
    dx, dy = _dev(x, y)
    o = Out(B, H, W, C)
    check(L.hands_upsample_bilinear_add_f32(ptr(dx), ptr(dy), o.ptr(), B, h, w, H, W, C, _stream()), "upsample_bilinear_add")
    _close("upsample_bilinear_add", f"{B}x{h}x{w}->{H}x{W}x{C}", o.get(), R.upsample_bilinear_add(x, y, B, h, w, H, W, C), 2e-6)


@pytest.mark.parametrize("B,h,w,C", [(3, 37, 41, 116), (1, 1, 3, 4)])
def test_upsample_nearest2x_add(B, h, w, C):
    L = _lib.lib()
    g = _gen(7, B, h, w, C)
    low, up1 = torch.randn(B, h, w, C, generator=g), torch.randn(B, 2 * h, 2 * w, C, generator=g)
    dl, du = _dev(low, up1)
    o = Out(B, 2 * h, 2 * w, C)
    check(L.hands_upsample_nearest2x_add_f32(ptr(dl), ptr(du), o.ptr(), B, h, w, C, _stream()), "upsample_nearest2x_add")
    e32 = up1 + F.interpolate(low.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1)
    _exact("upsample_nearest2x_add", f"{B}x{h}x{w}x{C}", o.get(), e32.contiguous(), R.upsample_nearest2x_add(low, up1, B, h, w, C))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("B,H,W,C", [(3, 148, 164, 116), (3, 74, 82, 116), (1, 2, 2, 4), (2, 6, 14, 8)])
def test_pool2x2(B, H, W, C, mode):
    """(3,148,164,116) has 527 916 OUTPUT float4, past the cap; the others are non-square maps under it and the smallest map."""
    L = _lib.lib()
    g = _gen(8, B, H, W, C)
    x = torch.randn(B, H, W, C, generator=g)
    dx, = _dev(x)
    o = Out(B, H // 2, W // 2, C)
    check(L.hands_pool2x2_nhwc_f32(ptr(dx), o.ptr(), B, H, W, C, mode, _stream()), "pool2x2")
    got, ref = o.get(), R.pool2x2_nhwc(x, B, H, W, C, mode)
    if mode == 0:
        _close("pool2x2 avg", f"{B}x{H}x{W}x{C}", got, ref, 1e-6)
    else:
        _exact("pool2x2 max", f"{B}x{H}x{W}x{C}", got, F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous(), ref)


@pytest.mark.parametrize("B,H,W,C", [(3, 113, 113, 432), (1, 1, 1, 4), (2, 2, 5, 8), (2, 17, 14, 64)])
def test_maxpool3x3s2(B, H, W, C):
    """(3,113,113,432): 1 052 676 output float4 against this kernel's cap of 4096 x 256 = 1 048 576."""
    L = _lib.lib()
    g = _gen(9, B, H, W, C)
    x = torch.randn(B, H, W, C, generator=g)
    dx, = _dev(x)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    o = Out(B, Ho, Wo, C)
    check(L.hands_maxpool3x3s2_nhwc_f32(ptr(dx), o.ptr(), B, H, W, C, _stream()), "maxpool3x3s2")
    e32 = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    got = o.get()
    assert not torch.isnan(got).any() and torch.equal(got, e32)
    assert torch.equal(got.double(), R.maxpool3x3s2_nhwc(x, B, H, W, C))
    print(f"EDGE|maxpool3x3s2|{B}x{H}x{W}x{C}|0.000e+00|0.000e+00")


@pytest.mark.parametrize("B,H,W", [(5, 331, 317), (1, 1, 1)])
def test_nchw3_to_nhwc4(B, H, W):
    L = _lib.lib()
    x = torch.randn(B, 3, H, W, generator=_gen(10, B, H, W))
    dx, = _dev(x)
    o = Out(B, H, W, 4)
    check(L.hands_nchw3_to_nhwc4_f32(ptr(dx), o.ptr(), B, H, W, _stream()), "nchw3_to_nhwc4")
    got = o.get()
    assert not torch.isnan(got).any() and torch.equal(got.double(), R.nchw3_to_nhwc4(x, B, H, W))
    assert torch.all(got[..., 3] == 0)
    print(f"EDGE|nchw3_to_nhwc4|{B}x{H}x{W}|0.000e+00|0.000e+00")


@pytest.mark.parametrize("B,HW,C,stride", [(65, 2, 8192, 8192), (3, 1, 8, 12), (2, 49, 2048, 2304)])
def test_sumpool_and_avgpool(B, HW, C, stride):
    """(65,2,8192): 133 120 threads' worth against the 2048 x 64 = 131 072 cap, stepped in `int`.  The sum's bound is the one of its
    7x7 test (1e-5); the mean is that sum divided once: 1e-5 / HW + one rounding of a value below 8 (4.8e-7) is under the pools'
    1e-6 for every HW here."""
    L = _lib.lib()
    x = torch.randn(B, HW, C, generator=_gen(11, B, HW, C))
    dx, = _dev(x)
    gap = (torch.arange(stride) >= C).view(1, stride)
    for name, fn, ref, bound in (("sumpool", L.hands_sumpool_nhwc_f32, R.sumpool_nhwc(x, B, HW, C, stride), 1e-5),
                                 ("avgpool", L.hands_avgpool_nhwc_f32, R.avgpool_nhwc(x, B, HW, C, stride), 1e-6)):
        o = Out(B, stride, keep=gap)
        check(fn(ptr(dx), o.ptr(), B, HW, C, stride, _stream()), name)
        _close(name, f"{B}x{HW}x{C} stride {stride}", o.get()[:, :C].contiguous(), ref, bound)


@pytest.mark.parametrize("B,ld,n_freq,amp", [(6600, 80, 4, 0.5), (3, 84, 4, 0.5), (1, 20, 1, 0.5), (5, 320, 16, 1e-3)])
def test_kpe_encode(B, ld, n_freq, amp):
    """B=6600 x ld=80 is 528 000 elements (`int` stepping).  amp 0.5: 0.5 * randn angles, as the model-shape test; n_freq = 16 with
    |angle| <= 1e-3 keeps 2^15 * angle within 33 rad."""
    L = _lib.lib()
    g = _gen(12, B, ld, n_freq)
    if amp == 0.5:
        ce, co = 0.5 * torch.randn(B, 2, generator=g), 0.5 * torch.randn(B, 8, generator=g)
    else:
        ce, co = amp * (2 * torch.rand(B, 2, generator=g) - 1), amp * (2 * torch.rand(B, 8, generator=g) - 1)
    dce, dco = _dev(ce, co)
    o = Out(B, ld)
    check(L.hands_kpe_encode_f32(ptr(dce), ptr(dco), o.ptr(), B, ld, n_freq, _stream()), "kpe_encode")
    got = o.get()
    _close("kpe_encode", f"{B}x{ld} n_freq {n_freq}", got, R.kpe_encode(ce, co, B, ld, n_freq), 1e-6)
    assert torch.all(got[:, 20 * n_freq:] == 0)


def _well_conditioned_6d(n, g):
    """n rows [a1 | a2] with |a1|, |a2| in [0.5, 2.8] and at least 45 degrees between them: Gram-Schmidt on randn pairs is as badly
    conditioned as the closest-to-parallel pair among them, and half a million pairs hold one within 0.002 rad; the bound of the
    96-pair model-shape test belongs to pairs like its own."""
    a1 = F.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    orth = F.normalize(v - (v * a1).sum(-1, keepdim=True) * a1, dim=-1)
    c = 2 * torch.rand(n, 1, generator=g, dtype=torch.float64) - 1
    s1, s2 = (0.5 + 1.5 * torch.rand(n, 1, generator=g, dtype=torch.float64) for _ in range(2))
    return torch.cat([s1 * a1, s2 * (orth + c * a1)], -1).float()


@pytest.mark.parametrize("B,ld6", [(32800, 96), (3, 112)])
def test_rot6d_to_matrix_cols(B, ld6):
    """B=32800: 524 800 joints (`int` stepping).  ld6=112: the 16 floats behind the 96 are NaN and never read.  Two degenerate
    joints whose result is exact in any precision: a2 parallel to a1 on an axis (b2 = (a2 - d b1) / max(0, 1e-12) = 0) and all zeros."""
    L = _lib.lib()
    g = _gen(13, B, ld6)
    d6 = torch.full((B, ld6), float("nan"))
    d6[:, :96] = _well_conditioned_6d(B * 16, g).view(B, 96)
    d6[B - 1, 6:12] = torch.tensor([0.0, 3.0, 0.0, 0.0, -5.0, 0.0])
    d6[B - 1, 90:96] = 0.0
    dd, = _dev(d6)
    o = Out(B, 16, 3, 3)
    check(L.hands_rot6d_to_matrix_cols_f32(ptr(dd), ld6, o.ptr(), B, _stream()), "rot6d_to_matrix_cols")
    got = o.get()
    assert torch.isfinite(got).all()
    _close("rot6d_to_matrix_cols", f"{B} ld6 {ld6}", got, R.rot6d_to_matrix_cols(d6, ld6, B), 5e-6)
    assert torch.equal(got[B - 1, 1], torch.tensor([[0.0, 0, 0], [1.0, 0, 0], [0, 0, 0]])) and torch.all(got[B - 1, 15] == 0)


@pytest.mark.parametrize("B,Hin,Win,S,col0,Wc", [(3, 64, 48, 512, 7, 343), (2, 224, 224, 256, 32, 192), (2, 100, 180, 64, 0, 64),
                                                 (1, 300, 200, 96, 10, 70), (2, 64, 64, 64, 0, 64), (1, 1, 1, 8, 2, 3)])
def test_resize_crop(B, Hin, Win, S, col0, Wc):
    """(3,64,48,512,7,343): 526 848 output pixels, past the cap, an 8x / 10.7x enlargement with an off-centre crop; then the model's
    shape, a non-square reduction, a reduction with an off-centre crop, the identity, and a single source pixel.  (1,300,200,96,10,70)
    found the float32 source coordinate: 5.9e-05 there before lerp_tap (csrc/common.h), 3.7e-07 with it."""
    L = _lib.lib()
    x = torch.randn(B, 3, Hin, Win, generator=_gen(14, B, Hin, Win, S))
    dx, = _dev(x)
    o = Out(B, S, Wc, 4)
    check(L.hands_resize_crop_nchw3_to_nhwc4_f32(ptr(dx), o.ptr(), B, Hin, Win, S, col0, Wc, _stream()), "resize_crop")
    got = o.get()
    _close("resize_crop", f"{B}x{Hin}x{Win}->{S} cols {col0}+{Wc}", got, R.resize_crop_nchw3_to_nhwc4(x, B, Hin, Win, S, col0, Wc), 2e-6)
    assert torch.all(got[..., 3] == 0)


# ---- reduction kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,C", [(1, 1, 64), (2, 15, 64), (3, 17, 128), (2, 1000, 256)])
def test_token_sum(B, N, C):
    """Fewer tokens than the 16 token groups, one more than 16, and a count that is no multiple of 16.  randn tokens are 20 x the
    model-shape test's 0.05 * randn: max(1e-4, 4 x ATen's float32 sum)."""
    L = _lib.lib()
    x = torch.randn(B, N, C, generator=_gen(15, B, N, C))
    dx, = _dev(x)
    o = Out(B, C)
    check(L.hands_token_sum_f32(ptr(dx), o.ptr(), B, N, C, _stream()), "token_sum")
    ref = R.token_sum(x, B, N, C)
    bound, e32 = _rule(1e-4, ref, R.token_sum, x, B, N, C)
    print(f"EDGE-F32|token_sum|{B}x{N}x{C}|{e32:.3e}")
    _close("token_sum", f"{B}x{N}x{C}", o.get(), ref, bound)


@pytest.mark.parametrize("npix", [1, 5, 2049])
def test_channel_pool(npix):
    """npix % 4 != 0: the last workgroup's waves without a pixel leave.  Pixel 0 holds 256 equal values (max = mean = the value,
    exactly: 256 x 0.375 is exact), the last pixel has its maximum in channel 255."""
    L = _lib.lib()
    x = torch.randn(npix, 256, generator=_gen(16, npix))
    x[npix - 1, 255] = 9.0
    x[0] = 0.375
    dx, = _dev(x)
    o = Out(npix, 4)
    check(L.hands_channel_pool_f32(ptr(dx), o.ptr(), npix, 256, _stream()), "channel_pool")
    got, ref = o.get(), R.channel_pool(x, npix, 256)
    assert torch.equal(got[:, 0].double(), ref[:, 0]) and torch.all(got[:, 2:] == 0)
    assert got[0, 0] == 0.375 and got[0, 1] == 0.375 and (npix == 1 or got[npix - 1, 0] == 9.0)
    _close("channel_pool", f"{npix}", got, ref, 1e-6)


def _softmax_inputs(B, N, J, ld_in, g, reach):
    lat = torch.full((B, N, ld_in), float("nan"))               # columns J..ld_in-1 are never read
    betas = 1 + 0.2 * torch.randn(J, generator=g)
    z = torch.randn(B, N, J, generator=g)
    z = z * (reach / (z * betas).abs().max().item())
    if J > 1 and N > 1:
        z[:, :, 0] = 0.37                                        # equal logits: uniform
        z[:, :, 1] = -0.5 * reach / betas[1].item()              # one dominant position: `reach` above all the others
        z[:, N // 3, 1] = 0.5 * reach / betas[1].item()
    lat[:, :, :J] = z
    return lat, betas


@pytest.mark.parametrize("reach", [12.0, 60.0])
@pytest.mark.parametrize("B,N,J,ld_in,ld_out", [(1, 1, 1, 1, 1), (2, 100, 21, 24, 32), (2, 257, 21, 21, 21), (1, 1024, 21, 24, 32)])
def test_spatial_softmax(B, N, J, ld_in, ld_out, reach):
    """A single position (most threads hold nothing), N < 256, one element past 256, the model's 1024.  reach = max |latent * beta|:
    12 is what the model-shape test's 3 * randn gives (its bound), 60 is beyond what anything has measured (the float32 rule)."""
    L = _lib.lib()
    lat, betas = _softmax_inputs(B, N, J, ld_in, _gen(17, B, N, J, reach), reach)
    dl, db = _dev(lat, betas)
    o = Out(B, N, ld_out)
    check(L.hands_spatial_softmax_f32(ptr(dl), ld_in, ptr(db), o.ptr(), ld_out, B, N, J, _stream()), "spatial_softmax")
    got, ref = o.get(), R.spatial_softmax(lat, ld_in, betas, ld_out, B, N, J)
    bound = 5e-6 * ref.max().item() + 1e-7
    if reach > 12.0:
        clean = torch.nan_to_num(lat)
        bound, e32 = _rule(bound, ref, R.spatial_softmax, clean, ld_in, betas, ld_out, B, N, J)
        print(f"EDGE-F32|spatial_softmax|{B}x{N}x{J} reach {reach}|{e32:.3e}")
    _close("spatial_softmax", f"{B}x{N}x{J} ld {ld_in}/{ld_out} reach {reach}", got, ref, bound)
    assert torch.all(got[:, :, J:] == 0)
    if J > 1 and N > 1:
        assert (got[:, :, 0] - 1.0 / N).abs().max().item() <= 2.0 ** -23 / N and got[:, N // 3, 1].min().item() > 0.99


@pytest.mark.parametrize("M", [1, 4, 5, 37])
@pytest.mark.parametrize("C", [256, 768, 1024, 1280])
def test_layernorm(C, M):
    """Every instantiation x a single row, one full workgroup of four rows, one row past it, the model's 37.  Rows of the
    model-shape test's scale (3 * randn + 0.5) at its bound, rows of 1000 + randn at the float32 rule, constant rows (variance 0:
    the output is beta, plus the added vector, exactly); eps 1e-5 and 1e-6; the added vector per row, per 4 rows and one for all."""
    L = _lib.lib()
    g = _gen(18, C, M)
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    vec = torch.randn(M, C, generator=g)
    rows = {"randn": 3 * torch.randn(M, C, generator=g) + 0.5, "offset": 1000 + torch.randn(M, C, generator=g),
            "const": (0.25 * torch.arange(1, M + 1, dtype=torch.float32)).view(M, 1).expand(M, C).contiguous()}
    dg, db, dv = _dev(gam, bet, vec)
    for kind, x in rows.items():
        dx, = _dev(x)
        for eps in (1e-5, 1e-6):
            for rpv in (None, 1, 4, M):
                o = Out(M, C)
                check(L.hands_layernorm_f32(ptr(dx), ptr(dg), ptr(db), o.ptr(), ptr(dv) if rpv else None, rpv or 1, M, C, eps, _stream()),
                      "layernorm")
                args = (x, gam, bet, vec if rpv else None, rpv or 1, M, C, eps)
                got, ref = o.get(), R.layernorm(*args)
                case = f"{kind} {M}x{C} eps {eps} rows_per_vec {rpv}"
                if kind == "const":
                    e32 = bet.expand(M, C) + vec[torch.arange(M) // rpv] if rpv else bet.expand(M, C)
                    assert torch.equal(got, e32.contiguous()), case
                bound = 2e-5
                if kind == "offset":
                    bound, e32 = _rule(2e-5, ref, R.layernorm, *args)
                    print(f"EDGE-F32|layernorm|{case}|{e32:.3e}")
                _close("layernorm", case, got, ref, bound)


@pytest.mark.parametrize("B,G", [(1, 2), (3, 14), (2, 6)])
def test_vit_tail(B, G):
    """One output pixel, the model's 14 x 14 grid, and 6 x 6: three windows per row, an odd number.  The class token is NaN: never
    read.  At (1,2) also the bit-equality with hands_layernorm_f32 followed by the window average in float32."""
    L = _lib.lib()
    C, eps = 768, 1e-6
    g = _gen(19, B, G)
    x = 3 * torch.randn(B, 1 + G * G, C, generator=g) + 0.5
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = R.vit_tail(x, gam, bet, B, G, C, eps)
    x[:, 0] = float("nan")
    dx, dg, db = _dev(x, gam, bet)
    o = Out(B, G // 2, G // 2, C)
    check(L.hands_vit_tail_f32(ptr(dx), ptr(dg), ptr(db), o.ptr(), B, G, C, eps, _stream()), "vit_tail")
    got = o.get()
    _close("vit_tail", f"{B} grid {G}", got, ref, 2e-5)
    if (B, G) == (1, 2):
        ln = Out(5, C)
        check(L.hands_layernorm_f32(ptr(dx), ptr(dg), ptr(db), ln.ptr(), None, 1, 5, C, eps, _stream()), "layernorm")
        r = ln.get()[1:]
        assert torch.equal(got.view(C), ((r[0] + r[1]) + (r[2] + r[3])) * 0.25)


# ---- attention kernels ---------------------------------------------------------------------------------------------------------------
def _flash_inputs(kind, B, N, heads, g):
    C, D = heads * 64, 64
    q, k, v, q2, k2, res = (torch.randn(B, N, C, generator=g) for _ in range(6))
    k2 = 0.05 * k2
    if kind == "randn":                      # the model-shape test's inputs
        q, k = 2.0 * q, 1.5 * k
    elif kind == "wide":                     # logits reach about +-70: near one-hot rows, large running-max jumps between tiles
        q, k = 4.0 * q, 4.0 * k
    elif kind == "planted":                  # two keys that dominate every row: one in the first key tile, a larger one in the last
        u = F.normalize(torch.randn(heads, D, generator=g), dim=-1).view(1, 1, C)
        q = q + 8.0 * u
        k[:, 17:18] = 40.0 * u
        k[:, N - 6:N - 5] = 40.8 * u
    return q, k, v, q2, k2, res


def _run_flash(B, N, heads, scale, kind):
    L = _lib.lib()
    C, D = heads * 64, 64
    q, k, v, q2, k2, res = _flash_inputs(kind, B, N, heads, _gen(20, B, N, heads, kind == "wide", kind == "planted"))
    d = _dev(q, k, v, q2, k2, res)
    ks = Out(B, C)
    check(L.hands_token_sum_f32(ptr(d[4]), ks.ptr(), B, N, C, _stream()), "token_sum")
    k2sum = ks.get()
    _close("token_sum", f"k2 {B}x{N}x{C}", k2sum, R.token_sum(k2, B, N, C), 1e-4)
    for name, gate, resid in (("plain", False, False), ("gate", True, False), ("residual", False, True), ("gate+residual", True, True)):
        o = Out(B, N, C)
        check(L.hands_flash_attention_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]) if gate else None, ks.ptr() if gate else None,
                                          ptr(d[5]) if resid else None, o.ptr(), B, N, heads, D, scale, _stream()), "flash_attention")
        args = (q, k, v, q2 if gate else None, k2sum if gate else None, res if resid else None, B, N, heads, D, scale)
        ref = R.flash_attention(*args)
        bound = 2e-5
        if kind != "randn":
            bound, e32 = _rule(2e-5, ref, R.flash_attention, *args)
            print(f"EDGE-F32|flash_attention|{kind} {name} {B}x{N}x{heads} scale {scale}|{e32:.3e}")
        _close("flash_attention", f"{kind} {name} {B}x{N}x{heads} scale {scale}", o.get(), ref, bound)


@pytest.mark.parametrize("scale", [0.125, 0.1])
@pytest.mark.parametrize("B,N,heads", [(1, 128, 1), (1, 384, 3), (3, 256, 5), (2, 1024, 4)])
def test_flash_attention(B, N, heads, scale):
    """1, 9, 30 and 64 workgroups (remainders 1, 1, 6, 0 of the 8-way XCD deal), 1, 3, 2 and 8 key tiles; scale 0.125 is folded into
    q, 0.1 is applied to the scores (the other instantiation); plain, gate only, residual only, gate + residual."""
    _run_flash(B, N, heads, scale, "randn")


@pytest.mark.parametrize("scale", [0.125, 0.1])
@pytest.mark.parametrize("kind", ["wide", "planted"])
def test_flash_attention_wide_logits(kind, scale):
    _run_flash(1, 384, 3, scale, kind)


def _attention_inputs(kind, B, T, heads, D, g):
    C = heads * D
    qkv = torch.randn(B, T, 3, C, generator=g)
    if kind == "wide":
        qkv[:, :, :2] *= 4.0
    elif kind == "uniform":                  # crop 0: every key equal -> every row of the softmax uniform, the output mean_t v
        qkv[0, :, 1] = qkv[0, 0, 1].clone()
    elif kind == "dominant":                 # two keys that dominate every row: token 0 and, larger, the last real token
        u = F.normalize(torch.randn(heads, D, generator=g), dim=-1).view(1, 1, C)
        qkv[:, :, 0] += 6.0 * u
        qkv[:, 0:1, 1] = (10.0 * D ** 0.5) * u
        qkv[:, T - 1:T, 1] = (10.2 * D ** 0.5) * u
    return qkv.view(B, T, 3 * C)


@pytest.mark.parametrize("kind", ["randn", "wide", "uniform", "dominant"])
@pytest.mark.parametrize("B,heads", [(1, 1), (2, 3)])
@pytest.mark.parametrize("T,D", [(192, 80), (197, 64)])
def test_attention(T, D, B, heads, kind):
    """Both instantiations at one workgroup and at six.  For 197 tokens the rows behind the last crop are the sentinel band: the
    padded queries 197..207 of the last wave store nothing."""
    L = _lib.lib()
    C, scale = heads * D, float(D ** -0.5)
    qkv = _attention_inputs(kind, B, T, heads, D, _gen(21, T, B, heads, len(kind)))
    dq, = _dev(qkv)
    o = Out(B, T, C)
    check(L.hands_attention_f32(ptr(dq), o.ptr(), B, T, heads, D, scale, _stream()), "attention")
    got, ref = o.get(), R.attention(qkv, B, T, heads, D, scale)
    bound = 5e-6
    if kind != "randn":
        bound, e32 = _rule(5e-6, ref, R.attention, qkv, B, T, heads, D, scale)
        print(f"EDGE-F32|attention{T}|{kind} {B}x{heads}|{e32:.3e}")
    _close(f"attention{T}", f"{kind} {B}x{heads}", got, ref, bound)
    if kind == "uniform":
        v0 = qkv.view(B, T, 3, C)[0, :, 2].double().mean(0)
        assert (got[0].double() - v0).abs().max().item() <= bound


@pytest.mark.parametrize("kind", ["randn", "wide"])
@pytest.mark.parametrize("B,heads", [(1, 1), (3, 8)])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 192, 1024])
def test_cross_attention_1q(T, B, heads, kind):
    """One key (63 lanes hold none), one short of a wave, a wave, one past it, the model's 192, and 1024: the whole `sattn` array."""
    L = _lib.lib()
    D = 64
    g = _gen(22, T, B, heads, len(kind))
    q, kv = torch.randn(B, heads * D, generator=g), torch.randn(B, T, 2 * heads * D, generator=g)
    if kind == "wide":
        q, kv[:, :, :heads * D] = 4.0 * q, 4.0 * kv[:, :, :heads * D]
    dq, dkv = _dev(q, kv)
    o = Out(B, heads * D)
    check(L.hands_cross_attention_1q_f32(ptr(dq), ptr(dkv), o.ptr(), B, T, heads, D, float(D ** -0.5), _stream()), "cross_attention_1q")
    args = (q, kv, B, T, heads, D, float(D ** -0.5))
    ref = R.cross_attention_1q(*args)
    bound = 5e-6
    if kind == "wide":
        bound, e32 = _rule(5e-6, ref, R.cross_attention_1q, *args)
        print(f"EDGE-F32|cross_attention_1q|wide T {T} {B}x{heads}|{e32:.3e}")
    _close("cross_attention_1q", f"{kind} T {T} {B}x{heads}", o.get(), ref, bound)


# ---- rejections: every condition below is checked by the host code before anything is launched --------------------------------------
class _Scratch:
    def __init__(self):
        self.x = torch.zeros(1 << 16, device=DEV)
        self.o = torch.full((1 << 16,), SENT, device=DEV)
        self.o2 = torch.full((1 << 16,), SENT, device=DEV)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.all(self.o == SENT)) and bool(torch.all(self.o2 == SENT))


def test_handocc_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), _Scratch()
    x, o, o2, st = ptr(s.x), ptr(s.o), ptr(s.o2), _stream()
    assert L.hands_upsample_bilinear_add_f32(x, x, o, 1, 2, 2, 4, 4, 6, st) == EINVAL                  # C % 4
    for dims in ((0, 2, 4, 4), (2, 0, 4, 4), (2, 2, 0, 4), (2, 2, 4, 0), (-1, 2, 4, 4)):
        assert L.hands_upsample_bilinear_add_f32(x, x, o, 1, *dims, 4, st) == EINVAL, dims
    assert L.hands_pool2x2_nhwc_f32(x, o, 1, 4, 4, 6, 0, st) == EINVAL
    assert L.hands_pool2x2_nhwc_f32(x, o, 1, 3, 4, 4, 0, st) == EINVAL                                 # odd H
    assert L.hands_pool2x2_nhwc_f32(x, o, 1, 4, 4, 4, 2, st) == EINVAL                                 # no such mode
    assert L.hands_channel_pool_f32(x, o, 4, 128, st) == EINVAL                                        # C != 256
    assert L.hands_gate_apply_f32(x, x, 1, o, o2, 4, 6, st) == EINVAL
    assert L.hands_add_embed2_f32(x, x, x, x, x, o, o2, 1, 4, 6, st) == EINVAL
    assert L.hands_add_rowvec_f32(x, x, o, 1, 4, 6, st) == EINVAL
    assert L.hands_token_sum_f32(x, o, 1, 4, 96, st) == EINVAL                                         # C % 64
    assert L.hands_token_sum_f32(x, o, 1, 0, 64, st) == EINVAL
    assert L.hands_bn_leaky_f32(x, x, x, o, 4, 6, st) == EINVAL
    assert L.hands_upsample_nearest2x_add_f32(x, x, o, 1, 2, 2, 6, st) == EINVAL
    assert L.hands_upsample_nearest2x_add_f32(x, x, o, 1, 0, 2, 4, st) == EINVAL
    assert L.hands_upsample_nearest2x_add_f32(x, x, o, 1, 2, 0, 4, st) == EINVAL
    assert L.hands_spatial_softmax_f32(x, 4, x, o, 4, 1, 0, 4, st) == EINVAL                           # N = 0
    assert L.hands_spatial_softmax_f32(x, 4, x, o, 4, 1, -3, 4, st) == EINVAL
    assert L.hands_spatial_softmax_f32(x, 3, x, o, 4, 1, 8, 4, st) == EINVAL                           # ld_in < J
    assert L.hands_spatial_softmax_f32(x, 4, x, o, 3, 1, 8, 4, st) == EINVAL                           # ld_out < J
    flash = lambda q2, ks, N, D: L.hands_flash_attention_f32(x, x, x, q2, ks, None, o, 1, N, 1, D, 0.125, st)
    assert flash(None, None, 128, 32) == EINVAL                                                        # head_dim != 64
    assert flash(None, None, 192, 64) == EINVAL                                                        # N % 128
    assert flash(None, None, 0, 64) == EINVAL                                                          # N = 0: a zero-size grid
    assert flash(None, None, -128, 64) == EINVAL
    assert flash(x, None, 128, 64) == EINVAL                                                           # q2 without k2sum
    assert s.untouched()


def test_transformer_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), _Scratch()
    x, o, st = ptr(s.x), ptr(s.o), _stream()
    for dims in ((0, 4, 8, 0, 8), (4, 0, 8, 0, 8), (4, 4, 8, 0, 0), (4, 4, 8, 4, 5), (4, 4, 8, -1, 4), (4, 4, 0, 0, 0)):
        assert L.hands_resize_crop_nchw3_to_nhwc4_f32(x, o, 1, *dims, st) == EINVAL, dims
    assert L.hands_layernorm_f32(x, x, x, o, None, 1, 4, 512, 1e-6, st) == EINVAL                      # no such instantiation
    assert L.hands_layernorm_f32(x, x, x, o, x, 0, 4, 256, 1e-6, st) == EINVAL                         # addvec with rows_per_vec 0
    assert L.hands_layernorm_f32(x, x, x, o, None, 1, 0, 256, 1e-6, st) == EINVAL
    assert L.hands_add_pos_f32(o, x, None, 1, 4, 6, st) == EINVAL
    assert L.hands_add_pos_f32(o, x, None, 1, 0, 4, st) == EINVAL
    assert L.hands_kpe_encode_f32(x, x, o, 2, 79, 4, st) == EINVAL                                     # ld < 20 * n_freq
    assert L.hands_kpe_encode_f32(x, x, o, 2, 400, 17, st) == EINVAL
    assert L.hands_kpe_encode_f32(x, x, o, 2, 80, 0, st) == EINVAL
    assert L.hands_attention_f32(x, o, 1, 192, 1, 64, 0.125, st) == EINVAL                             # neither built shape
    assert L.hands_attention_f32(x, o, 1, 197, 1, 80, 0.125, st) == EINVAL
    assert L.hands_attention_f32(x, o, 1, 196, 1, 64, 0.125, st) == EINVAL
    assert L.hands_cross_attention_1q_f32(x, x, o, 1, 1025, 1, 64, 0.125, st) == EINVAL                # T > 1024: past `sattn`
    assert L.hands_cross_attention_1q_f32(x, x, o, 1, 0, 1, 64, 0.125, st) == EINVAL
    assert L.hands_cross_attention_1q_f32(x, x, o, 1, 8, 1, 32, 0.125, st) == EINVAL                   # head_dim != 64
    assert L.hands_rot6d_to_matrix_cols_f32(x, 96, o, 0, st) == EINVAL
    assert s.untouched()


def test_vit_b_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), _Scratch()
    x, o, st = ptr(s.x), ptr(s.o), _stream()
    assert L.hands_vit_tokens_f32(x, x, x, o, 1, 1, 4, st) == EINVAL                                   # no patch token
    assert L.hands_vit_tokens_f32(x, x, x, o, 1, 2, 6, st) == EINVAL
    assert L.hands_vit_tokens_f32(x, x, x, o, 0, 2, 4, st) == EINVAL
    assert L.hands_vit_tail_f32(x, x, x, o, 1, 3, 768, 1e-6, st) == EINVAL                             # odd grid
    assert L.hands_vit_tail_f32(x, x, x, o, 1, 0, 768, 1e-6, st) == EINVAL
    assert L.hands_vit_tail_f32(x, x, x, o, 1, 2, 1024, 1e-6, st) == EINVAL                            # C != 768
    assert s.untouched()


def test_elementwise_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), _Scratch()
    x, o, st = ptr(s.x), ptr(s.o), _stream()
    for H, W in ((0, 4), (4, 0), (-2, 4)):
        assert L.hands_nchw3_to_nhwc4_f32(x, o, 1, H, W, st) == EINVAL, (H, W)
        assert L.hands_maxpool3x3s2_nhwc_f32(x, o, 1, H, W, 4, st) == EINVAL, (H, W)
    assert L.hands_maxpool3x3s2_nhwc_f32(x, o, 1, 4, 4, 6, st) == EINVAL
    for fn in (L.hands_sumpool_nhwc_f32, L.hands_avgpool_nhwc_f32):
        assert fn(x, o, 1, 0, 8, 8, st) == EINVAL                                                      # HW = 0
        assert fn(x, o, 1, 4, 6, 8, st) == EINVAL
        assert fn(x, o, 1, 4, 8, 10, st) == EINVAL                                                     # out_stride % 4
    assert s.untouched()


# ---- glue kernels of csrc/elementwise.hip: one case past the grid cap by a partial pass, one at the smallest legal size ---------------
def _angles(B, n_freq, g):
    """0.5 * randn angles as the model-shape tests; for n_freq = 16 |angle| <= 1e-3, which keeps 2^15 * angle within 33 rad."""
    if n_freq < 16:
        return 0.5 * torch.randn(B, 2, generator=g), 0.5 * torch.randn(B, 8, generator=g)
    return 1e-3 * (2 * torch.rand(B, 2, generator=g) - 1), 1e-3 * (2 * torch.rand(B, 8, generator=g) - 1)


@pytest.mark.parametrize("B,H,W,n_freq,mode,Cpad", [(3, 97, 89, 4, 3, 84), (2, 5, 5, 4, 1, 20), (2, 5, 5, 4, 2, 68), (1, 1, 1, 1, 1, 8),
                                                    (2, 5, 5, 16, 3, 324)])
def test_image_posenc(B, H, W, n_freq, mode, Cpad):
    """(3,97,89) x 21 float4 = 543 879 items.  Encodings at the bound of test_kpe_concat_vs_oracle; image and padding bit-equal."""
    L = _lib.lib()
    g = _gen(30, B, H, W, n_freq, mode)
    img = torch.randn(B, 3, H, W, generator=g)
    ce, co = _angles(B, n_freq, g)
    d = _dev(img, ce, co)
    o = Out(B, H, W, Cpad)
    check(L.hands_image_posenc_nhwc_f32(ptr(d[0]), ptr(d[1]) if mode & 1 else None, ptr(d[2]) if mode & 2 else None, o.ptr(), B, H, W,
                                        n_freq, mode, Cpad, _stream()), "image_posenc")
    got = o.get()
    _close("image_posenc", f"{B}x{H}x{W} n_freq {n_freq} mode {mode} Cpad {Cpad}", got, R.image_posenc_nhwc(img, ce, co, B, H, W, n_freq, mode, Cpad), 1e-6)
    nenc = (4 * n_freq if mode & 1 else 0) + (16 * n_freq if mode & 2 else 0)
    assert torch.equal(got[..., :3], img.permute(0, 2, 3, 1)) and torch.all(got[..., 3 + nenc:] == 0)


@pytest.mark.parametrize("B2,Bg,HW,C,n_freq,with_glb", [(14, 7, 457, 8, 16, True), (4, 2, 5, 8, 4, False), (2, 1, 1, 4, 1, True)])
def test_kpe_concat(B2, Bg, HW, C, n_freq, with_glb):
    """(14,7,457,8,16): 14 x 457 x 82 float4 = 524 636 items."""
    L = _lib.lib()
    g = _gen(31, B2, HW, C, n_freq)
    crop, glb = torch.randn(B2, HW, C, generator=g), torch.randn(Bg, HW, C, generator=g)
    ce, co = _angles(B2, n_freq, g)
    d = _dev(crop, glb, ce, co)
    o = Out(B2, HW, C + 20 * n_freq)
    check(L.hands_kpe_concat_f32(ptr(d[0]), ptr(d[1]) if with_glb else None, ptr(d[2]), ptr(d[3]), o.ptr(), B2, Bg, HW, C, n_freq,
                                 _stream()), "kpe_concat")
    got = o.get()
    ref = R.kpe_concat(crop, glb if with_glb else None, ce, co, B2, Bg, HW, C, n_freq)
    case = f"{B2}x{HW}x{C} n_freq {n_freq} glb {with_glb}"
    _exact("kpe_concat features", case, got[..., :C].contiguous(), crop + glb[torch.arange(B2) % Bg] if with_glb else crop, ref[..., :C])
    _close("kpe_concat encodings", case, got[..., C:].contiguous(), ref[..., C:], 1e-6)


@pytest.mark.parametrize("with_img", [True, False])
@pytest.mark.parametrize("n_freq", [0, 3])
@pytest.mark.parametrize("Hs,Ws,Rr,Ho,Wo", [(5, 9, 12, 7, 10), (5, 9, 1, 1, 1), (5, 9, 12, 1, 1), (12, 9, 12, 7, 10), (5, 12, 12, 12, 12)])
def test_dense_posenc(Hs, Ws, Rr, Ho, Wo, n_freq, with_img):
    """Non-square source and outputs, both interpolations; R = 1 and Ho = Wo = 1 (the `out > 1` guard of ac_tap); Hs == R on one axis
    only (that axis copies); Ho == Wo == R (no second interpolation).  n_freq 0: the six raw 'cam_conv' maps, offsets up to +-100."""
    L = _lib.lib()
    B, Ca = 2, (2 if n_freq else 6)
    g = _gen(32, Hs, Ws, Rr, Ho, n_freq)
    ang = 0.5 * torch.randn(B, Ca, Hs, Ws, generator=g)
    if not n_freq:
        ang[:, 2:4] *= 200.0
    msk = (torch.rand(B, Hs, Ws, generator=g) > 0.3).float()
    Cenc = 2 * n_freq * Ca if n_freq else Ca
    img = torch.randn(B, 3, Ho, Wo, generator=g) if with_img else None
    ld, c_off = ((3 + Cenc + 15) // 16 * 16, 3) if with_img else (Cenc + 8, 4)
    cols = torch.arange(ld)
    o = Out(B, Ho, Wo, ld, keep=None if with_img else ((cols < c_off) | (cols >= c_off + Cenc)).view(1, 1, 1, ld))
    d = _dev(ang, msk) + (_dev(img) if with_img else [None])
    check(L.hands_dense_posenc_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), o.ptr(), B, Ca, Hs, Ws, n_freq, Rr, Ho, Wo, ld, c_off, _stream()),
          "dense_posenc")
    got = o.get()
    args = (ang, msk, img, B, Ca, Hs, Ws, n_freq, Rr, Ho, Wo, ld, c_off)
    ref = R.dense_posenc(*args)
    enc_ref = ref[..., 3:3 + Cenc] if with_img else ref
    bound, e32 = _rule(2e-6 * max(1.0, enc_ref.abs().max().item()), ref, R.dense_posenc, *args)
    case = f"{Hs}x{Ws}->{Rr}->{Ho}x{Wo} n_freq {n_freq} img {with_img}"
    print(f"EDGE-F32|dense_posenc|{case}|{e32:.3e}")
    _close("dense_posenc", case, got if with_img else got[..., c_off:c_off + Cenc].contiguous(), ref, bound)
    if with_img:
        assert torch.equal(got[..., :3], img.permute(0, 2, 3, 1)) and torch.all(got[..., 3 + Cenc:] == 0)


@pytest.mark.parametrize("B,h,w,H,W,C", [(3, 5, 7, 83, 61, 140), (2, 1, 4, 3, 9, 8), (2, 4, 1, 6, 5, 8), (2, 3, 5, 1, 7, 4), (2, 6, 5, 6, 11, 4),
                                         (1, 1, 1, 1, 1, 4)])
def test_upsample_bilinear_ac(B, h, w, H, W, C):
    """(3,5,7)->(83,61) x 35 float4 = 531 615 items; sources of one row / one column, an output of one row, h == H with w != W."""
    L = _lib.lib()
    x = torch.randn(B, h, w, C, generator=_gen(33, B, h, w, H, W))
    dx, = _dev(x)
    o = Out(B, H, W, C)
    check(L.hands_upsample_bilinear_ac_f32(ptr(dx), o.ptr(), B, h, w, H, W, C, _stream()), "upsample_bilinear_ac")
    ref = R.upsample_bilinear_ac(x, B, h, w, H, W, C)
    bound, e32 = _rule(1e-6, ref, R.upsample_bilinear_ac, x, B, h, w, H, W, C)
    print(f"EDGE-F32|upsample_bilinear_ac|{B}x{h}x{w}->{H}x{W}x{C}|{e32:.3e}")
    _close("upsample_bilinear_ac", f"{B}x{h}x{w}->{H}x{W}x{C}", o.get(), ref, bound)


@pytest.mark.parametrize("B,Bg,HW,Ca,lda,Cb,ld,ld_add,shared", [(6, 3, 301, 250, 260, 37, 300, 256, False), (6, 3, 301, 250, 260, 37, 300, 0, False),
                                                             (4, 2, 5, 6, 6, 0, 6, 8, False), (4, 4, 5, 6, 9, 2, 12, 0, True), (1, 1, 1, 1, 1, 0, 1, 0, False)])
def test_concat_nhwc(B, Bg, HW, Ca, lda, Cb, ld, ld_add, shared):
    """(6,3,301) x ld 300 = 541 800 items with and without `add`; Cb = 0 with extra == NULL; one (HW, Cb) map shared by the batch
    (extra_batch_stride 0); a single element.  The columns behind Ca + Cb are zero."""
    L = _lib.lib()
    g = _gen(34, B, HW, Ca, Cb, ld_add)
    a, add = torch.randn(B, HW, lda, generator=g), (torch.randn(Bg, HW, ld_add, generator=g) if ld_add else None)
    ex = torch.randn(1 if shared else B, HW, Cb, generator=g) if Cb else None
    stride = 0 if shared or not Cb else HW * Cb
    d = [t.to(DEV).contiguous() if t is not None else None for t in (a, add, ex)]
    o = Out(B, HW, ld)
    check(L.hands_concat_nhwc_f32(ptr(d[0]), lda, Ca, ptr(d[1]), ld_add, ptr(d[2]), stride, Cb, o.ptr(), ld, B, Bg, HW, _stream()), "concat_nhwc")
    args = (a, lda, Ca, add, ld_add, ex, stride, Cb, ld, B, Bg, HW)
    with R.precision(torch.float32):
        e32 = R.concat_nhwc(*args)
    got = o.get()
    _exact("concat_nhwc", f"{B}x{HW} Ca {Ca}/{lda} Cb {Cb} ld {ld} add {ld_add} shared {shared}", got, e32, R.concat_nhwc(*args))
    assert torch.all(got[..., Ca + Cb:] == 0)


@pytest.mark.parametrize("B2,Bg,F_,ld_out,ld_shape", [(238, 119, 2048, 2208, 12), (4, 2, 0, 154, 10), (1, 1, 4, 160, 10)])
def test_grasp_input(B2, Bg, F_, ld_out, ld_shape):
    """238 x 2208 = 525 504 items; F = 0 at the smallest ld_out."""
    L = _lib.lib()
    g = _gen(35, B2, F_, ld_out)
    shape, rot, fv = torch.randn(B2, ld_shape, generator=g), torch.randn(B2, 144, generator=g), torch.randn(Bg, max(F_, 1), generator=g)
    d = _dev(shape, rot, fv)
    o = Out(B2, ld_out)
    check(L.hands_grasp_input_f32(ptr(d[0]), ld_shape, ptr(d[1]), ptr(d[2]), o.ptr(), B2, Bg, F_, ld_out, _stream()), "grasp_input")
    args = (shape, ld_shape, rot, fv, B2, Bg, F_, ld_out)
    with R.precision(torch.float32):
        e32 = R.grasp_input(*args)
    _exact("grasp_input", f"{B2}x{ld_out} F {F_}", o.get(), e32, R.grasp_input(*args))


@pytest.mark.parametrize("B,F_,ld", [(4682, 4, 120), (1, 0, 112)])
def test_hmr_init(B, F_, ld):
    """4682 x 112 = 524 384 items.  The F feature columns and the tail behind the 112 hold the sentinel and keep it."""
    L = _lib.lib()
    cam = torch.randn(B, 4, generator=_gen(36, B))
    dc, = _dev(cam)
    cols = torch.arange(ld)
    o = Out(B, ld, keep=((cols < F_) | (cols >= F_ + 112)).view(1, ld))
    check(L.hands_hmr_init_f32(o.ptr(), ptr(dc), B, ld, F_, _stream()), "hmr_init")
    got = o.get()[:, F_:F_ + 112].contiguous()
    state = torch.zeros(B, ld)
    with R.precision(torch.float32):
        e32 = R.hmr_init(state, cam, B, ld, F_)[:, F_:F_ + 112].contiguous()
    _exact("hmr_init", f"{B} F {F_} ld {ld}", got, e32, R.hmr_init(state, cam, B, ld, F_)[:, F_:F_ + 112])


@pytest.mark.parametrize("B,ld6", [(32769, 100), (1, 96)])
def test_rot6d_to_matrix(B, ld6):
    """32 769 x 16 = 524 304 joints; the four floats behind the 96 are NaN and never read.  Pairs at least 45 degrees apart, as for
    the columns variant above."""
    L = _lib.lib()
    d6 = torch.full((B, ld6), float("nan"))
    d6[:, :96] = _well_conditioned_6d(B * 16, _gen(37, B, ld6)).view(B, 96)
    dd, = _dev(d6)
    o = Out(B, 16, 3, 3)
    check(L.hands_rot6d_to_matrix_f32(ptr(dd), ld6, o.ptr(), B, _stream()), "rot6d_to_matrix")
    _close("rot6d_to_matrix", f"{B} ld6 {ld6}", o.get(), R.rot6d_to_matrix(d6, ld6, B), 5e-6)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_rot_conversions_second_pass(golden_dir):
    """The 513 rotations of rot_conversions.npz tiled to 524 365: row i of the two-pass launch is bit-equal to row i % 513 of a
    one-pass launch on the fixture, which test_device_rot_conversions_vs_reference_fixture pins to the reference."""
    import os

    import numpy as np
    L = _lib.lib()
    d = np.load(os.path.join(golden_dir, "rot_conversions.npz"))
    n = 524288 + 77
    for name, fn, src, width in (("matrix_to_axis_angle", L.hands_matrix_to_axis_angle_f32, torch.from_numpy(d["R"]).float().reshape(-1, 9), 3),
                                 ("axis_angle_to_matrix", L.hands_axis_angle_to_matrix_f32, torch.from_numpy(d["aa_in"]).float().reshape(-1, 3), 9)):
        m = src.shape[0]
        idx = torch.arange(n) % m
        ds, db = _dev(src, src[idx])
        small, big = Out(m, width), Out(n, width)
        check(fn(ptr(ds), small.ptr(), m, _stream()), name)
        check(fn(ptr(db), big.ptr(), n, _stream()), name)
        gs, gb = small.get(), big.get()
        assert not torch.isnan(gs).any() and _bits_equal(gb, gs[idx]), name
        print(f"EDGE|{name}|{n} rows against {m}|0.000e+00|0.000e+00")


def _flip_inputs(Bg, g):
    rot = O.axis_angle_to_matrix(torch.randn(2 * Bg, 16, 3, generator=g))
    return rot, torch.randn(2 * Bg, 10, generator=g), torch.randn(2 * Bg, 3, generator=g), torch.randn(2 * Bg, 3, generator=g)


def _run_flip(fl, ins, Bg):
    L = _lib.lib()
    d = _dev(fl, *ins)
    outs = [Out(2 * Bg, 16, 3, 3), Out(2 * Bg, 10), Out(2 * Bg, 3), Out(2 * Bg, 3)]
    check(L.hands_flip_swap_f32(*[ptr(t) for t in d], *[o.ptr() for o in outs], Bg, _stream()), "flip_swap")
    return [o.get() for o in outs]


def test_flip_swap_second_pass_and_single_samples():
    """Bg = 16 385: 524 320 items, a Bg = 5 problem with mixed flags tiled; bit-equal to the small launch, which
    test_rot6d_and_flip_vs_oracle pins.  Then Bg = 1 unflipped (a copy) and flipped (the other hand, mirrored)."""
    g = _gen(38)
    Bg, big = 5, 16385
    fl = torch.tensor([0, 1, 1, 0, 1])
    ins = _flip_inputs(Bg, g)
    small = _run_flip(fl, ins, Bg)
    idx = torch.arange(big) % Bg
    rows = torch.cat([idx, idx + Bg])
    got = _run_flip(fl[idx], [t[rows] for t in ins], big)
    for name, a, b in zip(("rotmat", "shape", "cam", "cam_init"), got, small):
        assert not torch.isnan(b).any() and _bits_equal(a, b[rows]), name
    print(f"EDGE|flip_swap|Bg {big} against Bg {Bg}|0.000e+00|0.000e+00")
    one = _flip_inputs(1, g)
    for name, a, b in zip(("rotmat", "shape", "cam", "cam_init"), _run_flip(torch.tensor([0]), one, 1), one):
        assert _bits_equal(a, b), name
    rot, shape, cam, cami = _run_flip(torch.tensor([1]), one, 1)
    aa = O.matrix_to_axis_angle(one[0].double()).clone()
    aa[..., 1:] *= -1
    sgn = torch.tensor([1.0, -1.0, 1.0])
    _close("flip_swap", "Bg 1 flipped", rot, O.axis_angle_to_matrix(aa).flip(0), 2e-6)
    assert torch.equal(shape, one[1].flip(0)) and torch.equal(cam, one[2].flip(0) * sgn) and torch.equal(cami, one[3].flip(0) * sgn)


@pytest.mark.parametrize("B", [1, 129, 300])
def test_rot_leftmul(B):
    """One thread, half a block and one, a block and 44 (B threads, never past the cap: it would take 300 MB).  144-float row stride:
    the fifteen other joints keep their bits."""
    L = _lib.lib()
    g = _gen(39, B)
    rot, fix = O.axis_angle_to_matrix(torch.randn(B, 16, 3, generator=g)), O.axis_angle_to_matrix(torch.randn(B, 3, generator=g))
    df, = _dev(fix)
    o = Out(B, 16, 3, 3, init=rot)
    check(L.hands_rot_leftmul_f32(o.ptr(), ptr(df), B, _stream()), "rot_leftmul")
    got, ref = o.get(), R.rot_leftmul(rot, fix, B)
    bound, e32 = _rule(1e-6, ref, R.rot_leftmul, rot, fix, B)
    print(f"EDGE-F32|rot_leftmul|{B}|{e32:.3e}")
    _close("rot_leftmul", f"{B}", got, ref, bound)
    assert _bits_equal(got[:, 1:], rot[:, 1:])


@pytest.mark.parametrize("flagged", [False, True])
@pytest.mark.parametrize("Bg", [1, 129, 300])
def test_perspective_correction(Bg, flagged):
    """2 Bg threads, each scanning the Bg flags.  No flag set: `rotmat` receives the corrected joint 0 too; one flag set (the last):
    `rotmat`, here all sentinel, is left as it was."""
    L = _lib.lib()
    g = _gen(40, Bg)
    rot = O.axis_angle_to_matrix(torch.randn(2 * Bg, 16, 3, generator=g))
    center = 0.4 * torch.randn(2 * Bg, 2, generator=g)
    fl = torch.zeros(Bg, dtype=torch.int64)
    fl[Bg - 1] = int(flagged)
    dc, dfl = _dev(center, fl)
    sent = torch.full((2 * Bg, 16, 3, 3), SENT)
    sw, un = Out(2 * Bg, 16, 3, 3, init=rot), Out(2 * Bg, 16, 3, 3, init=sent)
    check(L.hands_perspective_correction_f32(sw.ptr(), un.ptr(), ptr(dc), ptr(dfl), Bg, _stream()), "perspective_correction")
    gs, gu = sw.get(), un.get()
    rs, _ = R.perspective_correction(rot, sent, center, fl, Bg)
    bound, e32 = _rule(1e-6, rs, lambda *a: R.perspective_correction(*a)[0], rot, sent, center, fl, Bg)
    print(f"EDGE-F32|perspective_correction|Bg {Bg} flagged {flagged}|{e32:.3e}")
    _close("perspective_correction", f"Bg {Bg} flagged {flagged}", gs, rs, bound)
    assert _bits_equal(gs[:, 1:], rot[:, 1:]) and torch.all(gu[:, 1:] == SENT)
    assert torch.all(gu[:, 0] == SENT) if flagged else _bits_equal(gu[:, 0], gs[:, 0])


def test_glue_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), _Scratch()
    x, o, o2, st = ptr(s.x), ptr(s.o), ptr(s.o2), _stream()
    ip = lambda B, H, W, nf, mode, Cp, ce=x, co=x: L.hands_image_posenc_nhwc_f32(x, ce, co, o, B, H, W, nf, mode, Cp, st)
    assert ip(1, 2, 2, 4, 3, 80) == EINVAL and ip(1, 2, 2, 4, 3, 82) == EINVAL                        # Cpad too small / % 4
    assert ip(1, 2, 2, 0, 3, 84) == EINVAL and ip(1, 2, 2, 17, 1, 72) == EINVAL and ip(1, 2, 2, 4, 0, 84) == EINVAL and ip(1, 2, 2, 4, 4, 84) == EINVAL
    assert ip(0, 2, 2, 4, 3, 84) == EINVAL and ip(1, 0, 2, 4, 3, 84) == EINVAL
    assert ip(1, 2, 2, 4, 1, 20, None) == EINVAL and ip(1, 2, 2, 4, 2, 68, x, None) == EINVAL          # the mode's angles missing
    dp = lambda Ca, Hs, nf, Rr, Ho, ld, c_off, img=None: L.hands_dense_posenc_f32(x, x, img, o, 1, Ca, Hs, Hs, nf, Rr, Ho, Ho, ld, c_off, st)
    assert dp(2, 4, 3, 8, 4, 11, 0) == EINVAL and dp(2, 4, 3, 8, 4, 16, 5) == EINVAL                  # ld < c_off + Cenc
    assert dp(2, 4, 3, 8, 4, 16, 4, x) == EINVAL                                                       # with img c_off is 3
    assert dp(0, 4, 3, 8, 4, 16, 0) == EINVAL and dp(2, 0, 3, 8, 4, 16, 0) == EINVAL and dp(2, 4, 17, 8, 4, 80, 0) == EINVAL
    assert dp(2, 4, 3, 0, 4, 16, 0) == EINVAL and dp(2, 4, 3, 8, 0, 16, 0) == EINVAL and dp(2, 4, 3, 8, 4, 16, -1) == EINVAL
    cc = lambda lda, Ca, add, ld_add, extra, Cb, ld, B=2, Bg=1, HW=4: L.hands_concat_nhwc_f32(x, lda, Ca, add, ld_add, extra, 0, Cb, o, ld, B, Bg, HW, st)
    assert cc(4, 6, None, 0, None, 0, 8) == EINVAL and cc(6, 6, None, 0, None, 2, 8) == EINVAL        # lda < Ca; Cb without a map
    assert cc(6, 6, None, 0, x, 2, 7) == EINVAL and cc(6, 6, x, 5, None, 0, 8) == EINVAL              # ld < Ca + Cb; ld_add < Ca
    assert cc(6, 6, None, 0, None, 0, 8, B=0) == EINVAL and cc(6, 6, None, 0, None, 0, 8, Bg=0) == EINVAL and cc(6, 6, None, 0, None, 0, 8, HW=0) == EINVAL
    up = lambda h, w, H, W, C: L.hands_upsample_bilinear_ac_f32(x, o, 1, h, w, H, W, C, st)
    assert up(2, 2, 4, 4, 6) == EINVAL and up(2, 2, 4, 4, 0) == EINVAL and up(0, 2, 4, 4, 4) == EINVAL and up(2, 2, 4, 0, 4) == EINVAL
    assert L.hands_rot_leftmul_f32(o, x, 0, st) == EINVAL and L.hands_rot_leftmul_f32(o, None, 2, st) == EINVAL
    assert L.hands_perspective_correction_f32(o, o2, x, x, 0, st) == EINVAL and L.hands_perspective_correction_f32(o, o2, x, None, 2, st) == EINVAL
    kc = lambda B2, Bg, C, nf: L.hands_kpe_concat_f32(x, x, x, x, o, B2, Bg, 4, C, nf, st)
    assert kc(2, 1, 6, 4) == EINVAL and kc(2, 1, 8, 0) == EINVAL and kc(2, 1, 8, 17) == EINVAL and kc(0, 1, 8, 4) == EINVAL and kc(2, 0, 8, 4) == EINVAL
    assert L.hands_hmr_init_f32(o, x, 2, 115, 4, st) == EINVAL and L.hands_hmr_init_f32(o, x, 0, 116, 4, st) == EINVAL   # ld < F + 112
    assert L.hands_rot6d_to_matrix_f32(x, 96, o, 0, st) == EINVAL and L.hands_rot6d_to_matrix_f32(None, 96, o, 2, st) == EINVAL
    assert L.hands_flip_swap_f32(x, x, x, x, x, o, o2, o2, o2, 0, st) == EINVAL
    assert L.hands_flip_swap_f32(x, x, x, x, None, o, o2, o2, o2, 2, st) == EINVAL
    assert L.hands_grasp_input_f32(x, 10, x, x, o, 2, 1, 4, 157, st) == EINVAL and L.hands_grasp_input_f32(x, 10, x, x, o, 0, 1, 4, 160, st) == EINVAL
    assert L.hands_grasp_input_f32(x, 10, x, x, o, 2, 0, 4, 160, st) == EINVAL
    assert L.hands_matrix_to_axis_angle_f32(x, o, 0, st) == EINVAL and L.hands_axis_angle_to_matrix_f32(x, o, 0, st) == EINVAL
    assert L.hands_axis_angle_to_matrix_f32(None, o, 4, st) == EINVAL
    assert s.untouched()
