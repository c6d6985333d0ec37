"""Edge and isolation parity of the Winograd and stem kernels -- hands_conv3x3_winograd4_f32 (csrc/conv_wino4.hip, F(4x4, 3x3)),
hands_conv3x3_winograd_f32 (csrc/conv_wino.hip, F(2x2, 3x3)), hands_stem_conv_maxpool_nhwc_f32 and
hands_stem_conv_maxpool_nchw_f32 (csrc/stem_pool.hip) -- called through the C ABI on the smallest maps that reach each block
geometry.  tests/test_gpu_winograd.py, test_gpu_winograd4.py and the stem tests of test_gpu_parity.py check the arithmetic of
random layers with one tolerance per tensor on exact-size allocations; here

  1. every output is an edge_util.Out (sentinel bands on both sides, the sentinel in every gap [Cout, out_ps)), every input an
     edge_util.In (NaN in front and behind, NaN in every gap [Cin, in_ps), the pointer a non-zero multiple of 4 floats inside its
     allocation), weights and bias likewise: a store past the map or a read around the tensor fails the case;
  (a) every written element is compared with the float64 restatement (kernel_refs.conv_ref / stem_pool_ref, pinned on the CPU by
     tests/test_kernel_refs.py).  Stem: min(2e-5 max(1, max|ref|), (Kpad + 4) 2^-24 A_pool), the rule of test_gpu_conv_edges.py
     carried through the pool by |max a - max b| <= max|a - b|.  Winograd has no forward bound of that form; it keeps the
     project's constants (3e-5 for F(2x2), 5e-5 for F(4x4)) but per (image, channel): tol * max over the image's pixels of
     A = conv(|x|, |w|) + |bias|, so a small channel or image is held to its own scale;
  (b) w[c] and bias[c] times 2^e_c (e_c in [-6, 6], different inside a 4-channel quad and across the 32-channel seam) gives
     channel c times 2^e_c BIT FOR BIT: rounding commutes with a power of two (no value here is near the denormals), the
     activations are positively homogeneous, the pool is monotone.  The base run's bias is constant over groups of eight
     channels while its weights are not, so a bias read from a neighbouring quad shows only in the scaled run;
  (c) one interior image set to NaN (and once per kernel to +inf) leaves every other image's output bit-equal to the clean run,
     on geometries whose blocks hold tiles of several images, and comes out NaN wherever it is written, under every activation
     (ReLU and the max-pool hand a NaN on, as torch.relu and nn.MaxPool2d do: relu_f32 / pool_tap of csrc/common.h).  Stem: ONE NaN
     pixel, whose windows mix NaN and finite taps, gives NaN exactly where the float64 restatement has it and, for the NHWC4
     entry, the bits of the unfused pair;
  (d) the strided / offset launch equals the contiguous launch of the same values bit for bit (Winograd);
  (e) stem: every convolution output negative by construction (x > 0, w < 0, bias -8: with and without the bias), so a 0 in
     place of the pool's -inf changes every output; the NHWC4 entry equals hands_conv2d_nhwc_f32 + hands_maxpool3x3s2_nhwc_f32
     bit for bit on every shape and activation;
  (f) what the entries must refuse returns HANDS_EINVAL and launches nothing.
No call here hands a launching entry a pointer or stride outside the contract of include/hands_hip.h.

Geometries (nw = tile columns; "rows" = B * tile rows, never a multiple of the block's, so the last block is partial and, B > 1,
a block holds tiles of two images).  Which test covers what:

  entry / path                                  (a) (b) (c) (d)   cases
  F(4x4)  D = 2        W = 1 3 5 8               x   x   x   x    W4_CASES[0:5]
          D = 4        W = 9 13 16 | 17 19 | 57  x   x   x   x    W4_CASES[5:12], [21:24]   (one / two / four segments)
          linear 7     W = 25 26 27 28           x   x   x   x    W4_CASES[12:17]           (all four column remainders)
          linear 14    W = 53 55 56              x   x   x   x    W4_CASES[17:21]           (two virtual rows)
          channels (16,32) NOB 1 | (24,64) three k-stages, NOB 2 | (32,96) three blocks | (16,128) two workgroups
  F(2x2)  D = 4        W = 1 2 5 8 | 31          x   x   x   x    W2_CASES[0:5], [17:20]    (31: nw = 16 through nw % 4 == 0)
          linear 7/14  W = 13 14 | 27 28         x   x   x   x    W2_CASES[5:13]
          D = 8        W = 17 19 21              x   x   x   x    W2_CASES[13:17]
          channels (16,32) | (48,64) | (32,96)
  stem NHWC4 / planar  STEM_SHAPES x 3 acts      x   x   x   .    test_stem_edges (e: the pair), test_stem_all_negative (e)
  host checks                                                      test_*_rejections (f), test_engine_* (routing, executed MACs)
"""
import ctypes as C
import functools

import pytest
import torch

import kernel_refs as R
from edge_util import DEV, EINVAL, In, Out, Scratch, _close, _close_each, _gen, _stream, gap_mask, strided
from hands_amd import _lib
from hands_amd._lib import ConvDesc, ptr
from hands_amd.engine import ConvEngine
from hands_amd.packing import pack_conv, pack_linear

pytestmark = pytest.mark.gpu

NAN, INF, U = float("nan"), float("inf"), 2.0 ** -24
BF16X3 = 0x100
TOL = {"f4": 5e-5, "f2": 3e-5}          # tests/test_gpu_winograd4.py, tests/test_gpu_winograd.py
CHANNELS = {"f4": [(16, 32), (24, 64), (32, 96), (16, 128)], "f2": [(16, 32), (48, 64), (32, 96)]}

# (B, H, W, channel pair, act, strided layout)
W4_CASES = [
    (5, 5, 1, 0, 0, False), (3, 1, 3, 1, 1, True), (5, 3, 5, 2, 3, False), (7, 9, 8, 3, 1, False), (2, 4, 8, 0, 3, True),        # D = 2
    (5, 5, 9, 1, 0, True), (3, 9, 13, 2, 1, False), (3, 4, 16, 3, 3, False), (2, 3, 16, 0, 1, True),                            # D = 4
    (5, 5, 17, 1, 3, False), (3, 1, 19, 2, 0, True), (2, 9, 19, 0, 1, False),                                                   # D = 4, 2 segments
    (5, 5, 25, 0, 0, False), (3, 3, 26, 1, 1, True), (2, 9, 27, 2, 3, False), (5, 4, 28, 3, 1, False), (3, 1, 27, 0, 3, True),  # linear 7
    (3, 5, 53, 1, 0, False), (2, 3, 55, 2, 1, True), (3, 4, 56, 3, 3, False), (2, 9, 56, 0, 1, False),                          # linear 14
    (3, 5, 57, 1, 1, False), (2, 1, 57, 2, 3, True), (5, 9, 57, 3, 0, False),                                                   # D = 4, 4 segments
]
W2_CASES = [
    (5, 3, 1, 0, 0, False), (3, 1, 2, 1, 1, True), (3, 7, 5, 2, 3, False), (5, 2, 8, 0, 1, True), (3, 3, 8, 1, 3, False),        # D = 4
    (5, 3, 13, 0, 0, False), (3, 7, 14, 1, 1, True), (3, 1, 13, 2, 3, False), (5, 2, 14, 1, 3, False),                          # linear 7
    (3, 3, 27, 1, 0, True), (5, 1, 28, 2, 1, False), (2, 7, 28, 0, 3, False), (3, 2, 27, 0, 1, False),                          # linear 14
    (5, 3, 17, 0, 0, False), (3, 3, 19, 1, 1, True), (5, 1, 21, 2, 3, False), (3, 2, 21, 0, 1, True),                           # D = 8
    (3, 3, 31, 1, 0, False), (5, 2, 31, 2, 1, True), (3, 7, 31, 0, 3, False),                                                   # D = 4, nw = 16
]
CASES = {"f4": W4_CASES, "f2": W2_CASES}


def _block_rows(kind, W):
    """-> (tile rows, or for the linear orders tiles, per block; tiles per row in that count) of the launch for this width."""
    t = 4 if kind == "f4" else 2
    nw = -(-W // t)
    if nw in (7, 14):
        return 32, nw
    if kind == "f4":
        return (16 if nw <= 2 else 8), 1
    return (8 if (nw % 4 == 0 or nw < 8) else 4), 1


# ---- values, shared by every layout and test of a geometry ----------------------------------------------------------------------
def _exponents(Cout):
    c = torch.arange(Cout)
    return ((7 * c + 3 * (c // 4) + 5 * (c // 32)) % 13 - 6).double()


@functools.lru_cache(maxsize=None)
def _layer(kind, Cin, Cout, variant):
    """w, bias and the CPU pack of a layer.  variant 0: random bias; 1: the bias constant over groups of eight channels (the
    base of check (b)); 2: variant 1 with channel c times 2^e_c."""
    gen = _gen(7101, Cin, Cout)
    w = torch.randn(Cout, Cin, 3, 3, generator=gen) / (9 * Cin) ** 0.5
    bias = torch.randn(Cout, generator=gen)
    if variant:
        bias = bias[torch.arange(Cout) // 8 * 8].clone()
    if variant == 2:
        s = (2.0 ** _exponents(Cout)).float()
        w, bias = w * s.view(-1, 1, 1, 1), bias * s
    pc = pack_conv(w, bias, 1, 1, "cpu", winograd4=(kind == "f4"))
    assert (pc.Cin, pc.Cout) == (Cin, Cout) and (pc.wino4 if kind == "f4" else pc.wino) is not None
    return pc


@functools.lru_cache(maxsize=None)
def _image(B, H, W, Cin):
    return torch.randn(B, H, W, Cin, generator=_gen(7102, B, H, W, Cin))


@functools.lru_cache(maxsize=None)
def _reference(kind, B, H, W, Cin, Cout, act, variant):
    """-> (expected, bound), (B, H, W, Cout) float64: conv_ref of the contiguous layer; bound[b, :, :, c] = tol * max_pixels A[b, :, :, c]."""
    pc = _layer(kind, Cin, Cout, variant)
    d = ConvDesc(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, Cin, Cout, 0, pc.Kpad, act)
    exp, mag = R.conv_ref(d, _image(B, H, W, Cin).reshape(-1), pc.w, pc.bias, None, torch.zeros(B * H * W * Cout))
    mag = mag.view(B, H, W, Cout)
    return exp.view(B, H, W, Cout), (TOL[kind] * mag.amax(dim=(1, 2), keepdim=True)).expand(B, H, W, Cout).contiguous()


def _launch(kind, x, pc, act, gap, leads=(12, 4, 8)):
    """One launch on guarded buffers -> the written elements (B, H, W, Cout) on the CPU (bands and gaps checked by Out.get)."""
    L = _lib.lib()
    B, H, W, Cin = x.shape
    Cout, M = pc.Cout, B * H * W
    in_ps, out_ps = Cin + (4 if gap else 0), Cout + (4 if gap else 0)
    X = In(strided(x.reshape(M, Cin), in_ps, NAN), leads[0])
    Ud, Bd = In(pc.wino4 if kind == "f4" else pc.wino, leads[1]), In(pc.bias, leads[2])
    out = Out(M, out_ps, keep=gap_mask(M, out_ps, Cout))
    d = ConvDesc(B, H, W, Cin, H, W, Cout, 3, 3, 1, 1, in_ps, out_ps, 0, pc.Kpad, act)
    sup, fn = ((L.hands_conv3x3_winograd4_supported, L.hands_conv3x3_winograd4_f32) if kind == "f4" else
               (L.hands_conv3x3_winograd_supported, L.hands_conv3x3_winograd_f32))
    assert sup(C.byref(d)) == 1
    assert fn(C.byref(d), X.ptr(), Ud.ptr(), Bd.ptr(), out.ptr(), _stream()) == 0
    return out.get().view(M, out_ps)[:, :Cout].reshape(B, H, W, Cout).clone()


def _ids(kind):
    return [f"{kind}-{B}x{H}x{W}-c{ch}-a{act}-{'gap' if gap else 'contig'}" for B, H, W, ch, act, gap in CASES[kind]]


ALL = [(k,) + c for k in ("f4", "f2") for c in CASES[k]]


@pytest.mark.parametrize("kind,B,H,W,ch,act,gap", ALL, ids=_ids("f4") + _ids("f2"))
def test_winograd_edges(kind, B, H, W, ch, act, gap):
    """(1), (a) and, on the strided third of the table, (d)."""
    Cin, Cout = CHANNELS[kind][ch]
    pc, x = _layer(kind, Cin, Cout, 0), _image(B, H, W, Cin)
    got = _launch(kind, x, pc, act, gap)
    ref, bound = _reference(kind, B, H, W, Cin, Cout, act, 0)
    _close_each(f"wino_{kind}", f"a-{B}x{H}x{W}-c{ch}-a{act}-{'gap' if gap else 'contig'}", got, ref, bound)
    if gap:
        twin = _launch(kind, x, pc, act, False, leads=(4, 8, 12))
        assert torch.equal(got, twin), "layout changed the bits"


SCALED = [("f4", 5, 5, 25, 0, 1), ("f4", 3, 4, 56, 3, 3), ("f4", 7, 9, 8, 3, 0), ("f4", 3, 9, 13, 2, 1), ("f4", 5, 5, 17, 1, 3),
          ("f2", 5, 3, 13, 0, 3), ("f2", 3, 3, 27, 1, 1), ("f2", 3, 7, 5, 2, 0), ("f2", 3, 3, 19, 1, 1)]


@pytest.mark.parametrize("kind,B,H,W,ch,act", SCALED, ids=lambda v: str(v))
def test_winograd_channel_scaling_is_exact(kind, B, H, W, ch, act):
    """(b), with (a) on both runs: the scaled run spreads the channels over 2^12 of magnitude, which is where the per-channel
    bound parts from the per-tensor one."""
    Cin, Cout = CHANNELS[kind][ch]
    x = _image(B, H, W, Cin)
    outs = []
    for variant in (1, 2):
        got = _launch(kind, x, _layer(kind, Cin, Cout, variant), act, False)
        ref, bound = _reference(kind, B, H, W, Cin, Cout, act, variant)
        _close_each(f"wino_{kind}", f"b{variant}-{B}x{H}x{W}-c{ch}-a{act}", got, ref, bound)
        outs.append(got)
    s = (2.0 ** _exponents(Cout)).float()
    assert torch.equal(outs[1], outs[0] * s), ((outs[1] - outs[0] * s).abs() / s).max().item()


POISON = [("f4", 5, 5, 25, 0, 0, NAN), ("f4", 7, 9, 8, 3, 3, NAN), ("f4", 5, 5, 17, 1, 0, NAN), ("f4", 3, 5, 53, 1, 3, NAN),
          ("f4", 5, 4, 28, 3, 1, NAN), ("f4", 3, 4, 16, 3, 0, INF),
          ("f2", 5, 3, 13, 0, 0, NAN), ("f2", 3, 7, 5, 2, 3, NAN), ("f2", 3, 3, 27, 1, 3, NAN), ("f2", 5, 2, 8, 0, 1, NAN),
          ("f2", 3, 3, 31, 1, 0, NAN), ("f2", 3, 3, 19, 1, 3, NAN), ("f2", 5, 2, 14, 1, 0, INF)]


def _poison_check(name, clean, bad, b, act):
    """(c): image b is the poisoned one."""
    B = clean.shape[0]
    others = [i for i in range(B) if i != b]
    assert 0 < b < B - 1
    assert not torch.isnan(clean).any(), name
    assert torch.equal(bad[others], clean[others]), (name, "a non-finite image leaked into its neighbours")
    assert torch.isnan(bad[b]).all(), (name, act, "the poisoned image is not NaN throughout")


@pytest.mark.parametrize("kind,B,H,W,ch,act,poison", POISON, ids=lambda v: str(v))
def test_winograd_image_isolation(kind, B, H, W, ch, act, poison):
    per, mul = _block_rows(kind, W)
    assert -(-H // (4 if kind == "f4" else 2)) * mul < per, "no block of this geometry holds two images"
    Cin, Cout = CHANNELS[kind][ch]
    pc, x = _layer(kind, Cin, Cout, 0), _image(B, H, W, Cin)
    clean = _launch(kind, x, pc, act, False)
    xb = x.clone()
    xb[B // 2] = poison
    _poison_check((kind, B, H, W), clean, _launch(kind, xb, pc, act, False), B // 2, act)


# ---- the fused stem -------------------------------------------------------------------------------------------------------------
STEM_SHAPES = [(2, 7, 7), (1, 8, 9), (3, 10, 11), (1, 25, 29), (2, 28, 32), (2, 29, 33), (1, 27, 36), (3, 7, 64), (2, 57, 7)]
PLANAR_COL = [c * 52 + t for c in range(3) for t in range(49)]


def _pooled(H, W):
    Hc, Wc = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return Hc, Wc, (Hc - 1) // 2 + 1, (Wc - 1) // 2 + 1


@functools.lru_cache(maxsize=None)
def _stem_layer(variant):
    """The stem's weight in both packings.  variant 0: random; 2: channel c times 2^e_c; 3: w < 0 and bias -8 (check (e))."""
    gen = _gen(7103)
    w = torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5
    bias = torch.randn(64, generator=gen)
    if variant == 2:
        s = (2.0 ** _exponents(64)).float()
        w, bias = w * s.view(-1, 1, 1, 1), bias * s
    if variant == 3:
        w, bias = -0.25 * w.abs(), torch.full((64,), -8.0)
    pc = pack_conv(w, bias, 2, 3, "cpu", cin_pad_to=4)
    pp = pack_linear(w.reshape(64, 147), bias, "cpu", col_index=PLANAR_COL, k_total=160)
    assert pc.w.shape == (128, 208) and pp.w.shape == (128, 160)
    return pc, pp


@functools.lru_cache(maxsize=None)
def _stem_image(B, H, W, positive=False):
    x = torch.randn(B, 3, H, W, generator=_gen(7104, B, H, W))
    return x.abs() + 0.1 if positive else x


def _nhwc4(x):
    B, _, H, W = x.shape
    return torch.cat([x.permute(0, 2, 3, 1), torch.zeros(B, H, W, 1)], -1).contiguous()      # the 4th channel is 0 (header)


@functools.lru_cache(maxsize=None)
def _stem_reference(planar, B, H, W, act, variant):
    """-> (expected, bound) (B, Hp, Wp, 64): min(2e-5 max(1, max|ref|), (Kpad + 4) 2^-24 A_pool)."""
    pc, pp = _stem_layer(variant)
    x = _stem_image(B, H, W, variant == 3)
    ref, mag = R.stem_pool_ref(x, pp.w, pp.bias, B, H, W, act, planar=True) if planar else R.stem_pool_ref(_nhwc4(x), pc.w, pc.bias, B, H, W, act)
    first = 2e-5 * max(1.0, ref.abs().max().item())
    return ref, torch.minimum(torch.full_like(mag, first), ((160 if planar else 208) + 4) * U * mag)


def _stem_launch(planar, x, act, variant=0):
    """x (B, 3, H, W) on the CPU -> the pooled map (B, Hp, Wp, 64) of one launch on guarded buffers."""
    L = _lib.lib()
    B, _, H, W = x.shape
    _, _, Hp, Wp = _pooled(H, W)
    pc, pp = _stem_layer(variant)
    X = In(x, 4) if planar else In(_nhwc4(x), 8)
    Wd, Bd = In(pp.w if planar else pc.w, 12), In(pp.bias if planar else pc.bias, 4)
    out = Out(B * Hp * Wp, 64)
    fn = L.hands_stem_conv_maxpool_nchw_f32 if planar else L.hands_stem_conv_maxpool_nhwc_f32
    assert fn(X.ptr(), Wd.ptr(), Bd.ptr(), out.ptr(), B, H, W, act, _stream()) == 0
    return out.get().view(B, Hp, Wp, 64).clone()


def _unfused_pair(x, act, variant=0):
    """hands_conv2d_nhwc_f32 on the RGB0 image, then hands_maxpool3x3s2_nhwc_f32: what the NHWC4 entry promises to equal."""
    L = _lib.lib()
    B, _, H, W = x.shape
    Hc, Wc, Hp, Wp = _pooled(H, W)
    pc, _ = _stem_layer(variant)
    X, Wd, Bd = In(_nhwc4(x), 8), In(pc.w, 12), In(pc.bias, 4)
    mid, out = Out(B * Hc * Wc, 64), Out(B * Hp * Wp, 64)
    d = ConvDesc(B, H, W, 4, Hc, Wc, 64, 7, 7, 2, 3, 4, 64, 0, 208, act)
    assert L.hands_conv2d_nhwc_f32(C.byref(d), X.ptr(), Wd.ptr(), Bd.ptr(), None, mid.ptr(), _stream()) == 0
    mid.get()
    assert L.hands_maxpool3x3s2_nhwc_f32(mid.ptr(), out.ptr(), B, Hc, Wc, 64, _stream()) == 0
    return out.get().view(B, Hp, Wp, 64).clone()


@pytest.mark.parametrize("act", [0, 1, 3])
@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("planar", [False, True], ids=["nhwc4", "nchw"])
def test_stem_edges(planar, shape, act):
    """(1) and (a) on every shape and activation; (e), second half, for the NHWC4 entry."""
    B, H, W = shape
    x = _stem_image(B, H, W)
    got = _stem_launch(planar, x, act)
    ref, bound = _stem_reference(planar, B, H, W, act, 0)
    _close_each("stem_nchw" if planar else "stem_nhwc4", f"a-{B}x{H}x{W}-a{act}", got, ref, bound)
    if not planar:
        assert torch.equal(got, _unfused_pair(x, act)), "the fused stem differs from convolution + max-pool"


@pytest.mark.parametrize("act", [0, 3])
@pytest.mark.parametrize("planar", [False, True], ids=["nhwc4", "nchw"])
def test_stem_all_negative(planar, act):
    """(e): x > 0, w < 0, bias -8 -- every convolution output is negative with and without its bias (the kernels pool before they add
    it), so the maximum of EVERY window, the clipped border ones included, is below any 0 that stood in for a missing tap."""
    B, H, W = 2, 29, 33
    conv_max, _ = _stem_reference(planar, B, H, W, 0, 3)
    pc, _ = _stem_layer(3)
    assert conv_max.max().item() < -8.0 and pc.bias[:64].eq(-8).all()      # the largest value of every window: all of them are below the bias
    x = _stem_image(B, H, W, True)
    got = _stem_launch(planar, x, act, 3)
    ref, bound = _stem_reference(planar, B, H, W, act, 3)
    assert ref.max().item() < 0
    _close_each("stem_nchw" if planar else "stem_nhwc4", f"e-negative-a{act}", got, ref, bound)
    if not planar:
        assert torch.equal(got, _unfused_pair(x, act, 3))


@pytest.mark.parametrize("shape,act", [((2, 29, 33), 3), ((3, 10, 11), 1), ((1, 25, 29), 0)], ids=lambda v: str(v))
@pytest.mark.parametrize("planar", [False, True], ids=["nhwc4", "nchw"])
def test_stem_channel_scaling_is_exact(planar, shape, act):
    """(b) for the stem: bias and activation follow the maximum, all three commute with 2^e_c."""
    B, H, W = shape
    x = _stem_image(B, H, W)
    base, scaled = _stem_launch(planar, x, act), _stem_launch(planar, x, act, 2)
    ref, bound = _stem_reference(planar, B, H, W, act, 2)
    _close_each("stem_nchw" if planar else "stem_nhwc4", f"b2-{B}x{H}x{W}-a{act}", scaled, ref, bound)
    assert torch.equal(scaled, base * (2.0 ** _exponents(64)).float())


@pytest.mark.parametrize("act,poison", [(0, NAN), (3, NAN), (1, NAN), (0, INF)], ids=lambda v: str(v))
@pytest.mark.parametrize("shape", [(3, 10, 11), (3, 7, 64)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("planar", [False, True], ids=["nhwc4", "nchw"])
def test_stem_image_isolation(planar, shape, act, poison):
    """(c) for the stem.  The pool hands a NaN on, as nn.MaxPool2d does (fmaxf alone would answer the -inf it starts from)."""
    B, H, W = shape
    x = _stem_image(B, H, W)
    xb = x.clone()
    xb[1] = poison
    bad = _stem_launch(planar, xb, act)
    _poison_check(("stem", planar, shape), _stem_launch(planar, x, act), bad, 1, act)
    if not planar:
        pair = _unfused_pair(xb, act)
        assert torch.equal(torch.isnan(bad), torch.isnan(pair)) and torch.equal(bad.nan_to_num(), pair.nan_to_num())


@pytest.mark.parametrize("act", [0, 1, 3])
@pytest.mark.parametrize("planar", [False, True], ids=["nhwc4", "nchw"])
def test_stem_single_nan_pixel(planar, act):
    """(c), the partially poisoned window: one NaN value in one colour of one pixel of image 1.  The convolution outputs whose 7 x 7
    window holds it are NaN, the pool windows around them mix NaN and finite taps: NaN exactly where the float64 restatement
    (ATen, which hands NaN through relu and max-pool) has it, every other element within its bound, the neighbouring images
    bit-equal to the clean run, and the NHWC4 entry equal to convolution + max-pool under all three activations."""
    B, H, W = 3, 29, 33
    x = _stem_image(B, H, W)
    xb = x.clone()
    xb[1, 1, 13, 20] = NAN
    got, clean = _stem_launch(planar, xb, act), _stem_launch(planar, x, act)
    pc, pp = _stem_layer(0)
    ref, mag = R.stem_pool_ref(xb, pp.w, pp.bias, B, H, W, act, planar=True) if planar else R.stem_pool_ref(_nhwc4(xb), pc.w, pc.bias, B, H, W, act)
    holes = torch.isnan(ref)
    assert holes[1].any() and not holes[1].all() and not holes[0].any() and not holes[2].any()      # a partial poison: the case is what it says
    first = 2e-5 * max(1.0, ref[~holes].abs().max().item())
    bound = torch.minimum(torch.full_like(mag, first), ((160 if planar else 208) + 4) * U * mag)
    _close_each("stem_nchw" if planar else "stem_nhwc4", f"c-one-nan-pixel-a{act}", got, ref, bound)
    assert torch.equal(got[[0, 2]], clean[[0, 2]]) and torch.equal(got[1][~holes[1]], clean[1][~holes[1]])
    if not planar:
        pair = _unfused_pair(xb, act)
        assert torch.equal(torch.isnan(got), torch.isnan(pair)) and torch.equal(got.nan_to_num(), pair.nan_to_num())


# ---- (f) rejections and the engine's routing ------------------------------------------------------------------------------------
def test_stem_rejections():
    L, s, z = _lib.lib(), Scratch(), _stream()
    x, o = ptr(s.x), ptr(s.o)
    for fn in (L.hands_stem_conv_maxpool_nhwc_f32, L.hands_stem_conv_maxpool_nchw_f32):
        bad = {"H = 6": (x, x, x, o, 1, 6, 8, 1), "W = 6": (x, x, x, o, 1, 8, 6, 1), "B = 0": (x, x, x, o, 0, 8, 8, 1),
               "act = 2": (x, x, x, o, 1, 8, 8, 2), "act = 1 | 0x100": (x, x, x, o, 1, 8, 8, 1 | BF16X3),
               "x NULL": (None, x, x, o, 1, 8, 8, 1), "w NULL": (x, None, x, o, 1, 8, 8, 1), "bias NULL": (x, x, None, o, 1, 8, 8, 1),
               "out NULL": (x, x, x, None, 1, 8, 8, 1)}
        for name, a in bad.items():
            assert fn(*a, z) == EINVAL, (fn.__name__, name)
    assert s.untouched()


def test_winograd_rejections():
    L, s, z = _lib.lib(), Scratch(), _stream()
    x, o = ptr(s.x), ptr(s.o)

    def desc(Cin=32, Cout=32, Ho=8, in_ps=None, out_ps=None, act=1):
        return ConvDesc(2, 8, 8, Cin, Ho, 8, Cout, 3, 3, 1, 1, in_ps or Cin, out_ps or Cout, 0, 9 * Cin, act)

    for sup, macs, fn, extra in (
            (L.hands_conv3x3_winograd4_supported, L.hands_conv3x3_winograd4_executed_macs, L.hands_conv3x3_winograd4_f32,
             {"Cin = 8": desc(Cin=8), "bf16x3": desc(act=1 | BF16X3), "in_ps = Cin + 2": desc(in_ps=34)}),
            (L.hands_conv3x3_winograd_supported, L.hands_conv3x3_winograd_executed_macs, L.hands_conv3x3_winograd_f32,
             {"in_ps % 4": desc(in_ps=34)})):
        ok = desc()
        assert sup(C.byref(ok)) == 1 and macs(C.byref(ok)) > 0
        for k in range(4):                                   # each pointer one float off its 16 bytes
            a = [x, x, x, o]
            a[k] = ptr(s.o if k == 3 else s.x, 1)
            assert fn(C.byref(ok), *a, z) == EINVAL, (fn.__name__, "pointer", k)
            a[k] = None
            assert fn(C.byref(ok), *a, z) == EINVAL, (fn.__name__, "NULL", k)
        bad = dict(extra)
        bad.update({"out_ps < Cout": desc(out_ps=28), "Ho != H": desc(Ho=7)})
        for name, d in bad.items():
            assert sup(C.byref(d)) == 0 and macs(C.byref(d)) == 0, (fn.__name__, name)
            assert fn(C.byref(d), x, x, x, o, z) == EINVAL, (fn.__name__, name)
    assert s.untouched()


def _engine_case(winograd4):
    gen = _gen(7105, int(winograd4))
    x = torch.randn(2, 6, 6, 32, generator=gen)
    w = torch.randn(32, 32, 3, 3, generator=gen) / 288 ** 0.5
    bias = torch.randn(32, generator=gen)
    pc = pack_conv(w, bias, 1, 1, DEV, winograd4=winograd4)
    d = ConvDesc(2, 6, 6, 32, 6, 6, 32, 3, 3, 1, 1, 32, 32, 0, pc.Kpad, 1)
    ref, _ = R.conv_ref(d, x.reshape(-1), pc.w, pc.bias, None, torch.zeros(x.numel()))
    return x, pc, d, ref.view(2, 6, 6, 32)


def test_engine_routes_a_misaligned_f4_layer_to_the_direct_kernel():
    """The twin of test_winograd_misaligned_pointers_fall_back_to_the_direct_kernel for an F(4x4)-packed layer: the entry refuses
    the view one float into its buffer, ConvEngine.conv(..., x_off=1) takes conv_igemm_f32_kernel, and the result matches."""
    L = _lib.lib()
    x, pc, d, ref = _engine_case(True)
    flat = torch.full((x.numel() + 8,), NAN, device=DEV)
    flat[1:1 + x.numel()] = x.reshape(-1).to(DEV)
    out = torch.full((2, 6, 6, 32), NAN, device=DEV)
    assert L.hands_conv3x3_winograd4_f32(C.byref(d), ptr(flat, 1), ptr(pc.wino4), ptr(pc.bias), ptr(out), _stream()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    seen = []
    eng = ConvEngine()
    eng.winograd4 = True
    eng.hook = lambda phase, pc_, npix, st, has_res, kernel: seen.append(kernel)
    eng.conv(L, pc, flat, 2, 6, 6, out, True, _stream(), x_off=1)
    torch.cuda.synchronize()
    assert seen == ["conv_igemm_f32_kernel"] * 2
    _close("engine", "f4-misaligned-direct", out.cpu(), ref, 2e-5 * max(1.0, ref.abs().max().item()))


def test_engine_reports_the_executed_macs_of_the_f2_route():
    """ConvEngine.last_wino_macs == hands_conv3x3_winograd_executed_macs (tests/test_gpu_winograd4.py asserts the F(4x4) twin)."""
    L = _lib.lib()
    x, pc, d, ref = _engine_case(False)
    seen = []
    eng = ConvEngine()
    eng.hook = lambda phase, pc_, npix, st, has_res, kernel: seen.append(kernel)
    out = torch.full((2, 6, 6, 32), NAN, device=DEV)
    eng.conv(L, pc, x.to(DEV), 2, 6, 6, out, True, _stream())
    torch.cuda.synchronize()
    assert seen == ["conv_wino_f32_kernel"] * 2
    macs = L.hands_conv3x3_winograd_executed_macs(C.byref(d))
    assert eng.last_wino_macs == macs >= 16 * 2 * 3 * 3 * 32 * 32
    _close("engine", "f2-route", out.cpu(), ref, TOL["f2"] * ref.abs().max().item())
