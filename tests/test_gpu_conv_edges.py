"""Edge-descriptor parity of the implicit-GEMM convolution entry points (csrc/conv_igemm.hip), called through the C ABI with the
descriptor features the models use but tests/test_gpu_parity.py never isolates: pixel strides wider than the channel count,
pointers inside an allocation, a broadcast residual row, a residual that aliases the output, a cropped output map, non-square
kernels on non-square maps, a weight row longer than KH*KW*Cin, every activation in both epilogues.

Every case
  1. writes into an edge_util.Out: sentinel bands on both sides and the sentinel in every gap [Cout, out_pix_stride) must survive;
     the inputs carry NaN in every gap [Cin, in_pix_stride) / [Cout, res_pix_stride) and around the values, so a read outside a
     pixel's channels poisons the result; every pointer sits a non-zero multiple of 4 floats inside its allocation;
  2. equals, BIT FOR BIT, the same entry's launch on contiguous buffers holding the same values, with the full output map, the
     materialised residual, an out-of-place residual and the shortest Kpad (layout cannot change arithmetic; not asserted for
     bf16x3, whose header promises fp32 grade only; a split-K twin keeps the case's Kpad, which sets the slice boundaries);
  3. is compared element by element with the float64 restatement kernel_refs.conv_ref (pinned on the CPU by
     tests/test_kernel_refs.py) under min(2e-5 max(1, max|ref|), (K + 4) 2^-24 A L): the project's per-op tolerance
     (tests/test_gpu_parity.py) and the forward bound of a length-K fp32 sum plus bias, residual, activation and one ulp, with
     A = conv(|x|, |w|) + |bias| + |res| and L the activation's Lipschitz constant (1; 1.13 for GELU).  HANDS_ACC_F64 cases meet
     the condition of test_fp64_accumulation_is_correctly_rounded instead, bf16x3 cases that of test_conv_bf16x3_mode_is_fp32_grade.
No call here hands a launching entry a stride or pointer that breaks the 16-byte contract of include/hands_hip.h.

Features: F1 in_ps = Cin + 16, F2 out_ps = Cout + 8, F3 res_ps = Cout + 12, F4 res_ps = 0 (one row), F5 residual aliases the
output, F6 cropped map (corner / one row / one pixel), F7 KH != KW on H != W, F8 Kpad = K + 16 / + 48, F9 the four activations in
the full-tile and in the general epilogue.  Which entry covers which ("." = the entry does not take the field):

  entry                                   F1 F2 F3 F4 F5 F6 F7 F8 F9   test
  hands_conv2d_nhwc_f32  MODE 0 (any)      x  x  x  x  x  x  x  x  x   test_plain_entry[m0-*], test_patch_halves
                         MODE 2 (1x1)      x  x  x  x  x  x  .  .  x   test_plain_entry[pw-*]   (Kpad > Cin takes MODE 0: F8 there)
                         stem (Cin = 4)    x  x  x  x  x  x  x  x  x   test_plain_entry[stem-*]
    | SUM_BLOCK64 / SUM_BLOCK128 / ACC_F64 / MATH_BF16X3: the m0 / pw feature list again per flag (test_plain_entry[*-b64 ...])
  hands_conv2d_nhwc_splitk_n_f32 S = 2, 3  x  x  x  x  x  x  x  x  x   test_splitk_entries[n-*]  (+ ACC_F64: fp64 partial sums)
  hands_conv2d_nhwc_splitk_fused_f32       x  x  x  x  x  x  x  x  x   test_splitk_entries[fused-*]  (counters back at zero)
  hands_conv2d_nhwc_pre_f32  S = 1, 2      x  x  x  x  x  x  .  .  x   test_pre_entry            (pointwise only: Kpad == Cin)
  hands_conv2d_group_f32  2 and 3 jobs     x  x  x  x  x  x  .  .  x   test_grouped_launch       (= each job's single launch)
  hands_conv1x1_dual_nhwc_f32              x  x  .  .  .  .  .  .  x   test_dual_entry           (+ in2_pix_stride > Cin2, odd H2)
  hands_conv2d_nhwc_streamk_f32            x  x  x  .  .  .  .  .  .   test_stream_k_strided     (a workload-sized SK_CASES shape)
  host checks (HANDS_EINVAL, nothing launched)                         test_rejections
"""
import ctypes as C
import functools

import pytest
import torch

import kernel_refs as R
from edge_util import DEV, EINVAL, SENT, In, Out, Scratch, _close_each, _gen, _stream, gap_mask, strided
from hands_amd import _lib
from hands_amd._lib import ConvDesc, ConvJob, ptr
from hands_amd.packing import pack_conv
from test_gpu_parity import SK_CASES

pytestmark = pytest.mark.gpu

BF16X3, BLOCK128, BLOCK64, ACC64 = 0x100, 0x200, 0x400, 0x800
FLAG = {"f32": 0, "b64": BLOCK64, "b128": BLOCK128, "f64": ACC64, "bf16": BF16X3}
NAN = float("nan")
U = 2.0 ** -24


class Geo:
    """A layer geometry; (Hf, Wf) is the output map it produces."""

    def __init__(self, B, H, W, Cin, Cout, KH=1, KW=1, stride=1, pad=0):
        self.B, self.H, self.W, self.Cin, self.Cout, self.KH, self.KW, self.stride, self.pad = B, H, W, Cin, Cout, KH, KW, stride, pad
        self.Hf, self.Wf = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        self.K = KH * KW * Cin
        self.key = (B, H, W, Cin, Cout, KH, KW, stride, pad)


# the feature sets a case may combine (None = off)
def feat(in_gap=0, out_gap=0, res=None, crop=None, kextra=0):
    """res: None | 'dense' | 'gap' (F3) | 'row' (F4) | 'rowdense' (the row, materialised) | 'alias' (F5); crop: (Ho, Wo) | 'corner' | 'row' | 'pixel'."""
    return dict(in_gap=in_gap, out_gap=out_gap, res=res, crop=crop, kextra=kextra)


FEATS = {
    "contig": feat(),
    "F1": feat(in_gap=16),
    "F2": feat(out_gap=8),
    "F3": feat(res="gap"),
    "F4": feat(res="row"),
    "F5": feat(res="alias"),
    "F6corner": feat(crop="corner"),
    "F6row": feat(crop="row"),
    "F6pixel": feat(crop="pixel"),
    "F8k16": feat(kextra=16),
    "F8k48": feat(kextra=48),
    "F123": feat(in_gap=16, out_gap=8, res="gap"),                      # the HMR head's cam_init / refine GEMMs (HandsLight._forward_tail) without the alias
    "F125": feat(in_gap=16, out_gap=8, res="alias"),                    # the HMR state update (hmr_head.tf_head, HandsLight._forward_tail)
    "F24": feat(out_gap=8, res="row"),                                  # HAMER.forward: decout + the mean parameters
    "F256": feat(out_gap=8, res="alias", crop="row"),                   # vit_b16_trunk: the bottom patch half
    "F1268": feat(in_gap=16, out_gap=8, res="dense", crop="corner", kextra=16),
}


@functools.lru_cache(maxsize=None)
def _values(key, seed):
    """Seeded values of a geometry, shared by every layout of it: x (B, H, W, Cin), w (Cout, Cin, KH, KW), bias, a residual on the
    FULL map, the operand affine of the `pre` entry; the packed weight / bias of hands_amd.packing on the CPU."""
    g = Geo(*key)
    gen = _gen("conv_edges", seed, *key)
    x = torch.randn(g.B, g.H, g.W, g.Cin, generator=gen)
    w = torch.randn(g.Cout, g.Cin, g.KH, g.KW, generator=gen) / g.K ** 0.5
    bias = torch.randn(g.Cout, generator=gen)
    res = torch.randn(g.B, g.Hf, g.Wf, g.Cout, generator=gen)
    pre = (torch.rand(g.Cin, generator=gen) + 0.5, torch.randn(g.Cin, generator=gen) * 0.5)
    pc = pack_conv(w, bias, g.stride, g.pad, "cpu", winograd=False)
    assert (pc.Cin, pc.Cout, pc.Kpad) == (g.Cin, g.Cout, (g.K + 15) // 16 * 16)
    return x, w, bias, res, pre, pc


def _pack_wide(g, w, pc, kextra):
    """[Cout_pad][Kpad + kextra], k = (kh, kw, cin), zero fill: the header's layout written out (hands_amd.packing has no Kpad)."""
    wk = torch.zeros(pc.w.shape[0], pc.Kpad + kextra)
    wk[:g.Cout, :g.K] = w.permute(0, 2, 3, 1).reshape(g.Cout, g.K)
    assert torch.equal(wk[:, :pc.Kpad], pc.w)
    return wk


def _crop(g, crop):
    if crop is None:
        return g.Hf, g.Wf
    return {"corner": (max(1, g.Hf - 2), max(1, g.Wf - 3)), "row": (1, g.Wf), "pixel": (1, 1)}.get(crop, crop)


class Call:
    """One launch of an entry: descriptor, buffers and the prior contents of the output, built from a geometry's values and a
    feature set (or contiguous)."""

    def __init__(self, g, seed, act, f, pre=False):
        x, w, bias, res, prev, pc = _values(g.key, seed)
        self.g, self.f, self.act = g, f, act
        Ho, Wo = _crop(g, f["crop"])
        self.Ho, self.Wo, self.M = Ho, Wo, g.B * Ho * Wo
        in_ps, out_ps = g.Cin + f["in_gap"], g.Cout + f["out_gap"]
        self.x = strided(x.reshape(-1, g.Cin), in_ps, NAN)
        self.w = _pack_wide(g, w, pc, f["kextra"]) if f["kextra"] else pc.w
        self.bias = pc.bias
        self.pre = prev if pre else None
        rv = res[:, :Ho, :Wo].reshape(self.M, g.Cout)
        kind, res_ps = f["res"], 0
        self.res = None                                    # the flat residual buffer as the call sees it (CPU)
        prior = torch.full((self.M, out_ps), NAN)
        if kind == "dense":
            self.res, res_ps = rv.reshape(-1), g.Cout
        elif kind == "rowdense":
            self.res, res_ps = res[0, 0, 0].expand(self.M, g.Cout).reshape(-1).clone(), g.Cout
        elif kind == "gap":
            self.res, res_ps = strided(rv, g.Cout + 12, NAN), g.Cout + 12
        elif kind == "row":
            self.res, res_ps = res[0, 0, 0].clone(), 0
        elif kind == "alias":
            prior[:, :g.Cout], res_ps = rv, out_ps
        prior[:, g.Cout:] = SENT
        self.prior = prior.reshape(-1)
        self.d = ConvDesc(g.B, g.H, g.W, g.Cin, Ho, Wo, g.Cout, g.KH, g.KW, g.stride, g.pad, in_ps, out_ps, res_ps,
                          pc.Kpad + f["kextra"], act)
        # device side
        self.X, self.Wd, self.Bd = In(self.x, 12), In(self.w, 4), In(self.bias, 8)
        self.Rd = In(self.res, 8) if self.res is not None else None
        self.P = (In(prev[0], 4), In(prev[1], 4)) if pre else None
        init = prior.view(self.M, out_ps) if kind == "alias" else None
        self.out = Out(self.M, out_ps, init=init, keep=gap_mask(self.M, out_ps, g.Cout))

    def rp(self):
        return self.out.ptr() if self.f["res"] == "alias" else (self.Rd.ptr() if self.Rd is not None else None)

    def launch(self, entry, S=0):
        L, d, s = _lib.lib(), C.byref(self.d), _stream()
        a = (self.X.ptr(), self.Wd.ptr(), self.Bd.ptr(), self.rp(), self.out.ptr())
        if entry == "plain":
            return L.hands_conv2d_nhwc_f32(d, *a, s)
        n = max(0, L.hands_conv2d_workspace_floats(d, S))
        self.ws = torch.full((4 + n + 64,), NAN, device=DEV)
        wsp = ptr(self.ws, 4)
        if entry == "n":
            return L.hands_conv2d_nhwc_splitk_n_f32(d, *a, S, wsp, n, s)
        if entry == "fused":
            self.ctr = torch.zeros(64, dtype=torch.int32, device=DEV)
            return L.hands_conv2d_nhwc_splitk_fused_f32(d, *a, S, wsp, n, ptr(self.ctr), 64, s)
        if entry == "pre":
            return L.hands_conv2d_nhwc_pre_f32(d, a[0], self.P[0].ptr(), self.P[1].ptr(), *a[1:], S, wsp, n, s)
        raise AssertionError(entry)

    def written(self, body):
        return body.view(self.M, -1)[:, :self.g.Cout].reshape(self.g.B, self.Ho, self.Wo, self.g.Cout)

    def reference(self, round_sum=False):
        """-> (expected, A) of the written elements, (B, Ho, Wo, Cout)."""
        res = self.prior if self.f["res"] == "alias" else self.res
        exp, mag = R.conv_ref(self.d, self.x, self.w, self.bias, res, self.prior, pre=self.pre, round_sum=round_sum)
        return self.written(exp), self.written(mag)


def _bound(ref, mag, K, act):
    """min(2e-5 max(1, max|ref|), (K + 4) 2^-24 A L) per element (module docstring)."""
    lip = 1.13 if (act & 0xff) == 2 else 1.0
    first = 2e-5 * max(1.0, ref.abs().max().item())
    return torch.minimum(torch.full_like(mag, first), (K + 4) * U * mag * lip)


def _check(kernel, name, got, twin, call, flag, got32=None):
    """Assertions 2 and 3 of the module docstring on the written elements `got` (B, Ho, Wo, Cout); `twin` is the contiguous
    full-map launch's output (B, Hf, Wf, Cout)."""
    g = call.g
    assert not torch.isnan(got).any(), (kernel, name, "NaN in the written region")
    corner = twin[:, :call.Ho, :call.Wo]
    if flag == BF16X3:
        ref, mag = call.reference()
        scale = max(1.0, ref.abs().max().item())
        err, err32 = (got.double() - ref).abs().max().item(), (got32.double() - ref).abs().max().item()
        print(f"EDGE|{kernel}|{name}|{err:.3e}|{min(2e-5 * scale, 4 * err32 + 1e-7 * scale):.3e}")
        assert err < 2e-5 * scale and err < 4 * err32 + 1e-7 * scale, (kernel, name, err, err32)
        return
    assert torch.equal(got, corner), (kernel, name, "layout changed the bits", (got - corner).abs().max().item())
    if flag == ACC64:
        ref, _ = call.reference(round_sum=True)
        ref = ref.float()
        mism = (got != ref).float().mean().item()
        err, bnd = (got - ref).abs().max().item(), 2.4e-7 * max(1.0, ref.abs().max().item())
        print(f"EDGE|{kernel}|{name}|{err:.3e}|{bnd:.3e}")
        assert mism < 1e-5 and err <= bnd, (kernel, name, mism, err, bnd)
        return
    ref, mag = call.reference()
    _close_each(kernel, name, got, ref, _bound(ref, mag, g.K, call.act))


def _twin_feat(f, split):
    """Contiguous, full map, the residual out of place (F5) and materialised (F4); the shortest Kpad, except under split-K, whose
    slices are shares of the Kpad / 16 k-steps: there the summation order is a function of (layer, S, Kpad) by the header."""
    return feat(res=None if f["res"] is None else ("rowdense" if f["res"] == "row" else "dense"), kextra=f["kextra"] if split else 0)


def _run(kernel, name, g, seed, act, f, entry, S=0, pre=False):
    """One case: the featured launch, its contiguous twin (same entry, same S), all the assertions."""
    flag = act & ~0xff
    call = Call(g, seed, act, f, pre)
    twin = Call(g, seed, act, _twin_feat(f, S > 1), pre)
    assert call.launch(entry, S) == 0 and twin.launch(entry, S) == 0
    got, tw = call.written(call.out.get()), twin.written(twin.out.get())          # (bands and gaps checked by Out.get)
    got32 = None
    if flag == BF16X3:
        exact = Call(g, seed, act & 0xff, f, pre)
        assert exact.launch(entry, S) == 0
        got32 = exact.written(exact.out.get())
    if entry == "fused":
        assert int(call.ctr.abs().sum().item()) == 0 and int(twin.ctr.abs().sum().item()) == 0, "counters not left at zero"
    _check(kernel, name, got, tw, call, flag, got32)


# ---- geometries: the smallest that reach every tile path (K short: Cin in {16, 32, 48}; 32 takes the 128-byte chunk) -------------
M0 = {                                                      # MODE 0
    "w165c16": Geo(3, 5, 11, 16, 140, 3, 3, 1, 1),          # wide tile: one full + one partial m-tile, one full n-tile + 12 channels
    "w165c32": Geo(3, 5, 11, 32, 140, 3, 3, 1, 1),
    "w165c48": Geo(3, 5, 11, 48, 140, 3, 3, 1, 1),
    "wfull": Geo(4, 8, 8, 32, 128, 3, 3, 1, 1),             # M = 256, Cout = 128: every tile full (epilogue_full)
    "n293c64": Geo(1, 1, 293, 16, 64, 3, 3, 1, 1),          # narrow tile 256 x 64: one full + one partial m-tile
    "n293c20": Geo(1, 1, 293, 32, 20, 3, 3, 1, 1),
    "s2odd": Geo(3, 5, 11, 16, 140, 3, 3, 2, 1),            # stride 2 on an odd map
    "k1x3": Geo(3, 5, 11, 16, 140, 1, 3, 1, 0),             # F7
    "k3x1": Geo(3, 5, 11, 32, 20, 3, 1, 1, 0),
    "k5x3": Geo(3, 5, 11, 48, 140, 5, 3, 1, 1),
}
PW = {                                                      # MODE 2
    "same165": Geo(3, 5, 11, 48, 140),                      # stride 1, H == Ho: the same_pixel path (cropped: the decomposition)
    "samefull": Geo(4, 8, 8, 32, 128),
    "s2odd": Geo(3, 5, 11, 16, 140, 1, 1, 2, 0),            # stride 2 on an odd map
    "n293c64": Geo(293, 1, 1, 48, 64),
    "n293c20": Geo(1, 1, 293, 32, 20),
}
STEM = {                                                    # MODE 1, Cin = 4, on 9 x 11, both tile widths
    "7x7w": Geo(3, 9, 11, 4, 140, 7, 7, 2, 3),
    "7x7n": Geo(3, 9, 11, 4, 64, 7, 7, 2, 3),
    "3x3w": Geo(3, 9, 11, 4, 140, 3, 3, 1, 1),
    "3x3n": Geo(3, 9, 11, 4, 64, 3, 3, 1, 1),
}
ALL_F = ["F1", "F2", "F3", "F4", "F5", "F6corner", "F6row", "F6pixel", "F8k16", "F8k48", "F123", "F125", "F24", "F256", "F1268"]
NO_F8 = [n for n in ALL_F if "8" not in n]


def _plain_cases():
    c = []
    # fp32 chain: every feature on the wide / narrow / full-tile geometry of each mode; the other geometries take the combinations
    for n in ALL_F:
        c.append(("m0", "w165c16", "f32", 1, n))
    for n in ("F125", "F256", "F1268"):
        for gk in ("w165c32", "w165c48", "wfull", "n293c64", "n293c20", "s2odd"):
            c.append(("m0", gk, "f32", 3 if gk == "wfull" else 1, n))
    for gk in ("k1x3", "k3x1", "k5x3"):                                                    # F7
        c += [("m0", gk, "f32", 1, "contig"), ("m0", gk, "f32", 0, "F1268")]
    for n in NO_F8:
        c.append(("pw", "same165", "f32", 1, n))
    for n in ("F125", "F256"):
        for gk in ("samefull", "s2odd", "n293c64", "n293c20"):
            c.append(("pw", gk, "f32", 1, n))
    for gk in STEM:                                                                        # F2 and F6 (and the rest once)
        c += [("stem", gk, "f32", 1, "F2"), ("stem", gk, "f32", 3, "F6corner")]
    for n in ("F1", "F3", "F4", "F5", "F6row", "F6pixel", "F8k16", "F8k48", "F256", "F1268"):
        c.append(("stem", "7x7w", "f32", 1, n))
    # F9: the four activations, full-tile epilogue (with and without a residual) and the general one
    for act in (0, 1, 2, 3):
        c += [("m0", "wfull", "f32", act, "F2"), ("m0", "wfull", "f32", act, "F123"), ("pw", "samefull", "f32", act, "F125"),
              ("m0", "w165c32", "f32", act, "F123"), ("pw", "same165", "f32", act, "F2"), ("stem", "3x3w", "f32", act, "F24")]
    # the other summation forms: the feature list again, singly on one geometry per mode, combined on the others
    for fl in ("b64", "b128", "f64", "bf16"):
        for n in ("F1", "F2", "F3", "F4", "F5", "F6row", "F8k48", "F1268"):
            c.append(("m0", "w165c48", fl, 3, n))
        for n in ("F123", "F24", "F256"):
            c.append(("pw", "same165", fl, 1, n))
        c += [("m0", "wfull", fl, 0, "F125"), ("pw", "samefull", fl, 1, "F125"), ("m0", "n293c20", fl, 1, "F256"), ("pw", "s2odd", fl, 0, "F1")]
    seen, out = set(), []
    for t in c:
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


@pytest.mark.parametrize("mode,gk,fl,act,fname", _plain_cases(), ids=lambda v: str(v))
def test_plain_entry(mode, gk, fl, act, fname):
    """hands_conv2d_nhwc_f32: MODE 0, MODE 2 and the stem; one fp32 chain, 64- and 128-float blocks, fp64 accumulation, bf16x3."""
    g = {"m0": M0, "pw": PW, "stem": STEM}[mode][gk]
    _run("conv2d_nhwc", f"{mode}-{gk}-{fl}-a{act}-{fname}", g, 1, act | FLAG[fl], FEATS[fname], "plain")


def _splitk_cases():
    c = []
    for entry in ("n", "fused"):
        for n in ("F1", "F2", "F3", "F4", "F5", "F6corner", "F6pixel", "F8k16", "F1268"):       # K = 432 = 27 k-steps
            c.append((entry, "m0", "w165c48", "f32", 2, 1, n))
        for n in ("F123", "F24", "F256"):                   # K = 48 = 3 k-steps: one per slice
            c.append((entry, "pw", "same165", "f32", 3, 3, n))
        for n in ("F125", "F24"):
            c += [(entry, "m0", "wfull", "f32", 3, 2, n), (entry, "pw", "n293c64", "f32", 2, 0, n), (entry, "m0", "n293c20", "b64", 2, 1, n),
                  (entry, "m0", "w165c48", "f64", 3, 3, n), (entry, "pw", "n293c64", "f64", 2, 1, n)]
        c += [(entry, "m0", "w165c48", "f64", 2, 0, "F1268"), (entry, "m0", "k5x3", "f32", 3, 1, "F256")]
    return c


@pytest.mark.parametrize("entry,mode,gk,fl,S,act,fname", _splitk_cases(), ids=lambda v: str(v))
def test_splitk_entries(entry, mode, gk, fl, S, act, fname):
    """hands_conv2d_nhwc_splitk_n_f32 (slices + splitk_reduce_kernel / splitk_reduce_f64_kernel) and
    hands_conv2d_nhwc_splitk_fused_f32 (splitk_fused_tail; counters start and end at zero): out, res and partial are indexed
    separately by each of them."""
    g = {"m0": M0, "pw": PW}[mode][gk]
    assert g.K // 16 >= S                                   # really split
    _run(f"conv2d_splitk_{entry}", f"{mode}-{gk}-{fl}-S{S}-a{act}-{fname}", g, 2, act | FLAG[fl], FEATS[fname], entry, S)


@pytest.mark.parametrize("gk,fl,S,act,fname", [(gk, fl, S, act, n) for gk, fl, S, act in (
    ("same165", "f32", 1, 3), ("same165", "f32", 2, 1), ("samefull", "b64", 1, 2), ("n293c64", "f32", 2, 0), ("s2odd", "f32", 1, 3),
    ("same165", "f64", 1, 3), ("n293c20", "f64", 2, 1)) for n in (NO_F8 if gk == "same165" and fl == "f32" and S == 1 else ("F125", "F24"))],
    ids=lambda v: str(v))
def test_pre_entry(gk, fl, S, act, fname):
    """hands_conv2d_nhwc_pre_f32, S = 1 and S = 2: the operand is leaky_relu(x * scale + shift) on its way into LDS."""
    g = PW[gk]
    if S > 1:
        assert g.K // 16 >= S
    _run("conv2d_pre", f"{gk}-{fl}-S{S}-a{act}-{fname}", g, 3, act | FLAG[fl], FEATS[fname], "pre", S, pre=True)


def test_patch_halves():
    """The 8 x 16 / stride 16 patch halves of vit_b16_trunk (the widened conv_proj) scaled down to 2 x 4 / stride 4 on 4-row strips:
    the top half writes the (1, G) row, the bottom half -- input pointer two rows further, residual = the output in place -- adds
    its half.  Together they are the 4 x 4 / stride 4 patch embedding; each launch meets its own bound."""
    L, B, G, Cin, Cout = _lib.lib(), 6, 5, 16, 140
    gen = _gen("patch_halves")
    x = torch.randn(B, 4, 4 * G, Cin, generator=gen)
    w = torch.randn(Cout, Cin, 4, 4, generator=gen) / (16 * Cin) ** 0.5
    bias = torch.randn(Cout, generator=gen)
    top = pack_conv(w[:, :, :2].contiguous(), bias, 4, 0, "cpu", winograd=False)
    bot = pack_conv(w[:, :, 2:].contiguous(), torch.zeros(Cout), 4, 0, "cpu", winograd=False)
    in_ps, out_ps, M = Cin + 16, Cout + 8, B * G
    xs = torch.cat([strided(x.reshape(-1, Cin), in_ps, NAN), torch.full((2 * 4 * G * in_ps,), NAN)])   # the bottom half's nominal extent
    X = In(xs, 12)
    out = Out(M, out_ps, keep=gap_mask(M, out_ps, Cout))
    prior = strided(torch.full((M, Cout), NAN), out_ps, SENT)
    d0 = ConvDesc(B, 4, 4 * G, Cin, 1, G, Cout, 2, 4, 4, 0, in_ps, out_ps, 0, top.Kpad, 0)
    d1 = ConvDesc(B, 4, 4 * G, Cin, 1, G, Cout, 2, 4, 4, 0, in_ps, out_ps, out_ps, bot.Kpad, 0)
    W0, B0, W1, B1 = In(top.w, 4), In(top.bias, 4), In(bot.w, 4), In(bot.bias, 4)
    assert L.hands_conv2d_nhwc_f32(C.byref(d0), X.ptr(), W0.ptr(), B0.ptr(), None, out.ptr(), _stream()) == 0
    mid = out.get().clone().reshape(-1)
    e0, a0 = R.conv_ref(d0, xs, top.w, top.bias, None, prior)
    sel = ~gap_mask(M, out_ps, Cout).reshape(-1)
    _close_each("conv2d_nhwc", "patch-top", mid[sel], e0[sel], _bound(e0[sel], a0[sel], 8 * Cin, 0))
    off = 2 * 4 * G * in_ps
    assert L.hands_conv2d_nhwc_f32(C.byref(d1), X.ptr(off), W1.ptr(), B1.ptr(), out.ptr(), out.ptr(), _stream()) == 0
    got = out.get().reshape(-1)
    e1, a1 = R.conv_ref(d1, xs[off:], bot.w, bot.bias, mid, mid)
    _close_each("conv2d_nhwc", "patch-bottom", got[sel], e1[sel], _bound(e1[sel], a1[sel], 8 * Cin, 0))
    full = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), bias.double(), stride=4)      # (B, Cout, 1, G)
    err = (got.view(M, out_ps)[:, :Cout].double() - full.permute(0, 2, 3, 1).reshape(M, Cout)).abs().max().item()
    print(f"EDGE|conv2d_nhwc|patch-both|{err:.3e}|{2e-5 * max(1.0, full.abs().max().item()):.3e}")
    assert err <= 2e-5 * max(1.0, full.abs().max().item())


GROUPS = {
    # jobs of one kernel class: (geometry key in PW, act, feature)
    "wide3": ("f32", False, [("same165", 1, "F123"), ("samefull", 0, "F125"), ("s2odd", 3, "F256")]),
    "wide2": ("f32", False, [("s2odd", 2, "F24"), ("same165", 1, "F6corner")]),
    "narrow2": ("f32", False, [("n293c64", 1, "F125"), ("n293c20", 2, "F24")]),
    "narrow3b64": ("b64", False, [("n293c20", 3, "F123"), ("n293c64", 0, "F6pixel"), ("n293c20", 1, "contig")]),
    "pre2": ("f32", True, [("same165", 3, "F125"), ("samefull", 1, "F123")]),
}


@pytest.mark.parametrize("name", sorted(GROUPS))
def test_grouped_launch(name):
    """hands_conv2d_group_f32: two and three jobs of different M and different strides in one launch; every job has its own
    bands, equals its own single launch bit for bit, and meets the per-element bound."""
    L = _lib.lib()
    fl, pre, jobs = GROUPS[name]
    calls = [Call(PW[gk], 10 + i, act | FLAG[fl], FEATS[fn], pre) for i, (gk, act, fn) in enumerate(jobs)]
    single = [Call(PW[gk], 10 + i, act | FLAG[fl], FEATS[fn], pre) for i, (gk, act, fn) in enumerate(jobs)]
    arr = (ConvJob * len(calls))()
    for i, c in enumerate(calls):
        assert L.hands_conv2d_group_class(C.byref(c.d), int(pre)) == L.hands_conv2d_group_class(C.byref(calls[0].d), int(pre)) >= 0
        arr[i] = ConvJob(C.pointer(c.d), c.X.ptr(), c.Wd.ptr(), c.Bd.ptr(), c.rp(), c.out.ptr(), c.P[0].ptr() if pre else None,
                         c.P[1].ptr() if pre else None)
    assert L.hands_conv2d_group_f32(arr, len(calls), _stream()) == 0
    for i, (c, s) in enumerate(zip(calls, single)):
        assert s.launch("pre" if pre else "plain", 1) == 0
        got, one = c.written(c.out.get()), s.written(s.out.get())
        assert not torch.isnan(got).any() and torch.equal(got, one), (name, i)
        ref, mag = c.reference()
        _close_each("conv2d_group", f"{name}-job{i}", got, ref, _bound(ref, mag, c.g.K, c.act))


DUAL_CASES = [
    # B, Ho, Wo, K0, Cin2, Cout, stride2, H2, W2, in_gap, in2_gap, out_gap, act, flag
    (3, 5, 11, 16, 32, 140, 2, 9, 21, 16, 8, 8, 1, "f32"),       # odd H2 / W2: (Ho - 1) * 2 < H2
    (3, 5, 11, 48, 16, 140, 2, 10, 22, 0, 8, 0, 3, "f32"),       # in2_pix_stride > Cin2 alone
    (4, 8, 8, 32, 16, 128, 1, 8, 8, 16, 0, 8, 1, "f32"),         # stride2 = 1, every tile full
    (4, 8, 8, 16, 48, 128, 2, 15, 16, 16, 4, 8, 2, "f32"),       # full tiles, GELU
    (1, 1, 293, 16, 16, 64, 2, 1, 585, 16, 12, 8, 0, "f32"),     # narrow tile
    (1, 1, 293, 32, 32, 20, 1, 2, 293, 0, 8, 8, 1, "f32"),       # narrow tile, larger second map
    (3, 5, 11, 16, 32, 140, 2, 9, 21, 16, 8, 8, 1, "b64"),       # the block flags are ignored here: the one chain's bits
    (3, 5, 11, 16, 32, 140, 2, 9, 21, 16, 8, 8, 1, "bf16"),
]


@pytest.mark.parametrize("case", DUAL_CASES, ids=lambda v: "-".join(str(t) for t in v))
def test_dual_entry(case):
    """hands_conv1x1_dual_nhwc_f32: act(W0 x + W1 x2[::stride2] + bias) with every stride wider than its channels."""
    B, Ho, Wo, K0, C2, Cout, s2, H2, W2, ig, ig2, og, act, fl = case
    L, M = _lib.lib(), B * Ho * Wo
    gen = _gen("dual", *case[:-1])
    x, x2 = torch.randn(M, K0, generator=gen), torch.randn(B * H2 * W2, C2, generator=gen)
    w = torch.cat([torch.randn(Cout, K0, 1, 1, generator=gen) / K0 ** 0.5, torch.randn(Cout, C2, 1, 1, generator=gen) / C2 ** 0.5], 1)
    pc = pack_conv(w, torch.randn(Cout, generator=gen), 1, 0, "cpu", winograd=False)
    Wd, Bd = In(pc.w, 4), In(pc.bias, 8)

    def run(ig, ig2, og, flag):
        d = ConvDesc(B, Ho, Wo, K0, Ho, Wo, Cout, 1, 1, 1, 0, K0 + ig, Cout + og, 0, K0 + C2, act | flag)
        xs, x2s = strided(x, K0 + ig, NAN), strided(x2, C2 + ig2, NAN)
        X, X2 = In(xs, 12), In(x2s, 16)
        out = Out(M, Cout + og, keep=gap_mask(M, Cout + og, Cout))
        assert L.hands_conv1x1_dual_nhwc_f32(C.byref(d), X.ptr(), X2.ptr(), C2, H2, W2, s2, C2 + ig2, Wd.ptr(), Bd.ptr(), out.ptr(),
                                             _stream()) == 0
        got = out.get().view(M, Cout + og)[:, :Cout]
        prior = strided(torch.full((M, Cout), NAN), Cout + og, SENT)
        exp, mag = R.conv_ref(d, xs, pc.w, pc.bias, None, prior, dual=(x2s, C2, H2, W2, s2, C2 + ig2))
        return got, exp.view(M, -1)[:, :Cout], mag.view(M, -1)[:, :Cout]

    got, ref, mag = run(ig, ig2, og, FLAG[fl])
    twin, _, _ = run(0, 0, 0, 0)                                 # contiguous, one fp32 chain
    name = "-".join(str(t) for t in case)
    assert not torch.isnan(got).any()
    if fl == "bf16":
        scale = max(1.0, ref.abs().max().item())
        err, err32 = (got.double() - ref).abs().max().item(), (twin.double() - ref).abs().max().item()
        print(f"EDGE|conv1x1_dual|{name}|{err:.3e}|{min(2e-5 * scale, 4 * err32 + 1e-7 * scale):.3e}")
        assert err < 2e-5 * scale and err < 4 * err32 + 1e-7 * scale
        return
    assert torch.equal(got, twin), (name, "layout changed the bits")
    _close_each("conv1x1_dual", name, got, ref, _bound(ref, mag, K0 + C2, act))


@pytest.mark.parametrize("case", [SK_CASES[8]], ids=["sk8"])
def test_stream_k_strided(case):
    """hands_conv2d_nhwc_streamk_f32 with F1 + F2 + F3 on a shape of tests/test_gpu_parity.py's SK_CASES inside the stream-K
    window (the route does not exist below workload size): bands and gaps, the bits of the contiguous stream-K launch and of the
    plain launch on the same strided buffers, every element against the restatement."""
    B, Cin, H, Cout, k, stride, pad, use_res = case
    assert use_res and k == 1
    L = _lib.lib()
    g = Geo(B, H, H, Cin, Cout, k, k, stride, pad)
    f = FEATS["F123"]
    call, twin, plain = Call(g, 4, 1, f), Call(g, 4, 1, feat(res="dense")), Call(g, 4, 1, f)
    for c in (call, twin):
        G = L.hands_conv2d_streamk_grid(C.byref(c.d))
        assert G > 0, "not a stream-K launch: the case proves nothing"
        ws = torch.zeros(L.hands_conv2d_streamk_workspace_bytes() // 4 + 4, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        assert L.hands_conv2d_nhwc_streamk_f32(C.byref(c.d), c.X.ptr(), c.Wd.ptr(), c.Bd.ptr(), c.rp(), c.out.ptr(), ptr(ws, 4),
                                               (ws.numel() - 4) * 4, 1, _stream()) == 0
        torch.cuda.synchronize()
    assert plain.launch("plain") == 0
    got, tw, pl = call.written(call.out.get()), twin.written(twin.out.get()), plain.written(plain.out.get())
    assert torch.equal(got, pl), "stream-K differs from the plain launch on strided buffers"
    _check("conv2d_streamk", "sk8-F123", got, tw, call, 0)


def test_rejections():
    """Every host check of the convolution entries: HANDS_EINVAL, nothing launched, the sentinel buffers untouched."""
    L, s, z = _lib.lib(), Scratch(), _stream()
    x, o, o2 = ptr(s.x), ptr(s.o), ptr(s.o2)

    def desc(B=2, H=4, W=4, Cin=16, Ho=None, Wo=None, Cout=8, KH=1, KW=1, stride=1, pad=0, in_ps=None, out_ps=None, res_ps=0, Kpad=None, act=0):
        Hf, Wf = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
        return ConvDesc(B, H, W, Cin, Ho or Hf, Wo or Wf, Cout, KH, KW, stride, pad, in_ps or Cin, out_ps or Cout, res_ps,
                        Kpad or (KH * KW * Cin + 15) // 16 * 16, act)

    def plain(d, res=None):
        return L.hands_conv2d_nhwc_f32(C.byref(d), x, x, x, res, o, z)

    assert L.hands_conv2d_group_class(C.byref(desc()), 0) >= 0            # the base descriptor itself is a valid one
    bad = {
        "out_ps < Cout": desc(out_ps=4),
        "in_ps < Cin": desc(in_ps=12),
        "Ho + 1": desc(Ho=5),
        "Wo + 1": desc(Wo=5),
        "Ho + 1 padded": desc(KH=3, KW=3, pad=1, Ho=5),
        "Kpad < K": desc(KH=3, KW=3, pad=1, Kpad=128),
        "Kpad % 16": desc(Kpad=24),
        "Cin = 12": desc(Cin=12, Kpad=16),
        "in_ps % 4": desc(in_ps=18),
        "out_ps % 4": desc(out_ps=10),
        "Cout % 4": desc(Cout=6, out_ps=8),
        "act code": desc(act=4),
        "fp64 + bf16x3": desc(act=ACC64 | BF16X3),
        "fp64 stem": desc(Cin=4, KH=3, KW=3, pad=1, act=ACC64),
        "KH = 16 padded": desc(H=16, W=16, KH=16, KW=3, pad=1),
    }
    for name, d in bad.items():
        assert plain(d) == EINVAL, name
        assert L.hands_conv2d_nhwc_splitk_n_f32(C.byref(d), x, x, x, None, o, 2, o2, 1 << 16, z) == EINVAL, name
        assert L.hands_conv2d_nhwc_streamk_f32(C.byref(d), x, x, x, None, o, o2, 1 << 18, 1, z) == EINVAL, name
        assert L.hands_conv2d_group_class(C.byref(d), 0) == -1, name
        assert L.hands_conv2d_workspace_floats(C.byref(d), 2) == -1, name
    # the residual's stride counts only when there is a residual
    assert plain(desc(res_ps=10), res=x) == EINVAL and plain(desc(res_ps=-8), res=x) == EINVAL
    assert L.hands_conv2d_nhwc_splitk_fused_f32(C.byref(desc(Cin=64, res_ps=10)), x, x, x, x, o, 2, o2, 1 << 16, x, 64, z) == EINVAL
    # pre: a non-pointwise descriptor, bf16x3, a missing shift
    pre = lambda d, sc=x, sh=x, S=1: L.hands_conv2d_nhwc_pre_f32(C.byref(d), x, sc, sh, x, x, None, o, S, o2, 1 << 16, z)
    assert pre(desc(KH=3, KW=3, pad=1)) == EINVAL and pre(desc(act=BF16X3)) == EINVAL and pre(desc(), sh=None) == EINVAL
    assert pre(desc(Kpad=32)) == EINVAL and pre(desc(Cin=64), S=2, sc=None) == EINVAL
    # dual: (Ho - 1) * stride2 >= H2, Kpad != Cin + Cin2, fp64, strides
    dd = lambda **kw: desc(Kpad=32, **kw)
    dual = lambda d, Cin2=16, H2=7, W2=7, s2=2, ps2=16: L.hands_conv1x1_dual_nhwc_f32(C.byref(d), x, x, Cin2, H2, W2, s2, ps2, x, x, o, z)
    assert dual(dd(), H2=6) == EINVAL and dual(dd(), W2=6) == EINVAL
    assert dual(desc(Kpad=48)) == EINVAL and dual(dd(act=ACC64)) == EINVAL
    assert dual(dd(), ps2=12) == EINVAL and dual(dd(), ps2=18) == EINVAL and dual(dd(in_ps=18)) == EINVAL and dual(dd(out_ps=10)) == EINVAL
    assert dual(dd(out_ps=4)) == EINVAL and dual(dd(in_ps=12)) == EINVAL and dual(dd(), Cin2=12) == EINVAL and dual(dd(), s2=0) == EINVAL
    assert dual(dd(stride=2, Ho=4, Wo=4)) == EINVAL and dual(dd(Ho=3)) == EINVAL
    # group: two classes in one launch, n = 9, n = 0, a job that is not pointwise, a residual stride
    wide, narrow, conv3 = desc(Cout=128), desc(Cout=8), desc(KH=3, KW=3, pad=1)
    job = lambda d, res=None, out=o: ConvJob(C.pointer(d), x, x, x, res, out, None, None)
    grp = lambda *jobs, n=None: L.hands_conv2d_group_f32((ConvJob * max(1, len(jobs)))(*jobs), len(jobs) if n is None else n, z)
    assert L.hands_conv2d_group_class(C.byref(wide), 0) != L.hands_conv2d_group_class(C.byref(narrow), 0)
    assert grp(job(wide), job(narrow, out=o2)) == EINVAL
    assert grp(*[job(narrow)] * 9) == EINVAL and grp(job(narrow), n=0) == EINVAL
    b128, r10 = desc(act=BLOCK128), desc(res_ps=10)
    assert grp(job(conv3)) == EINVAL and grp(job(b128)) == EINVAL and grp(job(r10, res=x)) == EINVAL
    assert grp(ConvJob(C.pointer(narrow), x, x, x, None, o, x, None)) == EINVAL        # pre_scale without pre_shift
    assert s.untouched()
