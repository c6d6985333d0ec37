"""What the edge-shape GPU tests (test_gpu_kernel_edges.py, test_gpu_io_edges.py, test_gpu_conv_edges.py,
test_gpu_raster_edges.py, test_gpu_mano_edges.py, test_gpu_loss_edges.py, test_gpu_wino_stem_edges.py) share: guarded output buffers,
strided and offset inputs, seeded values and the comparisons that print `EDGE|kernel|case|error|bound` before they assert.  A plain
module, imported by all seven."""
import math

import torch

import kernel_refs as R
from hands_amd._lib import ptr

DEV = "cuda"
EINVAL = 10001
SENT = -7777.25       # exactly representable; no kernel here produces it
BAND = 256            # floats of sentinel on either side of an output


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k * 1000) if isinstance(k, float) else k for k in key)) % (2 ** 31))


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


class Out:
    """A device output of `shape` inside a buffer with a sentinel band on both sides.  The body starts as NaN (or as `init`, for
    an in-place kernel, or with the sentinel where `keep` is True: padding the kernel must not touch)."""

    def __init__(self, *shape, init=None, keep=None):
        self.shape, self.n = shape, math.prod(shape)
        self.buf = torch.full((2 * BAND + self.n,), SENT, device=DEV)
        body = self.buf[BAND:BAND + self.n].view(shape)
        if init is not None:
            body.copy_(init)
        else:
            body.fill_(float("nan"))
        self.keep = keep
        if keep is not None:
            body[keep.to(DEV).expand(shape)] = SENT

    def ptr(self):
        return ptr(self.buf, BAND)

    def get(self):
        """-> the body on the CPU, after checking the bands and the kept padding."""
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert torch.all(h[:BAND] == SENT), "wrote in front of the output"
        assert torch.all(h[BAND + self.n:] == SENT), "wrote behind the output"
        body = h[BAND:BAND + self.n].view(self.shape)
        if self.keep is not None:
            assert torch.all(body[self.keep.expand(self.shape)] == SENT), "wrote into padding"
        return body


class OutInt:
    """Out's counterpart for an int32 or uint8 output: sentinel bands of BAND elements on both sides, the body preset to a
    second value (`unwritten`) that no kernel here produces for int32 (indices are >= -1); for uint8 every value is a legitimate
    result, so an unwritten element shows only through the caller's comparison with the expected picture."""
    SENT = {torch.int32: -77777, torch.uint8: 0xA5}
    UNWRITTEN = {torch.int32: -99999, torch.uint8: 0x5A}

    def __init__(self, dtype, *shape):
        self.shape, self.n, self.dtype = shape, math.prod(shape), dtype
        self.sent, self.unwritten = self.SENT[dtype], self.UNWRITTEN[dtype]
        self.buf = torch.full((2 * BAND + self.n,), self.sent, dtype=dtype, device=DEV)
        self.buf[BAND:BAND + self.n] = self.unwritten

    def ptr(self):
        return ptr(self.buf, BAND)

    def get(self):
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert torch.all(h[:BAND] == self.sent), "wrote in front of the output"
        assert torch.all(h[BAND + self.n:] == self.sent), "wrote behind the output"
        body = h[BAND:BAND + self.n].view(self.shape)
        if self.dtype == torch.int32:
            assert not torch.any(body == self.unwritten), "an element was left unwritten"
        return body


def strided(vals, ps, fill):
    """vals (M, C) -> the flat CPU buffer of M pixels `ps` floats apart, every gap [C, ps) holding `fill` (the last pixel's too)."""
    M, C = vals.shape
    assert ps >= C
    buf = torch.full((M, ps), float(fill), dtype=vals.dtype)
    buf[:, :C] = vals
    return buf.reshape(-1)


class In:
    """A device input whose pointer sits `lead` floats (a non-zero multiple of 4) inside its allocation, NaN in front of and
    behind the values: a kernel that reads outside them poisons its result."""

    def __init__(self, flat, lead=8, tail=64):
        assert lead > 0 and lead % 4 == 0
        flat = flat.reshape(-1)
        self.lead, self.n = lead, flat.numel()
        h = torch.full((lead + self.n + tail,), float("nan"), dtype=flat.dtype)
        h[lead:lead + self.n] = flat
        self.buf = h.to(DEV)

    def ptr(self, off=0):
        return ptr(self.buf, self.lead + off)


def gap_mask(M, ps, C):
    """keep-mask of an Out(M, ps): True in the gap [C, ps) of every pixel."""
    return (torch.arange(ps) >= C).view(1, ps).expand(M, ps)


def _close(kernel, case, got, ref, bound):
    assert got.dtype == torch.float32 and got.shape == ref.shape, (kernel, case, got.shape, ref.shape)
    assert not torch.isnan(got).any(), (kernel, case, "NaN left in the written region")
    err = (got.double() - ref.double()).abs().max().item()
    print(f"EDGE|{kernel}|{case}|{err:.3e}|{bound:.3e}")
    assert err <= bound, (kernel, case, err, bound)


def _exact(kernel, case, got, expr32, ref):
    """Bit-equal to the float32 torch expression, which itself sits within float32 rounding of the float64 restatement: at most
    three additions, each rounded by half an ulp (2^-24 relative) of an intermediate no larger than twice the largest result."""
    assert expr32.dtype == torch.float32
    _close(kernel, case, got, ref, 6 * 2.0 ** -24 * max(1.0, ref.abs().max().item()))
    assert torch.equal(got, expr32.view(got.shape)), (kernel, case)


def _rule(existing, ref, fn, *args):
    """max(existing bound, 4 x the error of ATen's float32 evaluation of the restatement `fn` against `ref`)."""
    with R.precision(torch.float32):
        f32 = fn(*args)
    assert f32.dtype == torch.float32
    e32 = (f32.double() - ref).abs().max().item()
    return max(existing, 4 * e32), e32


def _close_each(kernel, case, got, ref, bound):
    """As _close with a bound per element (a tensor of ref's shape); NaN only, and exactly, where the reference has it.  Prints
    the element with the narrowest margin."""
    assert got.dtype == torch.float32 and got.shape == ref.shape == bound.shape, (kernel, case, got.shape, ref.shape)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (kernel, case, "NaN positions differ")
    err = torch.where(nan, torch.zeros_like(ref, dtype=torch.float64), (got.double() - ref.double()).abs())
    bnd = torch.where(nan, torch.ones_like(err), bound.double())
    i = (err / bnd).argmax() if err.numel() else 0
    print(f"EDGE|{kernel}|{case}|{err.flatten()[i].item():.3e}|{bnd.flatten()[i].item():.3e}")
    assert torch.all(err <= bnd), (kernel, case, err.flatten()[i].item(), bnd.flatten()[i].item())


class Scratch:
    """Buffers for a rejection test: an input of zeros and two sentinel-filled outputs no rejected call may touch."""

    def __init__(self):
        self.x = torch.zeros(1 << 16, device=DEV)
        self.o = torch.full((1 << 16,), SENT, device=DEV)
        self.o2 = torch.full((1 << 16,), SENT, device=DEV)

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.all(self.o == SENT)) and bool(torch.all(self.o2 == SENT))
