"""Edge cases of the kernels at the two ends of the pipeline -- csrc/metrics.hip (evaluation metrics, GT targets, 2-D
de-normalisation) and csrc/frontend.hip (hand boxes, the cubic warp, the per-pixel angle maps) -- through the C ABI, every output
element against tests/kernel_refs.py (metrics) or oracle/frontend_oracle.py (front-end).  Conventions as in
tests/test_gpu_kernel_edges.py: outputs inside guarded buffers, `EDGE|kernel|case|error|bound` printed before each assert.

The model-shape tests of these kernels use one batch of 24 (metrics), 224 x 224 images with img_res == out_res and axis-aligned
affines the box kernel made itself (front-end).  Here: batch sizes around the 64-thread block, every validity combination, hands
whose Procrustes cross-covariance has rank 0, 1 or 2 or equal singular values, general and singular affines, sources smaller than
the 4 x 4 cubic footprint, coordinates that saturate the fixed-point conversion, boxes on every edge of the image, img_res !=
out_res.

Bounds.  eval_metrics: per element max(4 x the float32 evaluation's error of the same output in the same launch, 4 x
spacing(float32(ref))) -- the second term is the three float32 roundings of (float)(s / 21) * valid * 1000 -- and never more than
the model-shape test's rtol 2e-5 + atol 5e-4 (mm / px); NaN exactly where the restatement has it.  gt_targets: the wrapper test's
rtol 2e-6 (2e-5 for the weak-perspective scale) + atol 2e-6, or 4 x the float32 evaluation's error if that is larger; pure
subtractions, unnormalize_kp2d, boxes, masks and the offset / coordinate maps are bit-equal.  warp: 2e-6, as
test_gpu_frontend_matches_oracle; angles 1 spacing (float64 atan2 rounded once) or 4 (float32 atan2f), affines 1 spacing."""
import ctypes as C

import numpy as np
import pytest
import torch

import kernel_refs as R
from edge_util import BAND, DEV, EINVAL, Out, Scratch, _close, _close_each, _dev, _exact, _gen, _stream
from hands_amd import _lib
from hands_amd._lib import EvalIn, EvalOut, check, ptr
from oracle import frontend_oracle as FO

pytestmark = pytest.mark.gpu
POISON = 3.0e38       # body of an output in which NaN is a legitimate result: an element left unwritten shows as an error
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ================================================================================================================================
# A. csrc/metrics.hip
# ================================================================================================================================
EVAL_KEYS = ("mpjpe/ra/h", "mpjpe/pa/ra/r", "mpjpe/pa/ra/l", "mpjpe/pa/ra/h", "mrrpe/r/l", "pix_err/r", "pix_err/l")


def _hands(B, g, noise=0.01):
    """The 13 members of hands_eval_in for B random two-hand samples: pred = gt + noise, pixels in [0, 224), every flag 1."""
    gr, gl = (0.1 * torch.randn(B, 21, 3, generator=g) + torch.tensor([0.1, -0.05, 0.8]) for _ in range(2))
    pr, pl = gr + noise * torch.randn(B, 21, 3, generator=g), gl + noise * torch.randn(B, 21, 3, generator=g)
    g2r, g2l = 224 * torch.rand(B, 21, 2, generator=g), 224 * torch.rand(B, 21, 2, generator=g)
    p2r, p2l = g2r + 3 * torch.randn(B, 21, 2, generator=g), g2l + 3 * torch.randn(B, 21, 2, generator=g)
    return [pr, pl, gr, gl, p2r, p2l, g2r, g2l, torch.ones(B), torch.ones(B), torch.ones(B), torch.ones(B, 21), torch.ones(B, 21)]


def _one_hand(gt, pr):
    """Rows with one crafted right hand each (B, 21, 3); the left hand is a copy of it, 2-D joints zero, every flag 1."""
    B = gt.shape[0]
    z = torch.zeros(B, 21, 2)
    return [pr, pr.clone(), gt, gt.clone(), z, z, z, z, torch.ones(B), torch.ones(B), torch.ones(B), torch.ones(B, 21), torch.ones(B, 21)]


def _run_eval(ins, B):
    L = _lib.lib()
    d = _dev(*[t.float() for t in ins])
    outs = [Out(B, init=torch.full((B,), POISON)) for _ in range(5)] + [Out(B, 21, init=torch.full((B, 21), POISON)) for _ in range(2)]
    ein, eout = EvalIn(*[ptr(t) for t in d]), EvalOut(*[o.ptr() for o in outs])
    check(L.hands_eval_metrics_f32(C.byref(ein), C.byref(eout), B, _stream()), "eval_metrics")
    return [o.get() for o in outs]


def _eval_bounds(ins, B):
    """-> [(ref, bound)] per output of hands_eval_out, as the module docstring states the bound."""
    ref = R.eval_metrics(*ins, B)
    with R.precision(torch.float32):
        f32 = R.eval_metrics(*ins, B)
    out = []
    for r, f in zip(ref, f32):
        assert f.dtype == torch.float32
        e = torch.nan_to_num((f.double() - r).abs(), nan=0.0, posinf=0.0)
        e32 = e.max().item() if e.numel() else 0.0
        spacing = torch.from_numpy(np.spacing(np.abs(torch.nan_to_num(r).float().numpy()))).double()
        cap = 2e-5 * torch.nan_to_num(r).abs() + 5e-4
        out.append((r, torch.minimum(torch.maximum(torch.full_like(r, 4 * e32), 4 * spacing), cap)))
    return out


def _check_eval(case, ins, B):
    got = _run_eval(ins, B)
    for k, g, (ref, bound) in zip(EVAL_KEYS, got, _eval_bounds(ins, B)):
        _close_each(f"eval_metrics {k}", case, g, ref, bound)
    return got


@pytest.fixture(scope="module")
def batch130():
    g = _gen(101)
    ins = _hands(130, g)
    for i in (8, 9, 10):                                          # a realistic mix of flags
        ins[i] = (torch.rand(130, generator=g) > 0.25).float()
    ins[11], ins[12] = ((torch.rand(130, 21, generator=g) > 0.2).float() for _ in range(2))
    return ins


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_eval_metrics_batch_sizes(batch130, B):
    """One thread, a full block of 64, a block and one thread, three blocks with a ragged tail."""
    _check_eval(f"B={B}", [t[130 - B:].contiguous() for t in batch130], B)


def test_eval_metrics_rows_do_not_depend_on_the_batch(batch130):
    big = _run_eval(batch130, 130)
    for row in (0, 64, 129):
        one = _run_eval([t[row:row + 1].contiguous() for t in batch130], 1)
        for k, a, b in zip(EVAL_KEYS, big, one):
            assert torch.equal(a[row:row + 1].view(torch.int32), b.view(torch.int32)), (k, row)
    print("EDGE|eval_metrics|rows 0, 64, 129 of B=130 against B=1|0.000e+00|0.000e+00")


def test_eval_metrics_validity_table():
    """All eight (is_valid, right_valid, left_valid) x joints_valid with no joint, every joint, only joint 20: 24 rows."""
    ins = _hands(24, _gen(102))
    combos = [(i, r, l) for i in (0, 1) for r in (0, 1) for l in (0, 1)]
    for row in range(24):
        (i, r, l), pat = combos[row % 8], row // 8
        ins[8][row], ins[9][row], ins[10][row] = float(i), float(r), float(l)
        jv = torch.zeros(21) if pat == 0 else torch.ones(21) if pat == 1 else torch.eye(21)[20]
        ins[11][row], ins[12][row] = jv, jv.flip(0) if pat == 2 else jv
    got = dict(zip(EVAL_KEYS, _check_eval("validity table", ins, 24)))
    for row in range(24):
        (i, r, l), pat = combos[row % 8], row // 8
        rv, lv = i * r, i * l
        assert torch.isnan(got["mpjpe/ra/h"][row]) == (rv + lv == 0) and torch.isnan(got["mrrpe/r/l"][row]) == (rv * lv == 0)
        assert (got["mpjpe/pa/ra/r"][row] == 0) == (rv == 0) and (got["mpjpe/pa/ra/l"][row] == 0) == (lv == 0)
        assert not torch.isnan(got["mpjpe/pa/ra/h"][row])
        for k, jv, v in (("pix_err/r", ins[11][row], rv), ("pix_err/l", ins[12][row], lv)):
            assert torch.equal(~torch.isnan(got[k][row]), (jv * v) != 0), (k, row)


def test_eval_metrics_garbage_in_invalid_hands():
    """Invalid hands holding 1e3-sized finite values (NaN is left out: np.linalg.svd raises on it, the reference defines nothing
    there): 0 in mpjpe/pa/ra/{r,l}, NaN in mpjpe/ra/h only with both hands invalid, and the other hand's numbers bit-equal to a
    launch in which the invalid hand holds ordinary joints."""
    g = _gen(103)
    clean = _hands(4, g)
    clean[9], clean[10] = torch.tensor([0.0, 1.0, 0.0, 1.0]), torch.tensor([1.0, 0.0, 0.0, 1.0])
    dirty = [t.clone() for t in clean]
    for row, (rv, lv) in enumerate(zip(clean[9].tolist(), clean[10].tolist())):
        for flag, idx in ((rv, (0, 2, 4, 6)), (lv, (1, 3, 5, 7))):
            if not flag:
                for i in idx:
                    dirty[i][row] = 1e3 * torch.randn(dirty[i][row].shape, generator=g)
    got = dict(zip(EVAL_KEYS, _check_eval("garbage in invalid hands", dirty, 4)))
    base = dict(zip(EVAL_KEYS, _run_eval(clean, 4)))
    assert got["mpjpe/pa/ra/r"][[0, 2]].tolist() == [0.0, 0.0] and got["mpjpe/pa/ra/l"][[1, 2]].tolist() == [0.0, 0.0]
    assert torch.isnan(got["mpjpe/ra/h"]).tolist() == [False, False, True, False]
    for k in EVAL_KEYS:
        assert torch.equal(got[k].view(torch.int32), base[k].view(torch.int32)), k


def _rotation(g):
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    return q * torch.sign(torch.linalg.det(q))


def _line_family():
    """The rank-1 inputs of docs/EXPERIMENTS.md: gt = 0.1 randn, the line a d with a in multiples of 1/512 (exact in float32)."""
    rng = np.random.default_rng(1)
    gt = torch.from_numpy((0.1 * rng.standard_normal((1, 21, 3))).astype(np.float32))
    a = rng.integers(-64, 64, (1, 21, 1)) / 512
    a[0, 0] = 0
    return gt, a, rng


DIRECTIONS = ((1, 0, 0), (1, 2, 0), (1, 1, 1), (3, 5, 7))


def test_eval_metrics_procrustes_collinear():
    """The predicted, then the ground-truth joints exactly on a line: the cross-covariance has rank 1.  The error is unique (it does
    not depend on how the singular frame is completed): 128.566 mm for the prediction on a line, whatever the direction.  Before the
    orthonormal completion in mpjpe_pa this was off by 0.1 to 3 mm."""
    gt, a, _ = _line_family()
    lines = [torch.from_numpy((a * np.array(d, np.float64)).astype(np.float32)) for d in DIRECTIONS]
    G = torch.cat([gt] * 4 + lines)
    P = torch.cat(lines + [gt] * 4)
    got = dict(zip(EVAL_KEYS, _check_eval("collinear, 4 directions x {pred, gt} on the line", _one_hand(G, P), 8)))
    for i, d in enumerate(DIRECTIONS):
        print(f"EDGE|eval_metrics mpjpe/pa/ra/r|pred on the line {d}|{abs(got['mpjpe/pa/ra/r'][i].item() - 128.566210):.3e}|2.000e-04")
        assert abs(got["mpjpe/pa/ra/r"][i].item() - 128.566210) <= 2e-4                    # 13 float32 spacings at 128
    assert torch.equal(got["mpjpe/pa/ra/r"].view(torch.int32), got["mpjpe/pa/ra/l"].view(torch.int32))


@pytest.mark.parametrize("eps", [1e-2, 1e-4, 1e-6, 1e-8])
def test_eval_metrics_procrustes_near_collinear(eps):
    gt, a, rng = _line_family()
    rows_g, rows_p = [], []
    for d in DIRECTIONS:
        line = torch.from_numpy((a * np.array(d, np.float64) + eps * 0.1 * rng.standard_normal((1, 21, 3))).astype(np.float32))
        rows_g += [gt, line]
        rows_p += [line, gt]
    _check_eval(f"near-collinear eps {eps}", _one_hand(torch.cat(rows_g), torch.cat(rows_p)), 8)


@pytest.mark.parametrize("s", [1e-3, 1.0, 1e3])
def test_eval_metrics_procrustes_similarity(s):
    """gt = s R pred + t with a random rotation and an offset of 50 m: what the alignment has to undo, at three scales."""
    g = _gen(104, s)
    pr = 0.1 * torch.randn(4, 21, 3, generator=g)
    gt = torch.stack([(s * (_rotation(g) @ p.double().T).T + 50.0 * torch.randn(3, generator=g).double()).float() for p in pr])
    _check_eval(f"gt = {s} R pred + 50 m", _one_hand(gt, pr), 4)


def test_eval_metrics_procrustes_degenerate_shapes():
    """Row 0 identical, 1 mirror image, 2 both hands in the plane z = 0, 3 prediction in that plane only, 4 / 5 the same in the
    plane spanned by (1,1,1) and (1,-1,0) (coefficients in multiples of 1/512: exact), 6 equal singular values (six joints on
    +-0.1 e_i, gt a rotated copy), 7 constant prediction (NaN), 8 constant ground truth (0)."""
    g = _gen(105)
    gt = 0.1 * torch.randn(9, 21, 3, generator=g)
    pr = gt + 0.01 * torch.randn(9, 21, 3, generator=g)
    pr[0] = gt[0]
    pr[1] = gt[1] * torch.tensor([1.0, 1.0, -1.0])
    gt[2, :, 2], pr[2, :, 2], pr[3, :, 2] = 0.0, 0.0, 0.0
    e1, e2 = torch.tensor([1.0, 1.0, 1.0]), torch.tensor([1.0, -1.0, 0.0])
    coef = lambda: torch.randint(-64, 64, (21, 2), generator=g).float() / 512
    tilt = lambda c: c[:, :1] * e1 + c[:, 1:] * e2
    gt[4], pr[4], pr[5] = tilt(coef()), tilt(coef()), tilt(coef())
    cross = torch.zeros(21, 3)
    for i in range(3):
        cross[1 + 2 * i, i], cross[2 + 2 * i, i] = 0.1, -0.1
    pr[6], gt[6] = cross, (_rotation(g) @ cross.double().T).T.float()
    pr[7] = torch.tensor([0.3, -0.2, 0.7])
    gt[8] = torch.tensor([0.3, -0.2, 0.7])
    got = dict(zip(EVAL_KEYS, _check_eval("identical, mirror, planes, equal singular values, constants", _one_hand(gt, pr), 9)))
    pa = got["mpjpe/pa/ra/r"]
    print(f"EDGE|eval_metrics mpjpe/pa/ra/r|identical pose|{pa[0].item():.3e}|1.000e-03")
    assert pa[0].item() < 1e-3 and pa[1].item() > 1.0 and torch.isnan(pa[7]) and pa[8].item() == 0.0
    assert torch.isnan(got["mpjpe/pa/ra/l"][7]) and torch.isnan(got["mpjpe/pa/ra/h"][7])


@pytest.mark.parametrize("B,NV", [(1, 1), (5, 778), (3, 257)])
def test_gt_targets(B, NV):
    """NV = 257: 771 floats are three passes of 256 threads plus 3, and i % 3 changes phase on every pass."""
    L = _lib.lib()
    g = _gen(106, B, NV)
    jc = 0.1 * torch.randn(B, 21, 3, generator=g)
    jf = jc + torch.tensor([0.1, -0.05, 0.8]) + 0.01 * torch.randn(B, 21, 3, generator=g)
    verts = 0.1 * torch.randn(B, NV, 3, generator=g)
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 900 + 200 * torch.rand(B, generator=g), 900 + 200 * torch.rand(B, generator=g)
    d = _dev(jc, verts, jf, K)
    v3d, cam_t, wp = Out(B, NV, 3), Out(B, 3), Out(B, 3)
    check(L.hands_gt_targets_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), 224.0, v3d.ptr(), cam_t.ptr(), wp.ptr(), B, NV, _stream()),
          "gt_targets")
    args = (jc, verts, jf, K, 224.0, B, NV)
    rv, rc, rw = R.gt_targets(*args)
    with R.precision(torch.float32):
        fv, _, fw = R.gt_targets(*args)
    gv, gc, gw = v3d.get(), cam_t.get(), wp.get()
    for name, got, ref, f32, rtol in (("v3d_cam", gv, rv, fv, 2e-6), ("cam_t_wp[0]", gw[:, :1], rw[:, :1], fw[:, :1], 2e-5)):
        assert not torch.isnan(got).any()
        e32 = (f32.double() - ref).abs().max().item()
        _close_each(f"gt_targets {name}", f"{B}x{NV}", got.contiguous(), ref, torch.maximum(rtol * ref.abs() + 2e-6, torch.full_like(ref, 4 * e32)))
    _exact("gt_targets cam_t", f"{B}x{NV}", gc, jf[:, 0] - jc[:, 0], rc)
    _exact("gt_targets cam_t_wp[1:]", f"{B}x{NV}", gw[:, 1:].contiguous(), (jf[:, 0] - jc[:, 0])[:, :2].contiguous(), rw[:, 1:])


@pytest.mark.parametrize("img_res", [224, 57])
@pytest.mark.parametrize("n", [1, 524288 + 77])
def test_unnormalize_kp2d(n, img_res):
    """524 365 elements: one full pass of the 2048 x 256 grid and a partial second one.  0.5 * res is exact in float32."""
    L = _lib.lib()
    x = torch.randn(n, generator=_gen(107, n, img_res))
    dx, = _dev(x)
    o = Out(n)
    check(L.hands_unnormalize_kp2d_f32(ptr(dx), o.ptr(), n, float(img_res), _stream()), "unnormalize_kp2d")
    _exact("unnormalize_kp2d", f"n {n} res {img_res}", o.get(), torch.tensor(0.5 * img_res, dtype=torch.float32) * (x + 1),
           R.unnormalize_kp2d(x, n, float(img_res)))


def test_metrics_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), Scratch()
    x, o, o2, st = ptr(s.x), ptr(s.o), ptr(s.o2), _stream()
    ein, eout = EvalIn(*[x] * 13), EvalOut(*[o] * 5, o2, o2)
    assert L.hands_eval_metrics_f32(C.byref(ein), C.byref(eout), 0, st) == EINVAL
    assert L.hands_eval_metrics_f32(C.byref(ein), C.byref(eout), -3, st) == EINVAL
    assert L.hands_eval_metrics_f32(None, C.byref(eout), 4, st) == EINVAL and L.hands_eval_metrics_f32(C.byref(ein), None, 4, st) == EINVAL
    for i in (0, 7, 12):
        a = [x] * 13
        a[i] = None
        assert L.hands_eval_metrics_f32(C.byref(EvalIn(*a)), C.byref(eout), 4, st) == EINVAL, i
    for i in (0, 6):
        a = [o] * 7
        a[i] = None
        assert L.hands_eval_metrics_f32(C.byref(ein), C.byref(EvalOut(*a)), 4, st) == EINVAL, i
    assert L.hands_gt_targets_f32(x, x, x, x, 224.0, o, o2, o2, 0, 778, st) == EINVAL
    assert L.hands_gt_targets_f32(x, x, x, x, 224.0, o, o2, o2, 2, 0, st) == EINVAL
    assert L.hands_gt_targets_f32(x, x, x, None, 224.0, o, o2, o2, 2, 778, st) == EINVAL
    assert L.hands_gt_targets_f32(x, x, x, x, 224.0, o, None, o2, 2, 778, st) == EINVAL
    assert L.hands_unnormalize_kp2d_f32(x, o, 0, 224.0, st) == EINVAL and L.hands_unnormalize_kp2d_f32(x, o, -5, 224.0, st) == EINVAL
    assert L.hands_unnormalize_kp2d_f32(None, o, 8, 224.0, st) == EINVAL
    assert s.untouched()


# ================================================================================================================================
# B. csrc/frontend.hip
# ================================================================================================================================
def _image(B, H, W, g):
    img = torch.rand(B, 3, H, W, generator=g)
    return (img + 0.3 * torch.randn(B, 3, H, W, generator=g)).clamp(-0.2, 1.2)       # exercises the clip to [0, 1]


def _run_warp(src, trans, Ho, Wo):
    L = _lib.lib()
    B, _, H, W = src.shape
    ds, = _dev(src)
    dt = trans.float().contiguous().to(DEV) if trans is not None else None
    o = Out(B, 3, Ho, Wo)
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    check(L.hands_warp_affine_cubic_norm_f32(ptr(ds), ptr(dt), o.ptr(), B, H, W, Ho, Wo, mean, std, _stream()), "warp")
    return o.get()


def _ref_warp(src, trans, Ho, Wo):
    eye = np.array([1, 0, 0, 0, 1, 0], np.float32)
    out = []
    for b in range(src.shape[0]):
        t = eye if trans is None else trans[b].float().numpy()
        patch = FO.warp_affine_cubic(src[b].numpy().transpose(1, 2, 0), t.reshape(2, 3), Ho, Wo)
        out.append(FO.normalize_img(np.clip(patch, 0, 1).transpose(2, 0, 1), MEAN, STD))
    return torch.from_numpy(np.stack(out))


def _background():
    """(0 - mean) / std in float32: what a pixel whose taps all miss the source holds."""
    return ((np.float32(0) - np.asarray(MEAN, np.float32)) / np.asarray(STD, np.float32)).astype(np.float32)


def _affine(deg, sx, sy, shear, H, W, Ho, Wo):
    """Forward map src -> dst: rotation x [[sx, shear], [0, sy]], the source centre onto the output centre."""
    th = np.deg2rad(deg)
    A = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]) @ np.array([[sx, shear], [0.0, sy]])
    t = np.array([Wo / 2, Ho / 2]) - A @ np.array([W / 2, H / 2])
    return torch.tensor([A[0, 0], A[0, 1], t[0], A[1, 0], A[1, 1], t[1]], dtype=torch.float32)


def test_warp_general_affine():
    """Rotations of 17, -40 and 90 degrees with scales 0.6 to 1.7 and a shear: all six entries of every affine non-zero, so M[1],
    M[3] and bdelta take part.  19 x 29 = 551 output pixels: three blocks, the last one partial."""
    H, W, Ho, Wo = 37, 53, 19, 29
    src = _image(3, H, W, _gen(201))
    trans = torch.stack([_affine(17, 0.6, 0.9, 0.2, H, W, Ho, Wo), _affine(-40, 1.7, 1.1, -0.3, H, W, Ho, Wo),
                         _affine(90, 0.8, 1.3, 0.25, H, W, Ho, Wo)])
    assert (trans != 0).all()
    got, ref = _run_warp(src, trans, Ho, Wo), _ref_warp(src, trans, Ho, Wo)
    bg = torch.from_numpy(_background()).view(1, 3, 1, 1)
    assert ((ref != bg).float().mean() > 0.5)                      # most of the output looks at the source
    _close("warp", "general affines 3x37x53 -> 19x29", got, ref, 2e-6)


def test_warp_identity_copies_and_pads():
    H, W = 37, 53
    src = _image(3, H, W, _gen(202))
    want = torch.from_numpy(np.stack([FO.normalize_img(np.clip(s.numpy(), 0, 1), MEAN, STD) for s in src]))
    got = _run_warp(src, None, H, W)
    assert torch.equal(got, want)
    print("EDGE|warp|trans NULL, same size: exact copy|0.000e+00|0.000e+00")
    big = _run_warp(src, None, H + 4, W + 5)
    bg = torch.from_numpy(_background()).view(1, 3, 1, 1)
    assert torch.equal(big[:, :, :H, :W], want) and torch.all(big[:, :, H:, :] == bg) and torch.all(big[:, :, :, W:] == bg)
    _close("warp", "trans NULL, 41x58 from 37x53", big, _ref_warp(src, None, H + 4, W + 5), 2e-6)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 3), (3, 4)])
def test_warp_tiny_sources(H, W):
    """Sources smaller than the 4 x 4 footprint: max(W - 3, 0) == 0, no output pixel takes the interior path."""
    src = _image(2, H, W, _gen(203, H, W))
    trans = torch.stack([_affine(0, 5 / max(W, 2), 3 / max(H, 2), 0.0, H, W, 5, 7), _affine(25, 1.6, 1.2, 0.1, H, W, 5, 7)])
    _close("warp", f"{H}x{W} -> 5x7", _run_warp(src, trans, 5, 7), _ref_warp(src, trans, 5, 7), 2e-6)
    _close("warp", f"{H}x{W} -> 5x7 trans NULL", _run_warp(src, None, 5, 7), _ref_warp(src, None, 5, 7), 2e-6)


def test_warp_outside_singular_and_saturated():
    """A window that misses the source, affines without an inverse (OpenCV sets D = 0), and translations of +-1e7 pixels, whose
    fixed-point coordinates saturate the conversion to int and the +-32768 clamp."""
    H, W, Ho, Wo = 9, 11, 6, 7
    src = _image(6, H, W, _gen(204))
    trans = torch.tensor([[1, 0, 1000, 0, 1, -1000], [0, 0, 0, 0, 0, 0], [1, 2, 3, 2, 4, 5], [1, 0, 1e7, 0, 1, 1e7],
                          [1, 0, -1e7, 0, 1, -1e7], [0.5, 0.1, 1e7, -0.2, 0.7, -1e7]], dtype=torch.float32)
    got, ref = _run_warp(src, trans, Ho, Wo), _ref_warp(src, trans, Ho, Wo)
    _close("warp", "outside, singular x2, saturated x3", got, ref, 2e-6)
    bg = torch.from_numpy(_background()).view(3, 1, 1)
    for b in (0, 3, 4, 5):
        assert torch.all(got[b] == bg) and torch.all(ref[b] == bg), b
    px = torch.from_numpy(FO.normalize_img(np.clip(src[1, :, :1, :1].numpy(), 0, 1), MEAN, STD))
    assert torch.all(got[1] == px)                                # the zero matrix maps every output pixel onto source pixel (0, 0)


class IntOut:
    """Out for an int32 output."""
    S = -77777

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((2 * BAND + self.n,), self.S, dtype=torch.int32, device=DEV)
        self.buf[BAND:BAND + self.n] = -2 ** 31

    def ptr(self):
        return ptr(self.buf, BAND)

    def get(self):
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert torch.all(h[:BAND] == self.S) and torch.all(h[BAND + self.n:] == self.S), "wrote outside the output"
        body = h[BAND:BAND + self.n].view(self.shape)
        assert torch.all(body != -2 ** 31), "left an element unwritten"
        return body


def _crafted_hands(res, ld, g):
    """(n, 21, ld) normalised joints that put the box arithmetic on its edges, for an image of `res` pixels."""
    hi = res - 1
    norm = lambda p: 2 * p / hi - 1

    def hand(x0, x1, y0, y1):
        j = torch.empty(21, 2)
        j[:, 0] = norm(x0 + (x1 - x0) * torch.rand(21, generator=g))
        j[:, 1] = norm(y0 + (y1 - y0) * torch.rand(21, generator=g))
        j[0], j[1] = torch.tensor([norm(x0), norm(y0)]), torch.tensor([norm(x1), norm(y1)])      # the extremes are hit exactly
        return j

    q = hi / 8.0
    hands = [hand(0, hi, 0, hi),                                            # joints exactly on -1 and +1
             hand(2 * q, 2 * q + 0.6, q, 5 * q), hand(q, 5 * q, 3 * q + 0.2, 3 * q + 0.9),     # width / height in (0, 1) pixel
             hand(3 * q, 3 * q, q, 6 * q),                                   # zero width, non-zero height
             hand(10.2, 41.5, 5.5, 20.7),                                    # x0 + x1 = 10 + 41: odd
             hand(-3 * q, 2 * q, 3 * q, 5 * q), hand(6 * q, 11 * q, 3 * q, 5 * q),             # clipped left / right
             hand(3 * q, 5 * q, -3 * q, 2 * q), hand(3 * q, 5 * q, 6 * q, 11 * q),             # clipped top / bottom
             hand(-5 * q, -2 * q, 3 * q, 5 * q), hand(10 * q, 13 * q, 3 * q, 5 * q),           # fully off: left / right
             hand(3 * q, 5 * q, -5 * q, -2 * q), hand(3 * q, 5 * q, 10 * q, 13 * q),           # fully off: above / below
             hand(q, 6.5 * q, 2 * q, 4 * q), hand(2.5 * q, 4 * q, 0.5 * q, 7 * q)]              # generic, wide and tall
    hands[0][0], hands[0][1] = torch.tensor([-1.0, -1.0]), torch.tensor([1.0, 1.0])
    j = torch.stack(hands)
    return j if ld == 2 else torch.cat([j, torch.full((len(hands), 21, ld - 2), 1e9)], -1)


@pytest.mark.parametrize("with_K", [True, False])
@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("ld", [2, 3])
@pytest.mark.parametrize("img_res,out_res", [(224, 224), (96, 96), (57, 128), (224, 112)])
def test_frontend_boxes(img_res, out_res, ld, B, with_K):
    """B = 33: 66 threads, a block of 64 and two.  ld = 3 carries a third column of 1e9 that is never read; bbox_scale 1.5 / 2.5."""
    L = _lib.lib()
    g = _gen(205, img_res, out_res, ld, B)
    scale = 1.5 if ld == 2 else 2.5
    pool = _crafted_hands(img_res, ld, g)
    n = pool.shape[0]
    jr = pool[[(3 * b + (5 if B == 1 else 0)) % n for b in range(B)]].contiguous()
    jl = pool[[(b + 4) % n for b in range(B)]].contiguous()
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 900 + 200 * torch.rand(B, generator=g), 900 + 200 * torch.rand(B, generator=g)
    K[:, 0, 2], K[:, 1, 2] = img_res / 2 + 5 * torch.randn(B, generator=g), img_res / 2 + 5 * torch.randn(B, generator=g)
    djr, djl, dK = _dev(jr, jl, K)
    boxes = [IntOut(B, 4) for _ in range(4)]
    fl = [Out(B, 6), Out(B, 6), Out(B, 2), Out(B, 2), Out(B, 8), Out(B, 8)]
    check(L.hands_frontend_boxes_f32(ptr(djr), ptr(djl), ld, ptr(dK) if with_K else None, B, img_res, out_res, scale,
                                     *[o.ptr() for o in boxes], *[o.ptr() for o in fl], _stream()), "frontend_boxes")
    bbox = {"r": boxes[0].get().numpy(), "l": boxes[1].get().numpy()}
    og = {"r": boxes[2].get().numpy(), "l": boxes[3].get().numpy()}
    trans, center, corner = ({"r": fl[i].get().numpy(), "l": fl[i + 1].get().numpy()} for i in (0, 2, 4))
    worst = {"trans": 0.0, "center": 0.0, "corner": 0.0}
    kinds = set()
    for b in range(B):
        for h, j in (("r", jr), ("l", jl)):
            box, rog = FO.bbox_from_joints2d(j[b].numpy(), img_res)
            patch, nb = FO.crop_window(box, img_res, scale)
            kinds.add("none" if box is None else "box")
            assert np.array_equal(bbox[h][b], np.asarray(nb).astype(np.int64)), (b, h, bbox[h][b], nb)
            assert np.array_equal(og[h][b], np.asarray(rog).astype(np.int64)), (b, h, og[h][b], rog)
            rt = FO.gen_trans_from_patch(patch[0], patch[1], patch[2], patch[3], out_res, out_res).reshape(6)
            lim = np.maximum(np.spacing(np.abs(rt)), 1e-12)
            assert np.all(np.abs(trans[h][b] - rt) <= lim), (b, h, trans[h][b], rt)
            worst["trans"] = max(worst["trans"], float((np.abs(trans[h][b] - rt) / lim).max()))
            ce, co = FO.kpe_angles(np.asarray(nb), K[b].numpy() if with_K else FO.no_intrx_matrix(img_res))
            for name, got, ref, ulps in (("center", center[h][b], ce, 1), ("corner", corner[h][b], co, 4 if with_K else 1)):
                lim = ulps * np.spacing(np.abs(ref)).astype(np.float32)
                assert np.all(np.abs(got - ref) <= lim), (b, h, name, got, ref)
                worst[name] = max(worst[name], float((np.abs(got - ref) / np.maximum(lim, 1e-45)).max()) * ulps)
    assert B == 1 or kinds == {"none", "box"}
    for k, v in worst.items():
        print(f"EDGE|frontend_boxes {k}|res {img_res}->{out_res} ld {ld} B {B} K {with_K} (spacings)|{v:.3e}|{4.0 if k == 'corner' and with_K else 1.0:.3e}")


@pytest.mark.parametrize("with_K", [True, False])
@pytest.mark.parametrize("nch", [2, 6])
@pytest.mark.parametrize("Rs", [1, 57, 224])
def test_frontend_dense_maps(Rs, nch, with_K):
    """R = 57: 3249 pixels, 13 blocks with a partial last one.  A single-pixel box, one touching (R-1, R-1), the whole image, a
    non-square one."""
    L = _lib.lib()
    m = Rs - 1
    bbox = torch.tensor([[m // 3, m // 2, m // 3, m // 2], [m - min(5, m), m - min(3, m), m, m], [0, 0, m, m],
                         [min(1, m), min(2, m), min(m, 1 + Rs // 2), min(m, 2 + Rs // 5)]], dtype=torch.int32)
    B = bbox.shape[0]
    g = _gen(206, Rs, nch)
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0], K[:, 1, 1] = 900 + 200 * torch.rand(B, generator=g), 900 + 200 * torch.rand(B, generator=g)
    K[:, 0, 2], K[:, 1, 2] = Rs / 2 + 5 * torch.randn(B, generator=g), Rs / 2 + 5 * torch.randn(B, generator=g)
    db, dK = bbox.to(DEV), K.to(DEV)
    ang, msk = Out(B, nch, Rs, Rs), Out(B, Rs, Rs)
    check(L.hands_frontend_dense_maps_f32(ptr(db), ptr(dK) if with_K else None, ang.ptr(), msk.ptr(), B, Rs, nch, _stream()), "dense_maps")
    ga, gm = ang.get().numpy(), msk.get().numpy()
    assert not np.isnan(ga).any() and not np.isnan(gm).any()
    worst = 0.0
    for b in range(B):
        ra, rm = FO.dense_maps(bbox[b].numpy(), K[b].numpy() if with_K else FO.no_intrx_matrix(Rs), Rs, cam_conv=nch == 6)
        assert np.array_equal(gm[b], rm) and np.array_equal(ga[b, 2:], ra[2:]), b
        lim = np.spacing(np.abs(ra[:2]))
        assert np.all(np.abs(ga[b, :2] - ra[:2]) <= lim), b
        worst = max(worst, float((np.abs(ga[b, :2] - ra[:2]) / lim).max()))
    print(f"EDGE|dense_maps angles|R {Rs} nch {nch} K {with_K} (spacings)|{worst:.3e}|1.000e+00")


def test_frontend_downscaled_end_to_end():
    """HandsFrontEnd with img_res_ds != img_res: the branch of __call__ that warps the full frame with [s, 0, 0, 0, s, 0], and
    boxes whose affines map 96-pixel windows onto 64-pixel crops."""
    from hands_amd import HandsFrontEnd
    B = 5
    g = _gen(207)
    img = _image(B, 96, 96, g)
    pool = _crafted_hands(96, 3, g)
    jr, jl = pool[[13, 0, 9, 5, 14]].contiguous(), pool[[14, 4, 13, 3, 8]].contiguous()
    jr[..., 2:], jl[..., 2:] = 1.0, 1.0
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 400.0
    K[:, 0, 2] = K[:, 1, 2] = 48.0
    fe = HandsFrontEnd({"img_res": 96, "img_res_ds": 64})
    out = fe(*_dev(img, jr, jl, K))
    geo = fe.boxes(*_dev(jr, jl, K))
    torch.cuda.synchronize()
    assert out["img"].shape == (B, 3, 64, 64) and out["r_img"].shape == (B, 3, 64, 64)
    worst = {"img": 0.0, "crop": 0.0}
    for b in range(B):
        ref = FO.frontend_sample(img[b].numpy(), jr[b].numpy(), jl[b].numpy(), K[b].numpy(), img_res=96, out_res=64)
        worst["img"] = max(worst["img"], float(np.abs(out["img"][b].cpu().numpy() - ref["img"]).max()))
        for h in "rl":
            assert np.array_equal(out[f"{h}_bbox"][b].cpu().numpy(), ref[f"{h}_bbox"].astype(np.int16)), (b, h)
            t, rt = geo[f"{h}_trans"][b].cpu().numpy(), ref[f"{h}_trans"].reshape(6)
            assert np.all(np.abs(t - rt) <= np.maximum(np.spacing(np.abs(rt)), 1e-12)), (b, h, t, rt)
            want = ref[f"{h}_img"]
            if not np.array_equal(t, rt):        # an affine one spacing away moves 1/32-pixel phases: warp with the device's own
                patch = FO.warp_affine_cubic(img[b].numpy().transpose(1, 2, 0), t.reshape(2, 3), 64, 64)
                want = FO.normalize_img(np.clip(patch, 0, 1).transpose(2, 0, 1), MEAN, STD)
            worst["crop"] = max(worst["crop"], float(np.abs(out[f"{h}_img"][b].cpu().numpy() - want).max()))
    print(f"EDGE|HandsFrontEnd 96->64|img|{worst['img']:.3e}|1.000e-06")
    print(f"EDGE|HandsFrontEnd 96->64|r_img, l_img|{worst['crop']:.3e}|2.000e-06")
    assert worst["img"] <= 1e-6 and worst["crop"] <= 2e-6


def test_frontend_entry_points_reject_what_is_outside_their_contract():
    L, s = _lib.lib(), Scratch()
    x, o, o2, st = ptr(s.x), ptr(s.o), ptr(s.o2), _stream()
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    warp = lambda B, H, W, Ho, Wo, m=mean: L.hands_warp_affine_cubic_norm_f32(x, None, o, B, H, W, Ho, Wo, m, std, st)
    assert warp(65536, 1, 1, 1, 1) == EINVAL                                                           # B is a grid dimension
    for dims in ((0, 4, 4, 4, 4), (1, 0, 4, 4, 4), (1, 4, 0, 4, 4), (1, 4, 4, 0, 4), (1, 4, 4, 4, 0), (1, -4, 4, 4, 4)):
        assert warp(*dims) == EINVAL, dims
    assert warp(1, 4, 4, 4, 4, None) == EINVAL
    assert L.hands_warp_affine_cubic_norm_f32(None, None, o, 1, 4, 4, 4, 4, mean, std, st) == EINVAL
    boxes = lambda B, ld, res, ores, scale, c=o2: L.hands_frontend_boxes_f32(x, x, ld, x, B, res, ores, scale, o, o, o, o, o2, o2, o2, o2, c, c, st)
    assert boxes(0, 2, 224, 224, 1.5) == EINVAL and boxes(2, 1, 224, 224, 1.5) == EINVAL                # ld < 2
    assert boxes(2, 2, 1, 224, 1.5) == EINVAL and boxes(2, 2, 224, 0, 1.5) == EINVAL
    assert boxes(2, 2, 224, 224, 0.0) == EINVAL and boxes(2, 2, 224, 224, float("nan")) == EINVAL
    assert boxes(2, 2, 224, 224, 1.5, None) == EINVAL
    dense = lambda B, res, nch: L.hands_frontend_dense_maps_f32(x, x, o, o2, B, res, nch, st)
    assert dense(0, 8, 2) == EINVAL and dense(65536, 8, 2) == EINVAL and dense(2, 0, 2) == EINVAL
    assert dense(2, 8, 3) == EINVAL and dense(2, 8, 0) == EINVAL                                       # 2 or 6 maps
    assert L.hands_frontend_dense_maps_f32(None, x, o, o2, 2, 8, 2, st) == EINVAL
    assert s.untouched()
