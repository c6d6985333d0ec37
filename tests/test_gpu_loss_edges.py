"""Edge tests of csrc/loss.hip (hands_loss_light_f32): maps of 1 to 9 elements per sample, many small-term chunks, the
scalar-load path, the all-invalid rule of transl/l, a poisoned workspace for every combination of optional groups, grasp and
pose extremes, and the rejections -- against tests/loss_ref.py in float64.

Bound (that of tests/test_gpu_losses.py): every key within 2 x d_ref of the float64 value, d_ref being loss_ref's own
float32-vs-float64 distance on the same inputs (asserted to lie in (0, 1e-6)); exact zeros, NaN positions and the bit-identity
checks carry no tolerance.  Every comparison prints ``EDGE|kernel|case|error|bound`` before it asserts."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import loss_ref
from edge_util import DEV, EINVAL, Out, Scratch, _stream
from hands_amd import _lib
from hands_amd._lib import ptr

pytestmark = pytest.mark.gpu

NK = _lib.LOSS_NKEYS


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def rel_dist(a, b):
    worst = 0.0
    for k in b:
        x, y = float(a[k][0]), float(b[k][0])
        if y != 0.0 and math.isfinite(y):
            worst = max(worst, abs(x - y) / abs(y))
    return worst


def _references(pred, gt, meta, args):
    r64 = loss_ref.compute_loss_light(pred, gt, meta, args, dtype=torch.float64)
    d_ref = rel_dist(loss_ref.compute_loss_light(pred, gt, meta, args), r64)
    assert 0.0 < d_ref < 1e-6, d_ref
    return r64, d_ref


def _check(case, got, r64, d_ref):
    """Every key within 2 d_ref of the float64 value; NaN exactly where the reference has it; an exact 0 stays 0."""
    assert list(got) == list(r64), case
    for k in r64:
        x, y = float(got[k][0][0]), float(r64[k][0][0])
        if math.isnan(y):
            print(f"EDGE|loss_light|{case} {k}|nan|nan")
            assert math.isnan(x), (case, k, x)
            continue
        print(f"EDGE|loss_light|{case} {k}|{abs(x - y):.3e}|{2.0 * d_ref * abs(y):.3e}")
        assert math.isfinite(x) and abs(x - y) <= 2.0 * d_ref * abs(y), (case, k, x, y, d_ref)


def _has_mix(v):
    """Both values occur within at least one aligned group of four consecutive samples."""
    v = v.reshape(-1).float()
    pad = (-v.numel()) % 4
    lo = torch.cat([v, torch.full((pad,), 2.0)]).view(-1, 4).min(1)[0]
    hi = torch.cat([v, torch.full((pad,), -1.0)]).view(-1, 4).max(1)[0]
    return bool(((lo == 0) & (hi == 1)).any())


def _mixed_case(B, S_mask, S_depth, seed):
    """loss_ref.random_case with the per-sample weights of the streamed terms mixed inside the first vector of four samples."""
    pred, gt, meta, args = loss_ref.random_case(B, S_mask, S_depth, seed)
    pat = {"render_valid_r": (1.0, 0.0, 1.0, 1.0), "render_valid_l": (0.0, 1.0, 1.0, 0.0)}
    for k, p in pat.items():
        gt[k][:min(B, 4)] = torch.tensor(p)[:min(B, 4)]
    for k, p in (("is_mask_loss", (1.0, 1.0, 0.0, 1.0)), ("is_depth_loss", (1.0, 0.0, 1.0, 1.0))):
        meta[k][:min(B, 4)] = torch.tensor(p)[:min(B, 4)]
    if B >= 2:
        for v in (gt["render_valid_r"], gt["render_valid_l"], meta["is_depth_loss"]):
            assert _has_mix(v)
        assert B < 4 or _has_mix(meta["is_mask_loss"])
    return pred, gt, meta, args


# ---- D1: tiny maps and many chunks --------------------------------------------------------------------------------------------
D1_CASES = [(8197, 1, 3), (8193, 2, 1), (65, 3, 2), (33, 3, 1), (2049, 1, 1),
            (8, 32, 1),                  # 8 * 1024 elements: exactly one chunk of 8192
            (2, 64, 1),                  # 2 * 4096 elements: one full chunk made of two samples
            (4, 64, 1)]                  # 4 * 4096 elements: exactly two chunks


@pytest.mark.parametrize("B,S_mask,S_depth", D1_CASES)
def test_d1_tiny_maps_and_many_chunks(B, S_mask, S_depth):
    """Per-sample lengths 1, 2, 3 (4 and 9 squared: 1, 4, 9): a 16-byte vector spans up to four samples whose validity and flag
    differ; totals that are no multiple of 4; more than 64 small-term chunks (B > 2048) and two streamed chunks at S = 1."""
    import hands_amd
    pred, gt, meta, args = _mixed_case(B, S_mask, S_depth, seed=1000 + B)
    r64, d_ref = _references(pred, gt, meta, args)
    dp, dg, dm = to_dev(pred), to_dev(gt), to_dev(meta)
    got = hands_amd.compute_loss_light(dp, dg, dm, args)
    _check(f"D1 B={B} S_mask={S_mask} S_depth={S_depth} d_ref={d_ref:.2e}", got, r64, d_ref)


# ---- D2: the scalar-load path ------------------------------------------------------------------------------------------------
def _offset_view(t):
    """The same values as a contiguous view that starts one float into its allocation: 4-byte aligned only."""
    base = torch.empty(t.numel() + 8, device=DEV)
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("S", [31, 3])
def test_d2_scalar_load_path_has_the_bits_of_the_vector_path(S):
    """loss_partials_kernel<false> (a mask or depth pointer that is not 16-byte aligned) assigns the same four elements to the
    same thread in the same order as the 16-byte path: all 43 outputs are bit-equal."""
    import hands_amd
    B = 37
    pred, gt, meta, args = _mixed_case(B, S, S, seed=2000 + S)
    r64, d_ref = _references(pred, gt, meta, args)
    dp, dg, dm = to_dev(pred), to_dev(gt), to_dev(meta)
    _, aligned = hands_amd.losses.loss_light_raw(dp, dg, dm, args)
    dp2, dg2 = dict(dp), dict(dg)
    for h in "rl":
        for d_, k in ((dp2, f"render.{h}"), (dg2, f"render.{h}"), (dp2, f"depth.{h}"), (dg2, f"depth.{h}")):
            d_[k] = _offset_view(d_[k])
            assert d_[k].contiguous().data_ptr() == d_[k].data_ptr()            # the wrapper hands this very view over
    _, offset = hands_amd.losses.loss_light_raw(dp2, dg2, dm, args)
    diff = int((aligned != offset).sum())
    print(f"EDGE|loss_light|D2 S={S} outputs differing between the 16-byte and the scalar path|{diff}|0")
    assert torch.equal(aligned, offset) and torch.isfinite(offset).all()
    _check(f"D2 S={S} scalar path d_ref={d_ref:.2e}", hands_amd.compute_loss_light(dp2, dg2, dm, args), r64, d_ref)


# ---- D3: the all-invalid rule of transl/l reads sum(right_valid * left_valid) -----------------------------------------------
@pytest.mark.parametrize("both_valid_at", [None, 4])
@pytest.mark.parametrize("with_nan", [True, False])
def test_d3_transl_rule_reads_the_product_of_the_validities(both_valid_at, with_nan):
    import hands_amd
    B = 9
    pred, gt, meta, args = loss_ref.random_case(B, 3, 2, seed=3000)
    gt["right_valid"] = (torch.arange(B) % 2 == 0).float()
    gt["left_valid"] = 1.0 - gt["right_valid"]
    if both_valid_at is not None:
        gt["left_valid"][both_valid_at] = 1.0
    meta["is_cam_loss"][:] = 1.0
    assert gt["right_valid"].sum() > 0 and gt["left_valid"].sum() > 0
    assert (gt["right_valid"] * gt["left_valid"]).sum().item() == (0 if both_valid_at is None else 1)
    if with_nan:
        assert gt["right_valid"][1] == 0
        pred["mano.cam_t.wp.r"][1, 2] = float("nan")          # the right hand of sample 1 is invalid
    r64, d_ref = _references(pred, gt, meta, args)
    got = hands_amd.compute_loss_light(to_dev(pred), to_dev(gt), to_dev(meta), args)
    _check(f"D3 both_valid_at={both_valid_at} nan={int(with_nan)}", got, r64, d_ref)
    t = float(got["loss/mano/transl/l"][0][0])
    if both_valid_at is None:
        assert t == 0.0 and float(r64["loss/mano/transl/l"][0][0]) == 0.0
    else:
        assert math.isnan(t) if with_nan else t > 0.0
    assert math.isnan(float(got["loss/mano/cam_t/r"][0][0])) == with_nan
    assert math.isfinite(float(got["loss/mano/cam_t/l"][0][0]))


# ---- D4: the workspace needs no zero-fill -------------------------------------------------------------------------------------
def _c_call(a, B, S_mask, S_depth, ws_ptr, out):
    return _lib.lib().hands_loss_light_f32(C.byref(a), B, S_mask, S_depth, ws_ptr, out.ptr(), out.ptr() + 4 * NK,
                                          out.ptr() + 8 * NK, _stream())


@pytest.mark.parametrize("combo", range(16))
def test_d4_poisoned_workspace(combo):
    """Through the C entry for each present / absent combination of the four optional groups: a workspace of exactly
    hands_loss_workspace_bytes full of NaN gives the bits of a zero-filled one, absent keys are 0, nothing outside is written."""
    from hands_amd.losses import LOSS_KEYS, bind_loss_inputs, loss_keys
    L = _lib.lib()
    B, S_mask, S_depth = 5, 3, 2
    pred, gt, meta, _ = _mixed_case(B, S_mask, S_depth, seed=4000)
    args = {"use_grasp_loss": bool(combo & 1), "use_render_seg_loss": bool(combo & 2), "use_depth_loss": bool(combo & 4),
            "regress_center_corner": bool(combo & 8)}
    a, keep, _, B_, sm, sd = bind_loss_inputs(to_dev(pred), to_dev(gt), to_dev(meta), args)
    assert (B_, sm, sd) == (B, S_mask if combo & 2 else 0, S_depth if combo & 4 else 0)
    nbytes = L.hands_loss_workspace_bytes(B, sm, sd)
    assert nbytes > 0 and nbytes % 8 == 0
    res = []
    for poison in (True, False):
        ws = Out(nbytes // 4) if poison else Out(nbytes // 4, init=torch.zeros(nbytes // 4))
        assert ws.ptr() % 8 == 0
        out = Out(2 * NK + 1)
        assert _c_call(a, B, sm, sd, ws.ptr(), out) == 0
        res.append(out.get())
        ws.get()                                             # the bands of the workspace
    diff = int((res[0] != res[1]).sum())
    print(f"EDGE|loss_light|D4 combo={combo:04b} outputs differing between a NaN and a zero workspace|{diff}|0")
    assert torch.equal(res[0], res[1]) and torch.isfinite(res[0]).all()
    present = set(loss_keys(args))
    for i, k in enumerate(LOSS_KEYS):
        if k not in present:
            assert res[0][i] == 0 and res[0][NK + i] == 0, k
    r64, d_ref = _references(pred, gt, meta, args)
    _check(f"D4 combo={combo:04b}", {k: (res[0][LOSS_KEYS.index(k)].view(1), 0) for k in loss_keys(args)}, r64, d_ref)
    del keep


# ---- D5: grasp and pose extremes ----------------------------------------------------------------------------------------------
def test_d5_grasp_and_pose_extremes():
    import hands_amd
    B = 8
    pred, gt, meta, args = loss_ref.random_case(B, 3, 2, seed=5000, switches=("grasp",))
    for h in "rl":
        lg = pred[f"grasp.{h}"]
        lg[0] = 0.0
        lg[0, 0] = 1e4                                       # one huge logit, the label on it (loss 0) ...
        lg[1] = 0.0
        lg[1, 8] = 1e4                                       # ... and off it (loss 1e4)
        lg[2] = -1e4                                         # all equal and hugely negative: log 9
        lg[3] = 3.5                                          # all equal
        lg[4, 0], lg[4, 8] = -1e4, 1e4
        gt[f"grasp.{h}"] = torch.tensor([0, 0, 8, 0, 8, 8, 0, 4])
        gt[f"grasp_valid_{h}"][:] = 1.0
        gt[f"mano.pose.{h}"][0] = 0.0                        # GT axis-angle of exactly zero
        ax = torch.tensor([2.0, -1.0, 2.0]) / 3.0
        gt[f"mano.pose.{h}"][1] = (1e-7 * ax).repeat(16)     # and of norm 1e-7: the series branch of the conversion
    gt["right_valid"][:] = 1.0
    gt["left_valid"][:] = 1.0
    meta["is_grasp_loss"][:] = 1.0
    meta["is_pose_loss"][:] = 1.0
    for h in "rl":
        ce = F.cross_entropy(pred[f"grasp.{h}"].double(), gt[f"grasp.{h}"], reduction="none")
        assert ce[0] == 0 and ce[1] == 1e4 and abs(ce[2] - math.log(9)) < 1e-10 and abs(ce[3] - math.log(9)) < 1e-10 and ce[4] == 0
    r64, d_ref = _references(pred, gt, meta, args)
    got = hands_amd.compute_loss_light(to_dev(pred), to_dev(gt), to_dev(meta), args)
    _check(f"D5 extremes d_ref={d_ref:.2e}", got, r64, d_ref)
    for h in "rl":
        want = F.cross_entropy(pred[f"grasp.{h}"].double(), gt[f"grasp.{h}"], reduction="none").mean().item()
        x = float(got[f"loss/grasp/{h}"][0][0])
        print(f"EDGE|loss_light|D5 grasp/{h} vs F.cross_entropy fp64|{abs(x - want):.3e}|{2.0 * d_ref * want:.3e}")
        assert abs(x - want) <= 2.0 * d_ref * want


# ---- D6: rejections -----------------------------------------------------------------------------------------------------------
def test_d6_rejections_launch_nothing():
    from hands_amd.losses import bind_loss_inputs
    L = _lib.lib()
    s = Scratch()
    B, S_mask, S_depth = 4, 3, 2
    pred, gt, meta, args = loss_ref.random_case(B, S_mask, S_depth, seed=6000)
    dp, dg, dm = to_dev(pred), to_dev(gt), to_dev(meta)
    a, keep, _, _, _, _ = bind_loss_inputs(dp, dg, dm, args)
    ws = torch.zeros(L.hands_loss_workspace_bytes(B, S_mask, S_depth) // 4 + 4, device=DEV)
    assert ptr(ws) % 8 == 0

    def call(a_, B_=B, sm=S_mask, sd=S_depth, w=ptr(ws)):
        return L.hands_loss_light_f32(C.byref(a_), B_, sm, sd, w, ptr(s.o), ptr(s.o, NK), ptr(s.o, 2 * NK), _stream())

    assert call(a, w=ptr(ws, 1)) == EINVAL                   # a workspace at an address = 4 (mod 8)
    assert call(a, w=None) == EINVAL
    for bad in (0, -1, 32769):
        assert call(a, sm=bad) == EINVAL and call(a, sd=bad) == EINVAL, bad
    assert call(a, B_=0) == EINVAL and call(a, B_=-2) == EINVAL
    # a (B, S) whose workgroup count does not fit an int: 2 * ceil(16384 * 32768^2 / 8192) = 2^32
    assert L.hands_loss_workspace_bytes(16384, 32768, 0) == 0 and L.hands_loss_workspace_bytes(16384, 0, 32768) == 0
    assert call(a, B_=16384, sm=32768) == EINVAL and call(a, B_=16384, sd=32768) == EINVAL
    for shape in ((0, 1, 1), (-1, 1, 1), (4, -1, 0), (4, 0, -1), (4, 32769, 0), (4, 0, 32769), (2 ** 31 - 1, 32768, 32768)):
        assert L.hands_loss_workspace_bytes(*shape) == 0, shape
    assert L.hands_loss_workspace_bytes(4, 32768, 0) > 0 and L.hands_loss_workspace_bytes(1, 0, 0) > 0
    assert s.untouched()
    # the S of an ABSENT group is ignored: the same bits whatever is passed for it
    base_args = dict(args, use_render_seg_loss=False, use_depth_loss=False)
    a2, keep2, _, _, sm2, sd2 = bind_loss_inputs(dp, dg, dm, base_args)
    assert (sm2, sd2) == (0, 0)
    outs = []
    for sm, sd in ((0, 0), (-1, 32769), (12345, -7)):
        out = Out(2 * NK + 1)
        assert L.hands_loss_light_f32(C.byref(a2), B, sm, sd, ptr(ws), out.ptr(), out.ptr() + 4 * NK, out.ptr() + 8 * NK, _stream()) == 0
        outs.append(out.get())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and torch.isfinite(outs[0]).all()
    del keep, keep2
