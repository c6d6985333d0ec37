"""Launch-geometry and edge parity tests of csrc/mano_lbs.hip: hands_mano_heads_f32 (every vertex split, ragged and tiny hand
counts, both input forms), hands_mano_pose_f32 / hands_mano_pose_aa_f32 / hands_mano_skin_f32 (row strides, the three-launch
chain), the camera clamp, and the rejections of all four entries -- against ``kernel_refs.mano_head_ref`` in float64.

Inputs (tests/mano_cases.py): a general K (independent fx / fy, skew, a last row that is not 0 0 1), betas from N(0,1) and
3 N(0,1), rotations random / identity / theta = 1e-7 / pi - 1e-4 / pi, tips at chunk edges, three kinds of asset.
Bounds: the project's MANO bounds (1e-6 on vertices and joints, rtol = atol = 2e-6 in camera space, 1e-5 on j2d.norm, rtol 1e-6
on cam_t), widened only by ``edge_util._rule``: 4 x the error of the float32 ATen evaluation of the reference on the same inputs.
Bit-identity checks carry no tolerance.  Every comparison prints ``EDGE|kernel|case|error|bound`` before it asserts."""
import ctypes as C

import pytest
import torch

import fake_mano
import kernel_refs as R
import mano_cases as MC
from edge_util import BAND, DEV, EINVAL, SENT, In, Out, Scratch, _close, _close_each, _rule, _stream, strided
from hands_amd import _lib
from hands_amd._lib import check, ptr
from hands_amd.engine import DEFAULT_ENGINE
from hands_amd.mano import synthetic_mano_asset
from hands_amd.packing import pack_mano
from oracle import hands_oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("vertices", "joints3d", "v3d.cam", "j3d.cam", "j2d.norm", "cam_t")      # in hands_mano_out's member order
SHAPES = {"vertices": (778, 3), "joints3d": (21, 3), "v3d.cam": (778, 3), "j3d.cam": (21, 3), "j2d.norm": (21, 2), "cam_t": (3,)}
MIN_S = R._f32(0.1)                     # the float the C entries receive
_ASSETS = {"syn_r": lambda: synthetic_mano_asset(True), "syn_l": lambda: synthetic_mano_asset(False),
           "real_r": lambda: fake_mano.realistic_mano_asset(True), "real_l": lambda: fake_mano.realistic_mano_asset(False),
           "dense_l": lambda: MC.dense_weight_asset(False)}
_packed = {}


def _asset(name, tips=O.TIP_IDS):
    """-> (asset, packed constants on the device with ``tips`` as tip_ids, hands_mano_consts)."""
    key = (name, tuple(tips))
    if key not in _packed:
        a = _ASSETS[name]()
        mp = pack_mano(a, DEV)
        mp["tip_ids"] = torch.tensor(tips, dtype=torch.int32, device=DEV)
        consts = _lib.ManoConsts(ptr(mp["pose_mean"]), ptr(mp["J_template"]), ptr(mp["J_shapedirs"]), ptr(mp["lbs_weights"]),
                                 ptr(mp["tip_ids"]))
        _packed[key] = (a, mp, consts)
    return _packed[key]


def _outs(B):
    return {k: Out(B, *SHAPES[k]) for k in KEYS}


def _mano_out(o):
    return _lib.ManoOut(*[o[k].ptr() for k in KEYS])


def _fused(names, tips, rot, betas, cam, K, B, aa, img_res=224.0, min_s=MIN_S, ld_betas=10):
    """hands_mano_heads_f32 on len(names) sides; rot / betas / cam hold side s in rows [s B, (s + 1) B).  Inputs sit behind NaN
    (In), betas ``ld_betas`` apart with NaN in the gap, outputs are NaN inside sentinel bands.  -> [dict of Out] per side."""
    L = _lib.lib()
    n = len(names)
    per = 48 if aa else 144
    rot_i, cam_i, K_i = In(rot.reshape(n * B, per)), In(cam.reshape(n * B, 3)), In(K.reshape(B, 9))
    bet_i = In(strided(betas.reshape(n * B, 10), ld_betas, float("nan")))
    sides = (_lib.ManoSide * n)()
    outs = []
    for s, name in enumerate(names):
        _, mp, consts = _asset(name, tips)
        o = _outs(B)
        sides[s] = _lib.ManoSide(consts, ptr(mp["blend"].w), ptr(mp["blend"].bias), rot_i.ptr(s * B * per),
                                 bet_i.ptr(s * B * ld_betas), cam_i.ptr(s * B * 3), _mano_out(o))
        outs.append(o)
    check(L.hands_mano_heads_f32(sides, n, K_i.ptr(), ld_betas, img_res, min_s, B, int(aa), _stream()), "mano_heads")
    torch.cuda.synchronize()
    return outs


class _Ref:
    """mano_head_ref in float64 and, on demand, its float32 evaluation (once) for ``_rule``."""

    def __init__(self, name, tips, rot, betas, cam, K, aa, img_res=224.0, min_s=MIN_S):
        self.args = (rot, betas, cam, K, _asset(name, tips)[0], img_res, min_s, tips, aa)
        self.r64 = R.mano_head_ref(*self.args)
        self.r32 = None
        assert self.r64["hz"].min().item() > 1.0, "the projection's divisor must stay well away from zero"

    def f32(self, key):
        if self.r32 is None:
            self.r32 = R.mano_head_ref(*self.args)          # called by _rule inside precision(float32)
        return self.r32[key]

    def check(self, kernel, case, key, got, rows=None):
        """``got`` against the reference's ``key`` at the project's bound for it, widened by the rule."""
        ref = self.r64[key] if rows is None else self.r64[key][rows]
        if key in ("vertices", "joints3d", "blend_row", "A", "joints16"):
            bound, e32 = _rule(1e-6, self.r64[key], self.f32, key)
            _close(kernel, f"{case} {key} e32={e32:.2e}", got, ref, bound)
        elif key == "j2d.norm":
            bound, e32 = _rule(1e-5, self.r64[key], self.f32, key)
            _close(kernel, f"{case} {key} e32={e32:.2e}", got, ref, bound)
        else:
            rtol, atol = (1e-6, 0.0) if key == "cam_t" else (2e-6, 2e-6)
            _, e32 = _rule(0.0, self.r64[key], self.f32, key)
            bound = torch.maximum(atol + rtol * ref.abs(), torch.full_like(ref, 4 * e32))
            _close_each(kernel, f"{case} {key} e32={e32:.2e}", got, ref, bound)

    def check_all(self, kernel, case, outs, tips):
        got = {k: outs[k].get() for k in KEYS}              # bands checked here
        for k in KEYS:
            self.check(kernel, case, k, got[k])
        assert torch.equal(got["joints3d"][:, 16:], got["vertices"][:, list(tips)]), (kernel, case, "tips are not the vertices")
        return got


# ---- B1: every vertex split ---------------------------------------------------------------------------------------------------
P = 48                                   # distinct hands per side; every larger launch tiles them
B1_NAMES = ("real_r", "dense_l")
# one hand count per band of the split rule (two sides), none a multiple of 16, five of them = 1 (mod 16)
B1_COUNTS = (97, 929, 1300, 1601, 2200, 3201, 6401)
_b1_cache = {}


def _b1_small(tips):
    """The 48-hand launch of both sides (split 13) with its inputs and references, computed once per tip set."""
    if tips not in _b1_cache:
        rot, _, betas, cam, K = MC.inputs(2 * P, 101, sigma=3.0)
        K = K[:P]
        assert _lib.lib().hands_mano_heads_vsplit(P, 2) == 13
        outs = _fused(B1_NAMES, tips, rot, betas, cam, K, P, False)
        refs = [_Ref(B1_NAMES[s], tips, rot[s * P:(s + 1) * P], betas[s * P:(s + 1) * P], cam[s * P:(s + 1) * P], K, False)
                for s in range(2)]
        small = [{k: o[k].get().to(DEV) for k in KEYS} for o in outs]
        _b1_cache[tips] = (rot, betas, cam, K, outs, refs, small)
    return _b1_cache[tips]


@pytest.mark.parametrize("tips", [O.TIP_IDS, MC.EDGE_TIPS], ids=["default_tips", "edge_tips"])
def test_b1_small_launch_against_reference(tips):
    _, _, _, _, outs, refs, _ = _b1_small(tips)
    for s in range(2):
        refs[s].check_all("mano_heads", f"B1 P={P} side{s} {B1_NAMES[s]}", outs[s], tips)


def test_b1_counts_cover_every_split():
    L = _lib.lib()
    splits = [L.hands_mano_heads_vsplit(B, 2) for B in B1_COUNTS]
    print("EDGE|mano_heads_vsplit|B -> split|" + " ".join(f"{b}:{v}" for b, v in zip(B1_COUNTS, splits)) + "|-")
    assert sorted(splits) == [1, 2, 3, 4, 5, 7, 13]
    assert all(B % 16 for B in B1_COUNTS) and any(B % 16 == 1 for B in B1_COUNTS) and all(B % P for B in B1_COUNTS)
    assert L.hands_mano_heads_vsplit(0, 2) == 0 and L.hands_mano_heads_vsplit(5, 0) == 0 and L.hands_mano_heads_vsplit(5, 3) == 0
    assert L.hands_mano_heads_vsplit(1, 1) == 13 and L.hands_mano_heads_vsplit(2 ** 31 - 1, 2) == 1


@pytest.mark.parametrize("tips", [O.TIP_IDS, MC.EDGE_TIPS], ids=["default_tips", "edge_tips"])
@pytest.mark.parametrize("B", B1_COUNTS)
def test_b1_every_split_equals_the_small_launch(B, tips):
    """Hand i of a B-hand launch (whatever split of the 13 vertex chunks over blockIdx.z it takes) is hand i % 48 of the 48-hand
    launch, bit for bit, all six outputs of both sides, compared on the device; nothing outside the outputs is written."""
    L = _lib.lib()
    rot, betas, cam, K, _, refs, small = _b1_small(tips)
    idx = torch.arange(B) % P
    two = lambda t: torch.cat([t[:P][idx], t[P:][idx]])
    outs = _fused(B1_NAMES, tips, two(rot), two(betas), two(cam), K[idx], B, False)
    vs = L.hands_mano_heads_vsplit(B, 2)
    didx = idx.to(DEV)
    for s in range(2):
        for k in KEYS:
            o = outs[s][k]
            assert bool(torch.all(o.buf[:BAND] == SENT)) and bool(torch.all(o.buf[BAND + o.n:] == SENT)), (B, vs, s, k, "band")
            body = o.buf[BAND:BAND + o.n].view(o.shape)
            bad = int((body != small[s][k][didx]).any(dim=tuple(range(1, body.dim()))).sum())
            print(f"EDGE|mano_heads|B1 B={B} split={vs} side{s} {k} hands differing|{bad}|0")
            assert bad == 0 and torch.equal(body, small[s][k][didx]), (B, vs, s, k)
        body = {k: outs[s][k].buf[BAND:BAND + outs[s][k].n].view(outs[s][k].shape) for k in KEYS}
        assert torch.equal(body["joints3d"][:, 16:], body["vertices"][:, list(tips)]), (B, vs, s, "tips")
        for k in ("j3d.cam", "j2d.norm"):                    # the tip joints against the reference, on the device
            ref = refs[s].r64[k][:, 16:]
            if k == "j2d.norm":
                bound = torch.full_like(ref, _rule(1e-5, refs[s].r64[k], refs[s].f32, k)[0])
            else:
                bound = torch.maximum(2e-6 + 2e-6 * ref.abs(), torch.full_like(ref, 4 * _rule(0.0, refs[s].r64[k], refs[s].f32, k)[1]))
            err = (body[k][:, 16:].double() - ref.to(DEV)[didx]).abs()
            worst = (err / bound.to(DEV)[didx]).max().item()
            print(f"EDGE|mano_heads|B1 B={B} split={vs} side{s} tip {k} (error / bound)|{worst:.3e}|1.000e+00")
            assert worst <= 1.0, (B, vs, s, k, worst)


# ---- B2: ragged and tiny B through the fused entry ------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["matrix", "axis_angle"])
@pytest.mark.parametrize("n_sides", [1, 2])
@pytest.mark.parametrize("B", [1, 2, 15, 16, 17, 33])
def test_b2_ragged_and_tiny_counts(B, n_sides, aa):
    names = ("syn_r", "syn_l")[:n_sides]
    rot, ax, betas, cam, K = MC.inputs(n_sides * B, 200 + B + 7 * n_sides, sigma=3.0 if aa else 1.0)
    K = K[:B]
    pose = ax if aa else rot
    outs = _fused(names, O.TIP_IDS, pose, betas, cam, K, B, aa)
    for s, name in enumerate(names):
        sl = slice(s * B, (s + 1) * B)
        ref = _Ref(name, O.TIP_IDS, pose[sl], betas[sl], cam[sl], K, aa)
        ref.check_all("mano_heads", f"B2 B={B} sides={n_sides} aa={int(aa)} side{s}", outs[s], O.TIP_IDS)


# ---- B3: strides --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld_betas", [10, 11, 16, 37])
def test_b3_fused_entry_beta_stride(ld_betas):
    B = 5
    rot, _, betas, cam, K = MC.inputs(2 * B, 300 + ld_betas, sigma=3.0)
    outs = _fused(("real_r", "real_l"), MC.EDGE_TIPS, rot, betas, cam, K[:B], B, False, ld_betas=ld_betas)
    for s, name in enumerate(("real_r", "real_l")):
        sl = slice(s * B, (s + 1) * B)
        _Ref(name, MC.EDGE_TIPS, rot[sl], betas[sl], cam[sl], K[:B], False).check_all(
            "mano_heads", f"B3 ld_betas={ld_betas} side{s}", outs[s], MC.EDGE_TIPS)


def _pose(name, pose, betas, B, aa, ld_betas, ld_blend):
    """hands_mano_pose_f32 / hands_mano_pose_aa_f32 -> (blend_in (B, ld_blend), A (B,16,12), joints16 (B,16,3)) as Out."""
    L = _lib.lib()
    _, _, consts = _asset(name)
    pose_i, bet_i = In(pose.reshape(B, -1)), In(strided(betas, ld_betas, float("nan")))
    blend, A, j16 = Out(B, ld_blend), Out(B, 16, 12), Out(B, 16, 3)
    fn = L.hands_mano_pose_aa_f32 if aa else L.hands_mano_pose_f32
    check(fn(C.byref(consts), pose_i.ptr(), bet_i.ptr(), ld_betas, blend.ptr(), ld_blend, A.ptr(), j16.ptr(), B, _stream()), "mano_pose")
    return blend, A, j16


@pytest.mark.parametrize("aa", [False, True], ids=["matrix", "axis_angle"])
@pytest.mark.parametrize("B", [1, 3, 4, 5])
@pytest.mark.parametrize("ld_blend,ld_betas", [(145, 10), (148, 11), (160, 16), (176, 37)])
def test_b3_pose_entries_strides(ld_blend, ld_betas, B, aa):
    """Both pose entries (the axis-angle one had no test): blend row, A and joints16 against the reference's intermediates;
    columns [145, ld_blend) are zero, nothing is written past a row's end or the last row (four hands per workgroup)."""
    name = "real_l"
    rot, ax, betas, cam, K = MC.inputs(B, 400 + B, sigma=3.0)
    pose = ax if aa else rot
    blend, A, j16 = _pose(name, pose, betas, B, aa, ld_betas, ld_blend)
    ref = _Ref(name, O.TIP_IDS, pose, betas, cam, K, aa)
    kernel, case = ("mano_pose_aa" if aa else "mano_pose"), f"B3 B={B} ld_blend={ld_blend} ld_betas={ld_betas}"
    row = blend.get()
    assert torch.all(row[:, 145:] == 0), (kernel, case, "padding columns are not zero")
    ref.check(kernel, case, "blend_row", row[:, :145].contiguous())
    assert torch.equal(row[:, :10], betas), (kernel, case, "betas are copied")
    ref.check(kernel, case, "A", A.get())
    ref.check(kernel, case, "joints16", j16.get())


@pytest.mark.parametrize("ld_vp", [2334, 2336, 2340])
def test_b3_skin_entry_stride_and_chain_against_fused(ld_vp):
    """pose -> blend GEMM -> skin with the general K and the edge tips; v_posed rows ``ld_vp`` apart with NaN in the gaps.
    Every output against the reference, and against the fused launch at the existing 5e-7 on the vertices (same math, another
    k order in the blend product)."""
    L = _lib.lib()
    name, B, tips = "dense_l", 5, MC.EDGE_TIPS
    rot, _, betas, cam, K = MC.inputs(B, 500, sigma=3.0)
    _, mp, consts = _asset(name, tips)
    blend, A, j16 = _pose(name, rot, betas, B, False, 10, 160)
    torch.cuda.synchronize()
    blend_in = blend.buf[BAND:BAND + B * 160].clone()
    vposed = torch.empty(B, 2336, device=DEV)
    DEFAULT_ENGINE.conv(L, mp["blend"], blend_in, B, 1, 1, vposed, False, _stream())
    torch.cuda.synchronize()
    vp_i = In(strided(vposed.cpu()[:, :2334].contiguous(), ld_vp, float("nan")))
    cam_i, K_i = In(cam), In(K.reshape(B, 9))
    o = _outs(B)
    mo = _mano_out(o)
    check(L.hands_mano_skin_f32(C.byref(consts), vp_i.ptr(), ld_vp, A.ptr(), j16.ptr(), cam_i.ptr(), K_i.ptr(), 224.0, MIN_S,
                                C.byref(mo), B, _stream()), "mano_skin")
    ref = _Ref(name, tips, rot, betas, cam, K, False)
    got = ref.check_all("mano_skin", f"B3 chain ld_vp={ld_vp}", o, tips)
    fused = _fused((name,), tips, rot, betas, cam, K, B, False)[0]
    fv = fused["vertices"].get()
    _close("mano_skin", f"B3 chain ld_vp={ld_vp} vertices vs fused", got["vertices"], fv, 5e-7)
    assert torch.equal(got["cam_t"], fused["cam_t"].get())


# ---- B4: camera ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_res", [224.0, 256.0, 192.5])
@pytest.mark.parametrize("min_s", [0.1, 0.25])
def test_b4_camera_clamp(min_s, img_res):
    """cam[:, 0] at min_s, one ulp either side, +-0, negative and large: cam_t has the bits of the float32 evaluation of the
    reference (each operation of the kernel's expression is one IEEE float32 operation), the other outputs keep their bounds."""
    ms = torch.tensor(min_s, dtype=torch.float32)
    scales = torch.stack([ms, torch.nextafter(ms, torch.tensor(0.0)), torch.nextafter(ms, torch.tensor(1.0)), torch.tensor(0.0),
                          torch.tensor(-0.0), torch.tensor(-0.5), torch.tensor(3.0)])
    B = scales.numel()
    rot, _, betas, cam, K = MC.inputs(B, 600, sigma=1.0)
    K = K[:1].repeat(B, 1, 1)                                # one focal length: cam_t.z depends on the scale alone
    cam[:, 0] = scales
    assert cam[4, 0].item() == 0.0 and torch.signbit(cam[4, 0])
    m32 = R._f32(min_s)
    outs = _fused(("syn_r",), O.TIP_IDS, rot, betas, cam, K, B, False, img_res=img_res, min_s=m32)[0]
    ref = _Ref("syn_r", O.TIP_IDS, rot, betas, cam, K, False, img_res=img_res, min_s=m32)
    got = ref.check_all("mano_heads", f"B4 min_s={min_s} img_res={img_res}", outs, O.TIP_IDS)
    with R.precision(torch.float32):
        want32 = ref.f32("cam_t")
    diff = (got["cam_t"] != want32).sum().item()
    print(f"EDGE|mano_heads|B4 min_s={min_s} img_res={img_res} cam_t elements off the fp32 evaluation|{diff}|0")
    assert torch.equal(got["cam_t"], want32)
    # at and below min_s the clamp gives one value; -0.0, 0.0 and -0.5 are clamped too
    z = got["cam_t"][:, 2]
    assert z[0] == z[1] == z[3] == z[4] == z[5] and z[2] <= z[0] and z[6] < z[2]


# ---- B5: rejections -----------------------------------------------------------------------------------------------------------
def test_b5_rejections_launch_nothing():
    """Every HANDS_EINVAL condition of the four entries (include/hands_hip.h), the alignment ones included: nothing is launched."""
    L = _lib.lib()
    s = Scratch()
    x, o = ptr(s.x), ptr(s.o)
    st = _stream()
    consts_fields = [n for n, _ in _lib.ManoConsts._fields_]
    out_fields = [n for n, _ in _lib.ManoOut._fields_]

    def consts(**kw):
        c = _lib.ManoConsts(*[x] * 5)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def mout(**kw):
        m = _lib.ManoOut(o, ptr(s.o, 8192), ptr(s.o, 16384), ptr(s.o2), ptr(s.o2, 8192), ptr(s.o2, 16384))
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    # the pose entries: (c, pose, betas, ld_betas, blend_in, ld_blend, A, joints16, B)
    for fn in (L.hands_mano_pose_f32, L.hands_mano_pose_aa_f32):
        good = [C.byref(consts()), x, x, 10, o, 145, ptr(s.o, 8192), ptr(s.o2), 2, st]
        bad = []
        for i in (0, 1, 2, 4, 6, 7):
            bad.append(good[:i] + [None] + good[i + 1:])
        for f in ("pose_mean", "J_template", "J_shapedirs"):
            bad.append([C.byref(consts(**{f: None}))] + good[1:])
        bad += [good[:3] + [9] + good[4:], good[:3] + [0] + good[4:], good[:5] + [144] + good[6:], good[:8] + [0, st], good[:8] + [-3, st]]
        for a in bad:
            assert fn(*a) == EINVAL, a
    # the skin entry: (c, v_posed, ld_vp, A, joints16, cam_wp, K, img_res, min_s, out, B)
    good = [C.byref(consts()), x, 2334, x, x, x, x, 224.0, 0.1, C.byref(mout()), 2, st]
    bad = [good[:i] + [None] + good[i + 1:] for i in (0, 1, 3, 4, 5, 6, 9)]
    bad += [[C.byref(consts(**{f: None}))] + good[1:] for f in ("lbs_weights", "tip_ids")]
    bad += [good[:9] + [C.byref(mout(**{f: None}))] + good[10:] for f in out_fields]
    bad += [good[:2] + [2333] + good[3:], good[:10] + [0, st], good[:10] + [-1, st]]
    bad += [[C.byref(consts(lbs_weights=x + off))] + good[1:] for off in (4, 8, 12)]        # 16-byte loads of the weights
    for a in bad:
        assert L.hands_mano_skin_f32(*a) == EINVAL, a
    # the fused entry: (sides, n_sides, K, ld_betas, img_res, min_s, B, axis_angle_input)
    side_fields = ("blend_w", "blend_bias", "rot", "betas", "cam_wp")

    def sides(n=2, cons=None, out=None, **kw):
        arr = (_lib.ManoSide * 2)()
        for i in range(2):
            arr[i] = _lib.ManoSide(consts(), x, x, x, x, x, mout())
        last = arr[n - 1]
        if cons is not None:
            last.consts = cons
        if out is not None:
            last.out = out
        for k, v in kw.items():
            setattr(last, k, v)
        return arr

    def fused(arr, n=2, K=x, ld=10, B=2, aa=0):
        return L.hands_mano_heads_f32(arr, n, K, ld, 224.0, 0.1, B, aa, st)

    assert fused(None) == EINVAL and fused(sides(), n=0) == EINVAL and fused(sides(), n=3) == EINVAL and fused(sides(), n=-1) == EINVAL
    assert fused(sides(), K=None) == EINVAL and fused(sides(), ld=9) == EINVAL and fused(sides(), B=0) == EINVAL
    assert fused(sides(), B=-5) == EINVAL and fused(sides(), B=-5, aa=1) == EINVAL
    for n in (1, 2):                                         # a bad member of the last side that is read
        for f in consts_fields:
            assert fused(sides(n, cons=consts(**{f: None})), n=n) == EINVAL, (n, f)
        for f in out_fields:
            assert fused(sides(n, out=mout(**{f: None})), n=n) == EINVAL, (n, f)
        for f in side_fields:
            assert fused(sides(n, **{f: None}), n=n) == EINVAL, (n, f)
        # alignment: the vertex arrays are stored 8 bytes wide, the blend matrix is loaded 16 bytes wide
        assert fused(sides(n, out=mout(vertices=o + 4)), n=n) == EINVAL and fused(sides(n, out=mout(v3d_cam=o + 4)), n=n) == EINVAL
        assert fused(sides(n, out=mout(vertices=o + 12)), n=n) == EINVAL
        for off in (4, 8, 12):
            assert fused(sides(n, blend_w=x + off), n=n) == EINVAL, (n, off)
    assert s.untouched()


def test_b5_the_project_s_own_buffers_meet_the_alignment():
    """hands_amd.mano_head lays the twelve outputs out in one allocation: the vertex arrays of both sides are 8-byte aligned
    for every batch size, so the new refusals never meet the package's own calls."""
    from hands_amd.mano_head import _mano_out_buffers
    for bz in (1, 2, 3, 5, 16, 37):
        for side in _mano_out_buffers(bz, DEV):
            assert side["vertices"].data_ptr() % 8 == 0 and side["v3d.cam"].data_ptr() % 8 == 0, bz
    for name in ("syn_r", "real_l"):
        _, mp, _ = _asset(name)
        assert mp["blend"].w.data_ptr() % 16 == 0 and mp["lbs_weights"].data_ptr() % 16 == 0
