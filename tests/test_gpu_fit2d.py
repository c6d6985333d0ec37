"""hands_mano_fit2d_f32 and what stands on it (hands_amd/fitting.py, ``fit_gt_2d`` in HandsWrapper, ``refine_predictions``) on the
device against the fp64 restatement (tests/fit2d_ref.py) of DESIGN.md section 7 "MANO fitting to 2-D keypoints".

Bars.  The rule of tests/test_gpu_fitting.py: the kernel computes in fp64 what the restatement computes and rounds once to
fp32, so per float output the bar is max(4 * 2^-24 * max(1, |ref|), 16 x the largest difference between the restatement and
its noise = 1e-15 twin on the same inputs, per output kind); ``steps`` and ``start`` are equal.  ``rmse``, ``j2d`` and
``transl`` are O(1..100), so the relative form of the floor matters.  The twin, measured on the CPU:
  step parity (fit2d_ref.step_parity_inputs, bases 100 / 200, all four stage pairs and three configurations): at most 1.3e-10 on
  rotation entries, 6.6e-12 on beta, 6.6e-14 on the translation, 3.1e-9 px on the rmse, 1.5e-11 m on j3d, 1.6e-8 px on j2d;
  full run (fit2d_ref.FULL_SEEDS = 1..8 at 6 + 14 iterations): 1.3e-10, 1.1e-10, 8.7e-13, 5.8e-10 px, 6.3e-12 m, 1.8e-9 px, and
  the same number of steps on all 8 rows.
16 x that stays below the floor everywhere, so the floor is the bar of every output.
The kernel on an MI355X, as the largest share of the bar: step parity 0.125 (pose), 0.247 (beta), 0.140 (transl), 0.222 (rmse),
0.238 (j3d), 0.245 (j2d); full run 0.125, 0.233, 0.116, 0.118, 0.161, 0.242 -- a quarter of the bar is the fp32 rounding of the
output itself (half an ulp, at most 2^-24 of the value), so the fp64 arithmetic adds nothing visible.
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

import fit2d_ref as G
import fit_ref as F
from edge_util import EINVAL, SENT, In, Out, OutInt

pytestmark = pytest.mark.gpu

CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs", "tip_lbs_weights", "tip_posedirs")
FLOATS = ("pose", "beta", "transl", "rmse", "j3d", "j2d")
OUT_ORDER = ("pose", "beta", "transl", "rmse", "steps", "start", "j3d", "j2d")
K1 = G.K_TEST.astype(np.float32)


def floor(ref):
    return 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def Ks(B):
    return np.repeat(K1[None], B, 0)


@pytest.fixture(scope="module")
def hands():
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], torch.device("cuda"))
    consts = [F.Consts(*[p[k].cpu().numpy() for k in CONST_KEYS]) for p in packs]
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": packs[0], "mano_l": packs[1]}, "img_res": 224})()
    return {"heads": heads, "packs": packs, "C": consts, "pair": pair}


def c_cfg(cfg):
    from hands_amd._lib import Fit2DCfg
    return Fit2DCfg(cfg["iters_rigid"], cfg["iters"], cfg["lambda_beta"], cfg["lambda_pose"], cfg["mu0"], cfg["robust_sigma"],
                    cfg["z_min"], int(cfg["fit_shape"]), int(cfg["prior_to_init"]))


def c_fit(sides, K, B, cfg=None, n_sides=None):
    """hands_mano_fit2d_f32 on guarded buffers.  sides: per side dict(pack, y, w=None, valid=None, init=None) of numpy arrays ->
    per side dict of numpy outputs (the bands around every output checked)."""
    from hands_amd import _lib
    from hands_amd._lib import ManoFit2DSide, ManoFitConsts, ptr
    cfg = cfg or G.config()
    f32 = lambda a: None if a is None else In(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    p = lambda b: None if b is None else b.ptr()
    Kin = f32(K)
    arr, keep, outs = (ManoFit2DSide * len(sides))(), [], []
    for i, s in enumerate(sides):
        ins = [f32(s["y"]), f32(s.get("w")), f32(s.get("valid"))] + [f32(a) for a in (s.get("init") or (None, None, None))]
        o = {"pose": Out(B, 16, 3, 3), "beta": Out(B, 10), "transl": Out(B, 3), "rmse": Out(B), "steps": OutInt(torch.int32, B),
             "start": OutInt(torch.int32, B), "j3d": Out(B, 21, 3), "j2d": Out(B, 21, 2)}
        arr[i] = ManoFit2DSide(ManoFitConsts(*[ptr(s["pack"][k]) for k in CONST_KEYS]), *[p(b) for b in ins],
                               *[o[k].ptr() for k in OUT_ORDER])
        keep.append(ins)
        outs.append(o)
    c = c_cfg(cfg)
    rc = _lib.lib().hands_mano_fit2d_f32(arr, n_sides or len(sides), Kin.ptr(), ctypes.byref(c), B, _stream())
    assert rc == 0, rc
    return [{k: v.get().numpy() for k, v in o.items()} for o in outs]


def close(what, got, ref_rows, twin_rows=None):
    """got: a side's outputs; ref_rows / twin_rows: the restatement's results per row.  Prints the narrowest margin per output."""
    for k in FLOATS:
        ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in ref_rows])
        g = np.asarray(got[k], np.float64)
        assert np.asarray(got[k]).dtype == np.float32 and g.shape == ref.shape, (what, k, g.shape, ref.shape)
        bnd, tw = floor(ref), 0.0
        if twin_rows is not None:
            with np.errstate(invalid="ignore"):
                tw = float(np.nanmax(np.abs(ref - np.stack([np.asarray(r["raw"][k], np.float64) for r in twin_rows])), initial=0.0))
            bnd = np.maximum(bnd, 16 * tw)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), (what, k, "NaN positions differ")
        fin = np.isfinite(ref)
        assert np.array_equal(g[~fin & ~nan], ref[~fin & ~nan]), (what, k, "infinities differ")
        with np.errstate(invalid="ignore"):
            ratio = np.where(fin, np.abs(g - ref) / bnd, 0.0)
        print(f"FIT2D|{what}|{k}|twin {tw:.3e}|{ratio.max():.3f} of the bar")
        assert (ratio <= 1.0).all(), (what, k, float(ratio.max()))
    for k in ("steps", "start"):
        assert np.array_equal(np.asarray(got[k]), np.array([r[k] for r in ref_rows], np.int32)), (what, k, got[k])


# ---- 1. step parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [(0, 0), (1, 0), (2, 1), (2, 3)])
def test_step_parity(hands, stages):
    """B = 5, both assets in one launch: the right hand from a caller's state with prior_to_init, the left from the generated
    start; uneven weights (rows 1, 4), five zero weights with NaN under them (row 2), a keypoint displaced by 80 px (row 3).
    Three launches, the configuration being per launch: plain, sigma = 30 px, fit_shape off; every row is compared in each."""
    for name, extra in (("plain", {}), ("sigma30", dict(robust_sigma=30.0)), ("noshape", dict(fit_shape=False))):
        cfg = G.config(iters_rigid=stages[0], iters=stages[1], prior_to_init=True, **extra)
        sides, refs, twins = [], [], []
        for i, (base, with_init) in enumerate(((100, True), (200, False))):
            y, w, init = G.step_parity_inputs(hands["C"][i], base, with_init)
            sides.append(dict(pack=hands["packs"][i], y=y, w=w, init=init))
            refs.append(G.fit_rows(hands["C"][i], y, Ks(5), w, init=init, cfg=cfg))
            twins.append(G.fit_rows(hands["C"][i], y, Ks(5), w, init=init, cfg=cfg, noise=1e-15, seed=5))
        assert all(G.margins_ok(r) for rr in refs for r in rr)                 # no tie decides
        got = c_fit(sides, Ks(5), 5, cfg)
        for i, h in enumerate("rl"):
            close(f"steps{stages[0]}+{stages[1]}.{name}.{h}", got[i], refs[i], twins[i])
        assert all(r["start"] == -1 for r in refs[0]) and all(0 <= r["start"] < 24 for r in refs[1])
        if stages == (2, 3):
            assert sum(r["steps"] for rr in refs for r in rr) >= 25            # the steps are real ones
            if name == "noshape":
                assert np.array_equal(bits(got[0]["beta"]), bits(sides[0]["init"][1])) and not got[1]["beta"].any()
        if stages[1] == 0:                                                     # a rigid stage alone: frozen unknowns keep their bits
            assert np.array_equal(bits(got[0]["pose"][:, 1:]), bits(sides[0]["init"][0][:, 1:]))
            assert np.array_equal(bits(got[0]["beta"]), bits(sides[0]["init"][1]))


# ---- 2. the full run -----------------------------------------------------------------------------------------------------------
def test_full_run_parity(hands):
    """6 + 14 iterations on the 8 seeds of fit2d_ref.FULL_SEEDS through hands_amd.fit_mano_2d.  Asserted of the reference first:
    every decision above 1e-9 c, the twin takes the same number of steps on at least 7 of the 8; ``steps`` is compared where
    the twin agrees."""
    import hands_amd
    C = hands["C"][0]
    y, w, ref, twin = G.full_run_reference(C)
    assert all(G.margins_ok(r) for r in ref)
    agree = np.array([a["steps"] == b["steps"] for a, b in zip(ref, twin)])
    assert agree.sum() >= 7
    out = hands_amd.fit_mano_2d(torch.from_numpy(y).cuda(), torch.from_numpy(Ks(8)).cuda(), hands["heads"][0], "r",
                                weights=torch.from_numpy(w).cuda(), config=hands_amd.Fit2DConfig(**G.FULL_CFG))
    assert list(out) == ["pose", "beta", "transl", "rmse", "steps", "start", "j3d", "j2d", "pose_aa"]
    got = {k: out[k].cpu().numpy() for k in OUT_ORDER}
    steps = got["steps"].copy()
    got["steps"] = np.where(agree, steps, np.array([r["steps"] for r in ref], np.int32))
    close("full", got, ref, twin)
    assert steps.dtype == np.int32 and steps.min() >= 8
    back = out["pose_aa"].cpu().numpy().astype(np.float64) + C.pose_mean
    again = np.stack([[F.exp_so3(row[3 * j:3 * j + 3]) for j in range(16)] for row in back])
    assert np.abs(again - got["pose"]).max() <= 1e-5                         # the fp32 quaternion route, as in test_gpu_fitting.py


# ---- 3. consistency with the LBS kernel ------------------------------------------------------------------------------------------
def test_fit_agrees_with_the_lbs_kernel(hands):
    """pose_aa, beta and transl (as the weak-perspective camera that gives it back) through hands_mano_heads_f32 with the same K:
    j3d.cam reproduces j3d within 2e-6 m (the LBS kernel's 6.9e-7 m against the oracle, the bar of test_gpu_fitting.py, plus
    the fp32 camera conversion: 2^-23 of a depth below 1 m); the un-normalised j2d.norm reproduces j2d within what 2e-6 m is
    in pixels, 2 * 2e-6 * f / Z_min of the row, plus 1e-4 px for the fp32 normalised coordinate (2^-24 of up to 5, times 112 px,
    twice); the weighted rms of that j2d against the keypoints is the reported rmse within the same pixel bar."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.fitting import _unnormalize
    from hands_amd.mano_head import ManoHeadsPlan
    B = 6
    ys, ws = [], []
    for i in range(2):
        y, w = zip(*[G.family_case(hands["C"][i], 40 + 10 * i + b)[:2] for b in range(B)])
        ys.append(np.stack(y))
        ws.append(np.stack(w))
    K = torch.from_numpy(Ks(B)).cuda()
    cfg = hands_amd.Fit2DConfig(iters_rigid=6, iters=14)
    fr, fl = hands_amd.fit_mano_hands_2d(torch.from_numpy(ys[0]).cuda(), torch.from_numpy(ys[1]).cuda(), K, hands["pair"],
                                         weights_r=torch.from_numpy(ws[0]).cuda(), weights_l=torch.from_numpy(ws[1]).cuda(), config=cfg)
    single = hands_amd.fit_mano_2d(torch.from_numpy(ys[1]).cuda(), K, hands["heads"][1], "l", weights=torch.from_numpy(ws[1]).cuda(),
                                   config=cfg)
    assert all(torch.equal(single[k], fl[k]) for k in single)          # one launch for both hands: the same bits
    rot = torch.cat([fr["pose_aa"], fl["pose_aa"]]).contiguous()
    shape = torch.cat([fr["beta"], fl["beta"]]).contiguous()
    t = torch.cat([fr["transl"], fl["transl"]]).double()
    cam = torch.stack([(2.0 * 1000.0 / t[:, 2] - 1e-9) / 224.0, t[:, 0], t[:, 1]], 1).float().contiguous()
    out = ManoHeadsPlan(_lib.lib(), hands["packs"][0], hands["packs"][1], rot, shape, cam, K.contiguous(), 224.0, B, aa_input=True).launch(_stream())
    for i, (h, f) in enumerate((("r", fr), ("l", fl))):
        j3d = f["j3d"].cpu().numpy().astype(np.float64)
        e3 = np.abs(out[f"mano.j3d.cam.{h}"].cpu().numpy() - j3d).max()
        px = _unnormalize(out[f"mano.j2d.norm.{h}"], 224.0).cpu().numpy().astype(np.float64)
        bar_px = 2 * 2e-6 * 1000.0 / j3d[:, :, 2].min(1) + 1e-4
        e2 = np.abs(px - f["j2d"].cpu().numpy()).max((1, 2))
        w = ws[i].astype(np.float64)
        with np.errstate(invalid="ignore"):
            d2 = np.where(w[..., None] > 0, (px - ys[i]) ** 2, 0.0).sum(2)
        rms = np.sqrt((w * d2).sum(1) / w.sum(1))
        er = np.abs(rms - f["rmse"].cpu().numpy())
        print(f"FIT2D|lbs|{h}|j3d {e3:.3e}|2e-6|j2d {(e2 / bar_px).max():.3f} of the bar|rmse {(er / bar_px).max():.3f} of the bar")
        assert e3 <= 2e-6 and (e2 <= bar_px).all() and (er <= bar_px).all() and j3d[:, :, 2].min() > 0.05


# ---- 4. independence and reproducibility -------------------------------------------------------------------------------------------
def test_a_hand_does_not_depend_on_its_neighbours(hands):
    cfg = G.config(iters_rigid=3, iters=5)
    C, pack = hands["C"][0], hands["packs"][0]
    y1, w1, _ = G.family_case(C, 31)
    alone = c_fit([dict(pack=pack, y=y1[None], w=w1[None])], Ks(1), 1, cfg)[0]
    assert alone["steps"][0] >= 4 and alone["start"][0] >= 0
    B, at = 5, (0, 2, 4)
    ys, ws = zip(*[G.family_case(C, 300 + b)[:2] for b in range(B)])
    y, w, valid = np.stack(ys), np.stack(ws), np.ones(B, np.float32)
    valid[1] = 0.0                                                     # an unfitted row next to it
    y[3] = np.nan                                                      # and one that is not finite
    K = Ks(B)
    K[1], K[3] = 2.0 * K[1], np.nan                                    # the neighbours' intrinsics are their own
    for b in at:
        y[b], w[b] = y1, w1
    yl, wl = zip(*[G.family_case(hands["C"][1], 400 + b)[:2] for b in range(B)])
    one = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], K, B, cfg)[0]
    two = c_fit([dict(pack=hands["packs"][1], y=np.stack(yl), w=np.stack(wl)), dict(pack=pack, y=y, w=w, valid=valid)], K, B, cfg)
    again = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], K, B, cfg)[0]
    for k in FLOATS:
        for b in at:
            assert np.array_equal(bits(one[k][b]), bits(alone[k][0])), (k, b)
        assert np.array_equal(bits(one[k]), bits(two[1][k])) and np.array_equal(bits(one[k]), bits(again[k])), k
    for k in ("steps", "start"):
        assert np.array_equal(one[k], two[1][k]) and np.array_equal(one[k], again[k])
        assert all(one[k][b] == alone[k][0] for b in at)
    assert np.isnan(one["rmse"][[1, 3]]).all() and np.isfinite(one["rmse"][[0, 2, 4]]).all()


# ---- 5. the rules ----------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_fitted(hands):
    cfg = G.config(iters_rigid=2, iters=2)
    C, pack = hands["C"][1], hands["packs"][1]
    B = 12
    ys, ws = zip(*[G.family_case(C, 500 + b)[:2] for b in range(B)])
    y, w, valid, K = np.stack(ys), np.ones((B, 21), np.float32), np.ones(B, np.float32), Ks(B)
    valid[1] = 0.0
    w[2] = 0.0
    w[2, [0, 7, 20]] = 1.0                                             # three weighted keypoints: not fitted
    y[3, 9, 1] = np.nan                                                # a NaN in a weighted keypoint
    y[7, 0, 0] = np.inf
    w[4, [2, 16]] = 0.0
    w[5, [2, 16]] = 0.0
    y[5] = y[4]
    y[4, [2, 16]] = np.nan                                             # NaN under weight 0: must not matter
    w[6] = 0.0
    w[6, [0, 4, 9, 18]] = 2.0                                          # four weighted keypoints: fitted
    K[8, 0, 1], K[9, 0, 0], K[10, 1, 1] = np.nan, 0.0, -1000.0         # intrinsics: not finite, K00 <= 0, K11 <= 0
    K[0, 2] = np.nan                                                   # row 2 of K is never read
    w[11] = 0.0
    w[11, [0, 4, 9, 18]] = 1.0
    y[11] = y[11, 0]                                                   # coincident keypoints: no start candidate qualifies
    got = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], K, B, cfg)[0]
    ref = G.fit_rows(C, y, K, w, valid, cfg=cfg)
    close("rules", got, ref)
    unfitted = G.unfitted(C)
    bad = (1, 2, 3, 7, 8, 9, 10, 11)
    for b in bad:
        assert got["steps"][b] == 0 and got["start"][b] == -1 and np.isnan(got["rmse"][b])
        assert np.isnan(got["j3d"][b]).all() and np.isnan(got["j2d"][b]).all()
        for k in ("pose", "beta", "transl"):
            assert np.array_equal(bits(got[k][b]), bits(unfitted[k])), (b, k)
    assert np.isfinite(got["rmse"][[0, 4, 5, 6]]).all() and got["steps"][4] >= 1 and (got["start"][[0, 4, 5, 6]] >= 0).all()
    for k in FLOATS:
        assert np.array_equal(bits(got[k][4]), bits(got[k][5])), k
    # weights = NULL and valid = NULL: every keypoint at weight 1, every row fitted
    plain = c_fit([dict(pack=pack, y=y[[0, 5]])], K[[0, 5]], 2, cfg)[0]
    close("rules.null", plain, G.fit_rows(C, y[[0, 5]], K[[0, 5]], cfg=cfg))
    ones = c_fit([dict(pack=pack, y=y[[0, 5]], w=np.ones((2, 21), np.float32), valid=np.ones(2, np.float32))], K[[0, 5]], 2, cfg)[0]
    assert all(np.array_equal(bits(plain[k]), bits(ones[k])) for k in FLOATS)
    # an initial state that is not finite, and one behind z_min: those rows alone are not fitted
    _, _, init = G.step_parity_inputs(C, 500, True)
    init = tuple(a[:4].copy() for a in init)
    init[0][1, 7, 1, 1] = np.nan
    init[2][2, 0] = -np.inf
    init[2][3, 2] = -0.5                                               # behind the camera: weighted joints at Z <= z_min
    got = c_fit([dict(pack=pack, y=y[[0, 5, 6, 0]], w=w[[0, 5, 6, 0]], init=init)], K[:4], 4, cfg)[0]
    close("rules.init", got, G.fit_rows(C, y[[0, 5, 6, 0]], K[:4], w[[0, 5, 6, 0]], init=init, cfg=cfg))
    assert np.isfinite(got["rmse"][0]) and np.isnan(got["rmse"][1:]).all() and (got["start"] == -1).all()


def test_rejected_calls_write_nothing(hands):
    from hands_amd import _lib
    from hands_amd._lib import Fit2DCfg, ManoFit2DSide, ManoFitConsts, ptr
    L, B = _lib.lib(), 2
    pack = hands["packs"][0]
    x = torch.zeros(B * 144, device="cuda")
    Kd = torch.from_numpy(Ks(B)).cuda()
    outs = {k: torch.full((B * 144,), SENT, device="cuda") for k in FLOATS}
    ints = {k: torch.full((B * 4,), -77777, dtype=torch.int32, device="cuda") for k in ("steps", "start")}
    good = (3, 3, 1e-2, 1e-2, 1e-3, 0.0, 0.05, 1, 0)

    def side(**drop):
        f = {k: ptr(pack[k]) for k in CONST_KEYS}
        f.update(kp2d=ptr(x), weights=None, valid=None, init_pose=None, init_beta=None, init_transl=None,
                 **{k: ptr(v) for k, v in outs.items()}, **{k: ptr(v) for k, v in ints.items()})
        f.update(drop)
        return ManoFit2DSide(ManoFitConsts(*[f[k] for k in CONST_KEYS]),
                             *[f[k] for k in ("kp2d", "weights", "valid", "init_pose", "init_beta", "init_transl") + OUT_ORDER])

    def call(sides=None, n=1, cfg=good, rows=B, null_sides=False, null_cfg=False, null_K=False):
        arr = (ManoFit2DSide * 2)(*(sides or [side(), side()]))
        c = Fit2DCfg(*cfg)
        return L.hands_mano_fit2d_f32(None if null_sides else arr, n, None if null_K else ptr(Kd), None if null_cfg else ctypes.byref(c),
                                      rows, _stream())

    nan, inf = float("nan"), float("inf")
    with_ = lambda i, v: tuple(v if j == i else c for j, c in enumerate(good))
    cases = [("sides", dict(null_sides=True)), ("cfg", dict(null_cfg=True)), ("K", dict(null_K=True))]
    cases += [(k, dict(sides=[side(**{k: None}), side()])) for k in CONST_KEYS + ("kp2d",) + OUT_ORDER]
    cases += [("second side", dict(sides=[side(), side(kp2d=None)], n=2))]
    cases += [("init " + "".join(k[5] for k in given), dict(sides=[side(**{k: ptr(x) for k in given}), side()]))
              for given in (("init_pose",), ("init_beta",), ("init_transl",), ("init_pose", "init_beta"),
                            ("init_pose", "init_transl"), ("init_beta", "init_transl"))]
    cases += [("B 0", dict(rows=0)), ("B -1", dict(rows=-1)), ("n_sides 0", dict(n=0)), ("n_sides 3", dict(n=3)),
              ("n_sides -1", dict(n=-1)), ("iters", dict(cfg=with_(1, -1))), ("iters_rigid", dict(cfg=with_(0, -1)))]
    cases += [(f"cfg[{i}] {v}", dict(cfg=with_(i, v))) for i in (2, 3, 4, 5) for v in (-1e-9, nan, inf, -inf)]
    cases += [(f"z_min {v}", dict(cfg=with_(6, v))) for v in (0.0, -0.05, nan, inf, -inf)]
    for name, kw in cases:
        assert call(**kw) == EINVAL, name
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in outs.values()) and all(bool((v == -77777).all()) for v in ints.values())
    assert call(sides=[side(**{k: ptr(x) for k in ("init_pose", "init_beta", "init_transl")}), side()]) == 0      # the table's complement
    assert call(n=2, cfg=(0, 0, 0.0, 0.0, 0.0, 0.0, 1e-3, 0, 0)) == 0
    torch.cuda.synchronize()


# ---- 6. the callers --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(recipe_model):
    return copy.deepcopy(recipe_model).to("cuda")


def _annotation(model, B, base):
    """Per hand: normalised keypoints (B,21,2) the model's own MANO assets generate, and K."""
    P = model.packed(torch.device("cuda"))
    norm = {}
    for h in "rl":
        C = F.Consts(*[P[f"mano_{h}"][k].cpu().numpy() for k in CONST_KEYS])
        px = np.stack([G.family_case(C, base + 10 * (h == "l") + b)[0] for b in range(B)])
        norm[h] = (2.0 * px / 224.0 - 1.0).astype(np.float32)
    return norm, torch.from_numpy(Ks(B)).cuda()


def test_fit_targets_2d_and_the_wrapper(model):
    """A 2-D-only batch (mano.j3d.full zeroed, dummy pose and beta): fit_gt_2d yields the full target dict, and the joints the
    MANO kernel builds from it, placed at the fitted translation and projected, reproduce the annotation to the fit's rmse --
    within 1e-2 px (2e-6 m of the fp32 LBS kernel at f / Z < 2.5e3, test 3) in the weighted rms."""
    import hands_amd
    from hands_amd.wrapper import HandsWrapper
    B = 3
    norm, K = _annotation(model, B, 600)
    targets = hands_amd.xdict({f"mano.j2d.norm.{h}": torch.from_numpy(norm[h]).cuda() for h in "rl"})
    for h in "rl":
        targets[f"mano.j3d.full.{h}"] = torch.zeros(B, 21, 3).cuda()
        targets[f"mano.pose.{h}"] = torch.zeros(B, 48).cuda()
        targets[f"mano.beta.{h}"] = torch.zeros(B, 10).cuda()
    before = {k: v.clone() for k, v in targets.items()}
    cfg = hands_amd.Fit2DConfig(iters_rigid=6, iters=14)
    meta = {"intrinsics": K, "right_valid": torch.tensor([1.0, 1.0, 0.0]).cuda()}
    t = hands_amd.fit_targets_2d(targets, model, meta, config=cfg)
    assert t is not targets and list(targets) == list(before) and all(torch.equal(targets[k], before[k]) for k in before)
    fr, fl = hands_amd.fit_mano_hands_2d(*[(0.5 * 224.0 * (targets[f"mano.j2d.norm.{h}"] + 1.0)) for h in "rl"], K, model,
                                         valid_r=meta["right_valid"], config=cfg)
    for h, f in (("r", fr), ("l", fl)):
        for key, k in (("mano.pose", "pose_aa"), ("mano.beta", "beta"), ("mano.j3d.full", "j3d"), ("mano.fit.rmse_px", "rmse"),
                       ("mano.fit.transl", "transl")):
            assert torch.equal(t[f"{key}.{h}"].view(torch.int32), f[k].view(torch.int32)), (key, h)
    assert bool(torch.isnan(t["mano.fit.rmse_px.r"][2])) and bool(torch.isfinite(t["mano.fit.rmse_px.r"][:2]).all())
    assert bool(torch.isfinite(t["mano.fit.rmse_px.l"]).all())

    w = HandsWrapper(model=model)
    assert w.fit_gt_2d is None
    w.fit_gt_2d = cfg
    full = w.process_data(targets, {"intrinsics": K})
    assert all(torch.equal(targets[k], before[k]) for k in before)
    Kd = K.double()
    for h in "rl":
        v = full[f"mano.vertices.{h}"]
        assert v.shape == (B, 778, 3) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(full[f"mano.v3d.cam.{h}"]).all())
        X = full[f"mano.joints3d.{h}"].double() + full[f"mano.fit.transl.{h}"].double()[:, None]
        uv = torch.stack([Kd[:, 0, 0, None] * X[..., 0] / X[..., 2] + Kd[:, 0, 2, None],
                          Kd[:, 1, 1, None] * X[..., 1] / X[..., 2] + Kd[:, 1, 2, None]], -1)
        ann = 0.5 * 224.0 * (targets[f"mano.j2d.norm.{h}"].double() + 1.0)
        rms = (uv - ann).pow(2).sum(2).mean(1).sqrt()
        rmse = full[f"mano.fit.rmse_px.{h}"].double()
        print(f"FIT2D|wrapper|{h}|rmse {rmse.max().item():.3e}|rms {rms.max().item():.3e}")
        assert bool((rms <= rmse + 1e-2).all()) and bool(torch.isfinite(rmse).all()), (h, rms, rmse)
        assert torch.equal(full[f"mano.j3d.cam.{h}"], full[f"mano.j3d.full.{h}"])
    w.fit_gt = hands_amd.FitConfig()
    with pytest.raises(ValueError, match="fit_gt and fit_gt_2d"):
        w.process_data(targets, {"intrinsics": K})
    w.fit_gt = w.fit_gt_2d = None
    given = hands_amd.xdict(dict(targets))
    assert w.process_data(given, {"intrinsics": K}) is given and not any("mano.fit." in k for k in given)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano_2d(torch.zeros(B, 21, 2).cuda(), K, model, "r", weights=torch.ones(B, 21))




def _prediction(hands, B):
    """A prediction dict as the MANO head gives it (hands_mano_heads_f32 on chosen parameters: family cases moved off their truth)
    plus two keys of other heads, and the keypoints: the projection of the truth."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import run_mano_heads
    rng = np.random.RandomState(11)
    rot, shape, cam, kp = [], [], [], {}
    for i, h in enumerate("rl"):
        C = hands["C"][i]
        ys = []
        for b in range(B):
            y, _, (R, beta, t) = G.family_case(C, 700 + 10 * i + b)
            ys.append(y)
            full = np.concatenate([F.log_so3(R[j] @ F.exp_so3(0.1 * rng.randn(3))) for j in range(16)]) - C.pose_mean
            rot.append(np.stack([F.exp_so3(full[3 * j:3 * j + 3]) for j in range(16)]))
            shape.append(beta + 0.3 * rng.randn(10))
            t = t + 0.02 * rng.randn(3)
            cam.append([2.0 * 1000.0 / (224.0 * t[2]), t[0], t[1]])
        kp[h] = torch.from_numpy(np.stack(ys)).cuda()
    dev = lambda a: torch.from_numpy(np.asarray(a, np.float32)).cuda().contiguous()
    rot, shape, cam, K = dev(rot), dev(shape), dev(cam), dev(Ks(B))
    pred = hands_amd.xdict(run_mano_heads(_lib.lib(), hands["packs"][0], hands["packs"][1], rot, shape, cam, cam, K, 224.0, B, _stream(), None))
    pred["grasp.r"] = torch.arange(B, dtype=torch.float32).cuda()
    pred["grasp.l"] = torch.ones(B, 3).cuda()
    return pred, kp, K


def test_refine_predictions_and_graph_replay(hands):
    """A prediction refined onto keypoints: keys and order of ``pred`` (+ refined.{r,l}); every key that is not one of the nine
    MANO-head keys is the tensor of ``pred``; rows that are not fitted keep the prediction's tensors bit for bit; the refined
    rows' j2d.norm is closer to the keypoints than the prediction's; a torch.cuda.graph replay of the fit gives the eager bits."""
    import hands_amd
    from hands_amd.smoothing import HEAD_KEYS
    B = 4
    pred, kp, K = _prediction(hands, B)
    assert len(pred) == 22
    valid_r = torch.tensor([1.0, 0.0, 1.0, 1.0]).cuda()
    kp["l"][2, 5, 0] = float("nan")                                      # a row with a non-finite keypoint
    out = hands_amd.refine_predictions(pred, kp["r"], kp["l"], hands["pair"], {"intrinsics": K}, valid_r=valid_r)
    assert isinstance(out, hands_amd.xdict) and list(out) == list(pred) + ["refined.r", "refined.l"]
    head = [f"mano.{k}.{h}" for h in "rl" for k in HEAD_KEYS]
    for k in pred:
        assert (k in head) or out[k] is pred[k], k
    assert out["refined.r"].dtype == torch.bool and out["refined.r"].tolist() == [True, False, True, True]
    assert out["refined.l"].tolist() == [True, True, False, True]
    kp["l"][2, 5, 0] = 0.0
    for h in "rl":
        moved = out[f"refined.{h}"]
        for k in HEAD_KEYS:
            a, b = out[f"mano.{k}.{h}"], pred[f"mano.{k}.{h}"]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(a[~moved].view(torch.int32), b[~moved].view(torch.int32)), (k, h)
        d = lambda t: (0.5 * 224.0 * (t[f"mano.j2d.norm.{h}"].double() + 1.0) - kp[h].double())[moved].pow(2).sum(2).mean(1).sqrt()
        print(f"FIT2D|refine|{h}|before {d(pred).tolist()}|after {d(out).tolist()}")
        assert bool((d(out) < d(pred)).all())
        assert not torch.equal(out[f"mano.vertices.{h}"][moved], pred[f"mano.vertices.{h}"][moved])
    # capture: the fit launch and its axis-angle launch, no allocation outside the graph's pool, no host synchronisation
    cfg = hands_amd.Fit2DConfig(iters_rigid=2, iters=3)
    eager = hands_amd.fit_mano_hands_2d(kp["r"], kp["l"], K, hands["pair"], valid_r=valid_r, config=cfg)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream, no parallel branches
        cap = hands_amd.fit_mano_hands_2d(kp["r"], kp["l"], K, hands["pair"], valid_r=valid_r, config=cfg)
    for f in cap:
        for v in f.values():
            v.fill_(-3)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, cap):
        for k in a:
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
        assert int(a["steps"].sum()) >= 4
