"""hands_mano_fit_f32 and what stands on it (hands_amd/fitting.py, ``fit_gt`` in HandsWrapper) on the device against the fp64
restatement (tests/fit_ref.py) of DESIGN.md section 7 "MANO fitting".

Bars.  The kernel computes in fp64 what the restatement computes and rounds once to fp32; the two differ by device-versus-host
libm and by the order of fp64 sums.  The damped system's condition is at most 61 / mu <= 1.7e6 at mu >= 1e-3 / 27, and the
restatement with every residual and Jacobian entry perturbed by 1e-15 moves no output by more than 1.1e-10 in three iterations,
so the fp32 rounding of the output dominates: BAR = 4 * 2^-24 * max(1, |ref|) per float output, the fourfold margin of
tests/test_gpu_smoothing.py; ``steps`` is equal.  The inputs are those of tests/test_fitting.py, where every accept / reject
decision of the restatement has a margin above 1e-9 of the cost.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import fit_ref as F
from edge_util import EINVAL, SENT, In, Out, OutInt

pytestmark = pytest.mark.gpu

CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "tip_v_template", "tip_shapedirs", "tip_lbs_weights", "tip_posedirs")
FLOATS = (("pose", (16, 3, 3)), ("beta", (10,)), ("transl", (3,)), ("rmse", ()))


def bar(ref):
    return 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def hands():
    """Per side: the MANO head, its packed constants on the device and the restatement's constants read back from them."""
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], torch.device("cuda"))
    consts = [F.Consts(*[p[k].cpu().numpy() for k in CONST_KEYS]) for p in packs]
    return {"heads": heads, "packs": packs, "C": consts}


def c_fit(sides, B, cfg=None, n_sides=None):
    """hands_mano_fit_f32 on guarded buffers.  sides: per side dict(pack, y, w=None, valid=None, init=None) of numpy arrays ->
    per side dict of numpy outputs (the bands around every output checked)."""
    from hands_amd import _lib
    from hands_amd._lib import FitCfg, ManoFitConsts, ManoFitSide, ptr
    cfg = cfg or F.config()
    f32 = lambda a: None if a is None else In(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    p = lambda b: None if b is None else b.ptr()
    arr, keep, outs = (ManoFitSide * len(sides))(), [], []
    for i, s in enumerate(sides):
        ins = [f32(s["y"]), f32(s.get("w")), f32(s.get("valid"))] + [f32(a) for a in (s.get("init") or (None, None, None))]
        o = {"pose": Out(B, 16, 3, 3), "beta": Out(B, 10), "transl": Out(B, 3), "rmse": Out(B), "steps": OutInt(torch.int32, B)}
        arr[i] = ManoFitSide(ManoFitConsts(*[ptr(s["pack"][k]) for k in CONST_KEYS]), *[p(b) for b in ins],
                             *[o[k].ptr() for k in ("pose", "beta", "transl", "rmse", "steps")])
        keep.append(ins)
        outs.append(o)
    c = FitCfg(cfg["iters"], cfg["lambda_beta"], cfg["lambda_pose"], cfg["mu0"])
    rc = _lib.lib().hands_mano_fit_f32(arr, n_sides or len(sides), ctypes.byref(c), B, _stream())
    assert rc == 0, rc
    return [{k: v.get().numpy() for k, v in o.items()} for o in outs]


def close(what, got, ref_rows):
    """got: a side's outputs; ref_rows: the restatement's results per row.  Prints the narrowest margin per output."""
    for k, _ in FLOATS:
        ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in ref_rows])
        g = got[k].astype(np.float64)
        assert got[k].dtype == np.float32 and g.shape == ref.shape, (what, k, g.shape, ref.shape)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), (what, k, "NaN positions differ")
        ratio = np.where(nan, 0.0, np.abs(g - ref) / bar(ref))
        print(f"FIT|{what}|{k}|{ratio.max():.3f} of the bar")
        assert (ratio <= 1.0).all(), (what, k, float(ratio.max()))
    assert np.array_equal(got["steps"], np.array([r["steps"] for r in ref_rows], np.int32)), (what, got["steps"])


# ---- 1. step parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2, 3])
def test_step_parity(hands, iters):
    """B = 5, both assets in one launch, uneven and zero weights (NaN coordinates under the zeros), the right hand from a
    caller's initial state, the left from the Kabsch state."""
    cfg = F.config(iters=iters)
    sides, refs = [], []
    for i, (base, with_init) in enumerate(((100, True), (200, False))):
        y, w, init = F.step_parity_inputs(hands["C"][i], base, with_init)
        sides.append(dict(pack=hands["packs"][i], y=y, w=w, init=init))
        refs.append(F.fit_rows(hands["C"][i], y, w, init=init, cfg=cfg))
    assert all(ok and abs(c2 - c) > 1e-9 * c for rr in refs for r in rr for c, c2, ok, _ in r["trace"])      # no tie decides
    got = c_fit(sides, 5, cfg)
    for i, h in enumerate("rl"):
        close(f"steps{iters}.{h}", got[i], refs[i])
    if iters == 3:
        assert sum(r["steps"] for rr in refs for r in rr) >= 20          # the steps are real ones


# ---- 2. the full run -----------------------------------------------------------------------------------------------------------
def test_full_run_parity(hands):
    """30 iterations, B = 16, through hands_amd.fit_mano.  The bar per output is 16 x the largest difference between the
    restatement and its noise = 1e-15 twin on these inputs, floored at BAR; ``steps`` is compared on the rows where the two
    agree, which must be at least 14 of the 16.  Measured on the CPU for these 16 cases: the twin differs by at most 6.0e-10 on
    rotation entries, 6.4e-11 on beta, 2.0e-13 on the translation, 3.5e-13 m on the rmse, and takes the same number of steps
    on all 16 rows -- so 16 x that stays below the floor, and BAR = 2.4e-7 is the bar of every output.  (The kernel on an
    MI355X: 3.0e-8, 1.2e-7, 3.0e-8 and 1.1e-11 -- the fp32 rounding of the outputs.)"""
    import hands_amd
    C = hands["C"][0]
    y, w, ref, twin = F.full_run_reference(C)
    out = hands_amd.fit_mano(torch.from_numpy(y).cuda(), hands["heads"][0], "r", weights=torch.from_numpy(w).cuda())
    agree = np.array([a["steps"] == b["steps"] for a, b in zip(ref, twin)])
    assert agree.sum() >= 14
    assert all(ok and abs(c2 - c) > 1e-9 * c for r in ref for c, c2, ok, _ in r["trace"])       # with the packed constants too
    for k, _ in FLOATS:
        r = np.stack([np.asarray(a["raw"][k], np.float64) for a in ref])
        t = np.stack([np.asarray(a["raw"][k], np.float64) for a in twin])
        bnd = np.maximum(16 * np.abs(r - t).max(), bar(r))
        err = np.abs(out[k].cpu().numpy().astype(np.float64) - r)
        print(f"FIT|full|{k}|twin {np.abs(r - t).max():.3e}|error {err.max():.3e}|{(err / bnd).max():.3f} of the bar")
        assert out[k].dtype == torch.float32 and (err <= bnd).all(), (k, float((err / bnd).max()))
    steps = out["steps"].cpu().numpy()
    assert steps.dtype == np.int32 and np.array_equal(steps[agree], np.array([a["steps"] for a in ref])[agree])
    assert float(out["rmse"].max()) <= 2e-3
    # pose_aa, the convention of process_data: adding pose_mean and taking Exp gives the fitted rotations back.  1e-5: the
    # fp32 quaternion route of hands_matrix_to_axis_angle_f32, some tens of roundings of 2^-24 at angles up to pi
    back = out["pose_aa"].cpu().numpy().astype(np.float64) + C.pose_mean
    again = np.stack([[F.exp_so3(row[3 * j:3 * j + 3]) for j in range(16)] for row in back])
    assert np.abs(again - out["pose"].cpu().numpy()).max() <= 1e-5


# ---- 3. consistency with the LBS kernel ------------------------------------------------------------------------------------------
def test_fit_agrees_with_the_lbs_kernel(hands):
    """The fitted pose (as pose_aa), beta and transl through hands_mano_heads_f32: the weighted rms of joints + t - y equals the reported rmse
    within 2e-6 m per hand (the LBS kernel's 6.9e-7 m against the oracle is the dominant term)."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import ManoHeadsPlan
    B = 6
    ys, ws = [], []
    for i in range(2):
        y, w = zip(*[F.family_case(hands["C"][i], 40 + 10 * i + b)[:2] for b in range(B)])
        ys.append(np.stack(y))
        ws.append(np.stack(w))
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": hands["packs"][0], "mano_l": hands["packs"][1]}})()
    fr, fl = hands_amd.fit_mano_hands(torch.from_numpy(ys[0]).cuda(), torch.from_numpy(ys[1]).cuda(), pair,
                                      weights_r=torch.from_numpy(ws[0]).cuda(), weights_l=torch.from_numpy(ws[1]).cuda())
    single = hands_amd.fit_mano(torch.from_numpy(ys[1]).cuda(), hands["heads"][1], "l", weights=torch.from_numpy(ws[1]).cuda())
    assert all(torch.equal(single[k], fl[k]) for k in single)          # one launch for both hands: the same bits
    # the full pose goes in as process_data hands it over: pose_aa (B,48), to which the kernel adds pose_mean
    rot = torch.cat([fr["pose_aa"], fl["pose_aa"]]).contiguous()
    shape = torch.cat([fr["beta"], fl["beta"]]).contiguous()
    cam = torch.ones(2 * B, 3, device="cuda")
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).cuda()
    out = ManoHeadsPlan(_lib.lib(), hands["packs"][0], hands["packs"][1], rot, shape, cam, K, 224.0, B, aa_input=True).launch(_stream())
    for i, (h, f) in enumerate((("r", fr), ("l", fl))):
        j = out[f"mano.joints3d.{h}"].cpu().numpy().astype(np.float64) + f["transl"].cpu().numpy().astype(np.float64)[:, None]
        w = ws[i].astype(np.float64)
        rms = np.sqrt((w[..., None] * (j - ys[i]) ** 2).sum((1, 2)) / w.sum(1))
        err = np.abs(rms - f["rmse"].cpu().numpy())
        print(f"FIT|lbs|{h}|{err.max():.3e}|2e-6")
        assert (err <= 2e-6).all(), (h, err)


# ---- 4. independence and reproducibility -------------------------------------------------------------------------------------------
def test_a_hand_does_not_depend_on_its_neighbours(hands):
    cfg = F.config(iters=8)
    C, pack = hands["C"][0], hands["packs"][0]
    y1, w1, _ = F.family_case(C, 31)
    alone = c_fit([dict(pack=pack, y=y1[None], w=w1[None])], 1, cfg)[0]
    assert alone["steps"][0] >= 4
    B, at = 67, (0, 33, 66)
    ys, ws = zip(*[F.family_case(C, 300 + b)[:2] for b in range(B)])
    y, w, valid = np.stack(ys), np.stack(ws), np.ones(B, np.float32)
    valid[[1, 32, 34, 65]] = 0.0                                       # unfitted rows next to it
    y[5] = np.nan
    for b in at:
        y[b], w[b] = y1, w1
    yl, wl = zip(*[F.family_case(hands["C"][1], 400 + b)[:2] for b in range(B)])
    one = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    two = c_fit([dict(pack=hands["packs"][1], y=np.stack(yl), w=np.stack(wl)), dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)
    again = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    for k in ("pose", "beta", "transl", "rmse"):
        for b in at:
            assert np.array_equal(bits(one[k][b]), bits(alone[k][0])), (k, b)
        assert np.array_equal(bits(one[k]), bits(two[1][k])) and np.array_equal(bits(one[k]), bits(again[k])), k
    assert np.array_equal(one["steps"], two[1]["steps"]) and np.array_equal(one["steps"], again["steps"])
    assert all(one["steps"][b] == alone["steps"][0] for b in at)
    assert np.isnan(one["rmse"][[1, 5, 32, 34, 65]]).all() and np.isfinite(np.delete(one["rmse"], [1, 5, 32, 34, 65])).all()


# ---- 5. the rules ----------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_fitted_and_unread_joints(hands):
    cfg = F.config(iters=3)
    C, pack = hands["C"][1], hands["packs"][1]
    B = 8
    ys, ws = zip(*[F.family_case(C, 500 + b)[:2] for b in range(B)])
    y, w, valid = np.stack(ys), np.ones((B, 21), np.float32), np.ones(B, np.float32)
    valid[1] = 0.0
    w[2] = 0.0
    w[2, [0, 7, 20]] = 1.0                                             # three weighted joints: not fitted
    y[3, 9, 2] = np.nan                                                # a NaN in a weighted joint
    y[7, 0, 0] = np.inf                                                # and an infinite one
    w[4, [2, 16]] = 0.0
    w[5, [2, 16]] = 0.0
    y[5] = y[4]
    y[4, [2, 16]] = np.nan                                             # NaN under weight 0: must not matter
    w[6] = 0.0
    w[6, [0, 4, 9, 18]] = 2.0                                          # four weighted joints: fitted
    got = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    close("rules", got, F.fit_rows(C, y, w, valid, cfg=cfg))
    unfitted = F.unfitted(C)
    for b in (1, 2, 3, 7):
        assert got["steps"][b] == 0 and np.isnan(got["rmse"][b])
        for k in ("pose", "beta", "transl"):
            assert np.array_equal(bits(got[k][b]), bits(unfitted[k])), (b, k)
    assert np.isfinite(got["rmse"][[0, 4, 5, 6]]).all() and got["steps"][4] >= 1
    for k in ("pose", "beta", "transl", "rmse"):
        assert np.array_equal(bits(got[k][4]), bits(got[k][5])), k
    assert got["steps"][4] == got["steps"][5]
    # weights = NULL and valid = NULL: every joint at weight 1, every row fitted
    plain = c_fit([dict(pack=pack, y=y[[0, 5]])], 2, cfg)[0]
    close("rules.null", plain, F.fit_rows(C, y[[0, 5]], cfg=cfg))
    ones = c_fit([dict(pack=pack, y=y[[0, 5]], w=np.ones((2, 21), np.float32), valid=np.ones(2, np.float32))], 2, cfg)[0]
    assert all(np.array_equal(bits(plain[k]), bits(ones[k])) for k in ("pose", "beta", "transl", "rmse"))
    # an initial state that is not finite: that row alone is not fitted
    _, _, init = F.step_parity_inputs(C, 500, True)
    init = tuple(a[:3].copy() for a in init)
    init[0][1, 7, 1, 1] = np.nan
    init[2][2, 0] = -np.inf
    got = c_fit([dict(pack=pack, y=y[:3], init=init)], 3, cfg)[0]
    close("rules.init", got, F.fit_rows(C, y[:3], init=init, cfg=cfg))
    assert np.isfinite(got["rmse"][0]) and np.isnan(got["rmse"][1:]).all()
    for b in (1, 2):
        assert all(np.array_equal(bits(got[k][b]), bits(unfitted[k])) for k in ("pose", "beta", "transl"))


# ---- 6. rejected calls -------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(hands):
    from hands_amd import _lib
    from hands_amd._lib import FitCfg, ManoFitConsts, ManoFitSide, ptr
    L, B = _lib.lib(), 2
    pack = hands["packs"][0]
    x = torch.zeros(B * 144, device="cuda")
    outs = {k: torch.full((B * 144,), SENT, device="cuda") for k in ("pose", "beta", "transl", "rmse")}
    steps = torch.full((B * 4,), -77777, dtype=torch.int32, device="cuda")

    def side(**drop):
        f = {k: ptr(pack[k]) for k in CONST_KEYS}
        f.update(joints=ptr(x), weights=None, valid=None, init_pose=None, init_beta=None, init_transl=None, steps=ptr(steps),
                 **{k: ptr(v) for k, v in outs.items()})
        f.update(drop)
        return ManoFitSide(ManoFitConsts(*[f[k] for k in CONST_KEYS]),
                           *[f[k] for k in ("joints", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta",
                                            "transl", "rmse", "steps")])

    def call(sides=None, n=1, cfg=(3, 1e-6, 1e-6, 1e-3), rows=B, null_sides=False, null_cfg=False):
        arr = (ManoFitSide * 2)(*(sides or [side(), side()]))
        c = FitCfg(*cfg)
        return L.hands_mano_fit_f32(None if null_sides else arr, n, None if null_cfg else ctypes.byref(c), rows, _stream())

    nan, inf = float("nan"), float("inf")
    cases = [("sides", dict(null_sides=True)), ("cfg", dict(null_cfg=True))]
    cases += [(k, dict(sides=[side(**{k: None}), side()])) for k in CONST_KEYS + ("joints", "pose", "beta", "transl", "rmse", "steps")]
    cases += [("second side", dict(sides=[side(), side(joints=None)], n=2))]
    cases += [("init " + "".join(k[5] for k in given), dict(sides=[side(**{k: ptr(x) for k in given}), side()]))
              for given in (("init_pose",), ("init_beta",), ("init_transl",), ("init_pose", "init_beta"),
                            ("init_pose", "init_transl"), ("init_beta", "init_transl"))]
    cases += [("B 0", dict(rows=0)), ("B -1", dict(rows=-1)), ("n_sides 0", dict(n=0)), ("n_sides 3", dict(n=3)),
              ("n_sides -1", dict(n=-1)), ("iters", dict(cfg=(-1, 1e-6, 1e-6, 1e-3)))]
    cases += [(f"cfg[{i}] {v}", dict(cfg=tuple(v if j == i else c for j, c in enumerate((3, 1e-6, 1e-6, 1e-3)))))
              for i in (1, 2, 3) for v in (-1e-9, nan, inf, -inf)]
    for name, kw in cases:
        assert call(**kw) == EINVAL, name
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in outs.values()) and bool((steps == -77777).all())
    assert call(sides=[side(**{k: ptr(x) for k in ("init_pose", "init_beta", "init_transl")}), side()]) == 0      # the table's complement
    assert call(n=2, cfg=(0, 0.0, 0.0, 0.0)) == 0
    torch.cuda.synchronize()


# ---- 7. the wrapper ----------------------------------------------------------------------------------------------------------------
def test_wrapper_fit_gt(golden_dir, recipe_model):
    import hands_amd
    from hands_amd.wrapper import HandsWrapper
    model = copy.deepcopy(recipe_model).to("cuda")
    w = HandsWrapper(model=model)
    assert w.fit_gt is None
    B = 3
    P = model.packed(torch.device("cuda"))
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).cuda()
    full = {}
    for h in "rl":
        C = F.Consts(*[P[f"mano_{h}"][k].cpu().numpy() for k in CONST_KEYS])
        full[h] = np.stack([F.family_case(C, 600 + 10 * (h == "l") + b)[0] for b in range(B)])
    targets = hands_amd.xdict({f"mano.j3d.full.{h}": torch.from_numpy(full[h]).cuda() for h in "rl"})
    with pytest.raises(KeyError):                                      # keypoints alone are not enough without the fit
        w.process_data(hands_amd.xdict(dict(targets)), {"intrinsics": K})
    w.fit_gt = hands_amd.FitConfig()
    t = w.process_data(targets, {"intrinsics": K})
    for h in "rl":
        assert t[f"mano.pose.{h}"].shape == (B, 48) and t[f"mano.beta.{h}"].shape == (B, 10)
        v, j = t[f"mano.vertices.{h}"], t[f"mano.joints3d.{h}"].double()
        assert v.shape == (B, 778, 3) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(t[f"mano.v3d.cam.{h}"]).all())
        rmse = t[f"mano.fit.rmse.{h}"].double()
        d = j + t[f"mano.fit.transl.{h}"].double()[:, None] - torch.from_numpy(full[h]).cuda().double()
        rms = d.pow(2).sum(2).mean(1).sqrt()
        print(f"FIT|wrapper|{h}|rmse {rmse.max().item():.3e}|rms {rms.max().item():.3e}")
        assert bool((rmse <= 2e-3).all()) and bool((rms <= rmse + 2e-6).all()), (h, rms, rmse)
    t.overwrite("is_valid", torch.ones(B).cuda())
    t.overwrite("right_valid", torch.ones(B).cuda())
    t.overwrite("left_valid", torch.ones(B).cuda())
    m = hands_amd.evaluate_mesh_metrics(t, t, {"intrinsics": K})
    assert len(m) and all(bool(torch.isfinite(x).all()) for x in m.values())
    # fit_gt = None: process_data is what it was -- the golden outputs, with the tolerances of
    # tests/test_wrapper.py::test_wrapper_test_mode_on_device, no mano.fit.* key, and the input dict handed back
    d = np.load(os.path.join(golden_dir, "process_data.npz"))
    tin = {k[3:]: torch.from_numpy(d[k]).cuda() for k in d.files if k.startswith("in/")}
    Kg = tin.pop("intrinsics")
    w.fit_gt = None
    given = hands_amd.xdict(dict(tin))
    b = w.process_data(given, {"intrinsics": Kg})
    assert b is given and not any("mano.fit." in k for k in b)
    for k in tin:
        if "j3d.full" not in k:
            assert torch.equal(b[k], tin[k]), k                          # mano.pose / mano.beta are the caller's
    for k in (k for k in d.files if k.startswith("out/")):
        tol = 2e-6 if "cam_t.wp" not in k else 2e-5
        np.testing.assert_allclose(b[k[4:]].cpu().numpy(), d[k], rtol=tol, atol=2e-6, err_msg=k)
    # with the fit on, the caller's dict is left alone and host tensors are moved as process_data moves everything else
    w.fit_gt = hands_amd.FitConfig(iters=2)
    host = hands_amd.xdict({f"mano.j3d.full.{h}": torch.from_numpy(full[h]) for h in "rl"})
    t2 = w.process_data(host, {"intrinsics": K})
    assert list(host) == ["mano.j3d.full.r", "mano.j3d.full.l"] and "mano.fit.rmse.r" in t2
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano(torch.from_numpy(full["r"]).cuda(), model, "r", weights=torch.ones(B, 21))
