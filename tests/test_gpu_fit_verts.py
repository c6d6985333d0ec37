"""hands_mano_fit_verts_f32 and what stands on it (hands_amd/fitting.py, ``fit_gt_verts`` in HandsWrapper) on the device against the
fp64 restatement (tests/fit_verts_ref.py) of DESIGN.md section 7 "MANO fitting to 778 vertices".

Bars.  The kernel computes in fp64 what the restatement computes and rounds once to fp32; the two differ by device-versus-host
libm and by the order of fp64 sums, so the fp32 rounding of the output dominates: BAR = 4 * 2^-24 * max(1, |ref|) per float
output, the bar of tests/test_gpu_fitting.py; ``steps`` is equal wherever the restatement's decisions have a margin above 1e-9
of the cost, which every test that compares it asserts itself.  Past convergence a decision is a tie at rounding level: the
full run bounds ``steps`` of a fully weighted row by the restatement's clear and tied decisions instead.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import fit_verts_ref as V
from edge_util import EINVAL, SENT, In, Out, OutInt

pytestmark = pytest.mark.gpu

CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights", "posedirs_vm")
FLOATS = ("pose", "beta", "transl", "rmse", "j3d")
NV = 778


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
    return {"heads": heads, "packs": packs, "C": [V.consts_from_pack(p) for p in packs]}


def c_fit(sides, B, cfg=None, n_sides=None):
    """hands_mano_fit_verts_f32 on guarded buffers.  sides: per side dict(pack, y, w=None, valid=None, init=None) of numpy arrays
    -> per side dict of numpy outputs (the bands around every output checked)."""
    from hands_amd import _lib
    from hands_amd._lib import FitCfg, ManoFitVertsConsts, ManoFitVertsSide, ptr
    cfg = cfg or V.config()
    f32 = lambda a: None if a is None else In(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    p = lambda b: None if b is None else b.ptr()
    arr, keep, outs = (ManoFitVertsSide * len(sides))(), [], []
    names = ("pose", "beta", "transl", "rmse", "steps", "j3d")
    for i, s in enumerate(sides):
        ins = [f32(s["y"]), f32(s.get("w")), f32(s.get("valid"))] + [f32(a) for a in (s.get("init") or (None, None, None))]
        o = {"pose": Out(B, 16, 3, 3), "beta": Out(B, 10), "transl": Out(B, 3), "rmse": Out(B), "steps": OutInt(torch.int32, B),
             "j3d": Out(B, 21, 3)}
        arr[i] = ManoFitVertsSide(ManoFitVertsConsts(*[ptr(s["pack"][k]) for k in CONST_KEYS]), *[p(b) for b in ins],
                                  *[o[k].ptr() for k in names])
        keep.append(ins)
        outs.append(o)
    c = FitCfg(cfg["iters"], cfg["lambda_beta"], cfg["lambda_pose"], cfg["mu0"])
    rc = _lib.lib().hands_mano_fit_verts_f32(arr, n_sides or len(sides), ctypes.byref(c), B, _stream())
    assert rc == 0, rc
    return [{k: v.get().numpy() for k, v in o.items()} for o in outs]


def close(what, got, ref_rows, steps=True):
    """got: a side's outputs; ref_rows: the restatement's results per row.  Prints the narrowest margin per output."""
    for k in FLOATS:
        ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in ref_rows])
        g = got[k].astype(np.float64)
        assert got[k].dtype == np.float32 and g.shape == ref.shape, (what, k, g.shape, ref.shape)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), (what, k, "NaN positions differ")
        ratio = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, g) - np.where(nan, 0.0, ref)) / bar(np.where(nan, 0.0, ref)))
        print(f"FITV|{what}|{k}|{ratio.max():.3f} of the bar")
        assert (ratio <= 1.0).all(), (what, k, float(ratio.max()))
    if steps:
        assert np.array_equal(got["steps"], np.array([r["steps"] for r in ref_rows], np.int32)), (what, got["steps"])


# ---- 1. step parity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 2, 3, 4])
def test_step_parity(hands, iters):
    """B = 6, both assets in one launch: all ones, uneven weights, 500 zero weights, zero weight on two whole tiles and the tail,
    20 weighted vertices, 4 weighted vertices; NaN coordinates under every zero weight; the right hand from a caller's initial
    state, the left from the Kabsch state."""
    cfg = V.config(iters=iters)
    sides, refs = [], []
    for i, (h, with_init) in enumerate((("r", True), ("l", False))):
        y, w, init = V.step_parity_inputs(hands["C"][i], V.STEP_BASES[h], with_init)
        sides.append(dict(pack=hands["packs"][i], y=y, w=w, init=init))
        refs.append(V.fit_rows(hands["C"][i], y, w, init=init, cfg=cfg))
    assert all(V.clear(r["trace"]) for rr in refs for r in rr)          # no tie decides
    got = c_fit(sides, 6, cfg)
    for i, h in enumerate("rl"):
        close(f"steps{iters}.{h}", got[i], refs[i])
    if iters == 4:
        assert sum(r["steps"] for rr in refs for r in rr) >= 30          # the steps are real ones


# ---- 2. the full run -----------------------------------------------------------------------------------------------------------
def test_full_run_parity(hands):
    """30 iterations, B = 6 (four fully weighted rows, two with 20 weighted vertices), through hands_amd.fit_mano_verts.  The bar
    per output is 16 x the difference between the restatement and its noise = 1e-15 twin on that row, floored at BAR;
    tests/test_fit_verts.py caps that twin term at 1e-6.  ``steps`` is equal on the sparse rows, whose 30 decisions all have a
    margin; on a fully weighted row it lies between the restatement's clear accepted decisions and those plus its ties."""
    import hands_amd
    C = hands["C"][0]
    y, w, ref, twin = V.full_run_reference(C)
    nd = len(V.FULL_DENSE)
    assert len(ref) == 6 and nd == 4
    out = hands_amd.fit_mano_verts(torch.from_numpy(y).cuda(), hands["heads"][0], "r", weights=torch.from_numpy(w).cuda())
    assert list(out) == ["pose", "beta", "transl", "rmse", "steps", "j3d", "pose_aa"]
    assert all(V.clear(r["trace"]) for r in ref[nd:])                   # with the packed constants too
    for k in FLOATS:
        r = np.stack([np.asarray(a["raw"][k], np.float64) for a in ref])
        t = np.stack([np.asarray(a["raw"][k], np.float64) for a in twin])
        dt = np.abs(r - t).reshape(6, -1).max(1).reshape((6,) + (1,) * (r.ndim - 1))
        assert 16 * dt.max() <= 1e-6, (k, float(dt.max()))
        bnd = np.maximum(16 * dt, bar(r))
        err = np.abs(out[k].cpu().numpy().astype(np.float64) - r)
        print(f"FITV|full|{k}|twin {dt.max():.3e}|error {err.max():.3e}|{(err / bnd).max():.3f} of the bar")
        assert out[k].dtype == torch.float32 and (err <= bnd).all(), (k, float((err / bnd).max()))
    steps = out["steps"].cpu().numpy()
    assert steps.dtype == np.int32 and np.array_equal(steps[nd:], np.array([a["steps"] for a in ref[nd:]]))
    for b in range(nd):
        n_clear = sum(1 for c, c2, ok, acc in ref[b]["trace"] if acc and ok and abs(c2 - c) > 1e-9 * c)
        n_tied = sum(1 for c, c2, ok, acc in ref[b]["trace"] if not (ok and abs(c2 - c) > 1e-9 * c))
        print(f"FITV|full|steps row {b}|{steps[b]}|clear {n_clear}|tied {n_tied}")
        assert n_clear <= steps[b] <= n_clear + n_tied, (b, steps[b], n_clear, n_tied)
    assert float(out["rmse"][:nd].max()) <= 4e-6
    back = out["pose_aa"].cpu().numpy().astype(np.float64) + C.pose_mean
    again = np.stack([[V.exp_so3(row[3 * j:3 * j + 3]) for j in range(16)] for row in back])
    assert np.abs(again - out["pose"].cpu().numpy()).max() <= 1e-5


# ---- 3. consistency with the LBS kernel ------------------------------------------------------------------------------------------
def test_fit_agrees_with_the_lbs_kernel(hands):
    """The fitted pose (as pose_aa) and beta through hands_mano_heads_f32: the weighted rms of vertices + transl - y equals the
    reported rmse within 2e-6 m per hand (the LBS kernel's 6.9e-7 m against the oracle is the dominant term).  A one-side
    launch gives the bits of the two-side launch."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import ManoHeadsPlan
    B = 4
    ys, ws = [], []
    for i in range(2):
        y, w = zip(*[V.family_case(hands["C"][i], 40 + 10 * i + b, keep=(None, None, 200, 20)[b])[:2] for b in range(B)])
        ys.append(np.stack(y))
        ws.append(np.stack(w))
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": hands["packs"][0], "mano_l": hands["packs"][1]}})()
    fr, fl = hands_amd.fit_mano_hands_verts(torch.from_numpy(ys[0]).cuda(), torch.from_numpy(ys[1]).cuda(), pair,
                                            weights_r=torch.from_numpy(ws[0]).cuda(), weights_l=torch.from_numpy(ws[1]).cuda())
    single = hands_amd.fit_mano_verts(torch.from_numpy(ys[1]).cuda(), hands["heads"][1], "l", weights=torch.from_numpy(ws[1]).cuda())
    assert all(torch.equal(single[k], fl[k]) for k in single)          # one launch for both hands: the same bits
    rot = torch.cat([fr["pose_aa"], fl["pose_aa"]]).contiguous()
    shape = torch.cat([fr["beta"], fl["beta"]]).contiguous()
    cam = torch.ones(2 * B, 3, device="cuda")
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).cuda()
    out = ManoHeadsPlan(_lib.lib(), hands["packs"][0], hands["packs"][1], rot, shape, cam, K, 224.0, B, aa_input=True).launch(_stream())
    for i, (h, f) in enumerate((("r", fr), ("l", fl))):
        v = out[f"mano.vertices.{h}"].cpu().numpy().astype(np.float64) + f["transl"].cpu().numpy().astype(np.float64)[:, None]
        w = ws[i].astype(np.float64)
        rms = np.sqrt((w[..., None] * (v - ys[i]) ** 2).sum((1, 2)) / w.sum(1))
        err = np.abs(rms - f["rmse"].cpu().numpy())
        print(f"FITV|lbs|{h}|{err.max():.3e}|2e-6")
        assert (err <= 2e-6).all(), (h, err)
        j = out[f"mano.joints3d.{h}"].cpu().numpy().astype(np.float64) + f["transl"].cpu().numpy().astype(np.float64)[:, None]
        assert np.abs(j - f["j3d"].cpu().numpy()).max() <= 2e-6


# ---- 4. independence and reproducibility -------------------------------------------------------------------------------------------
def test_a_hand_does_not_depend_on_its_neighbours(hands):
    cfg = V.config(iters=6)
    C, pack = hands["C"][0], hands["packs"][0]
    y1, w1, _ = V.family_case(C, 31)
    w1 = w1.copy()
    w1[::7] = 0.0
    alone = c_fit([dict(pack=pack, y=y1[None], w=w1[None])], 1, cfg)[0]
    assert alone["steps"][0] >= 4
    B, at = 67, (0, 33, 66)
    rng = np.random.RandomState(5)
    y = (y1[None] + 0.01 * rng.randn(B, NV, 3)).astype(np.float32)      # other meshes: the same hand, noisy
    w, valid = rng.uniform(0.5, 2.0, (B, NV)).astype(np.float32), np.ones(B, np.float32)
    valid[[1, 32, 34, 65]] = 0.0                                       # unfitted rows next to it
    y[5] = np.nan
    for b in at:
        y[b], w[b] = y1, w1
    yl = (V.family_case(hands["C"][1], 400)[0][None] + 0.01 * rng.randn(B, NV, 3)).astype(np.float32)
    one = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    two = c_fit([dict(pack=hands["packs"][1], y=yl), dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)
    again = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    for k in FLOATS:
        for b in at:
            assert np.array_equal(bits(one[k][b]), bits(alone[k][0])), (k, b)
        assert np.array_equal(bits(one[k]), bits(two[1][k])) and np.array_equal(bits(one[k]), bits(again[k])), k
    assert np.array_equal(one["steps"], two[1]["steps"]) and np.array_equal(one["steps"], again["steps"])
    assert all(one["steps"][b] == alone["steps"][0] for b in at)
    assert np.isnan(one["rmse"][[1, 5, 32, 34, 65]]).all() and np.isfinite(np.delete(one["rmse"], [1, 5, 32, 34, 65])).all()


# ---- 5. the rules ----------------------------------------------------------------------------------------------------------------
def test_rows_that_are_not_fitted_and_unread_vertices(hands):
    cfg = V.config(iters=3)
    C, pack = hands["C"][1], hands["packs"][1]
    B = 8
    ys = [V.family_case(C, 500 + b)[0] for b in range(B)]
    y, w, valid = np.stack(ys), np.ones((B, NV), np.float32), np.ones(B, np.float32)
    valid[1] = 0.0
    w[2] = 0.0
    w[2, [0, 300, 777]] = 1.0                                          # three weighted vertices: not fitted
    y[3, 9, 2] = np.nan                                                # a NaN in a weighted vertex
    y[7, 777, 0] = np.inf                                              # and an infinite one
    hidden = [2, 16, 47, 48, 500, 777]
    w[4, hidden] = 0.0
    w[5, hidden] = 0.0
    y[5] = y[4]
    y[4, hidden] = np.nan                                              # NaN under weight 0: must not matter
    w[6] = 0.0
    w[6, [0, 250, 500, 777]] = 2.0                                     # four weighted vertices: fitted
    got = c_fit([dict(pack=pack, y=y, w=w, valid=valid)], B, cfg)[0]
    ref = V.fit_rows(C, y, w, valid, cfg=cfg)
    assert all(V.clear(r["trace"]) for r in ref)
    close("rules", got, ref)
    unfitted = V.unfitted(C)
    for b in (1, 2, 3, 7):
        assert got["steps"][b] == 0 and np.isnan(got["rmse"][b]) and np.isnan(got["j3d"][b]).all()
        for k in ("pose", "beta", "transl"):
            assert np.array_equal(bits(got[k][b]), bits(unfitted[k])), (b, k)
    assert np.isfinite(got["rmse"][[0, 4, 5, 6]]).all() and got["steps"][4] >= 1 and got["steps"][6] >= 1
    for k in FLOATS:
        assert np.array_equal(bits(got[k][4]), bits(got[k][5])), k
    assert got["steps"][4] == got["steps"][5]
    # weights = NULL and valid = NULL: every vertex at weight 1, every row fitted
    plain = c_fit([dict(pack=pack, y=y[[0, 5]])], 2, cfg)[0]
    close("rules.null", plain, V.fit_rows(C, y[[0, 5]], cfg=cfg))
    ones = c_fit([dict(pack=pack, y=y[[0, 5]], w=np.ones((2, NV), np.float32), valid=np.ones(2, np.float32))], 2, cfg)[0]
    assert all(np.array_equal(bits(plain[k]), bits(ones[k])) for k in FLOATS) and np.array_equal(plain["steps"], ones["steps"])
    # an initial state that is not finite: that row alone is not fitted
    rng = np.random.RandomState(9)
    init = [V.near(V.family_case(C, 500 + b)[2], rng) for b in range(3)]
    init = tuple(np.stack([a[i] for a in init]).astype(np.float32) for i in range(3))
    init[0][1, 7, 1, 1] = np.nan
    init[2][2, 0] = -np.inf
    got = c_fit([dict(pack=pack, y=y[:3], init=init)], 3, cfg)[0]
    close("rules.init", got, V.fit_rows(C, y[:3], init=init, cfg=cfg))
    assert np.isfinite(got["rmse"][0]) and np.isnan(got["rmse"][1:]).all() and np.isnan(got["j3d"][1:]).all()
    for b in (1, 2):
        assert all(np.array_equal(bits(got[k][b]), bits(unfitted[k])) for k in ("pose", "beta", "transl"))


# ---- 6. rejected calls -------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(hands):
    from hands_amd import _lib
    from hands_amd._lib import FitCfg, ManoFitVertsConsts, ManoFitVertsSide, ptr
    L, B = _lib.lib(), 2
    pack = hands["packs"][0]
    x = torch.zeros(B * NV * 3, device="cuda")
    outs = {k: torch.full((B * 144,), SENT, device="cuda") for k in ("pose", "beta", "transl", "rmse", "j3d")}
    steps = torch.full((B * 4,), -77777, dtype=torch.int32, device="cuda")
    fields = ("verts", "weights", "valid", "init_pose", "init_beta", "init_transl", "pose", "beta", "transl", "rmse", "steps", "j3d")

    def side(**drop):
        f = {k: ptr(pack[k]) for k in CONST_KEYS}
        f.update(verts=ptr(x), weights=None, valid=None, init_pose=None, init_beta=None, init_transl=None, steps=ptr(steps),
                 **{k: ptr(v) for k, v in outs.items()})
        f.update(drop)
        return ManoFitVertsSide(ManoFitVertsConsts(*[f[k] for k in CONST_KEYS]), *[f[k] for k in fields])

    def call(sides=None, n=1, cfg=(3, 1e-6, 1e-6, 1e-3), rows=B, null_sides=False, null_cfg=False):
        arr = (ManoFitVertsSide * 2)(*(sides or [side(), side()]))
        c = FitCfg(*cfg)
        return L.hands_mano_fit_verts_f32(None if null_sides else arr, n, None if null_cfg else ctypes.byref(c), rows, _stream())

    nan, inf = float("nan"), float("inf")
    cases = [("sides", dict(null_sides=True)), ("cfg", dict(null_cfg=True))]
    cases += [(k, dict(sides=[side(**{k: None}), side()])) for k in CONST_KEYS + ("verts", "pose", "beta", "transl", "rmse", "steps", "j3d")]
    cases += [("second side", dict(sides=[side(), side(verts=None)], n=2)), ("second side j3d", dict(sides=[side(), side(j3d=None)], n=2))]
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
def test_wrapper_fit_gt_verts(golden_dir, recipe_model):
    import hands_amd
    from hands_amd.wrapper import HandsWrapper
    model = copy.deepcopy(recipe_model).to("cuda")
    w = HandsWrapper(model=model)
    assert w.fit_gt_verts is None
    B = 3
    P = model.packed(torch.device("cuda"))
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).cuda()
    full = {}
    for h in "rl":
        C = V.consts_from_pack(P[f"mano_{h}"])
        full[h] = np.stack([V.family_case(C, 600 + 10 * (h == "l") + b)[0] for b in range(B)])
    targets = hands_amd.xdict({f"mano.v3d.full.{h}": torch.from_numpy(full[h]).cuda() for h in "rl"})
    with pytest.raises(KeyError):                                      # vertices alone are not enough without the fit
        w.process_data(hands_amd.xdict(dict(targets)), {"intrinsics": K})
    w.fit_gt_verts = hands_amd.FitConfig()
    t = w.process_data(targets, {"intrinsics": K})
    assert list(targets) == ["mano.v3d.full.r", "mano.v3d.full.l"]
    for h in "rl":
        assert t[f"mano.pose.{h}"].shape == (B, 48) and t[f"mano.beta.{h}"].shape == (B, 10) and t[f"mano.j3d.full.{h}"].shape == (B, 21, 3)
        v = t[f"mano.vertices.{h}"]
        assert v.shape == (B, 778, 3) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(t[f"mano.v3d.cam.{h}"]).all())
        rmse = t[f"mano.fit.rmse.{h}"].double()
        d = v.double() + t[f"mano.fit.transl.{h}"].double()[:, None] - torch.from_numpy(full[h]).cuda().double()
        rms = d.pow(2).sum(2).mean(1).sqrt()
        print(f"FITV|wrapper|{h}|rmse {rmse.max().item():.3e}|rms {rms.max().item():.3e}")
        assert bool((rmse <= 4e-6).all()) and bool((rms <= rmse + 2e-6).all()), (h, rms, rmse)
    t.overwrite("is_valid", torch.ones(B).cuda())
    t.overwrite("right_valid", torch.ones(B).cuda())
    t.overwrite("left_valid", torch.ones(B).cuda())
    m = hands_amd.evaluate_mesh_metrics(t, t, {"intrinsics": K})
    assert len(m) and all(bool(torch.isfinite(x).all()) for x in m.values())
    # a present mano.j3d.full is left alone; right_valid / left_valid are honoured
    given_j = torch.zeros(B, 21, 3, device="cuda")
    both = hands_amd.xdict(dict(targets))
    both["mano.j3d.full.r"] = given_j
    valid = torch.tensor([1.0, 0.0, 1.0]).cuda()
    f = hands_amd.fit_targets_verts(both, model, {"right_valid": valid}, hands_amd.FitConfig(iters=2))
    assert f["mano.j3d.full.r"] is given_j and "mano.j3d.full.l" in f and "mano.j3d.full.l" not in both
    assert torch.isnan(f["mano.fit.rmse.r"]).tolist() == [False, True, False] and bool(torch.isfinite(f["mano.fit.rmse.l"]).all())
    # fit_gt_verts = None: process_data is what it was -- the golden outputs, with the tolerances of
    # tests/test_gpu_fitting.py::test_wrapper_fit_gt, no mano.fit.* key, and the input dict handed back
    d = np.load(os.path.join(golden_dir, "process_data.npz"))
    tin = {k[3:]: torch.from_numpy(d[k]).cuda() for k in d.files if k.startswith("in/")}
    Kg = tin.pop("intrinsics")
    w.fit_gt_verts = None
    given = hands_amd.xdict(dict(tin))
    b = w.process_data(given, {"intrinsics": Kg})
    assert b is given and not any("mano.fit." in k for k in b)
    for k in tin:
        if "j3d.full" not in k:
            assert torch.equal(b[k], tin[k]), k
    for k in (k for k in d.files if k.startswith("out/")):
        tol = 2e-6 if "cam_t.wp" not in k else 2e-5
        np.testing.assert_allclose(b[k[4:]].cpu().numpy(), d[k], rtol=tol, atol=2e-6, err_msg=k)
    # host tensors are moved as process_data moves everything else; two hooks set raise
    w.fit_gt_verts = hands_amd.FitConfig(iters=2)
    host = hands_amd.xdict({f"mano.v3d.full.{h}": torch.from_numpy(full[h]) for h in "rl"})
    t2 = w.process_data(host, {"intrinsics": K})
    assert list(host) == ["mano.v3d.full.r", "mano.v3d.full.l"] and "mano.fit.rmse.r" in t2
    for other in ("fit_gt", "fit_gt_2d"):
        setattr(w, other, hands_amd.FitConfig() if other == "fit_gt" else hands_amd.Fit2DConfig())
        with pytest.raises(ValueError):
            w.process_data(host, {"intrinsics": K})
        setattr(w, other, None)
    w.fit_gt_verts = None
    w.fit_gt, w.fit_gt_2d = hands_amd.FitConfig(), hands_amd.Fit2DConfig()
    with pytest.raises(ValueError, match="fit_gt and fit_gt_2d are both set"):
        w.process_data(host, {"intrinsics": K})
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano_verts(torch.from_numpy(full["r"]).cuda(), model, "r", weights=torch.ones(B, NV))
