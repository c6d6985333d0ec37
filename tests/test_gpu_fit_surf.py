"""hands_mano_fit_surf_f32 (csrc/fit_surf.hip) and hands_amd.fit_mano_surface on the device against the fp64 restatement
(tests/fit_surf_ref.py) of DESIGN.md section 7 "MANO fitting to surface correspondences and ICP registration".

Bars, as tests/test_gpu_fit_verts.py: the kernel computes in fp64 what the restatement computes and rounds once to fp32, so
BAR = 4 * 2^-24 * max(1, |ref|) per float output; ``steps`` -- and the outputs, which follow the decisions -- are compared for
the hands whose every accept / reject decision has a margin above 1e-9 of the cost, which is every hand here (asserted).
"""
import ctypes

import numpy as np
import pytest
import torch

import fit_surf_ref as S
import fit_verts_ref as V
from edge_util import EINVAL, SENT, In, Out, OutInt

pytestmark = pytest.mark.gpu

CONST_KEYS = ("pose_mean", "J_template", "J_shapedirs", "v_template", "shapedirs", "lbs_weights", "posedirs_vm", "faces_i32")
FLOATS = ("pose", "beta", "transl", "rmse", "j3d", "verts")
NAMES = ("pose", "beta", "transl", "rmse", "steps", "j3d", "verts")
NV = 778


def bar(ref):
    return 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def hands():
    """Per side: the MANO head, its packed constants on the device, the restatement's constants read back from them, the faces."""
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead, pack_mano_pair
    heads = [MANOHead(r, 1000.0, 224, asset=synthetic_mano_asset(r)) for r in (True, False)]
    packs = pack_mano_pair(heads[0], heads[1], torch.device("cuda"))
    return {"heads": heads, "packs": packs, "C": [V.consts_from_pack(p) for p in packs],
            "faces": [p["faces"].numpy() for p in packs]}


def c_fit(sides, B, cfg=None, n_sides=None):
    """hands_mano_fit_surf_f32 on guarded buffers.  sides: per side dict(pack, y, f, b, w=None, n=None, valid=None, init=None) of
    numpy arrays -> per side dict of numpy outputs (the bands around every output checked)."""
    from hands_amd import _lib
    from hands_amd._lib import FitSurfCfg, ManoFitSurfConsts, ManoFitSurfSide, ptr
    cfg = cfg or S.config()
    f32 = lambda a: None if a is None else In(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
    p = lambda b: None if b is None else b.ptr()
    arr, keep, outs = (ManoFitSurfSide * len(sides))(), [], []
    P = sides[0]["y"].shape[1]
    for i, s in enumerate(sides):
        ins = [f32(s["y"]), f32(s.get("w")), f32(s.get("valid"))] + [f32(a) for a in (s.get("init") or (None, None, None))]
        face = torch.from_numpy(np.ascontiguousarray(s["f"], np.int32)).cuda()
        more = [f32(s["b"]), f32(s.get("n"))]
        o = {"pose": Out(B, 16, 3, 3), "beta": Out(B, 10), "transl": Out(B, 3), "rmse": Out(B), "steps": OutInt(torch.int32, B),
             "j3d": Out(B, 21, 3), "verts": Out(B, NV, 3)}
        arr[i] = ManoFitSurfSide(ManoFitSurfConsts(*[ptr(s["pack"][k]) for k in CONST_KEYS]), *[p(b) for b in ins],
                                 *[o[k].ptr() for k in NAMES], ptr(face), *[p(b) for b in more])
        keep.append((ins, face, more))
        outs.append(o)
    c = FitSurfCfg(cfg["iters"], cfg["lambda_beta"], cfg["lambda_pose"], cfg["mu0"], cfg["tangent_weight"])
    rc = _lib.lib().hands_mano_fit_surf_f32(arr, n_sides or len(sides), ctypes.byref(c), B, P, _stream())
    assert rc == 0, rc
    return [{k: v.get().numpy() for k, v in o.items()} for o in outs]


def close(what, got, ref_rows):
    for k in FLOATS:
        ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in ref_rows])
        g = got[k].astype(np.float64)
        assert got[k].dtype == np.float32 and g.shape == ref.shape, (what, k, g.shape, ref.shape)
        nan = np.isnan(ref)
        assert np.array_equal(np.isnan(g), nan), (what, k, "NaN positions differ")
        ratio = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, g) - np.where(nan, 0.0, ref)) / bar(np.where(nan, 0.0, ref)))
        print(f"FITS|{what}|{k}|{ratio.max():.3f} of the bar")
        assert (ratio <= 1.0).all(), (what, k, float(ratio.max()))
    assert np.array_equal(got["steps"], np.array([r["steps"] for r in ref_rows], np.int32)), (what, got["steps"])


def batch(C, faces, base, B, P, with_init, with_normals, hide=True):
    """B hands of P rows on the model's own posed surface; with ``hide`` and P >= 16 rows 2 and P - 1 have weight 0, NaN values
    and face -1; the weights are uneven; the normals random unit vectors, row 0's zero and row 1's twice as long."""
    rng = np.random.RandomState(7000 + base)
    ys, fs, bs, ws, ns, init = [], [], [], [], [], ([], [], [])
    for k in range(B):
        y, f, b, truth = S.surface_case(C, faces, base + k, P)
        w = rng.uniform(0.5, 2.0, P).astype(np.float32)
        n = rng.randn(P, 3)
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        n[0], n[1] = 0.0, 2.0 * n[1]
        if hide and P >= 16:
            for r in (2, P - 1):
                w[r], y[r], b[r], n[r], f[r] = 0.0, np.nan, np.nan, np.nan, -1
        for a, v in zip(init, V.near(truth, rng)):
            a.append(v)
        ys.append(y); fs.append(f); bs.append(b); ws.append(w); ns.append(n)
    init = tuple(np.stack(a).astype(np.float32) for a in init) if with_init else None
    return dict(y=np.stack(ys), f=np.stack(fs), b=np.stack(bs), w=np.stack(ws), n=np.stack(ns) if with_normals else None, init=init)


def ref_of(C, faces, d, cfg, valid=None):
    return S.fit_rows(C, faces, d["y"], d["f"], d["b"], d.get("w"), d.get("n"), valid, d.get("init"), cfg)


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["none", 1.0, 0.1, 0.0])
@pytest.mark.parametrize("P", [4, 16, 17, 50])
def test_step_parity(hands, P, mode):
    """B = 3, both assets in one launch, four iterations: the right hand from a caller's initial state, the left from the Kabsch
    state; without normals (tangent_weight 0.1 then changes nothing) and with them at tangent_weight 1, 0.1 and 0."""
    tau = 0.1 if mode == "none" else mode
    cfg = S.config(iters=4, tangent_weight=tau)
    sides, refs = [], []
    for i, with_init in enumerate((True, False)):
        d = batch(hands["C"][i], hands["faces"][i], 100 * i + P, 3, P, with_init, mode != "none")
        sides.append(dict(pack=hands["packs"][i], **d))
        refs.append(ref_of(hands["C"][i], hands["faces"][i], d, cfg))
    got = c_fit(sides, 3, cfg)
    for i, h in enumerate("rl"):
        assert all(S.clear(r["trace"]) for r in refs[i]), (h, [r["trace"] for r in refs[i]])        # no tie decides
        close(f"P{P}.{mode}.{h}", got[i], refs[i])
    assert sum(r["steps"] for rr in refs for r in rr) >= 6             # the steps are real ones


def test_zero_iterations_return_the_start(hands):
    C, faces, pack = hands["C"][0], hands["faces"][0], hands["packs"][0]
    cfg = S.config(iters=0)
    d = batch(C, faces, 40, 3, 17, True, False)
    got = c_fit([dict(pack=pack, **d)], 3, cfg)[0]
    close("iters0.init", got, ref_of(C, faces, d, cfg))
    for k, a in zip(("pose", "beta", "transl"), d["init"]):
        assert np.array_equal(bits(got[k]), bits(a.reshape(got[k].shape))), k
    assert (got["steps"] == 0).all()
    d = batch(C, faces, 40, 3, 17, False, False)
    close("iters0.kabsch", c_fit([dict(pack=pack, **d)], 3, cfg)[0], ref_of(C, faces, d, cfg))


# ---- 2. the same bits ------------------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_launch_row_batch_side_or_trailing_rows(hands):
    cfg = S.config(iters=6, tangent_weight=0.1)
    C, faces, pack = hands["C"][0], hands["faces"][0], hands["packs"][0]
    one = batch(C, faces, 60, 1, 17, False, True)
    alone = c_fit([dict(pack=pack, **one)], 1, cfg)[0]
    assert alone["steps"][0] >= 2
    B, at = 5, (0, 3, 4)
    d = batch(C, faces, 61, B, 17, False, True)
    for b in at:
        for k in ("y", "f", "b", "w", "n"):
            d[k][b] = one[k][0]
    valid = np.ones(B, np.float32)
    valid[1] = 0.0
    left = batch(hands["C"][1], hands["faces"][1], 62, B, 17, False, True)
    first = c_fit([dict(pack=pack, valid=valid, **d)], B, cfg)[0]
    again = c_fit([dict(pack=pack, valid=valid, **d)], B, cfg)[0]
    two = c_fit([dict(pack=hands["packs"][1], **left), dict(pack=pack, valid=valid, **d)], B, cfg)[1]
    # trailing rows of weight 0 -- three more (the same tiles), then a whole extra tile -- NaN-filled, face -1
    pads = []
    for extra in (3, 31):
        e = {k: np.concatenate([d[k], np.full((B, extra) + d[k].shape[2:], -1 if k == "f" else (0.0 if k == "w" else np.nan),
                                               d[k].dtype)], 1) for k in ("y", "f", "b", "w", "n")}
        pads.append(c_fit([dict(pack=pack, valid=valid, init=None, **e)], B, cfg)[0])
    for k in NAMES:
        for b in at:
            assert np.array_equal(bits(first[k][b]), bits(alone[k][0])), (k, b)
        for other, name in ((again, "again"), (two, "two sides"), (pads[0], "+3 rows"), (pads[1], "+31 rows")):
            assert np.array_equal(bits(first[k]), bits(other[k])), (k, name)
    assert np.isnan(first["rmse"][1]) and np.isfinite(np.delete(first["rmse"], 1)).all()


# ---- 3. the rules ----------------------------------------------------------------------------------------------------------------
def test_hands_that_are_not_fitted_leave_their_neighbours_alone(hands):
    """One defect per hand, each between two good hands: face 1538, face -1, a NaN coefficient, a NaN normal, a +inf weight,
    three weighted rows, valid = 0, a NaN target, a non-finite initial value."""
    cfg = S.config(iters=3, tangent_weight=0.1)
    C, faces, pack = hands["C"][1], hands["faces"][1], hands["packs"][1]
    B, P = 19, 17
    good = batch(C, faces, 80, B, P, True, True)
    clean = c_fit([dict(pack=pack, **good)], B, cfg)[0]
    assert np.isfinite(clean["rmse"]).all()
    d = {k: (tuple(a.copy() for a in v) if k == "init" else v.copy()) for k, v in good.items()}
    valid = np.ones(B, np.float32)
    d["f"][1, 5] = 1538
    d["f"][3, 0] = -1
    d["b"][5, 6, 1] = np.nan
    d["n"][7, 8, 2] = np.nan
    d["w"][9, 3] = np.inf
    d["w"][11] = 0.0
    d["w"][11, [0, 8, 15]] = 1.0
    valid[13] = 0.0
    d["y"][15, 4, 0] = np.nan
    d["init"][1][17, 3] = np.inf
    got = c_fit([dict(pack=pack, valid=valid, **d)], B, cfg)[0]
    ref = ref_of(C, faces, d, cfg, valid)
    unfitted = S.unfitted(C)
    for b in range(B):
        if b % 2 == 0:
            for k in NAMES:
                assert np.array_equal(bits(got[k][b]), bits(clean[k][b])), (k, b)
        else:
            assert np.isnan(ref[b]["rmse"]), b
            assert got["steps"][b] == 0 and np.isnan(got["rmse"][b]) and np.isnan(got["j3d"][b]).all() and np.isnan(got["verts"][b]).all(), b
            for k in ("pose", "beta", "transl"):
                assert np.array_equal(bits(got[k][b]), bits(unfitted[k])), (b, k)
    # a NaN normal is not read at tangent_weight 1, nor are the defects of a row of weight 0; four weighted rows are fitted
    e = {k: (tuple(a.copy() for a in v) if k == "init" else v.copy()) for k, v in good.items()}
    e["n"][0, 8, 2] = np.nan
    e["w"][1, 5], e["f"][1, 5], e["b"][1, 5], e["y"][1, 5] = 0.0, 1538, np.inf, np.nan
    e["w"][2] = 0.0
    e["w"][2, [0, 5, 8, 15]] = 1.0
    cfg1 = S.config(iters=3, tangent_weight=1.0)
    sub = {k: (tuple(a[:3] for a in v) if k == "init" else v[:3]) for k, v in e.items()}
    got = c_fit([dict(pack=pack, **sub)], 3, cfg1)[0]
    ref = ref_of(C, faces, sub, cfg1)
    assert np.isfinite(got["rmse"]).all() and all(S.clear(r["trace"]) for r in ref)
    close("rules.read", got, ref)
    # weights = NULL: every row at weight 1
    plain = {k: (tuple(a[:2] for a in v) if k == "init" else v[:2]) for k, v in good.items()}
    plain["w"] = None
    for k in ("y", "b", "n"):
        plain[k] = np.nan_to_num(plain[k], nan=0.25)
    plain["f"] = np.maximum(plain["f"], 0)
    ones = dict(plain, w=np.ones((2, P), np.float32))
    a, c = c_fit([dict(pack=pack, **plain)], 2, cfg)[0], c_fit([dict(pack=pack, **ones)], 2, cfg)[0]
    assert all(np.array_equal(bits(a[k]), bits(c[k])) for k in NAMES) and np.isfinite(a["rmse"]).all()


# ---- 4. consistency with the LBS kernel and the Python layer -----------------------------------------------------------------------
def test_verts_are_the_forward_kernels_and_the_python_layer(hands):
    """``verts`` against hands_mano_heads_f32 at the returned parameters: 2e-6 m, the bar tests/test_gpu_fit_verts.py holds the
    LBS kernel to.  hands_amd.fit_mano_hands_surface gives the bits of the C entry, fit_mano_surface those of its side."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import ManoHeadsPlan
    B, P = 3, 50
    cfg = S.config(iters=5, tangent_weight=0.1)
    ds = [batch(hands["C"][i], hands["faces"][i], 90 + 10 * i, B, P, i == 0, True) for i in range(2)]
    raw = c_fit([dict(pack=hands["packs"][i], **ds[i]) for i in range(2)], B, cfg)
    t = lambda a: None if a is None else (tuple(torch.from_numpy(x).cuda() for x in a) if isinstance(a, tuple) else torch.from_numpy(a).cuda())
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": hands["packs"][0], "mano_l": hands["packs"][1]}})()
    pc = hands_amd.SurfaceFitConfig(iters=5, tangent_weight=0.1)
    fr, fl = hands_amd.fit_mano_hands_surface(t(ds[0]["y"]), t(ds[0]["f"]), t(ds[0]["b"]), t(ds[1]["y"]), t(ds[1]["f"]), t(ds[1]["b"]), pair,
                                              weights_r=t(ds[0]["w"]), weights_l=t(ds[1]["w"]), normals_r=t(ds[0]["n"]),
                                              normals_l=t(ds[1]["n"]), init_r=t(ds[0]["init"]), config=pc)
    assert list(fr) == ["pose", "beta", "transl", "rmse", "steps", "j3d", "verts", "pose_aa"]
    for f, r in ((fr, raw[0]), (fl, raw[1])):
        for k in NAMES:
            assert np.array_equal(bits(f[k].cpu().numpy()) if k != "steps" else f[k].cpu().numpy(), bits(r[k]) if k != "steps" else r[k]), k
    single = hands_amd.fit_mano_surface(t(ds[1]["y"]), t(ds[1]["f"].astype(np.int64)), t(ds[1]["b"]), hands["heads"][1], "l",
                                        weights=t(ds[1]["w"]), normals=t(ds[1]["n"]), config=pc)
    assert all(torch.equal(single[k], fl[k]) for k in single)
    rot = torch.cat([fr["pose_aa"], fl["pose_aa"]]).contiguous()
    shape = torch.cat([fr["beta"], fl["beta"]]).contiguous()
    cam = torch.ones(2 * B, 3, device="cuda")
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(B, 1, 1).cuda()
    out = ManoHeadsPlan(_lib.lib(), hands["packs"][0], hands["packs"][1], rot, shape, cam, K, 224.0, B, aa_input=True).launch(_stream())
    for h, f in (("r", fr), ("l", fl)):
        v = out[f"mano.vertices.{h}"].double() + f["transl"].double()[:, None]
        err = (v - f["verts"].double()).abs().max().item()
        print(f"FITS|lbs|{h}|{err:.3e}|2e-6")
        assert err <= 2e-6
        j = out[f"mano.joints3d.{h}"].double() + f["transl"].double()[:, None]
        assert (j - f["j3d"].double()).abs().max().item() <= 2e-6
    with pytest.raises(ValueError):
        hands_amd.fit_mano_surface(t(ds[0]["y"]), t(ds[0]["f"]), None, hands["heads"][0])
    with pytest.raises(ValueError):
        hands_amd.fit_mano_surface(t(ds[0]["y"]), t(ds[0]["f"][:, :7]), t(ds[0]["b"]), hands["heads"][0])
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.fit_mano_surface(t(ds[0]["y"]), t(ds[0]["f"]), t(ds[0]["b"]), hands["heads"][0], normals=torch.zeros(B, P, 3))


# ---- 5. rejected calls -------------------------------------------------------------------------------------------------------------
def test_rejected_calls_write_nothing(hands):
    from hands_amd import _lib
    from hands_amd._lib import FitSurfCfg, ManoFitSurfConsts, ManoFitSurfSide, ptr
    L, B, P = _lib.lib(), 2, 8
    pack = hands["packs"][0]
    x = torch.zeros(B * 144, device="cuda")
    fi = torch.zeros(B * P, dtype=torch.int32, device="cuda")
    outs = {k: torch.full((B * NV * 3,), SENT, device="cuda") for k in ("pose", "beta", "transl", "rmse", "j3d", "verts")}
    steps = torch.full((B * 4,), -77777, dtype=torch.int32, device="cuda")
    fields = [n for n, _ in ManoFitSurfSide._fields_][1:]

    def side(**drop):
        f = {k: ptr(pack[k]) for k in CONST_KEYS}
        f.update(points=ptr(x), weights=None, valid=None, init_pose=None, init_beta=None, init_transl=None, steps=ptr(steps),
                 face_idx=ptr(fi), bary=ptr(x), normals=None, **{k: ptr(v) for k, v in outs.items()})
        f.update(drop)
        return ManoFitSurfSide(ManoFitSurfConsts(*[f[k] for k in CONST_KEYS]), *[f[k] for k in fields])

    def call(sides=None, n=1, cfg=(3, 1e-6, 1e-6, 1e-3, 0.5), rows=B, pts=P, null_sides=False, null_cfg=False):
        arr = (ManoFitSurfSide * 2)(*(sides or [side(), side()]))
        c = FitSurfCfg(*cfg)
        return L.hands_mano_fit_surf_f32(None if null_sides else arr, n, None if null_cfg else ctypes.byref(c), rows, pts, _stream())

    nan, inf = float("nan"), float("inf")
    good = (3, 1e-6, 1e-6, 1e-3, 0.5)
    cases = [("sides", dict(null_sides=True)), ("cfg", dict(null_cfg=True))]
    cases += [(k, dict(sides=[side(**{k: None}), side()])) for k in CONST_KEYS + ("points", "face_idx", "bary", "pose", "beta", "transl",
                                                                                   "rmse", "steps", "j3d", "verts")]
    cases += [("second side", dict(sides=[side(), side(bary=None)], n=2))]
    cases += [("init " + "".join(k[5] for k in given), dict(sides=[side(**{k: ptr(x) for k in given}), side()]))
              for given in (("init_pose",), ("init_beta",), ("init_transl",), ("init_pose", "init_beta"),
                            ("init_pose", "init_transl"), ("init_beta", "init_transl"))]
    cases += [("B 0", dict(rows=0)), ("P 0", dict(pts=0)), ("P -1", dict(pts=-1)), ("P max + 1", dict(pts=16385)),
              ("n_sides 0", dict(n=0)), ("n_sides 3", dict(n=3)), ("iters", dict(cfg=(-1,) + good[1:]))]
    cases += [(f"cfg[{i}] {v}", dict(cfg=tuple(v if j == i else c for j, c in enumerate(good))))
              for i in (1, 2, 3) for v in (-1e-9, nan, inf, -inf)]
    cases += [(f"tau {v}", dict(cfg=good[:4] + (v,))) for v in (-1e-9, 1.0 + 1e-9, nan, inf)]
    for name, kw in cases:
        assert call(**kw) == EINVAL, name
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in outs.values()) and bool((steps == -77777).all())
    assert call(n=2, cfg=(0, 0.0, 0.0, 0.0, 0.0)) == 0                  # the table's complement
    assert call(sides=[side(normals=ptr(x), **{k: ptr(x) for k in ("init_pose", "init_beta", "init_transl")}), side()],
                cfg=good[:4] + (1.0,)) == 0
    torch.cuda.synchronize()
