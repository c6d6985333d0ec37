"""The inputs of tests/test_gpu_fit_verts_edges.py without a GPU: every launch of tests/fit_verts_edge_cases.py meets, on the fp64
restatement alone, the conditions it was chosen for (``fit_verts_edge_cases.conditions``) -- no tie decides a branch, the noise twin
takes the same steps and stays 16 x below the bar, the pivot that must be zero is zero, the Kabsch targets have rank 2 or more, the
selections and the weights select what DESIGN.md section 7 says, the half turns reach every sub-branch of Log, and the rejected
iterations are clear rejections -- and a selected weight of +inf leaves a row unfitted in all three restatements."""
import numpy as np
import pytest

import fit2d_ref as G
import fit_edge_cases as X
import fit_ref as F
import fit_verts_edge_cases as E
import fit_verts_ref as V
from hands_amd.mano import synthetic_mano_asset

ASSETS = {"r": synthetic_mano_asset(True), "l": synthetic_mano_asset(False)}
CONSTS = {h: V.consts_from_asset(a) for h, a in ASSETS.items()}


@pytest.mark.parametrize("family", list(E.FAMILIES))
def test_the_launches_meet_their_conditions(family):
    launches = E.FAMILIES[family](CONSTS)
    assert len({L["name"] for L in launches}) == len(launches)
    for L in launches:
        refs, twins = E.conditions(L, CONSTS, "cpu")
        for s, rr, tt in zip(L["sides"], refs, twins):
            gaps = " ".join(f"{k} {X.twin_gap(rr, tt, k):.1e}" for k in E.FLOATS)
            m = [x for r in rr for x in E.margins(r)]
            print(f"FITVEDGE|{L['name']}.{s['h']}|twin {gaps}|steps {[r['steps'] for r in rr]}|smallest margin {min(m, default=np.inf):.1e}")


def test_the_pivot_is_exactly_zero_and_only_the_flag_rejects():
    """On the pack with a dead shape column l and lambda_beta = 0, H[48 + l, 48 + l] is exactly 0.0 and its row and column are
    zero, damped or not: the restatement's Cholesky stops there, while a factorisation that went on with the pivot replaced by
    1 -- what the kernel does -- has every other pivot positive and gives a finite step.  Only ``ok`` keeps it from being taken."""
    L = E.pivot_launches(CONSTS)[0]
    assert L["name"] == "pivot.zero" and L["cfg"]["lambda_beta"] == 0.0
    for s in L["sides"]:
        C = E.consts_of(CONSTS, s)
        u = 48 + s["mod"][1]
        if s["init"] is not None:
            R, beta = s["init"][0][0].astype(np.float64), s["init"][1][0].astype(np.float64)
        else:
            R, beta = V.rest_pose(C), np.zeros(10)
        Jm = V.jacobian(C, R, beta, s["w"][0].astype(np.float64), L["cfg"])
        assert not Jm[:, u].any()
        H = Jm.T @ Jm
        assert H[u, u] == 0.0 and not np.signbit(H[u, u])
        H = H + 1e-3 * np.diag(np.diag(H))
        assert H[u, u] == 0.0 and not H[u].any() and not H[:, u].any() and V.cholesky(H) is None
        live = np.setdiff1d(np.arange(V.NU), [u])
        assert V.cholesky(H[np.ix_(live, live)]) is not None
        assert (np.diag(H)[live] > 0).all()


def test_a_weight_of_plus_infinity_leaves_the_row_unfitted():
    """A selected weight that is not finite: the unfitted row in all three restatements, with and without a caller's state; the
    same rows with that weight finite are fitted."""
    (L,) = E.weight_launches(CONSTS)
    for s in L["sides"]:
        C = CONSTS[s["h"]]
        assert np.isposinf(s["w"][3, E.INF_AT])
        init = None if s["init"] is None else tuple(a[3] for a in s["init"])
        r = V.fit(C, s["y"][3], s["w"][3], init=init, cfg=L["cfg"])
        u = V.unfitted(C)
        assert r["steps"] == 0 and np.isnan(r["rmse"]) and np.isnan(r["j3d"]).all() and r["trace"] == []
        assert all(np.array_equal(r[k], u[k]) for k in ("pose", "beta", "transl"))
        finite = s["w"][3].copy()
        finite[E.INF_AT] = 3.0
        assert np.isfinite(V.fit(C, s["y"][3], finite, init=init, cfg=L["cfg"])["rmse"])
    CJ = {h: F.consts_from_asset(a) for h, a in ASSETS.items()}
    for L in X.weight_launches(CJ):
        mod = F if L["dim"] == 3 else G
        for s in L["sides"]:
            C = CJ[s["h"]]
            assert np.isposinf(s["w"][5]).sum() == 1 and X.WEIGHT_FITTED[5] is False
            for w, fitted in ((s["w"][5], False), (np.where(np.isinf(s["w"][5]), np.float32(3.0), s["w"][5]), True)):
                init = None if s["init"] is None else tuple(a[5] for a in s["init"])
                args = (C, s["y"][5]) + ((L["K"][5],) if L["dim"] == 2 else ())
                r = mod.fit(*args, w, init=init, cfg=L["cfg"])
                assert bool(np.isfinite(r["rmse"])) == fitted, (L["name"], s["h"], fitted)
                if not fitted:
                    u = mod.unfitted(C)
                    assert r["steps"] == 0 and all(np.array_equal(r[k], u[k]) for k in ("pose", "beta", "transl"))
