"""The inputs of tests/test_gpu_fit_edges.py without a GPU: every launch of tests/fit_edge_cases.py meets, on the fp64
restatements alone, the conditions it was chosen for (``fit_edge_cases.conditions``) -- no tie decides a branch, the pivots that
must be zero are zero, row c selects start candidate c with a tenfold gap, the depth guard fires on candidates, the half turns reach
every sub-branch of Log, the weights select what DESIGN.md section 7 says -- and the restatements' handling of weights that are
no number leaves every earlier reference value as it was."""
import numpy as np
import pytest

import fit2d_ref as G
import fit_edge_cases as X
import fit_ref as F
from hands_amd.mano import synthetic_mano_asset

CONSTS = {"r": F.consts_from_asset(synthetic_mano_asset(True)), "l": F.consts_from_asset(synthetic_mano_asset(False))}
FAMILIES = {"pivot": X.pivot_launches, "intrinsics": X.intrinsics_launches, "start": X.start_launches, "depth": X.depth_launches,
            "half_turn": X.half_turn_launches, "weights": X.weight_launches, "damping": X.damping_launches}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_launches_meet_their_conditions(family):
    launches = FAMILIES[family](CONSTS)
    assert len({L["name"] for L in launches}) == len(launches)
    for L in launches:
        assert L["B"] <= 24 and L["cfg"].get("iters_rigid", 0) <= 4 and L["cfg"]["iters"] <= 4
        refs, twins = X.conditions(L, CONSTS, "cpu")
        for rr, tt in zip(refs, twins):
            keys = ("pose", "beta", "transl", "rmse") + (("j3d", "j2d") if L["dim"] == 2 else ())
            print(f"FITEDGE|{L['name']}|twin " + " ".join(f"{k} {X.twin_gap(rr, tt, k):.1e}" for k in keys) +
                  f"|steps {[r['steps'] for r in rr]}")


def test_the_pivot_is_exactly_zero_and_only_the_flag_rejects():
    """At lambda_pose = 0 with the tips unweighted, H has exactly zero rows and columns at the distal rotations, damped or not:
    the restatement's Cholesky stops there, while a factorisation that went on with the pivot replaced by 1 -- what the kernel
    does -- gives a finite step.  Only ``ok`` keeps that step from being taken."""
    L = X.pivot_launches(CONSTS)[0]
    assert L["name"] == "pivot3d.zero"
    s = L["sides"][0]
    C = CONSTS["r"]
    R, beta = s["init"][0][0].astype(np.float64), s["init"][1][0].astype(np.float64)
    w = s["w"][0].astype(np.float64)
    Jm = F.jacobian(C, R, beta, w, L["cfg"])
    H = Jm.T @ Jm
    H = H + 1e-3 * np.diag(np.diag(H))
    dead = [3 * j + c for j in (3, 6, 9, 12, 15) for c in range(3)]
    assert not H[dead].any() and not H[:, dead].any() and F.cholesky(H) is None
    live = np.setdiff1d(np.arange(F.NU), dead)
    assert F.cholesky(H[np.ix_(live, live)]) is not None


def test_weights_that_are_no_number_are_selected_out():
    """A NaN, negative or -0.0 weight is a joint that is not given: the result equals the one with that weight at 0 bit for bit,
    in both restatements, and the reported rmse is a number (``(w * e^2).sum()`` over a NaN weight was not)."""
    for L in X.weight_launches(CONSTS):
        for s in L["sides"]:
            C = CONSTS[s["h"]]
            zeroed = np.where(s["w"] > 0, s["w"], np.float32(0.0))
            if L["dim"] == 3:
                a, b = (F.fit_rows(C, s["y"], w, init=s["init"], cfg=L["cfg"]) for w in (s["w"], zeroed))
            else:
                a, b = (G.fit_rows(C, s["y"], L["K"], w, init=s["init"], cfg=L["cfg"]) for w in (s["w"], zeroed))
            for ra, rb, fitted in zip(a, b, X.WEIGHT_FITTED):
                assert bool(np.isfinite(ra["rmse"])) == fitted and ra["steps"] == rb["steps"] and ra["trace"] == rb["trace"]
                for k, v in ra["raw"].items():
                    assert np.asarray(v).tobytes() == np.asarray(rb["raw"][k]).tobytes(), (L["name"], k)


def test_the_weight_rule_leaves_the_earlier_references_alone():
    """The restatements now zero the weights they do not select.  On the inputs of every earlier parity test that line changes
    no bit of the weights -- each is positive or +0.0 --, so those tests' reference values are what they were."""
    seen = 0
    for h, base, with_init in (("r", 100, True), ("l", 200, False)):
        for mod in (F, G):
            w = mod.step_parity_inputs(CONSTS[h], base, with_init)[1]
            assert np.array_equal(np.where(w > 0, w, np.float32(0.0)).view(np.int32), w.view(np.int32))
            seen += 1
    for s in range(720):                                   # the family's weights (G.family_case hands on F's): every seed in use
        w = F.family_case(CONSTS["r"], s)[1]
        assert w.dtype == np.float32 and np.array_equal(np.where(w > 0, w, np.float32(0.0)).view(np.int32), w.view(np.int32))
    assert seen == 4 and max(F.FULL_SEEDS + G.FULL_SEEDS) < 720           # the full runs take the family's weights
