"""The branches of csrc/fit.hip (hands_mano_fit_f32, hands_mano_fit2d_f32) that the families of tests/test_gpu_fitting.py and
tests/test_gpu_fit2d.py do not reach, on the device against the fp64 restatements: a pivot that is exactly zero, general
intrinsics, each of the 24 start candidates, the depth guard on a candidate, half turns in the pose prior, weights that are no
number, negative or -0.0, and both ends of the damping.  The launches are those of tests/fit_edge_cases.py; every one goes through
the C ABI on guarded buffers (``c_fit`` of the two earlier files) and is compared through their ``close``.

Bars: those of the two earlier files, unchanged -- 4 * 2^-24 * max(1, |ref|) per float output, for 2-D the larger of that and
16 x the restatement's noise = 1e-15 twin; ``steps`` and ``start`` equal.  ``fit_edge_cases.conditions`` asserts, on the constants
read back from the device, what tests/test_fit_edges.py asserts on the CPU: no tie decides a branch of the restatement (every
decision has |c' - c| > 1e-9 c, unless a failed factorisation or an infinite c' decides), the twin takes the same steps, and for
the 3-D launches 16 x the twin stays below the floor.  No launch has more than 24 hands or more than 4 + 4 iterations.
"""
import numpy as np
import pytest
import torch

import fit2d_ref as G
import fit_edge_cases as X
import fit_ref as F
from test_gpu_fit2d import bits, hands  # noqa: F401  (the fixture: heads, packed constants, restatement constants per side)
from test_gpu_fit2d import c_fit as c_fit2d
from test_gpu_fit2d import close as close2d
from test_gpu_fitting import c_fit as c_fit3d
from test_gpu_fitting import close as close3d

pytestmark = pytest.mark.gpu


def run(L, hands):
    """One launch of fit_edge_cases on the device, compared with the restatement -> (outputs per side, references per side)."""
    Cs = {"r": hands["C"][0], "l": hands["C"][1]}
    refs, twins = X.conditions(L, Cs, "gpu")
    sides = []
    for s in L["sides"]:
        pack = hands["packs"]["rl".index(s["h"])]
        if s["flat"]:                                      # the same asset with a flat hand mean: Mref_j = Exp(0) = I
            pack = dict(pack, pose_mean=torch.zeros_like(pack["pose_mean"]))
        sides.append(dict(pack=pack, y=s["y"], w=s["w"], valid=s["valid"], init=s["init"]))
    if L["dim"] == 3:
        got = c_fit3d(sides, L["B"], L["cfg"])
    else:
        got = c_fit2d(sides, L["K"], L["B"], L["cfg"])
    for i, s in enumerate(L["sides"]):
        if L["dim"] == 3:
            close3d(f"{L['name']}.{s['h']}", got[i], refs[i])
        else:
            close2d(f"{L['name']}.{s['h']}", got[i], refs[i], twins[i])
    return got, refs


def launches(hands, family):
    return family({"r": hands["C"][0], "l": hands["C"][1]})


# ---- 1. a pivot that is not positive ---------------------------------------------------------------------------------------------
def test_a_zero_pivot_rejects_the_step(hands):
    """lambda_pose = 0, the tips unweighted: the pivots of the distal rotations are exactly 0.0.  The kernel factorises on with
    the pivot replaced by 1 and evaluates a finite candidate; only ``ok`` rejects it.  3-D: no step, the outputs are the start
    state (a caller's state bit for bit) and its rmse.  2-D: the rigid stage, whose frozen unknowns hide the zero columns, takes
    its steps and the full stage none.  The same rows at lambda_pose = 1e-6 take steps in a second launch."""
    by_name = {L["name"]: L for L in launches(hands, X.pivot_launches)}
    got, refs = run(by_name["pivot3d.zero"], hands)
    init = by_name["pivot3d.zero"]["sides"][0]["init"]
    for g in got:
        assert not g["steps"].any() and np.isfinite(g["rmse"]).all()
    for k, a in zip(("pose", "beta", "transl"), init):
        assert np.array_equal(bits(got[0][k]), bits(a)), k
    at0 = run(dict(by_name["pivot3d.zero"], name="pivot3d.zero.iters0", cfg=F.config(iters=0, lambda_pose=0.0)), hands)[0]
    for g, g0 in zip(got, at0):                            # the start state and its rmse: what no iteration at all gives
        assert all(np.array_equal(bits(g[k]), bits(g0[k])) for k in ("pose", "beta", "transl", "rmse"))
    live = run(by_name["pivot3d.live"], hands)[0]
    assert all((g["steps"] >= 1).all() for g in live)

    got, refs = run(by_name["pivot2d.zero"], hands)
    rigid = run(dict(by_name["pivot2d.zero"], name="pivot2d.zero.rigid", cfg=dict(by_name["pivot2d.zero"]["cfg"], iters=0)), hands)[0]
    for g, g0 in zip(got, rigid):                          # the full stage changed nothing
        assert (g["steps"] > 0).all() and np.array_equal(g["steps"], g0["steps"])
        assert all(np.array_equal(bits(g[k]), bits(g0[k])) for k in ("pose", "beta", "transl", "rmse", "j3d", "j2d"))
    live = run(by_name["pivot2d.live"], hands)[0]
    assert sum(int(g["steps"].sum()) for g in live) > sum(int(g["steps"].sum()) for g in got)


# ---- 2. general intrinsics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", X.INTRINSICS_STAGES)
def test_general_intrinsics(hands, stages):
    """fx != fy, two different skew entries, an off-centre principal point, all per row, row 2 of K NaN: the projection, its
    derivative and the 2 x 2 inverse of the generated start with every entry of K in its own place."""
    for L in launches(hands, X.intrinsics_launches):
        if L["name"].startswith(f"intrinsics.{stages[0]}+{stages[1]}."):
            got, refs = run(L, hands)
            assert (got[0]["start"] == -1).all() and (got[1]["start"] >= 0).all()


# ---- 3. all 24 start candidates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain", "general", "weighted"])
def test_every_start_candidate_is_selected(hands, name):
    """Row c is the rest hand under G_c: the kernel's tables (p0, p1, the parity and the sign bits) must select c and build G_c."""
    (L,) = [L for L in launches(hands, X.start_launches) if L["name"] == f"start.{name}"]
    got, refs = run(L, hands)
    for g in got:
        assert np.array_equal(g["start"], np.arange(24, dtype=np.int32)), g["start"]
        assert np.array_equal(g["pose"][:, 0], np.stack(G.START).astype(np.float32))


# ---- 4. the depth guard on a candidate -----------------------------------------------------------------------------------------------
def test_the_depth_guard_rejects_a_candidate(hands):
    """z_min 1e-3 m behind the nearest weighted joint of a caller's state: the restatement's trace has candidates of cost +inf,
    all rejected, and accepted steps after them; the kernel ends in the same state after the same number of steps."""
    for L in launches(hands, X.depth_launches):
        got, refs = run(L, hands)
        assert got[0]["steps"][0] >= 3 and got[0]["j3d"][0][L["sides"][0]["w"][0] > 0, 2].min() > L["cfg"]["z_min"]


# ---- 5. half turns in the pose prior -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 3])
def test_half_turns_in_the_pose_prior_3d(hands, iters):
    """Mref_j = I and finger rotations that are exact half turns (or the identity): the third branch of Log, each of its three
    sub-branches with each pattern of sign changes, and the >= ties, at lambda_pose = 1e-2 so that the prior decides the steps."""
    (L,) = [L for L in launches(hands, X.half_turn_launches) if L["name"] == f"halfturn3d.{iters}"]
    got, refs = run(L, hands)
    assert all((g["steps"] == iters).all() for g in got)


@pytest.mark.parametrize("stages", [(0, 0), (1, 2)])
def test_half_turns_in_the_pose_prior_2d(hands, stages):
    for own in ("mean", "own"):
        (L,) = [L for L in launches(hands, X.half_turn_launches) if L["name"] == f"halfturn2d.{stages[0]}+{stages[1]}.{own}"]
        run(L, hands)


# ---- 6. weights that are no number, negative or -0.0 ---------------------------------------------------------------------------------
def test_weights_that_select_nothing(hands):
    """NaN, -1, -inf, -0.0 and a denormal positive weight, NaN coordinates under every joint that is not selected.  Four selected
    joints among NaN weights are fitted, three are not (unfitted outputs, rmse NaN); a denormal is positive and counts; a
    selected weight of +inf leaves the row unfitted, with and without a caller's state."""
    for L in launches(hands, X.weight_launches):
        got, refs = run(L, hands)
        for i, g in enumerate(got):
            assert list(np.isfinite(g["rmse"])) == list(X.WEIGHT_FITTED)
            unfitted = (F if L["dim"] == 3 else G).unfitted(hands["C"][i])
            for b in (2, 5):
                assert g["steps"][b] == 0 and all(np.array_equal(bits(g[k][b]), bits(unfitted[k])) for k in ("pose", "beta", "transl"))
                if L["dim"] == 2:
                    assert g["start"][b] == -1 and np.isnan(g["j3d"][b]).all() and np.isnan(g["j2d"][b]).all()


# ---- 7. the damping's ends ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu0", [0.0, 1e7])
def test_the_ends_of_the_damping(hands, mu0):
    """mu0 = 0: H is not damped and an accepted step clamps mu to MU_MIN from below; mu0 = 1e7: above MU_MAX, steps of 1e-7 of
    the Gauss-Newton step are accepted with relative decreases of 1e-7 and up."""
    for L in launches(hands, X.damping_launches):
        if L["cfg"]["mu0"] == mu0:
            run(L, hands)
