"""The branches of csrc/fit_verts.hip (hands_mano_fit_verts_f32) that the family cases of tests/test_gpu_fit_verts.py do not reach,
on the device against the fp64 restatement tests/fit_verts_ref.py: a pivot that is exactly zero, the Kabsch start on a mirrored, a
planar, a far and the rest hand's own target, the geometry of the four-round selection count, weights that are no number, negative,
-0.0, denormal or +inf, both ends of the damping and a fit without priors, half turns in the pose prior, the five tips under
weight 0, and the outputs after a last iteration that was rejected.  The launches are those of tests/fit_verts_edge_cases.py; every
one goes through the C ABI on guarded buffers (``c_fit`` of tests/test_gpu_fit_verts.py) and is compared through that file's ``close``.

The bar is that file's, unchanged: 4 * 2^-24 * max(1, |ref|) per float output, NaN positions equal, ``steps`` equal.
``fit_verts_edge_cases.conditions`` asserts, on the constants read back from the (modified) device pack, what
tests/test_fit_verts_edges.py asserts on the CPU: every decision of the restatement has |c' - c| > 1e-9 c unless a failed
factorisation decides it, the noise = 1e-15 twin takes the same steps, and 16 x the twin's difference stays below the bar at every
element.  No launch has more than 8 hands or more than 6 iterations.
"""
import numpy as np
import pytest
import torch

import fit_verts_edge_cases as E
import fit_verts_ref as V
from test_gpu_fit_verts import bits, c_fit, close, hands  # noqa: F401  (the fixture: heads, packed constants, restatement constants)

pytestmark = pytest.mark.gpu

ALL = E.FLOATS + ("steps",)
STATE = ("pose", "beta", "transl")


def modified_pack(pack, mod):
    """The device pack with the tensors ``mod`` names replaced (fit_verts_edge_cases.modified on the device)."""
    if mod is None:
        return pack
    if mod == "flat":
        return dict(pack, pose_mean=torch.zeros_like(pack["pose_mean"]))
    out = dict(pack)
    for k in ("shapedirs", "J_shapedirs"):
        t = pack[k].clone().reshape(-1, 10)
        t[:, mod[1]] = 0.0
        out[k] = t.reshape(pack[k].shape).contiguous()
    return out


def run(L, hands, ys=None):
    """One launch on the device, compared with the restatement -> (outputs per side, references per side).  ``ys``: targets
    that replace the launch's on the device only -- the reference stays that of the launch."""
    Cs = {"r": hands["C"][0], "l": hands["C"][1]}
    sides = []
    for i, s in enumerate(L["sides"]):
        pack = modified_pack(hands["packs"]["rl".index(s["h"])], s["mod"])
        if s["mod"] is not None:                           # the matching constants, read back from the modified pack
            Cs[(s["h"], s["mod"])] = V.consts_from_pack(pack)
        sides.append(dict(pack=pack, y=s["y"] if ys is None else ys[i], w=s["w"], valid=s["valid"], init=s["init"]))
    refs, twins = E.conditions(L, Cs, "gpu")
    got = c_fit(sides, L["B"], L["cfg"])
    for i, s in enumerate(L["sides"]):
        close(f"{L['name']}.{s['h']}", got[i], refs[i])
    return got, refs


def launches(hands, family):
    return {L["name"]: L for L in E.FAMILIES[family]({"r": hands["C"][0], "l": hands["C"][1]})}


def same_bits(a, b, keys=ALL):
    return all(np.array_equal(a[k], b[k]) if k == "steps" else np.array_equal(bits(a[k]), bits(b[k])) for k in keys)


def other_non_finite(y, hide):
    """y with every coordinate of the vertices ``hide`` (a mask) replaced: +inf, -inf and a NaN of another payload in turn."""
    out = y.copy()
    vals = np.array([np.inf, -np.inf, 0.0], np.float32)
    vals[2:] = np.array([0x7FC01234], np.uint32).view(np.float32)
    fill = vals[np.arange(out.size).reshape(out.shape) % 3]
    out[hide] = fill[hide]
    assert not np.isfinite(out[hide]).any() and not np.array_equal(bits(out[hide]), bits(y[hide]))
    return out


# ---- 1. a pivot that is exactly zero ---------------------------------------------------------------------------------------------
def test_a_zero_pivot_rejects_the_step(hands):
    """lambda_beta = 0 on a pack whose shape column l is zero (l = 0 right, l = 9 left): the pivot of unknown 48 + l is exactly
    0.0.  The kernel factorises on with the pivot replaced by 1 and evaluates a finite candidate; only ``ok`` rejects it, and
    the outputs -- j3d and rmse too, which the candidate's evaluation overwrote in LDS -- are those of no iteration at all."""
    by_name = launches(hands, "pivot")
    got, _ = run(by_name["pivot.zero"], hands)
    at0, _ = run(by_name["pivot.zero.iters0"], hands)
    for g, g0 in zip(got, at0):
        assert not g["steps"].any() and np.isfinite(g["rmse"]).all() and np.isfinite(g["j3d"]).all()
        assert same_bits(g, g0)
    init = by_name["pivot.zero"]["sides"][0]["init"]
    for k, a in zip(STATE, init):                          # a caller's state comes back bit for bit
        assert np.array_equal(bits(got[0][k]), bits(a)), k
    live, _ = run(by_name["pivot.live"], hands)
    assert all((g["steps"] >= 1).all() for g in live)


# ---- 2. the Kabsch start away from a rotated hand ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kabsch.0", "kabsch.3", "kabsch.rest.1"])
def test_the_kabsch_start(hands, name):
    """A mirrored target (the proper rotation needs the sign of det V), a planar one (rank 2: U_2 = U_0 x U_1), one tens of metres
    away (the centring sums) and the rest hand itself (K symmetric, R_0 = I).  At iters = 0 the state is the Kabsch state: a
    proper rotation, the fingers M_j, beta = 0, and rmse and j3d are those of that state."""
    L = launches(hands, "kabsch")[name]
    got, refs = run(L, hands)
    if L["cfg"]["iters"]:
        return
    for i, (g, s) in enumerate(zip(got, L["sides"])):
        C = hands["C"][i]
        for b in range(L["B"]):
            R0 = g["pose"][b, 0].astype(np.float64)
            assert np.linalg.norm(R0.T @ R0 - np.eye(3)) <= 1e-6 and np.linalg.det(R0) > 0, (s["h"], E.KABSCH_ROWS[b], R0)
            assert np.array_equal(bits(g["pose"][b, 1:]), bits(C.M[1:].astype(np.float32))) and not g["beta"][b].any()
            Ev = V.evaluate(C, g["pose"][b].astype(np.float64), np.zeros(10))
            t = g["transl"][b].astype(np.float64)
            j3d, rmse = Ev["joints"] + t, V.rmse_of(C, None, None, t, s["y"][b].astype(np.float64), np.ones(V.NV), Ev)
            assert (np.abs(g["j3d"][b] - j3d) <= E.bar(j3d)).all() and abs(g["rmse"][b] - rmse) <= E.bar(rmse), (s["h"], E.KABSCH_ROWS[b])


# ---- 3. the geometry of the selection -----------------------------------------------------------------------------------------------
def test_the_geometry_of_the_selection(hands):
    """Four weighted vertices one per round of the count, four in the tail tile beside the absent vertices, the tail tile alone,
    one vertex slot of every tile, one tile: fitted.  Three vertices spread over the rounds, and three in the tail: the
    unfitted row bit for bit."""
    (L,) = launches(hands, "selection").values()
    got, refs = run(L, hands)
    for i, g in enumerate(got):
        u = V.unfitted(hands["C"][i])
        for b, fitted in enumerate(E.SELECTION_FITTED):
            if fitted:
                assert np.isfinite(g["rmse"][b]) and g["steps"][b] >= 1, (i, b)
            else:
                assert g["steps"][b] == 0 and np.isnan(g["rmse"][b]) and np.isnan(g["j3d"][b]).all(), (i, b)
                assert all(np.array_equal(bits(g[k][b]), bits(u[k])) for k in STATE), (i, b)


# ---- 4. weights that select nothing, a denormal and +inf ----------------------------------------------------------------------------
def test_weights_that_select_nothing(hands):
    """NaN, -1, -inf, -0.0 and a denormal positive weight interleaved, NaN coordinates under every weight that does not select;
    four selected vertices among NaN weights are fitted, three are not, a selected weight of +inf is not.  Whatever lies under a
    weight that does not select is never read into arithmetic: other non-finite values there change no output bit."""
    (L,) = launches(hands, "weights").values()
    got, refs = run(L, hands)
    for i, g in enumerate(got):
        assert list(np.isfinite(g["rmse"])) == list(E.WEIGHT_FITTED)
        u = V.unfitted(hands["C"][i])
        for b, fitted in enumerate(E.WEIGHT_FITTED):
            if not fitted:
                assert g["steps"][b] == 0 and np.isnan(g["j3d"][b]).all(), (i, b)
                assert all(np.array_equal(bits(g[k][b]), bits(u[k])) for k in STATE), (i, b)
    again, _ = run(L, hands, ys=[other_non_finite(s["y"], ~(s["w"] > 0)) for s in L["sides"]])
    assert all(same_bits(a, g) for a, g in zip(again, got))


# ---- 5. the damping's ends, and no priors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["damping.mu0", "damping.mu1e7", "damping.nopriors"])
def test_the_ends_of_the_damping(hands, name):
    """mu0 = 0: H is not damped and an accepted step clamps mu to MU_MIN from below; mu0 = 1e7: above MU_MAX, tiny steps with
    relative decreases of 1e-7 and up; lambda_beta = lambda_pose = 0: the data rows alone make H positive definite."""
    got, refs = run(launches(hands, "damping")[name], hands)
    assert all((g["steps"] >= 2).all() for g in got)


# ---- 6. half turns in the pose prior ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("lp", [1e-6, 1e-2])
def test_half_turns_in_the_pose_prior(hands, lp, iters):
    """pose_mean = 0 and finger rotations that are exact half turns (or the identity): the third branch of Log inside
    joint_state, each of its sub-branches with each pattern of sign changes and the >= ties, and entries of -2 in R_j - I for the
    pose blend shapes of the walk."""
    got, refs = run(launches(hands, "halfturn")[f"halfturn.{lp:g}.{iters}"], hands)
    if iters:
        assert all((g["steps"] >= 1).all() for g in got)


# ---- 7. the five tips under weight 0 ------------------------------------------------------------------------------------------------
def test_the_tips_under_weight_zero(hands):
    """Weight 0 and NaN targets on vertices 744, 320, 443, 554, 671: rows 16..20 of j3d are finite all the same and inside the
    bar, and another non-finite value under the tips changes no output bit.  A second row weights the tips and 20 others only."""
    (L,) = launches(hands, "tips").values()
    got, refs = run(L, hands)
    for i, g in enumerate(got):
        ref = np.asarray(refs[i][0]["raw"]["j3d"])[16:21]
        assert np.isfinite(g["j3d"][:, 16:21]).all() and (np.abs(g["j3d"][0, 16:21] - ref) <= E.bar(ref)).all()
        assert (g["steps"] >= 1).all()
    ys = []
    for s in L["sides"]:
        hide = np.zeros(s["w"].shape, bool)
        hide[0, list(E.TIP_VERTS)] = True
        assert np.isnan(s["y"][hide]).all()
        ys.append(other_non_finite(s["y"], hide))
    again, _ = run(L, hands, ys=ys)
    assert all(same_bits(a, g) for a, g in zip(again, got))


# ---- 8. a last iteration that was rejected ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", E.REJECTED_AT)
def test_the_outputs_after_a_rejected_last_iteration(hands, k):
    """Decision k of the restatement is a clear rejection: the launch at iters = k + 1 returns what the launch at iters = k
    returns, bit for bit -- the joints, the tips and the data cost in LDS belong to the rejected candidate until the current
    state is evaluated again."""
    by_name = launches(hands, "rejected")
    before, refs0 = run(by_name[f"rejected.{k}"], hands)
    after, refs1 = run(by_name[f"rejected.{k + 1}"], hands)
    assert refs1[0][0]["trace"][k][3] is False and refs0[0][0]["steps"] == refs1[0][0]["steps"]
    assert same_bits(after[0], before[0]) and np.isfinite(after[0]["rmse"]).all() and np.isfinite(after[0]["j3d"]).all()
