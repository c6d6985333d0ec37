"""Inputs for the edge and branch tests of the two fitting kernels of csrc/fit.hip (tests/test_fit_edges.py on the CPU,
tests/test_gpu_fit_edges.py on the device): small deterministic launches that reach what the random families do not -- a pivot
that is exactly zero, general intrinsics, each of the 24 start candidates, the depth guard on a candidate, half turns in the pose
prior, weights that are no number, negative or -0.0, and both ends of the damping.  Pure numpy on top of the two restatements.

A *launch* is a dict: ``name``, ``dim`` (3: hands_mano_fit_f32, 2: hands_mano_fit2d_f32), ``cfg``, ``K`` ((B,3,3) fp32, 2-D only),
``B`` and ``sides``, a list of dict(h = "r" / "l", flat, y, w, valid, init).  ``flat``: the asset with pose_mean replaced by zeros,
so that Mref_j = I exactly.  ``reference`` runs the restatement and its noise = 1e-15 twin over a launch, once per process.
"""
import math

import numpy as np

import fit2d_ref as G
import fit_ref as F

TIPS = (16, 17, 18, 19, 20)
K_GENERAL = np.array([[900.0, 3.0, 120.0], [-2.0, 1100.0, 100.0], [0.0, 0.0, 1.0]])
NAN = float("nan")


def plain_K(B):
    return np.repeat(G.K_TEST[None], B, 0).astype(np.float32)


def general_K(B):
    """(B,3,3) fp32: fx != fy, both skew entries non-zero and different, an off-centre principal point, all varied per row; row 2
    is NaN, since nothing reads it."""
    K = np.repeat(K_GENERAL[None], B, 0)
    b = np.arange(B)
    K[:, 0, 0] += 7.0 * b
    K[:, 1, 1] -= 5.0 * b
    K[:, 0, 1] += 0.5 * b
    K[:, 1, 0] -= 0.25 * b
    K[:, 0, 2] += 2.0 * b
    K[:, 1, 2] -= 3.0 * b
    K[:, 2] = NAN
    return K.astype(np.float32)


def project_rows(y3, K):
    """(B,21,3) camera points, NaN where a joint is not given -> (B,21,2) fp32 pixels under K[b], NaN in the same places."""
    out = np.stack([G.project(K[b].astype(np.float64), np.nan_to_num(y3[b].astype(np.float64), nan=1.0)) for b in range(len(y3))])
    out[np.isnan(y3).any(2)] = NAN
    return out.astype(np.float32)


def flat_consts(C):
    """C with pose_mean = 0: the flat-hand-mean configuration, M_j = Exp(0) = I exactly."""
    return F.Consts(np.zeros(48), C.J_template, C.J_shapedirs, C.tip_v, C.tip_sd, C.tip_w, C.tip_pd)


def side(h, y, w=None, init=None, valid=None, flat=False):
    return {"h": h, "y": y, "w": w, "init": init, "valid": valid, "flat": flat}


def launch(name, dim, sides, cfg, K=None):
    return {"name": name, "dim": dim, "sides": sides, "cfg": cfg, "K": K, "B": len(sides[0]["y"])}


def consts_of(Cs, s):
    return flat_consts(Cs[s["h"]]) if s["flat"] else Cs[s["h"]]


_REF = {}


def reference(L, Cs, key):
    """-> (refs, twins): per side the restatement's results per row and those of its noise = 1e-15 twin.  ``key`` names the set
    of constants ``Cs`` ({"r": Consts, "l": Consts}); computed once per (key, launch)."""
    k = (key, L["name"])
    if k not in _REF:
        refs, twins = [], []
        for s in L["sides"]:
            C = consts_of(Cs, s)
            if L["dim"] == 3:
                run = lambda **kw: F.fit_rows(C, s["y"], s["w"], s["valid"], s["init"], L["cfg"], **kw)
            else:
                run = lambda **kw: G.fit_rows(C, s["y"], L["K"], s["w"], s["valid"], s["init"], L["cfg"], **kw)
            refs.append(run())
            twins.append(run(noise=1e-15, seed=5))
        _REF[k] = (refs, twins)
    return _REF[k]


def decided(res, rel=1e-9):
    """No tie decides: every accept / reject decision of a result's trace has |c' - c| > rel * c, unless the factorisation failed
    or c' is +inf -- those decide by themselves."""
    return all((not ok) or math.isinf(c2) or abs(c2 - c) > rel * c for c, c2, ok, _ in res["trace"])


def twin_gap(refs, twins, k):
    """The largest difference of output k between the restatement and its twin over the rows of one side."""
    a = np.stack([np.asarray(r["raw"][k], np.float64) for r in refs])
    b = np.stack([np.asarray(r["raw"][k], np.float64) for r in twins])
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(a - b), initial=0.0))


def _family_rows(C, seeds, rng, with_init):
    """Family cases with unit weights: y (B,21,3) fp32, and a caller's state near the truth (as F.step_parity_inputs builds it)."""
    ys, init = [], ([], [], [])
    for s in seeds:
        y, _, (R, beta, t) = F.family_case(C, s)
        ys.append(y.copy())
        init[0].append(np.stack([R[j] @ F.exp_so3(0.2 * rng.randn(3)) for j in range(16)]))
        init[1].append(beta + 0.3 * rng.randn(10))
        init[2].append(t + 0.02 * rng.randn(3))
    return np.stack(ys), (tuple(np.stack(a).astype(np.float32) for a in init) if with_init else None)


# ---- 1. a pivot that is not positive ---------------------------------------------------------------------------------------------
PIVOT_SEEDS = (4, 5, 6)


def pivot_launches(Cs):
    """lambda_pose = 0 and weight 0 on the five tips: the columns of the distal rotations (joints 3, 6, 9, 12, 15) are exactly
    zero, their pivot is 0.0 on the host and on the device alike, and every full iteration is a rejected step.  The same rows at
    lambda_pose = 1e-6 take steps.  Right hand from a caller's state, left from the generated start, both in each launch."""
    out = []
    w = np.ones((len(PIVOT_SEEDS), 21), np.float32)
    w[:, TIPS] = 0.0
    rows = {}
    for h, with_init in (("r", True), ("l", False)):
        y3, init = _family_rows(Cs[h], PIVOT_SEEDS, np.random.RandomState(1004), with_init)
        y3[:, TIPS] = NAN
        rows[h] = (y3, init)
    for name, lp in (("zero", 0.0), ("live", 1e-6)):
        out.append(launch(f"pivot3d.{name}", 3, [side(h, rows[h][0], w, rows[h][1]) for h in "rl"], F.config(iters=4, lambda_pose=lp)))
        K = plain_K(len(PIVOT_SEEDS))
        out.append(launch(f"pivot2d.{name}", 2, [side(h, project_rows(rows[h][0], K), w, rows[h][1]) for h in "rl"],
                          G.config(iters_rigid=3, iters=4, lambda_pose=lp), K))
    return out


# ---- 2. general intrinsics ---------------------------------------------------------------------------------------------------------
INTRINSICS_STAGES = ((0, 0), (2, 1), (2, 3))


def intrinsics_launches(Cs):
    """The rows of the step-parity test (uneven weights, five zero weights with NaN under them, a keypoint displaced by 80 px in
    row 3) projected with a general K per row; plain and with sigma = 30 px; the right hand from a caller's state with
    prior_to_init, the left from the generated start."""
    K = general_K(5)
    sides = []
    for h, base, with_init in (("r", 100, True), ("l", 200, False)):
        y3, w, init = F.step_parity_inputs(Cs[h], base, with_init)
        y = project_rows(y3, K)
        y[3, 9] += np.float32(80.0)
        sides.append(side(h, y, w, init))
    out = []
    for st in INTRINSICS_STAGES:
        for name, sigma in (("plain", 0.0), ("sigma30", 30.0)):
            out.append(launch(f"intrinsics.{st[0]}+{st[1]}.{name}", 2, sides,
                              G.config(iters_rigid=st[0], iters=st[1], robust_sigma=sigma, prior_to_init=True), K))
    return out


# ---- 3. all 24 start candidates ----------------------------------------------------------------------------------------------------
def _start_rows(C, K):
    """Row c: the rest hand turned by G_c about its wrist joint, at a depth of about 0.7 m, projected with K[c]."""
    E = F.evaluate(C, F.rest_pose(C), np.zeros(10))
    J0 = E["J"][0]
    x = E["joints"] - J0
    y3 = np.stack([x @ Gc.T + J0 + np.array([0.012 - 0.001 * c, -0.008 + 0.0007 * c, 0.7 + 0.005 * (c % 5)]) for c, Gc in enumerate(G.START)])
    return project_rows(y3, K)


def start_launches(Cs, weight_seed=28):
    """B = 24, no iteration: row c must select candidate c.  Under the plain and under the general K; and once more under the
    general K with uneven weights, of which three per row are zero with NaN keypoints under them."""
    cfg = G.config(iters_rigid=0, iters=0)
    rng = np.random.RandomState(weight_seed)
    w = rng.uniform(0.5, 2.0, (24, 21)).astype(np.float32)
    for c in range(24):
        w[c, rng.choice(21, 3, replace=False)] = 0.0
    out = []
    for name, K, weighted in (("plain", plain_K(24), False), ("general", general_K(24), False), ("weighted", general_K(24), True)):
        sides = []
        for h in "rl":
            y = _start_rows(Cs[h], K)
            if weighted:
                y[w == 0] = NAN
            sides.append(side(h, y, w if weighted else None))
        out.append(launch(f"start.{name}", 2, sides, cfg, K))
    return out


def start_gaps(Cs, L):
    """Per side and row of a start launch: (the winning candidate, the runner-up's eps over the winner's)."""
    out = []
    for s in L["sides"]:
        C = consts_of(Cs, s)
        rows = []
        for b in range(L["B"]):
            w = np.ones(21) if s["w"] is None else s["w"][b].astype(np.float64)
            sel = w > 0
            y = np.where(sel[:, None], s["y"][b].astype(np.float64), 0.0)
            scores = sorted(G.start_scores(C, y, np.where(sel, w, 0.0), L["K"][b].astype(np.float64))[0])
            rows.append((scores[0][1], scores[1][0] / scores[0][0] if len(scores) > 1 else math.inf))
        out.append(rows)
    return out


# ---- 4. the depth guard on a candidate -----------------------------------------------------------------------------------------------
def depth_launches(Cs):
    """A caller's state, z_min 1e-3 m behind its nearest weighted joint: steps that bring a weighted joint to z_min or nearer cost
    +inf and are rejected, later ones are accepted.  z_min belongs to the launch, so every row has a launch of its own."""
    C = Cs["r"]
    y, w, init = G.step_parity_inputs(C, 100, True)
    out = []
    for b in range(5):
        R, beta, t = (a[b].astype(np.float64) for a in init)
        z = float((F.joints_of(C, R, beta) + t)[w[b] > 0, 2].min())
        out.append(launch(f"depth.row{b}", 2, [side("r", y[b:b + 1], w[b:b + 1], tuple(a[b:b + 1] for a in init))],
                          G.config(iters_rigid=3, iters=4, z_min=z - 1e-3), plain_K(1)))
    return out


# ---- 5. half turns in the pose prior -------------------------------------------------------------------------------------------------
def _half_turn(u):
    u = np.asarray(u, np.float64)
    return 2.0 * np.outer(u, u) / float(u @ u) - np.eye(3)


# exact in fp32, entries 0 / +-1: about the three axes and about four face diagonals
HALF_TURNS = [np.diag(d).astype(np.float64) for d in ((1, -1, -1), (-1, 1, -1), (-1, -1, 1))] + \
             [_half_turn(u) for u in ((1, 1, 0), (1, -1, 0), (1, 0, 1), (0, 1, -1))]
# rounded to fp32 they stay exactly symmetric (s = 0, so the half-turn branch is taken) with one axis component strictly the
# largest and the other two not zero: the sign flips of the second and third sub-branch, which no 0 / +-1 matrix reaches
OBLIQUE_TURNS = [_half_turn(u).astype(np.float32).astype(np.float64)
                 for u in ((3, 1, -2), (3, -1, -2), (-1, 3, -2), (-2, 3, 1), (-1, -2, 3), (1, -2, 3), (-2, 1, 3))]
# the joints that carry them, per row: over different fingers, proximal, middle and distal
HALF_TURN_JOINTS = ((1, 5, 9, 10, 14, 3, 7), (2, 6, 7, 11, 15, 1, 4), (3, 4, 8, 12, 13, 2, 5), (1, 5, 9, 10, 14, 3, 7))
HALF_TURN_SEEDS = (5, 6, 8, 9)


def half_turn_rows(C):
    """C: flat constants.  -> y3 (4,21,3) of family cases, and an initial state whose finger rotations are exact half turns on
    seven joints per row (rows 0..2: HALF_TURNS in rotating order, row 3: OBLIQUE_TURNS) and the identity on the other eight."""
    rng = np.random.RandomState(1005)
    y3, near = _family_rows(C, HALF_TURN_SEEDS, rng, True)
    pose = near[0].copy()
    pose[:, 1:] = np.eye(3, dtype=np.float32)
    for b, joints in enumerate(HALF_TURN_JOINTS):
        turns = OBLIQUE_TURNS if b == 3 else HALF_TURNS[b:] + HALF_TURNS[:b]
        for j, T in zip(joints, turns):
            pose[b, j] = T.astype(np.float32)
    return y3, (pose, near[1], near[2])


def half_turn_launches(Cs):
    out = []
    rows = {h: half_turn_rows(flat_consts(Cs[h])) for h in "rl"}
    for iters in (0, 1, 3):
        out.append(launch(f"halfturn3d.{iters}", 3, [side(h, rows[h][0], None, rows[h][1], flat=True) for h in "rl"],
                          F.config(iters=iters, lambda_pose=1e-2)))
    K = plain_K(4)
    for st in ((0, 0), (1, 2)):
        for own in (False, True):
            out.append(launch(f"halfturn2d.{st[0]}+{st[1]}.{'own' if own else 'mean'}", 2,
                              [side(h, project_rows(rows[h][0], K), None, rows[h][1], flat=True) for h in "rl"],
                              G.config(iters_rigid=st[0], iters=st[1], lambda_pose=1e-2, prior_to_init=own), K))
    return out


# ---- 6. weights that are no number, negative or -0.0 ---------------------------------------------------------------------------------
WEIGHT_SEEDS = (21, 22, 23, 24, 25, 26)
WEIGHT_FITTED = (True, True, False, True, True, False)
DENORMAL = 1e-40                                  # positive and below the smallest normal fp32 (1.18e-38)


def odd_weights():
    """(6,21) fp32.  Row 0: NaN, -1, -inf, -0.0 and a denormal among ones; row 1: four selected among NaN; row 2: three selected
    among NaN (not fitted); row 3: five uneven weights among negative ones; row 4: three selected and a denormal among -0.0 --
    the denormal is the fourth, so the row is fitted only where a denormal counts as positive; row 5: one +inf among ones -- a
    selected weight that is not finite, so the row is not fitted."""
    w = np.ones((6, 21), np.float32)
    w[0, [1, 5, 19]], w[0, 8], w[0, 11], w[0, [12, 17]], w[0, 3] = NAN, -1.0, -np.inf, -0.0, DENORMAL
    w[1] = NAN
    w[1, [0, 4, 9, 18]] = 2.0
    w[2] = NAN
    w[2, [0, 7, 20]] = 1.0
    w[3] = -1.0
    w[3, [0, 2, 6, 13, 20]] = (0.5, 3.0, 1.0, 2.0, 0.25)
    w[4] = -0.0
    w[4, [0, 4, 13]], w[4, 18] = 2.0, DENORMAL
    w[5, 7] = np.inf
    return w


def weight_launches(Cs):
    """Right hand from a caller's state, left from the generated start; NaN coordinates under every joint that is not selected."""
    w = odd_weights()
    rows = {}
    for h, with_init in (("r", True), ("l", False)):
        y3, init = _family_rows(Cs[h], WEIGHT_SEEDS, np.random.RandomState(1006), with_init)
        y3[~(w > 0)] = NAN
        rows[h] = (y3, init)
    K = general_K(len(WEIGHT_SEEDS))
    return [launch("weights3d", 3, [side(h, rows[h][0], w, rows[h][1]) for h in "rl"], F.config(iters=3)),
            launch("weights2d", 2, [side(h, project_rows(rows[h][0], K), w, rows[h][1]) for h in "rl"],
                   G.config(iters_rigid=2, iters=3), K)]


# ---- 7. the damping's ends ----------------------------------------------------------------------------------------------------------
def damping_launches(Cs):
    """mu0 = 0 (H is not damped, the first accepted step clamps mu to MU_MIN) and mu0 = 1e7 (above MU_MAX: the first rejection
    clamps it from above), default priors, the rows of the step-parity tests."""
    out = []
    for mu0 in (0.0, 1e7):
        s3, s2 = [], []
        for h, base, with_init in (("r", 100, True), ("l", 200, False)):
            y3, w, init = F.step_parity_inputs(Cs[h], base, with_init)
            s3.append(side(h, y3, w, init))
            y2, w2, init2 = G.step_parity_inputs(Cs[h], base, with_init)
            s2.append(side(h, y2, w2, init2))
        out.append(launch(f"damping3d.mu{mu0:g}", 3, s3, F.config(iters=3, mu0=mu0)))
        out.append(launch(f"damping2d.mu{mu0:g}", 2, s2, G.config(iters_rigid=2, iters=3, mu0=mu0), plain_K(5)))
    return out


# ---- the conditions the inputs must meet ---------------------------------------------------------------------------------------------
def floor(ref):
    return 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


def half_turn_branch(D):
    """The path of Log through a 3 x 3 matrix as DESIGN.md section 7 orders it: "general", "small", or ("half", k, flips) with
    k the sub-branch (the largest axis component, the lowest index on a tie) and flips the other two components' sign changes."""
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    c = 0.5 * (D[0, 0] + D[1, 1] + D[2, 2] - 1.0)
    if math.sqrt(float(v @ v)) >= 1e-9:
        return "general"
    if c >= 0.0:
        return "small"
    u = [math.sqrt(max(0.0, (D[i, i] - c) / (1.0 - c))) for i in range(3)]
    k = int(np.argmax(u))
    return ("half", k, tuple(bool(u[j] > 0.0 and D[j, k] + D[k, j] < 0.0) for j in range(3) if j != k))


def conditions(L, Cs, key):
    """Asserts what a launch's inputs are chosen for, on the restatement alone -> (refs, twins).  For every launch: no tie
    decides, and the twin takes the same steps; for a 3-D launch 16 x the twin's difference stays below the fp32 floor, so the
    floor alone is the bar (the 2-D comparison takes the larger of the two itself)."""
    refs, twins = reference(L, Cs, key)
    name = L["name"]
    rows = [r for rr in refs for r in rr]
    assert all(decided(r) for r in rows), name
    assert all(a["steps"] == b["steps"] and a.get("start") == b.get("start") for rr, tt in zip(refs, twins) for a, b in zip(rr, tt)), name
    if L["dim"] == 3:
        for rr, tt in zip(refs, twins):
            for k in ("pose", "beta", "transl", "rmse"):
                ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in rr])
                assert 16 * twin_gap(rr, tt, k) <= np.nanmin(floor(ref)), (name, k)
    fam = name.split(".")[0]
    if fam in ("pivot3d", "pivot2d"):
        rigid = L["cfg"].get("iters_rigid", 0)
        for r in rows:
            assert all(ok for _, _, ok, _ in r["trace"][:rigid]), name
            if name.endswith("zero"):                      # every full iteration fails to factorise, and only those
                assert [ok for _, _, ok, _ in r["trace"][rigid:]] == [False] * L["cfg"]["iters"], name
                assert r["steps"] == sum(acc for _, _, _, acc in r["trace"][:rigid]) and (rigid == 0 or r["steps"] > 0), name
            else:
                assert all(ok for _, _, ok, _ in r["trace"]), name
        if name == "pivot3d.live":
            assert all(r["steps"] >= 1 for r in rows)
        if name == "pivot2d.live":                         # the full stage moves too
            assert sum(acc for r in rows for _, _, _, acc in r["trace"][rigid:]) >= 6
        if name == "pivot3d.zero":                         # the columns are exactly zero at the state the fit starts from
            for s in L["sides"]:
                if s["init"] is not None:
                    for b in range(L["B"]):
                        R, beta = s["init"][0][b].astype(np.float64), s["init"][1][b].astype(np.float64)
                        Jm = F.jacobian(consts_of(Cs, s), R, beta, s["w"][b].astype(np.float64), L["cfg"])
                        for j in (3, 6, 9, 12, 15):
                            assert not Jm[:, 3 * j:3 * j + 3].any() and Jm[:, 3 * j - 3:3 * j].any()
    elif fam == "intrinsics":
        K = L["K"].astype(np.float64)
        assert np.isnan(K[:, 2]).all() and np.isfinite(K[:, :2]).all()
        assert (K[:, 0, 0] != K[:, 1, 1]).all() and (K[:, 0, 1] != 0).all() and (K[:, 1, 0] != 0).all()
        assert (K[:, 0, 1] != K[:, 1, 0]).all() and (K[:, 0, 2] != K[:, 1, 2]).all() and len({a.tobytes() for a in K}) == len(K)
        assert all(G.margins_ok(r) for r in rows), name
        assert all(r["start"] == -1 for r in refs[0]) and all(0 <= r["start"] < 24 for r in refs[1])
        if name.startswith("intrinsics.2+3"):
            assert sum(r["steps"] for r in rows) >= 25, name
    elif fam == "start":
        for rr, gaps in zip(refs, start_gaps(Cs, L)):
            assert [r["start"] for r in rr] == list(range(24)) and [c for c, _ in gaps] == list(range(24)), name
            assert min(g for _, g in gaps) >= 10.0, (name, min(g for _, g in gaps))
        if name == "start.weighted":
            w = L["sides"][0]["w"]
            assert ((w == 0).sum(1) == 3).all() and all(np.isnan(s["y"][w == 0]).all() for s in L["sides"])
    elif fam == "depth":
        (r,) = rows
        inf = [i for i, (_, c2, _, _) in enumerate(r["trace"]) if math.isinf(c2)]
        assert inf and all(c2 > 0 and not acc for _, c2, _, acc in (r["trace"][i] for i in inf)), name
        assert r["steps"] >= 3 and G.margins_ok(r), name
        assert np.asarray(r["raw"]["j3d"])[L["sides"][0]["w"][0] > 0, 2].min() > L["cfg"]["z_min"]
    elif fam in ("halfturn3d", "halfturn2d"):
        seen = set()
        for s in L["sides"]:
            pose = s["init"][0]
            assert pose.dtype == np.float32
            for b in range(L["B"]):
                for j in range(1, 16):
                    seen.add(half_turn_branch(pose[b, j].astype(np.float64)))          # Mref_j = I: D = R_j
            assert (consts_of(Cs, s).M == np.eye(3)).all()
        want = {"small"} | {("half", k, (a, b)) for k in range(3) for a in (False, True) for b in (False, True)}
        assert seen == want, (name, want - seen, seen - want)
        for T in HALF_TURNS:
            assert np.array_equal(T @ T.T, np.eye(3)) and set(np.unique(T)) <= {-1.0, 0.0, 1.0}
        for T in OBLIQUE_TURNS:
            assert np.array_equal(T, T.T) and np.array_equal(T, T.astype(np.float32).astype(np.float64))
        if fam == "halfturn3d":
            assert all(r["steps"] == L["cfg"]["iters"] for r in rows), name
        elif L["cfg"]["iters"]:
            assert all(r["steps"] >= 1 for r in rows) and sum(r["steps"] for r in rows) >= 9, name
    elif fam in ("weights3d", "weights2d"):
        for rr in refs:
            assert [bool(np.isfinite(r["rmse"])) for r in rr] == list(WEIGHT_FITTED), name
            assert all(r["steps"] >= 2 for r, f in zip(rr, WEIGHT_FITTED) if f), name
        w = L["sides"][0]["w"]
        assert [int((w[b] > 0).sum()) for b in (1, 2, 4)] == [4, 3, 4] and 0 < w[4, 18] < np.finfo(np.float32).tiny
        assert np.isposinf(w[5]).sum() == 1 and np.isfinite(np.delete(w[5], 7)).all() and all(np.isfinite(s["y"][5]).all() for s in L["sides"])
        assert np.isnan(w[0]).sum() == 3 and np.signbit(w[0, 12]) and w[0, 12] == 0 and all(np.isnan(s["y"][~(w > 0)]).all() for s in L["sides"])
    elif fam in ("damping3d", "damping2d"):
        if fam == "damping3d":
            assert all(r["steps"] == 3 for r in (rows if L["cfg"]["mu0"] > 0 else refs[0][2:])), name
        else:
            assert all(r["steps"] >= 2 for r in rows), name
        assert L["cfg"]["mu0"] == 0.0 or L["cfg"]["mu0"] > F.MU_MAX
    else:
        raise AssertionError(name)
    return refs, twins


def all_launches(Cs):
    return (pivot_launches(Cs) + intrinsics_launches(Cs) + start_launches(Cs) + depth_launches(Cs) + half_turn_launches(Cs) +
            weight_launches(Cs) + damping_launches(Cs))
