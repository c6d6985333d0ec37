"""Inputs for the edge and branch tests of the vertex fit of csrc/fit_verts.hip (tests/test_fit_verts_edges.py on the CPU,
tests/test_gpu_fit_verts_edges.py on the device): small deterministic launches that reach what the family cases of
tests/test_gpu_fit_verts.py do not -- a pivot that is exactly zero, the Kabsch start on a mirrored, a planar, a far and the rest
hand's own target, the geometry of the four-round selection count, weights that are no number, negative, -0.0, denormal or +inf,
both ends of the damping and a fit without priors, half turns in the pose prior, the five tips under weight 0, and a last
iteration that was rejected.  Pure numpy on top of the restatement tests/fit_verts_ref.py, in the shape of tests/fit_edge_cases.py.

A *launch* is a dict: ``name``, ``cfg``, ``B`` and ``sides``, a list of dict(h = "r" / "l", y, w, valid, init, mod).  ``mod`` names
the modified pack the side runs on: None, "flat" (pose_mean = 0, so that M_j = I exactly) or ("dead", l) (shapedirs[:, :, l] = 0 and
J_shapedirs[:, :, l] = 0: shape column l of the Jacobian is exactly zero).  ``modified`` makes the matching constants; a test on the
device hands in the constants it read back from its modified pack under the key (h, mod) instead.  No launch has more than 8 hands;
the rejection family has at most 6 iterations, every other one at most 4.
"""
import numpy as np

import fit_edge_cases as X
import fit_verts_ref as V

NV = V.NV
NAN = float("nan")
FLOATS = ("pose", "beta", "transl", "rmse", "j3d")
TIP_VERTS = (744, 320, 443, 554, 671)
DENORMAL = X.DENORMAL                             # positive and below the smallest normal fp32
MAX_B, MAX_ITERS, MAX_ITERS_REJECTED = 8, 4, 6


def bar(ref):
    return 4 * 2.0 ** -24 * np.maximum(1.0, np.abs(ref))


def modified(C, mod):
    """The constants of the pack ``mod`` names, from those of the plain pack."""
    if mod is None:
        return C
    if mod == "flat":
        return V.Consts(np.zeros(48), C.J_template, C.J_shapedirs, C.v_template, C.shapedirs, C.lbs_weights, C.posedirs)
    kind, l = mod
    assert kind == "dead"
    sd, Js = C.shapedirs.copy(), C.J_shapedirs.copy()
    sd[:, :, l], Js[:, :, l] = 0.0, 0.0
    return V.Consts(C.pose_mean, C.J_template, Js, C.v_template, sd, C.lbs_weights, C.posedirs)


def consts_of(Cs, s):
    """Cs: {"r": Consts, "l": Consts}, and optionally {(h, mod): Consts} read back from a modified pack."""
    key = (s["h"], s["mod"])
    return Cs[key] if key in Cs else modified(Cs[s["h"]], s["mod"])


def side(h, y, w=None, init=None, valid=None, mod=None):
    return {"h": h, "y": y, "w": w, "init": init, "valid": valid, "mod": mod}


def launch(name, sides, cfg):
    return {"name": name, "sides": sides, "cfg": cfg, "B": len(sides[0]["y"])}


def family_rows(C, seeds, rng_seed, with_init, keep=None):
    """Family cases: y (B,778,3) fp32, w (B,778) fp32 (``keep``: that many vertices at weight 1, NaN under the others) and a
    caller's state near the truth in fp32, or None."""
    rng = np.random.RandomState(rng_seed)
    ys, ws, init = [], [], ([], [], [])
    for s in seeds:
        y, w, truth = V.family_case(C, s, keep=keep)
        y = y.copy()
        y[w == 0] = NAN
        ys.append(y)
        ws.append(w)
        for a, v in zip(init, V.near(truth, rng)):
            a.append(v)
    return np.stack(ys), np.stack(ws), (tuple(np.stack(a).astype(np.float32) for a in init) if with_init else None)


def only(y_full, idx):
    """Weight 1 on the vertices ``idx`` alone, NaN coordinates everywhere else."""
    w, y = np.zeros(NV, np.float32), np.full((NV, 3), NAN, np.float32)
    w[list(idx)] = 1.0
    y[list(idx)] = y_full[list(idx)]
    return y, w


_REF = {}


def reference(L, Cs, key):
    """-> (refs, twins): per side the restatement's results per row and those of its noise = 1e-15 twin.  ``key`` names the set
    of constants; computed once per (key, launch)."""
    k = (key, L["name"])
    if k not in _REF:
        refs, twins = [], []
        for s in L["sides"]:
            C = consts_of(Cs, s)
            refs.append(V.fit_rows(C, s["y"], s["w"], s["valid"], s["init"], L["cfg"]))
            twins.append(V.fit_rows(C, s["y"], s["w"], s["valid"], s["init"], L["cfg"], noise=1e-15, seed=5))
        _REF[k] = (refs, twins)
    return _REF[k]


def margins(res):
    """|c' - c| / c of every decision of a result that the cost decides (a failed factorisation decides by itself)."""
    return [abs(c2 - c) / c for c, c2, ok, _ in res["trace"] if ok]


def kabsch_singular_values(C, y, w):
    """The singular values, descending, of the cross-covariance the restatement's Kabsch start decomposes."""
    w = np.ones(NV) if w is None else np.asarray(w, np.float32).astype(np.float64)
    sel = w > 0
    X0 = V.vertices_of(C, V.rest_pose(C), np.zeros(10))[sel]
    Y, ws = np.asarray(y, np.float32).astype(np.float64)[sel], w[sel]
    mx, my = (ws[:, None] * X0).sum(0) / ws.sum(), (ws[:, None] * Y).sum(0) / ws.sum()
    return np.linalg.svd(np.einsum("k,ka,kb->ab", ws, X0 - mx, Y - my), compute_uv=False)


# ---- 1. a pivot that is exactly zero ---------------------------------------------------------------------------------------------
PIVOT_SEEDS = (4, 5, 6)
DEAD = {"r": 0, "l": 9}                           # the dead shape column per side: two different lanes own it


def pivot_launches(Cs):
    """lambda_beta = 0 on a pack whose shape column l is zero: column 48 + l of the Jacobian is exactly zero, the pivot 0.0 on the
    host and on the device alike, and every iteration is a rejected step -- the kernel factorises on with the pivot replaced by 1
    and evaluates a finite candidate.  The same rows at iters = 0, and at lambda_beta = 1e-6, where they take steps.  The right
    hand from a caller's state, the left from the Kabsch start."""
    sides = []
    for h, with_init in (("r", True), ("l", False)):
        mod = ("dead", DEAD[h])
        y, w, init = family_rows(modified(Cs[h], mod), PIVOT_SEEDS, 2004, with_init)
        sides.append(side(h, y, w, init, mod=mod))
    return [launch("pivot.zero", sides, V.config(iters=3, lambda_beta=0.0)),
            launch("pivot.zero.iters0", sides, V.config(iters=0, lambda_beta=0.0)),
            launch("pivot.live", sides, V.config(iters=3, lambda_beta=1e-6))]


# ---- 2. the Kabsch start away from a rotated hand ----------------------------------------------------------------------------------
KABSCH_SEEDS = {"r": (31, 32, 33), "l": (41, 42, 43)}
KABSCH_ROWS = ("mirrored", "planar", "far", "rest")
FAR = np.array([30.0, -20.0, 50.0])


def kabsch_rows(C, seeds):
    """(4,778,3) fp32: a family case mirrored in x; one flattened onto the plane z = 0.5; one moved by FAR before the rounding to
    fp32; the rest hand's own vertices."""
    mirrored = V.family_case(C, seeds[0])[0].copy()
    mirrored[:, 0] = -mirrored[:, 0]
    planar = V.family_case(C, seeds[1])[0].copy()
    planar[:, 2] = np.float32(0.5)
    R, beta, t = V.family_case(C, seeds[2])[2]
    far = (V.vertices_of(C, R, beta) + t + FAR).astype(np.float32)
    rest = V.vertices_of(C, V.rest_pose(C), np.zeros(10)).astype(np.float32)
    return np.stack([mirrored, planar, far, rest])


def kabsch_launches(Cs):
    """All four rows at iters = 0; the first three at iters = 3.  The rest row starts converged -- its cost, 8e-15, is the rounding
    of y to fp32 alone --: its first decision has a margin of 2.3e-2 c, the second 4.8e-6 c, and the third is a tie (4.2e-10 c on
    the right asset), which DESIGN.md section 7 leaves untested by design.  So that row runs at iters = 1 in a launch of its own."""
    rows = {h: kabsch_rows(Cs[h], KABSCH_SEEDS[h]) for h in "rl"}
    return [launch("kabsch.0", [side(h, rows[h]) for h in "rl"], V.config(iters=0)),
            launch("kabsch.3", [side(h, rows[h][:3]) for h in "rl"], V.config(iters=3)),
            launch("kabsch.rest.1", [side(h, rows[h][3:]) for h in "rl"], V.config(iters=1))]


# ---- 3. the geometry of the selection -----------------------------------------------------------------------------------------------
SELECTIONS = ((0, 256, 512, 768),                 # one vertex per round of the four-round count
              (774, 775, 776, 777),               # all four in the tail tile, beside the absent vertices
              tuple(range(768, 778)),             # the tail tile alone
              tuple(range(0, NV, 16)),            # one vertex slot of every tile
              tuple(range(112, 128)),             # one tile
              (0, 256, 512), (775, 776, 777))     # three vertices: not fitted
SELECTION_FITTED = (True, True, True, True, True, False, False)
SELECTION_SEEDS = {"r": 50, "l": 60}


def selection_launches(Cs):
    sides = []
    for h, with_init in (("r", True), ("l", False)):
        seeds = [SELECTION_SEEDS[h] + b for b in range(len(SELECTIONS))]
        y_full, _, init = family_rows(Cs[h], seeds, 2006, with_init)
        yw = [only(y_full[b], idx) for b, idx in enumerate(SELECTIONS)]
        sides.append(side(h, np.stack([a for a, _ in yw]), np.stack([b for _, b in yw]), init))
    return [launch("selection", sides, V.config(iters=4))]


# ---- 4. weights that select nothing, a denormal and +inf ----------------------------------------------------------------------------
WEIGHT_SEEDS = {"r": (70, 71, 72, 73), "l": (80, 81, 82, 83)}
WEIGHT_FITTED = (True, True, False, False)
WEIGHT_FOUR = (5, 300, 520, 700)
INF_AT = 401


def odd_weights():
    """(4,778) fp32.  Row 0: 2 on every tenth vertex, NaN, -1, -inf, -0.0 and a denormal interleaved over the others; row 1: four
    vertices at 1 among NaN; row 2: three of them (not fitted); row 3: ones and one +inf (not fitted)."""
    w = np.ones((4, NV), np.float32)
    w[0] = np.array([NAN, -1.0, -np.inf, -0.0, DENORMAL], np.float32)[np.arange(NV) % 5]
    w[0, ::10] = 2.0
    w[1] = NAN
    w[1, list(WEIGHT_FOUR)] = 1.0
    w[2] = NAN
    w[2, list(WEIGHT_FOUR[:3])] = 1.0
    w[3, INF_AT] = np.inf
    return w


def weight_launches(Cs):
    """NaN coordinates under every weight that does not select.  The right hand from a caller's state, the left from Kabsch."""
    w = odd_weights()
    sides = []
    for h, with_init in (("r", True), ("l", False)):
        y, _, init = family_rows(Cs[h], WEIGHT_SEEDS[h], 2007, with_init)
        y[~(w > 0)] = NAN
        sides.append(side(h, y, w, init))
    return [launch("weights", sides, V.config(iters=3))]


# ---- 5. the damping's ends, and no priors -------------------------------------------------------------------------------------------
DAMPING_SEEDS = {"r": (90, 91), "l": (95, 96)}


def damping_launches(Cs):
    """mu0 = 0 (H is not damped; the first accepted step clamps mu to MU_MIN), mu0 = 1e7 (above MU_MAX: the first rejection clamps
    it from above) and lambda_beta = lambda_pose = 0 at the default mu0; fully weighted."""
    sides = []
    for h, with_init in (("r", True), ("l", False)):
        y, w, init = family_rows(Cs[h], DAMPING_SEEDS[h], 2008, with_init)
        sides.append(side(h, y, w, init))
    return [launch("damping.mu0", sides, V.config(iters=4, mu0=0.0)), launch("damping.mu1e7", sides, V.config(iters=4, mu0=1e7)),
            launch("damping.nopriors", sides, V.config(iters=4, lambda_beta=0.0, lambda_pose=0.0))]


# ---- 6. half turns in the pose prior ------------------------------------------------------------------------------------------------
def half_turn_rows(C):
    """C: flat constants.  Family cases (4,778,3) and a caller's state whose finger rotations are exact half turns on seven joints
    per row (fit_edge_cases.HALF_TURNS in rotating order, row 3: OBLIQUE_TURNS, over HALF_TURN_JOINTS) and the identity on the
    other eight: Log(M_j^T R_j) takes its third branch, and R_j - I has entries of -2 for the pose blend shapes."""
    y, w, near = family_rows(C, X.HALF_TURN_SEEDS, 2005, True)
    pose = near[0].copy()
    pose[:, 1:] = np.eye(3, dtype=np.float32)
    for b, joints in enumerate(X.HALF_TURN_JOINTS):
        turns = X.OBLIQUE_TURNS if b == 3 else X.HALF_TURNS[b:] + X.HALF_TURNS[:b]
        for j, T in zip(joints, turns):
            pose[b, j] = T.astype(np.float32)
    return y, (pose, near[1], near[2])


def half_turn_launches(Cs):
    rows = {h: half_turn_rows(modified(Cs[h], "flat")) for h in "rl"}
    sides = [side(h, rows[h][0], None, rows[h][1], mod="flat") for h in "rl"]
    return [launch(f"halfturn.{lp:g}.{iters}", sides, V.config(iters=iters, lambda_pose=lp)) for lp in (1e-6, 1e-2) for iters in (0, 1, 3)]


# ---- 7. the five tips under weight 0 ------------------------------------------------------------------------------------------------
TIP_SEEDS = {"r": (110, 111), "l": (120, 121)}


def tip_launches(Cs):
    """Row 0: weight 0 and NaN targets on the five tip vertices, weight 1 elsewhere -- j3d rows 16..20 come out of the walk all
    the same.  Row 1: weight 1 on the five tips and on 20 random other vertices only."""
    sides = []
    for h, with_init in (("r", True), ("l", False)):
        y, w, init = family_rows(Cs[h], TIP_SEEDS[h], 2009, with_init)
        w[0, list(TIP_VERTS)] = 0.0
        others = np.setdiff1d(np.arange(NV), TIP_VERTS)
        w[1] = 0.0
        w[1, list(TIP_VERTS)] = 1.0
        w[1, np.random.RandomState(2010).choice(others, 20, replace=False)] = 1.0
        y[w == 0] = NAN
        sides.append(side(h, y, w, init))
    return [launch("tips", sides, V.config(iters=4))]


# ---- 8. a last iteration that was rejected ------------------------------------------------------------------------------------------
REJECTED_SEED = 0
REJECTED_AT = (0, 3, 5)                           # the decisions of the restatement that are clear rejections (right asset, Kabsch)


def rejected_launches(Cs):
    """family_case(keep=20) of the right asset from the Kabsch start, at iters = k and k + 1 for every k of REJECTED_AT: decision
    k is rejected, so the two launches return the same state -- the second one only after evaluating the current state again."""
    y, w, _ = family_rows(Cs["r"], (REJECTED_SEED,), 2011, False, keep=20)
    iters = sorted({k + d for k in REJECTED_AT for d in (0, 1)})
    return [launch(f"rejected.{i}", [side("r", y, w)], V.config(iters=i)) for i in iters]


FAMILIES = {"pivot": pivot_launches, "kabsch": kabsch_launches, "selection": selection_launches, "weights": weight_launches,
            "damping": damping_launches, "halfturn": half_turn_launches, "tips": tip_launches, "rejected": rejected_launches}


# ---- the conditions the inputs must meet --------------------------------------------------------------------------------------------
def conditions(L, Cs, key):
    """Asserts what a launch's inputs are chosen for, on the restatement alone -> (refs, twins).  For every launch: no tie
    decides (|c' - c| > 1e-9 c unless a failed factorisation decides), the twin takes the same steps, and 16 x the twin's
    difference is at most the bar 4 * 2^-24 * max(1, |ref|) at every element of every float output, so that the bar alone is the
    bound on the device."""
    refs, twins = reference(L, Cs, key)
    name, cfg = L["name"], L["cfg"]
    fam = name.split(".")[0]
    assert L["B"] <= MAX_B and cfg["iters"] <= (MAX_ITERS_REJECTED if fam == "rejected" else MAX_ITERS), name
    rows = [r for rr in refs for r in rr]
    assert all(m > 1e-9 for r in rows for m in margins(r)), (name, min(m for r in rows for m in margins(r)))
    for rr, tt in zip(refs, twins):
        assert all(a["steps"] == b["steps"] and [x[2:] for x in a["trace"]] == [x[2:] for x in b["trace"]] for a, b in zip(rr, tt)), name
        for k in FLOATS:
            ref = np.stack([np.asarray(r["raw"][k], np.float64) for r in rr])
            twin = np.stack([np.asarray(r["raw"][k], np.float64) for r in tt])
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(twin), nan), (name, k)
            gap = np.where(nan, 0.0, np.abs(np.where(nan, 0.0, ref) - np.where(nan, 0.0, twin)))
            assert (16 * gap <= bar(np.where(nan, 0.0, ref))).all(), (name, k, float(gap.max()))
    fitted = lambda rr: [bool(np.isfinite(r["rmse"])) for r in rr]
    for s, rr in zip(L["sides"], refs):
        assert s["y"].dtype == np.float32 and (s["w"] is None or s["w"].dtype == np.float32)
        if s["w"] is not None:                             # NaN under every weight that does not select
            assert np.isnan(s["y"][~(s["w"] > 0)]).all(), name
    if fam == "pivot":
        for s, rr in zip(L["sides"], refs):
            l = s["mod"][1]
            C = consts_of(Cs, s)
            assert not C.shapedirs[:, :, l].any() and not C.J_shapedirs[:, :, l].any() and C.shapedirs.any(), name
            for r in rr:
                if name == "pivot.live":                   # every decision is an accepted step
                    assert [x[2:] for x in r["trace"]] == [(True, True)] * cfg["iters"] and r["steps"] == cfg["iters"], name
                else:                                      # (c, nan, False, False), the same c every time
                    assert all(np.isnan(c2) and not ok and not acc for _, c2, ok, acc in r["trace"]) and r["steps"] == 0, name
                    assert len({c for c, _, _, _ in r["trace"]}) <= 1 and len(r["trace"]) == cfg["iters"], name
        assert DEAD["r"] != DEAD["l"] and [s["init"] is None for s in L["sides"]] == [False, True]
    elif fam == "kabsch":
        for s, rr in zip(L["sides"], refs):
            assert s["init"] is None and s["w"] is None and all(fitted(rr)), name
            C = consts_of(Cs, s)
            names = {"kabsch.0": KABSCH_ROWS, "kabsch.3": KABSCH_ROWS[:3], "kabsch.rest.1": KABSCH_ROWS[3:]}[name]
            assert len(names) == L["B"], name
            for b, row in enumerate(names):
                sv = kabsch_singular_values(C, s["y"][b], None)
                assert sv[1] > 1e-3 * sv[0], (name, row, sv)
                R0 = rr[b]["raw"]["pose"][0] if cfg["iters"] == 0 else None
                if row == "mirrored":                      # otherwise the proper rotation is not unique
                    assert sv[1] - sv[2] > 1e-3 * sv[0], (name, row, sv)
                if row == "planar":
                    assert sv[2] <= 1e-12 * sv[0] and np.ptp(s["y"][b][:, 2]) == 0, (name, row, sv)
                if row == "far":
                    assert np.abs(s["y"][b].mean(0)).min() > 15.0
                if row == "rest" and R0 is not None:               # the identity, within what the rounding of y to fp32 turns it
                    assert np.abs(R0 - np.eye(3)).max() <= 1e-6, name
                if R0 is not None:
                    assert abs(np.linalg.det(R0) - 1.0) <= 1e-12 and np.abs(R0.T @ R0 - np.eye(3)).max() <= 1e-12, (name, row)
            if cfg["iters"]:
                assert all(r["steps"] >= 1 for r in rr), name
    elif fam == "selection":
        for s, rr in zip(L["sides"], refs):
            assert [tuple(np.flatnonzero(w > 0)) for w in s["w"]] == [tuple(i) for i in SELECTIONS], name
            assert fitted(rr) == list(SELECTION_FITTED), name
            assert all(r["steps"] >= 1 for r, f in zip(rr, SELECTION_FITTED) if f) and all(r["steps"] == 0 for r, f in zip(rr, SELECTION_FITTED) if not f)
        assert [n // 256 for n in SELECTIONS[0]] == [0, 1, 2, 3] and min(SELECTIONS[1]) // 16 == 48 and NV - 1 in SELECTIONS[1]
        assert {n % 16 for n in SELECTIONS[3]} == {0} and {n // 16 for n in SELECTIONS[4]} == {7} and len(SELECTIONS[4]) == 16
    elif fam == "weights":
        w = L["sides"][0]["w"]
        tiny = np.finfo(np.float32).tiny
        assert all(np.array_equal(s["w"].view(np.int32), w.view(np.int32)) for s in L["sides"])
        for rr in refs:
            assert fitted(rr) == list(WEIGHT_FITTED) and all(r["steps"] >= 1 for r, f in zip(rr, WEIGHT_FITTED) if f), name
        assert np.isnan(w[0]).any() and (w[0] == -1).any() and np.isneginf(w[0]).any() and (np.signbit(w[0]) & (w[0] == 0)).any()
        assert ((w[0] > 0) & (w[0] < tiny)).any() and (w[0] == 2).sum() == 78
        assert [int((x > 0).sum()) for x in w[1:3]] == [4, 3] and np.isnan(w[1]).sum() == NV - 4 and np.isnan(w[2]).sum() == NV - 3
        assert np.isposinf(w[3]).sum() == 1 and np.isfinite(np.delete(w[3], INF_AT)).all() and all(np.isfinite(s["y"][3]).all() for s in L["sides"])
        for b in range(4):                                 # no row is selected by denormals alone
            assert not (w[b] > 0).any() or (w[b] >= tiny).any()
    elif fam == "damping":
        assert all((s["w"] == 1).all() for s in L["sides"]) and all(r["steps"] >= 2 for r in rows), name
        assert {"damping.mu0": cfg["mu0"] == 0.0, "damping.mu1e7": cfg["mu0"] > V.MU_MAX,
                "damping.nopriors": cfg["lambda_beta"] == 0.0 and cfg["lambda_pose"] == 0.0 and cfg["mu0"] == V.config()["mu0"]}[name]
    elif fam == "halfturn":
        seen, tied = set(), 0
        for s in L["sides"]:
            pose = s["init"][0]
            assert pose.dtype == np.float32 and s["mod"] == "flat" and (consts_of(Cs, s).M == np.eye(3)).all()
            for b in range(L["B"]):
                for j in range(1, 16):
                    D = pose[b, j].astype(np.float64)                                  # M_j = I: M_j^T R_j = R_j
                    seen.add(X.half_turn_branch(D))
                    u = sorted(np.diag(D))                                             # the axis components grow with the diagonal
                    tied += X.half_turn_branch(D) != "small" and u[2] == u[1]
            assert (pose[:3, 1:] - np.eye(3, dtype=np.float32)).min(axis=(1, 2, 3)).tolist() == [-2.0] * 3     # the axis turns
        want = {"small"} | {("half", k, (a, b)) for k in range(3) for a in (False, True) for b in (False, True)}
        assert seen == want, (name, want - seen, seen - want)
        assert tied >= 4 and cfg["lambda_pose"] in (1e-6, 1e-2), (name, tied)           # a >= tie of the two largest components
        if cfg["iters"]:
            assert all(r["steps"] >= 1 for r in rows), name
    elif fam == "tips":
        for s, rr in zip(L["sides"], refs):
            w = s["w"]
            assert not w[0, list(TIP_VERTS)].any() and (np.delete(w[0], TIP_VERTS) == 1).all()
            assert (w[1, list(TIP_VERTS)] == 1).all() and (w[1] > 0).sum() == 25
            assert all(fitted(rr)) and all(np.isfinite(r["raw"]["j3d"]).all() and r["steps"] >= 1 for r in rr), name
        assert TIP_VERTS == tuple(V.TIP_IDS)
    elif fam == "rejected":
        (r,) = rows
        for k in REJECTED_AT:                              # a clear rejection with a factorisation that succeeded
            if cfg["iters"] > k:
                c, c2, ok, acc = r["trace"][k]
                assert ok and not acc and c2 - c > 1e-9 * c, (name, k)
        assert 0 in REJECTED_AT and len(REJECTED_AT) >= 2 and int((L["sides"][0]["w"] > 0).sum()) == 20
    else:
        raise AssertionError(name)
    return refs, twins


def all_launches(Cs):
    return [L for f in FAMILIES.values() for L in f(Cs)]
