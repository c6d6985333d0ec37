"""hands_mesh_correspond_f32 (csrc/mesh_correspond.hip), hands_amd.correspond_on_mesh and the ICP loop on it (register_mano,
register_mano_hands, register_predictions) on the device against the fp64 restatement (tests/fit_surf_ref.py) of DESIGN.md
section 7 "MANO fitting to surface correspondences and ICP registration".

Bars.  Correspondences: those of tests/test_gpu_surface_metrics.py for the same quantities -- every coordinate within 0.6 m,
|d - d_fp64| <= 5e-7 m, | |p - c| - d | <= 5e-7 m and c within 5e-7 m of the reported face; ``face_idx`` is compared only where
the restatement's runner-up face is farther by more than 1e-6 m (twice the bar; closer than that fp32 and fp64 may choose
differently); sum_i b_i v_i is within 5e-7 m of ``closest``.  One round: the fit's bar of tests/test_gpu_fit_surf.py.  The loop:
the restatement on registration_case(seeds 20, 21; P = 128), 6 rounds of 3 iterations at tangent_weight 0.1, takes the rms
cloud-to-surface distance from 3.38 / 3.36 mm to 0.702 / 0.318 mm (measured; DESIGN.md records it); the device's loop is held
to 4 x the larger and to ending below its start.
"""
import numpy as np
import pytest
import torch

import fit_surf_ref as S
import fit_verts_ref as V
import surface_ref as SR
from surface_asset import tube_hand_asset
from test_gpu_fit_surf import bar, bits

pytestmark = pytest.mark.gpu

BAR = 5e-7
LOOP_END_MAX = 4 * 0.702e-3
CENTRE = np.array([0.02, -0.03, 0.25])


def _cuda(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


@pytest.fixture(scope="module")
def assets():
    """name -> (MANOHead, packed constants on the device, the restatement's constants read back, faces (1538,3))."""
    from hands_amd.mano import synthetic_mano_asset
    from hands_amd.mano_head import MANOHead
    from hands_amd.packing import pack_mano
    out = {}
    for name, a in (("soup", synthetic_mano_asset(True)), ("tube", tube_hand_asset(True)), ("soup_l", synthetic_mano_asset(False))):
        pack = pack_mano(a, torch.device("cuda"))
        out[name] = (MANOHead(a.is_rhand, 1000.0, 224, asset=a), pack, V.consts_from_pack(pack), np.asarray(a.faces))
    return out


def posed(C, seed):
    _, _, (R, beta, _) = V.family_case(C, seed)
    return (V.vertices_of(C, R, beta) + CENTRE).astype(np.float32)


# ---- 1. the correspondences --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 33])
@pytest.mark.parametrize("name", ["soup", "tube"])
def test_correspondences_match_the_restatement(assets, name, P):
    import hands_amd
    _, _, C, faces = assets[name]
    B = 2
    rng = np.random.RandomState(50 + P)
    verts = np.stack([posed(C, 60 + b) for b in range(B)])
    pts = np.stack([verts[b][rng.randint(0, 778, P)] + 0.006 * rng.randn(P, 3) for b in range(B)]).astype(np.float32)
    assert max(np.abs(verts).max(), np.abs(pts).max()) <= 0.6
    w = rng.uniform(0.5, 2.0, (B, P)).astype(np.float32)
    if P > 1:
        w[0, 3], pts[0, 3] = 0.0, np.nan                               # a query of weight 0 is not read
        w[1, 5] = 0.0
    md = 0.006
    out = hands_amd.correspond_on_mesh(_cuda(pts), _cuda(verts), torch.from_numpy(faces), _cuda(w), max_dist=md)
    assert list(out) == ["dist", "face_idx", "closest", "bary", "normal", "weights"] and out["face_idx"].dtype == torch.int32
    got = {k: v.cpu().numpy() for k, v in out.items()}
    worst = [0.0] * 5
    for b in range(B):
        ref = S.correspond(pts[b], verts[b], faces, w[b], md)
        read = w[b] > 0
        assert np.array_equal(got["face_idx"][b] >= 0, read) and np.array_equal(ref["face_idx"] >= 0, read)
        for k in ("dist", "closest", "bary"):
            assert np.isnan(got[k][b][~read]).all(), k
        assert (got["normal"][b][~read] == 0).all() and (got["weights"][b][~read] == 0).all()
        p, v64 = pts[b][read].astype(np.float64), verts[b].astype(np.float64)
        d, c, f = got["dist"][b][read].astype(np.float64), got["closest"][b][read].astype(np.float64), got["face_idx"][b][read]
        back = np.einsum("ki,kic->kc", got["bary"][b][read].astype(np.float64), v64[faces[f]])
        errs = (np.abs(d - ref["dist"][read]), SR.distance_to_face(p, v64, faces, f) - ref["dist"][read],
                np.abs(np.sqrt(((p - c) ** 2).sum(-1)) - d), SR.distance_to_face(c, v64, faces, f), np.abs(back - c).max(-1))
        worst = [max(a, float(e.max())) for a, e in zip(worst, errs)]
        far = S.runner_up(p, v64, faces, ref["face_idx"][read]) - ref["dist"][read] > 2 * BAR
        same = (faces[f] == faces[ref["face_idx"][read]]).all(1)       # a padded list repeats faces: the triangle counts
        assert same[far].all(), (b, np.flatnonzero(far & ~same))
        n, nr = got["normal"][b][read], ref["normal"][read]
        unit = np.linalg.norm(n, axis=1)
        assert (np.abs(unit[unit > 0] - 1) <= 1e-6).all()
        assert np.array_equal((unit == 0)[same], (np.linalg.norm(nr, axis=1) == 0)[same])
        T = v64[faces[f]]
        ab, ac = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
        sin2 = (np.cross(ab, ac) ** 2).sum(1) / np.maximum((ab ** 2).sum(1) * (ac ** 2).sum(1), 1e-300)
        fat = same & (sin2 > 1.0 / 64)                                 # fp32 normals of fat faces: 1e-4 is 30 x their rounding
        assert np.abs(n[fat] - nr[fat]).max(initial=0.0) <= 1e-4
        # the gate: the weight where the distance is inside, 0 outside; a distance within the bar of max_dist may go either way
        gate = got["weights"][b][read]
        clear_in, clear_out = ref["dist"][read] < md - BAR, ref["dist"][read] > md + BAR
        assert np.array_equal(gate[clear_in], w[b][read][clear_in]) and (gate[clear_out] == 0).all()
        assert np.array_equal(gate > 0, got["dist"][b][read] <= np.float32(md))
    print(f"REG|correspond|{name}|P {P}|d {worst[0]:.2e}|face excess {worst[1]:.2e}|p-c {worst[2]:.2e}|c to face {worst[3]:.2e}|"
          f"sum b v {worst[4]:.2e}|{BAR:.0e}")
    assert max(worst) <= BAR
    # the first three outputs are closest_on_mesh's bits on the same inputs (where the query is read); max_dist <= 0: no gate
    wq = torch.ones(B, P).cuda()
    pts_ok = np.nan_to_num(pts, nan=0.1)
    full = hands_amd.correspond_on_mesh(_cuda(pts_ok), _cuda(verts), torch.from_numpy(faces), wq)
    none = hands_amd.correspond_on_mesh(_cuda(pts_ok), _cuda(verts), torch.from_numpy(faces))
    d0, i0, c0 = hands_amd.closest_on_mesh(_cuda(pts_ok), _cuda(verts), torch.from_numpy(faces), return_points=True)
    assert torch.equal(full["dist"].view(torch.int32), d0.view(torch.int32)) and torch.equal(full["face_idx"].long(), i0)
    assert torch.equal(full["closest"].view(torch.int32), c0.view(torch.int32)) and torch.equal(full["weights"], wq)
    assert all(torch.equal(full[k].view(torch.int32), none[k].view(torch.int32)) for k in full)


def test_correspond_rejects_bad_calls(assets):
    from hands_amd import _lib
    from hands_amd._lib import ptr
    from edge_util import EINVAL, SENT
    L = _lib.lib()
    x = torch.zeros(64, device="cuda")
    fi = torch.zeros(12, dtype=torch.int32, device="cuda")
    o = [torch.full((64,), SENT, device="cuda") for _ in range(5)]
    oi = torch.full((16,), -77777, dtype=torch.int32, device="cuda")

    def call(drop=None, B=1, P=4, Vn=8, F=4, md=0.0):
        a = [ptr(x), ptr(x), ptr(fi), None, None, md, ptr(o[0]), ptr(oi), ptr(o[1]), ptr(o[2]), ptr(o[3]), ptr(o[4])]
        if drop is not None:
            a[drop] = None
        return L.hands_mesh_correspond_f32(*a, B, P, Vn, F, torch.cuda.current_stream().cuda_stream)

    for drop in (0, 1, 2, 6, 7, 8, 9, 10, 11):
        assert call(drop) == EINVAL, drop
    for kw in (dict(B=0), dict(P=0), dict(Vn=0), dict(F=-1), dict(Vn=1025), dict(F=4097), dict(md=float("nan"))):
        assert call(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert all(bool((t == SENT).all()) for t in o) and bool((oi == -77777).all())
    assert call() == 0 and call(2, F=0) == 0
    torch.cuda.synchronize()


# ---- 2. one round ------------------------------------------------------------------------------------------------------------
def test_one_round_is_the_restated_fit_on_the_kernels_correspondences(assets):
    import hands_amd
    head, pack, C, faces = assets["tube"]
    B, P = 2, 33
    cases = [S.registration_case(C, faces, 40 + b, P) for b in range(B)]
    pts = np.stack([c[0] for c in cases])
    init = tuple(np.stack([c[1][i] for c in cases]) for i in range(3))
    w = np.random.RandomState(3).uniform(0.5, 2.0, (B, P)).astype(np.float32)
    w[1, 7], pts[1, 7] = 0.0, np.nan
    cfg = hands_amd.RegisterConfig(rounds=1, iters=3, tangent_weight=0.1)
    tinit = tuple(_cuda(a) for a in init)
    out = hands_amd.register_mano(_cuda(pts), head, "r", init=tinit, weights=_cuda(w), config=cfg)
    assert list(out) == ["pose", "beta", "transl", "rmse", "steps", "j3d", "verts", "pose_aa", "dist", "rounds_done"]
    assert out["rounds_done"].dtype == torch.int32 and out["rounds_done"].tolist() == [1, 1] and out["dist"].shape == (B, P)
    # by hand: round 0 returns init and its vertices; the kernel's correspondences feed the restated fit
    z = torch.zeros(B, P, dtype=torch.int32).cuda()
    e0 = torch.tensor([1.0, 0.0, 0.0]).repeat(B, P, 1).cuda()
    r0 = hands_amd.fit_mano_surface(_cuda(pts), z, e0, head, "r", weights=_cuda(w), init=tinit, config=hands_amd.SurfaceFitConfig(iters=0))
    assert all(torch.equal(r0[k], t) for k, t in zip(("pose", "beta", "transl"), tinit))
    cor = hands_amd.correspond_on_mesh(_cuda(pts), r0["verts"], pack["faces_i32"], _cuda(w))
    assert torch.equal(cor["dist"].view(torch.int32), out["dist"].view(torch.int32))
    g = {k: v.cpu().numpy() for k, v in cor.items()}
    ref = S.fit_rows(C, faces, pts, g["face_idx"], g["bary"], g["weights"], g["normal"], None, init, S.config(iters=3, tangent_weight=0.1))
    assert all(S.clear(r["trace"]) for r in ref) and sum(r["steps"] for r in ref) >= 4
    for k in ("pose", "beta", "transl", "rmse", "j3d", "verts"):
        r = np.stack([np.asarray(a["raw"][k], np.float64) for a in ref])
        ratio = (np.abs(out[k].cpu().numpy().astype(np.float64) - r) / bar(r)).max()
        print(f"REG|one round|{k}|{ratio:.3f} of the bar")
        assert ratio <= 1.0, k
    assert out["steps"].tolist() == [r["steps"] for r in ref]


# ---- 3. the loop ---------------------------------------------------------------------------------------------------------------
def test_the_loop_lowers_the_distance_as_the_restatement_does(assets):
    import hands_amd
    head, _, C, faces = assets["tube"]
    B, P = 2, 128
    cases = [S.registration_case(C, faces, 20 + b, P) for b in range(B)]
    pts = np.stack([c[0] for c in cases])
    init = tuple(_cuda(np.stack([c[1][i] for c in cases])) for i in range(3))
    cfg = hands_amd.RegisterConfig(rounds=6, iters=3)
    out = hands_amd.register_mano(_cuda(pts), head, "r", init=init, config=cfg)
    again = hands_amd.register_mano(_cuda(pts), head, "r", init=init, config=cfg)
    assert all(out[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes() for k in out)      # from launch to launch
    assert out["rounds_done"].tolist() == [6, 6]
    verts = out["verts"].cpu().numpy().astype(np.float64)
    for b in range(B):
        ref = S.register(C, faces, pts[b], cases[b][1], rounds=6, iters=3, tangent_weight=0.1)
        start, end = ref["history"][0], S.cloud_distance(pts[b], verts[b], faces)
        ref_end = S.cloud_distance(pts[b], ref["verts"].astype(np.float64), faces)
        print(f"REG|loop|hand {b}|start {start * 1e3:.3f} mm|device {end * 1e3:.4f} mm|restatement {ref_end * 1e3:.4f} mm|bar {LOOP_END_MAX * 1e3:.3f} mm")
        assert end < start and end <= LOOP_END_MAX


def test_the_truth_is_a_fixed_point(assets):
    """init = the truth on a noise-free cloud of the model's own surface, no priors: the vertices move by less than 1e-6 m (the
    bar of tests/test_fit_surf.py; the cloud's and the vertices' fp32 rounding is 3e-8 m) and the distance stays below it."""
    import hands_amd
    head, _, C, faces = assets["tube"]
    pts, _, (R, beta, t) = S.registration_case(C, faces, 5, 128)
    init = tuple(np.asarray(a, np.float32)[None] for a in (R, beta, t))
    v0 = V.vertices_of(C, init[0][0].astype(np.float64), init[1][0].astype(np.float64)) + init[2][0].astype(np.float64)
    out = hands_amd.register_mano(_cuda(pts[None]), head, "r", init=tuple(_cuda(a) for a in init),
                                  config=hands_amd.RegisterConfig(rounds=3, iters=3, lambda_beta=0.0, lambda_pose=0.0))
    move = np.abs(out["verts"][0].cpu().numpy().astype(np.float64) - v0).max()
    end = S.cloud_distance(pts, out["verts"][0].cpu().numpy().astype(np.float64), faces)
    print(f"REG|fixed point|moved {move:.3e} m|distance {end:.3e} m|1e-6")
    assert out["rounds_done"].tolist() == [3] and move <= 1e-6 and end <= 1e-6


def test_a_starved_hand_keeps_its_state(assets):
    """fit_surf_ref.starved_case under STARVE: hand 0 is pulled off its cloud by heavy priors in round 1, the 0.1 mm trim leaves
    round 2 and 3 fewer than four points, so it keeps round 1's state and rounds_done says 1; hand 1 sits at the mean pose, feels
    no prior and is fitted in all three rounds.  Both hands through register_mano_hands with the same asset on both sides."""
    import hands_amd
    head, pack, C, faces = assets["tube"]
    cases = [S.starved_case(C, faces, 30, False), S.starved_case(C, faces, 31, True)]
    refs = [S.register(C, faces, c[0], c[1], **S.STARVE) for c in cases]
    assert [r["rounds_done"] for r in refs] == [1, 3] and int((refs[0]["dist"] <= S.STARVE["max_dist"]).sum()) < 4
    pts = _cuda(np.stack([c[0] for c in cases]))
    init = tuple(_cuda(np.stack([c[1][i] for c in cases])) for i in range(3))
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": pack, "mano_l": pack}})()
    full = hands_amd.register_mano_hands(pts, pts, pair, init, init, config=hands_amd.RegisterConfig(**S.STARVE))
    one = hands_amd.register_mano_hands(pts, pts, pair, init, init, config=hands_amd.RegisterConfig(**dict(S.STARVE, rounds=1)))
    for f, o in zip(full, one):
        assert f["rounds_done"].tolist() == [1, 3] and o["rounds_done"].tolist() == [1, 1]
        for k in ("pose", "beta", "transl", "rmse", "steps", "j3d", "verts", "pose_aa"):
            assert torch.equal(f[k][0], o[k][0]), k                    # round 1's state, bit for bit
        assert not torch.equal(f["verts"][1], o["verts"][1])
        assert int((f["dist"][0] <= S.STARVE["max_dist"]).sum()) < 4 and bool(torch.isfinite(f["rmse"]).all())
    assert all(torch.equal(full[0][k], full[1][k]) for k in full[0])   # the same asset and data on both sides: the same bits
    # a hand no round accepts: rounds_done 0, the start handed back, rmse NaN
    none = hands_amd.register_mano(pts, head, "r", init=init, valid=torch.tensor([1.0, 0.0]).cuda(),
                                   config=hands_amd.RegisterConfig(rounds=2, iters=1))
    assert none["rounds_done"].tolist() == [2, 0] and torch.isnan(none["rmse"]).tolist() == [False, True]
    assert bool(torch.isnan(none["verts"][1]).all())


# ---- 4. predictions ------------------------------------------------------------------------------------------------------------
def test_register_predictions_moves_registered_rows_only(assets):
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import pack_mano_pair, run_mano_heads
    from hands_amd.smoothing import HEAD_KEYS
    B, P = 3, 64
    packs = pack_mano_pair(assets["soup"][0], assets["soup_l"][0], torch.device("cuda"))
    pair = type("Pair", (), {"packed": lambda self, dev: {"mano_r": packs[0], "mano_l": packs[1]}, "img_res": 224})()
    rng = np.random.RandomState(12)
    rot, shape, cam, cloud = [], [], [], {}
    for i, h in enumerate("rl"):
        C = assets[("soup", "soup_l")[i]][2]
        ys = []
        for b in range(B):
            y, _, (R, beta, t) = V.family_case(C, 800 + 10 * i + b)
            ys.append(y[rng.choice(778, P, replace=False)])
            full = np.concatenate([V.log_so3(R[j] @ V.exp_so3(0.05 * rng.randn(3))) for j in range(16)]) - C.pose_mean
            rot.append(np.stack([V.exp_so3(full[3 * j:3 * j + 3]) for j in range(16)]))
            shape.append(beta + 0.1 * rng.randn(10))
            t = t + 0.005 * rng.randn(3)
            cam.append([2.0 * 1000.0 / (224.0 * t[2]), t[0], t[1]])
        cloud[h] = _cuda(np.stack(ys))
    K = _cuda(np.repeat(np.array([[[1000.0, 0, 112.0], [0, 1000.0, 112.0], [0, 0, 1.0]]]), B, 0))
    pred = hands_amd.xdict(run_mano_heads(_lib.lib(), packs[0], packs[1], _cuda(rot), _cuda(shape), _cuda(cam), _cuda(cam), K, 224.0, B,
                                          torch.cuda.current_stream().cuda_stream, None))
    pred["grasp.r"] = torch.arange(B, dtype=torch.float32).cuda()
    valid_r = torch.tensor([1.0, 0.0, 1.0]).cuda()
    cloud["l"][2, 5, 0] = float("nan")                                 # a weighted point that is no number: the hand is not registered
    out = hands_amd.register_predictions(pred, cloud["r"], cloud["l"], pair, {"intrinsics": K}, valid_r=valid_r,
                                         config=hands_amd.RegisterConfig(rounds=3, iters=2))
    assert isinstance(out, hands_amd.xdict) and list(out) == list(pred) + ["refined.r", "refined.l"]
    assert out["refined.r"].tolist() == [True, False, True] and out["refined.l"].tolist() == [True, True, False]
    head = [f"mano.{k}.{h}" for h in "rl" for k in HEAD_KEYS]
    for k in pred:
        assert (k in head) or out[k] is pred[k], k
    cloud["l"][2, 5, 0] = 0.0
    for h in "rl":
        moved = out[f"refined.{h}"]
        for k in HEAD_KEYS:
            a, b = out[f"mano.{k}.{h}"], pred[f"mano.{k}.{h}"]
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(a[~moved].view(torch.int32), b[~moved].view(torch.int32)), (k, h)
        assert not torch.equal(out[f"mano.vertices.{h}"][moved], pred[f"mano.vertices.{h}"][moved])
