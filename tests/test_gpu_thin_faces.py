"""Nearly degenerate faces on the device (scenes: tests/thin_faces.py; the same arithmetic on the host: tests/test_thin_faces.py):
hands_mesh_closest_f32, hands_mesh_signed_f32, hands_eval_surface_metrics_f32 and hands_amd.interhand_field against the fp64
restatement, with the bars of tests/test_gpu_surface_metrics.py and tests/test_gpu_penetration.py as they stand there: distances,
face excess, | |p - c| - d | and c-to-face within 5e-7 m with no query excused, metric keys rtol 2e-5 / atol 5e-4 mm.

The single-face grid is one batch of 96 rows x 16 orientations x 6 vertex orders = 9216 samples of one triangle each, 256 queries
per face.  The kernels see it in one launch (the |sdf| and the reproducibility tests); check_closest takes it in eight -- one per
shape and edge length -- because its restatement costs a millisecond of host time per SAMPLE and a case has to stay quick.
The winding number is asserted on the `clear` set of the split cube only: across a thin face its true value jumps within the
face's height, and a single open triangle has no inside.
"""
import numpy as np
import pytest
import torch

import surface_ref as SR
import thin_faces as TF
from test_gpu_penetration import SIZE, check_signed, run_signed
from test_gpu_surface_metrics import BAR, CENTRE, _closest, _cuda, _rot, check_closest, check_metrics, _run

pytestmark = pytest.mark.gpu

ONE_FACE = np.array([[0, 1, 2]])
RATIOS = (1e-3, 1e-5)


def test_the_scenes_are_placed_as_the_existing_suites_place_theirs():
    assert (TF.CENTRE == CENTRE).all() and TF.SIZE == SIZE and TF.LIMIT == 0.6
    assert np.abs(TF.rot([1, 2, 3], 0.3) - _rot([1, 2, 3], 0.3)).max() == 0


@pytest.fixture(scope="module")
def grid():
    """tri (B,3,3), queries (B,P,3), row (B) and the restatement's fp64 distances (B,P), computed once."""
    tri, q, row = TF.single_face_batch()
    assert tri.shape == (6 * sum(TF.n_orient(r) for r in range(len(TF.ROWS))), 3, 3) and q.shape == (len(tri), TF.P, 3)
    return tri, q, row, TF.pair_distance(tri, q)


# ---- 1. hands_mesh_closest_f32 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", TF.LENGTHS)
@pytest.mark.parametrize("shape", TF.SHAPES)
def test_single_faces_closest(grid, shape, L):
    tri, q, row, _ = grid
    rows = [r for r, spec in enumerate(TF.ROWS) if spec[:2] == (shape, L)]
    assert len(rows) == 2 * len(TF.RATIOS)
    keep = np.isin(row, rows)
    dist, idx, _ = check_closest(q[keep], tri[keep], ONE_FACE, what=f"{shape} L={L:g}")
    assert (idx == 0).all() and np.isfinite(dist).all()


def _placed(name, ratio):
    """-> verts (B,V,3) fp32, faces, thin face indices: the split cube as it is, the collapsed grid as test_mano_counts places
    its grid (and a second, turned sample)."""
    if name == "split_cube":
        v, f, thin = TF.split_cube(ratio)
        return np.float32(v[None]), f, thin
    v, f, thin = TF.collapsed_grid(ratio)
    off = CENTRE * [1, 1, 0.9]
    return np.float32(np.stack([v + off, v @ _rot([1, 2, 3], 0.8).T + off * [-1, 1, 1]])), f, thin


def _mesh_queries(verts, faces, thin, seed):
    """The three query sets of every sample, cut to the same count per set: {set: (B,n,3)} and all of them (B,P,3)."""
    per = [TF.mesh_queries(v, faces, thin, seed + b) for b, v in enumerate(verts)]
    sets = {k: np.stack([p[k][:min(len(x[k]) for x in per)] for p in per]) for k in per[0]}
    return sets, np.concatenate(list(sets.values()), 1)


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", ["split_cube", "collapsed_grid"])
def test_meshes_closest(name, ratio):
    verts, faces, thin = _placed(name, ratio)
    sets, points = _mesh_queries(verts, faces, thin, seed=11)
    assert all(len(s[0]) >= 8 for s in sets.values())
    check_closest(points, verts, faces, what=f"{name} ratio {ratio:g}")


# ---- 2. hands_mesh_signed_f32 ----------------------------------------------------------------------------------------------
def _check_abs_sdf(points, verts, faces, what):
    """|sdf| and the reported face against the restatement on every finite query; the winding number is not asserted."""
    sdf, w, idx = run_signed(points, verts, faces)
    rd, ri, _ = SR.closest_on_mesh(points, verts, faces)
    fin = np.isfinite(rd)
    assert fin.all() and np.isfinite(sdf).all() and np.isfinite(w).all() and ((idx >= 0) & (idx < len(faces))).all()
    e_d = np.abs(np.abs(sdf.astype(np.float64)) - rd).max()
    e_f = max(float((SR.distance_to_face(points[b], verts[b], faces, idx[b]) - rd[b]).max()) for b in range(len(points)))
    print(f"THIN|signed|{what}|d {e_d:.2e} / {BAR:.1e}|face excess {e_f:.2e}")
    assert e_d <= BAR and e_f <= BAR, (what, e_d, e_f)


def test_single_faces_signed(grid):
    """The whole grid in one launch: |sdf| within the bar on every query, the face is the only one there is."""
    tri, q, row, ref = grid
    sdf, w, idx = run_signed(q, tri, ONE_FACE)
    assert np.isfinite(sdf).all() and (idx == 0).all()
    err = np.abs(np.abs(sdf.astype(np.float64)) - ref)
    for r, spec in enumerate(TF.ROWS):
        print(f"THIN|device|{'|'.join(str(x) for x in spec)}|worst {err[row == r].max():.2e} / {BAR:.0e}|over {(err[row == r] > BAR).sum()}")
    assert err.max() <= BAR, [(TF.ROWS[r], float(err[row == r].max())) for r in np.unique(row[(err > BAR).any(1)])]


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("name", ["split_cube", "collapsed_grid"])
def test_meshes_signed(name, ratio):
    verts, faces, thin = _placed(name, ratio)
    sets, points = _mesh_queries(verts, faces, thin, seed=11)
    _check_abs_sdf(points, verts, faces, f"{name} ratio {ratio:g}")
    if name == "split_cube":                               # closed: the full check where the winding number is decided
        sdf, w, _ = check_signed(sets["clear"], verts, faces, what=f"split cube ratio {ratio:g}, clear set")
        assert (sdf < 0).any() and (sdf > 0).any()


# ---- 3. the metrics and the field ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def collapsed_hands():
    """Ground truth: the collapsed grid under both hands (ratio 1e-3 right, 1e-5 left), B = 2; prediction: the same plus 2 mm of
    noise."""
    rng = np.random.RandomState(21)
    pred, targets, faces = {}, {}, []
    for s, ratio, x in (("r", 1e-3, 0.05), ("l", 1e-5, -0.04)):
        v, f, _ = TF.collapsed_grid(ratio)
        faces.append(f)
        gv = np.stack([v @ _rot([b + 1, 2, 3], 0.4 * b).T + [x, -0.03 + 0.01 * b, 0.42] for b in range(2)])
        gj = np.stack([g[rng.choice(778, 21, replace=False)] * [1, 1, 0.999] for g in gv])
        targets[f"mano.v3d.cam.{s}"], targets[f"mano.j3d.cam.{s}"] = np.float32(gv), np.float32(gj)
        pred[f"mano.v3d.cam.{s}"] = np.float32(gv + 2e-3 * rng.randn(*gv.shape))
        pred[f"mano.j3d.cam.{s}"] = np.float32(gj + 2e-3 * rng.randn(*gj.shape))
    assert max(np.abs(x).max() for d in (pred, targets) for x in d.values()) <= 0.6
    targets.update(is_valid=np.ones(2, np.float32), right_valid=np.ones(2, np.float32), left_valid=np.ones(2, np.float32))
    return pred, targets, tuple(faces)


def test_surface_metrics_on_collapsed_hands(collapsed_hands):
    pred, targets, faces = collapsed_hands
    got = _run(pred, targets, faces)
    check_metrics(got, SR.evaluate_surface(pred, targets, *faces), "collapsed grid")
    assert all(np.isfinite(v).all() for v in got.values()) and (got["p2s/ra/r"] > 0.3).all()       # the noise shows, mm


def test_interhand_field_on_collapsed_hands(collapsed_hands):
    from hands_amd import interhand_field
    _, targets, faces = collapsed_hands
    v_r, v_l = targets["mano.v3d.cam.r"], targets["mano.v3d.cam.l"]
    ref = SR.interhand_field(v_r, v_l, *faces)
    out = interhand_field({"mano.v3d.cam.r": _cuda(v_r), "mano.v3d.cam.l": _cuda(v_l)}, faces=faces)
    torch.cuda.synchronize()
    for k, (q, t, f) in (("rl", (v_r, v_l, faces[1])), ("lr", (v_l, v_r, faces[0]))):
        dist, idx = out["dist." + k].cpu().numpy(), out["idx." + k].cpu().numpy()
        e_d = np.abs(dist - ref["dist." + k]).max()
        e_f = max(float((SR.distance_to_face(q[b], t[b], f, idx[b]) - ref["dist." + k][b]).max()) for b in range(len(q)))
        print(f"THIN|field|{k}|d {e_d:.2e} / {BAR:.1e}|face excess {e_f:.2e}")
        assert e_d <= BAR and e_f <= BAR


# ---- 4. reproducibility ----------------------------------------------------------------------------------------------------
def test_bit_reproducible_and_batch_independent(grid):
    tri, q, row, _ = grid
    a, b = _closest(q, tri, ONE_FACE), _closest(q, tri, ONE_FACE)
    s, t = run_signed(q, tri, ONE_FACE), run_signed(q, tri, ONE_FACE)
    for x, y in zip(a + s, b + t):
        assert x.tobytes() == y.tobytes()
    for r in (TF.ROWS.index(("sliver", 1e-2, 1e-5, 1)), TF.ROWS.index(("cap", 1e-1, 1e-1, 0))):     # a thin row, a plain one
        keep = row == r
        alone = _closest(q[keep], tri[keep], ONE_FACE) + run_signed(q[keep], tri[keep], ONE_FACE)
        for x, y in zip(a + s, alone):
            assert x[keep].tobytes() == y.tobytes(), TF.ROWS[r]
