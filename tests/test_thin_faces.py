"""Nearly degenerate faces without a GPU (scenes: tests/thin_faces.py).

1. The fp64 restatement (surface_ref.point_triangle) against an exact evaluation of the same definition in rational arithmetic
   on the fp32 inputs: 1e-12 m after the square root, on pairs of every single-face row.
2. The kernel's own arithmetic -- make_face and tri_dist2 of csrc/mesh_distance_device.h, compiled for the host with the
   library's floating-point flags by tests/thin_face_host.cpp -- against the restatement on EVERY pair of every row: distance,
   closest point on the face, closest point at the distance, each within 5e-7 m (test_gpu_surface_metrics.BAR and its reasoning).
3. The restatement keeps the `clear` query set of the split cube away from a winding number of 0.5, as
   tests/test_gpu_thin_faces.py relies on.
tools/thin_face_table.py runs part 2 against the header of any revision and prints the table of docs/EXPERIMENTS.md.
"""
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import penetration_ref as PR
import surface_ref as SR
import thin_faces as TF

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BAR = 5e-7               # metres: test_gpu_surface_metrics.BAR
EXACT_BAR = 1e-12


# ---- 1. the restatement against rational arithmetic ------------------------------------------------------------------------
def _sub(u, v):
    return [x - y for x, y in zip(u, v)]


def _dot(u, v):
    return sum(x * y for x, y in zip(u, v))


def _cross(u, v):
    return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]


def _seg(p, a, b):
    ab = _sub(b, a)
    L = _dot(ab, ab)
    t = min(max(_dot(_sub(p, a), ab) / L, Fraction(0)), Fraction(1)) if L > 0 else Fraction(0)
    r = _sub(p, [x + t * y for x, y in zip(a, ab)])
    return _dot(r, r)


def exact_d2(p, a, b, c):
    """The definition of include/hands_hip.h, exactly: the minimum of the three clamped segment distances and -- where the
    normal is not zero and the three barycentrics are >= 0 -- of the distance to the plane, squared, as a Fraction."""
    p, a, b, c = ([Fraction(float(x)) for x in v] for v in (p, a, b, c))
    best = min(_seg(p, a, b), _seg(p, a, c), _seg(p, b, c))
    n = _cross(_sub(b, a), _sub(c, a))
    nn = _dot(n, n)
    if nn > 0 and all(_dot(n, _cross(_sub(u, p), _sub(v, p))) >= 0 for u, v in ((b, c), (c, a), (a, b))):
        best = min(best, _dot(_sub(p, a), n) ** 2 / nn)
    return best


@pytest.mark.parametrize("shape", TF.SHAPES)
def test_restatement_is_exact_on_thin_faces(shape):
    """30 (face, query) pairs of every row: every vertex order and every query family."""
    worst = 0.0
    for row, spec in enumerate(TF.ROWS):
        if spec[0] != shape:
            continue
        tri, q = TF.all_orders(*TF.single_faces(row))
        rng = np.random.RandomState(row)
        fam = TF.family_of()
        for i in range(30):
            f = (7 * i + rng.randint(6)) % len(tri)                         # 7 is coprime to 6: the orders take turns
            j = rng.choice(np.flatnonzero(fam == i % len(TF.FAMILIES)))
            d2 = SR.point_triangle(q[f, j][None], *(tri[f, k][None] for k in range(3)), want_point=False)[0][0, 0]
            err = abs(math.sqrt(d2) - math.sqrt(exact_d2(q[f, j], *tri[f])))
            worst = max(worst, err)
            assert err <= EXACT_BAR, (spec, f, j, err)
    print(f"THIN|restatement vs exact|{shape}|{worst:.2e} / {EXACT_BAR:.0e}")


# ---- 2. the kernel's arithmetic on the host --------------------------------------------------------------------------------
def build_host(out_dir, header_dir=None, extra=()):
    """tests/thin_face_host.cpp -> a program; header_dir: where mesh_distance_device.h is taken from (default: csrc)."""
    exe = os.path.join(str(out_dir), "thin_face_host")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", f"-I{header_dir or os.path.join(ROOT, 'hands_amd', 'csrc')}",
           f"-I{ROOT}/include", "-fno-fast-math", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "thin_face_host.cpp"),
           "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return exe


def run_host(exe, tri, q, work_dir):
    """-> d (n,P) fp64 = sqrt of tri_dist2<false>, closest (n,P,3) fp32 of tri_dist2<true>; the two variants' distances are
    the same bits."""
    n, P = q.shape[:2]
    path = os.path.join(str(work_dir), "pairs.bin")
    with open(path, "wb") as fh:
        fh.write(np.int32([n, P]).tobytes() + np.float32(tri).tobytes() + np.float32(q).tobytes())
    p = subprocess.run([exe, path], capture_output=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = np.frombuffer(p.stdout, np.float32)
    assert out.size == 5 * n * P
    d2, d2p, cl = out[:n * P], out[n * P:2 * n * P], out[2 * n * P:].reshape(n, P, 3)
    assert d2.tobytes() == d2p.tobytes()
    return np.sqrt(d2.astype(np.float64)).reshape(n, P), cl


def pair_errors(tri, q, d, cl):
    """The three errors (n,P) of the module docstring against the restatement."""
    q, cl = q.astype(np.float64), cl.astype(np.float64)
    return np.abs(d - TF.pair_distance(tri, q)), TF.pair_distance(tri, cl), np.abs(np.sqrt(((q - cl) ** 2).sum(-1)) - d)


def row_table(exe, work_dir, rows=None):
    """Per row: (worst of the three errors, number of queries with one of them over BAR, number of queries)."""
    out = []
    for row in (range(len(TF.ROWS)) if rows is None else rows):
        tri, q = TF.all_orders(*TF.single_faces(row))
        errs = np.maximum.reduce(pair_errors(tri, q, *run_host(exe, tri, q, work_dir)))
        out.append((float(np.nanmax(errs)), int((~(errs <= BAR)).sum()), errs.size))
    return out


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("thin_face_host")
    return build_host(d), d


@pytest.mark.parametrize("shape", TF.SHAPES)
def test_kernel_arithmetic_on_the_host(host_program, shape):
    exe, work = host_program
    rows = [r for r, spec in enumerate(TF.ROWS) if spec[0] == shape]
    table = row_table(exe, work, rows)
    for r, (worst, over, n) in zip(rows, table):
        print(f"THIN|host|{'|'.join(str(x) for x in TF.ROWS[r])}|worst {worst:.2e} / {BAR:.0e}|over {over} of {n}")
    bad = [(TF.ROWS[r], t) for r, t in zip(rows, table) if t[1] or not t[0] <= BAR]
    assert not bad, bad


def test_host_program_reproduces_the_closed_forms(host_program):
    """The program itself is sound: the closed forms of test_surface_metrics, bit for bit."""
    from test_surface_metrics import CLOSED_FORMS, TRI
    exe, work = host_program
    q = np.float32([[x[0] for x in CLOSED_FORMS]])
    d, cl = run_host(exe, np.float32(TRI)[None], q, work)
    assert (d[0] == [x[1] for x in CLOSED_FORMS]).all() and (cl[0] == np.float32([x[2] for x in CLOSED_FORMS])).all()


# ---- 3. the clear sets -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1e-3, 1e-5])
def test_clear_set_of_the_split_cube_stays_off_the_surface(ratio):
    v, f, thin = TF.split_cube(ratio)
    assert all(len(u) == 2 and u[0] == u[1][::-1] for u in PR.edge_uses(f).values())       # closed, consistently oriented
    v32 = np.float32(v)
    T = v32.astype(np.float64)[f[thin[0]]]
    e = np.sqrt(((T - np.roll(T, 1, 0)) ** 2).sum(-1)).max()
    h = np.linalg.norm(np.cross(T[1] - T[0], T[2] - T[0])) / e
    assert 0.3 * ratio <= h / e <= 3 * ratio, h / e                                        # the face is as thin as asked for
    clear = TF.mesh_queries(v32, f, thin, seed=1)["clear"]
    assert len(clear) >= 256
    w = PR.winding_number(clear, v32, f)
    share = (np.abs(np.abs(w) - 0.5) <= 1e-3).mean()
    inside = np.abs(w) >= 0.5
    print(f"THIN|clear set|ratio {ratio:g}|{len(clear)} queries|near 0.5: {share:.4f}|inside {inside.mean():.2f}")
    assert share <= 0.01 and 0.05 < inside.mean() < 0.95
    assert np.abs(w - np.round(w)).max() <= 1e-6           # a closed surface: an integer, whatever the thin face contributes


def test_collapsed_grid_has_its_thin_faces():
    for ratio in (1e-3, 1e-5):
        v, f, thin = TF.collapsed_grid(ratio)
        T = np.float32(v + TF.CENTRE).astype(np.float64)[f[thin]]
        e = np.sqrt(((T - np.roll(T, 1, 1)) ** 2).sum(-1)).max(1)
        h = np.linalg.norm(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]), axis=1) / e
        assert len(thin) == 8 and (h / e <= 3 * max(ratio, 2e-5)).all() and (h > 0).all(), h / e
