"""Temporal smoothing without a GPU: the fp64 restatement (tests/smooth_ref.py) of DESIGN.md section 7 "Temporal smoothing"
against closed forms it shares nothing with, its state rules and streaming invariance, the synthetic case that shows the filter
does its job, the host side of the two C-ABI entries and the Python names, and a compile-only resource guard of
csrc/smooth.hip."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import accel_ref as AR
import smooth_ref as SR

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SPLITS9 = ((9,), (4, 5), (1, 8), (1,) * 9)


def eye_pose(rows):
    return np.tile(np.eye(3, dtype=np.float32), (rows, 16, 1, 1))


def one_channel(R):
    """(T,3,3) -> the inputs of a stream whose rotation channel 0 is R and whose other channels rest."""
    T = len(R)
    pose = eye_pose(T)
    pose[:, 0] = R
    return pose, np.zeros((T, 10), np.float32), np.zeros((T, 3), np.float32)


def scalar_one_euro(x, dt, mc, beta, dc):
    """The scalar One-Euro filter of the paper, written out on its own."""
    a = lambda f: 1.0 / (1.0 + 1.0 / (2.0 * math.pi * f * dt))
    out, prev, xh, dh = [x[0]], x[0], x[0], 0.0
    for v in x[1:]:
        dh = a(dc) * ((v - prev) / dt) + (1.0 - a(dc)) * dh
        al = a(mc + beta * abs(dh))
        xh = al * v + (1.0 - al) * xh
        prev = v
        out.append(xh)
    return np.array(out)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def run_split(arrays, split, valid=None, seq=None, steps_of=lambda n: n, S=1, **kw):
    """Filter the rows in consecutive calls of split[i] time steps each, one list of streams carried along."""
    streams = [SR.Stream() for _ in range(S)]
    outs, at = [], 0
    for n in split:
        sl = slice(at * S, (at + n) * S)
        outs.append(SR.smooth(*(a[sl] for a in arrays), valid=None if valid is None else valid[sl],
                              seq=None if seq is None else seq[sl], steps=n, streams=streams, **kw))
        at += n
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(3))


# ---- independent pins of the restatement ---------------------------------------------------------------------------------------
def test_vector_channel_with_beta_zero_is_the_exponential_filter():
    T, fps, mc = 12, 30.0, 1.5
    _, beta, cam = SR.random_walk(T, 1)
    got = SR.smooth(eye_pose(T), beta, cam, fps=fps, cfg=SR.config(min_cutoff=mc, beta=0.0))
    tau = 1.0 / (2.0 * math.pi * mc)
    a = (1.0 / fps) / (tau + 1.0 / fps)                      # the first-order low-pass of time constant tau
    for x, y in ((beta, got[1]), (cam, got[2])):
        w = np.array([[a * (1.0 - a) ** (t - j) if j else (1.0 - a) ** t for j in range(T)] for t in range(T)])
        closed = np.tril(w) @ x.astype(np.float64)           # x^_t = (1-a)^t x_0 + sum_j a (1-a)^(t-j) x_j
        assert np.abs(closed - y).max() <= 2.0 ** -23 * np.abs(closed).max()
    assert same_bits((got[0],), (eye_pose(T),))


def test_fixed_axis_rotations_follow_the_scalar_filter():
    T, fps = 40, 30.0
    rng = np.random.RandomState(2)
    theta = np.cumsum(rng.uniform(-0.2, 0.2, T))
    for axis in ((0, 0, 1.0), (1.0, -2.0, 0.5)):
        for mc, b, dc in ((1.5, 0.5, 1.0), (0.8, 2.0, 3.0)):
            S = SR.Stream()
            dt, cfg = 1.0 / fps, SR.config(mc, b, dc)
            want = scalar_one_euro(theta, dt, mc, b, dc)
            for t in range(T):
                R = SR.axis_rotation(axis, theta[t])
                if t == 0:
                    S.start(np.tile(R, (16, 1, 1)), np.zeros(10), np.zeros(3), None)
                    got = R
                else:
                    got = SR._rotation(S, 0, R, dt, cfg["min_cutoff"][0], cfg["beta"][0], cfg["d_cutoff"][0])
                assert np.abs(got - SR.axis_rotation(axis, want[t])).max() <= 1e-12, (axis, t)


def test_exp_and_log_are_inverse():
    rng = np.random.RandomState(3)
    for angle in list(np.geomspace(1e-3, 3.0, 25)) + [1e-3, 3.0]:
        u = rng.randn(3)
        w = u / np.linalg.norm(u) * angle
        assert np.abs(SR.log_so3(SR.exp_so3(w)) - w).max() <= 1e-12 * max(1.0, 1.0 / math.sin(angle)), angle
        E = SR.exp_so3(w)
        assert np.abs(E.T @ E - np.eye(3)).max() <= 1e-14
    assert np.array_equal(SR.exp_so3(np.zeros(3)), np.eye(3)) and np.array_equal(SR.log_so3(np.eye(3)), np.zeros(3))
    tiny = np.array([3e-7, -2e-7, 1e-7])                     # the series branch
    assert np.abs(SR.log_so3(SR.exp_so3(tiny)) - tiny).max() <= 1e-18


def test_half_turn_branch_returns_an_axis_of_the_rotation():
    oblique = np.array([1.0, -2.0, 0.5])
    oblique /= np.linalg.norm(oblique)
    cases = [np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]), np.diag([-1.0, -1.0, 1.0]),
             2.0 * np.outer(oblique, oblique) - np.eye(3)]
    for D in cases:
        w = SR.log_so3(D)
        assert abs(np.linalg.norm(w) - math.pi) <= 1e-15
        assert np.abs(SR.exp_so3(w) - D).max() <= 1e-15 * 8, D
    assert np.array_equal(SR.log_so3(cases[0]), [math.pi, 0.0, 0.0])
    assert np.allclose(SR.log_so3(cases[3]) / math.pi, -oblique, atol=1e-15)          # the largest component (y) is positive


# ---- state rules ---------------------------------------------------------------------------------------------------------------
def test_invalid_nan_and_id_change_pass_through_and_restart():
    T = 9
    base = SR.random_walk(T, 4)
    for kind in ("invalid", "nan", "inf", "id"):
        arrays = tuple(a.copy() for a in base)
        valid, seq, k = np.ones(T, np.float32), np.full(T, 5, np.int64), 4
        if kind == "invalid":
            valid[k] = 0
        elif kind == "nan":
            arrays[1][k, 7] = np.nan
        elif kind == "inf":
            arrays[0][k, 15, 2, 2] = -np.inf
        else:
            seq[k:] = -3
        out = SR.smooth(*arrays, valid=valid, seq=seq)
        rows = [0, k] if kind == "id" else [0, k, k + 1]     # after a dead frame the next usable one starts the stream
        for r in range(T):
            same = same_bits(tuple(o[r] for o in out), tuple(a[r] for a in arrays))
            assert same == (r in rows), (kind, r)
        # the restart forgets: the tail equals a fresh run on the tail
        tail = rows[-1]
        fresh = SR.smooth(*(a[tail:] for a in arrays))
        assert same_bits(tuple(o[tail:] for o in out), fresh), kind


def test_every_frame_its_own_sequence_is_the_identity():
    arrays = SR.random_walk(7, 5)
    out = SR.smooth(*arrays, seq=np.arange(7))
    assert same_bits(out, arrays)
    assert not same_bits(SR.smooth(*arrays), arrays)


@pytest.mark.parametrize("mode", SR.SHAPE_MODES)
def test_shape_modes(mode):
    arrays = SR.random_walk(6, 6)
    out = SR.smooth(*arrays, cfg=SR.config(shape_mode=mode))
    x = arrays[1].astype(np.float64)
    if mode == "mean":
        want = (np.cumsum(x, 0) / np.arange(1, 7)[:, None]).astype(np.float32)
        assert np.abs(out[1] - want).max() <= 2.0 ** -23 * np.abs(want).max()
    elif mode == "none":
        assert same_bits((out[1],), (arrays[1],))
    else:
        assert not same_bits((out[1][1:],), (arrays[1][1:],))
    assert same_bits((out[0], out[2]), (SR.smooth(*arrays)[0], SR.smooth(*arrays)[2]))


# ---- streaming invariance ------------------------------------------------------------------------------------------------------
def test_any_split_into_calls_gives_the_same_arrays():
    T = 9
    arrays = SR.random_walk(T, 7)
    valid, seq = np.ones(T, np.float32), np.array([2, 2, 2, 2, 2, 2, 9, 9, 9])
    valid[3] = 0
    for mode in SR.SHAPE_MODES:
        cfg = SR.config(shape_mode=mode)
        one = SR.smooth(*arrays, valid=valid, seq=seq, cfg=cfg)
        for split in SPLITS9:
            assert same_bits(run_split(arrays, split, valid, seq, cfg=cfg), one), (mode, split)


def test_streams_layout_equals_separate_runs():
    T, S = 5, 3
    parts = [SR.random_walk(T, 800 + s) for s in range(S)]
    arrays = tuple(SR.interleave([p[i] for p in parts]) for i in range(3))
    seq = SR.interleave([np.array([s, s, s, s + 10, s + 10]) for s in range(S)])
    out = SR.smooth(*arrays, seq=seq, steps=T)
    for s in range(S):
        alone = SR.smooth(*parts[s], seq=seq[s::S])
        assert same_bits(tuple(o[s::S] for o in out), alone), s
    frames = run_split(arrays, (1,) * T, seq=seq, S=S)       # "streams": one frame of every stream per call
    assert same_bits(frames, out)


# ---- it does its job -----------------------------------------------------------------------------------------------------------
def accel_of_rotations(R, clean, fps):
    """Acceleration error of 20 points at 8 cm carried by R (T,3,3) against the same points carried by ``clean``."""
    rng = np.random.RandomState(11)
    p = rng.randn(20, 3)
    p = 0.08 * p / np.linalg.norm(p, axis=1, keepdims=True)
    move = lambda M: np.einsum("tij,nj->tni", M, p).astype(np.float32)
    return float(np.nanmean(AR.accel_error(move(clean), move(R), fps=fps)))


def test_default_config_halves_the_acceleration_error_of_a_jittered_rotation():
    fps = 30.0
    clean, noisy = SR.jitter_case(T=64, fps=fps, sigma=0.03)
    smoothed = SR.smooth(*one_channel(noisy), fps=fps)[0][:, 0]
    raw, got = accel_of_rotations(noisy, clean, fps), accel_of_rotations(smoothed.astype(np.float64), clean, fps)
    print(f"SMOOTH|jitter sigma 0.03|raw {raw:.3f} m/s^2|smoothed {got:.3f} m/s^2|ratio {got / raw:.3f}")
    assert got <= 0.5 * raw, (got, raw)


# ---- the host side -------------------------------------------------------------------------------------------------------------
def test_header_and_binding_hold_the_entries():
    from hands_amd import _lib
    header = open(os.path.join(ROOT, "include", "hands_hip.h")).read()
    assert re.search(r"^int\s+hands_smooth_mano_f32\s*\(", header, flags=re.M) and "hands_smooth_mano_f32" in _lib.SIGNATURES
    assert re.search(r"^long long\s+hands_smooth_state_bytes\s*\(void\)", header, flags=re.M)
    assert "hands_smooth_state_bytes" in _lib.EXTRA_SYMBOLS
    assert "#define HANDS_ABI_VERSION 5" in header and _lib.ABI_VERSION == 5
    side = re.search(r"typedef struct hands_smooth_side \{(.*?)\} hands_smooth_side;", header, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)\s*[,;]", side) == [n for n, _ in _lib.SmoothSide._fields_]
    cfg = re.search(r"typedef struct hands_smooth_cfg \{[^\n]*\n(.*?)\} hands_smooth_cfg;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[3\])?[,;]", cfg) == [n for n, _ in _lib.SmoothCfg._fields_]
    assert ctypes.sizeof(_lib.SmoothSide) == 8 * ctypes.sizeof(ctypes.c_void_p) and ctypes.sizeof(_lib.SmoothCfg) == 80
    for name, code in _lib.SMOOTH_SHAPE_MODES.items():
        assert f"#define HANDS_SMOOTH_SHAPE_{name.upper()} {code}" in header
    assert "smooth.hip" in open(os.path.join(ROOT, "hands_amd", "csrc", "Makefile")).read()
    n = _lib.lib().hands_smooth_state_bytes()
    # what the specification names, fp64: 16 x (raw 9, hat 9, estimate 3), shape 4 x 10, camera 3 x 3, then id, live, count
    assert n == 8 * (16 * 21 + 40 + 9 + 3) and n % 8 == 0


def test_names_are_exported():
    import hands_amd
    for n in ("SmoothConfig", "smooth_mano_params", "smooth_predictions", "TemporalSmoother"):
        assert n in hands_amd.__all__ and callable(getattr(hands_amd, n)), n
    c = hands_amd.SmoothConfig()
    assert (c.min_cutoff, c.beta, c.d_cutoff, c.shape_mode) == (1.5, 0.5, 1.0, "filter")
    assert "NOT tuned" in hands_amd.SmoothConfig.__doc__
    ref = SR.config()
    s = c.c_struct()
    assert (tuple(s.min_cutoff), tuple(s.beta), tuple(s.d_cutoff)) == (ref["min_cutoff"], ref["beta"], ref["d_cutoff"])
    assert tuple(hands_amd.SmoothConfig(beta=(0.1, 0.2, 0.3)).c_struct().beta) == (0.1, 0.2, 0.3)
    with pytest.raises(ValueError):
        hands_amd.SmoothConfig(shape_mode="median").c_struct()
    with pytest.raises(ValueError):
        hands_amd.TemporalSmoother(None, layout="frames")


def test_smoothing_refuses_cpu_tensors(recipe_model):
    import hands_amd
    pose, beta, cam = (torch.from_numpy(a) for a in SR.random_walk(3, 8))
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.smooth_mano_params(pose, beta, cam)
    pred = {f"mano.{k}.{h}": v for h in "rl" for k, v in (("pose", pose), ("beta", beta), ("cam_t.wp", cam))}
    meta = {"intrinsics": torch.eye(3).repeat(3, 1, 1)}
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.smooth_predictions(pred, recipe_model, meta)
    with pytest.raises(RuntimeError, match="HIP device only"):
        hands_amd.TemporalSmoother(recipe_model).update(pred, meta)


def test_entry_rejects_bad_arguments_without_a_gpu():
    from hands_amd import _lib
    L = _lib.lib()
    p, E = 16, 10001                                     # never dereferenced: every call below is refused
    good_side = lambda: _lib.SmoothSide(p, p, p, None, p, p, p, None)
    three = lambda v: (ctypes.c_double * 3)(*v)

    def call(sides=None, nsides=1, T=3, S=2, fps=30.0, mc=(1.5,) * 3, b=(0.5,) * 3, dc=(1.0,) * 3, mode=0, cfg=True, seq=p):
        arr = (_lib.SmoothSide * 2)(*(sides or [good_side(), good_side()]))
        c = _lib.SmoothCfg(three(mc), three(b), three(dc), mode)
        return L.hands_smooth_mano_f32(arr, nsides, seq, T, S, fps, ctypes.byref(c) if cfg else None, None)

    assert L.hands_smooth_mano_f32(None, 1, p, 3, 2, 30.0, ctypes.byref(_lib.SmoothCfg(three((1,) * 3), three((0,) * 3), three((1,) * 3), 0)),
                                   None) == E
    assert call(cfg=False) == E
    for i, name in enumerate(n for n, _ in _lib.SmoothSide._fields_):
        if name in ("valid", "state"):
            continue
        for which, nsides in ((0, 1), (0, 2), (1, 2)):
            sides = [good_side(), good_side()]
            setattr(sides[which], name, None)
            assert call(sides=sides, nsides=nsides) == E, (name, which, nsides)
    for nsides in (0, -1, 3):
        assert call(nsides=nsides) == E, nsides
    for T, S in ((0, 1), (-1, 1), (1, 0), (1, -4)):
        assert call(T=T, S=S) == E, (T, S)
    inf, nan = float("inf"), float("nan")
    for fps in (0.0, -30.0, inf, -inf, nan):
        assert call(fps=fps) == E, fps
    for g in range(3):
        for bad in (0.0, -1.0, inf, nan):
            v = [1.0] * 3
            v[g] = bad
            assert call(mc=v) == E and call(dc=v) == E, (g, bad)
        for bad in (-1e-9, inf, nan):
            v = [0.5] * 3
            v[g] = bad
            assert call(b=v) == E, (g, bad)
    for mode in (-1, 3, 99):
        assert call(mode=mode) == E, mode
    assert call(seq=None, T=0) == E


def test_wrapper_has_no_smoother_by_default(recipe_model):
    from hands_amd.wrapper import HandsWrapper
    w = HandsWrapper(model=recipe_model)
    assert w.smoother is None
    w.reset_smoother()                                   # nothing to reset: no error
    calls = []
    w.smoother = type("S", (), {"reset": lambda self: calls.append(1)})()
    w.reset_smoother()
    assert calls == [1]


# ---- compile-only resource guard -----------------------------------------------------------------------------------------------
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_smooth_kernel_resources(tmp_path):
    """csrc/smooth.hip as the Makefile builds it: the kernel uses no scratch and no LDS, and compiles without a warning."""
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{ROOT}/include", f"-I{ROOT}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
                        "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(ROOT, "hands_amd", "csrc", "smooth.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning:" not in p.stderr, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)[1:]
    field = lambda b, pat: int(re.search(pat, b).group(1))
    assert len(blocks) == 1 and "smooth_kernel" in blocks[0].split()[0]
    assert field(blocks[0], r"ScratchSize \[bytes/lane\]: (\d+)") == 0 and field(blocks[0], r"VGPRs Spill: (\d+)") == 0
    assert field(blocks[0], r"LDS Size \[bytes/block\]: (\d+)") == 0
