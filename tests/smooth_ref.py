"""The One-Euro filter over MANO parameters of DESIGN.md section 7 ("Temporal smoothing"), restated in fp64 numpy: one-shot and
streaming, both layouts.  It shares no code with the package; tests/test_smoothing.py pins it against closed forms, and
tests/test_gpu_smoothing.py holds csrc/smooth.hip and hands_amd/smoothing.py to it.

A *hand-stream* is the sequence of frames of one hand of one video: per frame 16 rotations (3x3), a 10-vector and a 3-vector.
Rows are T time steps of S parallel streams, row t * S + s.  ``Stream`` is the state of one hand-stream; handing the same list
of them to consecutive ``smooth`` calls is the streaming form.
"""
import math

import numpy as np

GROUPS = ("rot", "shape", "cam")
SHAPE_MODES = ("filter", "mean", "none")


def config(min_cutoff=1.5, beta=0.5, d_cutoff=1.0, shape_mode="filter"):
    """The nine numbers (a scalar stands for all three groups rot, shape, cam) and the shape mode."""
    three = lambda v: tuple(float(x) for x in (v if isinstance(v, (tuple, list)) else (v, v, v)))
    assert shape_mode in SHAPE_MODES
    return {"min_cutoff": three(min_cutoff), "beta": three(beta), "d_cutoff": three(d_cutoff), "shape_mode": shape_mode}


def alpha(f, dt):
    r = 2.0 * math.pi * f * dt
    return r / (r + 1.0)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def log_so3(D):
    v = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    s = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = 0.5 * (D[0, 0] + D[1, 1] + D[2, 2] - 1.0)
    theta = math.atan2(s, c)
    if s >= 1e-9:
        return v * (theta / s)
    if c >= 0.0:
        return v
    u = np.array([math.sqrt(max(0.0, (D[i, i] - c) / (1.0 - c))) for i in range(3)])      # a half turn
    k = int(np.argmax(u))                                                                  # the lowest index on a tie
    for j in range(3):
        if j != k and D[j, k] + D[k, j] < 0.0:
            u[j] = -u[j]
    return u * (math.pi / math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))


def exp_so3(w):
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    K = hat(w)
    if theta < 1e-6:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (math.sin(theta) / theta) * K + ((1.0 - math.cos(theta)) / (theta * theta)) * (K @ K)


class Stream:
    """The state of one hand-stream: dead until a usable frame starts it."""

    def __init__(self):
        self.live, self.id = False, 0
        self.rot_raw, self.rot_hat, self.rot_d = np.zeros((16, 3, 3)), np.zeros((16, 3, 3)), np.zeros((16, 3))
        self.vec = {g: {"raw": np.zeros(n), "hat": np.zeros(n), "d": np.zeros(n)} for g, n in (("shape", 10), ("cam", 3))}
        self.sum, self.n = np.zeros(10), 0

    def start(self, pose, beta, cam, sid):
        self.live, self.id = True, sid
        self.rot_raw, self.rot_hat, self.rot_d = pose.copy(), pose.copy(), np.zeros((16, 3))
        for g, x in (("shape", beta), ("cam", cam)):
            self.vec[g] = {"raw": x.copy(), "hat": x.copy(), "d": np.zeros(len(x))}
        self.sum, self.n = beta.copy(), 1


def _vector(st, x, dt, mc, b, dc):
    d = (x - st["raw"]) / dt
    st["d"] = st["d"] + alpha(dc, dt) * (d - st["d"])
    f = mc + b * math.sqrt(float(np.sum(st["d"] * st["d"])))
    st["hat"] = st["hat"] + alpha(f, dt) * (x - st["hat"])
    st["raw"] = x.copy()
    return st["hat"]


def _rotation(S, c, R, dt, mc, b, dc):
    w = log_so3(S.rot_raw[c].T @ R) / dt
    S.rot_d[c] = S.rot_d[c] + alpha(dc, dt) * (w - S.rot_d[c])
    f = mc + b * math.sqrt(float(np.sum(S.rot_d[c] * S.rot_d[c])))
    S.rot_hat[c] = S.rot_hat[c] @ exp_so3(alpha(f, dt) * log_so3(S.rot_hat[c].T @ R))
    S.rot_raw[c] = R.copy()
    return S.rot_hat[c]


def step(S, pose, beta, cam, valid, sid, dt, cfg):
    """One frame of one hand-stream: fp32 inputs (16,3,3), (10), (3) -> fp32 outputs, ``S`` advanced."""
    usable = (valid is None or valid != 0) and bool(np.isfinite(pose).all() and np.isfinite(beta).all() and np.isfinite(cam).all())
    if not usable:
        S.live = False
        return pose.copy(), beta.copy(), cam.copy()
    if not (S.live and (sid is None or sid == S.id)):
        S.start(pose.astype(np.float64), beta.astype(np.float64), cam.astype(np.float64), sid)
        return pose.copy(), beta.copy(), cam.copy()
    mc, b, dc = cfg["min_cutoff"], cfg["beta"], cfg["d_cutoff"]
    P = np.stack([_rotation(S, c, pose[c].astype(np.float64), dt, mc[0], b[0], dc[0]) for c in range(16)])
    x = beta.astype(np.float64)
    if cfg["shape_mode"] == "filter":
        Bo = _vector(S.vec["shape"], x, dt, mc[1], b[1], dc[1])
    elif cfg["shape_mode"] == "mean":
        S.sum, S.n = S.sum + x, S.n + 1
        Bo = S.sum / S.n
    else:
        Bo = x
    Co = _vector(S.vec["cam"], cam.astype(np.float64), dt, mc[2], b[2], dc[2])
    return P.astype(np.float32), Bo.astype(np.float32), Co.astype(np.float32)


def smooth(pose, beta, cam, valid=None, seq=None, fps=30.0, steps=None, cfg=None, streams=None):
    """pose (B,16,3,3), beta (B,10), cam (B,3) fp32 with B = T * S rows, ``steps`` = T (default: B, one stream); valid (B) or None,
    seq (B) integers or None.  ``streams``: a list of S ``Stream`` carried from call to call, or None for a fresh start that
    keeps nothing.  -> the three smoothed fp32 arrays."""
    pose, beta, cam = (np.ascontiguousarray(a, dtype=np.float32) for a in (pose, beta, cam))
    B = pose.shape[0]
    T = B if steps is None else int(steps)
    assert T >= 1 and B % T == 0 and pose.shape == (B, 16, 3, 3) and beta.shape == (B, 10) and cam.shape == (B, 3)
    S = B // T
    cfg = cfg or config()
    streams = [Stream() for _ in range(S)] if streams is None else streams
    assert len(streams) == S
    dt = 1.0 / float(np.float32(fps))
    out = np.empty_like(pose), np.empty_like(beta), np.empty_like(cam)
    for t in range(T):
        for s in range(S):
            r = t * S + s
            res = step(streams[s], pose[r], beta[r], cam[r], None if valid is None else valid[r],
                       None if seq is None else int(seq[r]), dt, cfg)
            for o, v in zip(out, res):
                o[r] = v
    return out


# ---- inputs for the tests ----------------------------------------------------------------------------------------------------
def axis_rotation(axis, angle):
    axis = np.asarray(axis, np.float64)
    return exp_so3(axis / np.linalg.norm(axis) * angle)


def random_walk(rows, seed, lo=1e-3, hi=0.6):
    """(rows,16,3,3), (rows,10), (rows,3) fp32 of ONE stream: every rotation channel walks by relative angles in [lo, hi] rad about
    random axes (away from the branch thresholds of Log), the vectors drift."""
    rng = np.random.RandomState(seed)
    pose = np.empty((rows, 16, 3, 3))
    cur = np.stack([axis_rotation(rng.randn(3), rng.uniform(0.1, 2.0)) for _ in range(16)])
    for t in range(rows):
        if t:
            cur = np.stack([cur[c] @ axis_rotation(rng.randn(3), rng.uniform(lo, hi)) for c in range(16)])
        pose[t] = cur
    beta = np.cumsum(0.05 * rng.randn(rows, 10), 0) + rng.randn(10)
    cam = np.cumsum(0.02 * rng.randn(rows, 3), 0) + np.array([0.8, 0.1, -0.1])
    return pose.astype(np.float32), beta.astype(np.float32), cam.astype(np.float32)


def interleave(per_stream):
    """S arrays (T, ...) of single streams -> (T * S, ...) in the row order t * S + s."""
    return np.ascontiguousarray(np.stack(per_stream, 1).reshape((-1,) + per_stream[0].shape[1:]))


def streams_case(T, S, seed):
    parts = [random_walk(T, seed * 1000 + s) for s in range(S)]
    return tuple(interleave([p[i] for p in parts]) for i in range(3))


def jitter_case(T=64, fps=30.0, sigma=0.03, seed=0, axis=(0.0, 0.0, 1.0)):
    """One rotation channel following 0.5 sin(2 pi 0.5 t / fps) rad about a fixed axis, clean and with per-frame rotation noise
    of ``sigma`` rad: -> clean (T,3,3), noisy (T,3,3), fp64."""
    rng = np.random.RandomState(seed)
    clean = np.stack([axis_rotation(axis, 0.5 * math.sin(2.0 * math.pi * 0.5 * t / fps)) for t in range(T)])
    noisy = np.stack([clean[t] @ exp_so3(sigma * rng.randn(3)) for t in range(T)])
    return clean, noisy
