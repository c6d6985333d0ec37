"""Temporal smoothing on device (csrc/smooth.hip): the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) over the MANO parameters
a model regresses frame by frame -- ``mano.pose`` filtered on SO(3), ``mano.beta`` and ``mano.cam_t.wp`` as vectors -- and the
re-posing of the smoothed parameters with the fused MANO head, so that the result is a consistent model output again.

The reference has no smoother: DESIGN.md section 7 "Temporal smoothing" is the specification and tests/smooth_ref.py its fp64
restatement.  Rows are T time steps of S parallel streams, row ``t * S + s``: a batch of consecutive frames of one video is
``T = B, S = 1`` (``layout="time"``), one frame from each of B cameras ``T = 1, S = B`` (``layout="streams"``).  Nothing here
synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib
from ._lib import SMOOTH_SHAPE_MODES, SmoothCfg, SmoothSide, check, ptr
from .mano_head import run_mano_heads
from .xdict import xdict

# the keys the MANO head computes, per hand; every other key of a prediction passes through smooth_predictions untouched
HEAD_KEYS = ("cam_t.wp", "cam_t", "joints3d", "vertices", "j3d.cam", "v3d.cam", "j2d.norm", "beta", "pose")
LAYOUTS = ("time", "streams")


@dataclass(frozen=True)
class SmoothConfig:
    """The nine numbers of the filter and the shape mode.  ``min_cutoff`` (Hz) is the cutoff of a channel at rest, ``beta`` how
    fast the cutoff grows with the filtered speed of the channel (rad/s for rotations, units/s for the vectors), ``d_cutoff``
    (Hz) the cutoff of that speed estimate; each is (rotations, shape, camera), a scalar standing for all three.
    ``shape_mode``: ``"filter"`` (the same filter), ``"mean"`` (the running mean since the stream started: a hand's shape does
    not change within a video) or ``"none"`` (pass through).

    The defaults (1.5, 0.5, 1.0, "filter") are starting values and NOT tuned on data -- no video data was available.  On a
    synthetic rotation channel (0.5 sin(2 pi 0.5 t) rad, noise of 0.03 rad a frame, 30 fps) they cut the acceleration error about
    five-fold, at the cost of lag."""
    min_cutoff: tuple | float = 1.5
    beta: tuple | float = 0.5
    d_cutoff: tuple | float = 1.0
    shape_mode: str = "filter"

    def c_struct(self) -> SmoothCfg:
        if self.shape_mode not in SMOOTH_SHAPE_MODES:
            raise ValueError(f"hands_amd: shape_mode is one of {tuple(SMOOTH_SHAPE_MODES)}, got {self.shape_mode!r}")
        three = lambda v: (C.c_double * 3)(*([float(x) for x in v] if isinstance(v, (tuple, list)) else [float(v)] * 3))
        return SmoothCfg(three(self.min_cutoff), three(self.beta), three(self.d_cutoff), SMOOTH_SHAPE_MODES[self.shape_mode])


def smooth_state(sides: int, streams: int, device) -> torch.Tensor:
    """A fresh (all zero) state of ``sides`` x ``streams`` hand-streams: opaque, to be handed to consecutive calls."""
    return torch.zeros(sides, streams, _lib.lib().hands_smooth_state_bytes() // 8, dtype=torch.int64, device=device)


def _device_of(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"hands_amd.{what} runs on a HIP device only (no CPU fallback)")
    return t.device


def _flags(v, B, dev):
    if v is None:
        return None
    v = torch.as_tensor(v).to(device=dev, dtype=torch.float32).contiguous()
    assert v.shape == (B,), (v.shape, B)
    return v


def _seq(seq_id, B, dev):
    if seq_id is None:
        return None
    s = torch.as_tensor(seq_id).to(dev)
    if s.is_floating_point() or s.dtype == torch.bool or s.shape != (B,):
        raise ValueError(f"hands_amd: seq_id is a ({B},) integer tensor, got {tuple(s.shape)} {s.dtype}")
    return s.to(torch.int64).contiguous()


def _launch(hands, outs, valids, seq, T, S, fps, config, state, dev):
    """hands / outs: per side (pose, beta, cam) contiguous fp32 tensors of T * S rows; state (sides, S, words) or None."""
    n = len(hands)
    if state is not None:
        assert state.dtype == torch.int64 and state.is_contiguous() and state.device == dev, "a state of smooth_state()"
        assert tuple(state.shape) == (n, S, _lib.lib().hands_smooth_state_bytes() // 8), (tuple(state.shape), n, S)
    sides = (SmoothSide * n)()
    for i, (h, o, v) in enumerate(zip(hands, outs, valids)):
        sides[i] = SmoothSide(ptr(h[0]), ptr(h[1]), ptr(h[2]), ptr(v), ptr(o[0]), ptr(o[1]), ptr(o[2]),
                              None if state is None else ptr(state[i]))
    cfg = (config or SmoothConfig()).c_struct()
    check(_lib.lib().hands_smooth_mano_f32(sides, n, ptr(seq), T, S, float(fps), C.byref(cfg),
                                           torch.cuda.current_stream(dev).cuda_stream), "hands_smooth_mano_f32")


def _inputs(pose, beta, cam, dev):
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    pose, beta, cam = f(pose), f(beta), f(cam)
    B = pose.shape[0]
    assert pose.shape == (B, 16, 3, 3) and beta.shape == (B, 10) and cam.shape == (B, 3), (pose.shape, beta.shape, cam.shape)
    return pose, beta, cam, B


def smooth_mano_params(pose, beta, cam, valid=None, seq_id=None, fps=30.0, steps=None, config=None, state=None):
    """The filter over the parameters of ONE hand (hands_smooth_mano_f32, one launch): pose (B,16,3,3) rotation matrices, beta
    (B,10), cam (B,3), rows being ``steps`` = T time steps of S = B / T parallel streams (default T = B: consecutive frames of one
    video).  Returns the three smoothed fp32 tensors.  A frame with ``valid`` (B) 0 or a non-finite input passes through bit for
    bit and restarts its stream, as does the first frame of another ``seq_id`` (B integers).  ``state``: ``smooth_state(1, S,
    device)``, carried from call to call -- a stream filtered in any split into calls gives the bits of one call; without it
    the call starts fresh and keeps nothing.  ``config``: a :class:`SmoothConfig` (its defaults are untuned starting values)."""
    dev = _device_of(pose, "smooth_mano_params")
    pose, beta, cam, B = _inputs(pose, beta, cam, dev)
    T = B if steps is None else int(steps)
    if T < 1 or B % T:
        raise ValueError(f"hands_amd: steps = {T} does not divide the {B} rows")
    outs = (torch.empty_like(pose), torch.empty_like(beta), torch.empty_like(cam))
    _launch([(pose, beta, cam)], [outs], [_flags(valid, B, dev)], _seq(seq_id, B, dev), T, B // T, fps, config, state, dev)
    return outs


def smooth_predictions(pred, model, meta_info, fps=30.0, valid_r=None, valid_l=None, seq_id=None, layout="time", config=None,
                       state=None) -> xdict:
    """A model's prediction dict with its MANO parameters smoothed over the batch and everything that follows from them
    recomputed: one filter launch for both hands, written into the right-then-left buffers of the MANO head, then one launch of
    the fused MANO head (hands_mano_heads_f32) with ``meta_info["intrinsics"]`` and the assets and ``img_res`` of ``model``
    (HandsLight, HAMER or HandOccNet).  Returns an xdict with the keys of ``pred`` in their order: the nine ``mano.*`` keys a
    hand's MANO head gives are new, every other key (``mano.cam_t.wp.init.*``, ``grasp.*``, ``depth.*``, ``center.*``,
    ``corner.*``) is the tensor of ``pred``.  ``layout="time"``: the B rows are consecutive frames of one video;
    ``"streams"``: one frame of each of B videos.  ``valid_r`` / ``valid_l`` (B), ``seq_id`` (B integers, else
    ``meta_info["seq_id"]``) and ``config`` as in :func:`smooth_mano_params`; ``state`` is ``smooth_state(2, S, device)``."""
    if layout not in LAYOUTS:
        raise ValueError(f"hands_amd: layout is one of {LAYOUTS}, got {layout!r}")
    dev = _device_of(pred["mano.pose.r"], "smooth_predictions")
    hands = [_inputs(pred[f"mano.pose.{h}"], pred[f"mano.beta.{h}"], pred[f"mano.cam_t.wp.{h}"], dev) for h in "rl"]
    B = hands[0][3]
    assert hands[1][3] == B
    T, S = (B, 1) if layout == "time" else (1, B)
    if seq_id is None and meta_info is not None and "seq_id" in meta_info:
        seq_id = meta_info["seq_id"]
    rot, shape, cam = torch.empty(2 * B, 16, 3, 3, device=dev), torch.empty(2 * B, 10, device=dev), torch.empty(2 * B, 3, device=dev)
    outs = [(rot[i * B:(i + 1) * B], shape[i * B:(i + 1) * B], cam[i * B:(i + 1) * B]) for i in range(2)]
    _launch([h[:3] for h in hands], outs, [_flags(valid_r, B, dev), _flags(valid_l, B, dev)], _seq(seq_id, B, dev), T, S, fps,
            config, state, dev)
    K = meta_info["intrinsics"].to(device=dev, dtype=torch.float32).contiguous()
    P = model.packed(dev)
    new = run_mano_heads(_lib.lib(), P["mano_r"], P["mano_l"], rot, shape, cam, cam, K, float(model.img_res), B,
                         torch.cuda.current_stream(dev).cuda_stream, None)
    head = {f"mano.{k}.{h}" for k in HEAD_KEYS for h in "rl"}
    return xdict({k: (new[k] if k in head else v) for k, v in pred.items()})


class TemporalSmoother:
    """:func:`smooth_predictions` over a stream of predictions that arrives call by call, the filter state kept on the device in
    between: ``update(pred, meta_info, valid_r=None, valid_l=None, seq_id=None)`` returns the smoothed dict of the batch, and
    what it returns over a stream does not depend on how the stream was cut into batches (``layout="time"``).  With
    ``layout="streams"`` every call brings one frame of each of B videos, and B must not change.  ``seq_id`` (else
    ``meta_info["seq_id"]``) is an integer tensor, taken as it is, or a list of B hashables such as ``os.path.dirname`` of each
    ``imgname``, which a dict kept across the calls maps to integers from 0; use one of the two forms in a stream.
    ``reset()`` forgets state and dict.  ``config`` defaults to :class:`SmoothConfig`, whose numbers are untuned starting
    values."""

    def __init__(self, model, fps=30.0, layout="time", config=None):
        if layout not in LAYOUTS:
            raise ValueError(f"hands_amd: layout is one of {LAYOUTS}, got {layout!r}")
        self.model, self.fps, self.layout, self.config = model, fps, layout, config
        self.reset()

    def reset(self):
        self._state = None
        self._names = {}

    def _ids(self, seq_id, dev):
        if seq_id is None or isinstance(seq_id, torch.Tensor):
            return seq_id
        return torch.tensor([self._names.setdefault(s, len(self._names)) for s in seq_id], dtype=torch.int64, device=dev)

    def update(self, pred, meta_info, valid_r=None, valid_l=None, seq_id=None) -> xdict:
        if seq_id is None and meta_info is not None and "seq_id" in meta_info:
            seq_id = meta_info["seq_id"]
        dev = _device_of(pred["mano.pose.r"], "TemporalSmoother")
        B = pred["mano.pose.r"].shape[0]
        S = 1 if self.layout == "time" else B
        if self._state is None:
            self._state = smooth_state(2, S, dev)
        elif self._state.shape[1] != S:
            raise ValueError(f"hands_amd.TemporalSmoother: layout 'streams' was started with {self._state.shape[1]} streams, "
                             f"this batch has {S}")
        return smooth_predictions(pred, self.model, meta_info, self.fps, valid_r, valid_l, self._ids(seq_id, dev), self.layout,
                                  self.config, self._state)
