"""Temporal metrics on device (csrc/accel.hip): the acceleration error of a prediction over consecutive frames.

``accel_error`` is the reference's ``compute_error_accel`` (src/utils/eval_modules.py:508-534) with the validity window and the
NaN padding of ``eval_acc_pose`` (:537-622) folded in, plus a sequence rule the reference does not need because it scores one
sequence held in memory.  ``evaluate_accel_metrics`` gives ``acc/h`` -- the reference's key -- and eight more in one launch.
``AccelMetrics`` is the streaming form for predictions that arrive batch by batch: it carries the last two frames across the
batch border, so the values an epoch averages do not depend on the batch size.  tests/accel_ref.py restates all of it in fp64.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import AccelEvalOut, MeshEvalIn, check, ptr
from .xdict import xdict

# keys of evaluate_accel_metrics without the hand suffix, in the order of hands_accel_eval_out (_lib.ACCEL_QUANTITIES)
ACCEL_KEYS = ("acc", "acc/j", "acc/abs")
_PRED_KEYS = ("mano.v3d.cam.r", "mano.v3d.cam.l", "mano.j3d.cam.r", "mano.j3d.cam.l")
_FLAG_KEYS = ("is_valid", "right_valid", "left_valid")


def _seq_on_device(seq_id, T: int, dev):
    """``seq_id`` (T integers, tensor or sequence) as the int32 tensor the kernels compare: the index of the run of equal
    neighbours a frame lies in, which keeps "three adjacent frames carry the same id" for ids of any width."""
    if seq_id is None:
        return None
    s = torch.as_tensor(seq_id).to(dev)
    if s.is_floating_point() or s.dtype == torch.bool or s.shape != (T,):
        raise ValueError(f"hands_amd: seq_id is a ({T},) integer tensor, got {tuple(s.shape)} {s.dtype}")
    run = torch.zeros(T, dtype=torch.int32, device=dev)
    if T > 1:
        run[1:] = torch.cumsum((s[1:] != s[:-1]).to(torch.int32), dim=0)
    return run


def accel_error(gt, pred, valid=None, seq_id=None, fps=30.0) -> torch.Tensor:
    """Acceleration error of ``pred`` against ``gt``, both (T,N,D) with D in 1..3 holding T consecutive frames in order
    (hands_accel_error_f32, one launch): with ``a[t] = (x[t-1] - 2 x[t] + x[t+1]) fps^2``, row ``t`` of the (T) fp32 result is
    ``mean_n |a_pred[t,n] - a_gt[t,n]|`` in units per second squared, for ``1 <= t <= T-2``; rows 0 and T-1 are NaN.  Row ``t`` is
    also NaN when ``valid`` (T) is 0 in one of the frames t-1, t, t+1 or when ``seq_id`` (T integers) differs among them; no
    ``seq_id`` means one sequence.  fp32 inputs, fp64 arithmetic, one rounding.

    With D = 1 it scores a distance field over time, as the reference's ``eval_acc_field`` does::

        f_gt, f_pred = interhand_field(targets, faces), interhand_field(pred, faces)
        err = accel_error(f_gt["dist.rl"][..., None], f_pred["dist.rl"][..., None], valid=valid)
    """
    dev = pred.device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.accel_error runs on a HIP device only (no CPU fallback)")
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    gt, pred = f(gt), f(pred)
    assert pred.dim() == 3 and gt.shape == pred.shape, (gt.shape, pred.shape)
    T, N, D = pred.shape
    valid = None if valid is None else f(torch.as_tensor(valid))
    assert valid is None or valid.shape == (T,)
    seq = _seq_on_device(seq_id, T, dev)
    out = torch.empty(T, device=dev)
    check(_lib.lib().hands_accel_error_f32(ptr(gt), ptr(pred), ptr(valid), ptr(seq), ptr(out), T, N, D, float(fps),
                                           torch.cuda.current_stream(dev).cuda_stream), "hands_accel_error_f32")
    return out


def evaluate_accel_metrics(pred: dict, targets: dict, meta_info: dict | None = None, fps=30.0, seq_id=None) -> xdict:
    """Acceleration errors of both hands in one launch (hands_eval_accel_metrics_f32), metres per second squared, each a (T)
    tensor on the device of the inputs, the batch read as T consecutive frames: ``acc/*`` over the vertices and ``acc/j/*`` over
    the 21 joints, both root-relative, ``acc/abs/*`` over the joints in camera space, for ``* = r, l, h`` (``h`` the nanmean of
    the hands; ``acc/h`` is the reference's key).  Inputs as :func:`evaluate_mesh_metrics`.  Rows 0 and T-1 are NaN, as is every
    row whose three frames are not all valid for the hand or do not share a sequence id; the ids come from ``seq_id``, else from
    ``meta_info["seq_id"]``, else the call is one sequence."""
    dev = pred["mano.v3d.cam.r"].device
    if dev.type != "cuda":
        raise RuntimeError("hands_amd.evaluate_accel_metrics runs on a HIP device only (no CPU fallback)")
    L = _lib.lib()
    f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
    T, V = pred["mano.v3d.cam.r"].shape[:2]
    keep = [f(pred["mano.v3d.cam.r"]), f(pred["mano.v3d.cam.l"]), f(targets["mano.v3d.cam.r"]), f(targets["mano.v3d.cam.l"]),
            f(pred["mano.j3d.cam.r"]), f(pred["mano.j3d.cam.l"]), f(targets["mano.j3d.cam.r"]), f(targets["mano.j3d.cam.l"]),
            f(targets["is_valid"]), f(targets["right_valid"]), f(targets["left_valid"])]
    assert all(t.shape == (T, V, 3) for t in keep[:4]) and all(t.shape == (T, 21, 3) for t in keep[4:8])
    assert all(t.shape == (T,) for t in keep[8:])
    if seq_id is None and meta_info is not None and "seq_id" in meta_info:
        seq_id = meta_info["seq_id"]
    seq = _seq_on_device(seq_id, T, dev)
    buf = torch.empty(len(ACCEL_KEYS) * 3, T, device=dev)
    aout = AccelEvalOut(*[ptr(buf[i]) for i in range(buf.shape[0])])
    check(L.hands_eval_accel_metrics_f32(C.byref(MeshEvalIn(*[ptr(t) for t in keep])), ptr(seq), C.byref(aout), T, V, float(fps),
                                         torch.cuda.current_stream(dev).cuda_stream), "hands_eval_accel_metrics_f32")
    return xdict({f"{k}/{s}": buf[3 * i + j] for i, k in enumerate(ACCEL_KEYS) for j, s in enumerate("rlh")})


class AccelMetrics:
    """The acceleration errors of a stream of frames that arrives batch by batch, e.g. from ``HandsWrapper.forward(..., "test")``.

    ``update(pred, targets, meta_info=None, seq_id=None)`` takes a batch of B consecutive frames (the inputs of
    :func:`evaluate_accel_metrics`) and returns its nine keys as (B) rows.  Row ``i`` scores the window that ENDS at frame ``i``
    of the batch -- frames i-2, i-1, i of the running stream -- so every value is returned as soon as its last frame is there;
    the frames before the batch are the last two of the earlier calls, which the object keeps.  Before the first call they are two
    invalid frames, so the first two rows of a stream are NaN.  Over a whole stream the returned values are those of one call
    on the concatenated frames, moved down by one row, whatever the batch sizes were.

    ``seq_id`` (else ``meta_info["seq_id"]``) names the sequence of each frame: an integer tensor, taken as it is, or a list of B
    hashables such as ``os.path.dirname`` of each ``imgname``, which a dict kept across the calls maps to integers from 0.  Use
    one of the two forms in a stream.  Without ids a batch belongs to one unnamed sequence (id -1).  ``reset()`` forgets the kept
    frames and the dict.  ``evaluate`` is the one-shot function the bookkeeping stands on."""

    def __init__(self, fps=30.0, evaluate=evaluate_accel_metrics):
        self.fps, self.evaluate = fps, evaluate
        self.reset()

    def reset(self):
        self._kept = None                               # (pred, targets, ids) of the last two frames
        self._names = {}

    def _ids(self, seq_id, B, dev):
        if seq_id is None:
            return torch.full((B,), -1, dtype=torch.int64, device=dev)
        if isinstance(seq_id, torch.Tensor):
            ids = seq_id.to(device=dev, dtype=torch.int64)
        else:
            ids = torch.tensor([self._names.setdefault(s, len(self._names)) for s in seq_id], dtype=torch.int64, device=dev)
        assert ids.shape == (B,), (ids.shape, B)
        return ids

    def update(self, pred, targets, meta_info=None, seq_id=None) -> xdict:
        if seq_id is None and meta_info is not None and "seq_id" in meta_info:
            seq_id = meta_info["seq_id"]
        dev = pred["mano.v3d.cam.r"].device
        B = pred["mano.v3d.cam.r"].shape[0]
        p = {k: pred[k].detach() for k in _PRED_KEYS}
        t = {k: targets[k].detach().to(dev) for k in _PRED_KEYS + _FLAG_KEYS}
        ids = self._ids(seq_id, B, dev)
        if self._kept is None:                          # two invalid frames
            zero = lambda x: x.new_zeros((2,) + tuple(x.shape[1:]))
            self._kept = ({k: zero(v) for k, v in p.items()}, {k: zero(v) for k, v in t.items()}, ids.new_full((2,), -1))
        kp, kt, kid = self._kept
        p = {k: torch.cat([kp[k].to(v.dtype), v]) for k, v in p.items()}
        t = {k: torch.cat([kt[k].to(v.dtype), v]) for k, v in t.items()}
        ids = torch.cat([kid, ids])
        out = self.evaluate(p, t, meta_info, fps=self.fps, seq_id=ids)
        last = lambda x: x[-2:].clone()                 # a copy: a view would hold the whole batch
        self._kept = ({k: last(v) for k, v in p.items()}, {k: last(v) for k, v in t.items()}, last(ids))
        return xdict({k: v[1:B + 1] for k, v in out.items()})
