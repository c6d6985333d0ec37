"""hands_smooth_mano_f32 and what stands on it (hands_amd/smoothing.py, ``smoother`` in HandsWrapper) on the device against the
fp64 restatement (tests/smooth_ref.py) of DESIGN.md section 7 "Temporal smoothing".

Bars.  The kernel computes in fp64 what the restatement computes and rounds once to fp32.  The two differ by device-versus-host
libm (sincos, atan2, sqrt) and by the order of a few fp64 sums over T <= 64 steps of a contracting recurrence: orders below
2^-24.  Rotation entries, which are at most 1: 4 * 2^-24 absolute.  Vectors: 4 * 2^-24 |ref| + 1e-12.  That is the fourfold
margin of tests/test_gpu_accel_metrics.py.  A row the restatement passes through is the input bit for bit.

Inputs.  Parity inputs keep the relative angle of consecutive frames in [1e-3, 0.6] rad (smooth_ref.random_walk), or exactly 0,
or exactly pi (signed permutations, exact in fp32), away from the branch thresholds of Log and Exp.
"""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import smooth_ref as SR
from edge_util import In, Out
from hands_amd._lib import ptr
from test_smoothing import SPLITS9, bits, eye_pose, one_channel

pytestmark = pytest.mark.gpu

UNWRITTEN = 123.0
BAR = 4 * 2.0 ** -24
STATE_SENT = -0x0123456789ABCDEF
I64 = np.iinfo(np.int64)
SHAPES = ((16, 3, 3), (10,), (3,))
NONDEFAULT = dict(min_cutoff=(0.7, 2.5, 1.1), beta=(1.3, 0.0, 0.05), d_cutoff=(2.0, 0.6, 1.5))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cfg(cfg):
    import hands_amd
    cfg = cfg or SR.config()
    return hands_amd.SmoothConfig(cfg["min_cutoff"], cfg["beta"], cfg["d_cutoff"], cfg["shape_mode"])


def close(what, got, ref, inputs):
    """got / ref / inputs: (pose, beta, cam).  Rows the restatement passes through are the input bits; the rest is inside the
    bar.  Prints the narrowest margin."""
    worst = 0.0
    for i, (g, r, x) in enumerate(zip(got, ref, inputs)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == np.float32 and g.shape == r.shape, (what, i, g.shape, r.shape)
        rows = r.shape[0]
        passed = (bits(r).reshape(rows, -1) == bits(x).reshape(rows, -1)).all(1)
        assert np.array_equal(bits(g)[passed], bits(x)[passed]), (what, i, "a passed-through row is not the input bits")
        fin = np.isfinite(r)
        assert fin[~passed].all(), (what, i)
        err = np.abs(g[~passed].astype(np.float64) - r[~passed])
        bnd = np.full(err.shape, BAR) if i == 0 else BAR * np.abs(r[~passed].astype(np.float64)) + 1e-12
        if err.size:
            worst = max(worst, float((err / bnd).max()))
        assert (err <= bnd).all(), (what, i, float((err / bnd).max()))
    print(f"SMOOTH|{what}|{worst:.3f} of the bar")


class GuardedState:
    """A zeroed state of `sides` x `S` streams between two bands of sentinel words."""
    PAD = 64

    def __init__(self, sides, S):
        from hands_amd import _lib
        self.words = _lib.lib().hands_smooth_state_bytes() // 8
        self.n = sides * S * self.words
        self.buf = torch.full((2 * self.PAD + self.n,), STATE_SENT, dtype=torch.int64, device="cuda")
        self.body = self.buf[self.PAD:self.PAD + self.n].view(sides, S, self.words)
        self.body.zero_()

    def get(self):
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert bool((h[:self.PAD] == STATE_SENT).all()) and bool((h[self.PAD + self.n:] == STATE_SENT).all()), "wrote around the state"
        return h[self.PAD:self.PAD + self.n].clone()


def c_smooth(hands, valids, seq, T, S, fps=30.0, cfg=None, state=None):
    """hands_smooth_mano_f32 on guarded buffers: hands = per side (pose, beta, cam) numpy of T * S rows -> per side the three
    outputs as numpy."""
    from hands_amd import _lib
    rows = T * S
    n = len(hands)
    ins = [[In(torch.from_numpy(a), lead=4 * (k + 1)) for k, a in enumerate(h)] for h in hands]
    vs = [None if v is None else In(torch.from_numpy(np.float32(v))) for v in valids]
    outs = [[Out(rows, *shp, init=torch.full((rows,) + shp, UNWRITTEN)) for shp in SHAPES] for _ in hands]
    s = None if seq is None else torch.from_numpy(np.asarray(seq, np.int64)).cuda()
    sides = (_lib.SmoothSide * n)()
    for i in range(n):
        sides[i] = _lib.SmoothSide(ins[i][0].ptr(), ins[i][1].ptr(), ins[i][2].ptr(), None if vs[i] is None else vs[i].ptr(),
                                   outs[i][0].ptr(), outs[i][1].ptr(), outs[i][2].ptr(),
                                   None if state is None else ptr(state.body[i]))
    c = _cfg(cfg).c_struct()
    rc = _lib.lib().hands_smooth_mano_f32(sides, n, ptr(s), T, S, fps, ctypes.byref(c), _stream())
    assert rc == 0, rc
    res = [[o.get().numpy() for o in side] for side in outs]                  # get() checks the bands
    for side in res:
        for o in side:
            assert not (o == UNWRITTEN).any(), "an element was left unwritten"
    if state is not None:
        state.get()
    return res


# ---- 1. the entry through the C ABI --------------------------------------------------------------------------------------------
ENTRY = ((1, 1), (2, 1), (5, 1), (9, 1), (1, 3), (3, 2), (4, 65))
_cases = {}


def entry_case(T, S):
    """Inputs, flags and the restatement's outputs of an entry case, computed once: -> hands, valids, seq, fps, {label: (cfg, refs)}."""
    if (T, S) in _cases:
        return _cases[T, S]
    rows = T * S
    hands = [SR.streams_case(T, S, 10 * T + S + h) for h in range(2)]
    valids, seq = [None, None], None
    if (T, S) == (9, 1):
        # right: start, go, invalid, start, go, NaN, start, start (the id changes), go
        # left:  start, go, go, Inf, start, go, go, start (the id changes), go
        valids[0] = np.ones(rows, np.float32)
        valids[0][2] = 0
        hands[0][0][5, 3, 1, 2] = np.nan
        hands[1][2][3, 1] = np.inf
        seq = np.array([I64.min] * 7 + [I64.max] * 2, np.int64)
    elif rows > 2:
        valids[1] = np.ones(rows, np.float32)
        valids[1][rows // 2] = 0
        if rows % 2 == 0:
            seq = np.array([(7 * s if t < T - 1 or s != 1 else -1) for t in range(T) for s in range(S)], np.int64)
    fps = 30.0 if T % 2 else 60.0
    cfgs = {"default": SR.config(), "mean": SR.config(shape_mode="mean", **NONDEFAULT), "none": SR.config(shape_mode="none")}
    refs = {k: (c, [SR.smooth(*h, valid=v, seq=seq, fps=fps, steps=T, cfg=c) for h, v in zip(hands, valids)]) for k, c in cfgs.items()}
    _cases[T, S] = hands, valids, seq, fps, refs
    return _cases[T, S]


@pytest.mark.parametrize("nsides", (1, 2))
@pytest.mark.parametrize("T,S", ENTRY)
def test_entry_against_the_restatement(T, S, nsides):
    hands, valids, seq, fps, refs = entry_case(T, S)
    for label, (cfg, ref) in refs.items():
        calls = [[0], [1]] if nsides == 1 else [[0, 1]]                           # one side at a time: each side's data in turn
        for which in calls:
            got = c_smooth([hands[i] for i in which], [valids[i] for i in which], seq, T, S, fps, cfg)
            for g, i in zip(got, which):
                close(f"entry T{T} S{S} n{nsides} {label} side{i}", g, ref[i], hands[i])
    if (T, S) == (9, 1):
        ref = refs["default"][1]
        passed = lambda r, x: (bits(r).reshape(9, -1) == bits(x).reshape(9, -1)).all(1).tolist()
        assert passed(ref[0][0], hands[0][0]) == [True, False, True, True, False, True, True, True, False]
        assert passed(ref[1][2], hands[1][2]) == [True, False, False, True, True, False, False, True, False]


# ---- 2. half turns -------------------------------------------------------------------------------------------------------------
def test_half_turn_between_consecutive_frames():
    swap, swap_neg = np.float32([[0, 1, 0], [1, 0, 0], [0, 0, -1]]), np.float32([[0, -1, 0], [-1, 0, 0], [0, 0, -1]])
    turns = [np.diag(np.float32([1, -1, -1])), np.diag(np.float32([-1, 1, -1])), np.diag(np.float32([-1, -1, 1])), swap, swap_neg]
    T = 4
    pose = eye_pose(T)
    for c, D in enumerate(turns):                                 # identity, then the half turn, held
        pose[1:, c] = D
    pose[1:, 5] = turns[3] @ turns[0]                             # a quarter turn about z beside them
    beta, cam = np.zeros((T, 10), np.float32), np.zeros((T, 3), np.float32)
    ref = SR.smooth(pose, beta, cam)
    got = c_smooth([(pose, beta, cam)], [None], None, T, 1)[0]
    close("half turn", got, ref, (pose, beta, cam))
    R = got[0].astype(np.float64)
    assert np.isfinite(R).all()
    assert np.abs(np.einsum("tcji,tcjk->tcik", R, R) - np.eye(3)).max() <= 1e-6
    assert not np.array_equal(got[0][1, :5], pose[1, :5])          # it moved towards the half turn: not there, not at rest
    assert not np.array_equal(got[0][1, :5], pose[0, :5])


# ---- 3. constant input ---------------------------------------------------------------------------------------------------------
def signed_permutations():
    """The 24 proper signed permutation matrices."""
    out = []
    for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in range(8):
            M = np.zeros((3, 3), np.float32)
            for i in range(3):
                M[i, p[i]] = -1.0 if sg >> i & 1 else 1.0
            if np.linalg.det(M) > 0:
                out.append(M)
    return out


def test_constant_input_returns_the_input_bits():
    perms = signed_permutations()
    assert len(perms) == 24
    T = 6
    for first in (0, 8):
        pose = np.tile(np.stack(perms[first:first + 16])[None], (T, 1, 1, 1))
        beta = np.tile(np.float32(np.linspace(-2.0, 2.0, 10)), (T, 1))
        cam = np.tile(np.float32([0.83, -0.21, 0.37]), (T, 1))
        for mode in SR.SHAPE_MODES[::2]:
            got = c_smooth([(pose, beta, cam)], [None], None, T, 1, cfg=SR.config(shape_mode=mode))[0]
            for g, x in zip(got, (pose, beta, cam)):
                assert np.array_equal(bits(g), bits(x)), (first, mode)


# ---- 4. streaming through the state buffer -------------------------------------------------------------------------------------
def run_in_calls(hands, valids, seq, split, S, cfg=None, with_state=True):
    state = GuardedState(len(hands), S) if with_state else None
    parts, at = [], 0
    for n in split:
        sl = slice(at * S, (at + n) * S)
        parts.append(c_smooth([tuple(a[sl] for a in h) for h in hands], [None if v is None else v[sl] for v in valids],
                              None if seq is None else seq[sl], n, S, cfg=cfg, state=state))
        at += n
    outs = [[np.concatenate([p[i][k] for p in parts]) for k in range(3)] for i in range(len(hands))]
    return outs, (state.get() if with_state else None)


def test_any_split_into_calls_gives_the_same_bits():
    T = 9
    hands = [SR.random_walk(T, 40 + h) for h in range(2)]
    valids = [np.ones(T, np.float32), None]
    valids[0][3] = 0
    seq = np.array([2, 2, 2, 2, 2, 2, 9, 9, 9], np.int64)
    for mode in SR.SHAPE_MODES[:2]:
        cfg = SR.config(shape_mode=mode)
        one, state_one = run_in_calls(hands, valids, seq, (T,), 1, cfg)
        assert bool((state_one != 0).any())
        for split in SPLITS9[1:]:
            got, state = run_in_calls(hands, valids, seq, split, 1, cfg)
            for i in range(2):
                for g, o in zip(got[i], one[i]):
                    assert np.array_equal(bits(g), bits(o)), (mode, split, i)
            assert torch.equal(state, state_one), (mode, split)
        fresh, _ = run_in_calls(hands, valids, seq, (T,), 1, cfg, with_state=False)       # NULL: a zero-initialised state
        for i in range(2):
            for g, o in zip(fresh[i], one[i]):
                assert np.array_equal(bits(g), bits(o)), (mode, i)
        ref = [SR.smooth(*h, valid=v, seq=seq, cfg=cfg) for h, v in zip(hands, valids)]
        for i in range(2):
            close(f"stream split {mode} side{i}", one[i], ref[i], hands[i])


def test_65_streams_in_two_calls():
    T, S = 4, 65
    hands, _, _, _, refs = entry_case(T, S)
    cfg, ref = refs["mean"]
    one, state_one = run_in_calls(hands[:1], [None], None, (T,), S, cfg)
    two, state_two = run_in_calls(hands[:1], [None], None, (2, 2), S, cfg)
    for g, o in zip(two[0], one[0]):
        assert np.array_equal(bits(g), bits(o))
    assert torch.equal(state_one, state_two)
    frames, state_frames = run_in_calls(hands[:1], [None], None, (1,) * T, S, cfg)         # the "streams" layout: T = 1 a call
    for g, o in zip(frames[0], one[0]):
        assert np.array_equal(bits(g), bits(o))
    assert torch.equal(state_one, state_frames)


def test_smooth_mano_params():
    import hands_amd
    from hands_amd.smoothing import smooth_state
    T, S = 3, 2
    hands, valids, seq, fps, refs = entry_case(T, S)
    cfg, ref = refs["mean"]
    x = [_cuda(a) for a in hands[1]]
    got = hands_amd.smooth_mano_params(*x, valid=_cuda(valids[1]), seq_id=seq.tolist(), fps=fps, steps=T, config=_cfg(cfg))
    close("smooth_mano_params", got, ref[1], hands[1])
    state = smooth_state(1, S, "cuda")
    parts = [hands_amd.smooth_mano_params(*(a[t * S:(t + 1) * S] for a in x), valid=_cuda(valids[1][t * S:(t + 1) * S]),
                                          seq_id=torch.from_numpy(seq[t * S:(t + 1) * S]), fps=fps, steps=1, config=_cfg(cfg), state=state)
             for t in range(T)]
    for k in range(3):
        assert torch.equal(torch.cat([p[k] for p in parts]).view(torch.int32), got[k].view(torch.int32)), k
    one = SR.random_walk(5, 3)                                                             # the default layout: T = B
    close("smooth_mano_params T = B", hands_amd.smooth_mano_params(*[_cuda(a) for a in one]), SR.smooth(*one), one)
    with pytest.raises(ValueError):
        hands_amd.smooth_mano_params(*x, steps=4)


# ---- 5. smooth_predictions on a real forward -----------------------------------------------------------------------------------
BZ = 4
PARAMS = ("pose", "beta", "cam_t.wp")


@pytest.fixture(scope="module")
def forward(recipe_model):
    from hands_amd.weights import synthetic_inputs
    model = copy.deepcopy(recipe_model).to("cuda")
    inputs, meta = synthetic_inputs(BZ, 3, device="cuda")
    pred = model(inputs, meta)
    dict(pred)                                                    # join the tail's stream
    torch.cuda.synchronize()
    return model, inputs, meta, pred


def _params(d, h, rows=slice(None)):
    return tuple(d[f"mano.{k}.{h}"][rows].detach().cpu().numpy() for k in PARAMS)


def _same(a, b, keys=None):
    for k in (keys or a.keys()):
        assert a[k].shape == b[k].shape and torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_smooth_predictions_on_a_forward(forward):
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import run_mano_heads
    from hands_amd.smoothing import HEAD_KEYS
    model, _, meta, pred = forward
    assert len(pred) == 22
    out = hands_amd.smooth_predictions(pred, model, meta)
    assert list(out) == list(pred) and isinstance(out, hands_amd.xdict)
    for h in "rl":
        x = _params(pred, h)
        close(f"smooth_predictions {h}", _params(out, h), SR.smooth(*x), x)
        assert not torch.equal(out[f"mano.pose.{h}"][1:], pred[f"mano.pose.{h}"][1:])
    head = [f"mano.{k}.{h}" for h in "rl" for k in HEAD_KEYS]
    for k in pred:
        assert (k in head) or out[k] is pred[k], k                # every other key is the tensor of pred
    assert len(head) == 18 and set(pred) - set(head) == {"mano.cam_t.wp.init.r", "mano.cam_t.wp.init.l", "grasp.r", "grasp.l"}
    cat = lambda k: torch.cat([out[f"mano.{k}.r"], out[f"mano.{k}.l"]]).contiguous()
    P = model.packed(torch.device("cuda", torch.cuda.current_device()))
    by_hand = run_mano_heads(_lib.lib(), P["mano_r"], P["mano_l"], cat("pose"), cat("beta"), cat("cam_t.wp"), cat("cam_t.wp"),
                             meta["intrinsics"].contiguous(), float(model.img_res), BZ, _stream(), None)
    _same(out, by_hand, head)
    assert not torch.equal(out["mano.vertices.r"], pred["mano.vertices.r"])
    # every frame its own sequence: the filter is the identity, and the re-posing gives the model's own bits
    _same(hands_amd.smooth_predictions(pred, model, meta, seq_id=torch.arange(BZ)), pred)
    _same(hands_amd.smooth_predictions(pred, model, dict(meta, seq_id=torch.arange(BZ).cuda())), pred)
    _same(hands_amd.smooth_predictions(pred, model, meta, layout="streams"), pred)            # a first frame of B streams
    # validity per hand: an invalid right frame passes through and restarts the right hand only
    flagged = hands_amd.smooth_predictions(pred, model, meta, valid_r=torch.tensor([1.0, 1.0, 0.0, 1.0]))
    x = _params(pred, "r")
    close("smooth_predictions valid_r", _params(flagged, "r"), SR.smooth(*x, valid=np.float32([1, 1, 0, 1])), x)
    _same(flagged, out, [k for k in head if k.endswith(".l")])
    with pytest.raises(ValueError):
        hands_amd.smooth_predictions(pred, model, meta, layout="frames")


def test_temporal_smoother(forward):
    import hands_amd
    model, _, meta, pred = forward
    whole = hands_amd.smooth_predictions(pred, model, meta)
    cut = lambda d, sl: {k: (v[sl] if torch.is_tensor(v) else v) for k, v in d.items()}
    sm = hands_amd.TemporalSmoother(model)

    def in_two(ids=None):
        parts = [sm.update(cut(pred, sl), cut(meta, sl), seq_id=None if ids is None else ids[sl]) for sl in (slice(0, 2), slice(2, 4))]
        return {k: torch.cat([p[k] for p in parts]) for k in whole}
    _same(in_two(), whole)                                         # bz 2 + 2 is bz 4
    again = in_two()                                               # the stream goes on: its first frame is filtered now
    assert not torch.equal(again["mano.pose.r"][0], pred["mano.pose.r"][0])
    sm.reset()
    _same(in_two(), whole)
    # ids as path strings and as integers
    ints = torch.tensor([0, 0, 1, 1])
    by_int = hands_amd.smooth_predictions(pred, model, meta, seq_id=ints)
    assert torch.equal(by_int["mano.pose.l"][2], pred["mano.pose.l"][2])
    sm.reset()
    _same(in_two(["a/x", "a/x", "b/y", "b/y"]), by_int)
    sm.reset()
    _same(in_two(ints), by_int)
    # one frame of each of B cameras per call
    cams = hands_amd.TemporalSmoother(model, layout="streams")
    _same(cams.update(pred, meta), pred)
    second = cams.update(pred, meta)                               # the same frames again: a constant stream
    for h in "rl":
        x = tuple(np.concatenate([a, a]) for a in _params(pred, h))
        ref = SR.smooth(*x, steps=2)
        close(f"TemporalSmoother streams {h}", _params(second, h), tuple(r[BZ:] for r in ref), tuple(a[BZ:] for a in x))
    with pytest.raises(ValueError):
        cams.update(cut(pred, slice(0, 2)), cut(meta, slice(0, 2)))


# ---- 6. the wrapper ------------------------------------------------------------------------------------------------------------
def test_wrapper_smoother(golden_dir, forward):
    import hands_amd
    from hands_amd.weights import synthetic_inputs
    from hands_amd.wrapper import HandsWrapper
    model = forward[0]
    B = 3
    d = np.load(os.path.join(golden_dir, "process_data.npz"))
    tin = {k[3:]: torch.from_numpy(d[k])[:B] for k in d.files if k.startswith("in/")}
    K = tin.pop("intrinsics")
    targets = {k: v.cuda() for k, v in tin.items()}
    g = torch.Generator().manual_seed(1)
    for h in "rl":
        targets[f"mano.j2d.norm.{h}"] = (0.5 * torch.randn(B, 21, 2, generator=g)).cuda()
        targets[f"joints_valid_{h}"] = torch.ones(B, 21).cuda()
    targets.update(is_valid=torch.ones(B).cuda(), right_valid=torch.tensor([1.0, 0.0, 1.0]).cuda(), left_valid=torch.ones(B).cuda())
    calls = []
    for seed in (4, 5):
        inputs, meta = synthetic_inputs(B, seed, device="cuda")
        meta["intrinsics"] = K.cuda()
        meta["imgname"] = [f"{seed}/{i}.jpg" for i in range(B)]
        calls.append((inputs, meta))
    w = HandsWrapper(model=model)
    assert w.smoother is None

    def by_hand(inputs, meta, smoother):
        """What forward(..., "test") does, driven from outside."""
        t, m = w.process_data(hands_amd.xdict(dict(targets)), hands_amd.xdict(meta)), hands_amd.xdict(meta)
        m.overwrite("mano.faces.r", w.model.mano_r.faces)
        m.overwrite("mano.faces.l", w.model.mano_l.faces)
        pred = w.model(inputs, m)
        if smoother is not None:
            pred = smoother.update(pred, m, valid_r=t["right_valid"] * t["is_valid"], valid_l=t["left_valid"] * t["is_valid"])
        for key in [k for k in pred if "2d.norm" in k]:
            pred[key.replace(".norm", "")] = w._unnormalize(pred[key])
            t[key.replace(".norm", "")] = w._unnormalize(t[key])
        return hands_amd.evaluate_metrics(pred, t, m).detach(), pred

    plain = [w.forward(inputs, dict(targets), meta, "test")[0] for inputs, meta in calls]
    for (inputs, meta), out in zip(calls, plain):                  # smoother = None: what it was
        ref, _ = by_hand(inputs, meta, None)
        assert list(out) == ["imgname"] + ["metric." + k for k in ref]
        for k in ref:
            assert torch.equal(out["metric." + k].view(torch.int32), ref[k].view(torch.int32)), k
    w.smoother = hands_amd.TemporalSmoother(model)
    second = hands_amd.TemporalSmoother(model)
    changed = 0
    for (inputs, meta), before in zip(calls, plain):
        out = w.forward(inputs, dict(targets), meta, "test")[0]
        ref, pred = by_hand(inputs, meta, second)
        assert list(out) == list(before)
        for k in ref:
            assert torch.equal(out["metric." + k].view(torch.int32), ref[k].view(torch.int32)), k
            changed += int(not torch.equal(out["metric." + k].view(torch.int32), before["metric." + k].view(torch.int32)))
    assert changed > 0
    # "vis" and "extract" are no frames of the stream: the raw prediction, and the state stays where it was
    raw = w.model(*calls[1])
    for mode in ("vis", "extract"):
        full = w.forward(calls[1][0], dict(targets), calls[1][1], mode)
        assert torch.equal(full["pred.mano.pose.r"], raw["mano.pose.r"].cpu()), mode
    third = w.forward(calls[0][0], dict(targets), calls[0][1], "test")[0]
    ref, _ = by_hand(*calls[0], second)
    for k in ref:
        assert torch.equal(third["metric." + k].view(torch.int32), ref[k].view(torch.int32)), k
    w.reset_smoother()
    first_again = w.forward(calls[0][0], dict(targets), calls[0][1], "test")[0]
    second.reset()
    ref, _ = by_hand(*calls[0], second)
    for k in ref:
        assert torch.equal(first_again["metric." + k].view(torch.int32), ref[k].view(torch.int32)), k
    w.smoother = None


def test_accel_metric_of_a_jittered_stream_goes_down(forward):
    """The synthetic parameter case of tests/test_smoothing.py (global orientation 0.5 sin(2 pi 0.5 t) rad, noise 0.03 rad a frame,
    T = 64, 30 fps), both hands, posed with the synthetic MANO asset: no trunk forward."""
    import hands_amd
    from hands_amd import _lib
    from hands_amd.mano_head import run_mano_heads
    model = forward[0]
    T, fps = 64, 30.0
    dev = torch.device("cuda", torch.cuda.current_device())
    P = model.packed(dev)
    K = torch.tensor([[1000.0, 0.0, 112.0], [0.0, 1000.0, 112.0], [0.0, 0.0, 1.0]]).repeat(T, 1, 1).cuda()

    def posed(rot_r, rot_l):
        rot = torch.cat([_cuda(one_channel(R.astype(np.float32))[0]) for R in (rot_r, rot_l)])
        shape = torch.zeros(2 * T, 10, device=dev)
        cam = torch.tensor([0.9, 0.05, -0.02], device=dev).repeat(2 * T, 1)
        return run_mano_heads(_lib.lib(), P["mano_r"], P["mano_l"], rot, shape, cam, cam, K, float(model.img_res), T, _stream(), None)
    sides = [SR.jitter_case(T, fps, 0.03, seed, axis) for seed, axis in ((0, (0.0, 0.0, 1.0)), (1, (1.0, 1.0, 0.0)))]
    clean, raw = posed(sides[0][0], sides[1][0]), posed(sides[0][1], sides[1][1])
    targets = dict(clean, is_valid=torch.ones(T, device=dev), right_valid=torch.ones(T, device=dev), left_valid=torch.ones(T, device=dev))
    smoothed = hands_amd.smooth_predictions(raw, model, {"intrinsics": K}, fps=fps)
    a_raw = hands_amd.evaluate_accel_metrics(raw, targets, fps=fps)
    a_smooth = hands_amd.evaluate_accel_metrics(smoothed, targets, fps=fps)
    for k in ("acc/r", "acc/l", "acc/h", "acc/j/h", "acc/abs/h"):
        r, s = torch.nanmean(a_raw[k]).item(), torch.nanmean(a_smooth[k]).item()
        print(f"SMOOTH|accel {k}|raw {r:.3f} m/s^2|smoothed {s:.3f} m/s^2|ratio {s / r:.3f}")
        assert s < r, (k, s, r)
