"""The launch sequences of the shared head stages (engine.linear_chain, grasp_head.run_grasp_head, hmr_head.cam_init /
iter_head) on CPU tensors, with a library and an engine that only record their calls: which layer goes out with which
activation, ``splitk`` mark, row strides and offsets, per model."""
from types import SimpleNamespace

import pytest
import torch

from hands_amd._lib import ACT_LEAKY_RELU, ACT_NONE, ACT_RELU
from hands_amd.engine import linear_chain
from hands_amd.grasp_head import GRASP_SPLITK, run_grasp_head
from hands_amd.hmr_head import cam_init, iter_head

STREAM = 77


class _Lib:
    """The library entries the heads call directly: records (name, the arguments that are not pointers) and returns success."""
    NOT_POINTERS = {"hands_grasp_input_f32": (1, 5, 6, 7, 8, 9), "hands_hmr_init_f32": (2, 3, 4, 5)}

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        def call(*args):
            self.log.append((name,) + tuple(args[i] for i in self.NOT_POINTERS[name]))
            return 0
        return call


class _Engine:
    """``ConvEngine.conv``'s signature; records (layer, Cin, Cout, rows, act, splitk, in_ps, x_off, out_ps, out_off, has_res) and
    which tensors the launch reads and writes."""

    def __init__(self, log):
        self.log, self.io = log, []

    def conv(self, L, pc, x, B, H, W, out, relu, stream, res=None, in_ps=None, out_ps=None, res_ps=None, x_off=0, out_off=0,
             res_off=0, splitk=False, splitk_n=0, pre=None, out_hw=None):
        assert (H, W, stream, splitk_n, pre, out_hw) == (1, 1, STREAM, 0, None, None)
        self.log.append((pc.name, pc.Cin, pc.Cout, B, int(relu), bool(splitk), in_ps, x_off, out_ps, out_off, res is not None))
        self.io.append((x, out))
        return 1, 1


def _layer(name, Cin, Cout):
    return SimpleNamespace(name=name, Cin=Cin, Cout=Cout)


def _bufs():
    ws = {}

    def buf(name, numel):
        assert name not in ws or ws[name].numel() >= numel
        return ws.setdefault(name, torch.zeros(numel))
    return ws, buf


def _grasp_layers(feat):
    return [_layer("g0", (feat + 154 + 15) // 16 * 16, 1024), _layer("g2", 1024, 512), _layer("g4", 512, 128), _layer("g6", 128, 12)]


# (model, feature columns, shape row length, first shape column): HandsLight reads the shape from its HMR state rows
GRASP_CASES = [("hands_light", 2048, 2048 + 112, 2048 + 96), ("hands_light", 0, 2048 + 112, 2048 + 96),
               ("hamer", 0, 10, 0), ("handoccnet", 0, 10, 0)]
GRASP_MARKS = {"hands_light": (True, True, True, False), "hamer": (True, True, True, True), "handoccnet": (True, True, False, False)}


@pytest.mark.parametrize("model,feat,shape_ld,shape_off", GRASP_CASES)
def test_grasp_head_launch_sequence(model, feat, shape_ld, shape_off):
    assert GRASP_SPLITK == GRASP_MARKS
    bz = 3
    B2, gld = 2 * bz, (feat + 154 + 15) // 16 * 16
    log = []
    eng, (ws, buf) = _Engine(log), _bufs()
    shape, rot, fv = torch.zeros(B2 * shape_ld), torch.zeros(B2, 144), torch.zeros(bz, 2048)
    kw = {"shape_ld": shape_ld, "shape_off": shape_off, "feat": fv, "feat_dim": feat} if model == "hands_light" else {}
    out = run_grasp_head(eng, _Lib(log), _grasp_layers(feat), GRASP_SPLITK[model], shape, rot, bz, STREAM, buf, **kw)
    m = GRASP_MARKS[model]
    assert log == [
        ("hands_grasp_input_f32", shape_ld, B2, bz, feat, gld, STREAM),
        ("g0", gld, 1024, B2, ACT_RELU, m[0], None, 0, None, 0, False),
        ("g2", 1024, 512, B2, ACT_RELU, m[1], None, 0, None, 0, False),
        ("g4", 512, 128, B2, ACT_RELU, m[2], None, 0, None, 0, False),
        ("g6", 128, 12, B2, ACT_NONE, m[3], None, 0, None, 0, False)]
    assert {k: v.numel() for k, v in ws.items()} == {"grasp_in": B2 * gld, "g1": B2 * 1024, "g2": B2 * 512, "g3": B2 * 128}
    # each layer reads what the one before it wrote; the last one writes a tensor of its own, 12 wide
    ins, outs = zip(*eng.io)
    assert ins[0] is ws["grasp_in"] and all(a is b for a, b in zip(ins[1:], outs[:-1])) and outs[-1].shape == (B2, 12)
    assert list(out.keys()) == ["grasp.r", "grasp.l"] and all(v.shape == (bz, 9) and v.is_contiguous() for v in out.values())


def _hmr_layers():
    F = 2048
    return {"ci0": _layer("ci0", F, 512), "ci2": _layer("ci2", 512, 512), "ci4": _layer("ci4", 512, 4),
            "r0": _layer("r0", F + 112, 1024), "r3": _layer("r3", 1024, 1024), "dec": _layer("dec", 1024, 112)}


def test_cam_init_chain_of_both_head_forms():
    """The iterative head reads the feat segment of its state rows in place (row stride ld, first float so); the transformer
    head reads pooled rows; both write their rows of ``caminit4``."""
    bz, side, ld = 3, 1, 2048 + 112
    so, co = side * bz * ld, side * bz * 4
    hp, cam4 = _hmr_layers(), torch.zeros(2 * bz, 4)
    for names, x, first in (((f"h512a{side}", f"h512b{side}"), torch.zeros(2 * bz * ld), {"in_ps": ld, "x_off": so}),
                            (("h512a", "h512b"), torch.zeros(bz, 2048), {})):
        log = []
        eng, (ws, buf) = _Engine(log), _bufs()
        cam_init(eng, buf, names, _Lib(log), hp, STREAM, x, bz, cam4, co, **first)
        assert log == [("ci0", 2048, 512, bz, 1, True, first.get("in_ps"), first.get("x_off", 0), None, 0, False),
                       ("ci2", 512, 512, bz, 1, True, None, 0, None, 0, False),
                       ("ci4", 512, 4, bz, 0, False, None, 0, None, co, False)]
        assert sorted(ws) == sorted(names) and all(v.numel() == bz * 512 for v in ws.values())
        assert eng.io[0][0] is x and eng.io[1][0] is ws[names[0]] and eng.io[2][0] is ws[names[1]] and eng.io[2][1] is cam4


def test_iter_head_launch_sequence():
    bz, side, F = 2, 1, 2048
    ld = F + 112
    so, co = side * bz * ld, side * bz * 4
    log = []
    eng, (ws, buf) = _Engine(log), _bufs()
    state, cam4 = torch.zeros(2 * bz * ld), torch.zeros(2 * bz, 4)
    iter_head(eng, buf, _Lib(log), _hmr_layers(), STREAM, side, bz, state, cam4, F)
    refine = [("r0", ld, 1024, bz, 1, True, ld, so, None, 0, False), ("r3", 1024, 1024, bz, 1, True, None, 0, None, 0, False),
              ("dec", 1024, 112, bz, 0, True, None, 0, ld, so + F, True)]
    assert log == [("ci0", F, 512, bz, 1, True, ld, so, None, 0, False), ("ci2", 512, 512, bz, 1, True, None, 0, None, 0, False),
                   ("ci4", 512, 4, bz, 0, False, None, 0, None, co, False), ("hands_hmr_init_f32", bz, ld, F, STREAM)] + 3 * refine
    # buffers that are live on two streams at once carry the side in their name
    assert sorted(ws) == [f"h512a{side}", f"h512b{side}", f"x1024a{side}", f"x1024b{side}"]


def test_linear_chain_buffers_and_last_layer():
    """Without ``out`` the last layer writes the last named buffer (HandOccNet's regressor MLP: three layers, every one marked)."""
    log = []
    eng, (ws, buf) = _Engine(log), _bufs()
    layers = [(_layer("base0", 1024, 1024), ACT_LEAKY_RELU, True), (_layer("base2", 1024, 512), ACT_LEAKY_RELU, True),
              (_layer("regs", 512, 112), ACT_NONE, True)]
    x = torch.zeros(5, 1024)
    y = linear_chain(eng, None, layers, x, 5, STREAM, buf, ("base0", "base2", "pred"))
    assert [e[:6] for e in log] == [("base0", 1024, 1024, 5, ACT_LEAKY_RELU, True), ("base2", 1024, 512, 5, ACT_LEAKY_RELU, True),
                                    ("regs", 512, 112, 5, ACT_NONE, True)]
    assert y is ws["pred"] and y.numel() == 5 * 112 and ws["base0"].numel() == 5 * 1024 and ws["base2"].numel() == 5 * 512
    # a single layer with every option: first and last at once
    log.clear()
    out = torch.zeros(64)
    assert linear_chain(eng, None, layers[2:], x, 5, STREAM, buf, (), out=out, in_ps=7, x_off=3, out_ps=9, out_off=11) is out
    assert log == [("regs", 512, 112, 5, ACT_NONE, True, 7, 3, 9, 11, False)]
