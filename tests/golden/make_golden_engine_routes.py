#!/usr/bin/env python3
"""Generate tests/golden/engine_routes.json: the launch route ConvEngine takes for every (engine setting, layer) pair of the grid
below, recorded without a GPU (tests/test_engine_routes.py compares against it).

The engine gets a stand-in for the library: the host-only policy queries (Winograd support, split-K factor, stream-K grid, group
class, workspace sizes) go to the real libhands_hip.so and are counted; every launch entry is recorded and answers 0;
hands_stream_is_capturing answers what the setting says.  Tensors are CPU tensors and the two torch.cuda calls of the workspace
code are no-ops, so that code runs unchanged.  Recorded per case: the launches (entry, every descriptor field, S, job count,
which of residual / workspace / counters were passed) interleaved with the hook events (begin: kernel, npix, has_res and
last_sum_block / last_acc64 / last_wino_macs at that moment; end: kernel), and the number of policy queries.
"""
import contextlib
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hands_amd import _lib  # noqa: E402
from hands_amd.engine import ConvEngine  # noqa: E402
from hands_amd.packing import PackedConv  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "engine_routes.json")

POLICY = ("hands_conv3x3_winograd_supported", "hands_conv3x3_winograd4_supported", "hands_conv3x3_winograd_executed_macs",
          "hands_conv3x3_winograd4_executed_macs", "hands_conv2d_splitk_factor", "hands_conv2d_streamk_grid",
          "hands_conv2d_group_class", "hands_conv2d_workspace_floats", "hands_conv2d_streamk_workspace_bytes")
# launch entry -> its arguments (include/hands_hip.h); d = descriptor, the rest by name
LAUNCHES = {
    "hands_conv3x3_winograd4_f32": "d x u bias out stream",
    "hands_conv3x3_winograd_f32": "d x u bias out stream",
    "hands_conv2d_nhwc_pre_f32": "d x scale shift w bias res out S ws ws_n stream",
    "hands_conv2d_nhwc_splitk_fused_f32": "d x w bias res out S ws ws_n ctr ctr_n stream",
    "hands_conv2d_nhwc_splitk_n_f32": "d x w bias res out S ws ws_n stream",
    "hands_conv2d_nhwc_streamk_f32": "d x w bias res out sk sk_bytes epoch stream",
    "hands_conv2d_nhwc_f32": "d x w bias res out stream",
    "hands_conv2d_group_f32": "jobs n stream",
    "hands_conv1x1_dual_nhwc_f32": "d x x2 K1 H2 W2 stride2 in2_ps w bias out stream",
    "hands_stem_conv_maxpool_nhwc_f32": "x w bias out B H W act stream",
    "hands_stem_conv_maxpool_nchw_f32": "x w bias out B H W act stream",
}
VALUES = {"S", "n", "K1", "H2", "W2", "stride2", "in2_ps", "B", "H", "W", "act"}   # recorded as they are
PRESENT = {"res", "ws", "ctr", "sk"}                                               # recorded as "was a pointer passed"


def _fields(p):
    d = p._obj if hasattr(p, "_obj") else p.contents          # C.byref(desc) or C.pointer(desc)
    return [getattr(d, f) for f, _ in _lib.ConvDesc._fields_]


class RecordingLib:
    """Stands in for libhands_hip.so in ConvEngine's calls (see the module docstring)."""

    def __init__(self, capturing):
        self._real, self._capturing = _lib.lib(), capturing
        self.queries, self.events = 0, []

    def __getattr__(self, name):
        if name in POLICY:
            real = getattr(self._real, name)

            def fn(*a):
                self.queries += 1
                return real(*a)
        elif name == "hands_stream_is_capturing":
            def fn(stream):
                self.queries += 1
                return int(self._capturing)
        elif name in LAUNCHES:
            def fn(*a):
                rec = {"entry": name}
                for k, v in zip(LAUNCHES[name].split(), a):
                    if k == "d":
                        rec["desc"] = _fields(v)
                    elif k == "jobs":
                        rec["jobs"] = [[_fields(j.desc), j.residual is not None, j.pre_scale is not None] for j in a[0][:a[1]]]
                    elif k in VALUES:
                        rec[k] = v
                    elif k in PRESENT:
                        rec[k] = v is not None
                self.events.append(["launch", rec])
                return 0
        else:
            raise AttributeError(name)
        fn.__name__ = name
        return fn


@contextlib.contextmanager
def cpu_stand_ins():
    """The two torch.cuda calls of the engine's workspace code as no-ops (CPU tensors need neither)."""
    class _Stream:
        def synchronize(self):
            pass
    saved = torch.cuda.synchronize, torch.cuda.current_stream
    torch.cuda.synchronize, torch.cuda.current_stream = (lambda *a, **k: None), (lambda *a, **k: _Stream())
    try:
        yield
    finally:
        torch.cuda.synchronize, torch.cuda.current_stream = saved


# ---- the grid --------------------------------------------------------------------------------------------------------------------
# engine settings: name -> (switches, hipGraph capture state of the launch stream)
SETTINGS = {
    "default": ({}, False),
    "hands_light": ({"winograd4": True}, False),
    "handoccnet": ({"chain_limit": 64, "chain_min_k": 0, "chain_in_kernel": True}, False),
    "latency": ({"latency_mode": True}, False),
    "overlap_off": ({"overlap": False}, False),
    "bf16x3": ({"math": "bf16x3"}, False),
    "chain_splitk": ({"chain_limit": 64, "chain_in_kernel": False}, False),
    "chain128_rules": ({"chain_limit": 128, "chain_in_kernel": True, "chain_min_k": 1024, "chain_max_pix": 1024,
                        "chain_skip_tokens": True}, False),
    "no_fused_reduce": ({"fuse_splitk_reduce": False}, False),
    "no_group": ({"group_launches": False}, False),
    "capture": ({"overlap": False}, True),
    "handoccnet_capture": ({"chain_limit": 64, "chain_in_kernel": True}, True),
    "stream_k_forced": ({"stream_k": True, "acc64": False, "chain_limit": 64, "chain_in_kernel": True}, False),
    "bad_chain_limit": ({"chain_limit": 96, "chain_in_kernel": True}, False),
}


def _pc(Cin, Cout, k=1, stride=1, pad=None, wino=False, acc64=False, sum_block=-1):
    pad = (k // 2) if pad is None else pad
    Kpad = (k * k * Cin + 15) // 16 * 16
    t = torch.zeros(4)
    return PackedConv(t, t, Cin, Cout, k, k, stride, pad, Kpad, k * k * Cin * Cout, t if wino else None, sum_block, acc64,
                      t if wino else None)


def _buf(n=64):
    return torch.zeros(n)


def _conv(pc, B, H, W, relu=1, **kw):
    return ("conv", dict(pc=pc, B=B, H=H, W=W, relu=relu, **kw))


def _job(pc, B, H, W, relu=1, **kw):
    return dict(pc=pc, x=_buf(), B=B, H=H, W=W, out=_buf(), relu=relu, **kw)


def _pre(Cin):
    return (_buf(Cin), _buf(Cin))


def layer_cases():
    """name -> (method, arguments): shapes of the three models' layers."""
    c = {
        "stem": _conv(_pc(4, 64, 7, 2, 3), 2, 128, 128),
        "expand_res": _conv(_pc(64, 256), 2, 56, 56, res=True),
        "conv3x3_wino": _conv(_pc(64, 64, 3, wino=True), 2, 56, 56),
        "conv3x3_wino_l4": _conv(_pc(512, 512, 3, wino=True), 64, 7, 7),
        "conv3x3_wino_misaligned": _conv(_pc(64, 64, 3, wino=True), 2, 56, 56, x_off=1),
        "conv3x3_s2": _conv(_pc(128, 128, 3, 2), 96, 56, 56),
        "conv1x1_streamk": _conv(_pc(256, 64), 64, 56, 56, res=True),
        "linear_splitk": _conv(_pc(1024, 1024), 2, 1, 1, relu=0, splitk=True),
        "linear_splitk_res": _conv(_pc(1024, 1024), 2, 1, 1, relu=0, splitk=True, res=True),
        "linear_splitk_n": _conv(_pc(512, 256), 2, 1, 1, relu=2, splitk_n=4),
        "tokens": _conv(_pc(256, 1024), 4096, 1, 1, relu=2),
        "pre": _conv(_pc(256, 128), 2, 64, 64, relu=3, pre=True),
        "pre_res": _conv(_pc(256, 256), 2, 64, 64, relu=0, pre=True, res=True),
        "pre_splitk_n": _conv(_pc(512, 256), 2, 1, 1, relu=3, pre=True, splitk_n=4),
        "acc64": _conv(_pc(256, 256, acc64=True), 2, 32, 32, relu=3),
        "acc64_3x3": _conv(_pc(256, 256, 3, wino=True, acc64=True), 2, 32, 32, relu=3),
        "acc64_linear": _conv(_pc(512, 512, acc64=True), 2, 1, 1, relu=3, splitk=True),
        "acc64_pre_res": _conv(_pc(256, 256, acc64=True), 2, 32, 32, relu=0, pre=True, res=True),
        "sum_block_128": _conv(_pc(512, 128, sum_block=128), 2, 16, 16),
        "sum_block_0": _conv(_pc(512, 128, sum_block=0), 2, 16, 16),
        "short_k": _conv(_pc(64, 64), 2, 56, 56),
        "strided_1x1": _conv(_pc(256, 512, 1, 2), 2, 56, 56),
        "dual": ("dual", dict(pc=_pc(64 + 256, 256), split=(64, 256, 1), B=2, Ho=56, Wo=56, H2=56, W2=56)),
        "dual_s2": ("dual", dict(pc=_pc(128 + 256, 512), split=(128, 256, 2), B=2, Ho=28, Wo=28, H2=56, W2=56)),
        "stem_pool": ("stem_pool", dict(pc=_pc(4, 64, 7, 2, 3), B=2, H=128, W=128)),
        "stem_pool_nchw": ("stem_pool_nchw", dict(pc=_pc(4, 64, 7, 2, 3), B=2, H=128, W=128)),
    }
    narrow, wide, narrow_pre = _pc(256, 64), _pc(256, 256), _pc(256, 64)
    c["group_one"] = ("group", [_job(narrow, 2, 32, 32)])
    c["group_mixed"] = ("group", [
        _job(narrow, 2, 32, 32), _job(wide, 2, 32, 32), _job(narrow_pre, 2, 32, 32, pre=_pre(256)),
        _job(_pc(256, 256, 3, wino=True), 2, 32, 32), _job(wide, 2, 32, 32, res=_buf()), _job(_pc(256, 256, acc64=True), 2, 32, 32),
        _job(narrow, 2, 32, 32, relu=3), _job(_pc(256, 128, 1, 2), 2, 64, 64), _job(_pc(64, 256), 2, 32, 32, res=_buf()),
        _job(_pc(512, 512, sum_block=128), 2, 16, 16)])
    c["group_many"] = ("group", [_job(_pc(256, 256), 2, 16, 16, res=_buf() if i % 3 == 0 else None) for i in range(9)]
                       + [_job(_pc(128, 64), 2, 16, 16) for _ in range(10)] + [_job(_pc(256, 64), 2, 16, 16, pre=_pre(256))])
    return c


def run_case(setting, case):
    """Drive one call on a fresh engine; return (record, begin/end has_res pairs of the hook)."""
    switches, capturing = SETTINGS[setting]
    method, a = case
    eng = ConvEngine()
    for k, v in switches.items():
        setattr(eng, k, v)
    L = RecordingLib(capturing)
    pairs = []

    def hook(phase, pc, npix, stream, has_res, kernel):
        if phase == "begin":
            L.events.append(["begin", kernel, npix, bool(has_res), eng.last_sum_block, bool(eng.last_acc64), eng.last_wino_macs])
            pairs.append([bool(has_res)])
        else:
            L.events.append(["end", kernel])
            pairs[-1].append(bool(has_res))
    eng.hook = hook
    stream = None
    try:
        if method == "conv":
            a = dict(a)
            pc, B, H, W = a.pop("pc"), a.pop("B"), a.pop("H"), a.pop("W")
            relu = a.pop("relu")
            if a.pop("res", False):
                a["res"] = _buf()
            if a.pop("pre", False):
                a["pre"] = _pre(pc.Cin)
            eng.conv(L, pc, _buf(), B, H, W, _buf(), relu, stream, **a)
        elif method == "group":
            eng.conv_group(L, [dict(j) for j in a], stream)
        elif method == "dual":
            eng.conv_dual(L, a["pc"], a["split"], _buf(), _buf(), a["B"], a["Ho"], a["Wo"], a["H2"], a["W2"], _buf(), stream)
        elif method == "stem_pool":
            eng.stem_pool(L, a["pc"], _buf(), 0, _buf(), a["B"], a["H"], a["W"], 1, stream)
        else:
            eng.stem_pool_nchw(L, a["pc"], _buf(), 0, _buf(), 0, a["B"], a["H"], a["W"], 1, stream)
    except ValueError:
        L.events.append(["raises", "ValueError"])
    return {"events": L.events, "queries": L.queries}, pairs


def record_all():
    """{"routes": [distinct event sequences], "cases": {"setting/layer": [index into routes, policy queries]}}"""
    cases = layer_cases()
    routes, index, table = [], {}, {}
    with cpu_stand_ins():
        for s in SETTINGS:
            for name, case in cases.items():
                rec = run_case(s, case)[0]
                key = json.dumps(rec["events"])
                if key not in index:
                    index[key] = len(routes)
                    routes.append(rec["events"])
                table[f"{s}/{name}"] = [index[key], rec["queries"]]
    return {"routes": routes, "cases": table}


def main():
    fixture = record_all()
    with open(FIXTURE, "w") as f:
        json.dump(fixture, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"{FIXTURE}: {len(fixture['cases'])} cases, {len(fixture['routes'])} routes, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
