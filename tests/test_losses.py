"""The validation loss dict (hands_amd/losses.py), host side: tests/loss_ref.py against the REAL reference's values
(tests/golden/loss_light.npz, written by tests/golden/make_golden_loss.py), the epoch aggregation against what the reference's
reform_outputs produced, and the key sets.  Tolerance: 4 x d_ref, the reference's own fp32-vs-fp64 distance of each case, read
from the fixture."""
import math
import os

import numpy as np
import pytest
import torch

import loss_ref
from hands_amd import losses
from loss_ref import check_against_reference


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return loss_ref.load_fixture(os.path.join(golden_dir, "loss_light.npz"))


def test_fixture_cases_are_what_they_claim(fixture):
    cases, _ = fixture
    assert sorted(cases) == list("abcdefgh")
    ref = lambda c: {k: float(v[0]) for k, v in zip(cases[c]["keys"], cases[c]["ref"])}
    assert all(v == 0.0 for k, v in ref("d").items() if "center" not in k and "corner" not in k)
    e = ref("e")
    assert [k for k, v in e.items() if math.isnan(v)] == ["loss/mano/cam_t/r", "loss/mano/transl/l"]
    f = ref("f")
    assert f["loss/mano/cam_t/r"] == 0.0 and f["loss/mano/transl/l"] == 0.0 and all(math.isfinite(v) for v in f.values())
    c = ref("c")
    assert all(c[k] == 0.0 for k in ("loss/mano/cam_t/r", "loss/mano/pose/r", "loss/mano/beta/r", "loss/grasp/r", "loss/center/r"))
    assert cases["g"]["pred"]["mano.beta.r"].shape[0] == 1 and cases["b"]["pred"]["render.r"].shape[-1] == 31
    assert all(0.0 < cases[c]["d_ref"] < 1e-6 for c in cases)


@pytest.mark.parametrize("name", list("abcdefgh"))
def test_loss_ref_fp32_matches_the_reference(fixture, name):
    case = fixture[0][name]
    got = loss_ref.compute_loss_light(case["pred"], case["gt"], case["meta"], case["args"])
    check_against_reference(case, got, f"loss_ref[{name}]")


def test_epoch_end_matches_reform_outputs(fixture):
    ep = fixture[1]
    got = losses.epoch_end(ep["steps"], postfix="__val")
    assert set(got) == {k + "__val" for k in ep["expect"]} and "loss__val" in got
    for k, v in ep["expect"].items():
        assert got[k + "__val"] == pytest.approx(v, rel=0, abs=0), k          # host arithmetic on the same numbers: equal
    assert any(torch.isnan(s["out_dict"]["metric.mpjpe/ra/h"]).any() for s in ep["steps"])
    assert len({len(s["out_dict"]["imgname"]) for s in ep["steps"]}) > 1
    assert all(math.isfinite(v) for v in got.values())
    assert list(losses.epoch_end(ep["steps"], postfix="__test"))[0].endswith("__test")


def test_key_order_and_weights():
    every = dict(use_grasp_loss=True, use_render_seg_loss=True, use_depth_loss=True, regress_center_corner=True)
    assert losses.loss_keys(every) == list(losses.LOSS_KEYS) == loss_ref.ALL_KEYS and len(losses.LOSS_KEYS) == 21
    assert losses.loss_keys({}) == list(losses.BASE_KEYS) == loss_ref.BASE_KEYS and len(losses.BASE_KEYS) == 11
    assert losses.loss_keys(dict(use_depth_loss=True))[11:] == ["loss/depth/r", "loss/depth/l"]
    assert dict(zip(losses.LOSS_KEYS, losses.LOSS_WEIGHTS)) == loss_ref.WEIGHTS


def test_cpu_tensors_raise(fixture):
    import hands_amd
    case = fixture[0]["a"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hands_amd.compute_loss_light(case["pred"], case["gt"], case["meta"], case["args"])
    with pytest.raises(TypeError):
        hands_amd.mul_loss_dict({"loss/mano/kp2d/r": (torch.zeros(1), 5.0)})
    assert all(n in hands_amd.__all__ for n in ("compute_loss_light", "mul_loss_dict", "total_loss", "epoch_end"))
