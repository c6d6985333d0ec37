"""HandsLight(tf_decoder=True) on the CPU side: the restated transformer head against the reference's fixture, the parameter
containers against the reference's state_dict inventory, the rejected combinations and the weight recipe's new branch."""
import json
import os
import re
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import hands_amd
from hands_amd.weights import recipe_tensor

import tf_decoder_ref as R

HEAD_KEYS = ("pose_6d", "shape", "cam_t.wp", "pose", "cam_t.wp.init")


def tf_args(**over):
    return type(hands_amd.DEFAULT_ARGS)(dict(hands_amd.DEFAULT_ARGS, **over))


@pytest.fixture(scope="module")
def head_fixture(golden_dir):
    d = np.load(os.path.join(golden_dir, "tf_decoder_head.npz"), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    feats = torch.relu(0.5 * torch.randn(2, 2128, 7, 7, generator=torch.Generator().manual_seed(meta["seed"])))
    return d, meta, feats


@pytest.mark.parametrize("side", ["r", "l"])
def test_restated_head_reproduces_the_reference(head_fixture, side):
    """tests/tf_decoder_ref.py in fp32 against the reference's fp32 outputs and per-iteration token means: within 4 x the
    reference's own fp32-minus-fp64 distance per key; in fp64 against its .double() run: 1e-10."""
    d, meta, feats = head_fixture
    err = meta["fp32_minus_fp64_max_abs"]
    out, xc = R.hand_hmr_tf(R.head_state_dict(side), feats)
    out64, xc64 = R.hand_hmr_tf(R.head_state_dict(side, torch.float64), feats.double())
    for k, got, got64 in [(k, out[k], out64[k]) for k in HEAD_KEYS] + [("xc", xc, xc64)]:
        ref32, ref64 = d[f"f32/{side}/{k}"], d[f"f64/{side}/{k}"]
        assert got.dtype == torch.float32 and tuple(got.shape) == ref32.shape, k
        e32 = np.abs(got.numpy().astype(np.float64) - ref32).max()
        e64 = np.abs(got64.numpy() - ref64).max()
        print(f"{side}/{k}: fp32 restatement vs reference {e32:.2e} (bar {4 * err[f'{side}/{k}']:.2e}), fp64 {e64:.2e}")
        assert e32 <= 4 * err[f"{side}/{k}"], (k, e32, err[f"{side}/{k}"])
        assert e64 <= 1e-10, (k, e64)
    assert xc.shape == (3, 2, 1024)


@pytest.mark.parametrize("name", ["default", "dense_latent", "plain", "vit"])
def test_tf_decoder_state_dict_equals_the_reference_inventory(golden_dir, name):
    """Names and shapes of HandsLight(tf_decoder=True).state_dict() equal the reference's (feature_conv.* and norm1-3.* are kept
    although the forward never reads them), apply_recipe fills every new tensor, and load_state_dict(strict=True) takes a
    reference-shaped dict."""
    inv = json.load(open(os.path.join(golden_dir, "tf_decoder_state_dict_keys.json")))[name]
    over = {"default": {}, "dense_latent": dict(pos_enc="dense_latent"),
            "plain": dict(pos_enc=None, use_grasp_loss=False, use_glb_feat_w_grasp=False), "vit": dict(backbone="vit_b_16")}[name]
    model = hands_amd.HandsLight(backbone=over.get("backbone", "resnet50"), args=tf_args(**over), tf_decoder=True)
    sd = {k: list(v.shape) for k, v in model.state_dict().items() if ".mano." not in k}
    assert sd == inv, (sorted(set(sd) ^ set(inv))[:10], [k for k in sd if k in inv and sd[k] != inv[k]][:10])
    assert any(k.startswith("feature_conv.") for k in sd) and any(".norm3." in k for k in sd)
    if name != "default":
        return
    new = [k for k in sd if ".hmr_layer." in k or ".cam_init_precursor." in k]
    before = {k: model.state_dict()[k].clone() for k in new}
    hands_amd.apply_recipe(model)
    after = model.state_dict()
    for k in new:
        if not k.endswith(("norm3.weight",)):          # norm3.weight keeps its constructor value; nothing reads it (no_norm)
            assert not torch.equal(before[k], after[k]), k
        assert torch.isfinite(after[k]).all(), k
    for k in new:
        if k.endswith(("out_proj.weight", "linear2.weight")):      # the damped residual branches: a quarter of He scale
            std = after[k].std().item() / (2.0 / after[k].shape[1]) ** 0.5
            assert 0.24 < std < 0.26, (k, std)
    ref_shaped = {k: torch.zeros_like(v) for k, v in after.items()}
    fresh = hands_amd.HandsLight(args=tf_args(), tf_decoder=True)
    assert not fresh.load_state_dict(ref_shaped, strict=True).missing_keys


@pytest.mark.parametrize("over", [dict(pos_enc="sinusoidal_cc"), dict(pos_enc="cam_conv"),
                                  dict(pos_enc=None, no_crops=True, use_glb_feat_w_grasp=False), dict(regress_center_corner=True)])
def test_tf_decoder_rejects_what_the_reference_cannot_run(over):
    with pytest.raises(NotImplementedError, match="tf_decoder with"):
        hands_amd.HandsLight(args=tf_args(**over), tf_decoder=True)


def test_args_tf_decoder_alone_still_raises_and_names_the_keyword():
    """The switch is the constructor keyword; ``args.tf_decoder`` without it is rejected as before, and the message says how to ask."""
    with pytest.raises(NotImplementedError, match="tf_decoder=True"):
        hands_amd.HandsLight(args=tf_args(tf_decoder=True))
    assert hands_amd.HandsLight(args=tf_args(tf_decoder=True), tf_decoder=True).tf_decoder
    assert not hands_amd.HandsLight().tf_decoder


def _inventory_keys(node, out):
    for k, v in node.items():
        if isinstance(v, dict):
            _inventory_keys(v, out)
        elif isinstance(v, list) and all(isinstance(i, int) for i in v) and "." in k:
            out[k] = v
    return out


def test_recipe_branch_touches_no_existing_key(golden_dir):
    """The new branch (x 0.25 on `.hmr_layer.` out_proj / linear2 weights) matches no key of the four inventories that existed before
    tf_decoder: every existing recipe value, and with it every existing fixture, is unchanged.  It does match the new head's keys."""
    matches = lambda k: ".hmr_layer." in k and k.endswith(("out_proj.weight", "linear2.weight"))
    seen = 0
    for fn in ("state_dict_keys.json", "switch_state_dict_keys.json", "vit_b16_state_dict_keys.json", "hamer_state_dict_keys.json"):
        keys = _inventory_keys(json.load(open(os.path.join(golden_dir, fn))), {})
        assert keys, fn
        seen += len(keys)
        assert not [k for k in keys if matches(k)], fn
    assert seen > 1000
    new = _inventory_keys(json.load(open(os.path.join(golden_dir, "tf_decoder_state_dict_keys.json")))["default"], {})
    hit = sorted(k for k in new if matches(k))
    assert len(hit) == 2 * 5, hit            # per head: decoder self / cross out_proj + linear2, encoder out_proj + linear2
    # and the value is the generic He-scale draw of the same key, times 0.25
    k = "head_r.hmr_layer.self_attn.layers.0.linear2.weight"
    g = torch.Generator().manual_seed(zlib.crc32(k.encode()))
    want = 0.25 * (torch.randn(1024, 1024, generator=g) * (2.0 / 1024) ** 0.5)
    assert torch.equal(recipe_tensor(k, torch.empty(1024, 1024)), want)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_wide_attention_kernel_resources(tmp_path):
    """csrc/tf_decoder.hip as the Makefile builds it: no kernel spills to scratch, every instantiation of the attention kernel keeps
    its LDS under 40 KB (four workgroups per CU by LDS) and the 7-key-block form (the 109 tokens) at most 168 registers = three
    workgroups of four waves per CU (docs/EXPERIMENTS.md)."""
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{root}/include", f"-I{root}/hands_amd/csrc",
                        "-fno-fast-math", "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "-c",
                        os.path.join(root, "hands_amd", "csrc", "tf_decoder.hip"), "-o", str(tmp_path / "o.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    blocks = re.split(r"Function Name: ", p.stderr)[1:]
    field = lambda b, pat: int(re.search(pat, b).group(1))
    seen = 0
    for b in blocks:
        assert field(b, r"ScratchSize \[bytes/lane\]: (\d+)") == 0 and field(b, r"VGPRs Spill: (\d+)") == 0, b.split()[0]
        m = re.search(r"wide_attention_kernelILi(\d)E", b.split()[0])
        if m:
            seen += 1
            regs = field(b, r" VGPRs: (\d+)") + field(b, r"AGPRs: (\d+)")
            assert field(b, r"LDS Size \[bytes/block\]: (\d+)") <= 40960
            assert regs <= {"4": 128, "7": 168, "8": 256}[m.group(1)], (m.group(1), regs)
    assert seen == 3
