"""Host-side tests of ``HandsLight(backbone='vit_b_16')`` (no GPU): construction, the state_dict inventory against what the
reference's constructor produced (tests/golden/make_golden_vit.py), checkpoint round trip, the weight recipe, and the CPU
stand-in of torchvision's ViT (tests/vit_b16_standin.py) against an independent implementation."""
import json
import os
import sys

import pytest
import torch

import hands_amd
from hands_amd.hands_light import DEFAULT_ARGS, _Args
from hands_amd.weights import recipe_tensor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vit_b16_standin as S  # noqa: E402

CONFIGS = {"default": {}, "separate": dict(separate_hands=True), "center_corner": dict(pos_enc="center+corner")}


def _model(over=None):
    return hands_amd.HandsLight(backbone="vit_b_16", args=_Args(dict(DEFAULT_ARGS, backbone="vit_b_16", **(over or {}))))


@pytest.fixture(scope="module")
def vit_model():
    return hands_amd.apply_recipe(_model()).eval()


def test_vit_backbone_constructs(vit_model):
    assert vit_model.backbone_name == "vit_b_16" and vit_model.feat_dim == 2048
    assert isinstance(vit_model.backbone.encoder.layers.encoder_layer_11.self_attention, torch.nn.MultiheadAttention)
    assert vit_model.backbone.encoder.ln.eps == 1e-6 and vit_model.backbone.heads.head.out_features == 1000
    assert hasattr(vit_model, "vit_conv") and hasattr(vit_model, "hand_backbone_vit_conv")
    with pytest.raises(NotImplementedError):          # every other value keeps raising
        hands_amd.HandsLight(backbone="resnet18")
    with pytest.raises(NotImplementedError):
        hands_amd.HandsLight(backbone="vit_l_16")
    with pytest.raises(NotImplementedError):          # the reference's own constructor fails on this combination (model.py:72-73)
        _model(dict(separate_hands=True, pos_enc="center"))
    # the CPU refusal of the forward is the ResNet one: no eager fall-back exists for the new trunk either
    inputs, meta = hands_amd.synthetic_inputs(1, 0)
    with pytest.raises(RuntimeError, match="HIP device"):
        vit_model(inputs, meta)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_vit_state_dict_names_and_shapes(golden_dir, name):
    want = json.load(open(os.path.join(golden_dir, "vit_b16_state_dict_keys.json")))[name]
    m = _model(CONFIGS[name])
    got = {k: list(v.shape) for k, v in m.state_dict().items() if ".mano." not in k}
    assert sorted(got) == sorted(want)
    assert got == want
    assert len(got) == {"default": 363, "separate": 522, "center_corner": 363}[name]
    if name == "center_corner":
        assert got["hand_backbone.conv_proj.weight"] == [768, 83, 16, 16] and got["backbone.conv_proj.weight"] == [768, 3, 16, 16]


def test_vit_state_dict_roundtrip_and_wrapper_prefix(vit_model):
    m2 = _model()
    ck = {"model." + k: v for k, v in vit_model.state_dict().items()}         # Lightning-style checkpoint
    res = m2.load_state_dict({k[len("model."):]: v for k, v in ck.items()}, strict=False)
    assert not res.missing_keys and not res.unexpected_keys
    for k in ("backbone.encoder.layers.encoder_layer_7.self_attention.in_proj_weight", "hand_backbone.class_token",
              "hand_backbone_vit_conv.2.running_var", "backbone.encoder.pos_embedding"):
        assert torch.equal(m2.state_dict()[k], vit_model.state_dict()[k]), k
    assert m2._packed is None


def test_recipe_new_keys_deterministic_and_old_keys_unchanged(vit_model, recipe_sd):
    sd = vit_model.state_dict()
    pre = "backbone.encoder.layers.encoder_layer_3."
    new = ["backbone.class_token", pre + "self_attention.in_proj_weight", pre + "self_attention.in_proj_bias", pre + "ln_1.weight",
           pre + "ln_2.weight", "backbone.encoder.ln.weight", "vit_conv.2.weight", "vit_conv.2.running_mean", "vit_conv.2.running_var"]
    for k in new:
        a, b = recipe_tensor(k, sd[k]), recipe_tensor(k, sd[k])
        assert a is not None and torch.equal(a, b) and torch.equal(a, sd[k]), k
    # scales: logits O(1), LayerNorm gains near one
    w = sd[pre + "self_attention.in_proj_weight"]
    assert abs(float(w.std()) * 768 ** 0.5 - 1.0) < 0.02
    assert abs(float(sd[pre + "ln_1.weight"].mean()) - 1.0) < 0.02 and float(sd["vit_conv.2.running_var"].min()) >= 1.0
    # additive only: keys that had a recipe before produce what they produced (sample of the ResNet model's inventory, plus the
    # generic branches the ViT keys fall into, pinned by value)
    for k in ("backbone.conv1.weight", "backbone.layer3.2.bn3.weight", "hand_backbone.layer4.0.downsample.1.running_var",
              "head_r.hmr_layer.decoders.pose_6d.bias", "feature_conv.0.weight", "grasp_classifier.6.bias", "head_l.cam_init.4.bias"):
        assert torch.equal(recipe_tensor(k, recipe_sd[k]), recipe_sd[k]), k
    g = torch.Generator().manual_seed(__import__("zlib").crc32(b"encoder.pos_embedding"))
    assert torch.equal(recipe_tensor("encoder.pos_embedding", torch.empty(1, 197, 768)), torch.randn((1, 197, 768), generator=g))
    k = pre + "ln_1.bias"
    g = torch.Generator().manual_seed(__import__("zlib").crc32(k.encode()))
    assert torch.equal(recipe_tensor(k, sd[k]), 0.01 * torch.randn((768,), generator=g))


def test_standin_matches_transformers_vit():
    """The stand-in's encoder (class token, position embedding, 12 blocks, final LayerNorm) against ``transformers.ViTModel`` with
    the same weights (in_proj split into query / key / value).  Bar 5e-5 on activations of magnitude ~5: two fp32 evaluation orders of
    12 blocks whose reductions are 768-3072 long differ by about eps * |x| * sqrt(K) = 6e-8 * 5 * 55 = 2e-5; a wrong composition
    (LayerNorm placement, eps 1e-12, tanh GELU, head split) is off by 1e-2 or more."""
    try:
        from transformers import ViTConfig, ViTModel
    except ImportError:
        pytest.skip("the `transformers` package is not installed: no independent ViT implementation to compare the stand-in with")
    net = hands_amd.apply_recipe(S.vit_b_16()).eval()
    cfg = ViTConfig(hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072, hidden_act="gelu",
                    layer_norm_eps=1e-6, image_size=224, patch_size=16, num_channels=3, qkv_bias=True,
                    hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    hf = ViTModel(cfg, add_pooling_layer=False).eval()
    sd = net.state_dict()
    new = {"embeddings.cls_token": sd["class_token"], "embeddings.position_embeddings": sd["encoder.pos_embedding"],
           "embeddings.patch_embeddings.projection.weight": sd["conv_proj.weight"],
           "embeddings.patch_embeddings.projection.bias": sd["conv_proj.bias"],
           "layernorm.weight": sd["encoder.ln.weight"], "layernorm.bias": sd["encoder.ln.bias"]}
    # layer names of transformers >= 5 (layers.i.attention.q_proj, mlp.fc1) or of the 4.x series (encoder.layer.i.attention.attention.query)
    v5 = "layers.0.attention.q_proj.weight" in hf.state_dict()
    names = (dict(q="attention.q_proj", k="attention.k_proj", v="attention.v_proj", o="attention.o_proj", fc1="mlp.fc1", fc2="mlp.fc2") if v5 else
             dict(q="attention.attention.query", k="attention.attention.key", v="attention.attention.value", o="attention.output.dense",
                  fc1="intermediate.dense", fc2="output.dense"))
    for i in range(12):
        s, d = f"encoder.layers.encoder_layer_{i}.", (f"layers.{i}." if v5 else f"encoder.layer.{i}.")
        wq, wk, wv = sd[s + "self_attention.in_proj_weight"].chunk(3, 0)
        bq, bk, bv = sd[s + "self_attention.in_proj_bias"].chunk(3, 0)
        for nm, w, b in (("q", wq, bq), ("k", wk, bk), ("v", wv, bv)):
            new[d + names[nm] + ".weight"], new[d + names[nm] + ".bias"] = w, b
        for a, b in (("self_attention.out_proj", names["o"]), ("ln_1", "layernorm_before"), ("ln_2", "layernorm_after"),
                     ("mlp.0", names["fc1"]), ("mlp.3", names["fc2"])):
            new[d + b + ".weight"], new[d + b + ".bias"] = sd[s + a + ".weight"], sd[s + a + ".bias"]
    res = hf.load_state_dict(new, strict=False)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "mask_token" not in k], res
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        tok = net._process_input(x)
        mine = net.encoder(torch.cat([net.class_token.expand(2, -1, -1), tok], 1))
        theirs = hf(pixel_values=x).last_hidden_state
    err, mag = (mine - theirs).abs().max().item(), theirs.abs().max().item()
    print(f"stand-in vs transformers.ViTModel: max abs {err:.3e} on activations of magnitude {mag:.2f}")
    assert mine.shape == (2, 197, 768) and err < 5e-5, (err, mag)


def test_standin_trunk_shapes_and_keys(golden_dir):
    """The stand-in carries torchvision's key names (the reference's state_dict inventory was recorded through it) and
    vit_trunk_features delivers what the ResNet-50 trunk does: (B, 2048, 7, 7)."""
    want = json.load(open(os.path.join(golden_dir, "vit_b16_state_dict_keys.json")))["default"]
    got = {"backbone." + k: list(v.shape) for k, v in S.vit_b_16().state_dict().items()}
    assert got == {k: v for k, v in want.items() if k.startswith("backbone.")} and len(got) == 152
    net, conv = S.vit_b_16().eval(), S.vit_conv().eval()
    with torch.no_grad():
        f = S.vit_trunk_features(net, conv, torch.zeros(1, 3, 224, 224))
    assert f.shape == (1, 2048, 7, 7)
