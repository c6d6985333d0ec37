"""GPU tests of HandsLight(tf_decoder=True): the wide single-head attention kernel, the token kernels, the transformer head alone and
the whole forward against the reference's fixtures (tests/golden/make_golden_tf_decoder.py)."""
import json
import os

import numpy as np
import pytest
import torch

import hands_amd
from hands_amd import _lib
from hands_amd._lib import check, ptr
from hands_amd.hmr_head import tf_head
from hands_amd.weights import synthetic_dense_inputs, synthetic_inputs
from oracle import hands_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = 10001
CANARY = -777.25
TFDEC_CASES = ("default", "flip", "dense_latent", "plain", "noglb", "depth", "vit")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def tf_args(**over):
    return type(hands_amd.DEFAULT_ARGS)(dict(hands_amd.DEFAULT_ARGS, **over))


# ---- hands_wide_attention_f32 ---------------------------------------------------------------------------------------------------
def _attention_inputs(Tq, Tk, D, B, layout, kind, seed):
    """(q, k, v) as VIEWS of the buffers the kernel reads in place, on the CPU.  layout 'qkv': one packed (B, T, 3 D) buffer (Tq == Tk);
    'kv': q on its own, k | v side by side in a (B, Tk, 2 D) buffer; 'plain': three buffers with a row stride of D + 4."""
    g = torch.Generator().manual_seed(seed)
    if layout == "qkv":
        buf = torch.randn(B, Tq, 3 * D, generator=g)
        q, k, v = buf[..., :D], buf[..., D:2 * D], buf[..., 2 * D:]
    elif layout == "kv":
        q = torch.randn(B, Tq, D, generator=g)
        buf = torch.randn(B, Tk, 2 * D, generator=g)
        k, v = buf[..., :D], buf[..., D:]
    else:
        q, k, v = (torch.randn(B, T, D + 4, generator=g)[..., :D] for T in (Tq, Tk, Tk))
    if kind == "onehot":          # logits x 8: rows close to one-hot
        q.mul_(8.0)
    elif kind == "plus50":        # every logit + 50: scale * q0 * k0 = 50 in the first dimension of every token
        c = (50.0 * D ** 0.5) ** 0.5
        q[..., 0] = c
        k[..., 0] = c
    return q, k, v


def _run_wide_attention(q, k, v, scale):
    """The kernel on device copies of the buffers q, k, v are views of (same strides); `out` has a row stride of D + 8, one spare
    row per batch element and a spare tail, all filled with a canary.  Returns (out view (B, Tq, D), the whole out buffer)."""
    L = _lib.lib()
    B, Tq, D = q.shape
    Tk = k.shape[1]
    dev = {}

    def on_dev(t):                # one device copy per underlying buffer; returns (tensor, element offset of the view)
        base = t._base if t._base is not None else t
        if id(base) not in dev:
            dev[id(base)] = base.to(DEV)
        return dev[id(base)], t.storage_offset()

    ldo = D + 8
    out = torch.full((B * (Tq + 1) * ldo + 64,), CANARY, device=DEV)
    (qd, qo), (kd, ko), (vd, vo) = on_dev(q), on_dev(k), on_dev(v)
    code = L.hands_wide_attention_f32(ptr(qd, qo), q.stride(0), q.stride(1), ptr(kd, ko), k.stride(0), k.stride(1),
                                      ptr(vd, vo), v.stride(0), v.stride(1), ptr(out), (Tq + 1) * ldo, ldo, B, Tq, Tk, D, scale,
                                      _stream())
    check(code, "wide_attention")
    torch.cuda.synchronize()
    full = out.cpu()
    return full[: B * (Tq + 1) * ldo].view(B, Tq + 1, ldo)[:, :Tq, :D], full


ATT_CASES = [  # Tq, Tk, D, B, layout, kind
    (1, 1, 64, 1, "plain", "unit"),
    (17, 5, 64, 3, "plain", "unit"),
    (17, 5, 64, 3, "plain", "plus50"),
    (128, 128, 128, 2, "plain", "unit"),
    (109, 109, 1024, 3, "qkv", "unit"),
    (109, 109, 1024, 3, "qkv", "onehot"),
    (109, 49, 1024, 3, "kv", "unit"),
    (109, 49, 1024, 3, "kv", "plus50"),
]


@pytest.mark.parametrize("case", ATT_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_wide_attention_vs_fp64(case):
    """out = softmax(scale Q K^T) V against an fp64 evaluation on the CPU.  Bar: 8 x the max-abs error of torch's own fp32 CPU
    evaluation of the same inputs against the same fp64 (4 x for a sequential MFMA chain against ATen's 16-lane blocked sums,
    2 x for a maximum over few draws).  Batch element 1 alone equals element 1 of the batch bit for bit; the stride gap and the rows
    behind the last query keep their canary."""
    Tq, Tk, D, B, layout, kind = case
    q, k, v = _attention_inputs(Tq, Tk, D, B, layout, kind, seed=1000 + Tq + Tk + D)
    scale = D ** -0.5
    ref64 = torch.softmax((q.double() @ k.double().transpose(1, 2)) * scale, -1) @ v.double()
    cpu32 = torch.softmax((q @ k.transpose(1, 2)) * scale, -1) @ v
    got, full = _run_wide_attention(q, k, v, scale)
    assert torch.isfinite(got).all()
    e_cpu = (cpu32.double() - ref64).abs().max().item()
    e_hip = (got.double() - ref64).abs().max().item()
    print(f"wide_attention {case}: hip {e_hip:.3e}  cpu fp32 {e_cpu:.3e}  ratio {e_hip / e_cpu if e_cpu else float('nan'):.2f}")
    assert e_hip <= 8 * e_cpu, (case, e_hip, e_cpu)
    # canaries: columns D..ldo of every row, the spare row of every batch element, the tail
    ldo = D + 8
    rows = full[: B * (Tq + 1) * ldo].view(B, Tq + 1, ldo)
    assert torch.all(rows[:, :, D:] == CANARY) and torch.all(rows[:, Tq] == CANARY) and torch.all(full[B * (Tq + 1) * ldo:] == CANARY)
    if B > 1:
        alone, _ = _run_wide_attention(q[1:2], k[1:2], v[1:2], scale)
        assert torch.equal(alone[0], got[1])


def test_wide_attention_rejects_what_is_outside_its_contract():
    L = _lib.lib()
    x = torch.zeros(4 * 129 * 128, device=DEV)
    o = torch.full((129 * 128,), CANARY, device=DEV)
    call = lambda Tq, Tk, D, ld: L.hands_wide_attention_f32(ptr(x), Tq * ld, ld, ptr(x), Tk * ld, ld, ptr(x), Tk * ld, ld, ptr(o), Tq * ld,
                                                            ld, 1, Tq, Tk, D, 0.125, _stream())
    assert call(128, 5, 64, 64) == 0
    assert call(129, 5, 64, 64) == EINVAL          # more than 128 queries
    assert call(5, 129, 64, 64) == EINVAL
    assert call(5, 5, 96, 96) == EINVAL            # D is not a multiple of 64
    assert call(5, 5, 64, 60) == EINVAL            # a row stride below D
    assert call(5, 5, 64, 66) == EINVAL            # a row stride that is no multiple of 4 floats
    assert call(0, 5, 64, 64) == EINVAL
    torch.cuda.synchronize()
    assert torch.all(o[128 * 64:] == CANARY)


# ---- hands_vector_tokens_f32, hands_token_mean_f32 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,C", [(3, 109, 1024), (1, 1, 64)])
def test_vector_tokens_and_token_mean(B, T, C):
    L = _lib.lib()
    g = torch.Generator().manual_seed(B * T + C)
    vec, w, b = torch.randn(B, T, generator=g), torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    ref = torch.relu(vec[..., None].double() * w.double() + b.double())
    out = torch.full((B * T * C + 16,), CANARY, device=DEV)
    vd, wd, bd = vec.to(DEV), w.to(DEV), b.to(DEV)
    check(L.hands_vector_tokens_f32(ptr(vd), T, T, 0, ptr(wd), ptr(bd), ptr(out), B, T, C, _stream()), "vector_tokens")
    got = out[: B * T * C].view(B, T, C)
    assert (got.cpu().double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()
    assert torch.all(out[B * T * C:] == CANARY)
    if T > 3:
        # the HMR state row: the last three tokens sit two floats further right
        row = torch.full((B, T + 3), 1e9)
        row[:, :T - 3], row[:, T - 1:T + 2] = vec[:, :T - 3], vec[:, T - 3:]
        out2, rd = torch.empty(B, T, C, device=DEV), row.to(DEV)
        check(L.hands_vector_tokens_f32(ptr(rd), T + 3, T - 3, 2, ptr(wd), ptr(bd), ptr(out2), B, T, C, _stream()), "vector_tokens")
        assert torch.equal(out2, got)
    assert L.hands_vector_tokens_f32(ptr(vd), T - 1, T, 0, ptr(wd), ptr(bd), ptr(out), B, T, C, _stream()) == EINVAL
    # token mean of the tokens just made
    mean = torch.full((B * C + 16,), CANARY, device=DEV)
    check(L.hands_token_mean_f32(ptr(got), ptr(mean), B, T, C, _stream()), "token_mean")
    want = got.cpu().double().mean(dim=1)
    assert (mean[: B * C].view(B, C).cpu().double() - want).abs().max().item() <= 1e-6 * want.abs().max().item()
    assert torch.all(mean[B * C:] == CANARY)
    one = torch.empty(C, device=DEV)
    check(L.hands_token_mean_f32(ptr(got, (B - 1) * T * C), ptr(one), 1, T, C, _stream()), "token_mean")
    assert torch.equal(one, mean[(B - 1) * C: B * C])
    assert L.hands_token_mean_f32(ptr(got), ptr(mean), B, T, 96, _stream()) == EINVAL


# ---- the head alone -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tf_model():
    return hands_amd.apply_recipe(hands_amd.HandsLight(args=tf_args(), tf_decoder=True)).eval().to(DEV)


def test_tf_head_alone_vs_reference_fp64(golden_dir, tf_model):
    """hmr_head.tf_head on the seeded feature map of tests/golden/tf_decoder_head.npz, both hands: the distance of every
    output (and of the last iteration's token mean) from the reference's fp64 run is at most 2 x the reference's own fp32 distance
    from it, per key."""
    d = np.load(os.path.join(golden_dir, "tf_decoder_head.npz"), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    err = meta["fp32_minus_fp64_max_abs"]
    feats = torch.relu(0.5 * torch.randn(2, 2128, 7, 7, generator=torch.Generator().manual_seed(meta["seed"])))
    bz = 2
    cat = feats.permute(0, 2, 3, 1).contiguous().repeat(2, 1, 1, 1).to(DEV)        # rows [0, bz): right hand, [bz, 2 bz): left
    L, model = _lib.lib(), tf_model
    dev = cat.device
    P = model.packed(dev)
    state = torch.zeros(2 * bz, 112, device=DEV)
    caminit4 = torch.zeros(2 * bz, 4, device=DEV)
    rot = torch.empty(2 * bz, 16, 3, 3, device=DEV)
    for side, name in ((0, "head_r"), (1, "head_l")):
        tf_head(model.engine, lambda nm, numel: model._buf(nm, numel, dev), L, P[name], _stream(), side, bz, 49, cat, state, caminit4,
                model.feat_dim, cat.shape[-1], model.tf_pass)
    check(L.hands_rot6d_to_matrix_f32(ptr(state), 112, ptr(rot), 2 * bz, _stream()), "rot6d")
    torch.cuda.synchronize()
    worst = {}
    for side, s in ((0, "r"), (1, "l")):
        rows = slice(side * bz, (side + 1) * bz)
        got = {"pose_6d": state[rows, :96], "shape": state[rows, 96:106], "cam_t.wp": state[rows, 108:111], "pose": rot[rows],
               "cam_t.wp.init": caminit4[rows, :3], "xc": model._ws[f"tf_xc{side}"][: bz * 1024].view(bz, 1024)}
        for k, v in got.items():
            ref64 = d[f"f64/{s}/{k}"] if k != "xc" else d[f"f64/{s}/xc"][-1]
            e = np.abs(v.cpu().numpy().astype(np.float64) - ref64).max()
            worst[f"{s}/{k}"] = (e, err[f"{s}/{k}"])
            print(f"tf head {s}/{k}: hip vs fp64 {e:.3e}  reference fp32 vs fp64 {err[f'{s}/{k}']:.3e}  ratio {e / err[f'{s}/{k}']:.2f}")
    bad = {k: v for k, v in worst.items() if v[0] > 2 * v[1]}
    assert not bad, bad


# ---- the whole forward ----------------------------------------------------------------------------------------------------------------
def _load_case(golden_dir, name):
    d = np.load(os.path.join(golden_dir, f"hands_light_tfdec_{name}.npz"), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    cfg = dict(meta["config"])
    backbone = cfg.pop("backbone", "resnet50")
    args = tf_args(backbone=backbone, **{k: v for k, v in cfg.items() if k != "tf_decoder"})
    inputs, meta_info = synthetic_inputs(meta["bz"], meta["seed"])
    meta_info["is_flipped"] = torch.from_numpy(d["is_flipped"])
    if cfg.get("pos_enc") == "dense_latent":
        inputs.update(synthetic_dense_inputs(meta["bz"], meta["seed"], "dense_latent"))
    return d, meta, backbone, args, inputs, meta_info


def _assert_fixture_tolerances(out, d, meta, what):
    """Vertices < 1e-6 m, MPJPE-RA < 1e-3 mm; the rest as test_switch_configurations_vs_reference_fixtures, except the camera-space
    and cam_t keys: atol = max(2e-5, 4 x the reference's own movement between 8 and 1 threads recorded in the fixture)."""
    move = meta["threads_8_vs_1"]["max_abs_per_key"]
    keys = [k[4:] for k in d.files if k.startswith("out/")]
    assert sorted(out.keys()) == sorted(keys)
    for k in keys:
        ref, got = d["out/" + k], out[k].cpu().numpy()
        assert got.shape == ref.shape, k
        print(f"{what} {k}: max abs {np.abs(got - ref).max():.3e} (reference 8 vs 1 threads {move[k]:.3e})")
    for k in keys:
        ref, got = d["out/" + k], out[k].cpu().numpy()
        if k.startswith(("grasp", "center.", "corner.")):
            np.testing.assert_allclose(got, ref, rtol=2e-4, atol=2e-4, err_msg=k)
        elif ".cam." in k or k.startswith("mano.cam_t."):
            np.testing.assert_allclose(got, ref, rtol=2e-5, atol=max(2e-5, 4 * move[k]), err_msg=k)
        elif k.startswith("depth."):
            np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * float(np.abs(ref).max()), err_msg=k)
        else:
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5, err_msg=k)
    for hn in "rl":
        verr = np.abs(out[f"mano.vertices.{hn}"].cpu().numpy() - d[f"out/mano.vertices.{hn}"]).max()
        mp = O.mpjpe_ra_mm(out[f"mano.joints3d.{hn}"].cpu(), torch.from_numpy(d[f"out/mano.joints3d.{hn}"]))
        assert verr < 1e-6 and mp < 1e-3, (what, hn, verr, mp)
    return keys


@pytest.mark.parametrize("name", TFDEC_CASES)
def test_tf_decoder_forward_vs_reference_fixtures(golden_dir, name, tf_model):
    d, meta, backbone, args, inputs, meta_info = _load_case(golden_dir, name)
    model = tf_model if name in ("default", "flip") else hands_amd.apply_recipe(hands_amd.HandsLight(backbone=backbone, args=args, tf_decoder=True)).eval().to(DEV)
    dev = lambda t: {k: v.to(DEV) for k, v in t.items()}
    out = model(dev(inputs), dev(meta_info))
    torch.cuda.synchronize()
    out = {k: v.clone() for k, v in out.items()}
    keys = _assert_fixture_tolerances(out, d, meta, name)
    # batch independence: sample 1 alone == sample 1 of the pair
    one = model({k: v[1:].contiguous() for k, v in dev(inputs).items()}, {k: v[1:].contiguous() for k, v in dev(meta_info).items()})
    for k in keys:
        assert torch.equal(one[k], out[k][1:]), k


def test_tf_decoder_graphed_forward_and_latency_mode(golden_dir, tf_model):
    """hipGraph replay equals the eager forward bit for bit; latency_mode=True stays within the fixture's tolerances."""
    from hands_amd import GraphedForward
    d, meta, _, _, inputs, meta_info = _load_case(golden_dir, "default")
    model = tf_model

    def batch(seed):
        i, m = synthetic_inputs(2, seed)
        m["is_flipped"] = torch.tensor([seed & 1, 0])
        return {k: v.to(DEV) for k, v in i.items()}, {k: v.to(DEV) for k, v in m.items()}

    gf = GraphedForward(model, *batch(0))
    for seed in (1, 2):
        i, m = batch(seed)
        want = {k: v.clone() for k, v in model(i, m).items()}
        got = gf(i, m)
        torch.cuda.synchronize()
        assert sorted(got.keys()) == sorted(want.keys())
        for k in want:
            assert torch.equal(got[k], want[k]), (seed, k)
    model.latency_mode = True
    try:
        out = model({k: v.to(DEV) for k, v in inputs.items()}, {k: v.to(DEV) for k, v in meta_info.items()})
        torch.cuda.synchronize()
        out = {k: v.clone() for k, v in out.items()}
    finally:
        model.latency_mode = False
    _assert_fixture_tolerances(out, d, meta, "latency_mode")


def test_tf_head_passes_are_batch_independent(golden_dir, tf_model):
    """The head walks its samples in passes of ``tf_pass`` (256 by default, so that its workspaces stop growing there): with one sample
    per pass the forward equals the single-pass one bit for bit."""
    _, _, _, _, inputs, meta_info = _load_case(golden_dir, "flip")
    dev = lambda t: {k: v.to(DEV) for k, v in t.items()}
    want = {k: v.clone() for k, v in tf_model(dev(inputs), dev(meta_info)).items()}
    tf_model.tf_pass = 1
    try:
        got = {k: v.clone() for k, v in tf_model(dev(inputs), dev(meta_info)).items()}
    finally:
        tf_model.tf_pass = 256
    for k in want:
        assert torch.equal(got[k], want[k]), k
