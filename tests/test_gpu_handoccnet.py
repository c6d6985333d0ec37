"""GPU parity tests of the handoccnet_light path through the C ABI."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hands_amd
from hands_amd import _lib
from hands_amd._lib import check, ptr
from hands_amd.weights import synthetic_inputs
from oracle import handoccnet_oracle as HO
from oracle import hands_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def test_flash_attention_vs_oracle():
    L = _lib.lib()
    g = torch.Generator().manual_seed(0)
    B, N, heads, D = 2, 1024, 4, 64
    C = heads * D
    q, k, v, q2, k2, res = (torch.randn(B, N, C, generator=g) for _ in range(6))
    q, k = 2.0 * q, 1.5 * k        # wide logits: exercises the online-softmax rescale across key tiles
    k2 = 0.05 * k2
    ref_gate = HO.attention(q.double(), k.double(), v.double(), q2.double(), k2.double(), heads, True)
    ref_plain = res.double() + HO.attention(q.double(), k.double(), v.double(), None, None, heads, False)
    d = [t.to(DEV) for t in (q, k, v, q2, k2, res)]
    k2sum = torch.empty(B, C, device=DEV)
    check(L.hands_token_sum_f32(ptr(d[4]), ptr(k2sum), B, N, C, _stream()))
    assert (k2sum.cpu().double() - k2.double().sum(1)).abs().max().item() < 1e-4
    out = torch.full((B, N, C), float("nan"), device=DEV)
    check(L.hands_flash_attention_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), ptr(k2sum), None, ptr(out), B, N, heads,
                                      D, float(D ** -0.5), _stream()))
    assert (out.cpu().double() - ref_gate).abs().max().item() < 2e-5
    check(L.hands_flash_attention_f32(ptr(d[0]), ptr(d[1]), ptr(d[2]), None, None, ptr(d[5]), ptr(out), B, N, heads, D,
                                      float(D ** -0.5), _stream()))
    assert (out.cpu().double() - ref_plain).abs().max().item() < 2e-5


def test_fpn_and_pool_kernels():
    L = _lib.lib()
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(2, 256, 8, 8, generator=g), torch.randn(2, 256, 16, 16, generator=g)
    d = [_nhwc(x).to(DEV), _nhwc(y).to(DEV)]
    out = torch.empty(2, 16, 16, 256, device=DEV)
    check(L.hands_upsample_bilinear_add_f32(ptr(d[0]), ptr(d[1]), ptr(out), 2, 8, 8, 16, 16, 256, _stream()))
    ref = F.interpolate(x, size=(16, 16), mode="bilinear", align_corners=False) + y
    assert (out.cpu().permute(0, 3, 1, 2) - ref).abs().max().item() < 2e-6
    for mode, fn in ((0, F.avg_pool2d), (1, F.max_pool2d)):
        o = torch.empty(2, 8, 8, 256, device=DEV)
        check(L.hands_pool2x2_nhwc_f32(ptr(d[1]), ptr(o), 2, 16, 16, 256, mode, _stream()))
        assert (o.cpu().permute(0, 3, 1, 2) - fn(y, 2, 2)).abs().max().item() < 1e-6
    # nearest upsample + add
    low, up1 = torch.randn(2, 256, 4, 4, generator=g), torch.randn(2, 256, 8, 8, generator=g)
    dd = [_nhwc(low).to(DEV), _nhwc(up1).to(DEV)]
    o = torch.empty(2, 8, 8, 256, device=DEV)
    check(L.hands_upsample_nearest2x_add_f32(ptr(dd[0]), ptr(dd[1]), ptr(o), 2, 4, 4, 256, _stream()))
    assert torch.equal(o.cpu().permute(0, 3, 1, 2), up1 + F.interpolate(low, scale_factor=2))


def test_gate_embed_bn_softmax_kernels():
    L = _lib.lib()
    g = torch.Generator().manual_seed(2)
    p2 = torch.randn(2, 256, 32, 32, generator=g)
    xd = _nhwc(p2).to(DEV)
    comp = torch.empty(2 * 1024, 4, device=DEV)
    check(L.hands_channel_pool_f32(ptr(xd), ptr(comp), 2048, 256, _stream()))
    c = comp.cpu().view(2, 32, 32, 4)
    assert torch.equal(c[..., 0], p2.max(1)[0]) and (c[..., 1] - p2.mean(1)).abs().max().item() < 1e-6
    logit = torch.randn(2048, 4, generator=g)
    ld = logit.to(DEV)
    pr, se = torch.empty(2048, 256, device=DEV), torch.empty(2048, 256, device=DEV)
    check(L.hands_gate_apply_f32(ptr(xd), ptr(ld), 4, ptr(pr), ptr(se), 2048, 256, _stream()))
    s = torch.sigmoid(logit[:, 0]).view(2, 1, 32, 32)
    assert (pr.cpu().view(2, 32, 32, 256).permute(0, 3, 1, 2) - p2 * s).abs().max().item() < 1e-6
    assert (se.cpu().view(2, 32, 32, 256).permute(0, 3, 1, 2) - p2 * (1 - s)).abs().max().item() < 1e-6
    # add_embed2 / add_rowvec
    q, k = torch.randn(2, 1024, 256, generator=g), torch.randn(2, 1024, 256, generator=g)
    qe, ke, kp = torch.randn(1024, 256, generator=g), torch.randn(1024, 256, generator=g), torch.randn(2, 256, generator=g)
    d = [t.to(DEV) for t in (q, k, qe, ke, kp)]
    oq, ok = torch.empty(2, 1024, 256, device=DEV), torch.empty(2, 1024, 256, device=DEV)
    check(L.hands_add_embed2_f32(*[ptr(t) for t in d], ptr(oq), ptr(ok), 2, 1024, 256, _stream()))
    assert torch.equal(oq.cpu(), (q + qe) + kp[:, None]) and torch.equal(ok.cpu(), (k + ke) + kp[:, None])
    check(L.hands_add_rowvec_f32(ptr(d[0]), ptr(d[4]), ptr(oq), 2, 1024, 256, _stream()))
    assert torch.equal(oq.cpu(), q + kp[:, None])
    # bn + leaky
    sc, sh = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g)
    dd = [sc.to(DEV), sh.to(DEV)]
    check(L.hands_bn_leaky_f32(ptr(d[0]), ptr(dd[0]), ptr(dd[1]), ptr(ok), 2048, 256, _stream()))
    assert (ok.cpu() - F.leaky_relu(q * sc + sh, 0.01)).abs().max().item() < 1e-6
    # spatial softmax
    lat = 3 * torch.randn(2, 1024, 24, generator=g)
    betas = 1 + 0.2 * torch.randn(21, generator=g)
    dl, db = lat.to(DEV), betas.to(DEV)
    heat = torch.full((2, 1024, 32), float("nan"), device=DEV)
    check(L.hands_spatial_softmax_f32(ptr(dl), 24, ptr(db), ptr(heat), 32, 2, 1024, 21, _stream()))
    ref = (lat[:, :, :21] * betas).double().softmax(dim=1)      # products in fp32 like the kernel, softmax in fp64
    h = heat.cpu()
    assert (h[:, :, :21].double() - ref).abs().max().item() < 5e-6 * ref.max().item() + 1e-7
    assert torch.all(h[:, :, 21:] == 0)


@pytest.fixture(scope="module")
def hon_gpu():
    return hands_amd.apply_recipe(hands_amd.HandOccNet()).eval().to(DEV)


@pytest.mark.parametrize("seed", [0, 1])
def test_handoccnet_forward_vs_golden(golden_dir, hon_gpu, seed):
    d = np.load(os.path.join(golden_dir, f"handoccnet_light_bz2_seed{seed}.npz"))
    inputs, meta_info = synthetic_inputs(2, seed, device=DEV)
    out = hon_gpu(inputs, meta_info)
    torch.cuda.synchronize()
    keys = [k[4:] for k in d.files if k.startswith("out/")]
    assert sorted(out.keys()) == sorted(keys) and len(out) == 22
    for k in keys:
        ref, got = d["out/" + k], out[k].cpu().numpy()
        assert got.shape == ref.shape and out[k].is_contiguous(), k
        tol = 5e-3 if k.startswith("grasp") else 2e-4
        np.testing.assert_allclose(got, ref, rtol=tol, atol=tol, err_msg=k)
    for hn in "rl":
        verr = np.abs(out[f"mano.vertices.{hn}"].cpu().numpy() - d[f"out/mano.vertices.{hn}"]).max()
        mp = O.mpjpe_ra_mm(out[f"mano.joints3d.{hn}"].cpu(), torch.from_numpy(d[f"out/mano.joints3d.{hn}"]))
        print(f"handoccnet seed {seed} hand {hn}: max vertex err {verr:.3e} m, MPJPE {mp:.3e} mm")
        assert verr < 1e-6 and mp < 1e-3, (verr, mp)


def test_handoccnet_winograd_scopes_stay_within_fp32_noise(hon_gpu):
    """HandOccNet's default (round 5): Winograd F(2x2,3x3) in EVERY 3x3 / stride-1 layer ("all") and no direct fp32 chain longer
    than 64 floats (engine.chain_limit = 64 summed inside the launch, on every launch with K >= 128).  "backbone" (trunk + FPN
    smoothing) was the default of rounds 3-4, engine.winograd = False is the direct kernel everywhere.  This network amplifies any
    fp32 re-association, so the routes differ by noise of the size each has against the reference (tools/hon_parity_ab.py: medians
    4-5e-7 m): <= 1.5e-6 m between any two of them here, and the launch mix is what the scope says."""
    assert hon_gpu.engine.winograd is True and hon_gpu.winograd_scope == "all"
    assert (hon_gpu.engine.chain_limit, hon_gpu.engine.chain_min_k, hon_gpu.engine.chain_in_kernel) == (64, 0, True)
    inputs, meta_info = synthetic_inputs(2, 0, device=DEV)
    outs, counts, splitk = {}, {}, {}
    try:
        for name, wino, scope in (("backbone", True, "backbone"), ("all", True, "all"), ("direct", False, "backbone")):
            hon_gpu.engine.winograd = wino
            if hon_gpu.winograd_scope != scope:
                hon_gpu.winograd_scope = scope
                hon_gpu.invalidate_packed()
            seen = []
            hon_gpu.conv_hook = lambda phase, pc, npix, st, has_res, kernel: seen.append(
                (kernel, pc.Kpad, -1 if hon_gpu.engine.last_acc64 else hon_gpu.engine.last_sum_block))
            outs[name] = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
            hon_gpu.conv_hook = None
            counts[name] = sum(k == "conv_wino_f32_kernel" for k, _, _ in seen) // 2
            splitk[name] = seen
    finally:
        hon_gpu.conv_hook = None
        hon_gpu.engine.winograd = True
        hon_gpu.winograd_scope = "all"
        hon_gpu.invalidate_packed()
    torch.cuda.synchronize()
    assert counts["direct"] == 0 and counts["backbone"] >= 10 and counts["all"] > counts["backbone"], counts
    # blocked summation: every direct fp32 launch with K >= 128 sums blocks of 64 floats, inside the launch (no launch becomes a
    # split-K launch because of it: the same kernels as the unblocked "direct" pass chose for themselves); the launches of the
    # fp64 stages (-1: the heat-map head and the MLPs, round 6) are not blocked -- they have no fp32 chain at all
    igemm = [(k, kp, blk) for k, kp, blk in splitk["all"] if k.startswith("conv_igemm")]
    assert igemm and all(blk in ((64 if kp >= 128 else 0), -1) for _, kp, blk in igemm), igemm
    assert 8 <= sum(blk == -1 for _, _, blk in igemm) // 2 <= 16, [t for t in igemm if t[2] == -1]
    assert sum(k == "conv_igemm_splitk_f32_kernel" for k, _, _ in igemm) <= sum(k == "conv_igemm_splitk_f32_kernel" for k, _, _ in splitk["direct"])
    for a_, b_ in (("backbone", "all"), ("backbone", "direct"), ("all", "direct")):
        for hn in "rl":
            assert (outs[a_][f"mano.vertices.{hn}"] - outs[b_][f"mano.vertices.{hn}"]).abs().max().item() < 1.5e-6, (a_, b_)


def test_handoccnet_batch_independence(hon_gpu):
    inputs, meta_info = synthetic_inputs(5, 3, device=DEV)
    big = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
    small = hon_gpu({k: v[:2].contiguous() for k, v in inputs.items()},
                    {k: v[:2].contiguous() for k, v in meta_info.items()})
    for k in small:
        assert torch.equal(big[k][:2], small[k]), k


def test_handoccnet_pipelined_forwards_keep_stream_semantics(hon_gpu):
    """HandOccNet.async_forward (default): call i runs on pipeline stream i % depth (three forwards in flight at this size) and
    is joined at the first use of its result.  Five un-consumed forwards in flight, the caller zeroing its inputs right after
    every call: each result equals the synchronous forward of ITS inputs bit for bit."""
    samples = [synthetic_inputs(2, seed, device=DEV) for seed in (0, 3, 5, 9, 11)]
    hon_gpu.async_forward = False
    try:
        sync = [{k: v.clone() for k, v in hon_gpu(i, m).items()} for i, m in samples]
    finally:
        hon_gpu.async_forward = True
    torch.cuda.synchronize()
    assert hon_gpu.pipeline_depth == "auto"
    pending = []
    for inputs, meta_info in samples:
        mine = ({k: v.clone() for k, v in inputs.items()}, {k: v.clone() for k, v in meta_info.items()})
        out = hon_gpu(*mine)
        assert out.is_pending
        for d in mine:
            for v in d.values():
                v.zero_()
        pending.append(out)
    for out, ref in zip(pending, sync):
        for k in ref:
            assert torch.equal(out[k], ref[k]), k


def test_graphed_handoccnet_hold_until_protects_an_asynchronous_reader(hon_gpu):
    """`bench.py --workload handoccnet_light --gpus N` replays captured forwards (depth 4) and all-gathers their STATIC outputs on a
    side stream (hands_amd.dist.gather_predictions of a pending result).  GraphedForward.hold_until(event) makes the next replay of
    that captured instance wait for the reader: here a slow reader (a device-side sleep before its copy) on its own stream, depth 2,
    six calls -- every copy must equal the eager forward of ITS call, not of the call that reused the instance."""
    from hands_amd import GraphedForward
    samples = [synthetic_inputs(2, seed, device=DEV) for seed in (0, 3, 5, 9, 11, 12)]
    eager = [{k: v.clone() for k, v in hon_gpu(i, m).items()} for i, m in samples]
    torch.cuda.synchronize()
    g2 = GraphedForward(hon_gpu, *samples[0], depth=2)
    reader = torch.cuda.Stream()
    copies = []
    for inputs, meta_info in samples:
        out = g2(inputs, meta_info)
        ready = out.__dict__["_ready"]
        with torch.cuda.stream(reader):
            reader.wait_event(ready)
            torch.cuda._sleep(20_000_000)                   # ~10 ms: longer than two forwards at this size
            copies.append({k: v.clone() for k, v in out.__dict__["_pending"].items()})
            done = torch.cuda.Event()
            done.record(reader)
        g2.hold_until(done)
    torch.cuda.synchronize()
    for got, ref in zip(copies, eager):
        for k in ref:
            assert torch.equal(got[k], ref[k]), k


@pytest.mark.parametrize("bz", [32, 256])
def test_handoccnet_full_size_batch_independence_and_parity(hon_gpu, bz):
    """BASELINE configs[3] sizes -- bz=32 (one GPU's shard of the 8-GPU run) and bz=256 (the whole batch on one GPU,
    512 crops at 256x256): first two and LAST two samples equal their own bz=2 forwards BIT FOR BIT, the forward is
    idempotent, and the last sample is within 1e-6 m / 1e-3 mm of the oracle (handoccnet_light/model.py:60-129)."""
    from hands_amd.mano import synthetic_mano_asset
    inputs, meta_info = synthetic_inputs(bz, 6, device=DEV)
    big = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
    for lo in (0, bz - 2):
        small = hon_gpu({k: v[lo:lo + 2].contiguous() for k, v in inputs.items()},
                        {k: v[lo:lo + 2].contiguous() for k, v in meta_info.items()})
        for k in small:
            assert torch.equal(big[k][lo:lo + 2], small[k]), (k, lo)
    again = hon_gpu(inputs, meta_info)
    for k in big:
        assert torch.equal(big[k], again[k]) and torch.isfinite(big[k]).all(), k
    sd = {k: v.detach().cpu() for k, v in hon_gpu.state_dict().items()}
    one_i = {k: v[bz - 1:].cpu() for k, v in inputs.items()}
    one_m = {k: v[bz - 1:].cpu() for k, v in meta_info.items()}
    ref = HO.handoccnet_forward(sd, synthetic_mano_asset(True), synthetic_mano_asset(False), one_i, one_m)
    for hn in "rl":
        verr = (big[f"mano.vertices.{hn}"][bz - 1:].cpu() - ref[f"mano.vertices.{hn}"]).abs().max().item()
        mp = O.mpjpe_ra_mm(big[f"mano.joints3d.{hn}"][bz - 1:].cpu(), ref[f"mano.joints3d.{hn}"])
        assert verr < 1e-6 and mp < 1e-3, (hn, verr, mp)


@pytest.mark.parametrize("case", [(64, 32, 32, 128, 1), (64, 8, 8, 128, 2), (37, 5, 7, 64, 1), (64, 4, 4, 256, 2)])
def test_preactivation_folded_into_the_convolution_is_bit_identical(case):
    """hands_conv2d_nhwc_pre_f32: leaky_relu(bn(x)) applied to the operand of the unit's first (pointwise) convolution on
    its way into LDS (hand_head.py:131-136,170-175) == hands_bn_leaky_f32 followed by the plain / split-K launch, bit for
    bit; and the whole forward is bit-identical with the fusion on and off."""
    from hands_amd.engine import ConvEngine
    from hands_amd.packing import pack_conv
    L = _lib.lib()
    B, H, W, Cout, S = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, W, 256, generator=g).to(DEV)
    sc, sh = (1 + 0.2 * torch.randn(256, generator=g)).to(DEV), (0.3 * torch.randn(256, generator=g)).to(DEV)
    pc = pack_conv(torch.randn(Cout, 256, 1, 1, generator=g) / 16, torch.randn(Cout, generator=g), 1, 0, DEV)
    res = torch.randn(B, H, W, pc.Cout, generator=g).to(DEV)
    eng = ConvEngine()
    t0 = torch.empty_like(x)
    check(L.hands_bn_leaky_f32(ptr(x), ptr(sc), ptr(sh), ptr(t0), B * H * W, 256, _stream()))
    a = torch.full((B, H, W, pc.Cout), float("nan"), device=DEV)
    b = torch.full((B, H, W, pc.Cout), float("nan"), device=DEV)
    eng.conv(L, pc, t0, B, H, W, a, 3, _stream(), res=res, splitk_n=S)
    eng.conv(L, pc, x, B, H, W, b, 3, _stream(), res=res, splitk_n=S, pre=(sc, sh))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    ref = F.leaky_relu(F.leaky_relu(x.double().cpu() * sc.double().cpu() + sh.double().cpu(), 0.01) @
                       pc.w[:pc.Cout, :256].double().cpu().T + pc.bias[:pc.Cout].double().cpu() + res.double().cpu(), 0.01)
    assert (b.double().cpu() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


def test_handoccnet_forward_is_bit_identical_without_the_folded_preactivation(hon_gpu):
    inputs, meta_info = synthetic_inputs(3, 8, device=DEV)
    a = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
    hon_gpu.engine.fuse_pre = False
    try:
        b = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
    finally:
        hon_gpu.engine.fuse_pre = True
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("bz", [2, 32])
def test_graphed_handoccnet_is_bit_identical(hon_gpu, bz):
    """hipGraph replay of HandOccNet.forward (model.py:60-129) == the eager call bit for bit: one captured instance, and
    TWO instances in flight (depth=2, the pipelined mode of the 8-GPU shard size: call i replayed on stream i & 1, joined
    at first use), on new inputs copied into the captured buffers, with the caller overwriting its inputs right after
    every call."""
    from hands_amd import GraphedForward
    samples = [synthetic_inputs(bz, seed, device=DEV) for seed in (0, 3, 5, 9)]
    eager = []
    for inputs, meta_info in samples:
        eager.append({k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()})
    torch.cuda.synchronize()
    g1 = GraphedForward(hon_gpu, *samples[0])
    for (inputs, meta_info), ref in zip(samples, eager):
        got = g1(inputs, meta_info)
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(got[k], ref[k]), (bz, k)
    g2 = GraphedForward(hon_gpu, *samples[0], depth=2)
    outs = []
    for (inputs, meta_info), ref in zip(samples, eager):
        mine = ({k: v.clone() for k, v in inputs.items()}, {k: v.clone() for k, v in meta_info.items()})
        out = g2(*mine)
        for d in mine:                      # the caller may overwrite its inputs as soon as the call returns
            for v in d.values():
                v.zero_()
        assert out.is_pending
        outs.append({k: v.clone() for k, v in out.items()})       # joins on the current stream; clone before reuse
    torch.cuda.synchronize()
    for got, ref in zip(outs, eager):
        for k in ref:
            assert torch.equal(got[k], ref[k]), (bz, k)
    bad = synthetic_inputs(bz + 1, 0, device=DEV)
    with pytest.raises(ValueError):
        g2(*bad)
    with pytest.raises(ValueError):         # persistent-workspace models cannot have two captured instances in flight
        GraphedForward(hands_amd.HandsLight(), *samples[0], depth=2)


def test_grouped_pointwise_launch_is_bit_identical_to_separate_launches():
    """hands_conv2d_group_f32 (ConvEngine.conv_group): independent pointwise layers of one kernel instantiation as ONE launch --
    different M, K, strides, activations, a residual, partial tiles, tile counts that are not multiples of 8 -- equal their own
    launches bit for bit; a member of another class (narrow tile, 3x3, fp64) silently takes its own launch; the C entry refuses a
    mixed group (HANDS_EINVAL, nothing launched)."""
    import ctypes as C
    from hands_amd.engine import ConvEngine
    from hands_amd.packing import pack_conv
    L = _lib.lib()
    g = torch.Generator().manual_seed(11)
    mk = lambda Cout, Cin, k=1, stride=1: pack_conv(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5,
                                                    torch.randn(Cout, generator=g), stride, k // 2, DEV)
    xs = {256: torch.randn(5, 16, 16, 256, generator=g).to(DEV), 512: torch.randn(3, 9, 7, 512, generator=g).to(DEV),
          64: torch.randn(70, 1, 1, 64, generator=g).to(DEV)}
    res = torch.randn(5, 16, 16, 256, generator=g).to(DEV)
    pre = ((torch.rand(256, generator=g) + 0.5).to(DEV), (0.1 * torch.randn(256, generator=g)).to(DEV))
    specs = [  # pc, x key, B, H, W, act, res, pre
        (mk(256, 256), 256, 5, 16, 16, 3, res, None), (mk(128, 256), 256, 5, 16, 16, 0, None, None),
        (mk(512, 256, 1, 2), 256, 5, 16, 16, 1, None, None), (mk(72, 512), 512, 3, 9, 7, 3, None, None),
        (mk(256, 64), 64, 70, 1, 1, 2, None, None),
        (mk(64, 256), 256, 5, 16, 16, 1, None, None),          # narrow tile: another class
        (mk(128, 256, 3), 256, 5, 16, 16, 1, None, None),      # 3x3: not a pointwise layer
        (mk(128, 256), 256, 5, 16, 16, 3, None, pre), (mk(256, 256), 256, 5, 16, 16, 3, None, pre),     # the PRE class: a group of its own
    ]

    def run(grouped, chain):
        eng = ConvEngine()
        eng.winograd = False
        eng.group_launches = grouped
        if chain:
            eng.chain_limit, eng.chain_in_kernel = 64, True
        kernels = []
        eng.hook = lambda phase, pc_, npix, st, has_res, kernel: kernels.append((kernel, getattr(pc_, "members", 1))) if phase == "begin" else None
        jobs = []
        for pc, xk, B, H, W, act, r, p in specs:
            Ho, Wo = (H + 2 * pc.pad - pc.KH) // pc.stride + 1, (W + 2 * pc.pad - pc.KW) // pc.stride + 1
            j = {"pc": pc, "x": xs[xk], "B": B, "H": H, "W": W, "relu": act, "out": torch.full((B, Ho, Wo, pc.Cout), float("nan"), device=DEV)}
            if r is not None:
                j["res"] = r
            if p is not None:
                j["pre"] = p
            jobs.append(j)
        eng.conv_group(L, jobs, _stream())
        torch.cuda.synchronize()
        return [j["out"] for j in jobs], kernels

    for chain in (False, True):
        a, ka = run(False, chain)
        b, kb = run(True, chain)
        assert all(k == ("conv_igemm_f32_kernel", 1) for k in ka) and len(ka) == len(specs)
        groups = sorted(m for k, m in kb if k == "conv_igemm_group_f32_kernel")
        # without blocks: the five wide plain layers together + the two PRE layers; with 64-float blocks the K = 64 layer keeps a
        # single chain (another class) and leaves the plain group
        assert groups == ([2, 4] if chain else [2, 5]), kb
        for i, (ta, tb) in enumerate(zip(a, b)):
            assert torch.isfinite(tb).all() and torch.equal(ta, tb), i
    # the C entry itself: mixed classes are refused before anything is launched
    d0 = _lib.ConvDesc(5, 16, 16, 256, 16, 16, 256, 1, 1, 1, 0, 256, 256, 0, 256, 0)
    d1 = _lib.ConvDesc(5, 16, 16, 256, 16, 16, 64, 1, 1, 1, 0, 256, 64, 0, 256, 0)
    assert L.hands_conv2d_group_class(C.byref(d0), 0) == 0 and L.hands_conv2d_group_class(C.byref(d1), 0) == 1
    out = torch.full((5, 16, 16, 256), float("nan"), device=DEV)
    arr = (_lib.ConvJob * 2)(_lib.ConvJob(C.pointer(d0), ptr(xs[256]), ptr(specs[0][0].w), ptr(specs[0][0].bias), None, ptr(out), None, None),
                             _lib.ConvJob(C.pointer(d1), ptr(xs[256]), ptr(specs[5][0].w), ptr(specs[5][0].bias), None, ptr(out), None, None))
    assert L.hands_conv2d_group_f32(arr, 2, _stream()) == 10001
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_handoccnet_forward_is_bit_identical_without_grouped_launches(hon_gpu):
    """The grouped launches of the forward (conv1 + downsample, the FPN laterals, the q / k / v projections, the hourglass branch
    pairs) are a launch schedule: every output equals the one-launch-per-layer forward bit for bit, at 3 and at 32 samples."""
    for bz in (3, 32):
        inputs, meta_info = synthetic_inputs(bz, 8, device=DEV)
        a = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
        hon_gpu.engine.group_launches = False
        try:
            b = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
        finally:
            hon_gpu.engine.group_launches = True
        for k in a:
            assert torch.equal(a[k], b[k]), (bz, k)


def test_handoccnet_crop_chunks_are_bit_identical(hon_gpu):
    """A forward that runs alone (``async_forward`` off) cuts its crops into ``chunks`` jobs from 128 crops on
    (streams.run_crop_chunks): bz = 64 as three uneven jobs of 42 / 43 / 43 crops returns every key bit for bit as one job."""
    inputs, meta_info = synthetic_inputs(64, 6, device=DEV)
    keep = hon_gpu.chunks
    hon_gpu.async_forward = False
    try:
        outs = {}
        for n in (1, 3):
            hon_gpu.chunks = n
            outs[n] = {k: v.clone() for k, v in hon_gpu(inputs, meta_info).items()}
    finally:
        hon_gpu.async_forward, hon_gpu.chunks = True, keep
    assert list(outs[3].keys()) == list(outs[1].keys()) and len(outs[1]) == 22
    for k in outs[1]:
        assert torch.equal(outs[3][k], outs[1][k]), k
