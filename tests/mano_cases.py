"""Inputs of the MANO edge tests (tests/test_gpu_mano_edges.py) and of the CPU pins of ``kernel_refs.mano_head_ref``
(tests/test_kernel_refs.py): a general intrinsic matrix, rotations at the places the conversions switch formula, tip vertices
at chunk edges, an asset whose skinning weights are all non-zero.  A plain module; nothing here is imported by the package."""
import copy
import math

import numpy as np
import torch

from hands_amd.mano import synthetic_mano_asset
from oracle import hands_oracle as O

# chunk = vertex // 64 of the fused kernel: vertex 0 (first of chunk 0), 63 | 64 (a chunk boundary), 767 (last of chunk 11),
# 777 (the last vertex, in chunk 12, the short last chunk)
EDGE_TIPS = (0, 63, 64, 767, 777)
ROT_KINDS = ("identity", "theta=1e-7", "theta=pi-1e-4", "theta=pi", "random")


def general_K(B, g):
    """(B, 3, 3): fx and fy vary independently, a skew and its (different) transpose entry of a few pixels, a last row that is
    not (0, 0, 1): K20, K21 about +-1e-3 and K22 in [0.95, 1.05]."""
    rn = lambda: torch.randn(B, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1] = 1000.0 + 20.0 * rn(), 950.0 + 30.0 * rn()
    K[:, 0, 1], K[:, 1, 0] = 3.0 + rn(), -2.0 + 0.5 * rn()
    K[:, 0, 2], K[:, 1, 2] = 112.0 + 5.0 * rn(), 100.0 + 5.0 * rn()
    K[:, 2, 0], K[:, 2, 1] = 1e-3 * (1.0 + 0.1 * rn()), -1e-3 * (1.0 + 0.1 * rn())
    K[:, 2, 2] = 0.95 + 0.1 * torch.rand(B, generator=g)
    return K


def axis_angles(B, g, seed=0):
    """(B, 48) float32 axis-angle rows: hand i < 4 is of kind ROT_KINDS[(i + seed) % 5] in all 16 joints -- identity, an angle
    of 1e-7 (under the 1e-6 switch to the series), pi - 1e-4 and pi (about an axis whose largest component is unambiguous, so the
    quaternion branch does not depend on rounding) --, every other hand is random with angles up to ~2."""
    aa = 0.6 * torch.randn(B, 16, 3, generator=g, dtype=torch.float64)
    ax = torch.tensor([3.0, -2.0, 1.0], dtype=torch.float64)
    ax = ax / ax.norm()
    for i in range(min(B, 4)):
        kind = ROT_KINDS[(i + seed) % 5]
        if kind == "identity":
            aa[i] = 0.0
        elif kind == "theta=1e-7":
            aa[i] = 1e-7 * ax
        elif kind == "theta=pi-1e-4":
            aa[i] = (math.pi - 1e-4) * ax
        elif kind == "theta=pi":
            aa[i] = math.pi * ax
    return aa.reshape(B, 48).float()


def inputs(B, seed, sigma=1.0):
    """-> rot (B,16,3,3), aa (B,48), betas (B,10) ~ sigma N(0,1), cam (B,3), K (B,3,3), float32.  ``rot`` is the float32 matrix
    of ``aa`` (evaluated in float64): the matrix entries and the axis-angle entries describe the same poses, not the same bits."""
    g = torch.Generator().manual_seed(seed)
    aa = axis_angles(B, g, seed)
    rot = O.axis_angle_to_matrix(aa.double().reshape(-1, 3)).reshape(B, 16, 3, 3).float()
    betas = sigma * torch.randn(B, 10, generator=g)
    cam = torch.tensor([1.0, 0.0, 0.0]) + 0.1 * torch.randn(B, 3, generator=g)
    return rot, aa, betas, cam, general_K(B, g)


def dense_weight_asset(is_rhand=True):
    """The synthetic asset with all 16 skinning weights of every vertex non-zero (rows still sum to 1)."""
    a = copy.deepcopy(synthetic_mano_asset(is_rhand))
    rng = np.random.RandomState(42 if is_rhand else 43)
    w = 0.05 + rng.rand(*a.lbs_weights.shape)
    a.lbs_weights = (w / w.sum(1, keepdims=True)).astype(np.float32)
    assert (a.lbs_weights > 0).all()
    return a.validate()


def mano_head_loops(aa, betas, cam, K, asset, img_res, min_s, tip_ids):
    """MANOHead.forward written out per hand, joint and vertex in float64 numpy, from axis-angle rows: an evaluation that
    shares no batched statement with ``kernel_refs.mano_head_ref``.  -> vertices, joints3d, j3d.cam, j2d.norm, cam_t."""
    f8 = lambda a: np.asarray(a, dtype=np.float64)
    aa, betas, cam, K = (f8(t.detach().cpu().numpy()) for t in (aa, betas, cam, K))
    vt, sd, pd, Jr, W = f8(asset.v_template), f8(asset.shapedirs), f8(asset.posedirs), f8(asset.J_regressor), f8(asset.lbs_weights)
    mean = np.concatenate([np.zeros(3), f8(asset.hands_mean)])
    B = aa.shape[0]
    out = {k: np.zeros(s) for k, s in (("vertices", (B, 778, 3)), ("joints3d", (B, 21, 3)), ("j3d.cam", (B, 21, 3)),
                                        ("j2d.norm", (B, 21, 2)), ("cam_t", (B, 3)))}
    for b in range(B):
        R = []
        for j in range(16):                                  # smplx batch_rodrigues: theta = |r + 1e-8|
            r = aa[b, 3 * j:3 * j + 3] + mean[3 * j:3 * j + 3]
            th = math.sqrt(sum((x + 1e-8) ** 2 for x in r))
            k = r / th
            Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
            R.append(np.eye(3) + math.sin(th) * Kx + (1.0 - math.cos(th)) * (Kx @ Kx))
        feat = np.concatenate([(R[j] - np.eye(3)).reshape(-1) for j in range(1, 16)])
        v_shaped = np.array([[vt[v, c] + sum(sd[v, c, l] * betas[b, l] for l in range(10)) for c in range(3)] for v in range(778)])
        v_posed = v_shaped + (feat @ pd).reshape(778, 3)
        J = Jr @ v_shaped
        G = [None] * 16
        for j in range(16):
            p = O.PARENTS[j]
            loc = np.eye(4)
            loc[:3, :3], loc[:3, 3] = R[j], (J[j] if p < 0 else J[j] - J[p])
            G[j] = loc if p < 0 else G[p] @ loc
        A = []
        for j in range(16):
            a = G[j].copy()
            a[:3, 3] = G[j][:3, 3] - G[j][:3, :3] @ J[j]
            A.append(a)
        for v in range(778):
            T = np.zeros((4, 4))
            for j in range(16):
                T += W[v, j] * A[j]
            out["vertices"][b, v] = T[:3, :3] @ v_posed[v] + T[:3, 3]
        s = max(cam[b, 0], min_s)
        ct = np.array([cam[b, 1], cam[b, 2], 2.0 * ((K[b, 0, 0] + K[b, 1, 1]) / 2.0) / (img_res * s + 1e-9)])
        out["cam_t"][b] = ct
        for j in range(21):
            X = G[j][:3, 3] if j < 16 else out["vertices"][b, tip_ids[j - 16]]
            out["joints3d"][b, j] = X
            Xc = X + ct
            out["j3d.cam"][b, j] = Xc
            h = K[b] @ Xc
            out["j2d.norm"][b, j] = [2.0 * (h[0] / h[2]) / img_res - 1.0, 2.0 * (h[1] / h[2]) / img_res - 1.0]
    return {k: torch.from_numpy(v) for k, v in out.items()}
