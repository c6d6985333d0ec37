"""Torch restatement of the reference's validation loss dict, for the tests and tools/bench_loss.py.

Restates ``compute_loss_light`` (src/callbacks/loss/loss_arctic_sf.py:20-206) with the helpers of
src/utils/loss_modules.py:97-152 and the weighting / total of src/models/generic/wrapper.py:19-23,100-115, dtype-generic:
``compute_loss_light(..., dtype=torch.float64)`` runs every float input in fp64.  tests/test_losses.py pins this file to the
real reference through tests/golden/loss_light.npz; nothing here is imported by the package.
"""
import math

import torch
import torch.nn.functional as F

BASE_KEYS = ["loss/mano/cam_t/r", "loss/mano/cam_t/l", "loss/mano/kp2d/r", "loss/mano/kp3d/r", "loss/mano/pose/r",
             "loss/mano/beta/r", "loss/mano/kp2d/l", "loss/mano/kp3d/l", "loss/mano/pose/l", "loss/mano/transl/l",
             "loss/mano/beta/l"]
ALL_KEYS = BASE_KEYS + ["loss/grasp/r", "loss/grasp/l", "loss/mask/r", "loss/mask/l", "loss/depth/r", "loss/depth/l",
                        "loss/center/r", "loss/center/l", "loss/corner/r", "loss/corner/l"]
WEIGHTS = dict(zip(ALL_KEYS, [1.0, 1.0, 5.0, 5.0, 10.0, 0.001, 5.0, 5.0, 10.0, 1.0, 0.001, 0.1, 0.1, 10.0, 10.0, 1.0, 1.0,
                              1.0, 1.0, 1.0, 1.0]))


def axis_angle_to_matrix(aa):
    """pytorch3d's axis_angle_to_matrix = quaternion_to_matrix(axis_angle_to_quaternion(.))."""
    ang = torch.norm(aa, p=2, dim=-1, keepdim=True)
    half = ang * 0.5
    small = ang.abs() < 1e-6
    s = torch.empty_like(ang)
    s[~small] = torch.sin(half[~small]) / ang[~small]
    s[small] = 0.5 - (ang[small] * ang[small]) / 48
    q = torch.cat([torch.cos(half), aa * s], dim=-1)
    r, i, j, k = torch.unbind(q, -1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(q.shape[:-1] + (3, 3))


def _vector_loss(p, g, valid):
    d = ((p - g) ** 2).reshape(p.shape[0], -1)
    if valid.sum() == 0:
        return torch.zeros_like(d)
    return d * valid[..., None]


def _joints_loss(p, g, jvalid):
    return ((p - g) ** 2) * jvalid[:, :, None]


def _get(args, k, d=None):
    return args.get(k, d) if hasattr(args, "get") else getattr(args, k, d)


def compute_loss_light(pred, gt, meta_info, args, dtype=None):
    """-> {key: (tensor of shape (1,), weight)} in the reference's key order."""
    def c(t):
        return t.to(dtype) if (dtype is not None and t.is_floating_point()) else t
    P = lambda k: c(pred[k])
    G = lambda k: c(gt[k])
    M = lambda k: c(meta_info[k]).to(P("mano.beta.r").dtype)[..., None]
    bz = meta_info["is_j2d_loss"].shape[0]
    fl = lambda k: G(k).to(P("mano.beta.r").dtype)
    valid = {"r": fl("right_valid"), "l": fl("left_valid")}
    t = {}
    for h in "rl":
        gt_rot = axis_angle_to_matrix(G(f"mano.pose.{h}").reshape(-1, 3)).reshape(-1, 16, 3, 3)
        t[f"pose/{h}"] = _vector_loss(P(f"mano.pose.{h}"), gt_rot, valid[h]) * M("is_pose_loss")
        t[f"beta/{h}"] = _vector_loss(P(f"mano.beta.{h}"), G(f"mano.beta.{h}"), valid[h]) * M("is_beta_loss")
        jv = fl(f"joints_valid_{h}")
        t[f"kp2d/{h}"] = _joints_loss(P(f"mano.j2d.norm.{h}"), G(f"mano.j2d.norm.{h}"), jv).reshape(bz, -1) * M("is_j2d_loss")
        p3, g3 = P(f"mano.j3d.cam.{h}"), G(f"mano.j3d.cam.{h}")
        t[f"kp3d/{h}"] = _joints_loss(p3 - p3[:, :1], g3 - g3[:, :1], jv).reshape(bz, -1) * M("is_j3d_loss")
        cam = _vector_loss(P(f"mano.cam_t.wp.{h}"), G(f"mano.cam_t.wp.{h}"), valid[h])
        cam = cam + _vector_loss(P(f"mano.cam_t.wp.init.{h}"), G(f"mano.cam_t.wp.{h}"), valid[h])
        t[f"cam_t/{h}"] = cam * M("is_cam_loss")
    t["transl/l"] = _vector_loss(P("mano.cam_t.wp.l") - P("mano.cam_t.wp.r"), G("mano.cam_t.wp.l") - G("mano.cam_t.wp.r"),
                                 valid["r"] * valid["l"]) * M("is_cam_loss")
    out = {k: (t[k[len("loss/mano/"):]].mean().view(-1), WEIGHTS[k]) for k in BASE_KEYS}

    def add(name, fn):
        for h in "rl":
            out[f"loss/{name}/{h}"] = (fn(h).mean().view(-1), WEIGHTS[f"loss/{name}/{h}"])
    if _get(args, "use_grasp_loss", False):
        add("grasp", lambda h: (F.cross_entropy(P(f"grasp.{h}"), gt[f"grasp.{h}"], reduction="none") *
                                fl(f"grasp_valid_{h}")).reshape(bz, -1) * M("is_grasp_loss"))
    if _get(args, "use_render_seg_loss", False):
        add("mask", lambda h: ((P(f"render.{h}") - G(f"render.{h}")).abs().reshape(bz, -1) *
                               fl(f"render_valid_{h}")[..., None]) * M("is_mask_loss"))
    if _get(args, "use_depth_loss", False):
        add("depth", lambda h: (P(f"depth.{h}") - G(f"depth.{h}")).abs().reshape(bz, -1) * M("is_depth_loss"))
    if _get(args, "regress_center_corner", False):
        add("center", lambda h: _vector_loss(P(f"center.{h}"), G(f"center.{h}"), valid[h]))
        add("corner", lambda h: _vector_loss(P(f"corner.{h}"), G(f"corner.{h}"), valid[h]))
    return out


def finish(loss_dict):
    """generic/wrapper.py:100-115: 0-dim weighted values and their sum under 'loss'."""
    out = {k: v.mean() * w for k, (v, w) in loss_dict.items()}
    total = 0.0
    for k in list(out):
        total = total + out[k]
    out["loss"] = total
    return out


def random_case(B, S_mask, S_depth, seed, device="cpu", switches=("grasp", "mask", "depth", "cc")):
    """Generated inputs in the layout compute_loss_light reads: (pred, gt, meta_info, args)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    flag = lambda *s, p=0.7: (ru(*s) < p).float()
    pred, gt, meta = {}, {}, {}
    for h in "rl":
        gt[f"mano.pose.{h}"] = 0.5 * rn(B, 48)
        pred[f"mano.pose.{h}"] = axis_angle_to_matrix((gt[f"mano.pose.{h}"] + 0.2 * rn(B, 48)).reshape(-1, 3)).reshape(B, 16, 3, 3)
        gt[f"mano.beta.{h}"] = rn(B, 10)
        pred[f"mano.beta.{h}"] = gt[f"mano.beta.{h}"] + 0.3 * rn(B, 10)
        gt[f"mano.j3d.cam.{h}"] = 0.1 * rn(B, 21, 3) + torch.tensor([0.0, 0.0, 0.6])
        pred[f"mano.j3d.cam.{h}"] = gt[f"mano.j3d.cam.{h}"] + 0.02 * rn(B, 21, 3)
        gt[f"mano.j2d.norm.{h}"] = 0.5 * rn(B, 21, 2)
        pred[f"mano.j2d.norm.{h}"] = gt[f"mano.j2d.norm.{h}"] + 0.1 * rn(B, 21, 2)
        gt[f"mano.cam_t.wp.{h}"] = rn(B, 3) + torch.tensor([8.0, 0.0, 0.0])
        pred[f"mano.cam_t.wp.{h}"] = gt[f"mano.cam_t.wp.{h}"] + 0.3 * rn(B, 3)
        pred[f"mano.cam_t.wp.init.{h}"] = gt[f"mano.cam_t.wp.{h}"] + 0.5 * rn(B, 3)
        gt[f"joints_valid_{h}"] = flag(B, 21, p=0.85)
        if "grasp" in switches:
            pred[f"grasp.{h}"] = 2.0 * rn(B, 9)
            gt[f"grasp.{h}"] = torch.randint(0, 9, (B,), generator=g)
            gt[f"grasp_valid_{h}"] = flag(B)
        if "mask" in switches:
            pred[f"render.{h}"] = ru(B, 1, S_mask, S_mask)
            gt[f"render.{h}"] = (ru(B, 1, S_mask, S_mask) < 0.3).float()
            gt[f"render_valid_{h}"] = flag(B)
        if "depth" in switches:
            pred[f"depth.{h}"] = 0.6 + 0.2 * rn(B, S_depth, S_depth)
            gt[f"depth.{h}"] = 0.6 + 0.2 * rn(B, S_depth, S_depth)
        if "cc" in switches:
            for nm, n in (("center", 2), ("corner", 8)):
                gt[f"{nm}.{h}"] = ru(B, n)
                pred[f"{nm}.{h}"] = gt[f"{nm}.{h}"] + 0.1 * rn(B, n)
    gt["is_valid"] = flag(B, p=0.9)
    gt["right_valid"], gt["left_valid"] = flag(B), flag(B)
    for k in ("cam", "j2d", "j3d", "pose", "beta", "grasp", "mask", "depth"):
        meta[f"is_{k}_loss"] = flag(B, p=0.8)
    args = {"use_grasp_loss": "grasp" in switches, "use_render_seg_loss": "mask" in switches,
            "use_depth_loss": "depth" in switches, "regress_center_corner": "cc" in switches}
    mv = lambda d: {k: v.to(device) for k, v in d.items()}
    return mv(pred), mv(gt), mv(meta), args


def load_fixture(path):
    """tests/golden/loss_light.npz (written by tests/golden/make_golden_loss.py from the real reference) ->
    ({case: {"pred", "gt", "meta", "args", "keys", "weights", "ref" (list of fp32 (1,) arrays), "d_ref", "d_threads"}}, epoch)."""
    import json
    import numpy as np
    d = np.load(path)
    info = json.loads(str(d["meta"]))
    groups = ("pred", "gt", "meta")
    base = {g: {k[len(f"base/{g}."):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(f"base/{g}.")} for g in groups}
    cases = {}
    for name, ci in info["cases"].items():
        c = {"args": ci["args"], "keys": ci["keys"], "weights": ci["weights"], "d_ref": ci["d_ref"], "d_threads": ci["d_threads"]}
        for g in groups:
            t = dict(base[g])
            pre = f"case/{name}/{g}."
            t.update({k[len(pre):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(pre)})
            c[g] = {k: (v[:ci["slice"]] if ci["slice"] else v) for k, v in t.items()}
        c["ref"] = [d[f"case/{name}/out/{i}"] for i in range(len(ci["keys"]))]
        cases[name] = c
    ep = info["epoch"]
    steps = []
    for i in range(ep["steps"]):
        od = {"imgname": ep["imgnames"][i]}
        pre = f"epoch/step{i}/out_dict/"
        od.update({k[len(pre):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(pre)})
        pre = f"epoch/step{i}/loss/"
        steps.append({"out_dict": od, "loss": {k[len(pre):]: torch.from_numpy(d[k]) for k in d.files if k.startswith(pre)}})
    expect = {k[len("epoch/out/"):]: float(d[k]) for k in d.files if k.startswith("epoch/out/")}
    return cases, {"steps": steps, "expect": expect}


def check_against_reference(case, got, what):
    """got: {key: (tensor (1,), weight)}.  Same keys, order and weights; exact zeros and NaN positions equal; the rest within
    4 x d_ref of the case."""
    assert list(got) == case["keys"], what
    rtol = 4.0 * case["d_ref"]
    for k, w, ref in zip(case["keys"], case["weights"], case["ref"]):
        v, gw = got[k]
        assert tuple(v.shape) == (1,) and v.dtype == torch.float32 and gw == w, (what, k)
        x, r = float(v[0]), float(ref[0])
        print(f"{what} {k}: got {x!r} ref {r!r} rel {abs(x - r) / abs(r) if r not in (0.0,) and math.isfinite(r) else 0.0:.3g} (rtol {rtol:.3g})")
        if math.isnan(r):
            assert math.isnan(x), (what, k, x)
        elif r == 0.0:
            assert x == 0.0, (what, k, x)
        else:
            assert abs(x - r) <= rtol * abs(r), (what, k, x, r, rtol)
