"""``HandsLight`` -- the WildHands forward path on MI355X, behind the reference's module API.

Same constructor, ``forward(inputs, meta_info) -> xdict`` contract, 22 output keys and
``state_dict`` names as the reference model (src/models/hands_light/model.py:15-437), but every
statement of ``forward`` runs as a hand-written gfx950 kernel from ``libhands_hip.so``:

    statement (model.py)                      kernel (include/hands_hip.h)
    :193,238-239  ResNet-50 trunks            hands_stem_conv_maxpool_nchw_f32 (conv1 + bn1 + relu + max-pool from the NCHW image),
                                              hands_conv2d_nhwc_f32 / hands_conv1x1_dual_nhwc_f32 (fp32 MFMA implicit GEMM, BN
                                              folded, bias / residual / ReLU epilogue), hands_conv3x3_winograd4_f32 (the 3x3 /
                                              stride-1 layers as Winograd F(4x4,3x3); hands_conv3x3_winograd_f32 = F(2x2) fallback)
    :196          sum-pool                    hands_sumpool_nhwc_f32
    :258-271      KPE + concat                hands_kpe_concat_f32
    :313-314      feature_conv                hands_conv2d_nhwc_f32 x4
    :320-321      HandHMR x2                  hands_conv2d_nhwc_f32 (cam_init, 3 x refine+decoders),
                                              hands_hmr_init_f32, hands_rot6d_to_matrix_f32
    :341-368      is_flipped swap             hands_flip_swap_f32 (per sample, no host sync)
    :378-390      MANOHead x2                 hands_mano_heads_f32 (both hands, one launch; the three-launch chain
                                              hands_mano_pose_f32 -> blend GEMM -> hands_mano_skin_f32 is its cross-check)
    :401-404      grasp classifier            hands_grasp_input_f32, hands_conv2d_nhwc_f32 x4

    :194-195,233-242,483-493  ViT-B/16 trunks (backbone='vit_b_16') hands_conv2d_nhwc_f32 (conv_proj 16x16/s16, qkv, out_proj +
                                              residual, fc1 + GELU, fc2 + residual), hands_vit_tokens_f32 (class token + position
                                              embedding), hands_layernorm_f32 (C = 768), hands_attention_f32 (197 tokens, 12 x 64),
                                              hands_vit_tail_f32 (encoder.ln + AvgPool2d(2)), vit_conv as one folded 3x3 layer

    hmr_layer.py:17-42, 67-86  transformer head (tf_decoder=True)   hands_vector_tokens_f32 (109 scalar tokens), hands_wide_attention_f32
                                              (one head of dimension 1024: tokens x tokens, tokens x 49 pixels), hands_token_mean_f32,
                                              every Linear on hands_conv2d_nhwc_f32 (bias / ReLU / residual epilogue); feature_conv
                                              is not run

torch is used for parameter containers, device buffers and streams only.  Built configurations: backbones resnet50 and vit_b_16,
tf_decoder=False with every pos_enc of model.py -- 'center+corner_latent' (shipped default), 'sinusoidal_cc', 'center', 'corner',
'center+corner', 'dense', 'dense_latent', 'cam_conv', 'pcl', 'perspective_correction', None -- ``no_crops`` (arctic_light), the
grasp head with / without the global feature vector or absent, ``separate_hands``, ``regress_center_corner``,
``use_glb_feat=False``, ``use_depth_loss`` (the depth head); the constructor keyword tf_decoder=True with pos_enc 'center+corner_latent', 'dense_latent' or
None (the reference itself fails on tf_decoder with 'sinusoidal_cc', 'cam_conv', ``no_crops`` or ``regress_center_corner``);
backbone='resnet18' and the renderer switch raise ``NotImplementedError``.

This file is the model: its defaults, constructor switches, packing and forward orchestration, workspaces and streams.  The
trunks are ``resnet50.py`` / ``vit_b16.py``, the HandHMR heads (iterative ``iter_head``, transformer ``tf_head``) and the depth
head ``hmr_head.py``, the MANO head ``mano_head.py``, the grasp classifier ``grasp_head.py``, chains of per-sample linear
layers ``engine.linear_chain``, the fork / join of side-stream jobs ``streams.py``.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import _lib
from ._lib import check, ptr
from .engine import DEFAULT_ENGINE, ConvEngine, EngineSwitches, linear_chain
from .grasp_head import GRASP_SPLITK, pack_grasp_head, run_grasp_head
from .hmr_head import TF_PASS, HandHMR, depth_head, iter_head, pack_hmr_head, tf_head
from .mano_head import MANOHead, ManoHeadsPlan, pack_mano_pair, run_mano_heads  # noqa: F401  (ManoHeadsPlan: importable from here)
from .packing import HMR_VEC, pack_conv, pack_linear
from .resnet50 import ResNet50Params, pack_resnet50_trunk, resnet50_trunk
from .streams import SideJobs
from .vit_b16 import ViTB16Params, pack_vit_b16_trunk, vit_b16_trunk, vit_conv_params
from .xdict import _Args, args_getter, stream_xdict, xdict

BACKBONES = ("resnet50", "vit_b_16")      # model.py:19-31 also names resnet18: not built

LATENT_ENC = ("center+corner_latent", "sinusoidal_cc")
IMAGE_ENC = {"center": 1, "corner": 2, "center+corner": 3}     # -> mode of hands_image_posenc_nhwc_f32

DEFAULT_ARGS = _Args(backbone="resnet50", pos_enc="center+corner_latent", n_freq_pos_enc=4,
                     use_glb_feat=True, separate_hands=False, tf_decoder=False, use_grasp_loss=True,
                     use_glb_feat_w_grasp=True, no_crops=False, use_depth_loss=False,
                     regress_center_corner=False, use_render_seg_loss=False, img_res=224,
                     focal_length=1000.0)


# --------------------------------------------------------------------------------------------------
class _PackedHolder:
    """Packed (kernel-layout) weights of one parameter set, shared by a model and its replicas: any of them
    invalidating it (load_state_dict, .to(), invalidate_packed) makes all of them repack on the next forward."""

    def __init__(self):
        self.packed, self.dev, self.version = None, None, 0

    def invalidate(self):
        self.packed = None
        self.version += 1


class HandsLight(EngineSwitches, nn.Module):
    def __init__(self, backbone="resnet50", focal_length=1000.0, img_res=224, args=None,
                 mano_assets=None, tf_decoder=False):
        super().__init__()
        self.engine = ConvEngine()
        # Winograd F(4x4,3x3) (csrc/conv_wino4.hip, 2.25 multiplications per output) for the stride-1 3x3 convolutions of these
        # ResNet stages; the others keep F(2x2,3x3).  Round 5, one box, alternating: alone on the chip a launch takes the time of its
        # F(2x2) twin (layers 1-3) or 9 % less (layer 4), but it spends ~45 % fewer matrix-pipe cycles, and in the shipped multi-stream
        # mode that is +1.6 % on the forward with all four stages (+0.4 % with stage 4 only); end-to-end error over 200 random inputs
        # unchanged (median 2.4e-7 m, max 4.4e-7 against 2.5e-7 / 4.9e-7 with F(2x2): tools/hl_parity_sweep.py).  A packing-time
        # choice (36 Cout Cin floats per layer, 130 MB per trunk): call invalidate_packed() after changing it; engine.winograd4 = False
        # falls back to F(2x2) without repacking.
        self.winograd4_stages = (1, 2, 3, 4)
        self.engine.winograd4 = True
        self.trunk_chunks = (1, 2)    # (global, hand) trunk jobs, one HIP stream each (ViT-B/16: (1, 1), set below)
        self.async_tail = True        # tail of the forward on its own stream, joined at first use of the result
        self._calls = 0
        args = args if args is not None else DEFAULT_ARGS
        get = args_getter(args)
        self.args = args
        if backbone not in BACKBONES:
            raise NotImplementedError(f"hands_amd.HandsLight: backbone={backbone!r} is not built (built: {BACKBONES})")
        self.backbone_name = backbone
        # Configuration switches (model.py:33-157).  Built: the latent KPE ('center+corner_latent', and 'sinusoidal_cc' whose
        # forward is the same code, model.py:258-271 / 288-304), the image-level encodings 'center' / 'corner' /
        # 'center+corner' (extra input channels of the hand trunk's conv1, model.py:60-77, 203-218), no encoding (None),
        # `no_crops` (both heads read the pooled global features, model.py:199-201, 316-318: the arctic_light configuration),
        # the grasp head with and without the global feature vector, or absent.
        pos_enc = get("pos_enc")
        self.pos_enc = pos_enc
        # 'dense' (per-pixel angle maps as extra conv1 channels, model.py:220-224), 'dense_latent' / 'cam_conv' (the maps resized
        # to the 7x7 feature map and concatenated, :244-256 / :276-288), 'pcl' / 'perspective_correction' (no encoding; the global
        # rotation is corrected after the heads, :330-334 / :370-376)
        self.enc_mode = ("latent" if pos_enc in LATENT_ENC else "image" if pos_enc in IMAGE_ENC else
                         "dense" if pos_enc == "dense" else "dense_latent" if pos_enc in ("dense_latent", "cam_conv") else
                         "none" if pos_enc in (None, "pcl", "perspective_correction") else None)
        self.rot_fix = {"pcl": 1, "perspective_correction": 2}.get(pos_enc, 0)
        self.use_depth_loss = bool(get("use_depth_loss", False))
        self.img_res_ds = int(get("img_res_ds", img_res) or img_res)
        self.no_crops = bool(get("no_crops", False))
        self.use_grasp_loss = bool(get("use_grasp_loss", False))
        self.use_glb_feat_w_grasp = bool(get("use_glb_feat_w_grasp", False))
        self.separate_hands = bool(get("separate_hands", False))       # model.py:40-50: own trunk weights per side
        self.regress_center_corner = bool(get("regress_center_corner", False))   # model.py:157-172, 426-433
        self.use_glb_feat = bool(get("use_glb_feat", False))
        # tf_decoder (model.py:34-38, 312-314): feature_conv is skipped and both heads read the concatenated 7x7 map through the
        # transformer head (hmr_layer.py:17-42, 67-86) -- ``hmr_head.tf_head``
        # The switch is the constructor's keyword ``tf_decoder=True``, like ``backbone``.  ``args.tf_decoder`` alone keeps raising
        # NotImplementedError, as it always has here: a caller who hands over the reference's args gets the head only by asking
        # for it by name.
        self.tf_decoder = bool(tf_decoder)
        self.tf_pass = TF_PASS     # samples per pass of the transformer head (results do not depend on it)
        tf = self.tf_decoder
        unsupported = {
            f"pos_enc={pos_enc!r}": self.enc_mode is None,
            # the reference itself fails on these: feat_mlp / cam_init_precursor are built feat_dim wide for every encoding but
            # 'center+corner_latent' and 'dense_latent' (hmr_layer.py:26-31, hand_hmr.py:22-27) and then meet the 2128 / 2054
            # channel map ("mat1 and mat2 shapes cannot be multiplied"); the pooled vector of no_crops has no (h, w) to unpack
            # (hmr_layer.py:74); center_head meets the 4-D map (model.py:431)
            "args.tf_decoder (the transformer head is built: ask for it with HandsLight(..., tf_decoder=True))":
                bool(get("tf_decoder", False)) and not tf,
            "tf_decoder with sinusoidal_cc": tf and pos_enc == "sinusoidal_cc",
            "tf_decoder with cam_conv": tf and pos_enc == "cam_conv",
            "tf_decoder with no_crops": tf and self.no_crops,
            "tf_decoder with regress_center_corner": tf and self.regress_center_corner,
            # runs in the reference, not checked against it here: no fixture
            f"tf_decoder with pos_enc={pos_enc!r} (checked: 'center+corner_latent', 'dense_latent', None)":
                tf and pos_enc not in ("center+corner_latent", "dense_latent", None, "sinusoidal_cc", "cam_conv"),
            "use_depth_loss with no_crops": self.use_depth_loss and self.no_crops,      # `depth_r` undefined in the reference (:308-310, 422)
            "use_render_seg_loss (call hands_amd.MANORenderer on the output instead)": bool(get("use_render_seg_loss", False)),
            # the reference itself fails on these combinations (`features` / `feat_vec` undefined, model.py:191-201, 402-404;
            # center_head on a 4-D map, :428)
            "use_glb_feat=False with no_crops": not self.use_glb_feat and self.no_crops,
            "use_glb_feat=False with use_glb_feat_w_grasp": (not self.use_glb_feat and self.use_grasp_loss and self.use_glb_feat_w_grasp),
            "regress_center_corner with no_crops": self.regress_center_corner and self.no_crops,
            # (model.py:72-73 hands conv_proj's bias TENSOR to nn.Conv2d(bias=...): "Boolean value of Tensor ... is ambiguous")
            "separate_hands with a widened conv_proj on vit_b_16": (backbone == "vit_b_16" and self.separate_hands
                                                                    and self.enc_mode in ("image", "dense")),
        }
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            raise NotImplementedError(f"hands_amd.HandsLight: unsupported config switches {bad}")
        self.n_freq = int(get("n_freq_pos_enc", 4))
        feat_dim = 2048
        self.feat_dim = feat_dim
        vit = backbone == "vit_b_16"
        Trunk = ViTB16Params if vit else ResNet50Params
        self.backbone = Trunk()               # (the reference builds it even with use_glb_feat = False: same state_dict keys)
        if vit:                               # model.py:25-29: the tail that turns the 14x14 tokens into (2048, 7, 7) features
            self.vit_conv = vit_conv_params()
            # the 2 bz crops stay ONE job: its GEMMs have 394 bz rows (fc1: x 3072 columns), enough tiles to fill the chip alone
            self.trunk_chunks = (1, 1)
        # model.py:60-77: conv1 of the hand trunk takes the image-level encoding as extra input channels
        self.enc_channels = ({1: 4, 2: 16, 3: 20}[IMAGE_ENC[pos_enc]] * self.n_freq if self.enc_mode == "image" else
                             4 * self.n_freq if self.enc_mode == "dense" else 0)
        # (ViT: `conv_proj` is what is widened, model.py:45-58, 71-78; every hand trunk has its own vit_conv)
        if self.separate_hands:
            self.hand_backbone_r = Trunk(3 + self.enc_channels)
            self.hand_backbone_l = Trunk(3 + self.enc_channels)
            if vit:
                self.hand_backbone_r_vit_conv = vit_conv_params()
                self.hand_backbone_l_vit_conv = vit_conv_params()
        else:
            self.hand_backbone = Trunk(3 + self.enc_channels)
            if vit:
                self.hand_backbone_vit_conv = vit_conv_params()
        self.latent_channels = (5 * 4 * self.n_freq if self.enc_mode == "latent" else 4 * self.n_freq if pos_enc == "dense_latent" else
                                6 if pos_enc == "cam_conv" else 0)
        fc_dim = feat_dim + self.latent_channels                                           # model.py:79-88
        # (tf_decoder: feat_mlp and cam_init_precursor take the concatenated map, hmr_layer.py:26-31 / hand_hmr.py:22-27)
        self.head_r = HandHMR(feat_dim, True, 3, tf_in=fc_dim if tf else None)
        self.head_l = HandHMR(feat_dim, False, 3, tf_in=fc_dim if tf else None)
        self.feature_conv = nn.Sequential(
            nn.Conv2d(fc_dim, 1024, 1, bias=False), nn.ReLU(inplace=True),
            nn.Conv2d(1024, 512, 3, bias=False), nn.ReLU(inplace=True),
            nn.Conv2d(512, 256, 3, bias=False), nn.ReLU(inplace=True),
            nn.Flatten(), nn.Linear(256 * 3 * 3, feat_dim), nn.ReLU(inplace=True))
        assets = mano_assets or (None, None)
        self.mano_r = MANOHead(True, focal_length, img_res, assets[0])
        self.mano_l = MANOHead(False, focal_length, img_res, assets[1])
        if self.use_grasp_loss:                                                            # model.py:113-125
            gdim = 10 + 144 + (feat_dim if self.use_glb_feat_w_grasp else 0)
            self.grasp_classifier = nn.Sequential(
                nn.Linear(gdim, 1024), nn.ReLU(inplace=True), nn.Linear(1024, 512),
                nn.ReLU(inplace=True), nn.Linear(512, 128), nn.ReLU(inplace=True), nn.Linear(128, 9))
        if self.use_depth_loss:                                                            # model.py:133-155
            cv = lambda i, o: nn.Conv2d(i, o, 3, 1, 1)
            up = lambda k: nn.Upsample(scale_factor=k, mode="bilinear", align_corners=True)
            self.depth_mlp = nn.Sequential(
                cv(fc_dim + 2, 256), nn.ReLU(True), cv(256, 256), nn.ReLU(True), up(4), cv(256, 128), nn.ReLU(True),
                cv(128, 128), nn.ReLU(True), up(4), cv(128, 64), nn.ReLU(True), cv(64, 32), nn.ReLU(True), up(2),
                cv(32, 16), nn.ReLU(True), cv(16, 1))
        if self.regress_center_corner:
            mk = lambda n: nn.Sequential(nn.Linear(feat_dim, 512), nn.ReLU(inplace=True), nn.Linear(512, 128),
                                         nn.ReLU(inplace=True), nn.Linear(128, n))
            self.corner_head = mk(8)
            self.center_head = mk(2)
        self.mode = "train"
        self.img_res = img_res
        self.focal_length = focal_length
        self._holder = _PackedHolder()
        self._ws = {}
        self.register_load_state_dict_post_hook(lambda m, k: m.invalidate_packed())

    # ---- packing ------------------------------------------------------------------------------
    @property
    def _packed(self):
        return self._holder.packed

    def invalidate_packed(self):
        """Drop the packed weights (shared with every replica): call after writing parameters IN PLACE
        (``load_state_dict`` and ``.to()`` do it themselves; ``apply_recipe`` calls it)."""
        self._holder.invalidate()
        if any(isinstance(v, torch.Tensor) and v.is_cuda for v in self._ws.values()):
            torch.cuda.synchronize()      # an asynchronous tail of an earlier forward may still use the workspaces
        self._ws = {}

    def _apply(self, fn, *a, **k):
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    @torch.no_grad()
    def _pack(self, dev):
        cpu = lambda t: t.detach().cpu()
        F = self.feat_dim
        P = {"head_r": pack_hmr_head(self.head_r, dev, F, self.tf_decoder), "head_l": pack_hmr_head(self.head_l, dev, F, self.tf_decoder)}
        if self.backbone_name == "vit_b_16":
            pack_trunk = lambda name: pack_vit_b16_trunk(getattr(self, name), getattr(self, "vit_conv" if name == "backbone" else name + "_vit_conv"), dev)
        else:
            pack_trunk = lambda name: pack_resnet50_trunk(getattr(self, name), dev, self.winograd4_stages)
        if self.use_glb_feat:
            P["backbone"] = pack_trunk("backbone")
        if not self.no_crops:
            if self.separate_hands:
                P["hand_backbone_r"] = pack_trunk("hand_backbone_r")
                P["hand_backbone_l"] = pack_trunk("hand_backbone_l")
            else:
                P["hand_backbone"] = pack_trunk("hand_backbone")
        if self.regress_center_corner:
            for nm, head in (("cc_center", self.center_head), ("cc_corner", self.corner_head)):
                P[nm] = [pack_linear(cpu(head[0].weight), cpu(head[0].bias), dev), pack_linear(cpu(head[2].weight), cpu(head[2].bias), dev),
                         pack_linear(cpu(head[4].weight), cpu(head[4].bias), dev, n_total=8)]
        fc = self.feature_conv
        # 'dense_latent' / 'cam_conv': the concatenated map is stored with its channel count padded to a multiple of 16 (zeros)
        if not self.tf_decoder:      # (tf_decoder: feature_conv keeps its parameters and is never run, model.py:312-314)
            P["fc0"] = pack_conv(cpu(fc[0].weight), None, 1, 0, dev,
                                 cin_pad_to=self._cat_ld() if self.enc_mode == "dense_latent" else None)
        if self.use_depth_loss:
            dm = self.depth_mlp
            P["depth"] = [pack_conv(cpu(dm[i].weight), cpu(dm[i].bias), 1, 1, dev,
                                    cin_pad_to=self._depth_ld() if i == 0 else None) for i in (0, 2, 5, 7, 10, 12, 15, 17)]
            lin = torch.linspace(-1, 1, 7)                                # model.py:172-175 (`init_grid`, 'ij' meshgrid)
            xg, yg = torch.meshgrid(lin, lin, indexing="ij")
            P["depth_grid"] = torch.stack([xg, yg], dim=-1).reshape(49, 2).contiguous().to(dev)
        if not self.tf_decoder:
            P["fc2"] = pack_conv(cpu(fc[2].weight), None, 1, 0, dev)
            P["fc4"] = pack_conv(cpu(fc[4].weight), None, 1, 0, dev)
            # nn.Flatten on NCHW (B,256,3,3): reference column c*9 + hw; NHWC buffer column hw*256 + c
            col = [(k % 9) * 256 + (k // 9) for k in range(256 * 9)]
            P["fc7"] = pack_linear(cpu(fc[7].weight), cpu(fc[7].bias), dev, col_index=col)
        if self.use_grasp_loss:
            P["grasp"] = pack_grasp_head(self.grasp_classifier[0::2], dev, F if self.use_glb_feat_w_grasp else 0)
        P["mano_r"], P["mano_l"] = pack_mano_pair(self.mano_r, self.mano_l, dev)
        return P

    def _cat_ld(self):
        """Row length of the map feature_conv reads (model.py:79-88): F + encoding channels, padded to 16 for the per-pixel modes."""
        n = self.feat_dim + self.latent_channels
        return (n + 15) // 16 * 16 if self.enc_mode == "dense_latent" else n

    def _depth_ld(self):
        return (self.feat_dim + self.latent_channels + 2 + 15) // 16 * 16

    def replica(self):
        """A second handle on the SAME parameters and packed weights with its own workspaces, side
        streams and engine switches, for a second request stream: two forwards in flight (one per torch
        stream, one replica each) overlap the tail of one with the trunks of the other.  Plain PyTorch
        stream semantics: each forward's outputs are valid on the stream it was called on.  The packed
        weights live in a holder both share, so ``load_state_dict`` / ``.to()`` / ``invalidate_packed`` on
        either one is seen by both."""
        self.packed(next(self.parameters()).device)
        import copy
        r = copy.copy(self)
        r._ws = {}
        r.engine = self.engine.clone_settings()
        return r

    def packed(self, dev):
        h = self._holder
        if h.packed is None or h.dev != dev:
            h.packed, h.dev = self._pack(dev), dev
        return h.packed

    # ---- buffers ------------------------------------------------------------------------------
    def _side_stream(self, dev, name="side_stream"):
        st = self._ws.get(name)
        if st is None or st.device != dev:
            st = torch.cuda.Stream(device=dev)
            self._ws[name] = st
        return st

    def _buf(self, name, numel, dev):
        t = self._ws.get(name)
        if t is None or t.numel() < numel or t.device != dev:
            if t is not None and t.is_cuda:
                # a workspace is being replaced (larger batch): an asynchronous tail or a side stream of an earlier
                # forward may still be using the old block, which the allocator would hand out again at once
                torch.cuda.synchronize(t.device)
            t = torch.empty(numel, dtype=torch.float32, device=dev)
            self._ws[name] = t
        return t

    # ---- kernel launch helpers ----------------------------------------------------------------
    # model-less launch helpers on the default engine (tests / tools driving a single layer)
    _conv = staticmethod(lambda *a, **kw: DEFAULT_ENGINE.conv(*a, **kw))
    _conv_dual = staticmethod(lambda *a, **kw: DEFAULT_ENGINE.conv_dual(*a, **kw))

    def _trunk(self, L, P, segs, B, res_in, stream, tag, cap_B, out=None, out_off=0):
        """One trunk job on this model's engine and workspaces: ``resnet50_trunk``, or ``vit_b16_trunk`` for a ViT-B/16
        parameter set (same contract): B images as NCHW segments -> (B,7,7,2048) features."""
        dev = segs[0][0].device
        trunk = vit_b16_trunk if "vit" in P else resnet50_trunk
        return trunk(self.engine, lambda name, numel: self._buf(name, numel, dev), L, P, segs, B, res_in, stream, tag, cap_B, out, out_off)

    # ---- forward ------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, inputs, meta_info):
        L = _lib.lib()
        img = inputs["img"]
        dev = img.device
        if dev.type != "cuda":
            raise RuntimeError("hands_amd.HandsLight runs on a HIP device only (no CPU fallback); "
                               "move the module and its inputs to 'cuda'")
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
        img, r_img, l_img = f32(img), f32(inputs["r_img"]), f32(inputs["l_img"])
        K = f32(meta_info["intrinsics"])
        assert K.shape[1:] == (3, 3)                               # transforms.py:322-326
        bz, c, res, res_w = img.shape
        assert c == 3 and res == res_w and r_img.shape == img.shape and l_img.shape == img.shape
        B2 = 2 * bz
        F = self.feat_dim
        P = self.packed(dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        buf = lambda n, numel: self._buf(n, numel, dev)

        # -- trunks (model.py:193, 238-239).  r and l crops share `hand_backbone`, so the 2*bz crops
        #    are one batch; the 3*bz trunk passes are cut into `trunk_chunks` jobs that run on separate
        #    HIP streams: each conv launch is only 400-3000 workgroups on 256 CUs, and workgroups of
        #    the other streams fill its tail (and HBM-bound layers overlap with MFMA-bound ones).
        main = torch.cuda.current_stream(dev)
        # The tail of the forward (feature_conv, HMR heads, MANO, grasp: ~3 ms of launch-bound work) runs on its
        # own stream and is NOT joined back: the result is a stream_xdict that makes the consumer's stream
        # wait at first access, so the next forward's trunks start under this forward's tail.  The trunk
        # outputs the tail reads are double-buffered by call parity; everything the tail reads from the
        # caller (angles, intrinsics, flags) is copied on the caller's stream first.
        async_tail = bool(self.async_tail and self.engine.overlap and not torch.cuda.is_current_stream_capturing())
        par = self._calls & 1 if async_tail else 0
        self._calls += 1
        if not torch.cuda.is_current_stream_capturing():
            # the tail two calls ago read these feature buffers (long finished); a synchronous call waits for
            # every earlier asynchronous tail
            for q in ((par,) if async_tail else (0, 1)):
                prev_tail = self._ws.get(f"tail_done{q}")
                if prev_tail is not None:
                    main.wait_event(prev_tail)
        featg = buf(f"feat_g{par}", bz * 49 * F) if self.use_glb_feat else None
        feath = buf(f"feat_h{par}", B2 * 49 * F) if not self.no_crops else None
        gch, hch = self.trunk_chunks if self.engine.overlap else (1, 1)
        if self.no_crops:          # model.py:199-201: no hand trunks; the global job may as well be cut in two
            gch, hch = (2 if self.engine.overlap else 1), 0
        if self.separate_hands and hch:
            hch = 2                # one job per side: the sides have their own weights (model.py:226-228)
        gch, hch = (max(1, min(gch, bz)) if self.use_glb_feat else 0), min(hch, B2)
        need_cc = (not self.no_crops) and self.enc_mode in ("latent", "image")    # model.py:199-201: no_crops skips every encoding
        center = (torch.cat([f32(inputs["r_center_angle"]), f32(inputs["l_center_angle"])], 0)
                  if (need_cc or self.rot_fix == 2) else None)
        corner = torch.cat([f32(inputs["r_corner_angle"]), f32(inputs["l_corner_angle"])], 0) if need_cc else None
        rot_in = torch.cat([f32(inputs["r_rot"]), f32(inputs["l_rot"])], 0) if self.rot_fix == 1 else None    # 'pcl' (B2, 3, 3)
        wide = None
        dense_enc = None
        if self.enc_mode in ("dense", "dense_latent") and not self.no_crops:
            # model.py:462-481: per-pixel angle maps (bz, 2 | 6, w, h) + crop masks, encoded / masked / resized on the device
            ang = [f32(inputs["r_dense_angle"]), f32(inputs["l_dense_angle"])]
            msk = [f32(inputs["r_dense_mask"]), f32(inputs["l_dense_mask"])]
            Ca, Hs, Ws = ang[0].shape[1:]
            L_enc = 0 if self.pos_enc == "cam_conv" else self.n_freq
            assert (2 * L_enc * Ca if L_enc else Ca) == (self.enc_channels if self.enc_mode == "dense" else self.latent_channels)
            if self.enc_mode == "dense":
                # model.py:220-224: cat([crop, encoding]) as the NHWC input of the widened conv1
                assert res == self.img_res_ds, "pos_enc='dense': the crops must have the size args.img_res_ds"
                Cp = P["hand_backbone_r" if self.separate_hands else "hand_backbone"]["stem_wide"].Cin
                wide = buf("wide_in", B2 * res * res * Cp)
                for side, im in enumerate((r_img, l_img)):
                    check(L.hands_dense_posenc_f32(ptr(ang[side]), ptr(msk[side]), ptr(im), ptr(wide, side * bz * res * res * Cp),
                                                   bz, Ca, Hs, Ws, L_enc, self.img_res_ds, res, res, Cp, 3, stream), "dense_posenc")
            else:
                # model.py:244-249 / 276-281: resized to img_res_ds and then to the 7x7 feature map -- an input-only computation,
                # done here on the caller's stream so that the tail never reads the caller's maps
                Ce = self.latent_channels
                dense_enc = buf(f"dense_enc{par}", B2 * 49 * Ce)
                for side in (0, 1):
                    check(L.hands_dense_posenc_f32(ptr(ang[side]), ptr(msk[side]), None, ptr(dense_enc, side * bz * 49 * Ce),
                                                   bz, Ca, Hs, Ws, L_enc, self.img_res_ds, 7, 7, Ce, 0, stream), "dense_posenc")
        if self.enc_mode == "image" and not self.no_crops:
            # model.py:203-218: cat([crop, enc repeated over the pixels]) as the NHWC input of the widened conv1
            Cp = P["hand_backbone_r" if self.separate_hands else "hand_backbone"]["stem_wide"].Cin
            wide = buf("wide_in", B2 * res * res * Cp)
            mode = IMAGE_ENC[self.pos_enc]
            for side, im in enumerate((r_img, l_img)):
                check(L.hands_image_posenc_nhwc_f32(ptr(im), ptr(center, side * bz * 2), ptr(corner, side * bz * 8),
                                                    ptr(wide, side * bz * res * res * Cp), bz, res, res, self.n_freq, mode, Cp,
                                                    stream), "image_posenc")
        jobs = []   # (weights, NCHW segments [(tensor, first image, n)], first row of the job, n images, out buffer)
        for c in range(gch):
            lo, hi = c * bz // gch, (c + 1) * bz // gch
            jobs.append((P["backbone"], [(img, lo, hi - lo)], lo, hi - lo, featg))
        for c in range(hch):       # rows [0, bz) of the hand batch are the right crops, [bz, 2 bz) the left crops
            lo, hi = c * B2 // hch, (c + 1) * B2 // hch
            segs = []
            if wide is not None:
                segs.append((wide, lo, hi - lo))
            else:
                if lo < bz:
                    segs.append((r_img, lo, min(hi, bz) - lo))
                if hi > bz:
                    segs.append((l_img, max(lo, bz) - bz, hi - max(lo, bz)))
            jobs.append((P[("hand_backbone_r", "hand_backbone_l")[c]] if self.separate_hands else P["hand_backbone"], segs, lo, hi - lo, feath))
        side_jobs = SideJobs(main)
        fh = fw = 7
        for ji, (Pt, segs, lo, n, ob) in enumerate(jobs):
            # the largest job (last) stays on the caller's stream
            st = main if (ji == len(jobs) - 1 or not self.engine.overlap) else self._side_stream(dev, f"side{ji}")
            side_jobs.begin(st)
            _, fh, fw = self._trunk(L, Pt, segs, n, res, st.cuda_stream, f"j{ji}", n, out=ob, out_off=lo * 49 * F)
            side_jobs.end(st)
        side_jobs.join()         # only after every job has been enqueued
        assert fh * fw == 49
        HW = fh * fw
        # small per-sample inputs the tail reads: private copies made on the caller's stream (center / corner above)
        flipped = meta_info["is_flipped"].to(device=dev, dtype=torch.int64).contiguous()
        if async_tail:
            K, flipped = K.clone(), flipped.clone()
            tail = self._side_stream(dev, "tail")
            evt = torch.cuda.Event()
            evt.record(main)
            tail.wait_event(evt)
            for t in (center, corner, K, flipped, rot_in):
                if t is not None:
                    t.record_stream(tail)
        else:
            tail = main
        with torch.cuda.stream(tail):
            output = self._forward_tail(L, P, dev, tail, bz, fh, fw, featg, feath, center, corner, K, flipped, dense_enc, rot_in)
        if not async_tail:
            return output
        ready = torch.cuda.Event()
        ready.record(tail)
        self._ws[f"tail_done{par}"] = ready
        return stream_xdict(output, ready, dev)

    def _forward_tail(self, L, P, dev, main, bz, fh, fw, featg, feath, center, corner, K, flipped, dense_enc=None, rot_in=None):
        """Everything after the trunks (model.py:196-411), enqueued on ``main`` (the tail stream)."""
        B2, F, HW = 2 * bz, self.feat_dim, fh * fw
        stream = main.cuda_stream
        buf = lambda n, numel: self._buf(n, numel, dev)
        feat_vec = buf("feat_vec", bz * F)
        if self.use_grasp_loss and self.use_glb_feat_w_grasp:
            # sum-pool (model.py:196); only the grasp head reads it
            check(L.hands_sumpool_nhwc_f32(ptr(featg), ptr(feat_vec), bz, HW, F, F, stream), "sumpool")
        # HMR state rows [feat F | vectors 112] (hands_hmr_init_f32); the transformer head keeps the vectors only (`vo` = their column)
        ld, vo = (HMR_VEC, 0) if self.tf_decoder else (F + HMR_VEC, F)
        state = buf("state", B2 * ld)
        cat_ld = self._cat_ld() if self.enc_mode in ("latent", "dense_latent") else F      # row length of `cat` below
        if self.no_crops:
            # model.py:316-318 -> HandHMR.forward(features, use_pool=True) (hand_hmr.py:73-78): both heads read the average-pooled
            # GLOBAL feature map -- written straight into the feat segment of the right and the left state rows
            for side in (0, 1):
                check(L.hands_avgpool_nhwc_f32(ptr(featg), ptr(state, side * bz * ld), bz, HW, F, ld, stream), "avgpool")
        else:
            if self.enc_mode == "latent":
                # -- KPE concat (model.py:258-271, 288-304) ------------------------------------------------
                Cc = F + 20 * self.n_freq
                cat = buf("cat", B2 * HW * Cc)
                check(L.hands_kpe_concat_f32(ptr(feath), ptr(featg) if self.use_glb_feat else None, ptr(center), ptr(corner),
                                             ptr(cat), B2, bz, HW, F, self.n_freq, stream), "kpe_concat")
            elif self.enc_mode == "dense_latent":
                # -- cat([features (+ global features), resized per-pixel maps]) (model.py:250-256, 282-288) -------------------
                Cc, Ce = self._cat_ld(), self.latent_channels
                cat = buf("cat", B2 * HW * Cc)
                check(L.hands_concat_nhwc_f32(ptr(feath), F, F, ptr(featg) if self.use_glb_feat else None, F, ptr(dense_enc),
                                              HW * Ce, Ce, ptr(cat), Cc, B2, bz, HW, stream), "concat")
            else:
                cat = feath            # pos_enc None / image-level: feature_conv reads the crop features as they are
            depth = (depth_head(self.engine, buf, L, P, dev, stream, cat, B2, bz, fh, fw, F + self.latent_channels, cat_ld, self._depth_ld())
                     if self.use_depth_loss else None)
            # -- feature_conv (model.py:91-101, 313-314) -> HMR state rows ---------------------------
            if not self.tf_decoder:
                f1 = buf("fc1", B2 * HW * 1024)
                self.engine.conv(L, P["fc0"], cat, B2, fh, fw, f1, True, stream)
                f2 = buf("fc2", B2 * (fh - 2) * (fw - 2) * 512)
                h2, w2 = self.engine.conv(L, P["fc2"], f1, B2, fh, fw, f2, True, stream)
                f3 = buf("fc3", B2 * (h2 - 2) * (w2 - 2) * 256)
                h3, w3 = self.engine.conv(L, P["fc4"], f2, B2, h2, w2, f3, True, stream, splitk_n=8)   # 3x3 output map: 72 tiles at bz=256, K=4608
                assert h3 * w3 * 256 == P["fc7"].Cin
                self.engine.conv(L, P["fc7"], f3, B2, 1, 1, state, True, stream, out_ps=ld, splitk=True)

        # -- HandHMR x2 (hand_hmr.py:73-92, hmr_layer.py:67-86) ----------------------------------
        caminit4 = buf("caminit4", B2 * 4)
        # the two heads are independent chains of latency-bound M = bz GEMMs: run them side by side
        heads = SideJobs(main)
        for side, hp in ((0, P["head_r"]), (1, P["head_l"])):
            hs = main if (side == 1 or not self.engine.overlap) else self._side_stream(dev, "side_head")
            heads.begin(hs)
            sh = hs.cuda_stream
            if self.tf_decoder:
                tf_head(self.engine, buf, L, hp, sh, side, bz, HW, cat, state, caminit4, F, cat_ld, self.tf_pass)
            else:
                iter_head(self.engine, buf, L, hp, sh, side, bz, state, caminit4, F)
            heads.end(hs)
        heads.join()
        rotmat = buf("rotmat", B2 * 144)
        check(L.hands_rot6d_to_matrix_f32(ptr(state, vo), ld, ptr(rotmat), B2, stream), "rot6d")
        if self.rot_fix == 1:      # 'pcl' (model.py:330-334): in place on the heads' output -- the flip swap and the grasp head see it
            check(L.hands_rot_leftmul_f32(ptr(rotmat), ptr(rot_in), B2, stream), "rot_leftmul")
        st = state[: B2 * ld].view(B2, ld)
        shape = st[:, vo + 96:vo + 106].contiguous()
        cam = st[:, vo + 108:vo + 111].contiguous()
        caminit = caminit4[: B2 * 4].view(B2, 4)[:, :3].contiguous()

        # -- is_flipped swap (model.py:341-368), per sample on device ----------------------------
        rot_m = torch.empty(B2, 16, 3, 3, device=dev)
        shape_m = torch.empty(B2, 10, device=dev)
        cam_m = torch.empty(B2, 3, device=dev)
        caminit_m = torch.empty(B2, 3, device=dev)
        check(L.hands_flip_swap_f32(ptr(flipped), ptr(rotmat), ptr(shape), ptr(cam), ptr(caminit),
                                    ptr(rot_m), ptr(shape_m), ptr(cam_m), ptr(caminit_m), bz, stream),
              "flip_swap")

        if self.rot_fix == 2:      # 'perspective_correction' (model.py:370-376): after the swap, see hands_hip.h for the grasp quirk
            check(L.hands_perspective_correction_f32(ptr(rot_m), ptr(rotmat), ptr(center), ptr(flipped), bz, stream), "persp")

        # -- MANOHead x2 (mano_head.py:21-65) -----------------------------------------------------
        output = run_mano_heads(L, P["mano_r"], P["mano_l"], rot_m, shape_m, cam_m, caminit_m, K,
                                float(self.img_res), bz, stream, buf, self.engine)

        # -- center / corner regression from the feature_conv vectors (model.py:426-433) -------------------
        extra = None
        if self.regress_center_corner:
            extra = xdict()
            for nm, key in (("cc_center", "center"), ("cc_corner", "corner")):
                l0, l1, l2 = P[nm]
                o = torch.empty(B2, 8, device=dev)
                linear_chain(self.engine, L, [(l0, True, True), (l1, True, True), (l2, False, False)], state, B2, stream, buf,
                             ("cc_h1", "cc_h2"), out=o, in_ps=ld)
                n = 2 if key == "center" else 8
                extra[key + ".r"] = o[:bz, :n].contiguous()
                extra[key + ".l"] = o[bz:, :n].contiguous()
        # -- grasp classifier on the UN-flipped HMR outputs (model.py:401-411) -------------------
        if self.use_depth_loss and not self.no_crops:          # model.py:420-424 (merged after the grasp outputs, before center / corner)
            dx = xdict()
            dx["depth.r"], dx["depth.l"] = depth
            if extra is None:
                extra = dx
            else:
                dx.merge(extra)
                extra = dx
        if not self.use_grasp_loss:
            if extra is not None:
                output.merge(extra)
            return output
        output.merge(run_grasp_head(self.engine, L, P["grasp"], GRASP_SPLITK["hands_light"], state, rotmat, bz, stream, buf, shape_ld=ld,
                                    shape_off=vo + 96, feat=feat_vec, feat_dim=F if self.use_glb_feat_w_grasp else 0))
        if extra is not None:          # model.py:426-433: merged after the grasp outputs
            output.merge(extra)
        return output
