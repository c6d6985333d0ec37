/*
 * hands_hip.h -- C ABI of libhands_hip.so: the MI355X (gfx950) forward path of the WildHands
 * hand-mesh regressor (hands_light), hand-written HIP.
 *
 * The reference (ap229997/hands) is 100 % Python and has no FFI: the boundary of its hot path is
 * `HandsLight.forward(inputs, meta_info)` (src/models/hands_light/model.py:187-437).  Every entry
 * point below replaces the ATen ops that one statement of that function dispatches; the statement
 * is cited per function.  INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - All pointers are DEVICE pointers to fp32 unless stated.  The caller owns every buffer; the
 *     library never allocates, frees or synchronises.  Work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).
 *   - Activations are NHWC ("pixel-major"): element (b,h,w,c) at ((b*H+h)*W+w)*pix_stride + c.
 *   - Return value: 0 on success, otherwise a hipError_t (or HANDS_EINVAL for a bad descriptor);
 *     hands_error_string() gives text.  No global mutable state; re-entrant across streams.
 */
#ifndef HANDS_HIP_H
#define HANDS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HANDS_EINVAL 10001
#define HANDS_ABI_VERSION 5

typedef void* hands_stream_t;

int hands_abi_version(void);
const char* hands_error_string(int code);
/* 1 if `stream` is being captured into a hipGraph, 0 if not, < 0 = -(hipError_t).  The host side asks this about the
 * stream it is about to LAUNCH on (torch's "current stream" is not necessarily that stream) before it takes a path that
 * is illegal under capture: growing / zero-filling a workspace (hands_conv2d_nhwc_streamk_f32's epoch flags). */
int hands_stream_is_capturing(hands_stream_t stream);
/* 16 hex digits: sha256 over the kernel sources (every .hip / .h / .cpp of csrc/ and the headers of include/) THIS library was built from.  A stored
 * counter summary (profiles/rNN_pmc_*.json) describes one binary: bench.py uses it only when the hashes agree. */
const char* hands_csrc_sha16(void);

/* ---------------------------------------------------------------------------------------------
 * The chip's own ceilings, measured beside the kernels they bound (csrc/ceilings.hip).  No reference
 * counterpart.  hands_ceiling_mfma_f32: 512 workgroups x 4 waves run `iters` x 32 v_mfma_f32_32x32x2_f32 and nothing else
 * (random_operands != 0: full-mantissa lane-dependent operands instead of constants -- the matrix pipe clocks ~7 % lower on real
 * data); returns the FLOPs the launch executes (time it with events on `stream`), < 0 = -(error).  `out` takes 512 * 256 floats.
 * hands_ceiling_hbm_read_f32: a streaming read of n_floats (use >= 1 GiB: beyond the 256 MB Infinity Cache), 16-byte loads. */
long long hands_ceiling_mfma_f32(float* out, long long out_floats, int iters, int random_operands, hands_stream_t stream);
int hands_ceiling_hbm_read_f32(const float* in, long long n_floats, float* out, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution / linear layer as implicit GEMM on fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *   out[m, n] = act( bias[n] + sum_k patch(m, k) * w[n, k]  (+ residual[m, n]) )
 *   m = (b, ho, wo) flattened, k = (kh, kw, cin) flattened, act selected by desc.act.
 * Replaces nn.Conv2d + eval-mode BatchNorm2d (folded into w/bias by the host) + ReLU + the
 * bottleneck's residual add: src/nets/backbone/resnet.py:134-154,264-280; feature_conv
 * model.py:91-101; and every nn.Linear of the heads (H=W=KH=KW=1): hand_hmr.py:34-40,
 * hmr_layer.py:47-62, model.py:117-125.
 *
 * Weight layout (produced once by hands_amd.packing): [Cout_pad][Kpad] row-major, k ordered
 * (kh, kw, cin), Kpad = round_up(KH*KW*Cin, 16) zero-filled, Cout_pad = round_up(Cout, 128)
 * zero-filled.  bias has Cout_pad entries.  Cin % 4 == 0 and Cout % 4 == 0 are required;
 * Cin % 16 == 0 unless Cin == 4 (the RGB0 stem).
 * Limits (HANDS_EINVAL beyond them; every layer of the three models is far inside): for Cin != 4, padded
 * convolutions take KH, KW <= 15 (tap validity is one 15 + 15 bit word per output pixel), Kpad < 2^21, and
 * (256 / (Ho*Wo) + 2) * H * W * in_pix_stride * 4 < 2^31 (the kernels address a tile's inputs with 32-bit
 * byte offsets from the first image the tile touches).
 *
 * Layout contract of a descriptor and its buffers (all entry points that take a hands_conv_desc; tests/test_gpu_conv_edges.py):
 *   - Every global access is 16 bytes wide.  in_pix_stride, out_pix_stride, res_pix_stride (and the dual entry's in2_pix_stride)
 *     are multiples of 4 floats -- HANDS_EINVAL otherwise -- and `in`, `in2`, `out`, `residual`, `w_packed`, `bias` are 16-byte
 *     aligned: a PRECONDITION the library cannot check cheaply for device pointers and does not check.  Pointers may sit
 *     anywhere inside an allocation; only the channels [0, Cin) of an input pixel, [0, Cout) of a residual pixel are read and
 *     only [0, Cout) of an output pixel is written -- the floats between Cout and out_pix_stride keep their contents.
 *   - res_pix_stride == 0: `residual` is ONE row of Cout floats added to every output pixel (hamer_light's mean parameters).
 *   - `residual` may alias `out` exactly -- the same pointer and the same pixel stride (an in-place update: every thread reads
 *     the residual values of an element before it writes that element) -- but must not overlap it in any other way.
 *   - Ho, Wo may be smaller than the map the geometry (H, W, KH, KW, stride, pad) produces: the launch computes the top-left
 *     Ho x Wo corner of that map, B * Ho * Wo pixels stored densely (a larger map is HANDS_EINVAL).
 *   - Kpad may exceed round_up(KH*KW*Cin, 16) by any multiple of 16: the extra columns of every weight row must be zero (they
 *     are multiplied with zeros, not skipped).  The single-launch result does not depend on the extra columns; a split-K launch
 *     cuts the Kpad / 16 k-steps into S shares, so its summation order is a function of (layer, S, Kpad).  Not for a pointwise layer on the `pre` / grouped / dual entries, whose weight
 *     row is exactly the pixel's channels (Kpad == Cin, dual: Cin + Cin2).
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_conv_desc {
  int32_t B, H, W, Cin;      /* input  (B,H,W,Cin) */
  int32_t Ho, Wo, Cout;      /* output (B,Ho,Wo,Cout) */
  int32_t KH, KW, stride, pad;
  int32_t in_pix_stride;     /* floats between consecutive input pixels  (>= Cin,  % 4 == 0) */
  int32_t out_pix_stride;    /* floats between consecutive output pixels (>= Cout, % 4 == 0) */
  int32_t res_pix_stride;    /* floats between consecutive residual pixels (% 4 == 0; 0 = one row for every pixel); ignored if residual==NULL */
  int32_t Kpad;              /* packed weight row length (% 16 == 0, >= KH*KW*Cin; columns beyond that are zero) */
  int32_t act;               /* HANDS_ACT_*: epilogue activation after bias (+ residual) */
} hands_conv_desc;

#define HANDS_ACT_NONE 0
#define HANDS_ACT_RELU 1        /* max(x, 0); a NaN stays NaN, as in torch.relu (every convolution entry and the fused stems) */
#define HANDS_ACT_GELU 2        /* nn.GELU(): x*0.5*(1+erf(x/sqrt(2)))  (vit.py:76, pose_transformer.py:44) */
#define HANDS_ACT_LEAKY_RELU 3  /* negative slope 0.01 (handoccnet_light/backbone.py) */
#define HANDS_ACT_MASK 0xff
/* Optional arithmetic flag OR'ed into desc.act (default 0 = exact fp32 MFMA, the parity path): both operands are
 * split on the fly into three bf16 planes whose sum is the fp32 value exactly, and the products b_i * b_j with
 * i + j <= 2 run on the bf16 matrix pipe with fp32 accumulation (dropped terms <= 2^-24 of a product).  A separately
 * reported mode: results are fp32-grade but NOT bit-identical to the fp32 chain.  Honoured by
 * hands_conv2d_nhwc_f32 and hands_conv1x1_dual_nhwc_f32 (not the RGB0 stem); the stream-K entry hands such a descriptor to
 * hands_conv2d_nhwc_f32 (honoured); the split-K entries run a launch they really split as exact fp32 (S <= 1 or a too small
 * workspace: the hands_conv2d_nhwc_f32 call, honoured); hands_conv2d_nhwc_pre_f32 rejects it (HANDS_EINVAL). */
#define HANDS_MATH_BF16X3 0x100
/* Blocked fp32 summation, OR'ed into desc.act (round 5): the k-ordered FMA chain of every output is cut into blocks of 128 /
 * 64 floats (8 / 4 k-steps); a block's sum is added to a second accumulator set in block order -- no fp32 accumulation chain
 * longer than the block, inside the launch (no workspace, no second pass).  Same products, another association: results differ
 * from the single chain by fp32 rounding and are closer to an fp64 evaluation (and to ATen's blocked CPU sums).  A fixed function
 * of the layer: batch-size invariant and deterministic.  Honoured by hands_conv2d_nhwc_f32, hands_conv2d_nhwc_pre_f32 and the
 * split-K entries (each K slice is blocked); ignored by the stem and the dual pointwise entry, the stream-K entry falls back to
 * the plain launch.  At most one of the two, and not together with HANDS_MATH_BF16X3 (HANDS_EINVAL). */
#define HANDS_SUM_BLOCK128 0x200
#define HANDS_SUM_BLOCK64 0x400
/* fp64 accumulation, OR'ed into desc.act (round 6): the same fp32 operands, products accumulated by v_mfma_f64_16x16x4_f64 and the
 * bias added in fp64 -- the stored value is the correctly rounded fp32 of (sum + bias), then residual and activation in fp32 as the
 * reference's separate statements do.  Half the fp32 matrix rate: for the few layers whose rounding a network amplifies
 * (handoccnet_light's heat-map head, hand_head.py:75-94,266-280), not for throughput.  Batch-size invariant and deterministic.
 * Honoured by hands_conv2d_nhwc_f32, hands_conv2d_nhwc_pre_f32 and the split-K entries (the partial sums are fp64 there:
 * hands_conv2d_workspace_floats doubles, the workspace must be 8-byte aligned); the stream-K entry runs it as ONE plain launch;
 * hands_conv1x1_dual_nhwc_f32 has no fp64 form and rejects it; not for the RGB0 stem (Cin == 4) and not together with the flags
 * above (HANDS_EINVAL). */
#define HANDS_ACC_F64 0x800

int hands_conv2d_nhwc_f32(const hands_conv_desc* d, const float* in, const float* w_packed,
                          const float* bias, const float* residual, float* out,
                          hands_stream_t stream);

/* Grouped launch (round 6): up to 8 INDEPENDENT pointwise layers (1x1, no padding, any stride) in ONE launch -- the q / k / v
 * projections of an attention block (handoccnet_light/transformer.py:117-135), the FPN laterals (backbone.py:54-57), the two
 * branches of an hourglass level (hand_head.py:217-235), conv1 + downsample of a stage's first bottleneck (resnet.py:134-154).
 * Every job computes exactly what hands_conv2d_nhwc_f32 (pre_scale == NULL) / hands_conv2d_nhwc_pre_f32 (S = 1) would, bit for
 * bit; all jobs of a launch must run the same kernel instantiation: hands_conv2d_group_class(desc, pre) >= 0 and equal for all
 * (-1: not a pointwise layer, or a flag the grouped kernel has no form for -- bf16x3, 128-float blocks, fp64 accumulation),
 * otherwise HANDS_EINVAL and nothing is launched.  The outputs of a launch must not overlap each other or any input of it. */
typedef struct hands_conv_job {
  const hands_conv_desc* desc;
  const float* in;
  const float* w_packed;
  const float* bias;
  const float* residual;      /* or NULL */
  float* out;
  const float* pre_scale;     /* both NULL, or the operand affine of hands_conv2d_nhwc_pre_f32 */
  const float* pre_shift;
} hands_conv_job;
int hands_conv2d_group_class(const hands_conv_desc* d, int pre);
int hands_conv2d_group_f32(const hands_conv_job* jobs, int n, hands_stream_t stream);

/* 3x3 / stride 1 / pad 1 convolution (+ folded BatchNorm bias + activation) as Winograd F(2x2, 3x3) on the fp32 matrix
 * cores (csrc/conv_wino.hip): 16 instead of 36 multiplications per 2x2 output pixels and (cin, cout) pair.  Same layer
 * semantics as hands_conv2d_nhwc_f32 with desc.KH = KW = 3, stride 1, pad 1 and no residual
 * (conv2 / bn2 / relu of a stride-1 Bottleneck: src/nets/backbone/resnet.py:140-142); `u_packed` is the
 * hands_pack_conv3x3_winograd_f64 form of the BN-folded weight, `bias` the same vector hands_pack_conv_f64 produced.
 * All arithmetic is fp32 in a fixed, batch-size-independent order; the result differs from hands_conv2d_nhwc_f32 by
 * fp32 rounding only (Winograd re-associates the 3x3 sum).  Requires Cin % 16 == 0, Cout % 32 == 0, act in
 * {NONE, RELU, LEAKY_RELU}; hands_conv3x3_winograd_supported() returns 1 when `d` can take this route. */
int hands_conv3x3_winograd_supported(const hands_conv_desc* d);
/* multiply-accumulates the matrix cores execute for the layer on this route (16 per 2x2 output tile and (cin, cout) pair,
 * idle tile lanes of partial blocks included); 0 if unsupported.  The algorithmic count is 9 * B * H * W * Cin * Cout. */
long long hands_conv3x3_winograd_executed_macs(const hands_conv_desc* d);
int hands_conv3x3_winograd_f32(const hands_conv_desc* d, const float* in, const float* u_packed, const float* bias,
                               float* out, hands_stream_t stream);

/* The same layer as Winograd F(4x4, 3x3) (csrc/conv_wino4.hip, round 5): 36 multiplications per 4x4 output pixels and
 * (cin, cout) pair -- 2.25 per output against 4 for F(2x2, 3x3) and 9 for the direct form.  Same semantics and restrictions as
 * hands_conv3x3_winograd_f32 (Cin % 8 == 0, Cin >= 16, Cout % 32 == 0, no residual; conv2 / bn2 / relu of a stride-1
 * Bottleneck, src/nets/backbone/resnet.py:140-142); `u_packed` is the hands_pack_conv3x3_winograd4_f64 form of the BN-folded
 * weight.  fp32 throughout in a fixed, batch-size-independent order; the larger transform constants of F(4x4) make the
 * per-layer rounding error ~20x that of F(2x2) (still fp32 noise: DESIGN.md), so a model opts in per layer family
 * (HandsLight: on, HandOccNet: off).  _executed_macs counts 36 per 4x4 tile and (cin, cout) pair, idle tile lanes included. */
int hands_conv3x3_winograd4_supported(const hands_conv_desc* d);
long long hands_conv3x3_winograd4_executed_macs(const hands_conv_desc* d);
int hands_conv3x3_winograd4_f32(const hands_conv_desc* d, const float* in, const float* u_packed, const float* bias,
                                float* out, hands_stream_t stream);

/* Deterministic split-K form of the same layer for latency-bound GEMMs (1x1 / linear layers with few
 * rows and a long K: the HMR / decoder / regressor heads).  hands_conv2d_splitk_factor() returns the
 * number of K slices S the library would use (1 = no split): S = min(8, Kpad/256) for linear layers
 * (H = W = 1) with B <= 2048 rows and Kpad >= 512 -- a function of the layer only, so every output bit
 * is independent of the batch size up to 2048 rows.  The caller provides
 * `workspace` of >= S * M * Cout floats (M = B*Ho*Wo); slices write raw partial sums, a second launch
 * adds them in ascending slice order and applies bias / residual / activation.  With S == 1 or a
 * too-small workspace the call is identical to hands_conv2d_nhwc_f32. */
int hands_conv2d_splitk_factor(const hands_conv_desc* d);
int hands_conv2d_nhwc_splitk_f32(const hands_conv_desc* d, const float* in, const float* w_packed,
                                 const float* bias, const float* residual, float* out, float* workspace,
                                 long long workspace_floats, hands_stream_t stream);
/* Same with a caller-chosen slice count S (clamped to Kpad/16; any convolution, not only linear
 * layers): the small-batch serving mode, where a layer has a handful of output tiles and a K of
 * 2304-4608 walked serially.  The summation order depends on S, so results are reproducible for a
 * given (layer, S) but not bit-identical to the S = 1 call. */
int hands_conv2d_nhwc_splitk_n_f32(const hands_conv_desc* d, const float* in, const float* w_packed,
                                   const float* bias, const float* residual, float* out, int S,
                                   float* workspace, long long workspace_floats, hands_stream_t stream);
/* The same with the reduction FUSED into the launch (round 6): `counters` = n_counters ints, zero before the first call and left
 * zero by every call (one array per stream: concurrent launches must not share it).  The slice of a tile that arrives last adds
 * the partial sums in ascending slice order and applies bias / residual / activation -- the output bits of the two-launch form,
 * one launch.  n_counters below the launch's tile count (ceil(M / 128) * ceil(Cout / 128), or ceil(M / 256) for Cout <= 64):
 * falls back to the two launches.  `out` may alias `residual` (an in-place residual update), never `in`: the last slice of a tile
 * writes `out` while slices of other tiles still read `in`. */
int hands_conv2d_nhwc_splitk_fused_f32(const hands_conv_desc* d, const float* in, const float* w_packed,
                                       const float* bias, const float* residual, float* out, int S,
                                       float* workspace, long long workspace_floats, int* counters,
                                       long long n_counters, hands_stream_t stream);

/* Pointwise layer (1x1, no padding) whose INPUT first goes through a per-channel affine + LeakyReLU(0.01):
 *     out = act( bias + W . leaky_relu(in * pre_scale[c] + pre_shift[c]) (+ residual) )
 * i.e. the eval BatchNorm -> LeakyReLU that precedes conv1 of a pre-activation residual unit
 * (handoccnet_light/hand_head.py:131-136,170-175) folded into the convolution's operand staging instead of a launch of
 * hands_bn_leaky_f32 plus a round trip of the activations.  pre_scale / pre_shift: Cin floats (hands_fold_bn_f32 of a unit
 * weight).  S > 1: the same with the deterministic S-slice split-K (workspace as for hands_conv2d_nhwc_splitk_n_f32).
 * Bit-identical to hands_bn_leaky_f32 followed by the plain / split-K launch. */
int hands_conv2d_nhwc_pre_f32(const hands_conv_desc* desc, const float* in, const float* pre_scale, const float* pre_shift,
                              const float* w_packed, const float* bias, const float* residual, float* out, int S,
                              float* workspace, long long workspace_floats, hands_stream_t stream);

/* Stream-K form of hands_conv2d_nhwc_f32 for launches whose tile count quantises badly on the chip (400-1600
 * tiles on 256 CUs leave 12-24 % of it idle): G persistent workgroups take equal shares of the (tile, k-step)
 * units; a tile cut between two workgroups is finished by the second one CONTINUING the first one's fp32 FMA chain
 * from its dumped accumulators, so every output bit equals the plain launch (and stays independent of the batch
 * size).  hands_conv2d_streamk_grid() returns G, or 0 when the library would take the plain launch (short K, few
 * or very many tiles, < 5 % to gain) -- the call is then identical to hands_conv2d_nhwc_f32.
 * workspace: hands_conv2d_streamk_workspace_bytes() bytes of device memory, ZEROED once by the caller, private to
 * one stream at a time; epoch: any nonzero value different from the one passed with the previous call on the
 * same workspace (a per-workspace counter), POSITIVE in production.  A negative epoch is a test hook: no workgroup
 * publishes its hand-off, so every consumer takes the bounded-wait fallback and recomputes the missing k-steps
 * itself (slow, same bits). */
long long hands_conv2d_streamk_workspace_bytes(void);
int hands_conv2d_streamk_grid(const hands_conv_desc* d);
int hands_conv2d_nhwc_streamk_f32(const hands_conv_desc* d, const float* in, const float* w_packed,
                                  const float* bias, const float* residual, float* out, void* workspace,
                                  long long workspace_bytes, int epoch, hands_stream_t stream);

/* Two 1x1 convolutions summed into one output: out = act(W0 * in + W1 * in2[stride2-sampled] + bias).
 * `d` describes the first one (stride 1, H = Ho, W = Wo, Cin = K0) with Kpad = K0 + Cin2; the packed
 * weight row is [W0 (K0) | W1 (Cin2)], both with their BatchNorm folded, bias = b0 + b1.  This is the
 * last convolution of a ResNet bottleneck fused with the block's downsample branch
 * (src/nets/backbone/resnet.py:134-154: `out = bn3(conv3(out)); identity = downsample(x); out += identity`):
 * the identity tensor is never written to or re-read from HBM.  in2 is (B, H2, W2, Cin2) with
 * in2_pix_stride floats per pixel; output pixel (ho, wo) reads in2 pixel (ho*stride2, wo*stride2). */
int hands_conv1x1_dual_nhwc_f32(const hands_conv_desc* d, const float* in, const float* in2, int Cin2, int H2,
                                int W2, int stride2, int in2_pix_stride, const float* w_packed,
                                const float* bias, float* out, hands_stream_t stream);

/* The ResNet stem as one kernel: conv 7x7 / stride 2 / pad 3 on the RGB0 image (B,H,W,4) with the
 * folded eval-BatchNorm, activation, and max-pool 3x3 / stride 2 / pad 1 -- conv1, bn1, relu, maxpool of
 * src/nets/backbone/resnet.py:264-268 (LeakyReLU variant: src/models/handoccnet_light/backbone.py:44-47).
 * w_packed is the stem's hands_conv2d_nhwc_f32 weight ([128][208], k = (kh, kw, rgb0)), bias [>=64];
 * out (B, Hp, Wp, 64) with Hc = (H-1)/2+1, Hp = (Hc-1)/2+1.  Bit-identical to hands_conv2d_nhwc_f32
 * followed by hands_maxpool3x3s2_nhwc_f32; the (B,Hc,Wc,64) map is never written to HBM. */
int hands_stem_conv_maxpool_nhwc_f32(const float* x4, const float* w_packed, const float* bias, float* out,
                                     int B, int H, int W, int act, hands_stream_t stream);

/* The same stem reading the reference's NCHW image (B,3,H,W) directly -- no NHWC4 conversion launch -- with the
 * contraction ordered (colour plane, kh, kw): w_planar is [128][160] row-major, k = plane * 52 + kh * 7 + kw (taps
 * 49..51 of each plane and k >= 156 zero), i.e. hands_pack_linear_f64 of the folded (64, 147) weight with
 * col_index[c * 49 + tap] = c * 52 + tap, k_total = 160.  K = 160 instead of 208: 23 % fewer MFMAs.  Same result as
 * hands_stem_conv_maxpool_nhwc_f32 up to the fp32 rounding of a different summation order. */
int hands_stem_conv_maxpool_nchw_f32(const float* x_nchw, const float* w_planar, const float* bias, float* out,
                                     int B, int H, int W, int act, hands_stream_t stream);

/* NCHW (B,3,H,W) image batch -> NHWC with C padded to 4 (4th channel = 0).
 * Replaces the implicit layout of inputs["img"|"r_img"|"l_img"] (model.py:188,238-239).  B, H, W >= 1, else HANDS_EINVAL. */
int hands_nchw3_to_nhwc4_f32(const float* in, float* out, int B, int H, int W, hands_stream_t stream);

/* MaxPool2d(kernel 3, stride 2, padding 1) on NHWC.  resnet.py:268. C % 4 == 0; B, H, W >= 1, else HANDS_EINVAL.
 * A NaN inside a window makes that output NaN, as in nn.MaxPool2d; so does the pool of the two fused stem entries, under
 * every activation (HANDS_ACT_RELU hands a NaN on as well). */
int hands_maxpool3x3s2_nhwc_f32(const float* in, float* out, int B, int H, int W, int C,
                                hands_stream_t stream);

/* feat_vec[b, c] = sum_p feat[b, p, c]  (a SUM over the 7x7 map, not a mean).  model.py:196.
 * C % 4 == 0, out_stride % 4 == 0; B, HW >= 1, else HANDS_EINVAL. */
int hands_sumpool_nhwc_f32(const float* feat, float* out, int B, int HW, int C, int out_stride,
                           hands_stream_t stream);

/* out[b, c] = mean_p feat[b, p, c]: nn.AdaptiveAvgPool2d(1) at the top of HandHMR.forward(use_pool=True)
 * (src/nets/hand_heads/hand_hmr.py:73-78), taken when HandsLight runs with no_crops (src/models/hands_light/model.py:316-318,
 * the arctic_light configuration): both heads read the pooled GLOBAL feature map.  Same summation order as
 * hands_sumpool_nhwc_f32, then one division by HW. */
int hands_avgpool_nhwc_f32(const float* feat, float* out, int B, int HW, int C, int out_stride,
                           hands_stream_t stream);

/* Image-level positional encodings, pos_enc = 'center' (mode 1) | 'corner' (mode 2) | 'center+corner' (mode 3)
 * (src/models/hands_light/model.py:203-218: torch.cat([img, enc.view(bz,-1,1,1).repeat(1,1,w,h)], dim=1)):
 * out (B, H, W, Cpad) NHWC = [r g b | center enc 4 n_freq | corner enc 16 n_freq | zero padding], img_nchw (B,3,H,W),
 * center_angle (B,2), corner_angle (B,8); the encoding is that of hands_kpe_concat_f32 (model.py:444-460).  The result
 * is the input of the hand trunk's widened conv1 through hands_conv2d_nhwc_f32 (Cin = Cpad, a multiple of 16). */
int hands_image_posenc_nhwc_f32(const float* img_nchw, const float* center_angle, const float* corner_angle, float* out,
                                int B, int H, int W, int n_freq, int mode, int Cpad, hands_stream_t stream);


/* Per-pixel positional encodings, pos_enc = 'dense' | 'dense_latent' | 'cam_conv' (src/models/hands_light/model.py:462-481, call
 * sites :220-224, :244-256, :276-288).  angle (B, Ca, Hs, Ws) NCHW, mask (B, Hs, Ws).  n_freq > 0: the 2 n_freq Ca channels
 * sin / cos(2^k angle[ci]) laid out (k, ci, {sin, cos}); n_freq == 0: the Ca raw maps ('cam_conv'); times the mask; then
 * F.interpolate(bilinear, align_corners=True) to (R, R) (args.img_res_ds) and from there to (Ho, Wo) (Ho == R: the first only).
 * The result goes to channels [c_off, c_off + Cenc) of the NHWC map out (B, Ho, Wo, ld).  img_nchw != NULL ((B, 3, Ho, Wo),
 * c_off == 3): the whole pixel is written, [r g b | encoding | zeros] -- the input of the hand trunk's widened conv1
 * ('dense'); NULL: only the encoding channels (the 7x7 map hands_concat_nhwc_f32 appends to the features). */
int hands_dense_posenc_f32(const float* angle, const float* mask, const float* img_nchw, float* out, int B, int Ca, int Hs, int Ws,
                           int n_freq, int R, int Ho, int Wo, int ld, int c_off, hands_stream_t stream);

/* torch.cat along the channels of NHWC maps: out[b, p, :] = [a[b, p, :Ca] (+ add[b % Bg, p, :Ca]) | extra[b, p, :Cb] | zeros],
 * row strides lda / ld_add / Cb / ld, extra_batch_stride floats between samples of `extra` (0: one map for every sample).
 * model.py:252-256, 284-288 (features (+ global features) with the resized per-pixel maps), :177-185 (`broadcast`: the depth
 * head's (x, y) grid).  add / extra may be NULL (Cb = 0). */
int hands_concat_nhwc_f32(const float* a, int lda, int Ca, const float* add, int ld_add, const float* extra,
                          long long extra_batch_stride, int Cb, float* out, int ld, int B, int Bg, int HW, hands_stream_t stream);

/* out (B, H, W, C) = nn.Upsample / F.interpolate(x (B, h, w, C), mode='bilinear', align_corners=True): the three upsamplings of
 * the depth head (model.py:141, 146, 151).  C % 4 == 0. */
int hands_upsample_bilinear_ac_f32(const float* x, float* out, int B, int h, int w, int H, int W, int C, hands_stream_t stream);

/* pos_enc = 'pcl' (model.py:330-334): rotmat[b, 0] = rot[b] @ rotmat[b, 0] in place; rotmat (B, 16, 3, 3), rot (B, 3, 3). */
int hands_rot_leftmul_f32(float* rotmat, const float* rot, int B, hands_stream_t stream);

/* pos_enc = 'perspective_correction' (model.py:370-376): rot_swapped[b, 0] = Rx(-c[b,0]) Ry(-c[b,1]) @ rot_swapped[b, 0] on the
 * rotations AFTER the is_flipped swap (2 Bg rows: right then left; center_angle (2 Bg, 2)).  pytorch3d.euler_angles_to_matrix
 * ('XYZ') is absent from the reference tree: published definition, parity unpinned.  The reference assigns in place: in a batch
 * without a flipped sample that tensor is the heads' own output, which the grasp head reads afterwards -- the corrected matrix
 * is then also written to rotmat (the unswapped rotations); with a flipped sample rotmat stays as it is. */
int hands_perspective_correction_f32(float* rot_swapped, float* rotmat, const float* center_angle, const int64_t* is_flipped,
                                     int Bg, hands_stream_t stream);

/* out[b2, p, :] = cat(crop[b2,p,:] + glb[b2 % Bg, p, :], center_enc(b2), corner_enc(b2)).
 * crop holds the right-hand samples then the left-hand samples (2*Bg rows); encodings are the
 * reference's [sin(2^k a), cos(2^k a)] laid out (L, c, 2).  model.py:258-271, 444-460.
 * center_angle (2*Bg, 2), corner_angle (2*Bg, 8); out channels = C + 4*L + 16*L.
 * glb == NULL: use_glb_feat = False, the crop features are concatenated as they are (model.py:266-267). */
int hands_kpe_concat_f32(const float* crop, const float* glb, const float* center_angle,
                         const float* corner_angle, float* out, int B2, int Bg, int HW, int C,
                         int n_freq, hands_stream_t stream);

/* HMR state rows (ld = F + 112, every segment 16-byte aligned):
 *   [feat F | pose6d 96 | shape 10 | 0 0 | cam 3 | 0]
 * Writes the identity-6D / zero-shape initial vectors (hand_hmr.py:46-56) and copies the cam_init
 * MLP output (rows of 4 floats: s, tx, ty, pad) into columns F..F+111 of every row. */
int hands_hmr_init_f32(float* state, const float* cam_init, int B, int ld, int F,
                       hands_stream_t stream);

/* rotation_6d_to_matrix (pytorch3d; call site hand_hmr.py:85-87): Gram-Schmidt, rows.
 * pose6d rows have stride ld6; rotmat is (B,16,3,3) contiguous. */
int hands_rot6d_to_matrix_f32(const float* pose6d, int ld6, float* rotmat, int B,
                              hands_stream_t stream);

/* is_flipped branch of HandsLight.forward (model.py:341-368): per-sample swap of the two hands'
 * predictions with mirrored axis-angle (y,z negated) and cam ty sign flip.  Arrays hold the right
 * hand in rows [0,Bg) and the left hand in rows [Bg,2Bg).  is_flipped: int64 (Bg).
 * In/out: rotmat (2Bg,16,3,3), shape (2Bg,10), cam (2Bg,3), cam_init (2Bg,3) -> *_out. */
int hands_flip_swap_f32(const int64_t* is_flipped, const float* rotmat, const float* shape,
                        const float* cam, const float* cam_init, float* rotmat_out,
                        float* shape_out, float* cam_out, float* cam_init_out, int Bg,
                        hands_stream_t stream);

/* The rotation conversions of the MANO head on their own (the same device functions
 * hands_mano_pose_f32 and hands_flip_swap_f32 inline): matrix_to_axis_angle =
 * quaternion_to_axis_angle(matrix_to_quaternion(.)) (common/rot.py:118-193, 55-83; called at
 * src/nets/hand_heads/mano_head.py:27-31) and its inverse axis_angle_to_matrix (common/rot.py:754-782,
 * 86-115; model.py:345-353).  rotmat (n,3,3) row-major, axis_angle (n,3). */
int hands_matrix_to_axis_angle_f32(const float* rotmat, float* axis_angle, long long n, hands_stream_t stream);
int hands_axis_angle_to_matrix_f32(const float* axis_angle, float* rotmat, long long n, hands_stream_t stream);

/* grasp-head input rows [feat_vec(F) | rotmat(144) | shape(10) | 0-pad]: the reference's
 * cat([shape, pose.view(bz,-1), feat_vec]) (model.py:401-404) with the columns permuted so the
 * segments are 16-byte aligned; the packed grasp_classifier.0 weight uses the same permutation.
 * Rows [0,Bg) are the right hand, [Bg,2Bg) the left; feat_vec (Bg,F) is shared by both. */
int hands_grasp_input_f32(const float* shape, int ld_shape, const float* rotmat,
                          const float* feat_vec, float* out, int B2, int Bg, int F, int ld_out,
                          hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MANO layer (MANOHead.forward, src/nets/hand_heads/mano_head.py:21-65 -> common/rot.py:118-193,
 * smplx.MANO / smplx.lbs, common/camera.py:456-474, common/transforms.py:316-329,
 * common/data_utils.py:361-365).  Three launches per hand side:
 *   1. hands_mano_pose_f32     rotmat -> axis-angle -> (+pose_mean) -> Rodrigues -> pose feature;
 *                              joints J(beta); forward kinematics -> skinning transforms A (B,16,12)
 *                              and posed joints (B,16,3); writes the blend-GEMM input rows
 *                              [beta(10) | pose_feature(135) | 0-pad] (B, ld_blend).
 *   2. hands_conv2d_nhwc_f32   v_posed = v_template + [beta|pf] @ [shapedirs; posedirs]
 *                              (the 778x3 x 145 contraction on MFMA), output (B, ld_vp).
 *   3. hands_mano_skin_f32     per-vertex blend of A, apply, fingertip joints, weak-perspective
 *                              camera, K-projection, 2x/res-1 normalisation.
 *
 * Contract of the four MANO entries (hands_mano_pose_f32, hands_mano_pose_aa_f32, hands_mano_skin_f32,
 * hands_mano_heads_f32; tests/test_gpu_mano_edges.py).  Every array is dense fp32 except the rows with a stride:
 * betas (B, ld_betas >= 10), blend_in (B, ld_blend >= 145; the pose entries write columns [0,145) and ZERO
 * columns [145, ld_blend)), v_posed (B, ld_vp >= 2334; columns past 2334 are not read).  K is (B,3,3) row-major
 * and general: the projection is (K X)_xy / (K X)_z.  tip_ids are five vertex indices in [0, 778), not checked.
 * Alignment: 4 bytes everywhere except
 *   - hands_mano_skin_f32:  consts.lbs_weights 16 bytes (a vertex's 16 weights are four 16-byte loads);
 *   - hands_mano_heads_f32: out.vertices and out.v3d_cam 8 bytes (stored two floats at a time; a hand's 2334
 *                           floats keep that alignment from row to row), blend_w 16 bytes (16-byte loads).
 * HANDS_EINVAL (nothing launched): a NULL pointer -- argument, descriptor or any member the entry reads (the pose
 * entries: pose_mean, J_template, J_shapedirs; the skin entry: lbs_weights, tip_ids and the six outputs; the fused
 * entry: all five constants, blend_w, blend_bias, rot, betas, cam_wp and the six outputs of every side) --,
 * B <= 0, ld_betas < 10, ld_blend < 145, ld_vp < 2334, n_sides outside {1, 2}, or a pointer that misses the
 * alignment above.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_mano_consts {
  const float* pose_mean;   /* (48)      zeros(3) ++ hands_mean(45) */
  const float* J_template;  /* (16,3)    J_regressor @ v_template */
  const float* J_shapedirs; /* (48,10)   J_regressor @ shapedirs */
  const float* lbs_weights; /* (778,16) */
  const int32_t* tip_ids;   /* (5) */
} hands_mano_consts;

int hands_mano_pose_f32(const hands_mano_consts* c, const float* rotmat, const float* betas,
                        int ld_betas, float* blend_in, int ld_blend, float* A, float* joints16,
                        int B, hands_stream_t stream);

typedef struct hands_mano_out {
  float* vertices;  /* (B,778,3) */
  float* joints3d;  /* (B,21,3)  */
  float* v3d_cam;   /* (B,778,3) */
  float* j3d_cam;   /* (B,21,3)  */
  float* j2d_norm;  /* (B,21,2)  */
  float* cam_t;     /* (B,3)     */
} hands_mano_out;

int hands_mano_skin_f32(const hands_mano_consts* c, const float* v_posed, int ld_vp,
                        const float* A, const float* joints16, const float* cam_wp,
                        const float* K, float img_res, float min_s, const hands_mano_out* out,
                        int B, hands_stream_t stream);

/* MANOHead.forward for ONE or BOTH hands in a single launch: everything hands_mano_pose_f32 ->
 * hands_conv2d_nhwc_f32 (blend) -> hands_mano_skin_f32 compute, fused (pose / forward kinematics, the
 * 2334 x 145 blend contraction on the fp32 matrix cores with the 16 hands of a block as the MFMA N
 * dimension, skinning, camera, projection).  sides[s] carries that side's constants (hands_pack_mano_f32),
 * inputs (rot (B,16,3,3) rotation matrices -- or (B,48) axis-angle when axis_angle_input != 0 --, betas
 * (B, ld_betas), cam_wp (B,3)) and outputs; K (B,3,3) is shared.  Replaces mano_head.py:21-65 for
 * mano_r and mano_l (model.py:378-390) and the ground-truth MANO pass (process_arctic.py:16-40). */
typedef struct hands_mano_side {
  hands_mano_consts consts;
  const float* blend_w;     /* [2432][160] */
  const float* blend_bias;  /* [2432] */
  const float* rot;
  const float* betas;
  const float* cam_wp;
  hands_mano_out out;
} hands_mano_side;

int hands_mano_heads_f32(const hands_mano_side* sides, int n_sides, const float* K, int ld_betas,
                         float img_res, float min_s, int B, int axis_angle_input, hands_stream_t stream);
/* The number of blockIdx.z slices hands_mano_heads_f32 cuts the 13 chunks of 64 vertices into for (B, n_sides): one of
 * {1, 2, 3, 4, 5, 7, 13}, the smallest that yields ~800 workgroups (slice z owns chunks [13 z / n, 13 (z + 1) / n));
 * 0 for B <= 0 or n_sides outside {1, 2}.  A pure function (no device access); no output bit depends on it. */
int hands_mano_heads_vsplit(int B, int n_sides);

/* ---------------------------------------------------------------------------------------------
 * hamer_light (ViT-H/16 + cross-attention decoder head): src/models/hamer_light/.
 * GEMMs (patch embed, qkv, proj, MLP, to_kv, decoders ...) run on hands_conv2d_nhwc_f32.
 * --------------------------------------------------------------------------------------------- */

/* F.interpolate(bilinear, align_corners=False) (Hin,Win)->(S,S) of an NCHW (B,3,..) batch, keep
 * columns [col0, col0+Wc), write NHWC4 (B,S,Wc,4).  hamer_light/model.py:82-100.
 * B, Hin, Win, S, Wc >= 1 and 0 <= col0 <= S - Wc, else HANDS_EINVAL. */
int hands_resize_crop_nchw3_to_nhwc4_f32(const float* in, float* out, int B, int Hin, int Win, int S,
                                         int col0, int Wc, hands_stream_t stream);

/* LayerNorm over the last dim C in {256,768,1024,1280} (768: the ViT-B/16 trunk of hands_light); out = LN(x)*gamma+beta (+ addvec[row/rows_per_vec]).
 * vit.py:128-151,338 (eps 1e-6), pose_transformer.py:22-33 (eps 1e-5); the optional add is the KPE
 * re-added to the final feature map (hamer_light/model.py:102-104). */
int hands_layernorm_f32(const float* x, const float* gamma, const float* beta, float* out,
                        const float* addvec, int rows_per_vec, int M, int C, float eps,
                        hands_stream_t stream);

/* x[b,t,:] = ((x[b,t,:] + pos[1+t,:]) + pos[0,:]) + vec[b,:]   (vec may be NULL).  vit.py:326-330. */
int hands_add_pos_f32(float* x, const float* pos, const float* vec, int B, int T, int C,
                      hands_stream_t stream);

/* rows [center_enc 4L | corner_enc 16L | 0-pad] of the key-point encoding (pos_emb.py:53-67). */
int hands_kpe_encode_f32(const float* center_angle, const float* corner_angle, float* out, int B, int ld,
                         int n_freq, hands_stream_t stream);

/* softmax((scale*q) k^T) v per (batch, head) on fp32 MFMA.  qkv rows are tokens: [q | k | v], each
 * heads*head_dim wide (vit.py:110-126).  Built for T=192, head_dim=80 (ViT-H/16 at 256x192) and for T=197,
 * head_dim=64 (ViT-B/16 at 224x224: 196 patches + class token, nn.MultiheadAttention's in_proj row order; this shape
 * used to return HANDS_EINVAL): attention_kernel<12,80,192> and attention_kernel<13,64,197> of csrc/transformer.hip, one
 * kernel template.  T=197 is padded to 208 inside the kernel: padded keys carry zero weight, padded query rows are not
 * stored -- `out` is written for rows [0, B*197) only.  Any other shape: HANDS_EINVAL. */
int hands_attention_f32(const float* qkv, float* out, int B, int T, int heads, int head_dim, float scale,
                        hands_stream_t stream);

/* ---- ViT-B/16 trunk of hands_light (HandsLight(backbone='vit_b_16'), hands_light/model.py:483-493; replaces
 * "only backbone='resnet50' is built").  The encoder's GEMMs and vit_conv run on hands_conv2d_nhwc_f32 /
 * hands_conv3x3_winograd*_f32, its LayerNorms on hands_layernorm_f32 (C = 768), its attention on hands_attention_f32. ---- */

/* Token assembly (model.py:484-487 + Encoder.forward's `input + pos_embedding`): patch (B, T-1, C) rows of the patch
 * embedding, class_token (C), pos (T, C) -> x (B, T, C) with x[b,0] = class_token + pos[0], x[b,1+t] = patch[b,t] + pos[1+t].
 * One add per element (equal to torch.cat + add bit for bit).  C % 4 == 0.  (hands_add_pos_f32 is HaMeR's different rule.) */
int hands_vit_tokens_f32(const float* patch, const float* class_token, const float* pos, float* x, int B, int T, int C,
                         hands_stream_t stream);

/* Tail of vit_forward: encoder.ln (eps) on the patch tokens 1..grid*grid of x (B, 1+grid*grid, C), then AvgPool2d(2) of
 * the grid x grid token map -> out (B, grid/2, grid/2, C) NHWC; each token is normalised first, then four are averaged
 * (model.py:488-491, utils.py:29).  The class token is never read.  C = 768, grid even. */
int hands_vit_tail_f32(const float* x, const float* gamma, const float* beta, float* out, int B, int grid, int C, float eps,
                       hands_stream_t stream);

/* ---- transformer head of hands_light (HandsLight(tf_decoder=True): hmr_layer.py:17-42, 67-86, hand_hmr.py:19-31, 57-62,
 * hands_light/transformer.py with no_norm=True).  Its Linear layers (in_proj, out_proj, linear1 / linear2, feat_mlp,
 * cam_init_precursor, the decoders) run on hands_conv2d_nhwc_f32 with the bias / ReLU / residual epilogue. ---- */

/* Single-head attention at a wide head dimension: out[b] = softmax(scale * Q[b] K[b]^T) V[b], Q (Tq, D), K and V (Tk, D),
 * out (Tq, D); 1 <= Tq, Tk <= 128, D a multiple of 64 (1024 in the head).  Every operand has its own row stride ld* (floats,
 * >= D, a multiple of 4) and batch stride (floats, a multiple of 4), so the packed (B, T, 3 D) output of in_proj and a
 * (B, Tk, 2 D) [k | v] buffer are read in place; all four pointers 16-byte aligned.  D streams through LDS in 64-float chunks
 * on v_mfma_f32_16x16x4_f32 while the Tq x Tk scores stay in registers; the D-sum of a score is blocked (64 products per block,
 * blocks added in order).  Keys >= Tk carry exactly zero weight; only rows < Tq and columns < D of `out` are written.  The
 * summation order depends on (Tq, Tk, D) only: a batch element's result does not depend on B.  Anything outside this contract
 * (and B > 65535) returns HANDS_EINVAL without a launch. */
int hands_wide_attention_f32(const float* q, long long q_batch_stride, int ldq, const float* k, long long k_batch_stride, int ldk,
                             const float* v, long long v_batch_stride, int ldv, float* out, long long out_batch_stride, int ldo,
                             int B, int Tq, int Tk, int D, float scale, hands_stream_t stream);

/* out[b,t,:] = relu(vec[b*ldvec + col(t)] * w + bias): nn.Linear(1, C) + ReLU on every scalar of the (B, T) vector buffer
 * (`vector_mlp`, hmr_layer.py:72-73).  col(t) = t for t < split and t + gap from there on: the HMR state row
 * [pose6d 96 | shape 10 | 0 0 | cam 3 | 0] is read in place with split = 106, gap = 2; a dense (B, T) buffer with split = T,
 * gap = 0.  w, bias (C); out (B, T, C); C % 4 == 0; ldvec covers the last token's column. */
int hands_vector_tokens_f32(const float* vec, int ldvec, int split, int gap, const float* w, const float* bias, float* out, int B,
                            int T, int C, hands_stream_t stream);

/* out[b,c] = (sum_t x[b,t,c]) / N (torch.mean over the tokens, hmr_layer.py:78), the sum in hands_token_sum_f32's fixed order.
 * C % 64 == 0. */
int hands_token_mean_f32(const float* x, float* out, int B, int N, int C, hands_stream_t stream);

/* one query token per sample against T context tokens: q (B, heads*64), kv rows [k | v] (B*T,
 * 2*heads*64) -> out (B, heads*64); dots = (q.k)*scale (pose_transformer.py:113-123). */
int hands_cross_attention_1q_f32(const float* q, const float* kv, float* out, int B, int T, int heads,
                                 int head_dim, float scale, hands_stream_t stream);

/* rot6d_to_rotmat with b1,b2,b3 as COLUMNS (hamer_light/geometry.py:47-62). */
int hands_rot6d_to_matrix_cols_f32(const float* pose6d, int ld6, float* rotmat, int B,
                                   hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * handoccnet_light (LeakyReLU ResNet-50 + FPN + CBAM gate + FIT/SET attention + hourglass regressor):
 * src/models/handoccnet_light/.  Convolutions and linear layers run on hands_conv2d_nhwc_f32
 * (HANDS_ACT_LEAKY_RELU epilogue); all tensors NHWC, C % 4 == 0.
 * --------------------------------------------------------------------------------------------- */

/* out = F.interpolate(x (B,h,w,C) -> (H,W), bilinear, align_corners=False) + y.  backbone.py:40-42.
 * C % 4 == 0; B, h, w, H, W >= 1, else HANDS_EINVAL. */
int hands_upsample_bilinear_add_f32(const float* x, const float* y, float* out, int B, int h, int w,
                                    int H, int W, int C, hands_stream_t stream);

/* 2x2 stride-2 pooling: mode 0 = AvgPool2d (backbone.py:38,62), 1 = max (hand_head.py:219,276). */
int hands_pool2x2_nhwc_f32(const float* in, float* out, int B, int H, int W, int C, int mode,
                           hands_stream_t stream);

/* ChannelPool (cbam.py:66-68): out[pix] = [max_c x, mean_c x, 0, 0]; C must be 256. */
int hands_channel_pool_f32(const float* x, float* out, long long npix, int C, hands_stream_t stream);

/* SpatialGate tail (cbam.py:78-82): s = sigmoid(logit[pix*logit_stride]); primary = x*s;
 * secondary = x*(1-s). */
int hands_gate_apply_f32(const float* x, const float* logit, int logit_stride, float* primary,
                         float* secondary, long long npix, int C, hands_stream_t stream);

/* out_q = (query + q_emb[t]) + kpe[b]; out_k = (key + k_emb[t]) + kpe[b]; tokens (B,N,C), embeddings
 * (N,C), kpe (B,C).  transformer.py:119-134. */
int hands_add_embed2_f32(const float* query, const float* key, const float* q_emb, const float* k_emb,
                         const float* kpe, float* out_q, float* out_k, int B, int N, int C,
                         hands_stream_t stream);

/* out[b,t,:] = x[b,t,:] + vec[b,:]   (handoccnet_light/model.py:88-89). */
int hands_add_rowvec_f32(const float* x, const float* vec, float* out, int B, int N, int C,
                         hands_stream_t stream);

/* out[b,c] = sum_t x[b,t,c]. */
int hands_token_sum_f32(const float* x, float* out, int B, int N, int C, hands_stream_t stream);

/* out = LeakyReLU_0.01(x * scale[c] + shift[c]): eval BatchNorm (folded by the host) + activation
 * in front of a convolution (pre-activation residual units, hand_head.py:131-133,170-172). */
int hands_bn_leaky_f32(const float* x, const float* scale, const float* shift, float* out,
                       long long npix, int C, hands_stream_t stream);

/* out = up1 + nearest_upsample_2x(low (B,h,w,C))   (hand_head.py:228-230).  C % 4 == 0; B, h, w >= 1, else HANDS_EINVAL. */
int hands_upsample_nearest2x_add_f32(const float* low, const float* up1, float* out, int B, int h,
                                     int w, int C, hands_stream_t stream);

/* heatmaps[b,t,j] = softmax_t(latents[b,t,j] * betas[j]) for j < J, 0 for J <= j < ld_out
 * (hand_head.py:62-67).  Row strides ld_in / ld_out (>= J).  B, N, J >= 1, else HANDS_EINVAL. */
int hands_spatial_softmax_f32(const float* latents, int ld_in, const float* betas, float* heatmaps,
                              int ld_out, int B, int N, int J, hands_stream_t stream);

/* softmax((q k^T) * scale) v per (batch, head) with online softmax on fp32 MFMA; q,k,v,out (B*N,
 * heads*64).  Optional FIT gate: output rows scaled by sigmoid((q2 . k2sum[b]) * scale), k2sum (B,
 * heads*64) = sum over the tokens of k2; optional residual added to the output.
 * transformer.py:71-98,146-153.  N a positive multiple of 128, head_dim == 64, k2sum given whenever q2 is; anything else
 * (N = 0 included) returns HANDS_EINVAL without a launch. */
int hands_flash_attention_f32(const float* q, const float* k, const float* v, const float* q2,
                              const float* k2sum, const float* resid, float* out, int B, int N,
                              int heads, int head_dim, float scale, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Evaluation metrics on the (gathered) predictions, on device: src/utils/eval_modules.py:97-134
 * (mpjpe/ra/h), :136-219,320-343 (mpjpe/pa/ra/{r,l,h}, Procrustes with a 3x3 SVD per hand),
 * :386-407 (mrrpe/r/l), :410-428 (pix_err/{r,l}); common/metrics.py:23-55.  Millimetres / pixels,
 * NaN conventions as the reference (invalid hand -> NaN, except the PA error which it multiplies
 * by the validity flag).  All arrays fp32: joints (B,21,3), 2-D joints (B,21,2) in pixels,
 * per-sample flags (B), per-joint flags (B,21).
 * Rank-deficient Procrustes: the alignment is a proper rotation whatever the rank of the cross-covariance of the two hands.
 * Planar joints (rank 2) and joints on a line (rank 1, predicted or ground truth) give the error of the reference's LAPACK
 * SVD, which there does not depend on how the singular frame is completed; a constant prediction gives NaN (the scale is
 * 0 / 0, as in the reference), a constant ground truth 0.  The joints of an invalid hand are still read (the PA error is
 * multiplied by the flag): they must be finite for the 0 to come out, as in the reference.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_eval_in {
  const float *pred_j3d_r, *pred_j3d_l, *gt_j3d_r, *gt_j3d_l;
  const float *pred_j2d_r, *pred_j2d_l, *gt_j2d_r, *gt_j2d_l;
  const float *is_valid, *right_valid, *left_valid, *joints_valid_r, *joints_valid_l;
} hands_eval_in;

typedef struct hands_eval_out {
  float *mpjpe_ra_h, *mpjpe_pa_ra_r, *mpjpe_pa_ra_l, *mpjpe_pa_ra_h, *mrrpe_rl; /* (B) each */
  float *pix_err_r, *pix_err_l;                                                  /* (B,21) */
} hands_eval_out;

int hands_eval_metrics_f32(const hands_eval_in* in, const hands_eval_out* out, int B,
                           hands_stream_t stream);

/* The other branch of eval_mpjpe_pa_ra, taken when 'egoexo' is in meta_info['dataset'] (src/utils/eval_modules.py:231-317):
 * per hand only the joints flagged in joints3d_valid_{r,l} (B,21; any non-zero value flags) are scored.  abs = mean
 * camera-space error, rao = mean error after subtracting the FIRST flagged joint, pa_ra = Procrustes error of that
 * root-aligned subset times hand_valid * is_valid (an invalid hand gives 0, not NaN, :217).  No joint flagged: NaN in all
 * three; one joint flagged: rao 0 and pa_ra NaN (scale 0 / 0, as the reference).  Two or three joints flagged: the reference's
 * compute_similarity_transform transposes its (n,3) input unless n is 2 or 3 (:144), so two joints are aligned as THREE points
 * in the plane and three joints as the three COLUMNS of the 3 x 3 array, the error running along the rows of the result; this
 * entry does the same.  h = nanmean of r and l.  Millimetres.
 * `in` is the struct of hands_eval_metrics_f32, every pointer of it mandatory (the 2-D ones are not read).
 * HANDS_EINVAL (nothing launched): a NULL pointer, B <= 0. */
typedef struct hands_eval_masked_out {
  float *rao_r, *rao_l, *rao_h, *abs_r, *abs_l, *abs_h, *pa_ra_r, *pa_ra_l, *pa_ra_h; /* (B) each */
} hands_eval_masked_out;

int hands_eval_metrics_masked_f32(const hands_eval_in* in, const float* joints3d_valid_r, const float* joints3d_valid_l,
                                  const hands_eval_masked_out* out, int B, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh metrics on device (csrc/mesh_metrics.hip), one launch per batch, no allocation, no host synchronisation, no atomics:
 * bit-reproducible from run to run and independent of the batch a sample sits in.  Replaces the host loop a user writes over
 * mano.v3d.cam.* (a V x V nearest-neighbour search per hand in numpy); the F-score is the FreiHAND evaluation's
 * calculate_fscore, the AUC its PCK curve, the alignment compute_similarity_transform of src/utils/eval_modules.py:136-187.
 *
 * Inputs fp32: vertices (B,V,3) with 1 <= V <= HANDS_MESH_MAX_V, joints (B,21,3), flags (B).  Per hand, two alignments:
 *   ra  the root joint j3d[:,0] is subtracted from joints and vertices, pred from pred and gt from gt, in fp32;
 *   pa  the similarity transform fitted (fp64) on the root-aligned V vertices -- for auc_*_j on the 21 joints, the alignment
 *       of mpjpe/pa/ra -- is applied to the root-aligned prediction.  Rank-deficient clouds as hands_eval_metrics_f32.
 * Outputs (B) each, HANDS_MESH_NQ quantities x {r, l, h}, h = nanmean of r and l:
 *   mpvpe    mean over vertices of |gt_v - pred_v|, millimetres;
 *   f5, f15  F = 2PR / (P + R), 0 when P + R = 0, with P = mean_i(min_j |gt_i - pred_j| < th), R = mean_j(min_i |pred_j - gt_i|
 *            < th), th = 0.005 m / 0.015 m, strict <;
 *   auc_v, auc_j  area under the PCK curve (fraction of vertices / joints with error <= t_k, t_k = k * 0.05 / 99 m,
 *            k = 0..99), trapezoid rule, divided by 0.05.
 * A hand with hand_valid * is_valid == 0 gives NaN in every output and its coordinates are not read; a valid hand with any
 * non-finite vertex or joint coordinate gives NaN in every output of that hand.  A constant prediction gives NaN in the pa
 * outputs, a constant ground truth mpvpe_pa 0.
 * HANDS_EINVAL (nothing launched): a NULL pointer, B <= 0, V outside [1, HANDS_MESH_MAX_V].
 * --------------------------------------------------------------------------------------------- */
#define HANDS_MESH_MAX_V 1024
#define HANDS_MESH_NQ 10
typedef struct hands_mesh_eval_in {
  const float *pred_v3d_r, *pred_v3d_l, *gt_v3d_r, *gt_v3d_l; /* (B,V,3) */
  const float *pred_j3d_r, *pred_j3d_l, *gt_j3d_r, *gt_j3d_l; /* (B,21,3) */
  const float *is_valid, *right_valid, *left_valid;           /* (B) */
} hands_mesh_eval_in;

typedef struct hands_mesh_eval_out { /* (B) each; quantity q, hand s (r, l, h) is pointer 3 * q + s of the struct */
  float *mpvpe_ra_r, *mpvpe_ra_l, *mpvpe_ra_h, *f5_ra_r, *f5_ra_l, *f5_ra_h, *f15_ra_r, *f15_ra_l, *f15_ra_h;
  float *auc_ra_v_r, *auc_ra_v_l, *auc_ra_v_h, *auc_ra_j_r, *auc_ra_j_l, *auc_ra_j_h;
  float *mpvpe_pa_r, *mpvpe_pa_l, *mpvpe_pa_h, *f5_pa_r, *f5_pa_l, *f5_pa_h, *f15_pa_r, *f15_pa_l, *f15_pa_h;
  float *auc_pa_v_r, *auc_pa_v_l, *auc_pa_v_h, *auc_pa_j_r, *auc_pa_j_l, *auc_pa_j_h;
} hands_mesh_eval_out;

int hands_eval_mesh_metrics_f32(const hands_mesh_eval_in* in, const hands_mesh_eval_out* out, int B, int V,
                                hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Distances from points to a triangle surface (csrc/mesh_distance.hip): brute force over the faces, no acceleration structure,
 * no allocation, no host synchronisation, no atomics, no runtime call in front of a launch (the launches record into a
 * hipGraph); bit-reproducible from run to run and independent of the batch a sample sits in.  The reference's lineage measures
 * the field between two hands to the nearest VERTEX (pytorch3d.ops.knn_points, src/utils/interfield.py); these entries measure
 * to the surface, and nothing here is pinned to pytorch3d, which is absent.
 *
 * hands_mesh_closest_f32: points (B,P,3), verts (B,V,3) fp32, faces (F,3) int32 shared by the batch, valid (B) or NULL.
 *   dist[b,p]      Euclidean distance from the point to the closed triangle, minimised over the faces: squared distances and
 *                  their comparison in fp32, a strict < in ascending face order (the lowest index wins an exact tie), one
 *                  square root at the end.  Point to triangle: the minimum of the three clamped segment distances and, where
 *                  the normal is not zero and the projection falls inside, the distance to the plane.  "Inside" and the plane
 *                  distance are fp32 too, except for a THIN face -- the sine of the angle at its first vertex is at most 1/64,
 *                  which slivers and caps are from every vertex -- where fp32 barycentrics are rounding noise: they are
 *                  fp64 from the fp32 vertices there, good down to a height of 1e-6 of the longest edge
 *                  (csrc/mesh_distance_device.h);
 *   face_idx[b,p]  (or NULL) that face;  closest[b,p] (or NULL) the closest point on it.
 *   A degenerate face -- a repeated vertex index, collinear vertices -- is the segment or the point it collapses to.  A face with
 *   an index outside [0, V) or with a non-finite vertex is skipped.  No face left, or F == 0: dist +inf, face_idx -1, closest
 *   NaN.  A query with a non-finite coordinate: dist NaN, face_idx -1, closest NaN.  A sample with valid[b] == 0: the same, and
 *   neither its points nor its vertices are read.
 *   One workgroup per (sample, HANDS_SURF_CHUNK queries); vertices and faces (16-bit indices) in 36 KB of static LDS.
 *   HANDS_EINVAL (nothing launched): NULL points / verts / dist, NULL faces with F != 0, B, P or V <= 0, F < 0,
 *   V > HANDS_MESH_MAX_V, F > HANDS_SURF_MAX_F.
 *
 * hands_mesh_signed_f32 (csrc/mesh_signed.hip): the inputs, limits, skip and tie rules of hands_mesh_closest_f32; the same walk over the faces also sums
 * the generalised winding number of the mesh about the query (Jacobson et al. 2013),
 *   w(p) = 1/(4 pi) sum_f Omega_f,  Omega_f = 2 atan2( a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b| ),
 * a = v0 - p, b = v1 - p, c = v2 - p (Van Oosterom & Strackee 1983), fp32, in ascending face order in one lane.  A term whose two
 * arguments are both 0 (a query on a vertex of the face) is 0, as is the term of a face whose fp32 normal is exactly zero (a
 * repeated index: the face hands_mesh_closest_f32 treats as a segment or a point); a skipped face adds nothing.  For a
 * closed, outward-oriented mesh w is 1 inside and 0 outside, -1 inside where the faces are oriented inwards.
 *   winding[b,p]   (or NULL) w;
 *   sdf[b,p]       -dist where |w| >= 0.5, else +dist, dist as hands_mesh_closest_f32 gives it;
 *   face_idx[b,p]  (or NULL) the closest face.
 *   No face left, or F == 0: winding 0, sdf +inf, face_idx -1.  A query with a non-finite coordinate, or valid[b] == 0 (nothing
 *   of the sample is read): winding NaN, sdf NaN, face_idx -1.  The mesh has to be closed for the sign to mean anything: an open
 *   boundary (MANO's wrist) leaves w near 0.5 around it -- hands_amd.seal_mesh closes it on the host.
 *   One workgroup per (sample, HANDS_SIGNED_CHUNK queries), a lane owns one query.  HANDS_EINVAL as hands_mesh_closest_f32, with
 *   sdf in the place of dist.
 *
 * hands_eval_surface_metrics_f32: the inputs and the two alignments (ra, pa) of hands_eval_mesh_metrics_f32, plus the face
 * list of each hand (F_r, F_l in [0, HANDS_SURF_MAX_F]; NULL only with F == 0).  With X the aligned prediction, Y the ground
 * truth and T the hand's faces, per hand and alignment, (B) each, millimetres, distances not squared:
 *   p2s      1000 * 1/2 [ mean_i d(X_i, surface(Y,T)) + mean_j d(Y_j, surface(X,T)) ], d as dist above;
 *   chamfer  1000 * 1/2 [ mean_i min_j |X_i - Y_j| + mean_j min_i |Y_j - X_i| ], the distances the F-score thresholds.
 * HANDS_SURF_NQ quantities x {r, l, h}, h = nanmean of r and l.  Sums are fp64 through one fixed tree.  NaN as the mesh
 * metrics: an invalid hand (not read), a valid hand with any non-finite vertex or joint coordinate, the pa outputs of a constant
 * prediction; a hand none of whose faces is usable (F == 0, every face with an index outside [0, V)) gives NaN in p2s and
 * leaves chamfer as it is.  Two launches: one workgroup per (sample, hand, alignment), then h.
 * HANDS_EINVAL (nothing launched): a NULL pointer, B <= 0, V outside [1, HANDS_MESH_MAX_V], F outside [0, HANDS_SURF_MAX_F].
 * --------------------------------------------------------------------------------------------- */
#define HANDS_SURF_MAX_F 4096
#define HANDS_SURF_CHUNK 512 /* queries per workgroup of hands_mesh_closest_f32 */
#define HANDS_SURF_NQ 4
int hands_mesh_closest_f32(const float* points, const float* verts, const int32_t* faces, const float* valid, float* dist,
                           int32_t* face_idx, float* closest, int B, int P, int V, int F, hands_stream_t stream);
#define HANDS_SIGNED_CHUNK 256 /* queries per workgroup of hands_mesh_signed_f32 */
int hands_mesh_signed_f32(const float* points, const float* verts, const int32_t* faces, const float* valid, float* sdf,
                          float* winding, int32_t* face_idx, int B, int P, int V, int F, hands_stream_t stream);

typedef struct hands_surf_eval_out { /* (B) each; quantity q, hand s (r, l, h) is pointer 3 * q + s of the struct */
  float *p2s_ra_r, *p2s_ra_l, *p2s_ra_h, *p2s_pa_r, *p2s_pa_l, *p2s_pa_h;
  float *chamfer_ra_r, *chamfer_ra_l, *chamfer_ra_h, *chamfer_pa_r, *chamfer_pa_l, *chamfer_pa_h;
} hands_surf_eval_out;

int hands_eval_surface_metrics_f32(const hands_mesh_eval_in* in, const int32_t* faces_r, const int32_t* faces_l, int F_r,
                                   int F_l, const hands_surf_eval_out* out, int B, int V, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal metrics on device (csrc/accel.hip): the acceleration error of compute_error_accel / eval_acc_pose
 * (src/utils/eval_modules.py:508-622) over T consecutive frames given in order, metres per second squared.  One launch per
 * entry, one workgroup per output row, no allocation, no host synchronisation, no atomics: the bits of a row depend on its
 * three frames alone -- not on T, on the row's position or on the run.
 *
 * hands_accel_error_f32: gt, pred (T,N,D) fp32 with D in 1..3, valid (T) or NULL, seq_id (T) or NULL, fps > 0.
 *   a[t] = (x[t-1] - 2 x[t] + x[t+1]) fps^2,   out[t] = mean_n | a_pred[t,n,:] - a_gt[t,n,:] |_2   for 1 <= t <= T-2;
 *   rows 0 and T-1 are NaN, the layout of eval_acc_pose after its padding.  Row t is NaN, and no coordinate of its window is
 *   read, when one of the frames t-1, t, t+1 has valid == 0 (NULL: every frame is valid) or when the three frames do not carry
 *   the same seq_id (NULL: the call is one sequence, as in the reference).  Inputs are fp32, everything from the first
 *   subtraction on is fp64, the result is rounded once to fp32.  A non-finite coordinate in a valid window propagates as IEEE
 *   arithmetic propagates it (a NaN gives NaN, an infinity +inf or NaN), with no special case.  No upper limit on N: a lane walks
 *   the points lane, lane + 256, ...  Sums are fp64 in one fixed order: the lane's points in index order, a shuffle tree inside
 *   the wave, the waves in order.
 *   HANDS_EINVAL (nothing launched): NULL gt / pred / out, T <= 0, N <= 0, D outside 1..3, fps not finite or <= 0.
 *
 * hands_eval_accel_metrics_f32: the inputs of hands_eval_mesh_metrics_f32 with B read as T (any V >= 1), seq_id (T) or NULL.
 *   A hand's frame is valid where {right,left}_valid * is_valid != 0; the window and sequence rules are those above, per hand.
 *   HANDS_ACCEL_NQ quantities x {r, l, h}, (T) each, h = nanmean of r and l (NaN when both are):
 *     acc      the V vertices, root-relative: joint 0 of j3d of the same frame subtracted, pred from pred and gt from gt
 *              (acc_h is the reference's acc/h);
 *     acc_j    the 21 joints, root-relative;
 *     acc_abs  the 21 joints as they are (camera space).
 *   Both hands of a row in one workgroup.  HANDS_EINVAL (nothing launched): a NULL in, out or member of either, T <= 0,
 *   V <= 0, fps not finite or <= 0.
 * --------------------------------------------------------------------------------------------- */
#define HANDS_ACCEL_NQ 3
int hands_accel_error_f32(const float* gt, const float* pred, const float* valid, const int32_t* seq_id, float* out, int T,
                          int N, int D, float fps, hands_stream_t stream);

typedef struct hands_accel_eval_out { /* (T) each; quantity q, hand s (r, l, h) is pointer 3 * q + s of the struct */
  float *acc_r, *acc_l, *acc_h, *acc_j_r, *acc_j_l, *acc_j_h, *acc_abs_r, *acc_abs_l, *acc_abs_h;
} hands_accel_eval_out;

int hands_eval_accel_metrics_f32(const hands_mesh_eval_in* in, const int32_t* seq_id, const hands_accel_eval_out* out, int T,
                                 int V, float fps, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Temporal smoothing on device (csrc/smooth.hip): the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) over the MANO
 * parameters of hand-streams, rotations filtered on SO(3).  DESIGN.md section 7 "Temporal smoothing" is the specification
 * (frame states, channel updates, Log and Exp with their branches); the reference has no counterpart.  One launch, one wave per
 * (side, stream), time a serial loop inside the kernel; no allocation, no host synchronisation, no atomics.  fp32 in, fp64
 * arithmetic, each output rounded once; a frame that is not filtered is copied bit for bit.
 *
 * Rows are T time steps of S parallel streams, row t * S + s: pose (T*S,16,3,3), beta (T*S,10), cam (T*S,3), valid (T*S) or
 * NULL (every frame valid), seq_id (T*S) or NULL (one sequence), shared by the sides.  A frame is usable when valid != 0 and
 * its 157 inputs are finite; an unusable frame, and the first usable frame after one or after a change of seq_id, pass through.
 * state: NULL (start fresh, keep nothing) or S blocks of hands_smooth_state_bytes() bytes per side, 8-byte aligned, opaque,
 * all zero before the first call; read at the start of the call and written back at its end, so a stream filtered in any split
 * into calls gives the bits of one call.  Outputs must not overlap inputs, state or each other.
 * shape_mode: the One-Euro filter, the running mean since the stream started, or the input.
 * HANDS_EINVAL (nothing launched): NULL sides / cfg or a NULL pose, beta, cam or output of a side, nsides outside 1..2,
 * T < 1, S < 1, fps / min_cutoff / d_cutoff not finite or <= 0, beta not finite or < 0, an unknown shape_mode.
 * --------------------------------------------------------------------------------------------- */
#define HANDS_SMOOTH_SHAPE_FILTER 0
#define HANDS_SMOOTH_SHAPE_MEAN 1
#define HANDS_SMOOTH_SHAPE_NONE 2

typedef struct hands_smooth_side {
  const float *pose, *beta, *cam, *valid;
  float *pose_out, *beta_out, *cam_out;
  void* state;
} hands_smooth_side;

typedef struct hands_smooth_cfg { /* index 0: rotations, 1: shape, 2: camera; cutoffs in Hz */
  double min_cutoff[3], beta[3], d_cutoff[3];
  int shape_mode;
} hands_smooth_cfg;

long long hands_smooth_state_bytes(void);
int hands_smooth_mano_f32(const hands_smooth_side* sides, int nsides, const long long* seq_id, int T, int S, float fps,
                          const hands_smooth_cfg* cfg, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MANO fitting on device (csrc/fit.hip): a Levenberg-Marquardt fit of MANO to 21 3-D joints per hand -- the 16 rotations of the
 * FULL pose (pose_mean added; hands_mano_heads_f32 takes it as axis-angle Log R_j - pose_mean_j), beta (10) and a translation (3).  DESIGN.md
 * section 7 "MANO fitting" is the specification (residual, analytic Jacobian, damping, accept / reject); the reference has no
 * counterpart.  One launch for both hands, grid (B, n_sides), one workgroup per hand, the hands independent: a hand's outputs
 * do not depend on B, on its row, on n_sides or on the other rows.  No allocation, no host synchronisation, no atomics; exactly
 * `iters` iterations whatever the data.  fp32 in, fp64 arithmetic, each output rounded once.
 *
 * Per side: joints (B,21,3) in metres, in this library's joint order (16 + the tips 744/320/443/554/671); weights (B,21) >= 0 or
 * NULL (all 1) -- a joint of weight 0 is never read, its coordinates may be NaN; valid (B) or NULL (every row fitted);
 * init_pose (B,16,3,3), init_beta (B,10), init_transl (B,3): all three (the initial state) or all NULL (the rest pose,
 * rigidly aligned to the joints).  Outputs: pose (B,16,3,3), beta (B,10), transl (B,3), rmse (B) = sqrt(sum_k w_k |j_k + t -
 * y_k|^2 / sum_k w_k) in metres, steps (B) int32 = accepted steps; they must not overlap the inputs or each other.
 * A row is not fitted when valid == 0, fewer than four joints have weight > 0, a weighted joint or a given initial value is not
 * finite: pose = (I, Exp(hands_mean_1..15)), beta = 0, transl = 0, rmse = NaN, steps = 0.  iters == 0 returns the initial state
 * and its rmse.
 * consts: pose_mean (48), J_template (16,3), J_shapedirs (48,10) as in hands_mano_consts, and the rows of the five tip vertices
 * of v_template (5,3), shapedirs (5,3,10), lbs_weights (5,16) and their posedirs columns (135,15) [feature][3 tip + coordinate].
 * HANDS_EINVAL (nothing launched): NULL sides / cfg, a NULL constant, joints or output of a side, one or two of init_* given,
 * B <= 0, n_sides outside 1..2, iters < 0, lambda_beta / lambda_pose / mu0 negative or not finite.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_mano_fit_consts {
  const float *pose_mean, *J_template, *J_shapedirs;
  const float *tip_v_template, *tip_shapedirs, *tip_lbs_weights, *tip_posedirs;
} hands_mano_fit_consts;

typedef struct hands_mano_fit_side {
  hands_mano_fit_consts consts;
  const float *joints, *weights, *valid, *init_pose, *init_beta, *init_transl;
  float *pose, *beta, *transl, *rmse;
  int32_t* steps;
} hands_mano_fit_side;

typedef struct hands_fit_cfg { /* lambda_*: weights of the shape and pose priors; mu0: the first damping */
  int iters;
  double lambda_beta, lambda_pose, mu0;
} hands_fit_cfg;

int hands_mano_fit_f32(const hands_mano_fit_side* sides, int n_sides, const hands_fit_cfg* cfg, int B, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MANO fitting to 2-D keypoints (csrc/fit.hip, beside the 3-D fit and on its device routines): the same 61 unknowns fitted to 21
 * keypoints in PIXELS under the perspective projection of K.  DESIGN.md section 7 "MANO fitting to 2-D keypoints" is the
 * specification, tests/fit2d_ref.py its fp64 restatement.  Launch and guarantees as hands_mano_fit_f32: grid (B, n_sides), one
 * four-wave workgroup per hand, fp32 in, fp64 arithmetic, one rounding per output, no atomics, no allocation, no host
 * synchronisation (the call can be captured); a hand's outputs do not depend on B, its row, n_sides or its neighbours; exactly
 * iters_rigid + iters iterations whatever the data.  The fit reproduces the KEYPOINTS; depth, scale and the 3-D hand are not
 * recovered uniquely from one view.
 *
 * Per side the fields of hands_mano_fit_side with kp2d (B,21,2) in place of joints, and three more outputs: start (B) int32, the
 * index 0..23 of the signed permutation the generated initial state took (-1 with a caller's state or a row not fitted), j3d
 * (B,21,3) = joints + transl in camera space and j2d (B,21,2) = their projection in pixels, both for all 21 joints.  K (B,3,3),
 * shared by the sides; only rows 0 and 1 are read.  rmse = sqrt(sum_k w_k |pi(X_k) - y_k|^2 / sum_k w_k) in pixels, without the
 * robust kernel and the priors.
 * cfg: iters_rigid iterations that free only the global rotation and the translation, then iters that free everything (or all
 * but beta with fit_shape == 0); robust_sigma > 0 switches the Geman-McClure kernel on (pixels); a state in which a weighted
 * joint has Z <= z_min costs +inf; prior_to_init != 0 with a caller's state makes that state the reference of both priors.
 * A row is not fitted when valid == 0, fewer than four keypoints have weight > 0, a weighted keypoint, an entry of K rows 0-1 or a
 * given initial value is not finite, K00 <= 0 or K11 <= 0, the initial state trips the depth guard, or no start candidate
 * qualifies: the outputs of an unfitted row of hands_mano_fit_f32, start = -1, j3d and j2d NaN.
 * HANDS_EINVAL (nothing launched): the cases of hands_mano_fit_f32, a NULL K, start, j3d or j2d, iters_rigid < 0, robust_sigma
 * negative or not finite, z_min not finite or <= 0.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_mano_fit2d_side {
  hands_mano_fit_consts consts;
  const float *kp2d, *weights, *valid, *init_pose, *init_beta, *init_transl;
  float *pose, *beta, *transl, *rmse;
  int32_t *steps, *start;
  float *j3d, *j2d;
} hands_mano_fit2d_side;

typedef struct hands_fit2d_cfg {
  int iters_rigid, iters;
  double lambda_beta, lambda_pose, mu0, robust_sigma, z_min;
  int fit_shape, prior_to_init;
} hands_fit2d_cfg;

int hands_mano_fit2d_f32(const hands_mano_fit2d_side* sides, int n_sides, const float* K, const hands_fit2d_cfg* cfg, int B,
                         hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MANO fitting to 778 vertices (csrc/fit_verts.hip, on the device routines of csrc/fit_device.h): the same 61 unknowns fitted to
 * the 778 vertices of a mesh in MANO topology, in metres.  DESIGN.md section 7 "MANO fitting to 778 vertices" is the
 * specification, tests/fit_verts_ref.py its fp64 restatement.  Launch and guarantees as hands_mano_fit_f32: grid (B, n_sides),
 * one four-wave workgroup per hand, fp32 in, fp64 arithmetic, one rounding per output, no atomics, no allocation, no host
 * synchronisation (the call can be captured); every sum has an order the code alone fixes: a hand's outputs do not depend on
 * B, its row, n_sides or its neighbours and are the same bits from launch to launch; exactly iters iterations whatever the
 * data.  The fit reproduces the VERTICES: where the mesh is a MANO mesh it recovers pose and shape; it does no
 * correspondence-free registration (vertex n of the target is vertex n of the model) and fits no scale.
 *
 * Per side the fields of hands_mano_fit_side with verts (B,778,3) in place of joints and weights (B,778) >= 0 or NULL (all 1) -- a
 * vertex of weight 0 (or of a weight that is negative or no number) is never read, its coordinates may be NaN: that is how a
 * partial or occluded mesh is fitted --, and one more output: j3d (B,21,3) = the fitted joints (16 + the tips 744/320/443/554/671)
 * + transl.  rmse = sqrt(sum_n w_n |v_n + t - y_n|^2 / sum_n w_n) in metres, priors left out.  The initial state without init_*
 * is the rest hand under the weighted rigid alignment of its vertices onto verts.
 * A row is not fitted when valid == 0, fewer than four vertices have weight > 0, a weighted vertex or a given initial value is
 * not finite: the outputs of an unfitted row of hands_mano_fit_f32, j3d NaN.  iters == 0 returns the initial state, its rmse
 * and its j3d.
 * consts: pose_mean (48), J_template (16,3), J_shapedirs (48,10) as in hands_mano_fit_consts; v_template (778,3), shapedirs
 * (778,3,10) and lbs_weights (778,16) as the asset has them; posedirs_vm (778,135,3): the asset's posedirs (135, 778*3) with the
 * vertex first, posedirs_vm[(n * 135 + f) * 3 + c] = posedirs[f][3 n + c], so that a vertex's 405 values are contiguous.
 * HANDS_EINVAL (nothing launched): the cases of hands_mano_fit_f32, a NULL among these constants, a NULL verts or j3d.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_mano_fit_verts_consts {
  const float *pose_mean, *J_template, *J_shapedirs;
  const float *v_template, *shapedirs, *lbs_weights;
  const float* posedirs_vm;
} hands_mano_fit_verts_consts;

typedef struct hands_mano_fit_verts_side {
  hands_mano_fit_verts_consts consts;
  const float *verts, *weights, *valid, *init_pose, *init_beta, *init_transl;
  float *pose, *beta, *transl, *rmse;
  int32_t* steps;
  float* j3d;
} hands_mano_fit_verts_side;

int hands_mano_fit_verts_f32(const hands_mano_fit_verts_side* sides, int n_sides, const hands_fit_cfg* cfg, int B,
                             hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * MANO fitting to surface correspondences (csrc/fit_surf.hip, on csrc/fit_device.h and csrc/fit_mesh_device.h): the 61 unknowns,
 * the iteration and the priors of hands_mano_fit_verts_f32 with P data rows per hand that are points ON the model's faces.
 * DESIGN.md section 7 "MANO fitting to surface correspondences and ICP registration" is the specification,
 * tests/fit_surf_ref.py its fp64 restatement.  Launch and guarantees as hands_mano_fit_verts_f32; the rows stream in tiles of 16
 * from global memory, so P (1 .. HANDS_FIT_SURF_MAX_P, the same for every hand of a call) bounds time, not memory.
 *
 * Per side: points (B,P,3) the targets y_k in metres; face_idx (B,P) int32 in [0, 1538), an index into consts.faces; bary (B,P,3)
 * the coefficients b_k, finite, neither clamped nor normalised; weights (B,P) >= 0 or NULL (all 1); normals (B,P,3) or NULL; valid
 * and init_* as hands_mano_fit_side.  c_k = sum_i b_ki v_{faces[f_k][i]}; the residual is sqrt(w_k) A_k (c_k + t - y_k), A_k = I
 * without normals, with tangent_weight == 1 (the normals are then not read) or for a zero normal, else
 * A_k = n n^T + sqrt(tangent_weight) (I - n n^T) with n = normals[k] as given.
 * rmse = sqrt(sum_k w_k |c_k + t - y_k|^2 / sum_k w_k), Euclidean: without A and without the priors.
 * A row of weight 0 (or of a weight that is negative or no number) is never read: its point, coefficients and normal may be NaN
 * and its face -1.  A tile of 16 rows whose weights are all zero is skipped; zero-weight rows appended behind the last weighted
 * one change no bit of any output.  The initial state without init_* is the rest hand under the weighted rigid alignment of its
 * surface points onto the targets.  Outputs: those of hands_mano_fit_verts_f32 and verts (B,778,3) = the fitted vertices +
 * transl.  iters == 0 returns the initial state, its rmse, j3d and verts.
 * A hand is not fitted when valid == 0, fewer than four rows have weight > 0, a weighted row has a weight of +inf, a non-finite
 * point, coefficient or (where they are read) normal, or a face outside [0, 1538) -- checked before anything is read through
 * it --, or a given initial value is not finite: the outputs of an unfitted row of hands_mano_fit_verts_f32, verts NaN.
 * consts: those of hands_mano_fit_verts_f32 and faces (1538,3) int32, vertex indices in [0, 778).
 * HANDS_EINVAL (nothing launched): the cases of hands_mano_fit_verts_f32 with points / face_idx / bary / verts / faces among the
 * required pointers, P outside [1, HANDS_FIT_SURF_MAX_P], tangent_weight outside [0, 1] or no number.
 * --------------------------------------------------------------------------------------------- */
#define HANDS_FIT_SURF_MAX_P 16384
typedef struct hands_mano_fit_surf_consts {
  hands_mano_fit_verts_consts mano;
  const int32_t* faces;
} hands_mano_fit_surf_consts;

typedef struct hands_mano_fit_surf_side {
  hands_mano_fit_surf_consts consts;
  const float *points, *weights, *valid, *init_pose, *init_beta, *init_transl;
  float *pose, *beta, *transl, *rmse;
  int32_t* steps;
  float *j3d, *verts;
  const int32_t* face_idx;
  const float *bary, *normals;
} hands_mano_fit_surf_side;

typedef struct hands_fit_surf_cfg { /* hands_fit_cfg and the weight of the tangential part of a residual */
  int iters;
  double lambda_beta, lambda_pose, mu0, tangent_weight;
} hands_fit_surf_cfg;

int hands_mano_fit_surf_f32(const hands_mano_fit_surf_side* sides, int n_sides, const hands_fit_surf_cfg* cfg, int B, int P,
                            hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Closest point with what a fit needs (csrc/mesh_correspond.hip, on csrc/mesh_distance_device.h): hands_mesh_closest_f32 -- the
 * same walk, tie rule, limits, skip rules and NaN / -1 conventions, the same bits in dist, face_idx and closest -- plus, per
 * query, the coefficients of the closest point on its face, that face's unit normal and a gated weight.  One launch.
 *   bary[b,p]    the coefficients b with closest ~ sum_i b_i verts[faces[face_idx][i]], from the candidate that gave the minimum
 *                and in its arithmetic: the plane (1 - v - w, v, w), edge ab (1 - t, t, 0), ac (1 - t, 0, t), bc (0, 1 - t, t);
 *                NaN where face_idx is -1;
 *   normal[b,p]  ab x ac / |ab x ac| of that face in fp32, zero for a face whose fp32 normal is zero and where face_idx is -1;
 *   w_out[b,p]   w_in (1 with w_in NULL) where max_dist <= 0 or dist <= max_dist, else 0 (a NaN dist passes no positive gate).
 * A query with w_in == 0 (or negative, or no number) is not read: dist NaN, face_idx -1, closest and bary NaN, normal 0, w_out 0.
 * HANDS_EINVAL (nothing launched): as hands_mesh_closest_f32, and a NULL face_idx, closest, bary, normal or w_out, max_dist no number.
 * --------------------------------------------------------------------------------------------- */
int hands_mesh_correspond_f32(const float* points, const float* verts, const int32_t* faces, const float* valid, const float* w_in,
                              float max_dist, float* dist, int32_t* face_idx, float* closest, float* bary, float* normal,
                              float* w_out, int B, int P, int V, int F, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The validation loss dict on device, forward only (csrc/loss.hip): compute_loss_light of
 * src/callbacks/loss/loss_arctic_sf.py:20-206 (vector_loss / joints_loss / grasp_loss / render_loss of
 * src/utils/loss_modules.py:97-152) with the weighting and the total of src/models/generic/wrapper.py:19-23,100-115.
 * Two launches on `stream` whatever terms are present, no host synchronisation, no atomics: the outputs are
 * bit-reproducible from run to run.
 *
 * Every value is the mean over ALL B*D elements of (difference -> square or abs -> x validity -> x is_*_loss), elements in
 * fp32, accumulation in fp64.  A vector_loss term (cam_t, pose, beta, transl, center, corner) whose validity vector sums to
 * zero is exactly 0, NaNs included; otherwise a NaN of an invalid sample propagates, as in the reference.
 *
 * Shapes (fp32 unless stated; flags and validities are per sample (B) except joints_valid (B,21)):
 *   pred_pose (B,16,3,3) rotation matrices against gt_pose (B,48) axis-angle; beta (B,10); j3d (B,21,3) camera-space joints
 *   (compared root-relative); j2d (B,21,2) normalised; cam_wp / cam_wp_init (B,3); grasp logits (B,9) against int64 labels
 *   (B) -- ASSUMED in [0, 9), NOT checked on the device; mask (B,S_mask,S_mask) and depth (B,S_depth,S_depth), contiguous;
 *   center (B,2), corner (B,8).
 * The first HANDS_LOSS_N_MANDATORY pointers are mandatory.  Each optional group (grasp, mask, depth, center+corner) is all
 * there or all NULL; a NULL group's keys are skipped (outputs 0, not part of the total).
 *
 * Output order (HANDS_LOSS_NKEYS = 21) and weights, as the reference's dict: cam_t/r 1, cam_t/l 1, kp2d/r 5, kp3d/r 5,
 * pose/r 10, beta/r 0.001, kp2d/l 5, kp3d/l 5, pose/l 10, transl/l 1, beta/l 0.001, grasp/{r,l} 0.1, mask/{r,l} 10,
 * depth/{r,l} 1, center/{r,l} 1, corner/{r,l} 1.  out_weighted21[k] = out_unweighted21[k] * weight[k] (fp32), out_total[0] =
 * their sum over the present keys in that order (fp32).
 *
 * workspace: hands_loss_workspace_bytes(B, S_mask, S_depth) bytes (0 for a bad shape), 8-byte aligned, caller-owned, every
 * byte the second launch reads is written by the first (no zero-fill needed).  S of an absent group is ignored.
 * HANDS_EINVAL (nothing launched): a NULL mandatory pointer / workspace / output, B <= 0, a half-given group, S outside
 * [1, 32768] for a present group.
 * --------------------------------------------------------------------------------------------- */
#define HANDS_LOSS_NKEYS 21
#define HANDS_LOSS_N_MANDATORY 31
typedef struct hands_loss_in {
  /* mandatory (31) */
  const float *pred_pose_r, *pred_pose_l, *pred_beta_r, *pred_beta_l, *pred_j3d_r, *pred_j3d_l, *pred_j2d_r, *pred_j2d_l;
  const float *pred_cam_wp_r, *pred_cam_wp_l, *pred_cam_wp_init_r, *pred_cam_wp_init_l;
  const float *gt_pose_r, *gt_pose_l, *gt_beta_r, *gt_beta_l, *gt_j3d_r, *gt_j3d_l, *gt_j2d_r, *gt_j2d_l;
  const float *gt_cam_wp_r, *gt_cam_wp_l;
  const float *right_valid, *left_valid, *joints_valid_r, *joints_valid_l;
  const float *is_cam_loss, *is_j2d_loss, *is_j3d_loss, *is_pose_loss, *is_beta_loss;
  /* use_grasp_loss */
  const float *pred_grasp_r, *pred_grasp_l;
  const long long *gt_grasp_r, *gt_grasp_l;
  const float *grasp_valid_r, *grasp_valid_l, *is_grasp_loss;
  /* use_render_seg_loss */
  const float *pred_mask_r, *pred_mask_l, *gt_mask_r, *gt_mask_l, *render_valid_r, *render_valid_l, *is_mask_loss;
  /* use_depth_loss */
  const float *pred_depth_r, *pred_depth_l, *gt_depth_r, *gt_depth_l, *is_depth_loss;
  /* regress_center_corner */
  const float *pred_center_r, *pred_center_l, *gt_center_r, *gt_center_l;
  const float *pred_corner_r, *pred_corner_l, *gt_corner_r, *gt_corner_l;
} hands_loss_in;

long long hands_loss_workspace_bytes(int B, int S_mask, int S_depth);
int hands_loss_light_f32(const hands_loss_in* in, int B, int S_mask, int S_depth, void* workspace,
                         float* out_unweighted21, float* out_weighted21, float* out_total, hands_stream_t stream);

/* GT preprocessing of the wrapper's test mode (src/callbacks/process/process_arctic.py:4-75):
 *   hands_mano_pose_aa_f32   = hands_mano_pose_f32 for AXIS-ANGLE input (B,48) (GT MANO parameters);
 *   hands_gt_targets_f32     : Tr0 = mean_j(j3d_full - joints); v3d_cam = verts + Tr0;
 *                              cam_t = j3d_full[0] - joints[0];
 *                              cam_t_wp = [2 f / (res * cam_t.z + 1e-9), cam_t.x, cam_t.y]  (common/camera.py:10-29);
 *   hands_unnormalize_kp2d_f32: 0.5 * res * (x + 1)  (common/data_utils.py:368-373, generic/wrapper.py:118-134). */
int hands_mano_pose_aa_f32(const hands_mano_consts* c, const float* axis_angle, const float* betas,
                           int ld_betas, float* blend_in, int ld_blend, float* A, float* joints16,
                           int B, hands_stream_t stream);
int hands_gt_targets_f32(const float* joints, const float* verts, const float* j3d_full, const float* K,
                         float img_res, float* v3d_cam, float* cam_t, float* cam_t_wp, int B, int NV,
                         hands_stream_t stream);
int hands_unnormalize_kp2d_f32(const float* x, float* out, long long n, float img_res,
                               hands_stream_t stream);

/* ---- (f2) crop / KPE front-end, the step before the path -------------------------------------------
 * hands_frontend_boxes_f32: per sample and hand, from the normalised GT 2-D joints (B,21,ld>=2):
 *   box [x0,y0,w,h] = int16-truncated min/max of ((j+1)/2)*(res-1), clipped to [0,res-1]
 *                                                  (src/datasets/hands_light_dataset.py:137-152);
 *   crop window [x0,y0,x1,y1] of crop_and_pad (common/data_utils.py:495-509; an empty box -> whole image);
 *   the float32 2x3 affine gen_trans_from_patch_cv builds for it (common/data_utils.py:56-91, rot=0);
 *   center (2) / corner (8) angles atan2(p - c, f) of the window (hands_light_dataset.py:256-279); K == NULL: args.no_intrx
 *   (hands_light_dataset.py:247-253) -- the encodings use f = c = img_res / 2 (a float64 matrix: the corner angles are then
 *   evaluated in double like the center angles) instead of the camera's intrinsics; hands_frontend_dense_maps_f32 likewise.
 *   bbox_og = the box itself, or [0,0,res-1,res-1] when empty (hands_light_dataset.py:145-152).
 * hands_warp_affine_cubic_norm_f32: cv2.warpAffine(src, trans, (Wo,Ho), INTER_CUBIC) with constant-0
 *   border (generate_patch_image_clean, common/data_utils.py:423-460), then clip to [0,1] and
 *   (x - mean)/std (hands_light_dataset.py:171-178,528).  src (B,3,H,W) in [0,1], out (B,3,Ho,Wo);
 *   trans (B,6) device pointer or NULL for the identity; mean3/std3 are HOST pointers to 3 floats.
 *   OpenCV is not vendored by the reference: the kernel follows its published fixed-point cubic
 *   remap (see oracle/frontend_oracle.py, "parity unpinned"). */
/* Per-pixel maps of the crop windows for pos_enc 'dense' / 'dense_latent' (nch = 2) and 'cam_conv' (nch = 6)
 * (src/datasets/hands_light_dataset.py:281-333): angle (B, nch, img_res, img_res) = atan2(x - cx, fx), atan2(y - cy, fy)
 * (, x - cx, y - cy, 2 x / img_res - 1, 2 y / img_res - 1) for the window pixels x in [x0, x1], y in [y0, y1] -- first map index x
 * -- in the top-left corner of a zero map; mask (B, img_res, img_res) = 1 on the window.  bbox (B, 4) int32 [x0, y0, x1, y1] as
 * written by hands_frontend_boxes_f32, K (B, 3, 3).  The inputs of hands_dense_posenc_f32. */
int hands_frontend_dense_maps_f32(const int32_t* bbox, const float* K, float* angle, float* mask, int B, int img_res, int nch,
                                  hands_stream_t stream);

int hands_frontend_boxes_f32(const float* j2d_r, const float* j2d_l, int ld, const float* K, int B,
                             int img_res, int out_res, double bbox_scale,
                             int32_t* bbox_r, int32_t* bbox_l, int32_t* bbox_og_r, int32_t* bbox_og_l,
                             float* trans_r, float* trans_l, float* center_r, float* center_l,
                             float* corner_r, float* corner_l, hands_stream_t stream);
int hands_warp_affine_cubic_norm_f32(const float* src, const float* trans, float* out, int B, int H, int W,
                                     int Ho, int Wo, const float* mean3, const float* std3,
                                     hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Soft-silhouette renderer of the predicted meshes (csrc/render.hip), forward only: MANORenderer / DiffRenderer,
 * src/models/hands_light/renderer.py:112-207, called at hands_light/model.py:413-420 on mano.v3d.cam.{r,l}.  The reference
 * delegates to pytorch3d (MeshRasterizer: blur_radius > 0, faces_per_pixel = 10, perspective_correct = False; then
 * SoftSilhouetteShader), which is third party and absent: the kernel restates the published naive rasterize_meshes path and
 * sigmoid_alpha_blend ("parity unpinned"; the semantics are written out in the header of csrc/render.hip).
 *   verts (B, n_verts, 3) in the camera frame, hand b at verts + b * ld_verts (ld_verts >= 3 n_verts floats);
 *   faces (n_faces, 3) int32, shared by the batch; a face with an index outside [0, n_verts) or a vertex at Z <= 0 is skipped
 *   (the latter a stated deviation: pytorch3d projects such vertices through the camera centre);
 *   K (B, 3, 3): only K00, K11, K02, K12 are read (no skew), in pixels of the S x S image;
 *   pixel (r, c) samples the image point (c + 0.5, r + 0.5); sigma and blur_radius in squared NDC units
 *   (the reference: 1e-5 and log(1/1e-6 - 1) * 1e-5); faces_per_pixel nearest candidates are blended, ties to the lower index.
 *   mask (B, S, S) = alpha in [0, 1].  Optional (NULL = not written), from the same pass, over the faces that CONTAIN the pixel:
 *   face_idx (B, S, S) int32, -1 where empty, and zbuf (B, S, S), the screen-space interpolated depth, 0 where empty.
 *   Every pixel of every output is written, whatever the faces: n_faces = 0 (faces must still be non-NULL) gives mask 0,
 *   face_idx -1, zbuf 0.  Skipped besides the two kinds above: a face with a NaN vertex, a face whose projected |area| (the edge
 *   function of its corners, twice the triangle's) is <= 1e-8, collinear ones included; a face with an infinite vertex is a
 *   candidate at no pixel.  Each of these leaves every output bit-equal to the call without the face.  An edge of squared NDC
 *   length <= 1e-8 counts as its END point in the distance to the face's outline.  Equal depths: faces are visited in index
 *   order and a later face replaces an earlier one only when strictly nearer, in the top faces_per_pixel as in face_idx / zbuf;
 *   the depths of translated copies of a fronto-parallel face are bit-equal.  ld_verts > 3 n_verts: the padding is not read.
 * HANDS_EINVAL (nothing launched): faces_per_pixel outside [1, 10]; a vertex block that does not fit in LDS beside the face
 * list (12 n_verts + 24 608 > 65 536 bytes, i.e. n_verts > 3410); sigma <= 0; blur_radius < 0; S outside [1, 16384].
 * n_faces is unbounded: a tile whose face list overflows its LDS share is processed in chunks.  The tile and the list are
 * the shaded renderer's (HANDS_SHADE_TILE_W, _TILE_H, _LIST_CAP below): the two kernels share csrc/raster_tile.h. */
int hands_render_silhouette_f32(const float* verts, int ld_verts, int n_verts, const int32_t* faces, int n_faces, const float* K, int B, int S, float sigma, float blur_radius, int faces_per_pixel, float* mask, int32_t* face_idx, float* zbuf, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Shaded renderer of up to four meshes per image (csrc/shade.hip), forward only: the hard z-buffer pictures of
 * common/rend_utils.py::Renderer (overlay and rotated side views).  The reference draws them with pyrender on OpenGL, which
 * is third party and absent: "parity unpinned"; the semantics are written out in DESIGN.md section 7 and restated in fp64 in
 * tests/shade_ref.py.  Two launches per picture:
 *
 * hands_mesh_prepare_f32, once per mesh: per (image, vertex) the rigid transform P' = R P + t (T (B, 3, 4) row-major, NULL =
 *   identity), the area-weighted vertex normal (the sum of (P'1 - P'0) x (P'2 - P'0) over the faces that hold the vertex, in
 *   ascending face order, gathered through a CSR table: csr_off (n_verts + 1) offsets into csr_face, the face indices; no
 *   atomics, bit-reproducible; a squared sum <= 1e-30 gives the zero vector; a face whose cross product is not finite adds
 *   nothing) and the projection of the silhouette renderer (K00, K11, K02, K12 only; csrc/raster_tile.h).  Writes 8 floats
 *   per vertex into the caller's workspace, image b's vertex v at workspace + 8 (b n_verts + v): P'x P'y P'z nx | ny nz xn yn.
 *   hands_mesh_workspace_floats(B, n_verts) = 8 B n_verts.  A face index of csr_face or a vertex index of faces outside its
 *   range is skipped.
 *
 * hands_render_shaded_f32: one workgroup of 256 lanes per (image, HANDS_SHADE_TILE_W x HANDS_SHADE_TILE_H pixels).  The faces
 *   of every mesh that is valid for the image (valid (B) floats, NULL or != 0 = present) are binned against the tile in
 *   (mesh, face) order into a list of HANDS_SHADE_LIST_CAP records in LDS, processed in chunks when it overflows.  A face
 *   covers a pixel under the silhouette renderer's rule (csrc/raster_tile.h holds it for both: all Z > 0, |area| > 1e-8,
 *   w0, w1, w2 > 0 with the area + 1e-8 denominator, both windings); depth is perspective-correct (1/z = sum w_i / z_i),
 *   the nearest wins, equal depths go to the lower (mesh, face).
 *   The winner is shaded with interpolated position and normal: glTF 2.0 metallic-roughness, one directional light of
 *   intensity 3 along the view axis, ambient 0.5, two-sided.  Uncovered pixels take image (B, 3, S, S), or 1.0 when NULL.
 *   Outputs, each optional (NULL = not written): rgb (B, S, S, 3) floats, rgb8 (B, S, S, 3) = floor(255 clamp(rgb, 0, 1)),
 *   depth (B, S, S) with 0 where empty, face_id (B, S, S) with -1 where empty, else face index + the mesh's face_offset.
 *   scene is a HOST pointer, read before the call returns.  No allocation, no synchronisation: capturable.
 *   A mesh with n_faces = 0 (faces still non-NULL) or valid[b] == 0 draws nothing in image b, wherever it stands among the
 *   meshes; with nothing to draw every requested output is still written (background, depth 0, face_id -1).  Each output
 *   requested alone is bit-equal to the same output of a call that requests all four.  A zero interpolated normal (squared
 *   length <= 1e-30: an empty CSR row, opposite faces) is replaced by the view direction.
 * HANDS_EINVAL (nothing launched): n_meshes outside [1, 4], a NULL workspace / faces, a workspace that is not 16-byte aligned (both
 * entries), S outside [1, 16384], no output at all.
 * HANDS_SHADE_TILE_W, _TILE_H and _LIST_CAP are the tile and the face list of csrc/raster_tile.h: hands_render_silhouette_f32
 * uses the same tile and list. */
#define HANDS_SHADE_MAX_MESHES 4
#define HANDS_SHADE_TILE_W 32
#define HANDS_SHADE_TILE_H 8
#define HANDS_SHADE_LIST_CAP 384
typedef struct hands_shade_mesh {
  const float* workspace;      /* (B, n_verts, 8) written by hands_mesh_prepare_f32 */
  const int32_t* faces;        /* (n_faces, 3), shared by the batch */
  const float* valid;          /* (B) or NULL */
  int32_t n_verts, n_faces;
  int32_t face_offset;         /* added to the face index in face_id */
  float color[3];              /* base colour in [0, 1] */
  float metallic, roughness;
} hands_shade_mesh;
typedef struct hands_shade_scene {
  hands_shade_mesh mesh[HANDS_SHADE_MAX_MESHES];
  int32_t n_meshes;
} hands_shade_scene;
long long hands_mesh_workspace_floats(int B, int n_verts);
int hands_mesh_prepare_f32(const float* verts, int ld_verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* csr_off, const int32_t* csr_face, const float* K, const float* T, int B, int S, float* workspace, hands_stream_t stream);
int hands_render_shaded_f32(const hands_shade_scene* scene, const float* image, int B, int S, float* rgb, unsigned char* rgb8, float* depth, int32_t* face_id, hands_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One-time HOST-side packing (csrc/pack.cpp): reference-layout parameters -> the layouts above.
 * Host pointers only, no GPU call, no allocation kept.  A host in any language packs a reference
 * checkpoint with these and uploads the results; hands_amd/packing.py is a thin ctypes wrapper.
 *   hands_pack_conv_dims   sizes of the packed buffers for a (Cout, Cin, KH, KW) convolution whose input
 *                          channels are padded to cin_pad_to (0 = Cin; 4 for the RGB0 stem).
 *   hands_fold_bn_f32      eval-mode BatchNorm2d folded into the preceding conv, in fp64
 *                          (resnet.py:137-149 applies them separately): per_out = Cin*KH*KW.
 *   hands_pack_conv_f64    (Cout,Cin,KH,KW) fp64 -> w_packed [Cout_pad][Kpad] fp32, bias [Cout_pad] (NULL = 0).
 *   hands_pack_linear_f64  nn.Linear (N,K) as a 1x1 conv with optional input-column / output-row
 *                          permutations (the HMR state row, the grasp row, the NCHW nn.Flatten order).
 *   hands_pack_conv1x1_dual_f64  weight of hands_conv1x1_dual_nhwc_f32: [W0 | W1], bias b0 + b1.
 *   hands_pack_mano_f32    MANO constants (hands_mano_consts members + the blend GEMM weight/bias).
 *   hands_pack_conv3x3_winograd_f64  U = G g G^T (fp64, rounded once) of a (Cout, Cin, 3, 3) weight in MFMA operand
 *                          order for hands_conv3x3_winograd_f32; hands_pack_conv3x3_winograd_floats = 16 * Cout * Cin
 *                          (0 if the shape is not supported: Cout % 32, Cin % 16).
 *   hands_pack_conv3x3_winograd4_f64  the F(4x4, 3x3) form: U = G g G^T with the 6x3 G of Lavin & Gray, operand order
 *                          [Cout/32][Cin/8][f = 6 xi + nu][lane 64][4] for hands_conv3x3_winograd4_f32; _floats = 36 * Cout * Cin
 *                          (0 if unsupported: Cout % 32, Cin % 8).
 * hands_conv2d_workspace_floats: floats of split-K workspace hands_conv2d_nhwc_splitk_n_f32 needs for
 *   S slices (S <= 0: the library's own hands_conv2d_splitk_factor); 0 when no split is taken.
 * --------------------------------------------------------------------------------------------- */
typedef struct hands_packed_dims {
  int32_t Cin;       /* channels the kernel sees (padded) = desc.Cin */
  int32_t Cout;      /* channels the kernel stores = round_up(Cout, 4) = desc.Cout */
  int32_t Cout_pad;  /* rows of w_packed / entries of bias = round_up(Cout, 128) */
  int32_t Kpad;      /* row length of w_packed = round_up(KH*KW*Cin, 16) = desc.Kpad */
} hands_packed_dims;

int hands_pack_conv_dims(int Cout, int Cin, int KH, int KW, int cin_pad_to, hands_packed_dims* dims);
int hands_fold_bn_f32(int Cout, long long per_out, const float* w, const float* gamma, const float* beta,
                      const float* mean, const float* var, double eps, double* w_folded, double* bias_folded);
int hands_pack_conv_f64(int Cout, int Cin, int KH, int KW, int cin_pad_to, const double* w_oihw,
                        const double* bias, float* w_packed, float* bias_packed);
int hands_pack_linear_f64(int N, int K, const double* w, const double* bias, const int32_t* col_index,
                          int k_total, const int32_t* row_index, int n_total, float* w_packed,
                          float* bias_packed);
int hands_pack_conv1x1_dual_f64(int Cout, int K0, int K1, const double* w0, const double* b0,
                                const double* w1, const double* b1, float* w_packed, float* bias_packed);
/* blend_w_packed (2432, 160): row m = [shapedirs[m, 0..9] | posedirs[0..134, m] | v_template[m] | 14 zeros], rows 2334.. zero;
 * blend_bias_packed (2432) = v_template.  hands_mano_heads_f32 multiplies column 145 with a constant 1 in its input rows (its
 * accumulators start at zero: no bias load in front of a tile); the three-launch chain (hands_mano_pose_f32 -> GEMM ->
 * hands_mano_skin_f32) writes 0 there and adds blend_bias_packed in the GEMM epilogue. */
int hands_pack_mano_f32(const float* v_template, const float* shapedirs, const float* posedirs,
                        const float* J_regressor, const float* hands_mean, float* pose_mean,
                        float* J_template, float* J_shapedirs, float* blend_w_packed,
                        float* blend_bias_packed);
long long hands_conv2d_workspace_floats(const hands_conv_desc* d, int S);
long long hands_pack_conv3x3_winograd_floats(int Cout, int Cin);
int hands_pack_conv3x3_winograd_f64(int Cout, int Cin, const double* w_oihw, float* u_packed);
long long hands_pack_conv3x3_winograd4_floats(int Cout, int Cin);
int hands_pack_conv3x3_winograd4_f64(int Cout, int Cin, const double* w_oihw, float* u_packed);

#ifdef __cplusplus
}
#endif
#endif /* HANDS_HIP_H */
