// vit_b.hip -- kernels of the ViT-B/16 trunk of hands_light (HandsLight(backbone='vit_b_16')) that are not GEMMs:
// token assembly (class token + position embedding) and the tail  encoder.ln -> drop class token -> AvgPool2d(2)  that turns
// tokens into the 7x7 NHWC map vit_conv reads.  Its self-attention over 197 tokens with 12 heads x 64 is
// attention_kernel<13, 64, 197> of transformer.hip; the tail's LayerNorm is layernorm_row of common.h, as layernorm_kernel's is.
// Reference: src/models/hands_light/model.py:483-493 (vit_forward), src/nets/backbone/utils.py:27-34 (vit_conv); the encoder
// is torchvision's VisionTransformer (nn.MultiheadAttention(768, 12), LayerNorm eps 1e-6).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

// ---- x[b,0,:] = class_token + pos[0];  x[b,1+t,:] = patch[b,t,:] + pos[1+t]   (model.py:484-487 + Encoder.forward) -----------
// One add per element: equal to torch.cat + add bit for bit.
__global__ void vit_tokens_kernel(const float4* __restrict__ patch, const float4* __restrict__ cls, const float4* __restrict__ pos,
                                  float4* __restrict__ x, int B, int T, int C4) {
  const long long total = (long long)B * T * C4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const long long bt = i / C4;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const float4 a = t == 0 ? cls[c] : patch[((long long)b * (T - 1) + (t - 1)) * C4 + c];
    const float4 p = pos[(long long)t * C4 + c];
    x[i] = make_float4(a.x + p.x, a.y + p.y, a.z + p.z, a.w + p.w);
  }
}

// ---- encoder.ln on the patch tokens + AvgPool2d(2): (B, 1 + G*G, 768) tokens -> (B, G/2, G/2, 768) NHWC ----------------------
// One workgroup per output pixel, one wave per token of its 2x2 window: each token is normalised by layernorm_row, as in
// layernorm_kernel (two-pass mean / variance over the row in registers), then the four normalised rows are averaged -- the reference's order
// (model.py:488-491: encoder.ln, x[:, 1:], permute + reshape, then vit_conv's AvgPool2d).  The class token is never read; the
// (B,197,768) -> (B,768,14,14) permute never exists: token-major rows already are NHWC with an image stride of (1+G*G)*768.
__global__ void __launch_bounds__(256) vit_tail_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float* __restrict__ out, int G, float eps) {
  constexpr int C = 768, VPL = 3;
  __shared__ float4 rows[4][C / 4];
  const int Go = G >> 1;
  const int pix = blockIdx.x;                       // b * Go * Go + oy * Go + ox
  const int ox = pix % Go, oy = (pix / Go) % Go, b = pix / (Go * Go);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int tok = 1 + (2 * oy + (w >> 1)) * G + 2 * ox + (w & 1);
  layernorm_row<VPL>(x + ((long long)b * (1 + G * G) + tok) * C, gamma, beta, eps, lane,
                     [&](int i, float4 y) { rows[w][lane + 64 * i] = y; });
  __syncthreads();
  if (threadIdx.x < C / 4) {
    const float4 a = rows[0][threadIdx.x], bq = rows[1][threadIdx.x], c = rows[2][threadIdx.x], d = rows[3][threadIdx.x];
    float4 y;
    y.x = ((a.x + bq.x) + (c.x + d.x)) * 0.25f;
    y.y = ((a.y + bq.y) + (c.y + d.y)) * 0.25f;
    y.z = ((a.z + bq.z) + (c.z + d.z)) * 0.25f;
    y.w = ((a.w + bq.w) + (c.w + d.w)) * 0.25f;
    reinterpret_cast<float4*>(out + (long long)pix * C)[threadIdx.x] = y;
  }
}

}  // namespace

extern "C" {

int hands_vit_tokens_f32(const float* patch, const float* class_token, const float* pos, float* x, int B, int T, int C,
                         hands_stream_t stream) {
  if (!patch || !class_token || !pos || !x || B <= 0 || T < 2 || C <= 0 || C % 4) return HANDS_EINVAL;
  hipLaunchKernelGGL(vit_tokens_kernel, dim3(hands_grid_1d((long long)B * T * C / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const float4*)patch, (const float4*)class_token, (const float4*)pos, (float4*)x, B, T, C / 4);
  HANDS_LAUNCH_CHECK();
}

int hands_vit_tail_f32(const float* x, const float* gamma, const float* beta, float* out, int B, int grid, int C, float eps,
                       hands_stream_t stream) {
  if (!x || !gamma || !beta || !out || B <= 0 || grid < 2 || grid % 2 || C != 768) return HANDS_EINVAL;
  const long long blocks = (long long)B * (grid / 2) * (grid / 2);
  if (blocks > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(vit_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, out, grid, eps);
  HANDS_LAUNCH_CHECK();
}

}  // extern "C"
