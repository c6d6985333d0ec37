// vit_b.hip -- kernels of the ViT-B/16 trunk of hands_light (HandsLight(backbone='vit_b_16')) that are not GEMMs:
// token assembly (class token + position embedding), fp32-MFMA self-attention over 197 tokens with 12 heads x 64, and the
// tail  encoder.ln -> drop class token -> AvgPool2d(2)  that turns tokens into the 7x7 NHWC map vit_conv reads.
// Reference: src/models/hands_light/model.py:483-493 (vit_forward), src/nets/backbone/utils.py:27-34 (vit_conv); the encoder
// is torchvision's VisionTransformer (nn.MultiheadAttention(768, 12), LayerNorm eps 1e-6).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// exp(x) for finite x <= 0 (the form of transformer.hip: exp2 of a compensated x * log2(e))
__device__ __forceinline__ float exp_nonpos(float x) {
  const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-08f;
  const float n = rintf(x * L2E_HI);
  float f = fmaf(x, L2E_HI, -n);
  f = fmaf(x, L2E_LO, f);
  return ldexpf(__builtin_amdgcn_exp2f(f), (int)n);
}

__device__ __forceinline__ float f4e(const float4& v, int t) {
  return t == 0 ? v.x : (t == 1 ? v.y : (t == 2 ? v.z : v.w));
}

// 16 bytes at p when `real`, zeros otherwise (padded tokens: nothing is read past the tensor)
__device__ __forceinline__ float4 ld4_or_zero(bool real, const float* p) {
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (real) r = *reinterpret_cast<const float4*>(p);
  return r;
}

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

// ---- multi-head self-attention on fp32 MFMA for a token count that is NOT a multiple of 16 ---------------------------------
// The sibling of attention_kernel<12,80> (transformer.hip; same operand roles, same softmax, same register-fed second product --
// read its header first) for TR real tokens padded to T = 16 * TW: ViT-B/16 at 224x224 has TR = 197 (196 patches + class
// token), D = 64, so T = 208 = 13 blocks of 16.
//   * Padded K rows (tokens TR..T-1) and padded V^T columns are written as ZEROS, so every LDS word an MFMA reads is defined:
//     the scores of padded keys are exactly 0 (finite), and their probabilities are set to exactly 0 before the second
//     product, so 0 * 0 is all they ever contribute.
//   * Padded keys do not reach the softmax: they are left out of the row maximum and of the sum.
//   * Padded query rows (the last wave's queries TR..T-1) load zeros instead of reading past the tensor, run through the same
//     instruction stream (uniform softmax over finite scores, no NaN), and are never stored: nothing beyond row TR-1 of a
//     crop's output is written.
// Partition: ONE WAVE PER 16-QUERY BLOCK, 13 waves = 832 threads per (head, crop).  attention_kernel<12,80> chose twelve waves
// because they are three per SIMD; thirteen blocks do not divide over four SIMDs whatever is done with them.  The alternatives
// were (a) twelve waves that share the 13th block -- its 5 real queries would need a cross-wave softmax (keys split over
// waves: an LDS round trip and two more barriers for 2.5 % of the queries) -- or (b) seven waves of two blocks (the 6-wave
// imbalance the ViT-H header measured, plus a half-empty 14th block = 7 % wasted MFMAs against 5.6 % here).  With 13 waves a
// workgroup sits 4-3-3-3 on the SIMDs.  55.3 KB of LDS (208 x 68 floats of K, then 64 x 212 of V^T in its place) would let
// two workgroups share a CU, but the registers do not: 52 score registers + 16 of Q + 16 of parked V + the K fragment are
// 116 VGPRs, four waves per SIMD, so ONE workgroup is resident per CU and its fill and barrier phases are not hidden under
// another's MFMAs as they are for ViT-H (two resident workgroups would need 7 waves on a SIMD = 72 VGPRs: the compiler
// reaches that only by spilling 164 bytes per lane).  That, and the tail block (11/16 of one wave's MFMAs = 5.3 % of the
// launch), is why this kernel's rate per algorithmic FLOP is below attention_kernel<12,80>'s; docs/EXPERIMENTS.md has both,
// measured in one run.
// Fixed summation order per (head, crop): results do not depend on the batch size.
template <int TW, int D, int TR>
__global__ void __launch_bounds__(64 * TW) attention_pad_kernel(const float* __restrict__ qkv, float* __restrict__ out, int heads,
                                                                float scale) {
  constexpr int T = 16 * TW;         // padded token count
  constexpr int KR = D + 4;          // K row (floats)
  constexpr int VR = T + 4;          // V^T row
  constexpr int NT = 64 * TW;
  constexpr int NKK = D / 16;
  constexpr int DB = D / 16;
  constexpr int FILL = T * (D / 4) / NT;
  static_assert(D % 16 == 0 && T * (D / 4) % NT == 0 && NT % T == 0, "fill loops assume whole iterations");
  static_assert(TR <= T && TR > T - 16, "TR real tokens fill all but the last 16-token block");
  __shared__ __attribute__((aligned(16))) float lds[(T * KR > D * VR ? T * KR : D * VR)];
  float* sK = lds;                   // [T][KR]
  float* sV = lds;                   // [D][VR]  (V transposed) in K's place, once every wave is done with K

  const int h = blockIdx.x, b = blockIdx.y;
  const int C = heads * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const float* base = qkv + (long long)b * TR * 3 * C + h * D;

  // K tile -> LDS (rows TR..T-1 zero)
  {
    float4 kv[FILL];
#pragma unroll
    for (int it = 0; it < FILL; ++it) {
      const int i = tid + it * NT;
      const int t = i / (D / 4), dq = i - t * (D / 4);
      kv[it] = ld4_or_zero(t < TR, base + (long long)t * 3 * C + C + dq * 4);
    }
#pragma unroll
    for (int it = 0; it < FILL; ++it) {
      const int i = tid + it * NT;
      const int t = i / (D / 4), dq = i - t * (D / 4);
      *reinterpret_cast<float4*>(sK + t * KR + dq * 4) = kv[it];
    }
  }
  // this wave's Q fragments, pre-scaled: lane (query l15, group g) holds d = 16 kk + 4 g + j
  const int query = wave * 16 + l15;
  const bool qreal = query < TR;
  float4 qf[NKK];
  {
    const float* qrow = base + (long long)(qreal ? query : 0) * 3 * C + 4 * g;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      float4 v = ld4_or_zero(qreal, qrow + kk * 16);
      v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
      qf[kk] = v;
    }
  }
  __syncthreads();
  // V: requested now, parked in registers under Q.K^T.  thread = (token ft, 16-byte slot fq + it * NT / T)
  const int ft = tid % T, fq = tid / T;
  float4 vv[FILL];
#pragma unroll
  for (int it = 0; it < FILL; ++it)
    vv[it] = ld4_or_zero(ft < TR, base + (long long)ft * 3 * C + 2 * C + (fq + it * (NT / T)) * 4);

  // S^T = K . (scale Q)^T
  f32x4 s[TW];
#pragma unroll
  for (int kb = 0; kb < TW; ++kb) { s[kb][0] = 0.f; s[kb][1] = 0.f; s[kb][2] = 0.f; s[kb][3] = 0.f; }
  {
    const float* krow = sK + l15 * KR + 4 * g;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
#pragma unroll
      for (int kb = 0; kb < TW; ++kb) {
        const float4 kf = *reinterpret_cast<const float4*>(krow + kb * 16 * KR + kk * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          s[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(kf, j), f4e(qf[kk], j), s[kb], 0, 0, 0);
      }
    }
  }
  __syncthreads();   // every wave is done with K
  // V^T -> LDS in K's place (columns TR..T-1 zero; columns T..VR-1 are never read)
#pragma unroll
  for (int it = 0; it < FILL; ++it) {
    float* d = sV + (fq + it * (NT / T)) * 4 * VR + ft;
    d[0 * VR] = vv[it].x;
    d[1 * VR] = vv[it].y;
    d[2 * VR] = vv[it].z;
    d[3 * VR] = vv[it].w;
  }
  // softmax over the REAL keys of this lane's query.  Register r of key block kb holds key 16 kb + 4 g + r: only the last
  // block has padded keys
  constexpr int LB = TW - 1;
  const int nreal = TR - 16 * LB - 4 * g;      // registers r < nreal of the last block hold real keys
  float m = s[0][0];                 // key 0 (g = 0) .. key 12 (g = 3): always real
#pragma unroll
  for (int kb = 0; kb < LB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, s[kb][r]);
#pragma unroll
  for (int r = 0; r < 4; ++r) m = r < nreal ? fmaxf(m, s[LB][r]) : m;
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < LB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s[kb][r] = exp_nonpos(s[kb][r] - m); sum += s[kb][r]; }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float e = exp_nonpos(r < nreal ? s[LB][r] - m : 0.f);
    s[LB][r] = r < nreal ? e : 0.f;
    sum += s[LB][r];
  }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const float inv_sum = 1.0f / sum;
#pragma unroll
  for (int kb = 0; kb < TW; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[kb][r] *= inv_sum;
  __syncthreads();   // V^T complete

  // O^T = V^T . P
  f32x4 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) { o[db][0] = 0.f; o[db][1] = 0.f; o[db][2] = 0.f; o[db][3] = 0.f; }
  {
    const float* vrow = sV + l15 * VR + 4 * g;
#pragma unroll
    for (int kb = 0; kb < TW; ++kb) {
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const float4 vf = *reinterpret_cast<const float4*>(vrow + db * 16 * VR + kb * 16);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(vf, i), s[kb][i], o[db], 0, 0, 0);
      }
    }
  }
  // O^T[d = 16 db + 4 g + i][query l15] -> out[(b*TR + query)*C + h*D + d]; padded queries store nothing
  if (qreal) {
    float* orow = out + ((long long)b * TR + query) * C + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < DB; ++db)
      *reinterpret_cast<float4*>(orow + db * 16) = make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
  }
}

// ---- encoder.ln on the patch tokens + AvgPool2d(2): (B, 1 + G*G, 768) tokens -> (B, G/2, G/2, 768) NHWC ----------------------
// One workgroup per output pixel, one wave per token of its 2x2 window: each token is normalised as layernorm_kernel does
// (two-pass mean / variance over the row in registers), then the four normalised rows are averaged -- the reference's order
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
  const float4* xr = reinterpret_cast<const float4*>(x + ((long long)b * (1 + G * G) + tok) * C);
  float4 v[VPL];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    v[i] = xr[lane + 64 * i];
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const float a = v[i].x - mean, bb = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
    q += (a * a + bb * bb) + (c * c + d * d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.0f / sqrtf(q / (float)C + eps);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const float4 gg = g4[lane + 64 * i], bb = b4[lane + 64 * i];
    float4 y;
    y.x = (v[i].x - mean) * rstd * gg.x + bb.x;
    y.y = (v[i].y - mean) * rstd * gg.y + bb.y;
    y.z = (v[i].z - mean) * rstd * gg.z + bb.z;
    y.w = (v[i].w - mean) * rstd * gg.w + bb.w;
    rows[w][lane + 64 * i] = y;
  }
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

// hands_attention_f32's launch for (T, head_dim) = (197, 64): see transformer.hip
int hands_detail_attention_t197_d64(const float* qkv, float* out, int B, int heads, float scale, hipStream_t stream) {
  hipLaunchKernelGGL((attention_pad_kernel<13, 64, 197>), dim3(heads, B), dim3(64 * 13), 0, stream, qkv, out, heads, scale);
  return (int)hipGetLastError();
}

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
