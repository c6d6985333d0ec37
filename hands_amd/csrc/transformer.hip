// transformer.hip -- kernels of the hamer_light path (ViT-H/16 backbone + cross-attention decoder head)
// that are not GEMMs: bilinear resize+crop to NHWC4, LayerNorm, position/KPE adds, fp32-MFMA
// multi-head attention (192 tokens, 16 heads x 80), single-query cross-attention.
// Reference: src/models/hamer_light/{model.py:75-151, vit.py:89-151,320-342, pos_emb.py:28-64,
// pose_transformer.py:89-124,160-201}.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

// ---- F.interpolate(bilinear, align_corners=False) + column crop, NCHW3 -> NHWC4 ---------------------
// model.py:82-100: resize (Hin,Win) -> (S,S), then keep columns [col0, col0+Wc).
__global__ void resize_crop_kernel(const float* __restrict__ in, float4* __restrict__ out, int B, int Hin,
                                   int Win, int S, int col0, int Wc) {
  const long long total = (long long)B * S * Wc;
  const double sh = (double)Hin / (double)S, sw = (double)Win / (double)S;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int xo = (int)(i % Wc);
    long long t = i / Wc;
    const int yo = (int)(t % S);
    const int b = (int)(t / S);
    const LerpTap ty = lerp_tap(yo, sh, Hin), tx = lerp_tap(xo + col0, sw, Win);
    const int y0 = ty.i0, y1 = ty.i1, x0 = tx.i0, x1 = tx.i1;
    const float ly = ty.l, lx = tx.l;
    const float hy = 1.f - ly, hx = 1.f - lx;
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = in + ((long long)b * 3 + c) * Hin * Win;
      const float p00 = p[y0 * Win + x0], p01 = p[y0 * Win + x1], p10 = p[y1 * Win + x0], p11 = p[y1 * Win + x1];
      r[c] = hy * (hx * p00 + lx * p01) + ly * (hx * p10 + lx * p11);
    }
    out[i] = make_float4(r[0], r[1], r[2], 0.f);
  }
}

// ---- LayerNorm over the last dim, one wave per row; optional per-group row vector added after --------
template <int VPL>   // float4 per lane: C = 256 * VPL
__global__ void __launch_bounds__(256) layernorm_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ out,
                                                        const float* __restrict__ addvec, int rows_per_vec,
                                                        int M, float eps) {
  constexpr int C = 256 * VPL;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float4* a4 = addvec ? reinterpret_cast<const float4*>(addvec + (long long)(row / rows_per_vec) * C) : nullptr;
  float4* orow = reinterpret_cast<float4*>(out + (long long)row * C);
  layernorm_row<VPL>(x + (long long)row * C, gamma, beta, eps, lane, [&](int i, float4 y) {
    if (a4) { const float4 a = a4[lane + 64 * i]; y.x += a.x; y.y += a.y; y.z += a.z; y.w += a.w; }
    orow[lane + 64 * i] = y;
  });
}

// ---- x[b,t,:] = ((x + pos[1+t]) + pos[0]) + vec[b]   (vit.py:326-330) --------------------------------
__global__ void add_pos_kernel(float4* __restrict__ x, const float4* __restrict__ pos, const float4* __restrict__ vec,
                               int B, int T, int C4) {
  const long long total = (long long)B * T * C4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const long long bt = i / C4;
    const int t = (int)(bt % T), b = (int)(bt / T);
    float4 v = x[i];
    const float4 p1 = pos[(long long)(1 + t) * C4 + c], p0 = pos[c];
    v.x = (v.x + p1.x) + p0.x; v.y = (v.y + p1.y) + p0.y; v.z = (v.z + p1.z) + p0.z; v.w = (v.w + p1.w) + p0.w;
    if (vec) { const float4 k = vec[(long long)b * C4 + c]; v.x += k.x; v.y += k.y; v.z += k.z; v.w += k.w; }
    x[i] = v;
  }
}

// ---- KPE encoding rows [center 4L | corner 16L | 0-pad]  (pos_emb.py:53-67, same layout as model.py:444-460)
__global__ void kpe_encode_kernel(const float* __restrict__ center, const float* __restrict__ corner,
                                  float* __restrict__ out, int B, int ld, int L) {
  const int total = B * ld;
  const int nce = 4 * L, nco = 16 * L;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / ld, e = i - b * ld;
    float v = 0.f;
    if (e < nce + nco) {
      const bool ce = e < nce;
      const int ee = ce ? e : e - nce;
      const int nc = ce ? 2 : 8;
      const float* ang = ce ? center + b * 2 : corner + b * 8;
      const int sc = ee & 1, ci = (ee >> 1) % nc, k = (ee >> 1) / nc;
      const float xx = (float)(1 << k) * ang[ci];
      v = sc ? cosf(xx) : sinf(xx);
    }
    out[i] = v;
  }
}

// ---- multi-head self-attention on fp32 MFMA -----------------------------------------------------------
// One workgroup per (head, crop): TR real tokens in T = 16 * TW token slots, TW waves of 16 queries each, on
// v_mfma_f32_16x16x4_f32.  Two instantiations: <12, 80, 192> (ViT-H/16 of hamer_light, TR == T) and <13, 64, 197> (ViT-B/16 of
// hands_light at 224x224: 196 patches + class token, padded to 208 = 13 blocks of 16).
//   S^T[key][query] = sum_d K[key][d] * (scale * Q[query][d])      (K rows = MFMA A, Q rows = MFMA B)
// A lane holds, for ITS query (lane & 15), four keys of every 16-key block (keys 16 kb + 4 g + i, g = lane >> 4): the
// softmax over keys is lane-local plus two exchanges (lane ^ 16, lane ^ 32).  The probabilities feed the second product
// straight from the accumulator registers:
//   O^T[d][query] = sum_key V^T[d][key] * P[key][query]           (V^T rows = MFMA A, P = MFMA B)
// where MFMA step i of key block kb contracts the keys {16 kb + 4 g + i : g = 0..3} -- exactly the keys the four lane
// groups hold in accumulator register i.
// Fixed summation order per (head, crop): results do not depend on the batch size.
//
// Why 12 waves of 16 queries and not 6 waves of 32 (the form of rounds 1-3, on v_mfma_f32_32x32x2_f32): tools/prof_attn.py
// (per-wave phase stamps + HW_ID) showed that a 6-wave workgroup lands 2-2-1-1 on a CU's four SIMDs -- with two such
// workgroups resident two SIMDs carry four waves and two carry two, the light SIMDs' waves wait at the workgroup barriers for
// the loaded ones (p90 25 us of a 60 us wave life) and the matrix pipe sat at 48 % busy.  Twelve waves are three per SIMD;
// the head dimension 80 is five 16-row blocks exactly (the 32-row form padded it to 96: 17 % of the P.V MFMAs) and the score
// registers halve (48 per lane): 80 VGPRs and 64.5 KB of LDS (V^T takes K's place) = TWO workgroups per CU, six waves per
// SIMD, so one workgroup's fill and barrier phases run under the other's MFMAs; V is requested right after the first barrier
// and waits in registers under Q.K^T.  358 -> 266 us per call at 128 crops (round 4; own LDS regions for K and V^T, one
// workgroup per CU: 284 us).
//
// A token count that is NOT a multiple of 16 (PAD: TR < T; only the last 16-token block has padded tokens).  Every PAD-only
// operation below is behind `!PAD ||` and folds away when TR == T:
//   * Padded K rows (tokens TR..T-1) and padded V^T columns are written as ZEROS, so every LDS word an MFMA reads is defined:
//     the scores of padded keys are exactly 0 (finite), and their probabilities are set to exactly 0 before the second
//     product, so 0 * 0 is all they ever contribute.
//   * Padded keys do not reach the softmax: they are left out of the row maximum and of the sum.
//   * Padded query rows (the last wave's queries TR..T-1) load zeros instead of reading past the tensor, run through the same
//     instruction stream (uniform softmax over finite scores, no NaN), and are never stored: nothing beyond row TR-1 of a
//     crop's output is written.
// Partition for 197 tokens: ONE WAVE PER 16-QUERY BLOCK, 13 waves = 832 threads per (head, crop).  Thirteen blocks do not
// divide over four SIMDs whatever is done with them.  The alternatives were (a) twelve waves that share the 13th block -- its
// 5 real queries would need a cross-wave softmax (keys split over waves: an LDS round trip and two more barriers for 2.5 % of
// the queries) -- or (b) seven waves of two blocks (the 6-wave imbalance measured above, plus a half-empty 14th block = 7 %
// wasted MFMAs against 5.6 % here).  With 13 waves a workgroup sits 4-3-3-3 on the SIMDs.  55.3 KB of LDS (208 x 68 floats of
// K, then 64 x 212 of V^T in its place) would let two workgroups share a CU, but the registers do not: 52 score registers +
// 16 of Q + 16 of parked V + the K fragment are 119 VGPRs, four waves per SIMD, so ONE workgroup is resident per CU and its
// fill and barrier phases are not hidden under another's MFMAs as they are for ViT-H (two resident workgroups would need 7
// waves on a SIMD = 72 VGPRs: the compiler reaches that only by spilling 164 bytes per lane).  That, and the tail block
// (11/16 of one wave's MFMAs = 5.3 % of the launch), is why <13, 64, 197>'s rate per algorithmic FLOP is below
// <12, 80, 192>'s; docs/EXPERIMENTS.md has both, measured in one run.
template <int TW, int D>
constexpr int attention_lds_bytes() {
  return 4 * (16 * TW * (D + 4) > D * (16 * TW + 4) ? 16 * TW * (D + 4) : D * (16 * TW + 4));     // K, then V^T in its place
}

// The register allocator's target, waves per SIMD: a workgroup's waves on its fullest SIMD, times the workgroups per CU the
// reasoning above arrives at -- two when the waves divide evenly over the four SIMDs (3 x 2 = 6: 80 registers), one
// otherwise (13 waves: 4, up to 128 registers).
template <int TW>
constexpr int attention_waves_per_simd() {
  return TW % 4 == 0 ? 2 * (TW / 4) : (TW + 3) / 4;
}

template <int TW, int D, int TR>
__global__ void __launch_bounds__(64 * TW)
__attribute__((amdgpu_waves_per_eu(attention_waves_per_simd<TW>(), attention_waves_per_simd<TW>())))
attention_kernel(const float* __restrict__ qkv, float* __restrict__ out, int heads, float scale) {
  constexpr int T = 16 * TW;         // token slots
  constexpr bool PAD = TR != T;
  constexpr int KR = D + 4;          // K row (floats): (D + 4) * 4 B = an odd number of 16-byte slots for D = 80
  constexpr int VR = T + 4;          // V^T row
  constexpr int NT = 64 * TW;
  constexpr int NKK = D / 16;        // 16-float steps of the head dimension: one float4 per lane group and step
  constexpr int DB = D / 16;         // 16-row blocks of V^T / O^T
  constexpr int FILL = T * (D / 4) / NT;
  static_assert(D % 16 == 0 && T * (D / 4) % NT == 0 && NT % T == 0, "fill loops assume whole iterations");
  static_assert(TR <= T && TR > T - 16, "TR real tokens fill all but the last 16-token block");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* sK = lds;                   // [T][KR]
  float* sV = lds;                   // [D][VR]  (V transposed) in K's place, once every wave is done with K

  const int h = blockIdx.x, b = blockIdx.y;
  const int C = heads * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const float* base = qkv + (long long)b * TR * 3 * C + h * D;

  // K tile -> LDS (rows TR..T-1 zero): consecutive lanes walk the 16-byte slots of a token's row (coalesced 320-byte rows
  // for D = 80); all loads of a thread in flight before its first LDS store
  {
    float4 kv[FILL];
#pragma unroll
    for (int it = 0; it < FILL; ++it) {
      const int i = tid + it * NT;
      const int t = i / (D / 4), dq = i - t * (D / 4);
      kv[it] = ld4_or_zero(!PAD || t < TR, base + (long long)t * 3 * C + C + dq * 4);
    }
#pragma unroll
    for (int it = 0; it < FILL; ++it) {
      const int i = tid + it * NT;
      const int t = i / (D / 4), dq = i - t * (D / 4);
      *reinterpret_cast<float4*>(sK + t * KR + dq * 4) = kv[it];
    }
  }
  // this wave's Q fragments, pre-scaled (vit.py:118 scales q before the matmul): lane (query l15, group g) holds
  // d = 16 kk + 4 g + j
  const int query = wave * 16 + l15;
  const bool qreal = !PAD || query < TR;
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
  // V: requested now (after the barrier, whose s_waitcnt would otherwise wait for it), parked in registers under Q.K^T and
  // transposed into LDS afterwards.  thread = (token ft, 16-byte slot fq + it * NT / T): lanes walk tokens,
  // so the transposed scalar LDS writes are conflict-free
  const int ft = tid % T, fq = tid / T;
  float4 vv[FILL];
#pragma unroll
  for (int it = 0; it < FILL; ++it)
    vv[it] = ld4_or_zero(!PAD || ft < TR, base + (long long)ft * 3 * C + 2 * C + (fq + it * (NT / T)) * 4);

  // S^T = K . (scale Q)^T: TW independent accumulation chains (one per key block), the k-step outermost
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
  // V^T -> LDS in K's place (lanes walk tokens: the transposed scalar writes are conflict-free; columns TR..T-1 zero,
  // columns T..VR-1 are never read)
#pragma unroll
  for (int it = 0; it < FILL; ++it) {
    float* d = sV + (fq + it * (NT / T)) * 4 * VR + ft;
    d[0 * VR] = vv[it].x;
    d[1 * VR] = vv[it].y;
    d[2 * VR] = vv[it].z;
    d[3 * VR] = vv[it].w;
  }
  // softmax over the keys of this lane's query: exp(x - max) * (1 / sum): one reciprocal per query; e * (1 / sum) vs
  // e / sum differ by the last rounding only.  Register r of key block kb holds key 16 kb + 4 g + r: only registers
  // r >= nreal of the last block hold padded keys
  constexpr int LB = TW - 1;
  const int nreal = TR - 16 * LB - 4 * g;
  float m = s[0][0];                 // key 0 (g = 0) .. key 12 (g = 3): always real
#pragma unroll
  for (int kb = 0; kb < TW; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = (!PAD || kb < LB || r < nreal) ? fmaxf(m, s[kb][r]) : m;
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < TW; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool real = !PAD || kb < LB || r < nreal;
      const float e = exp_nonpos(real ? s[kb][r] - m : 0.f);
      s[kb][r] = real ? e : 0.f;
      sum += s[kb][r];
    }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const float inv_sum = 1.0f / sum;
#pragma unroll
  for (int kb = 0; kb < TW; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[kb][r] *= inv_sum;
  __syncthreads();   // V^T complete

  // O^T = V^T . P: DB independent chains (one per 16-row block of V^T), the key block outermost
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
  // O^T[d = 16 db + 4 g + i][query l15] -> out[(b*TR + query)*C + h*D + d], 4 consecutive d per store; padded queries
  // store nothing
  if (qreal) {
    float* orow = out + ((long long)b * TR + query) * C + h * D + 4 * g;
#pragma unroll
    for (int db = 0; db < DB; ++db)
      *reinterpret_cast<float4*>(orow + db * 16) = make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
  }
}

// ---- single-query cross-attention (decoder head): one wave per (batch, head), head dim 64 ------------
// dots[t] = (q . k[t]) * scale; softmax over t; out = sum_t attn[t] v[t]   (pose_transformer.py:113-123)
__global__ void __launch_bounds__(64) cross_attention_1q_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                float* __restrict__ out, int T, int heads, float scale) {
  constexpr int D = 64;
  __shared__ float sq[D];
  __shared__ float sattn[1024];
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int inner = heads * D;
  sq[lane] = q[(long long)b * inner + h * D + lane];
  __syncthreads();
  const float* kbase = kv + (long long)b * T * 2 * inner + h * D;
  float mx = -INFINITY;
  for (int t = lane; t < T; t += 64) {
    const float4* kr = reinterpret_cast<const float4*>(kbase + (long long)t * 2 * inner);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < D / 4; ++i) {
      const float4 kk = kr[i];
      acc += sq[4 * i] * kk.x; acc += sq[4 * i + 1] * kk.y; acc += sq[4 * i + 2] * kk.z; acc += sq[4 * i + 3] * kk.w;
    }
    acc *= scale;
    sattn[t] = acc;
    mx = fmaxf(mx, acc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
  for (int t = lane; t < T; t += 64) { const float e = expf(sattn[t] - mx); sattn[t] = e; sum += e; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  __syncthreads();
  const float* vbase = kbase + inner + lane;
  float acc = 0.f;
  for (int t = 0; t < T; ++t) acc += (sattn[t] / sum) * vbase[(long long)t * 2 * inner];
  out[(long long)b * inner + h * D + lane] = acc;
}

// ---- rot6d_to_rotmat, COLUMNS convention (geometry.py:47-62) ------------------------------------------
__global__ void rot6d_cols_kernel(const float* __restrict__ pose6d, int ld6, float* __restrict__ rotmat, int B) {
  const int total = B * 16;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i >> 4, j = i & 15;
    const float* s = pose6d + (long long)b * ld6 + j * 6;
    const float a1x = s[0], a1y = s[1], a1z = s[2], a2x = s[3], a2y = s[4], a2z = s[5];
    const float n1 = fmaxf(sqrtf(a1x * a1x + a1y * a1y + a1z * a1z), 1e-12f);
    const float b1x = a1x / n1, b1y = a1y / n1, b1z = a1z / n1;
    const float d = b1x * a2x + b1y * a2y + b1z * a2z;
    float b2x = a2x - d * b1x, b2y = a2y - d * b1y, b2z = a2z - d * b1z;
    const float n2 = fmaxf(sqrtf(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12f);
    b2x /= n2; b2y /= n2; b2z /= n2;
    const float b3x = b1y * b2z - b1z * b2y, b3y = b1z * b2x - b1x * b2z, b3z = b1x * b2y - b1y * b2x;
    float* o = rotmat + (long long)i * 9;
    o[0] = b1x; o[1] = b2x; o[2] = b3x;
    o[3] = b1y; o[4] = b2y; o[5] = b3y;
    o[6] = b1z; o[7] = b2z; o[8] = b3z;
  }
}

// hands_attention_f32's launch of one instantiation.  More than the 64 KB default cap of dynamic LDS (<12, 80, 192>: 64.5 KB)
// needs the kernel's limit raised, once per device; an instantiation under the cap (<13, 64, 197>: 56 576 B) makes no runtime
// call before its launch -- it runs inside stream capture.
template <int TW, int D, int TR>
int launch_attention(const float* qkv, float* out, int B, int heads, float scale, hipStream_t stream) {
  constexpr int LDS = attention_lds_bytes<TW, D>();
  if constexpr (LDS > 64 * 1024) {
    static std::atomic<int> lds_set[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return HANDS_EINVAL;
    if (!lds_set[dev].load(std::memory_order_acquire)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attention_kernel<TW, D, TR>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
      if (e != hipSuccess) return (int)e;
      lds_set[dev].store(1, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL((attention_kernel<TW, D, TR>), dim3(heads, B), dim3(64 * TW), LDS, stream, qkv, out, heads, scale);
  HANDS_LAUNCH_CHECK();
}

}  // namespace

extern "C" {

int hands_resize_crop_nchw3_to_nhwc4_f32(const float* in, float* out, int B, int Hin, int Win, int S, int col0,
                                         int Wc, hands_stream_t stream) {
  if (!in || !out || B <= 0 || Hin <= 0 || Win <= 0 || S <= 0 || col0 < 0 || Wc <= 0 || col0 + Wc > S) return HANDS_EINVAL;
  hipLaunchKernelGGL(resize_crop_kernel, dim3(hands_grid_1d((long long)B * S * Wc, 256)), dim3(256), 0,
                     (hipStream_t)stream, in, (float4*)out, B, Hin, Win, S, col0, Wc);
  HANDS_LAUNCH_CHECK();
}

int hands_layernorm_f32(const float* x, const float* gamma, const float* beta, float* out, const float* addvec,
                        int rows_per_vec, int M, int C, float eps, hands_stream_t stream) {
  if (!x || !gamma || !beta || !out || M <= 0 || (addvec && rows_per_vec <= 0)) return HANDS_EINVAL;
  const dim3 grid((M + 3) / 4), block(256);
  if (C == 1280)
    hipLaunchKernelGGL(layernorm_kernel<5>, grid, block, 0, (hipStream_t)stream, x, gamma, beta, out, addvec,
                       rows_per_vec, M, eps);
  else if (C == 1024)
    hipLaunchKernelGGL(layernorm_kernel<4>, grid, block, 0, (hipStream_t)stream, x, gamma, beta, out, addvec,
                       rows_per_vec, M, eps);
  else if (C == 768)     // ViT-B/16 (hands_light, backbone='vit_b_16')
    hipLaunchKernelGGL(layernorm_kernel<3>, grid, block, 0, (hipStream_t)stream, x, gamma, beta, out, addvec,
                       rows_per_vec, M, eps);
  else if (C == 256)
    hipLaunchKernelGGL(layernorm_kernel<1>, grid, block, 0, (hipStream_t)stream, x, gamma, beta, out, addvec,
                       rows_per_vec, M, eps);
  else
    return HANDS_EINVAL;
  HANDS_LAUNCH_CHECK();
}

int hands_add_pos_f32(float* x, const float* pos, const float* vec, int B, int T, int C, hands_stream_t stream) {
  if (!x || !pos || B <= 0 || T <= 0 || C % 4) return HANDS_EINVAL;
  hipLaunchKernelGGL(add_pos_kernel, dim3(hands_grid_1d((long long)B * T * C / 4, 256)), dim3(256), 0,
                     (hipStream_t)stream, (float4*)x, (const float4*)pos, (const float4*)vec, B, T, C / 4);
  HANDS_LAUNCH_CHECK();
}

int hands_kpe_encode_f32(const float* center_angle, const float* corner_angle, float* out, int B, int ld,
                         int n_freq, hands_stream_t stream) {
  if (!center_angle || !corner_angle || !out || B <= 0 || n_freq < 1 || n_freq > 16 || ld < 20 * n_freq)
    return HANDS_EINVAL;
  hipLaunchKernelGGL(kpe_encode_kernel, dim3(hands_grid_1d((long long)B * ld, 256)), dim3(256), 0,
                     (hipStream_t)stream, center_angle, corner_angle, out, B, ld, n_freq);
  HANDS_LAUNCH_CHECK();
}

int hands_attention_f32(const float* qkv, float* out, int B, int T, int heads, int head_dim, float scale,
                        hands_stream_t stream) {
  if (!qkv || !out || B <= 0 || heads <= 0) return HANDS_EINVAL;
  if (T == 192 && head_dim == 80)      // ViT-H/16 at 256x192
    return launch_attention<12, 80, 192>(qkv, out, B, heads, scale, (hipStream_t)stream);
  if (T == 197 && head_dim == 64)      // ViT-B/16 at 224x224 (196 patches + class token)
    return launch_attention<13, 64, 197>(qkv, out, B, heads, scale, (hipStream_t)stream);
  return HANDS_EINVAL;
}

int hands_cross_attention_1q_f32(const float* q, const float* kv, float* out, int B, int T, int heads,
                                 int head_dim, float scale, hands_stream_t stream) {
  if (!q || !kv || !out || B <= 0 || T <= 0 || T > 1024 || head_dim != 64 || heads <= 0) return HANDS_EINVAL;
  hipLaunchKernelGGL(cross_attention_1q_kernel, dim3(heads, B), dim3(64), 0, (hipStream_t)stream, q, kv, out, T,
                     heads, scale);
  HANDS_LAUNCH_CHECK();
}

int hands_rot6d_to_matrix_cols_f32(const float* pose6d, int ld6, float* rotmat, int B, hands_stream_t stream) {
  if (!pose6d || !rotmat || B <= 0) return HANDS_EINVAL;
  hipLaunchKernelGGL(rot6d_cols_kernel, dim3(hands_grid_1d((long long)B * 16, 256)), dim3(256), 0,
                     (hipStream_t)stream, pose6d, ld6, rotmat, B);
  HANDS_LAUNCH_CHECK();
}

}  // extern "C"
