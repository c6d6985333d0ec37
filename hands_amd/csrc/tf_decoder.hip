// tf_decoder.hip -- kernels of the hands_light transformer head (tf_decoder=True) that are not GEMMs: single-head attention at
// a head dimension of up to 1024 on the fp32 MFMA pipe, the scalar-token embedding and the token mean.
// Reference: src/nets/hmr_layer.py:17-42, 67-86; src/models/hands_light/transformer.py:533-539, 652-658 (no_norm=True).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

// ---- wide single-head attention ------------------------------------------------------------------------------------------
// out[b] = softmax(scale * Q[b] K[b]^T) V[b] with Tq, Tk <= 128 and a head dimension D that is a multiple of 64 (1024 in the
// head: 109 scalar tokens against themselves or against the 49 feature pixels).  attention_kernel<TW, D, TR> of transformer.hip
// keeps a whole K of T x (D + 4) floats in LDS -- 448 KB at D = 1024 -- so here D STREAMS through LDS in chunks of 64 floats
// while the Tq x Tk scores stay in registers:
//
//   work split   one workgroup of FOUR waves per (batch element, block of 64 queries); wave w owns queries 64 qb + 16 w ..+15
//                against ALL keys, so the softmax never leaves the wave and no workgroup recomputes another's scores.  Two
//                query blocks of one batch element read the same K and V (the second from L2); nothing else is shared.
//   phase 1      S^T[key][query] = sum_d K[key][d] Q[query][d]  (K rows = MFMA A from LDS, Q rows = MFMA B from global memory:
//                a query row is read by one wave only).  v_mfma_f32_16x16x4_f32, NKB independent accumulators per wave (one
//                per 16-key block).  BLOCKED summation: every 64-float chunk accumulates from zero and is added to the running
//                score, so no fp32 chain is longer than 64 products + D / 64 block adds (conv_igemm's HANDS_SUM_BLOCK64).
//   softmax      as in attention_kernel: a lane holds, for ITS query (lane & 15), keys 16 kb + 4 g + r (g = lane >> 4) in
//                register r of block kb; the row maximum and the sum are lane-local plus two exchanges (lane ^ 16, lane ^ 32).
//   phase 2      O^T[d][query] = sum_key V[key][d] P[key][query], one 64-float chunk of V at a time in the SAME LDS buffer,
//                row-major as it lies in memory (the A operand is read as scalars: lanes walk d, the four lane groups sit 16
//                banks apart); the probabilities feed the MFMA from the accumulator registers they were computed in.
//
// PAD rules (transformer.hip, attention_kernel): K and V rows of keys >= Tk are written to LDS as ZEROS, so every word an MFMA
// reads is defined and the score of a padded key is exactly 0; padded keys are left out of the row maximum and of the sum and
// their probabilities are set to exactly 0.  Query rows >= Tq load zeros, run the same instruction stream and are never
// stored; a wave with no real query skips its MFMAs (it still fills LDS and meets the barriers).
// The order of every sum is a function of (Tq, Tk, D) only: a batch element's result does not depend on B.
//
// Occupancy: 4 waves (one per SIMD) and 68 x 16 NKB x 4 bytes of LDS per workgroup (17 408 / 30 464 / 34 816 B at NKB = 4 / 7 / 8:
// four workgroups per CU by LDS).  Registers decide: two score sets (the running sum and the chunk's block sum, 4 NKB each), NKB
// staging float4 and the Q fragment come to 114 / 146 / 194 VGPRs + AGPRs, i.e. 4 / 3 / 2 workgroups per CU, nothing spilled.  At
// bz = 256 a hand's launch is 256 x 2 workgroups = two per CU, all resident at once; docs/EXPERIMENTS.md has the measured rates.
constexpr int WA_DC = 64;            // floats of the head dimension per LDS chunk
constexpr int WA_ROW = WA_DC + 4;    // LDS row (floats): 16-byte aligned, rows 4 banks apart
constexpr int WA_WAVES = 4;
constexpr int WA_NT = 64 * WA_WAVES;

struct WideAttnArgs {
  const float* q; const float* k; const float* v; float* out;
  long long q_bs, k_bs, v_bs, o_bs;    // batch strides (floats)
  int ldq, ldk, ldv, ldo;              // row strides (floats)
  int Tq, Tk, D;
  float scale;
};

// rows [0, 16 NKB) x 64 floats at column c0 of a (T, ld) matrix -> LDS; rows >= T are zeros.  Thread = (row i / 16, 16-byte
// slot i % 16): a wave's 64 lanes cover four whole 256-byte row segments
template <int NKB>
__device__ __forceinline__ void wa_load_chunk(float4 (&r)[NKB], const float* src, int ld, int T, int c0, int tid) {
#pragma unroll
  for (int it = 0; it < NKB; ++it) {
    const int i = tid + it * WA_NT;
    const int t = i >> 4, dq = i & 15;
    r[it] = ld4_or_zero(t < T, src + (long long)(t < T ? t : 0) * ld + c0 + dq * 4);
  }
}

template <int NKB>
__device__ __forceinline__ void wa_store_chunk(const float4 (&r)[NKB], float* lds, int tid) {
#pragma unroll
  for (int it = 0; it < NKB; ++it) {
    const int i = tid + it * WA_NT;
    *reinterpret_cast<float4*>(lds + (i >> 4) * WA_ROW + (i & 15) * 4) = r[it];
  }
}

template <int NKB>
__global__ void __launch_bounds__(WA_NT) wide_attention_kernel(const WideAttnArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[16 * NKB * WA_ROW];      // a K chunk, later a V chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y;
  const int query = blockIdx.x * (16 * WA_WAVES) + wave * 16 + l15;
  const bool qreal = query < a.Tq;
  const bool wave_real = blockIdx.x * (16 * WA_WAVES) + wave * 16 < a.Tq;      // wave-uniform
  const float* qrow = a.q + b * a.q_bs + (long long)(qreal ? query : 0) * a.ldq + 4 * g;
  const float* kb_ = a.k + b * a.k_bs;
  const float* vb_ = a.v + b * a.v_bs;
  const int NC = a.D / WA_DC;

  // ---- phase 1: scores ------------------------------------------------------------------------------------------------
  f32x4 s[NKB];
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb) { s[kb][0] = 0.f; s[kb][1] = 0.f; s[kb][2] = 0.f; s[kb][3] = 0.f; }
  float4 stage[NKB];
  wa_load_chunk<NKB>(stage, kb_, a.ldk, a.Tk, 0, tid);
  for (int c = 0; c < NC; ++c) {
    float4 qf[WA_DC / 16];           // lane (query l15, group g) holds d = 64 c + 16 kk + 4 g + j
#pragma unroll
    for (int kk = 0; kk < WA_DC / 16; ++kk) qf[kk] = ld4_or_zero(qreal, qrow + c * WA_DC + kk * 16);
    __syncthreads();                 // every wave is done with the previous chunk
    wa_store_chunk<NKB>(stage, lds, tid);
    __syncthreads();
    if (c + 1 < NC) wa_load_chunk<NKB>(stage, kb_, a.ldk, a.Tk, (c + 1) * WA_DC, tid);      // in flight under the MFMAs
    if (wave_real) {
      f32x4 p[NKB];
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) { p[kb][0] = 0.f; p[kb][1] = 0.f; p[kb][2] = 0.f; p[kb][3] = 0.f; }
      const float* krow = lds + l15 * WA_ROW + 4 * g;
#pragma unroll
      for (int kk = 0; kk < WA_DC / 16; ++kk) {
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
          const float4 kf = *reinterpret_cast<const float4*>(krow + kb * 16 * WA_ROW + kk * 16);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            p[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4e(kf, j), f4e(qf[kk], j), p[kb], 0, 0, 0);
        }
      }
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) s[kb] += p[kb];       // block sums added in chunk order
    }
  }

  // ---- softmax over the keys of this lane's query; register r of block kb holds key 16 kb + 4 g + r ------------------------
  float m = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[kb][r] *= a.scale;
      m = (16 * kb + 4 * g + r < a.Tk) ? fmaxf(m, s[kb][r]) : m;
    }
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));   // key 0 is real: finite from here on
  float sum = 0.f;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool real = 16 * kb + 4 * g + r < a.Tk;
      const float e = exp_nonpos(real ? s[kb][r] - m : 0.f);
      s[kb][r] = real ? e : 0.f;
      sum += s[kb][r];
    }
  sum += __shfl_xor(sum, 16);
  sum += __shfl_xor(sum, 32);
  const float inv_sum = 1.0f / sum;
#pragma unroll
  for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) s[kb][r] *= inv_sum;

  // ---- phase 2: O^T = V^T . P, 64 output columns per chunk ----------------------------------------------------------------
  float* orow = a.out + b * a.o_bs + (long long)(qreal ? query : 0) * a.ldo + 4 * g;
  wa_load_chunk<NKB>(stage, vb_, a.ldv, a.Tk, 0, tid);
  for (int c = 0; c < NC; ++c) {
    __syncthreads();                 // every wave is done with the previous chunk (the last K chunk when c == 0)
    wa_store_chunk<NKB>(stage, lds, tid);
    __syncthreads();
    if (c + 1 < NC) wa_load_chunk<NKB>(stage, vb_, a.ldv, a.Tk, (c + 1) * WA_DC, tid);
    if (wave_real) {
      f32x4 o[WA_DC / 16];
#pragma unroll
      for (int db = 0; db < WA_DC / 16; ++db) { o[db][0] = 0.f; o[db][1] = 0.f; o[db][2] = 0.f; o[db][3] = 0.f; }
      // MFMA step i of key block kb contracts the keys {16 kb + 4 g + i}: A = V[that key][d = 16 db + l15], B = the probability
      // register i of block kb
      const float* vcol = lds + 4 * g * WA_ROW + l15;
#pragma unroll
      for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
          for (int db = 0; db < WA_DC / 16; ++db)
            o[db] = __builtin_amdgcn_mfma_f32_16x16x4f32(vcol[(kb * 16 + i) * WA_ROW + db * 16], s[kb][i], o[db], 0, 0, 0);
        }
      }
      // O^T[d = 16 db + 4 g + r][query l15]: four consecutive d per store; padded queries store nothing
      if (qreal) {
#pragma unroll
        for (int db = 0; db < WA_DC / 16; ++db)
          *reinterpret_cast<float4*>(orow + c * WA_DC + db * 16) = make_float4(o[db][0], o[db][1], o[db][2], o[db][3]);
      }
    }
  }
}

// ---- tgt[b,t,:] = relu(vec[b,t] * w + bias): nn.Linear(1, C) + ReLU on every scalar of the vector (hmr_layer.py:72-73) ------
// token t is column t of the vector row, or t + gap from token `split` on (the HMR state row keeps two pad floats in front of its
// cam segment)
__global__ void vector_tokens_kernel(const float* __restrict__ vec, int ldvec, int split, int gap, const float4* __restrict__ w,
                                     const float4* __restrict__ bias, float4* __restrict__ out, int B, int T, int C4) {
  const long long total = (long long)B * T * C4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C4);
    const long long bt = i / C4;
    const int t = (int)(bt % T), b = (int)(bt / T);
    const float x = vec[(long long)b * ldvec + t + (t >= split ? gap : 0)];
    const float4 ww = w[c], bb = bias[c];
    out[i] = make_float4(fmaxf(x * ww.x + bb.x, 0.f), fmaxf(x * ww.y + bb.y, 0.f), fmaxf(x * ww.z + bb.z, 0.f),
                         fmaxf(x * ww.w + bb.w, 0.f));
  }
}

// ---- out[b,c] = (sum_t x[b,t,c]) / N (torch.mean(xc, dim=1), hmr_layer.py:78).  The sum is token_sum_kernel's (handocc.hip): one
// workgroup per (sample, 64 channels), 16 token groups that add tokens g, g + 16, .. in order, partial sums added in group
// order -- a fixed order for every batch size
__global__ void __launch_bounds__(256) token_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int N, int C) {
  __shared__ float4 part[16][16];
  const int cblocks = C / 64;
  const int b = blockIdx.x / cblocks, cb = blockIdx.x - b * cblocks;
  const int g = threadIdx.x >> 4, c4 = threadIdx.x & 15;
  const float4* p = reinterpret_cast<const float4*>(x + ((long long)b * N) * C + cb * 64) + c4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int t = g; t < N; t += 16) {
    const float4 v = p[(long long)t * (C / 4)];
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  part[g][c4] = s;
  __syncthreads();
  if (threadIdx.x < 16) {
    float4 r = part[0][threadIdx.x];
    for (int k = 1; k < 16; ++k) {
      const float4 v = part[k][threadIdx.x];
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    const float n = (float)N;
    *reinterpret_cast<float4*>(out + (long long)b * C + cb * 64 + threadIdx.x * 4) = make_float4(r.x / n, r.y / n, r.z / n, r.w / n);
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int hands_wide_attention_f32(const float* q, long long q_batch_stride, int ldq, const float* k, long long k_batch_stride, int ldk,
                             const float* v, long long v_batch_stride, int ldv, float* out, long long out_batch_stride, int ldo,
                             int B, int Tq, int Tk, int D, float scale, hands_stream_t stream) {
  if (!q || !k || !v || !out || B <= 0 || B > 65535 || Tq < 1 || Tq > 128 || Tk < 1 || Tk > 128 || D < 64 || D % 64)
    return HANDS_EINVAL;
  if (ldq < D || ldk < D || ldv < D || ldo < D || ((ldq | ldk | ldv | ldo) & 3)) return HANDS_EINVAL;
  if (q_batch_stride < 0 || k_batch_stride < 0 || v_batch_stride < 0 || out_batch_stride < 0 ||
      ((q_batch_stride | k_batch_stride | v_batch_stride | out_batch_stride) & 3))
    return HANDS_EINVAL;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out)) return HANDS_EINVAL;
  // a batch of more than one element must not write one element's rows over another's
  if (B > 1 && out_batch_stride < (long long)(Tq - 1) * ldo + D) return HANDS_EINVAL;
  const WideAttnArgs a{q, k, v, out, q_batch_stride, k_batch_stride, v_batch_stride, out_batch_stride,
                       ldq, ldk, ldv, ldo, Tq, Tk, D, scale};
  const dim3 grid((Tq + 16 * WA_WAVES - 1) / (16 * WA_WAVES), B), block(WA_NT);
  // key blocks of 16: 4 (the 49 feature pixels), 7 (the 109 tokens) or 8
  if (Tk <= 64)
    hipLaunchKernelGGL(wide_attention_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
  else if (Tk <= 112)
    hipLaunchKernelGGL(wide_attention_kernel<7>, grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(wide_attention_kernel<8>, grid, block, 0, (hipStream_t)stream, a);
  HANDS_LAUNCH_CHECK();
}

int hands_vector_tokens_f32(const float* vec, int ldvec, int split, int gap, const float* w, const float* bias, float* out, int B,
                            int T, int C, hands_stream_t stream) {
  if (!vec || !w || !bias || !out || B <= 0 || T <= 0 || C <= 0 || C % 4 || split < 0 || gap < 0) return HANDS_EINVAL;
  if (ldvec < T + (split < T ? gap : 0)) return HANDS_EINVAL;       // the last token's column lies inside the row
  if (!aligned16(w) || !aligned16(bias) || !aligned16(out)) return HANDS_EINVAL;
  hipLaunchKernelGGL(vector_tokens_kernel, dim3(hands_grid_1d((long long)B * T * (C / 4), 256)), dim3(256), 0,
                     (hipStream_t)stream, vec, ldvec, split, gap, (const float4*)w, (const float4*)bias, (float4*)out, B, T, C / 4);
  HANDS_LAUNCH_CHECK();
}

int hands_token_mean_f32(const float* x, float* out, int B, int N, int C, hands_stream_t stream) {
  if (!x || !out || B <= 0 || N <= 0 || C <= 0 || C % 64 || !aligned16(x) || !aligned16(out)) return HANDS_EINVAL;
  if ((long long)B * (C / 64) > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(token_mean_kernel, dim3((unsigned)(B * (C / 64))), dim3(256), 0, (hipStream_t)stream, x, out, B, N, C);
  HANDS_LAUNCH_CHECK();
}

}  // extern "C"
