// common.h -- shared helpers for the gfx950 kernels of libhands_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define HANDS_LAUNCH_CHECK() return (int)hipGetLastError()

static inline int hands_grid_1d(long long work, int block, int cap = 256 * 8) {
  long long g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// ---- device side ---------------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));      // MFMA 16x16 accumulator
typedef float f32x16 __attribute__((ext_vector_type(16)));    // MFMA 32x32 accumulator

__device__ __forceinline__ float f4e(const float4& v, int t) {
  return t == 0 ? v.x : (t == 1 ? v.y : (t == 2 ? v.z : v.w));
}

// NaN handling of ReLU and max-pool, one copy for every kernel (torch.relu and nn.MaxPool2d hand a NaN on; fmaxf is IEEE maxNum
// and drops a NaN operand: fmaxf(NaN, 0) = 0, and a window of NaN alone keeps the -inf its maximum starts from).
// relu_f32: the bits of fmaxf(v, 0.f) for every v that is not NaN (-0 -> +0), NaN for NaN.
__device__ __forceinline__ float relu_f32(float v) { return v <= 0.f ? 0.f : v; }
__device__ __forceinline__ float4 relu_f32(const float4& v) {
  return make_float4(relu_f32(v.x), relu_f32(v.y), relu_f32(v.z), relu_f32(v.w));
}
// One tap of a 4-channel max-pool and its end: the maximum is fmaxf's (finite and infinite windows keep its bits), a flag per
// channel remembers a NaN tap (one compare per value, the OR on the scalar unit) and replaces the maximum at the end.  Shared by
// maxpool3x3s2_kernel and the two fused stems, which promise the same bits.
struct PoolNan4 { bool x = false, y = false, z = false, w = false; };
__device__ __forceinline__ void pool_tap(float4& m, PoolNan4& seen, const float4& v) {
  m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
  seen.x |= v.x != v.x; seen.y |= v.y != v.y; seen.z |= v.z != v.z; seen.w |= v.w != v.w;
}
__device__ __forceinline__ float4 pool_finish(const float4& m, const PoolNan4& seen) {
  const float q = __builtin_nanf("");
  return make_float4(seen.x ? q : m.x, seen.y ? q : m.y, seen.z ? q : m.z, seen.w ? q : m.w);
}

// exp(x) for finite x <= 0: exp2 of a compensated x * log2(e) (v_exp_f32 on [-0.5, 0.5] + v_ldexp_f32, ~1 ulp; the
// library's expf carries range checks that cannot trigger here)
__device__ __forceinline__ float exp_nonpos(float x) {
  const float L2E_HI = 1.44269502162933349609375f, L2E_LO = 1.925963033500011e-08f;
  const float n = rintf(x * L2E_HI);
  float f = fmaf(x, L2E_HI, -n);                           // x * log2(e) - n with one rounding
  f = fmaf(x, L2E_LO, f);
  return ldexpf(__builtin_amdgcn_exp2f(f), (int)n);
}

// Source tap of bilinear interpolation, align_corners=False (ATen's area_pixel_compute_source_index): destination index dst of a
// resize n_in -> n_out reads src = max(0, (dst + 0.5) * n_in / n_out - 0.5) -> i0 = floor(src), i1 = min(i0 + 1, n_in - 1), weight
// `l` of i1.  The coordinate is formed in fp64 and rounded once, as the weight: in fp32 a ratio that is not a dyadic fraction
// (200 -> 96: 2.08333...) loses |src| * 2^-24 of the weight, 4e-5 of a randn image's pixel at column 160 -- tests/
// test_gpu_kernel_edges.py holds every ratio to 2e-6.  Where ratio and coordinate are exact in fp32 (the models' 2x and
// 224 -> 256) both forms give the same bits.
struct LerpTap { int i0, i1; float l; };
__device__ __forceinline__ LerpTap lerp_tap(int dst, double scale, int n_in) {
  double s = ((double)dst + 0.5) * scale - 0.5;
  s = s < 0.0 ? 0.0 : s;
  LerpTap t;
  t.i0 = (int)s;
  t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
  t.l = (float)(s - (double)t.i0);
  return t;
}

// 16 bytes at p when `real`, zeros otherwise (padded tokens: nothing is read past the tensor)
__device__ __forceinline__ float4 ld4_or_zero(bool real, const float* p) {
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (real) r = *reinterpret_cast<const float4*>(p);
  return r;
}

// LayerNorm of one row of C = 256 * VPL floats by one wave: lane holds the float4 slots lane + 64 i.  Two passes over the
// row in registers (mean, then the variance of the centred values), each closed by a __shfl_xor tree, then the affine
// y = (x - mean) * rstd * gamma + beta, handed slot by slot to emit(i, y) -- the caller's store.
template <int VPL, class Emit>
__device__ __forceinline__ void layernorm_row(const float* x_row, const float* gamma, const float* beta, float eps, int lane,
                                              Emit emit) {
  constexpr int C = 256 * VPL;
  const float4* xr = reinterpret_cast<const float4*>(x_row);
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
    const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
    q += (a * a + b * b) + (c * c + d * d);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = 1.0f / sqrtf(q / (float)C + eps);
  const float4* g4 = reinterpret_cast<const float4*>(gamma);
  const float4* b4 = reinterpret_cast<const float4*>(beta);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const float4 g = g4[lane + 64 * i], bb = b4[lane + 64 * i];
    float4 y;
    y.x = (v[i].x - mean) * rstd * g.x + bb.x;
    y.y = (v[i].y - mean) * rstd * g.y + bb.y;
    y.z = (v[i].z - mean) * rstd * g.z + bb.z;
    y.w = (v[i].w - mean) * rstd * g.w + bb.w;
    emit(i, y);
  }
}
