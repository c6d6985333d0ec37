// accel.hip -- temporal metrics on device (hands_accel_error_f32, hands_eval_accel_metrics_f32 of include/hands_hip.h): the
// acceleration error of compute_error_accel / eval_acc_pose (src/utils/eval_modules.py:508-622) over T consecutive frames,
//   a[t] = (x[t-1] - 2 x[t] + x[t+1]) fps^2,   err[t] = mean_n |a_pred[t,n] - a_gt[t,n]|,   1 <= t <= T-2,
// with the validity convolution and the NaN padding of eval_acc_pose folded in: a row whose window holds an invalid frame or
// straddles two sequences is NaN and reads no coordinate, rows 0 and T-1 are NaN.
// One launch, one workgroup per output row.  The primitive runs 256 lanes; the fused entry 512: lanes [0, 256) score the right
// hand, [256, 512) the left, in lock step -- every __syncthreads is reached by both halves whatever the flags say -- and the
// last step forms h = nanmean(r, l) in the same workgroup.  A lane walks its points n = lane, lane + 256, ... (no upper limit
// on their number), fp32 loads, fp64 from the first subtraction on.  Sums are fp64 through one fixed order: the lane's own
// points in index order, __shfl_down inside a wave, then the four waves in order (half_sum of mesh_metrics.hip) -- no atomics,
// no scratch, and a row's bits depend on its three frames alone, not on T, its position or the run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

constexpr int NJ = 21;
constexpr int NT = 256;                          // lanes per hand
constexpr int NW = NT / 64;
constexpr int NQ = HANDS_ACCEL_NQ;

__device__ __forceinline__ float nanmean2(float a, float b) {
  const bool na = isnan(a), nb = isnan(b);
  return ((na ? 0.f : a) + (nb ? 0.f : b)) / (float)((na ? 0 : 1) + (nb ? 0 : 1));
}

// sum over the 256 lanes of one hand, valid on all of them: shuffle tree inside each wave, then the waves in order
template <int N>
__device__ __forceinline__ void half_sum(double (&v)[N], double (*red)[N], int tid) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_down(v[n], o);
  if ((tid & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[tid >> 6][n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = ((red[0][n] + red[1][n]) + red[2][n]) + red[3][n];
}

// (x[t-1] - 2 x[t] + x[t+1]) fps^2 in fp64, in this order
__device__ __forceinline__ double accel(double x0, double x1, double x2, double fps2) { return ((x0 - 2.0 * x1) + x2) * fps2; }

__global__ void __launch_bounds__(NT) accel_error_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         const float* __restrict__ valid, const int32_t* __restrict__ seq,
                                                         float* __restrict__ out, int T, int N, int D, double fps2) {
  __shared__ double red[NW][1];
  const int t = blockIdx.x, tid = threadIdx.x;
  bool live = t >= 1 && t <= T - 2;              // the same for every lane of the workgroup
  if (live && valid) live = valid[t - 1] != 0.f && valid[t] != 0.f && valid[t + 1] != 0.f;
  if (live && seq) live = seq[t - 1] == seq[t] && seq[t] == seq[t + 1];
  if (!live) {                                    // nothing of the window is read
    if (tid == 0) out[t] = __builtin_nanf("");
    return;
  }
  const long long F = (long long)N * D;          // floats per frame
  const float* g0 = gt + (long long)(t - 1) * F;
  const float* p0 = pred + (long long)(t - 1) * F;
  double v[1] = {0.0};
  for (int n = tid; n < N; n += NT) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (c < D) {
        const long long i = (long long)n * D + c;
        const double ag = accel((double)g0[i], (double)g0[i + F], (double)g0[i + 2 * F], fps2);
        const double ap = accel((double)p0[i], (double)p0[i + F], (double)p0[i + 2 * F], fps2);
        const double d = ap - ag;
        s += d * d;
      }
    v[0] += sqrt(s);
  }
  half_sum(v, red, tid);
  if (tid == 0) out[t] = (float)(v[0] / (double)N);
}

struct HandLds {
  double red[NW][NQ];
  float res[NQ];
};

__global__ void __launch_bounds__(2 * NT) accel_metrics_kernel(hands_mesh_eval_in in, const int32_t* __restrict__ seq,
                                                               hands_accel_eval_out out, int T, int V, double fps2) {
  __shared__ HandLds lds[2];
  const int t = blockIdx.x, hand = threadIdx.x / NT, tid = threadIdx.x % NT;
  HandLds& S = lds[hand];
  bool live = t >= 1 && t <= T - 2;              // the same for the 256 lanes of a hand
  if (live) {
    const float* hv = hand ? in.left_valid : in.right_valid;
    for (int k = -1; k <= 1; ++k) live = live && in.is_valid[t + k] * hv[t + k] != 0.f;
  }
  if (live && seq) live = seq[t - 1] == seq[t] && seq[t] == seq[t + 1];

  double v[NQ] = {0.0, 0.0, 0.0};                // sums of |a_pred - a_gt|: vertices root-relative, joints root-relative, joints
  if (live) {                                     // an invalid window is not read
    const long long FV = (long long)V * 3;
    const float* pv = (hand ? in.pred_v3d_l : in.pred_v3d_r) + (long long)(t - 1) * FV;
    const float* gv = (hand ? in.gt_v3d_l : in.gt_v3d_r) + (long long)(t - 1) * FV;
    const float* pj = (hand ? in.pred_j3d_l : in.pred_j3d_r) + (long long)(t - 1) * NJ * 3;
    const float* gj = (hand ? in.gt_j3d_l : in.gt_j3d_r) + (long long)(t - 1) * NJ * 3;
    double pr[3][3], gr[3][3];                    // joint 0 of the three frames
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        pr[k][c] = (double)pj[k * NJ * 3 + c];
        gr[k][c] = (double)gj[k * NJ * 3 + c];
      }
    for (int n = tid; n < V; n += NT) {
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const long long i = 3LL * n + c;
        const double ap = accel((double)pv[i] - pr[0][c], (double)pv[i + FV] - pr[1][c], (double)pv[i + 2 * FV] - pr[2][c], fps2);
        const double ag = accel((double)gv[i] - gr[0][c], (double)gv[i + FV] - gr[1][c], (double)gv[i + 2 * FV] - gr[2][c], fps2);
        const double d = ap - ag;
        s += d * d;
      }
      v[0] += sqrt(s);
    }
    if (tid < NJ) {
      double s_rel = 0.0, s_abs = 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int i = 3 * tid + c;
        const double p0 = (double)pj[i], p1 = (double)pj[i + NJ * 3], p2 = (double)pj[i + 2 * NJ * 3];
        const double g0 = (double)gj[i], g1 = (double)gj[i + NJ * 3], g2 = (double)gj[i + 2 * NJ * 3];
        const double dr = accel(p0 - pr[0][c], p1 - pr[1][c], p2 - pr[2][c], fps2) -
                          accel(g0 - gr[0][c], g1 - gr[1][c], g2 - gr[2][c], fps2);
        const double da = accel(p0, p1, p2, fps2) - accel(g0, g1, g2, fps2);
        s_rel += dr * dr;
        s_abs += da * da;
      }
      v[1] = sqrt(s_rel);
      v[2] = sqrt(s_abs);
    }
  }
  half_sum(v, S.red, tid);
  if (tid == 0) {
    const float NaN = __builtin_nanf("");
    S.res[0] = live ? (float)(v[0] / (double)V) : NaN;
    S.res[1] = live ? (float)(v[1] / (double)NJ) : NaN;
    S.res[2] = live ? (float)(v[2] / (double)NJ) : NaN;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x;
    const float r = lds[0].res[q], l = lds[1].res[q];
    float* const* o = reinterpret_cast<float* const*>(&out);
    o[3 * q][t] = r;
    o[3 * q + 1][t] = l;
    o[3 * q + 2][t] = nanmean2(r, l);
  }
}

bool fps_ok(float fps) { return isfinite(fps) && fps > 0.f; }

}  // namespace

extern "C" int hands_accel_error_f32(const float* gt, const float* pred, const float* valid, const int32_t* seq_id, float* out,
                                     int T, int N, int D, float fps, hands_stream_t stream) {
  if (!gt || !pred || !out || T <= 0 || N <= 0 || D < 1 || D > 3 || !fps_ok(fps)) return HANDS_EINVAL;
  hipLaunchKernelGGL(accel_error_kernel, dim3(T), dim3(NT), 0, (hipStream_t)stream, gt, pred, valid, seq_id, out, T, N, D,
                     (double)fps * (double)fps);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_eval_accel_metrics_f32(const hands_mesh_eval_in* in, const int32_t* seq_id, const hands_accel_eval_out* out,
                                            int T, int V, float fps, hands_stream_t stream) {
  static_assert(sizeof(hands_accel_eval_out) == 3 * NQ * sizeof(void*), "three pointers per quantity");
  if (!in || !out || T <= 0 || V <= 0 || !fps_ok(fps)) return HANDS_EINVAL;
  const void* const* pi = reinterpret_cast<const void* const*>(in);
  for (size_t i = 0; i < sizeof(hands_mesh_eval_in) / sizeof(void*); ++i)
    if (!pi[i]) return HANDS_EINVAL;
  const void* const* po = reinterpret_cast<const void* const*>(out);
  for (size_t i = 0; i < sizeof(hands_accel_eval_out) / sizeof(void*); ++i)
    if (!po[i]) return HANDS_EINVAL;
  hipLaunchKernelGGL(accel_metrics_kernel, dim3(T), dim3(2 * NT), 0, (hipStream_t)stream, *in, seq_id, *out, T, V,
                     (double)fps * (double)fps);
  HANDS_LAUNCH_CHECK();
}
