// mesh_metrics.hip -- mesh metrics on device (hands_eval_mesh_metrics_f32 of include/hands_hip.h): per hand MPVPE, F@5mm, F@15mm
// and the AUC of the PCK curve over vertices and joints, each after root alignment (ra) and after Procrustes alignment (pa).
// One launch, one workgroup of 512 lanes per sample: lanes [0, 256) score the right hand, [256, 512) the left, in lock step --
// every __syncthreads is reached by both halves whatever the validity flags say (an invalid hand is scored on zeros and its
// results are replaced by NaN), and the last step forms h = nanmean(r, l) in the same workgroup.  Both root-aligned vertex
// clouds of a hand sit in LDS (2 x V x 12 bytes); a lane owns the vertices lane, lane + 256, ... (at most 4) in registers and
// walks all candidates of the nearest-neighbour searches from LDS, where every lane reads the same address (a broadcast).
// Sums are fp64 (counts are integers carried in fp64, exact) through one fixed tree: __shfl_down inside a wave, then the four
// waves in order -- no atomics, so the bits do not depend on the run or on the batch around a sample.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"

namespace {

constexpr int NJ = 21;
constexpr int NT = 256;                          // lanes per hand
constexpr int NW = NT / 64;
constexpr int MAXV = HANDS_MESH_MAX_V;
constexpr int QPL = MAXV / NT;                   // vertices a lane owns, at most
constexpr int NQ = HANDS_MESH_NQ;
constexpr int NRED = 10;                         // widest reduction (K and var1)
static_assert(MAXV % NT == 0, "a lane owns MAXV / NT vertices");

struct HandLds {
  float P[MAXV * 3], G[MAXV * 3];                // root-aligned prediction (later: Procrustes-aligned) and ground truth
  float PJ[NJ * 3], GJ[NJ * 3];                  // root-aligned joints
  double red[NW][NRED];
  double xf[13];                                 // scale, R (9), t (3) of the vertex fit
  double jw[2];                                  // AUC weights of the joints: ra, pa (NaN: the joint fit is not finite)
  float res[NQ];
};

__device__ __forceinline__ float nanmean2(float a, float b) {
  const bool na = isnan(a), nb = isnan(b);
  return ((na ? 0.f : a) + (nb ? 0.f : b)) / (float)((na ? 0 : 1) + (nb ? 0 : 1));
}

// sum over the 256 lanes of one hand, valid on all of them: shuffle tree inside each wave, then the waves in order
template <int N>
__device__ void half_sum(double (&v)[N], double (*red)[NRED], int tid) {
  static_assert(N <= NRED, "red is too narrow");
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_down(v[n], o);
  __syncthreads();                               // red may still be read from the previous call
  if ((tid & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[tid >> 6][n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = ((red[0][n] + red[1][n]) + red[2][n]) + red[3][n];
}

// Share of one point in 198 x (area under the PCK curve / 0.05): with k0 the smallest k such that e <= t_k = k * 0.05 / 99,
// the trapezoid rule over k = 0..99 gives 1 for k0 = 0, (99.5 - k0) / 99 for 1 <= k0 <= 99, 0 beyond.  A NaN error counts 0.
__device__ int auc_weight198(double e) {
  const double h = 0.05 / 99.0;
  if (!(e > 0.0)) return e == 0.0 ? 198 : 0;     // e = 0; negative or NaN cannot come from a norm of finite numbers
  const double x = ceil(e / h);
  if (!(x < 101.0)) return 0;
  int k = (int)x;                                 // 1 .. 100, off by at most one from the rounding of e / h
  if (e <= (double)(k - 1) * h) --k;
  else if (e > (double)k * h) ++k;
  return k <= 0 ? 198 : (k <= 99 ? 199 - 2 * k : 0);
}

// The five vertex quantities of one alignment from the clouds in LDS and the lane's own vertices p (prediction), g (ground
// truth); n_own of them are real.  res[0..4) = mpvpe (m), F@5mm, F@15mm, AUC over the vertices.
__device__ void vertex_stage(const HandLds& S, const float (&p)[QPL][3], const float (&g)[QPL][3], int n_own, int V, int tid,
                             double (*red)[NRED], float* res) {
  float m1[QPL], m2[QPL];                         // squared distance: own gt vertex -> nearest prediction, own prediction -> nearest gt
#pragma unroll
  for (int k = 0; k < QPL; ++k) m1[k] = m2[k] = INFINITY;
#pragma unroll 2
  for (int j = 0; j < V; ++j) {
    const float px = S.P[3 * j], py = S.P[3 * j + 1], pz = S.P[3 * j + 2];
    const float gx = S.G[3 * j], gy = S.G[3 * j + 1], gz = S.G[3 * j + 2];
#pragma unroll
    for (int k = 0; k < QPL; ++k) {
      const float ax = g[k][0] - px, ay = g[k][1] - py, az = g[k][2] - pz;
      const float bx = p[k][0] - gx, by = p[k][1] - gy, bz = p[k][2] - gz;
      m1[k] = fminf(m1[k], (ax * ax + ay * ay) + az * az);
      m2[k] = fminf(m2[k], (bx * bx + by * by) + bz * bz);
    }
  }
  double v[6] = {0, 0, 0, 0, 0, 0};               // sum of errors, AUC weight, then the counts P@5, R@5, P@15, R@15
#pragma unroll
  for (int k = 0; k < QPL; ++k)
    if (k < n_own) {
      const float dx = g[k][0] - p[k][0], dy = g[k][1] - p[k][1], dz = g[k][2] - p[k][2];
      const float e = sqrtf((dx * dx + dy * dy) + dz * dz);
      const float d1 = sqrtf(m1[k]), d2 = sqrtf(m2[k]);
      v[0] += (double)e;
      v[1] += (double)auc_weight198((double)e);
      v[2] += d1 < 0.005f ? 1.0 : 0.0;
      v[3] += d2 < 0.005f ? 1.0 : 0.0;
      v[4] += d1 < 0.015f ? 1.0 : 0.0;
      v[5] += d2 < 0.015f ? 1.0 : 0.0;
    }
  half_sum(v, red, tid);
  const double n = (double)V;
  res[0] = (float)(v[0] / n);
  for (int f = 0; f < 2; ++f) {
    const double P = v[2 + 2 * f] / n, R = v[3 + 2 * f] / n;
    res[1 + f] = P + R > 0.0 ? (float)(2.0 * P * R / (P + R)) : 0.f;
  }
  res[3] = (float)(v[1] / (198.0 * n));
}

// One copy of the solve for its two call sites, out of line: inlined, its fp64 temporaries would set the register budget of the
// whole kernel, the nearest-neighbour loops included
__device__ __noinline__ void solve(const double K[3][3], double var1, double R[3][3], double* scale) {
  procrustes_solve(K, var1, R, scale);
}

// AUC weights of the 21 joints, by one lane: root-aligned, and aligned by the similarity transform fitted on the joints with
// the operations of mpjpe_pa (metrics.hip) in their order
__device__ __noinline__ void joint_stage(HandLds& S) {
  int w_ra = 0;
  for (int j = 0; j < NJ; ++j) {
    const float dx = S.GJ[3 * j] - S.PJ[3 * j], dy = S.GJ[3 * j + 1] - S.PJ[3 * j + 1], dz = S.GJ[3 * j + 2] - S.PJ[3 * j + 2];
    w_ra += auc_weight198((double)sqrtf((dx * dx + dy * dy) + dz * dz));
  }
  S.jw[0] = (double)w_ra;
  double mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
  for (int j = 0; j < NJ; ++j)
    for (int c = 0; c < 3; ++c) { mu1[c] += (double)S.PJ[3 * j + c]; mu2[c] += (double)S.GJ[3 * j + c]; }
  for (int c = 0; c < 3; ++c) { mu1[c] /= NJ; mu2[c] /= NJ; }
  double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0;
  for (int j = 0; j < NJ; ++j)
    for (int a = 0; a < 3; ++a) {
      const double x1 = (double)S.PJ[3 * j + a] - mu1[a];
      var1 += x1 * x1;
      for (int b = 0; b < 3; ++b) K[a][b] += x1 * ((double)S.GJ[3 * j + b] - mu2[b]);
    }
  double R[3][3], scale, t[3];
  solve(K, var1, R, &scale);
  for (int a = 0; a < 3; ++a) t[a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
  int w_pa = 0;
  bool finite = true;
  for (int j = 0; j < NJ; ++j) {
    double d2 = 0;
    for (int a = 0; a < 3; ++a) {
      const double h = scale * (R[a][0] * (double)S.PJ[3 * j] + R[a][1] * (double)S.PJ[3 * j + 1] + R[a][2] * (double)S.PJ[3 * j + 2]) + t[a];
      d2 += ((double)S.GJ[3 * j + a] - h) * ((double)S.GJ[3 * j + a] - h);
    }
    finite = finite && isfinite(d2);
    w_pa += auc_weight198(sqrt(d2));
  }
  S.jw[1] = finite ? (double)w_pa : (double)__builtin_nanf("");
}

__global__ void __launch_bounds__(2 * NT) mesh_metrics_kernel(hands_mesh_eval_in in, hands_mesh_eval_out out, int V) {
  __shared__ HandLds lds[2];
  const int b = blockIdx.x, hand = threadIdx.x / NT, tid = threadIdx.x % NT;
  HandLds& S = lds[hand];
  const float NaN = __builtin_nanf("");
  const bool live = in.is_valid[b] * (hand ? in.left_valid[b] : in.right_valid[b]) != 0.f;
  const float* pv = (hand ? in.pred_v3d_l : in.pred_v3d_r) + (long long)b * V * 3;
  const float* gv = (hand ? in.gt_v3d_l : in.gt_v3d_r) + (long long)b * V * 3;
  const float* pj = (hand ? in.pred_j3d_l : in.pred_j3d_r) + (long long)b * NJ * 3;
  const float* gj = (hand ? in.gt_j3d_l : in.gt_j3d_r) + (long long)b * NJ * 3;

  // ---- load and root-align in fp32 (eval_mpjpe_ra); an invalid hand is not read.  Every coordinate is looked at once here,
  //      the root among the joints: `bad` counts the non-finite ones
  float pr0[3] = {0.f, 0.f, 0.f}, gr0[3] = {0.f, 0.f, 0.f};
  if (live)
    for (int c = 0; c < 3; ++c) { pr0[c] = pj[c]; gr0[c] = gj[c]; }
  int bad = 0;
  for (int i = tid; i < V * 3; i += NT) {
    const float x = live ? pv[i] : 0.f, y = live ? gv[i] : 0.f;
    bad += (isfinite(x) ? 0 : 1) + (isfinite(y) ? 0 : 1);
    S.P[i] = x - pr0[i % 3];
    S.G[i] = y - gr0[i % 3];
  }
  if (tid < NJ * 3) {
    const float x = live ? pj[tid] : 0.f, y = live ? gj[tid] : 0.f;
    bad += (isfinite(x) ? 0 : 1) + (isfinite(y) ? 0 : 1);
    S.PJ[tid] = x - pr0[tid % 3];
    S.GJ[tid] = y - gr0[tid % 3];
  }
  __syncthreads();

  float p[QPL][3], g[QPL][3];
  int n_own = 0;
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int q = tid + k * NT;
    const bool own = q < V;
    n_own += own ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[k][c] = own ? S.P[3 * q + c] : 0.f;
      g[k][c] = own ? S.G[3 * q + c] : 0.f;
    }
  }

  float res[NQ];
  vertex_stage(S, p, g, n_own, V, tid, S.red, res);                        // ra: res[0..4)

  // ---- similarity transform of the root-aligned vertices (compute_similarity_transform): means, then K and var1, in fp64
  double m[7] = {0, 0, 0, 0, 0, 0, (double)bad};
#pragma unroll
  for (int k = 0; k < QPL; ++k)
    if (k < n_own)
      for (int c = 0; c < 3; ++c) { m[c] += (double)p[k][c]; m[3 + c] += (double)g[k][c]; }
  half_sum(m, S.red, tid);
  const bool hand_bad = m[6] != 0.0;
  double mu1[3], mu2[3];
  for (int c = 0; c < 3; ++c) { mu1[c] = m[c] / (double)V; mu2[c] = m[3 + c] / (double)V; }
  double kv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                          // K row-major, var1
#pragma unroll
  for (int k = 0; k < QPL; ++k)
    if (k < n_own)
      for (int a = 0; a < 3; ++a) {
        const double x1 = (double)p[k][a] - mu1[a];
        kv[9] += x1 * x1;
        for (int c = 0; c < 3; ++c) kv[3 * a + c] += x1 * ((double)g[k][c] - mu2[c]);
      }
  half_sum(kv, S.red, tid);
  if (tid < 64) {                                                          // wave 0: the vertex fit, every lane the same
    double K[3][3], R[3][3], scale;
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) K[a][c] = kv[3 * a + c];
    solve(K, kv[9], R, &scale);
    if (tid == 0) {
      S.xf[0] = scale;
      for (int a = 0; a < 3; ++a) {
        for (int c = 0; c < 3; ++c) S.xf[1 + 3 * a + c] = R[a][c];
        S.xf[10 + a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
      }
    }
  } else if (tid == 64) {                                                  // wave 1, one lane: the joints, meanwhile
    joint_stage(S);
  }
  __syncthreads();                                                         // also: every lane is done reading P (ra stage)
  bool fit_finite = true;
  {
    const double scale = S.xf[0];
#pragma unroll
    for (int k = 0; k < QPL; ++k)
      if (k < n_own)
        for (int a = 0; a < 3; ++a) {
          const double h = scale * (S.xf[1 + 3 * a] * (double)p[k][0] + S.xf[2 + 3 * a] * (double)p[k][1] +
                                    S.xf[3 + 3 * a] * (double)p[k][2]) + S.xf[10 + a];
          S.P[3 * (tid + k * NT) + a] = (float)h;
        }
    for (int i = 0; i < 13; ++i) fit_finite = fit_finite && isfinite(S.xf[i]);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < QPL; ++k)
    if (k < n_own)
      for (int c = 0; c < 3; ++c) p[k][c] = S.P[3 * (tid + k * NT) + c];
  vertex_stage(S, p, g, n_own, V, tid, S.red, res + 5);                    // pa: res[5..9)

  if (tid == 0) {
    res[4] = (float)(S.jw[0] / (198.0 * NJ));
    res[9] = (float)(S.jw[1] / (198.0 * NJ));                             // NaN when the joint fit is not finite
    if (!fit_finite)                                                       // a constant prediction: scale = 0 / 0, as mpjpe_pa
      for (int q = 5; q < 9; ++q) res[q] = NaN;
    res[0] *= 1000.0f;                                                     // millimetres
    res[5] *= 1000.0f;
    for (int q = 0; q < NQ; ++q) S.res[q] = live && !hand_bad ? res[q] : NaN;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const int q = threadIdx.x;
    const float r = lds[0].res[q], l = lds[1].res[q];
    float* const* o = reinterpret_cast<float* const*>(&out);
    o[3 * q][b] = r;
    o[3 * q + 1][b] = l;
    o[3 * q + 2][b] = nanmean2(r, l);
  }
}

}  // namespace

extern "C" int hands_eval_mesh_metrics_f32(const hands_mesh_eval_in* in, const hands_mesh_eval_out* out, int B, int V,
                                           hands_stream_t stream) {
  static_assert(sizeof(hands_mesh_eval_out) == 3 * NQ * sizeof(void*), "three pointers per quantity");
  if (!in || !out || B <= 0 || V < 1 || V > MAXV) return HANDS_EINVAL;
  const void* const* pi = reinterpret_cast<const void* const*>(in);
  for (size_t i = 0; i < sizeof(hands_mesh_eval_in) / sizeof(void*); ++i)
    if (!pi[i]) return HANDS_EINVAL;
  const void* const* po = reinterpret_cast<const void* const*>(out);
  for (size_t i = 0; i < sizeof(hands_mesh_eval_out) / sizeof(void*); ++i)
    if (!po[i]) return HANDS_EINVAL;
  hipLaunchKernelGGL(mesh_metrics_kernel, dim3(B), dim3(2 * NT), 0, (hipStream_t)stream, *in, *out, V);
  HANDS_LAUNCH_CHECK();
}
