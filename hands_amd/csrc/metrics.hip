// metrics.hip -- evaluation metrics on device for the gathered predictions:
// root-aligned MPJPE, Procrustes-aligned MPJPE (3x3 SVD per hand), hand-to-hand MRRPE, 2-D pixel error.
// Reference: src/utils/eval_modules.py:97-134,136-219,320-343,386-428; common/metrics.py:23-55;
// common/torch_utils.py:14-19 (nanmean).  One thread per sample; the work is ~2 kFLOP per hand.  eval_metrics_masked_kernel is
// the other branch of eval_mpjpe_pa_ra (:231-317): only the flagged joints of a hand, rooted at the first of them.
// The 3x3 solve behind every alignment is procrustes_solve (procrustes_device.h), shared with mesh_metrics.hip.
// Rank-deficient Procrustes: the rotation is V diag(1,1,det V) U^T with U an orthonormal frame whatever the rank of the
// cross-covariance K.  Rank 2 (planar joints): U_2 = U_0 x U_1.  Rank 1 (the predicted or the ground-truth joints on a line):
// U_1 is completed from the unit axis least aligned with U_0; the error does not depend on the completion and equals the one
// of the reference's LAPACK SVD.  K = 0: a constant prediction gives NaN (scale = 0 / 0, as the reference), a constant ground
// truth gives 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"

namespace {

constexpr int NJ = 21;

// mean over joints of || (gt_j - gt_0) - (pr_j - pr_0) ||     (eval_modules.py:107-121)
__device__ float mpjpe_ra(const float* gt, const float* pr) {
  float s = 0.f;
  for (int j = 0; j < NJ; ++j) {
    float d2 = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float d = (gt[3 * j + c] - gt[c]) - (pr[3 * j + c] - pr[c]);
      d2 += d * d;
    }
    s += sqrtf(d2);
  }
  return s / (float)NJ;
}

// compute_similarity_transform of a 2 x 3 array: the reference transposes its (n,3) input unless n is 2 or 3
// (eval_modules.py:144), so two selected joints are read as THREE points in the plane, point k = (S[0][k], S[1][k]), and the
// error is taken along the rows of the 2 x 3 result (:216).  The proper rotation maximising trace(R K) in the plane is closed
// form: trace(R K) = cos(th) (K00 + K11) + sin(th) (K01 - K10).
__device__ float pa_error_2x3(const double S1[][3], const double S2[][3]) {
  double mu1[2], mu2[2], K[2][2] = {{0, 0}, {0, 0}}, var1 = 0;
  for (int a = 0; a < 2; ++a) {
    mu1[a] = ((S1[a][0] + S1[a][1]) + S1[a][2]) / 3.0;
    mu2[a] = ((S2[a][0] + S2[a][1]) + S2[a][2]) / 3.0;
  }
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 2; ++a) {
      const double x1 = S1[a][k] - mu1[a];
      var1 += x1 * x1;
      for (int b = 0; b < 2; ++b) K[a][b] += x1 * (S2[b][k] - mu2[b]);
    }
  const double c0 = K[0][0] + K[1][1], s0 = K[0][1] - K[1][0], tr = sqrt(c0 * c0 + s0 * s0);
  const double c = tr > 0 ? c0 / tr : 1.0, sn = tr > 0 ? s0 / tr : 0.0;      // tr = 0: the scale is 0 (or NaN), any rotation
  const double R[2][2] = {{c, -sn}, {sn, c}};
  const double scale = tr / var1;
  double s = 0;
  for (int a = 0; a < 2; ++a) {
    const double t = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1]);
    double d2 = 0;
    for (int k = 0; k < 3; ++k) {
      const double h = scale * (R[a][0] * S1[0][k] + R[a][1] * S1[1][k]) + t;
      d2 += (S2[a][k] - h) * (S2[a][k] - h);
    }
    s += sqrt(d2);
  }
  return (float)(s / 2.0);
}

// Procrustes-aligned mean error of ROOT-ALIGNED joints (eval_modules.py:136-219) over the n <= 21 joints sel[0..n) (all 21 in
// order when sel is null), root = the first of them.  n = 2 and n = 3 follow the reference's reading of a 2 x 3 / 3 x 3
// array (see pa_error_2x3): for n = 3 the COLUMNS are the points and the error is taken along the rows.
__device__ float mpjpe_pa_sel(const float* gt, const float* pr, const int* sel, int n) {
  double S1[NJ][3], S2[NJ][3], mu1[3] = {0, 0, 0}, mu2[3] = {0, 0, 0};
  const int root = sel ? sel[0] : 0;
  if (n == 2 || n == 3) {
    double T1[3][3], T2[3][3];
    for (int j = 0; j < n; ++j)
      for (int c = 0; c < 3; ++c) {
        T1[j][c] = (double)(pr[3 * sel[j] + c] - pr[3 * root + c]);
        T2[j][c] = (double)(gt[3 * sel[j] + c] - gt[3 * root + c]);
      }
    if (n == 2) return pa_error_2x3(T1, T2);
    for (int j = 0; j < 3; ++j)                          // point j = column j
      for (int c = 0; c < 3; ++c) {
        S1[j][c] = T1[c][j]; S2[j][c] = T2[c][j];
        mu1[c] += S1[j][c]; mu2[c] += S2[j][c];
      }
  } else {
    for (int j = 0; j < n; ++j) {
      const int js = sel ? sel[j] : j;
      for (int c = 0; c < 3; ++c) {
        S1[j][c] = (double)(pr[3 * js + c] - pr[3 * root + c]);      // root alignment in fp32, as the reference
        S2[j][c] = (double)(gt[3 * js + c] - gt[3 * root + c]);
        mu1[c] += S1[j][c]; mu2[c] += S2[j][c];
      }
    }
  }
  for (int c = 0; c < 3; ++c) { mu1[c] /= n; mu2[c] /= n; }
  double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0;
  for (int j = 0; j < n; ++j)
    for (int a = 0; a < 3; ++a) {
      const double x1 = S1[j][a] - mu1[a];
      var1 += x1 * x1;
      for (int b = 0; b < 3; ++b) K[a][b] += x1 * (S2[j][b] - mu2[b]);
    }
  double R[3][3], scale;
  procrustes_solve(K, var1, R, &scale);
  double t[3];
  for (int a = 0; a < 3; ++a) t[a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
  if (n == 3) {                                          // error along the rows of the 3 x 3 result: one per coordinate
    double d2[3] = {0, 0, 0};
    for (int j = 0; j < 3; ++j)
      for (int a = 0; a < 3; ++a) {
        const double h = scale * (R[a][0] * S1[j][0] + R[a][1] * S1[j][1] + R[a][2] * S1[j][2]) + t[a];
        d2[a] += (S2[j][a] - h) * (S2[j][a] - h);
      }
    return (float)(((sqrt(d2[0]) + sqrt(d2[1])) + sqrt(d2[2])) / 3.0);
  }
  double s = 0;
  for (int j = 0; j < n; ++j) {
    double d2 = 0;
    for (int a = 0; a < 3; ++a) {
      const double h = scale * (R[a][0] * S1[j][0] + R[a][1] * S1[j][1] + R[a][2] * S1[j][2]) + t[a];
      d2 += (S2[j][a] - h) * (S2[j][a] - h);
    }
    s += sqrt(d2);
  }
  return (float)(s / n);
}

__device__ float mpjpe_pa(const float* gt, const float* pr) { return mpjpe_pa_sel(gt, pr, nullptr, NJ); }

__device__ __forceinline__ float nanmean2(float a, float b) {
  const bool na = isnan(a), nb = isnan(b);
  return ((na ? 0.f : a) + (nb ? 0.f : b)) / (float)((na ? 0 : 1) + (nb ? 0 : 1));
}

__global__ void eval_metrics_kernel(hands_eval_in in, hands_eval_out out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float NaN = __builtin_nanf("");
  const float isv = in.is_valid[b];
  const float rv = in.right_valid[b] * isv, lv = in.left_valid[b] * isv;
  const float* gr = in.gt_j3d_r + (long long)b * NJ * 3;
  const float* gl = in.gt_j3d_l + (long long)b * NJ * 3;
  const float* pr = in.pred_j3d_r + (long long)b * NJ * 3;
  const float* pl = in.pred_j3d_l + (long long)b * NJ * 3;
  const float ra_r = rv != 0.f ? mpjpe_ra(gr, pr) : NaN;
  const float ra_l = lv != 0.f ? mpjpe_ra(gl, pl) : NaN;
  out.mpjpe_ra_h[b] = nanmean2(ra_r, ra_l) * 1000.0f;
  const float pa_r = mpjpe_pa(gr, pr) * rv, pa_l = mpjpe_pa(gl, pl) * lv;   // invalid -> 0, not nan (:217)
  out.mpjpe_pa_ra_r[b] = pa_r * 1000.0f;
  out.mpjpe_pa_ra_l[b] = pa_l * 1000.0f;
  out.mpjpe_pa_ra_h[b] = nanmean2(pa_r, pa_l) * 1000.0f;
  float d2 = 0.f;
  for (int c = 0; c < 3; ++c) {
    const float d = (pl[c] - pr[c]) - (gl[c] - gr[c]);
    d2 += d * d;
  }
  out.mrrpe_rl[b] = (lv * rv) != 0.f ? sqrtf(d2) * 1000.0f : NaN;
  for (int j = 0; j < NJ; ++j) {
    const long long i = (long long)b * NJ + j;
    const float dxr = in.gt_j2d_r[2 * i] - in.pred_j2d_r[2 * i], dyr = in.gt_j2d_r[2 * i + 1] - in.pred_j2d_r[2 * i + 1];
    const float dxl = in.gt_j2d_l[2 * i] - in.pred_j2d_l[2 * i], dyl = in.gt_j2d_l[2 * i + 1] - in.pred_j2d_l[2 * i + 1];
    out.pix_err_r[i] = in.joints_valid_r[i] * rv != 0.f ? sqrtf(dxr * dxr + dyr * dyr) : NaN;
    out.pix_err_l[i] = in.joints_valid_l[i] * lv != 0.f ? sqrtf(dxl * dxl + dyl * dyl) : NaN;
  }
}

// The egoexo branch of eval_mpjpe_pa_ra (eval_modules.py:231-317) for one hand: only the joints flagged in jv3d (21) count,
// the root is the first of them.  None flagged: all three NaN.  The PA error is multiplied by the hand's validity (:217).
__device__ void masked_hand(const float* gt, const float* pr, const float* jv3d, float valid, float* rao, float* abs_, float* pa) {
  int sel[NJ], n = 0;
  for (int j = 0; j < NJ; ++j)
    if (jv3d[j] != 0.f) sel[n++] = j;                   // .bool(): any non-zero flag (a NaN flag included)
  if (n == 0) {
    *rao = *abs_ = *pa = __builtin_nanf("");
    return;
  }
  float sa = 0.f, sr = 0.f;
  for (int k = 0; k < n; ++k) {
    float a2 = 0.f, r2 = 0.f;
    for (int c = 0; c < 3; ++c) {
      const float g = gt[3 * sel[k] + c], p = pr[3 * sel[k] + c];
      const float da = g - p, dr = (g - gt[3 * sel[0] + c]) - (p - pr[3 * sel[0] + c]);
      a2 += da * da;
      r2 += dr * dr;
    }
    sa += sqrtf(a2);
    sr += sqrtf(r2);
  }
  *abs_ = sa / (float)n;
  *rao = sr / (float)n;
  *pa = mpjpe_pa_sel(gt, pr, sel, n) * valid;
}

__global__ void eval_metrics_masked_kernel(hands_eval_in in, const float* __restrict__ jv3d_r, const float* __restrict__ jv3d_l,
                                           hands_eval_masked_out out, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float isv = in.is_valid[b];
  const float rv = in.right_valid[b] * isv, lv = in.left_valid[b] * isv;
  const long long o = (long long)b * NJ;
  float rao_r, abs_r, pa_r, rao_l, abs_l, pa_l;
  masked_hand(in.gt_j3d_r + o * 3, in.pred_j3d_r + o * 3, jv3d_r + o, rv, &rao_r, &abs_r, &pa_r);
  masked_hand(in.gt_j3d_l + o * 3, in.pred_j3d_l + o * 3, jv3d_l + o, lv, &rao_l, &abs_l, &pa_l);
  out.rao_r[b] = rao_r * 1000.0f; out.rao_l[b] = rao_l * 1000.0f; out.rao_h[b] = nanmean2(rao_r, rao_l) * 1000.0f;
  out.abs_r[b] = abs_r * 1000.0f; out.abs_l[b] = abs_l * 1000.0f; out.abs_h[b] = nanmean2(abs_r, abs_l) * 1000.0f;
  out.pa_ra_r[b] = pa_r * 1000.0f; out.pa_ra_l[b] = pa_l * 1000.0f; out.pa_ra_h[b] = nanmean2(pa_r, pa_l) * 1000.0f;
}

// process_data_light (src/callbacks/process/process_arctic.py:41-73): camera-space targets from the
// canonical GT MANO output and the annotated camera-space joints.
__global__ void gt_targets_kernel(const float* __restrict__ joints, const float* __restrict__ verts,
                                  const float* __restrict__ j3d_full, const float* __restrict__ Kmat, float img_res,
                                  float* __restrict__ v3d_cam, float* __restrict__ cam_t, float* __restrict__ cam_t_wp,
                                  int B, int NV) {
  __shared__ float tr[3];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* jc = joints + (long long)b * NJ * 3;
  const float* jf = j3d_full + (long long)b * NJ * 3;
  if (tid < 3) {
    float s = 0.f;                                     // Tr0 = (j3d.full - joints).mean(dim=1)
    for (int j = 0; j < NJ; ++j) s += jf[3 * j + tid] - jc[3 * j + tid];
    tr[tid] = s / (float)NJ;
    cam_t[b * 3 + tid] = jf[tid] - jc[tid];            // root_cam - root_cano
  }
  if (tid == 0) {
    const float f = (Kmat[b * 9 + 0] + Kmat[b * 9 + 4]) / 2.0f;
    const float tz = jf[2] - jc[2];
    cam_t_wp[b * 3 + 0] = 2.0f * f / (img_res * tz + 1e-9f);    // camera.py:10-29
    cam_t_wp[b * 3 + 1] = jf[0] - jc[0];
    cam_t_wp[b * 3 + 2] = jf[1] - jc[1];
  }
  __syncthreads();
  const float* v = verts + (long long)b * NV * 3;
  float* o = v3d_cam + (long long)b * NV * 3;
  for (int i = tid; i < NV * 3; i += blockDim.x) o[i] = v[i] + tr[i % 3];
}

// unormalize_kp2d (common/data_utils.py:368-373): 0.5 * res * (x + 1)
__global__ void unnormalize_kernel(const float* __restrict__ x, float* __restrict__ out, long long n, float img_res) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = 0.5f * img_res * (x[i] + 1.0f);
}

}  // namespace

extern "C" int hands_gt_targets_f32(const float* joints, const float* verts, const float* j3d_full, const float* K,
                                    float img_res, float* v3d_cam, float* cam_t, float* cam_t_wp, int B, int NV,
                                    hands_stream_t stream) {
  if (!joints || !verts || !j3d_full || !K || !v3d_cam || !cam_t || !cam_t_wp || B <= 0 || NV <= 0) return HANDS_EINVAL;
  hipLaunchKernelGGL(gt_targets_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, joints, verts, j3d_full, K, img_res,
                     v3d_cam, cam_t, cam_t_wp, B, NV);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_unnormalize_kp2d_f32(const float* x, float* out, long long n, float img_res, hands_stream_t stream) {
  if (!x || !out || n <= 0) return HANDS_EINVAL;
  hipLaunchKernelGGL(unnormalize_kernel, dim3(hands_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, x, out, n, img_res);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_eval_metrics_f32(const hands_eval_in* in, const hands_eval_out* out, int B, hands_stream_t stream) {
  if (!in || !out || B <= 0) return HANDS_EINVAL;
  const void* const* pi = reinterpret_cast<const void* const*>(in);
  for (size_t i = 0; i < sizeof(hands_eval_in) / sizeof(void*); ++i)
    if (!pi[i]) return HANDS_EINVAL;
  const void* const* po = reinterpret_cast<const void* const*>(out);
  for (size_t i = 0; i < sizeof(hands_eval_out) / sizeof(void*); ++i)
    if (!po[i]) return HANDS_EINVAL;
  hipLaunchKernelGGL(eval_metrics_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *in, *out, B);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_eval_metrics_masked_f32(const hands_eval_in* in, const float* joints3d_valid_r, const float* joints3d_valid_l,
                                             const hands_eval_masked_out* out, int B, hands_stream_t stream) {
  if (!in || !out || !joints3d_valid_r || !joints3d_valid_l || B <= 0) return HANDS_EINVAL;
  const void* const* pi = reinterpret_cast<const void* const*>(in);
  for (size_t i = 0; i < sizeof(hands_eval_in) / sizeof(void*); ++i)
    if (!pi[i]) return HANDS_EINVAL;
  const void* const* po = reinterpret_cast<const void* const*>(out);
  for (size_t i = 0; i < sizeof(hands_eval_masked_out) / sizeof(void*); ++i)
    if (!po[i]) return HANDS_EINVAL;
  hipLaunchKernelGGL(eval_metrics_masked_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *in, joints3d_valid_r,
                     joints3d_valid_l, *out, B);
  HANDS_LAUNCH_CHECK();
}
