// fit_device.h -- the device routines the MANO fitting kernels share (fit.hip: the fits to 21 3-D joints and to 21 2-D keypoints;
// fit_verts.hip: the fit to 778 vertices): the 61 unknowns and the packed lower triangle, the LDS state of a hand, the 3 x 3
// products, Log / Exp on SO(3), the kinematic tree, d p_i / d beta along the chain and the Cholesky factorisation and solve.
// DESIGN.md section 7 "MANO fitting" is the specification.  Every routine is called by all 256 lanes of a workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"

namespace {

constexpr int NT = 256;                          // lanes of a workgroup
constexpr int NU = 61;                           // unknowns: 16 x 3 rotation increments, 10 shape, 3 translation
constexpr int NR = 63;                           // data rows: 21 joints x 3
constexpr int HP = NU * (NU + 1) / 2;            // the packed lower triangle: entry (a, b <= a) at a (a + 1) / 2 + b
constexpr int UB = 48, UT = 58;                  // first shape column, first translation column
constexpr double PI = 3.14159265358979323846;
constexpr double MU_MIN = 1e-9, MU_MAX = 1e6;

template <int ROWS>                              // data rows: 63 (3-D joints) or 42 (2-D keypoints)
struct Lds {
  double J[ROWS * NU];
  double H[HP];
  double diag[NU], g[NU], d[NU];                 // the pivots of the factor, J^T r, the step
  double R[2][144], beta[2][10], t[2][3];        // state 0: current, 1: candidate
  double M[144];                                 // Exp(pose_mean_j)
  // of the state evaluate() saw last
  double Jr[48], Q[144], p[48], vp[15], x[240], A[45], joints[63], lg[45], r[ROWS];
  double dp[480];                                // d p_i / d beta, (16, 3, 10)
  double y[ROWS], w[21], sw[21];                 // the target, w_k and the row scale of joint k
  double c[2];                                   // cost, and sum_k w_k |e_k|^2 of the rmse
};

// D = A^T B, row-major 3x3
__device__ __forceinline__ void mul_tn(const double* A, const double* B, double* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}

__device__ __forceinline__ void mul_nn(const double* A, const double* B, double* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// Log and Exp on SO(3) with the branches of DESIGN.md section 7 (the arithmetic of smooth.hip)
__device__ __forceinline__ void log_so3(const double* D, double* w) {
  const double v0 = 0.5 * (D[7] - D[5]), v1 = 0.5 * (D[2] - D[6]), v2 = 0.5 * (D[3] - D[1]);
  const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  const double c = 0.5 * (((D[0] + D[4]) + D[8]) - 1.0);
  if (s >= 1e-9) {
    const double k = atan2(s, c) / s;
    w[0] = v0 * k; w[1] = v1 * k; w[2] = v2 * k;
  } else if (c >= 0.0) {
    w[0] = v0; w[1] = v1; w[2] = v2;
  } else {                                       // a half turn: the axis from the symmetric part
    double u0 = sqrt(fmax(0.0, (D[0] - c) / (1.0 - c)));
    double u1 = sqrt(fmax(0.0, (D[4] - c) / (1.0 - c)));
    double u2 = sqrt(fmax(0.0, (D[8] - c) / (1.0 - c)));
    const double s01 = D[1] + D[3], s02 = D[2] + D[6], s12 = D[5] + D[7];
    if (u0 >= u1 && u0 >= u2) {
      u1 = s01 < 0.0 ? -u1 : u1;
      u2 = s02 < 0.0 ? -u2 : u2;
    } else if (u1 >= u2) {
      u0 = s01 < 0.0 ? -u0 : u0;
      u2 = s12 < 0.0 ? -u2 : u2;
    } else {
      u0 = s02 < 0.0 ? -u0 : u0;
      u1 = s12 < 0.0 ? -u1 : u1;
    }
    const double k = PI / sqrt((u0 * u0 + u1 * u1) + u2 * u2);
    w[0] = u0 * k; w[1] = u1 * k; w[2] = u2 * k;
  }
}

__device__ __forceinline__ void exp_so3(const double* w, double* E) {
  const double theta = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double K2[9];
  mul_nn(K, K, K2);
  double a = 1.0, b = 0.5;
  if (theta >= 1e-6) {
    double sn, cs;
    sincos(theta, &sn, &cs);
    a = sn / theta;
    b = (1.0 - cs) / (theta * theta);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * K[i]) + b * K2[i];
}

// joint i is joint j or one of its descendants (wrist 0, finger f = joints 1 + 3 f .. 3 + 3 f)
__device__ __forceinline__ bool at_or_below(int j, int i) { return j == 0 || (i >= j && (i - 1) / 3 == (j - 1) / 3); }
__device__ __forceinline__ int parent_of(int i) { return (i - 1) % 3 == 0 ? 0 : i - 1; }      // i >= 1

// d p_i / d beta along the chain, at the state kinematics() saw last; ends with a barrier
template <int ROWS>
__device__ void shape_chain(Lds<ROWS>& S, const hands_mano_fit_consts& C, int tid) {
  if (tid < 10) {                                // d p_i / d beta_l along the chain, l = tid
    for (int i = 0; i < 16; ++i) {
      const int a = i == 0 ? 0 : parent_of(i);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double v = (double)C.J_shapedirs[(3 * i + c) * 10 + tid];
        if (i > 0) {
          const double e0 = (double)C.J_shapedirs[(3 * i) * 10 + tid] - (double)C.J_shapedirs[(3 * a) * 10 + tid];
          const double e1 = (double)C.J_shapedirs[(3 * i + 1) * 10 + tid] - (double)C.J_shapedirs[(3 * a + 1) * 10 + tid];
          const double e2 = (double)C.J_shapedirs[(3 * i + 2) * 10 + tid] - (double)C.J_shapedirs[(3 * a + 2) * 10 + tid];
          const double* q = S.Q + 9 * a + 3 * c;
          v = S.dp[(3 * a + c) * 10 + tid] + ((q[0] * e0 + q[1] * e1) + q[2] * e2);
        }
        S.dp[(3 * i + c) * 10 + tid] = v;
      }
    }
  }
  __syncthreads();
}

// Cholesky of the packed lower triangle in place (the pivots' roots go to S.diag), then L L^T d = -g.  -> false at a pivot that
// is not positive; the same value on every lane.
template <int ROWS>
__device__ bool solve(Lds<ROWS>& S, int tid) {
  bool ok = true;
  const int i = tid & 63, jg = tid >> 6;
  for (int k = 0; k < NU; ++k) {
    const double piv = S.H[k * (k + 1) / 2 + k];
    ok = ok && piv > 0.0;
    const double dd = sqrt(piv > 0.0 ? piv : 1.0);
    if (tid > k && tid < NU) S.H[tid * (tid + 1) / 2 + k] /= dd;       // the pivot itself stays: other lanes still read it
    if (tid == 0) S.diag[k] = dd;
    __syncthreads();
    if (i > k && i < NU) {
      const double lik = S.H[i * (i + 1) / 2 + k];
      for (int j = k + 1 + jg; j <= i; j += 4) S.H[i * (i + 1) / 2 + j] -= lik * S.H[j * (j + 1) / 2 + k];
    }
    __syncthreads();
  }
  if (tid < 64) {                                // wave 0: forward, then backward substitution; lane u holds entry u
    const int u = tid < NU ? tid : NU - 1;
    double b = tid < NU ? -S.g[tid] : 0.0;
    for (int k = 0; k < NU; ++k) {
      const double yk = __shfl(b, k) / S.diag[k];
      if (tid == k) b = yk;
      if (tid > k && tid < NU) b -= S.H[u * (u + 1) / 2 + k] * yk;
    }
    for (int k = NU - 1; k >= 0; --k) {
      const double xk = __shfl(b, k) / S.diag[k];
      if (tid == k) b = xk;
      if (tid < k) b -= S.H[k * (k + 1) / 2 + u] * xk;
    }
    if (tid < NU) S.d[tid] = b;
  }
  __syncthreads();
  return ok;
}

}  // namespace
