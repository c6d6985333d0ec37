// fit_device.h -- the device routines the MANO fitting kernels share (fit.hip: the fits to 21 3-D joints and to 21 2-D keypoints;
// fit_verts.hip: the fit to 778 vertices): the 61 unknowns and the packed lower triangle, the LDS state of a hand, the 3 x 3
// products, Log / Exp on SO(3), the kinematic tree, d p_i / d beta along the chain, the Cholesky factorisation and solve, and the
// driver -- the set-up of a hand's state, the Levenberg-Marquardt stage, the stores -- with the host's argument rules.
// DESIGN.md section 7 "MANO fitting" is the specification.  Every device routine but place_rigid is called by all 256 lanes of a
// workgroup.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
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

// ---- the driver: what a fit does around its own evaluate / linearise (DESIGN.md section 7 "The shared driver") ----------------
// The unknowns a stage leaves alone.  FREE_ALL: none; FREE_RIGID: all but delta_0 and t; FREE_NO_SHAPE: beta.
enum { FREE_ALL = 0, FREE_RIGID = 1, FREE_NO_SHAPE = 2 };
__device__ __forceinline__ bool is_frozen(int a, int mode) {
  return mode == FREE_RIGID ? (a >= 3 && a < UT) : (mode == FREE_NO_SHAPE ? (a >= UB && a < UT) : false);
}

// S.M = Exp(pose_mean_j), lanes 64..79; no barrier
template <int ROWS>
__device__ __forceinline__ void mean_pose(Lds<ROWS>& S, const float* pose_mean, int tid) {
  if (tid >= 64 && tid < 80) {
    const int j = tid - 64;
    const double w[3] = {(double)pose_mean[3 * j], (double)pose_mean[3 * j + 1], (double)pose_mean[3 * j + 2]};
    double E[9];
    exp_so3(w, E);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.M[9 * j + k] = E[k];
  }
}

// A caller's initial state into state 0, lanes 0..156; -> the lane read a value that is not finite.  No barrier.
template <int ROWS, class Side>
__device__ __forceinline__ bool read_init(Lds<ROWS>& S, const Side& sd, long long b, int tid) {
  if (!sd.init_pose || tid >= 157) return false;
  const float v = tid < 144 ? sd.init_pose[b * 144 + tid] : (tid < 154 ? sd.init_beta[b * 10 + tid - 144] : sd.init_transl[b * 3 + tid - 154]);
  if (tid < 144) S.R[0][tid] = (double)v;
  else if (tid < 154) S.beta[0][tid - 144] = (double)v;
  else S.t[0][tid - 154] = (double)v;
  return !isfinite(v);
}

// Whether the row is fitted: valid, four or more selected data points, no lane saw a bad value.  A barrier; the same on every lane.
template <class Side>
__device__ __forceinline__ bool row_fitted(const Side& sd, long long b, int nsel, bool bad) {
  const bool any_bad = __syncthreads_or(bad);
  return (sd.valid ? sd.valid[b] != 0.f : true) && nsel >= 4 && !any_bad;
}

// The outputs of a row that is not fitted: pose (I, M_1..M_15), zeros, NaN, no step.  A kernel adds those only it has.
template <int ROWS, class Side>
__device__ __forceinline__ void store_unfitted(const Lds<ROWS>& S, const Side& sd, long long b, int tid) {
  if (tid < 144) sd.pose[b * 144 + tid] = (float)S.M[tid];
  else if (tid < 154) sd.beta[b * 10 + tid - 144] = 0.f;
  else if (tid < 157) sd.transl[b * 3 + tid - 154] = 0.f;
  else if (tid == 157) sd.rmse[b] = __builtin_nanf("");
  else if (tid == 158) sd.steps[b] = 0;
}

// State 0 = the rest hand: R = M, beta = 0, t = 0.  Ends with a barrier.
template <int ROWS>
__device__ __forceinline__ void rest_state(Lds<ROWS>& S, int tid) {
  if (tid < 144) S.R[0][tid] = S.M[tid];
  else if (tid < 154) S.beta[0][tid - 144] = 0.0;
  else if (tid < 157) S.t[0][tid - 154] = 0.0;
  __syncthreads();
}

// One lane: the rigid alignment y ~ Rm (x - mx) + my as the global rotation and translation of state 0.  MANO turns about the
// wrist joint J_0 (S.Jr of the rest state): y ~ Rm (x - J_0) + J_0 + t.
template <int ROWS>
__device__ __forceinline__ void place_rigid(Lds<ROWS>& S, const double (*Rm)[3], const double* mx, const double* my) {
  for (int a = 0; a < 3; ++a) {
    const double e0 = mx[0] - S.Jr[0], e1 = mx[1] - S.Jr[1], e2 = mx[2] - S.Jr[2];
    S.t[0][a] = (my[a] - ((Rm[a][0] * e0 + Rm[a][1] * e1) + Rm[a][2] * e2)) - S.Jr[a];
    for (int c = 0; c < 3; ++c) S.R[0][3 * a + c] = Rm[a][c];
  }
}

// One stage of Levenberg-Marquardt on state 0: exactly n iterations with the unknowns of `mode` frozen, the damping from mu0.
// evaluate(s) leaves the cost of state s in S.c[0] and ends with a barrier; linearise(mu, mode) leaves g and the damped H of
// state 0 for solve().  c0: the cost of state 0, steps: the accepted steps so far, fresh: what evaluate() left in LDS belongs
// to state 0 -- after an accepted step it does, the candidate having become the current state, and the evaluation is not
// repeated (it would give the same bits).  The stage ends with state 0 evaluated (fresh).  The only data-dependent branch is
// accept / reject, uniform in the workgroup.
template <int ROWS, class Evaluate, class Linearise>
__device__ __forceinline__ void lm_stage(Lds<ROWS>& S, int n, int mode, double mu0, double& c0, int& steps, bool& fresh, int tid,
                                         Evaluate evaluate, Linearise linearise) {
  double mu = mu0;
  for (int it = 0; it < n; ++it) {
    if (!fresh) {
      evaluate(0);
      c0 = S.c[0];
    }
    linearise(mu, mode);
    const bool ok = solve(S, tid);
    if (tid < 16) {                              // the candidate: R_j Exp(delta_j), beta + delta_beta, t + delta_t
      double Rn[9];
      if (is_frozen(3 * tid, mode)) {            // a frozen rotation is copied, so that it keeps its bits
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn[k] = S.R[0][9 * tid + k];
      } else {
        const double w[3] = {S.d[3 * tid], S.d[3 * tid + 1], S.d[3 * tid + 2]};
        double X[9];
        exp_so3(w, X);
        mul_nn(S.R[0] + 9 * tid, X, Rn);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) S.R[1][9 * tid + k] = Rn[k];
    } else if (tid >= 64 && tid < 74) {
      S.beta[1][tid - 64] = S.beta[0][tid - 64] + S.d[UB + tid - 64];
    } else if (tid >= 74 && tid < 77) {
      S.t[1][tid - 74] = S.t[0][tid - 74] + S.d[UT + tid - 74];
    }
    __syncthreads();
    evaluate(1);
    const double c1 = S.c[0];
    const bool accept = ok && c1 < c0;           // strict, false for NaN and for +inf; the same on every lane
    fresh = accept;
    if (accept) {
      c0 = c1;
      if (tid < 144) S.R[0][tid] = S.R[1][tid];
      else if (tid < 154) S.beta[0][tid - 144] = S.beta[1][tid - 144];
      else if (tid < 157) S.t[0][tid - 154] = S.t[1][tid - 154];
      mu = fmax(mu / 3.0, MU_MIN);
      ++steps;
    } else {
      mu = fmin(5.0 * mu, MU_MAX);
    }
    __syncthreads();
  }
  if (!fresh) {
    evaluate(0);
    c0 = S.c[0];
    fresh = true;
  }
}

// sum_k w_k of the 21 joints or keypoints, in their order; one lane
template <int ROWS>
__device__ __forceinline__ double weight_sum(const Lds<ROWS>& S) {
  double sw = 0.0;
  for (int k = 0; k < 21; ++k) sw += S.w[k];
  return sw;
}

// The outputs of a fitted row from state 0, which evaluate() saw last: pose, beta, transl, steps and
// rmse = sqrt(S.c[1] / sum_w()) -- sum_w runs on lane 157 alone.  A kernel adds those only it has.
template <int ROWS, class Side, class SumW>
__device__ __forceinline__ void store_fitted(const Lds<ROWS>& S, const Side& sd, long long b, int steps, int tid, SumW sum_w) {
  if (tid < 144) sd.pose[b * 144 + tid] = (float)S.R[0][tid];
  else if (tid < 154) sd.beta[b * 10 + tid - 144] = (float)S.beta[0][tid - 144];
  else if (tid < 157) sd.transl[b * 3 + tid - 154] = (float)S.t[0][tid - 154];
  else if (tid == 157) sd.rmse[b] = (float)sqrt(S.c[1] / sum_w());
  else if (tid == 158) sd.steps[b] = steps;
}

// ---- host: the argument rules the three entries share --------------------------------------------------------------------------
inline bool non_negative(double v) { return isfinite(v) && v >= 0.0; }

template <class Cfg>                             // hands_fit_cfg and the fields hands_fit2d_cfg shares with it
bool fit_cfg_ok(const Cfg& c) {
  return c.iters >= 0 && non_negative(c.lambda_beta) && non_negative(c.lambda_pose) && non_negative(c.mu0);
}

// a side: every pointer of `required` is given, and the initial state is all three tensors or none
template <class Side>
bool fit_side_ok(const Side& d, std::initializer_list<const void*> required) {
  for (const void* p : required)
    if (!p) return false;
  const int given = (d.init_pose != nullptr) + (d.init_beta != nullptr) + (d.init_transl != nullptr);
  return given == 0 || given == 3;
}

}  // namespace
