// fit.hip -- MANO fitting on device (hands_mano_fit_f32 of include/hands_hip.h): a Levenberg-Marquardt fit of the 16 rotations
// of the full pose, the shape and a translation (61 unknowns) to 21 3-D joints.  DESIGN.md section 7 "MANO fitting" is the
// specification, tests/fit_ref.py its fp64 restatement; the reference has no fitter.
// One launch fits every hand of a call: grid (B, n_sides), one workgroup of four waves per hand, the hands independent.  fp32 in,
// fp64 arithmetic, one rounding per output.  A hand's problem lives in LDS (61 KB): the data rows of the Jacobian (63 x 61), the
// lower triangle of H = J^T J with the priors and the damping on its diagonal -- the Cholesky factor overwrites it, H is formed
// again in every iteration --, the two states (current, candidate) and what forward kinematics leaves of the current one.
// The work of an iteration spreads over the 256 lanes: the 3 x 3 blocks of the Jacobian (one item a lane and pass), the 1891
// entries of H (a dot product of 63 each), the column scaling and the trailing update of the Cholesky factorisation; the two
// triangular solves run in wave 0 with the right-hand side in registers and the pivot value passed by shuffle.
// H is formed on the vector pipe, not with v_mfma_f64: it is 117 k multiply-adds of an iteration whose length the 61
// dependent Cholesky columns (two barriers each) set, so the matrix pipe would shorten what is not the critical path, at the
// cost of a second operand layout of J.
// The iteration runs exactly `iters` times; the only data-dependent branch is accept / reject, uniform in the workgroup.  No
// atomics, no inter-workgroup synchronisation, no allocation; per-lane arrays are indexed by constants only (no scratch).
//
// hands_mano_fit2d_f32 fits the same unknowns to 21 2-D keypoints in pixels (DESIGN.md section 7 "MANO fitting to 2-D keypoints",
// tests/fit2d_ref.py): a second kernel of the same launch shape on the same device routines -- kinematics, shape_chain,
// rotation_block, shape_column, normal_equations, solve, Log / Exp; the LDS layout is one template on the number of data rows.
// Its own are the perspective projection with the row scales of the robust kernel (evaluate2d), the projection of each 3 x 3
// block in registers, so that only 42 data rows are stored (linearise2d), the start from 2-D alone (24 signed permutations, one
// lane a candidate), the rigid stage before the full one with its frozen unknowns (identity rows in H: the factorisation skips
// nothing and is exact), the depth guard (+inf cost) and the outputs j3d / j2d, which are in LDS at the end.  53 KB of LDS.
//
// Log / Exp, the 3 x 3 products, the tree, shape_chain, solve and the LDS state are in fit_device.h, which fit_verts.hip (the fit
// to 778 vertices) shares; kinematics stays here: it evaluates the five tips from the tip pack, which that fit does not carry.
// The driver is there too: the mean pose, the read of a caller's state, the `fitted` rule, the rest state, the placement of a
// rigid alignment, the Levenberg-Marquardt stage (lm_stage) and the stores of the outputs every fit has.  A kernel here reads its
// target, makes its start, hands lm_stage its evaluate and linearise and stores what only it has.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"
#include "fit_device.h"

namespace {

// Forward kinematics, the five tips and the pose prior's Log(Mref_j^T R_j) of state s.  Every lane of the workgroup calls it.
template <int ROWS>
__device__ __forceinline__ void kinematics(Lds<ROWS>& S, const hands_mano_fit_consts& C, int s, const double* Mref, int tid) {
  const double* R = S.R[s];
  const double* be = S.beta[s];
  if (tid < 48) {                                // rest joints of this shape
    double a = (double)C.J_template[tid];
#pragma unroll
    for (int l = 0; l < 10; ++l) a += (double)C.J_shapedirs[tid * 10 + l] * be[l];
    S.Jr[tid] = a;
  } else if (tid >= 64 && tid < 79) {            // the tips before skinning: template, shape and pose blend shapes
    const int mc = tid - 64;
    double a = (double)C.tip_v_template[mc];
#pragma unroll
    for (int l = 0; l < 10; ++l) a += (double)C.tip_shapedirs[mc * 10 + l] * be[l];
#pragma unroll 5
    for (int f = 0; f < 135; ++f) a += (R[9 + f] - ((f % 9) % 4 == 0 ? 1.0 : 0.0)) * (double)C.tip_posedirs[f * 15 + mc];
    S.vp[mc] = a;
  } else if (tid >= 128 && tid < 143) {          // the pose prior: Log(M_j^T R_j), j = 1..15
    const int j = tid - 127;
    double D[9], w[3];
    mul_tn(Mref + 9 * j, R + 9 * j, D);
    log_so3(D, w);
#pragma unroll
    for (int c = 0; c < 3; ++c) S.lg[3 * (j - 1) + c] = w[c];
  }
  __syncthreads();
  if (tid < 5) {                                 // a finger's chain from the wrist
    double Qa[9], pa[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Qa[i] = R[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) pa[c] = S.Jr[c];
#pragma unroll
    for (int n = 0; n < 3; ++n) {
      const int i = 1 + 3 * tid + n, a = n == 0 ? 0 : i - 1;
      double Qi[9], pi[3];
      mul_nn(Qa, R + 9 * i, Qi);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double e0 = S.Jr[3 * i] - S.Jr[3 * a], e1 = S.Jr[3 * i + 1] - S.Jr[3 * a + 1], e2 = S.Jr[3 * i + 2] - S.Jr[3 * a + 2];
        pi[c] = pa[c] + ((Qa[3 * c] * e0 + Qa[3 * c + 1] * e1) + Qa[3 * c + 2] * e2);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) S.Q[9 * i + k] = Qa[k] = Qi[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) S.p[3 * i + c] = pa[c] = pi[c];
    }
  } else if (tid == 5) {
#pragma unroll
    for (int k = 0; k < 9; ++k) S.Q[k] = R[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) S.p[c] = S.Jr[c];
  }
  __syncthreads();
  for (int it = tid; it < 240 + 45; it += NT) {
    if (it < 240) {                              // x[m][i]: tip m as joint i carries it
      const int m = it / 48, i = (it % 48) / 3, c = it % 3;
      const double* q = S.Q + 9 * i + 3 * c;
      S.x[it] = S.p[3 * i + c] + ((q[0] * (S.vp[3 * m] - S.Jr[3 * i]) + q[1] * (S.vp[3 * m + 1] - S.Jr[3 * i + 1])) +
                                  q[2] * (S.vp[3 * m + 2] - S.Jr[3 * i + 2]));
    } else {                                     // A[m] = sum_i W_mi Q_i
      const int m = (it - 240) / 9, ab = (it - 240) % 9;
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) a += (double)C.tip_lbs_weights[m * 16 + i] * S.Q[9 * i + ab];
      S.A[it - 240] = a;
    }
  }
  __syncthreads();
  if (tid < 15) {
    const int m = tid / 3, c = tid % 3;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) a += (double)C.tip_lbs_weights[m * 16 + i] * S.x[m * 48 + 3 * i + c];
    S.joints[48 + tid] = a;
  } else if (tid >= 64 && tid < 112) {
    S.joints[tid - 64] = S.p[tid - 64];
  }
  __syncthreads();
}

// The residual and the cost of the 3-D fit at the state kinematics() saw last (state s).
__device__ __forceinline__ void evaluate(Lds<NR>& S, const hands_mano_fit_consts& C, int s, double lb, double lp, int tid) {
  kinematics(S, C, s, S.M, tid);
  const double* be = S.beta[s];
  if (tid < 64) {                                // residual and cost: wave 0
    double r = 0.0;
    if (tid < NR) {
      const int k = tid / 3;
      r = S.w[k] > 0.0 ? S.sw[k] * ((S.joints[tid] + S.t[s][tid % 3]) - S.y[tid]) : 0.0;      // selected, not multiplied
      S.r[tid] = r;
    }
    double data = r * r;
    double all = data + (tid < 10 ? lb * (be[tid] * be[tid]) : 0.0) + (tid < 45 ? lp * (S.lg[tid] * S.lg[tid]) : 0.0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      data += __shfl_xor(data, o);
      all += __shfl_xor(all, o);
    }
    if (tid == 0) {
      S.c[0] = all;
      S.c[1] = data;
    }
  }
  __syncthreads();
}


// B (3 x 3) = d point k / d delta_j (k < 16 a joint, else tip k - 16) at the state kinematics() saw last (state s)
template <int ROWS>
__device__ __forceinline__ void rotation_block(const Lds<ROWS>& S, const hands_mano_fit_consts& C, int s, int k, int j, double* B) {
  const double* Qj = S.Q + 9 * j;
  double v[3] = {0.0, 0.0, 0.0};
  bool moves = true;
  if (k < 16) {
    moves = k != j && at_or_below(j, k);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = S.p[3 * k + c] - S.p[3 * j + c];
  } else {
    const int m = k - 16;
#pragma unroll 1
    for (int i = 0; i < 16; ++i)
      if (at_or_below(j, i)) {
        const double wi = (double)C.tip_lbs_weights[m * 16 + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += wi * (S.x[m * 48 + 3 * i + c] - S.p[3 * j + c]);
      }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {                  // column c of -[v]x Q_j = (column c of Q_j) x v
    const double q0 = Qj[c], q1 = Qj[3 + c], q2 = Qj[6 + c];
    B[c] = moves ? q1 * v[2] - q2 * v[1] : 0.0;
    B[3 + c] = moves ? q2 * v[0] - q0 * v[2] : 0.0;
    B[6 + c] = moves ? q0 * v[1] - q1 * v[0] : 0.0;
  }
  if (k >= 16 && j >= 1) {                       // the pose blend shapes: (sum_i W_i Q_i) posedirs_tip vec(R_j [e_a]x)
    const int m = k - 16;
    const double* Rj = S.R[s] + 9 * j;
    const float* pd = C.tip_posedirs + 9 * (j - 1) * 15 + 3 * m;
    const double* Am = S.A + 9 * m;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double dR[9];
#pragma unroll
      for (int r = 0; r < 3; ++r) {              // R [e_a]x: columns (0, R2, -R1), (-R2, 0, R0), (R1, -R0, 0)
        dR[3 * r] = a == 0 ? 0.0 : (a == 1 ? -Rj[3 * r + 2] : Rj[3 * r + 1]);
        dR[3 * r + 1] = a == 0 ? Rj[3 * r + 2] : (a == 1 ? 0.0 : -Rj[3 * r]);
        dR[3 * r + 2] = a == 0 ? -Rj[3 * r + 1] : (a == 1 ? Rj[3 * r] : 0.0);
      }
      double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int f = 0; f < 9; ++f)
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] += dR[f] * (double)pd[f * 15 + c];
#pragma unroll
      for (int r = 0; r < 3; ++r) B[3 * r + a] += (Am[3 * r] * u[0] + Am[3 * r + 1] * u[1]) + Am[3 * r + 2] * u[2];
    }
  }
}

// v (3) = d point k / d beta_l, after shape_chain()
template <int ROWS>
__device__ __forceinline__ void shape_column(const Lds<ROWS>& S, const hands_mano_fit_consts& C, int k, int l, double* v) {
  if (k < 16) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = S.dp[(3 * k + c) * 10 + l];
  } else {
    const int m = k - 16;
    v[0] = v[1] = v[2] = 0.0;
#pragma unroll 1
    for (int i = 0; i < 16; ++i) {
      const double wi = (double)C.tip_lbs_weights[m * 16 + i];
      const double e0 = (double)C.tip_shapedirs[(3 * m) * 10 + l] - (double)C.J_shapedirs[(3 * i) * 10 + l];
      const double e1 = (double)C.tip_shapedirs[(3 * m + 1) * 10 + l] - (double)C.J_shapedirs[(3 * i + 1) * 10 + l];
      const double e2 = (double)C.tip_shapedirs[(3 * m + 2) * 10 + l] - (double)C.J_shapedirs[(3 * i + 2) * 10 + l];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double* q = S.Q + 9 * i + 3 * c;
        v[c] += wi * (((q[0] * e0 + q[1] * e1) + q[2] * e2) + S.dp[(3 * i + c) * 10 + l]);
      }
    }
  }
}

// g = J^T r and the damped H from the data rows in S.J, the priors included (bbar: the shape prior's reference, NULL for 0).  A
// frozen unknown has a zero row and column, diagonal 1 (before the damping) and g = 0: its step is exactly 0 and the Cholesky
// factor of the other unknowns is what it would be without it.
template <int ROWS>
__device__ void normal_equations(Lds<ROWS>& S, int s, double lb, double lp, double mu, const double* bbar, int mode, int tid) {
  if (tid < NU) {                                // g = J^T r, the priors with d Log / d delta = I
    double a = 0.0;
#pragma unroll 3
    for (int r = 0; r < ROWS; ++r) a += S.J[r * NU + tid] * S.r[r];
    if (tid >= 3 && tid < UB) a += lp * S.lg[tid - 3];
    if (tid >= UB && tid < UT) a += lb * (bbar ? S.beta[s][tid - UB] - bbar[tid - UB] : S.beta[s][tid - UB]);
    S.g[tid] = is_frozen(tid, mode) ? 0.0 : a;
  }
  for (int e = tid; e < HP; e += NT) {           // H + mu diag H, lower triangle
    int a = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
    if (a * (a + 1) / 2 > e) --a;
    if ((a + 1) * (a + 2) / 2 <= e) ++a;
    const int b = e - a * (a + 1) / 2;
    double h = 0.0;
#pragma unroll 3
    for (int r = 0; r < ROWS; ++r) h += S.J[r * NU + a] * S.J[r * NU + b];
    if (a == b) {
      if (a >= 3 && a < UB) h += lp;
      if (a >= UB && a < UT) h += lb;
    }
    if (is_frozen(a, mode) || is_frozen(b, mode)) h = a == b ? 1.0 : 0.0;
    if (a == b) h += mu * h;
    S.H[e] = h;
  }
  __syncthreads();
}

// The data rows of the 3-D fit's Jacobian at the state evaluate() saw last (state s), g = J^T r and the damped H.
__device__ void linearise(Lds<NR>& S, const hands_mano_fit_consts& C, int s, double lb, double lp, double mu, int tid) {
  shape_chain(S, C, tid);
  for (int it = tid; it < 336 + 210 + NR; it += NT) {
    if (it < 336) {                              // d point k / d delta_j, a 3 x 3 block
      const int k = it / 16, j = it % 16;
      double B[9];
      rotation_block(S, C, s, k, j, B);
      const bool on = S.w[k] > 0.0;
      const double sw = S.sw[k];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) S.J[(3 * k + r) * NU + 3 * j + c] = on ? sw * B[3 * r + c] : 0.0;
    } else if (it < 336 + 210) {                 // d point k / d beta_l
      const int k = (it - 336) / 10, l = (it - 336) % 10;
      double v[3];
      shape_column(S, C, k, l, v);
      const bool on = S.w[k] > 0.0;
      const double sw = S.sw[k];
#pragma unroll
      for (int c = 0; c < 3; ++c) S.J[(3 * k + c) * NU + UB + l] = on ? sw * v[c] : 0.0;
    } else {                                     // d / d t = I
      const int row = it - (336 + 210), k = row / 3, c = row % 3;
      const bool on = S.w[k] > 0.0;
      const double sw = S.sw[k];
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) S.J[row * NU + UT + cc] = (on && cc == c) ? sw : 0.0;
    }
  }
  __syncthreads();
  normal_equations(S, s, lb, lp, mu, nullptr, FREE_ALL, tid);
}


struct Sides {
  hands_mano_fit_side s[2];
};

__global__ void __launch_bounds__(NT) mano_fit_kernel(Sides sides, hands_fit_cfg cfg) {
  __shared__ Lds<NR> S;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const hands_mano_fit_side& sd = sides.s[blockIdx.y];
  const hands_mano_fit_consts& C = sd.consts;
  const double lb = cfg.lambda_beta, lp = cfg.lambda_pose;

  // the target: a joint of weight 0 (or of a weight that is no number) is never read
  bool sel = false, bad = false;
  if (tid < 21) {
    const double w = sd.weights ? (double)sd.weights[b * 21 + tid] : 1.0;
    sel = w > 0.0;
    S.w[tid] = sel ? w : 0.0;
    S.sw[tid] = sel ? sqrt(w) : 0.0;
    bad = sel && !isfinite(w);                   // a selected weight of +inf: the row is not fitted
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = sel ? sd.joints[(b * 21 + tid) * 3 + c] : 0.f;
      bad = bad || !isfinite(v);
      S.y[3 * tid + c] = (double)v;
    }
  }
  mean_pose(S, C.pose_mean, tid);
  bad = read_init(S, sd, b, tid) || bad;         // a caller's initial state
  const int nsel = __syncthreads_count(sel);
  if (!row_fitted(sd, b, nsel, bad)) {           // the whole workgroup leaves
    store_unfitted(S, sd, b, tid);
    return;
  }

  if (!sd.init_pose) {                           // the rest hand, aligned rigidly to the target
    rest_state(S, tid);
    evaluate(S, C, 0, lb, lp, tid);
    if (tid == 0) {
      double sw = 0.0, mx[3] = {0.0, 0.0, 0.0}, my[3] = {0.0, 0.0, 0.0};
      for (int k = 0; k < 21; ++k)
        if (S.w[k] > 0.0) {
          sw += S.w[k];
          for (int c = 0; c < 3; ++c) {
            mx[c] += S.w[k] * S.joints[3 * k + c];
            my[c] += S.w[k] * S.y[3 * k + c];
          }
        }
      for (int c = 0; c < 3; ++c) { mx[c] /= sw; my[c] /= sw; }
      double K[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, var1 = 0.0;
      for (int k = 0; k < 21; ++k)
        if (S.w[k] > 0.0)
          for (int a = 0; a < 3; ++a) {
            const double x1 = S.joints[3 * k + a] - mx[a];
            var1 += S.w[k] * x1 * x1;
            for (int c = 0; c < 3; ++c) K[a][c] += S.w[k] * x1 * (S.y[3 * k + c] - my[c]);
          }
      double Rm[3][3], scale;
      procrustes_solve(K, var1, Rm, &scale);     // the scale is not used: the alignment is rigid
      place_rigid(S, Rm, mx, my);
    }
  }
  __syncthreads();

  double c0 = 0.0;
  int steps = 0;
  bool fresh = false;
  lm_stage(S, cfg.iters, FREE_ALL, cfg.mu0, c0, steps, fresh, tid, [&](int s) { evaluate(S, C, s, lb, lp, tid); },
           [&](double mu, int) { linearise(S, C, 0, lb, lp, mu, tid); });
  store_fitted(S, sd, b, steps, tid, [&] { return weight_sum(S); });
}

// ---- the fit to 2-D keypoints (hands_mano_fit2d_f32; DESIGN.md section 7 "MANO fitting to 2-D keypoints") ----------------------
constexpr int NR2 = 42;                          // data rows: 21 keypoints x 2

struct Cam {                                     // what the 2-D fit keeps beside Lds<NR2>
  double K[6];                                   // rows 0 and 1 of the intrinsics
  double Mbar[144], bbar[10];                    // the references of the priors
  double rw[21];                                 // sqrt(w_k); Lds::sw holds the row scale s_k of the state evaluated last
  double X[63], uv[42], P[126];                  // of that state: camera points, their projection, d pi / d X (2 x 3 a joint)
  double sig2, zmin;
};

// Projection, residual, row scales and cost of state s; +inf where a weighted joint is not in front of z_min.
__device__ __forceinline__ void evaluate2d(Lds<NR2>& S, Cam& E, const hands_mano_fit_consts& C, int s, double lb, double lp, int tid) {
  kinematics(S, C, s, E.Mbar, tid);
  if (tid < 64) {                                // wave 0
    double rho = 0.0, we2 = 0.0;
    int shallow = 0;
    if (tid < 21) {
      const double x = S.joints[3 * tid] + S.t[s][0], y = S.joints[3 * tid + 1] + S.t[s][1], z = S.joints[3 * tid + 2] + S.t[s][2];
      const double px = E.K[0] * x + E.K[1] * y, py = E.K[3] * x + E.K[4] * y;
      const double u = px / z + E.K[2], v = py / z + E.K[5];
      E.X[3 * tid] = x; E.X[3 * tid + 1] = y; E.X[3 * tid + 2] = z;
      E.uv[2 * tid] = u; E.uv[2 * tid + 1] = v;
      double sk = 0.0, e0 = 0.0, e1 = 0.0;
      if (S.w[tid] > 0.0) {                      // selected, not multiplied
        shallow = !(z > E.zmin);
        e0 = u - S.y[2 * tid];
        e1 = v - S.y[2 * tid + 1];
        const double e2 = e0 * e0 + e1 * e1;
        const double f = E.sig2 > 0.0 ? E.sig2 / (E.sig2 + e2) : 1.0;      // Geman-McClure
        we2 = S.w[tid] * e2;
        rho = we2 * f;
        sk = E.rw[tid] * f;
        double* P = E.P + 6 * tid;
        P[0] = E.K[0] / z; P[1] = E.K[1] / z; P[2] = -px / (z * z);
        P[3] = E.K[3] / z; P[4] = E.K[4] / z; P[5] = -py / (z * z);
      }
      S.sw[tid] = sk;
      S.r[2 * tid] = sk * e0;
      S.r[2 * tid + 1] = sk * e1;
    }
    const double db = tid < 10 ? S.beta[s][tid] - E.bbar[tid] : 0.0;
    double all = rho + (tid < 10 ? lb * (db * db) : 0.0) + (tid < 45 ? lp * (S.lg[tid] * S.lg[tid]) : 0.0);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      we2 += __shfl_xor(we2, o);
      all += __shfl_xor(all, o);
      shallow |= __shfl_xor(shallow, o);
    }
    if (tid == 0) {
      S.c[0] = shallow ? (double)INFINITY : all;
      S.c[1] = we2;
    }
  }
  __syncthreads();
}

// The 42 data rows s_k P_k D_k at the state evaluate2d() saw last (state s), g and the damped H with the stage's frozen unknowns.
__device__ void linearise2d(Lds<NR2>& S, const Cam& E, const hands_mano_fit_consts& C, int s, double lb, double lp, double mu,
                            int mode, int tid) {
  shape_chain(S, C, tid);
  for (int it = tid; it < 336 + 210 + 21; it += NT) {
    if (it < 336) {                              // the 3 x 3 block, projected in registers
      const int k = it / 16, j = it % 16;
      double B[9];
      rotation_block(S, C, s, k, j, B);
      const bool on = S.w[k] > 0.0;
      const double sk = S.sw[k];
      const double* P = E.P + 6 * k;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
          S.J[(2 * k + r) * NU + 3 * j + c] = on ? sk * ((P[3 * r] * B[c] + P[3 * r + 1] * B[3 + c]) + P[3 * r + 2] * B[6 + c]) : 0.0;
    } else if (it < 336 + 210) {
      const int k = (it - 336) / 10, l = (it - 336) % 10;
      double v[3];
      shape_column(S, C, k, l, v);
      const bool on = S.w[k] > 0.0;
      const double sk = S.sw[k];
      const double* P = E.P + 6 * k;
#pragma unroll
      for (int r = 0; r < 2; ++r) S.J[(2 * k + r) * NU + UB + l] = on ? sk * ((P[3 * r] * v[0] + P[3 * r + 1] * v[1]) + P[3 * r + 2] * v[2]) : 0.0;
    } else {                                     // d X / d t = I
      const int k = it - (336 + 210);
      const bool on = S.w[k] > 0.0;
      const double sk = S.sw[k];
      const double* P = E.P + 6 * k;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) S.J[(2 * k + r) * NU + UT + c] = on ? sk * P[3 * r + c] : 0.0;
    }
  }
  __syncthreads();
  normal_equations(S, s, lb, lp, mu, E.bbar, mode, tid);
}

struct Sides2 {
  hands_mano_fit2d_side s[2];
};

__global__ void __launch_bounds__(NT) mano_fit2d_kernel(Sides2 sides, const float* __restrict__ Kin, hands_fit2d_cfg cfg) {
  __shared__ Lds<NR2> S;
  __shared__ Cam E;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const hands_mano_fit2d_side& sd = sides.s[blockIdx.y];
  const hands_mano_fit_consts& C = sd.consts;
  const double lb = cfg.lambda_beta, lp = cfg.lambda_pose;

  // the target: a keypoint of weight 0 (or of a weight that is no number) is never read
  bool sel = false, bad = false;
  if (tid < 21) {
    const double w = sd.weights ? (double)sd.weights[b * 21 + tid] : 1.0;
    sel = w > 0.0;
    S.w[tid] = sel ? w : 0.0;
    E.rw[tid] = sel ? sqrt(w) : 0.0;
    bad = sel && !isfinite(w);                   // a selected weight of +inf: the row is not fitted
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const float v = sel ? sd.kp2d[(b * 21 + tid) * 2 + c] : 0.f;
      bad = bad || !isfinite(v);
      S.y[2 * tid + c] = (double)v;
    }
  } else if (tid >= 32 && tid < 38) {            // K: rows 0 and 1
    const float v = Kin[b * 9 + tid - 32];
    bad = bad || !isfinite(v) || ((tid == 32 || tid == 36) && !(v > 0.f));
    E.K[tid - 32] = (double)v;
  } else if (tid == 38) {
    E.sig2 = cfg.robust_sigma * cfg.robust_sigma;
    E.zmin = cfg.z_min;
  }
  // mean_pose, read_init and row_fitted of fit_device.h, written out: through the three calls this kernel was 1.5 to 2.9 % slower
  // (docs/EXPERIMENTS.md), so the text stays here until that is understood
  if (tid >= 64 && tid < 80) {
    const int j = tid - 64;
    const double w[3] = {(double)C.pose_mean[3 * j], (double)C.pose_mean[3 * j + 1], (double)C.pose_mean[3 * j + 2]};
    double M[9];
    exp_so3(w, M);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.M[9 * j + k] = M[k];
  }
  if (sd.init_pose && tid < 157) {               // a caller's initial state
    const float v = tid < 144 ? sd.init_pose[b * 144 + tid] : (tid < 154 ? sd.init_beta[b * 10 + tid - 144] : sd.init_transl[b * 3 + tid - 154]);
    bad = bad || !isfinite(v);
    if (tid < 144) S.R[0][tid] = (double)v;
    else if (tid < 154) S.beta[0][tid - 144] = (double)v;
    else S.t[0][tid - 154] = (double)v;
  }
  const int nsel = __syncthreads_count(sel);
  const bool any_bad = __syncthreads_or(bad);
  bool fitted = (sd.valid ? sd.valid[b] != 0.f : true) && nsel >= 4 && !any_bad;
  int start = -1;

  if (fitted) {                                  // uniform in the workgroup, as every branch on `fitted` below
    const bool own = sd.init_pose && cfg.prior_to_init;                 // the priors pull towards the caller's state
    if (tid < 144) E.Mbar[tid] = own ? S.R[0][tid] : S.M[tid];
    else if (tid < 154) E.bbar[tid - 144] = own ? S.beta[0][tid - 144] : 0.0;
    if (!sd.init_pose) {                         // the rest hand under the best of the 24 axis-aligned rotations, weak perspective
      rest_state(S, tid);
      kinematics(S, C, 0, E.Mbar, tid);
      if (tid < 21) {                            // n_k = K[:2,:2]^-1 (y_k - K[:2,2]), kept in E.uv
        const double det = E.K[0] * E.K[4] - E.K[1] * E.K[3];
        const double d0 = S.y[2 * tid] - E.K[2], d1 = S.y[2 * tid + 1] - E.K[5];
        E.uv[2 * tid] = (E.K[4] * d0 - E.K[1] * d1) / det;
        E.uv[2 * tid + 1] = (E.K[0] * d1 - E.K[3] * d0) / det;
      }
      __syncthreads();
      if (tid < 64) {                            // wave 0: lane c < 24 scores candidate c
        const int c = tid < 24 ? tid : 0, pm = c >> 2;
        const int p0 = pm >> 1, p1 = pm == 0 ? 1 : (pm == 1 ? 2 : (pm == 2 ? 0 : (pm == 3 ? 2 : (pm == 4 ? 0 : 1))));
        const int p2 = 3 - p0 - p1;
        const double s0 = (c & 2) ? -1.0 : 1.0, s1 = (c & 1) ? -1.0 : 1.0;
        const double par = (pm == 0 || pm == 3 || pm == 4) ? 1.0 : -1.0;
        double sw = 0.0, a0 = 0.0, a1 = 0.0, n0 = 0.0, n1 = 0.0;
        for (int k = 0; k < 21; ++k)
          if (S.w[k] > 0.0) {
            const double w = S.w[k];
            sw += w;
            a0 += w * (s0 * (S.joints[3 * k + p0] - S.Jr[p0]));
            a1 += w * (s1 * (S.joints[3 * k + p1] - S.Jr[p1]));
            n0 += w * E.uv[2 * k];
            n1 += w * E.uv[2 * k + 1];
          }
        a0 /= sw; a1 /= sw; n0 /= sw; n1 /= sw;
        double den = 0.0, num = 0.0;
        for (int k = 0; k < 21; ++k)
          if (S.w[k] > 0.0) {
            const double da0 = s0 * (S.joints[3 * k + p0] - S.Jr[p0]) - a0, da1 = s1 * (S.joints[3 * k + p1] - S.Jr[p1]) - a1;
            den += S.w[k] * (da0 * da0 + da1 * da1);
            num += S.w[k] * (da0 * (E.uv[2 * k] - n0) + da1 * (E.uv[2 * k + 1] - n1));
          }
        const double sc = num / den;
        double eps = 0.0;
        for (int k = 0; k < 21; ++k)
          if (S.w[k] > 0.0) {
            const double da0 = s0 * (S.joints[3 * k + p0] - S.Jr[p0]) - a0, da1 = s1 * (S.joints[3 * k + p1] - S.Jr[p1]) - a1;
            const double q0 = sc * da0 - (E.uv[2 * k] - n0), q1 = sc * da1 - (E.uv[2 * k + 1] - n1);
            eps += S.w[k] * (q0 * q0 + q1 * q1);
          }
        const bool qual = tid < 24 && den > 0.0 && sc > 0.0 && eps < (double)INFINITY;
        int best = -1;
        double best_eps = 0.0;
        for (int k = 0; k < 24; ++k) {           // the smallest, ties to the lowest index; the same on every lane
          const double ek = __shfl(eps, k);
          const int qk = __shfl((int)qual, k);
          if (qk && (best < 0 || ek < best_eps)) {
            best = k;
            best_eps = ek;
          }
        }
        if (tid == best) {                       // at most one lane
          double G[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            if (q == p0) G[q] = s0;
            if (q == p1) G[3 + q] = s1;
            if (q == p2) G[6 + q] = par * s0 * s1;
          }
#pragma unroll
          for (int q = 0; q < 9; ++q) S.R[0][q] = G[q];
          S.t[0][0] = (n0 - sc * a0) / sc - S.Jr[0];
          S.t[0][1] = (n1 - sc * a1) / sc - S.Jr[1];
          S.t[0][2] = 1.0 / sc - S.Jr[2];
        }
        if (tid == 0) S.d[0] = (double)best;
      }
      __syncthreads();
      start = (int)S.d[0];
      fitted = start >= 0;
      __syncthreads();                           // S.d is written again in the iteration
    }
  }
  __syncthreads();                               // E.Mbar, E.bbar and the start state are complete

  double c0 = 0.0;
  int steps = 0;
  bool fresh = true;                             // the first evaluation is the depth guard's
  if (fitted) {
    evaluate2d(S, E, C, 0, lb, lp, tid);
    c0 = S.c[0];
    fitted = c0 < (double)INFINITY;              // the depth guard on the initial state
  }
  if (!fitted) {                                 // the whole workgroup leaves; NaN in j3d and j2d
    const float nanf_ = __builtin_nanf("");
    store_unfitted(S, sd, b, tid);
    if (tid == 159) sd.start[b] = -1;
    if (tid < 63) sd.j3d[b * 63 + tid] = nanf_;
    else if (tid >= 64 && tid < 106) sd.j2d[b * 42 + tid - 64] = nanf_;
    return;
  }

  // the rigid stage, then the full one; the depth guard (+inf cost) keeps a candidate from being accepted
  for (int stage = 0; stage < 2; ++stage)
    lm_stage(S, stage == 0 ? cfg.iters_rigid : cfg.iters, stage == 0 ? FREE_RIGID : (cfg.fit_shape ? FREE_ALL : FREE_NO_SHAPE),
             cfg.mu0, c0, steps, fresh, tid, [&](int s) { evaluate2d(S, E, C, s, lb, lp, tid); },
             [&](double mu, int mode) { linearise2d(S, E, C, 0, lb, lp, mu, mode, tid); });

  store_fitted(S, sd, b, steps, tid, [&] { return weight_sum(S); });
  if (tid == 159) sd.start[b] = start;
  if (tid < 63) sd.j3d[b * 63 + tid] = (float)E.X[tid];
  else if (tid >= 64 && tid < 106) sd.j2d[b * 42 + tid - 64] = (float)E.uv[tid - 64];
}

bool consts_given(const hands_mano_fit_consts& c) {
  return c.pose_mean && c.J_template && c.J_shapedirs && c.tip_v_template && c.tip_shapedirs && c.tip_lbs_weights && c.tip_posedirs;
}

}  // namespace

extern "C" int hands_mano_fit_f32(const hands_mano_fit_side* sides, int n_sides, const hands_fit_cfg* cfg, int B,
                                  hands_stream_t stream) {
  if (!sides || !cfg || n_sides < 1 || n_sides > 2 || B <= 0 || !fit_cfg_ok(*cfg)) return HANDS_EINVAL;
  Sides k;
  for (int i = 0; i < 2; ++i) {
    const hands_mano_fit_side& d = k.s[i] = sides[i < n_sides ? i : 0];
    if (!consts_given(d.consts) || !fit_side_ok(d, {d.joints, d.pose, d.beta, d.transl, d.rmse, d.steps})) return HANDS_EINVAL;
  }
  hipLaunchKernelGGL(mano_fit_kernel, dim3(B, n_sides), dim3(NT), 0, (hipStream_t)stream, k, *cfg);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_mano_fit2d_f32(const hands_mano_fit2d_side* sides, int n_sides, const float* K, const hands_fit2d_cfg* cfg,
                                    int B, hands_stream_t stream) {
  if (!sides || !cfg || !K || n_sides < 1 || n_sides > 2 || B <= 0 || !fit_cfg_ok(*cfg) || cfg->iters_rigid < 0) return HANDS_EINVAL;
  if (!non_negative(cfg->robust_sigma) || !isfinite(cfg->z_min) || !(cfg->z_min > 0.0)) return HANDS_EINVAL;
  Sides2 k;
  for (int i = 0; i < 2; ++i) {
    const hands_mano_fit2d_side& d = k.s[i] = sides[i < n_sides ? i : 0];
    if (!consts_given(d.consts) || !fit_side_ok(d, {d.kp2d, d.pose, d.beta, d.transl, d.rmse, d.steps, d.start, d.j3d, d.j2d}))
      return HANDS_EINVAL;
  }
  hipLaunchKernelGGL(mano_fit2d_kernel, dim3(B, n_sides), dim3(NT), 0, (hipStream_t)stream, k, K, *cfg);
  HANDS_LAUNCH_CHECK();
}
