// fit_verts.hip -- MANO fitting to 778 vertices (hands_mano_fit_verts_f32 of include/hands_hip.h): the Levenberg-Marquardt fit of
// fit.hip -- 16 rotations of the full pose, the shape, a translation: 61 unknowns -- with the 778 vertices of a mesh in MANO
// topology as the data, 2334 rows.  DESIGN.md section 7 "MANO fitting to 778 vertices" is the specification,
// tests/fit_verts_ref.py its fp64 restatement.  Launch as the siblings: grid (B, n_sides), one workgroup of four waves per hand,
// fp32 in, fp64 arithmetic, one rounding per output, exactly `iters` iterations, no atomics, no allocation.
//
// The Jacobian (2334 x 61 doubles, 1.1 MB) cannot live in LDS, so an iteration streams the vertices in 49 tiles of 16 (the last
// has 6 absent vertices: zero rows).  Sixteen lanes share a vertex, lane j of them owns joint j for the whole walk: it holds
// Q_j, p_j, J_j and R_j - I in registers, reads the 27 pose blend shapes of its joint (once, for the vertex and for its block of
// the Jacobian), forms x_{n,j} and, after three butterflies over the sixteen lanes (v~_n, v_n, sum_i W_i Q_i), its 3 x 3 block
// d v_n / d delta_j and one more column: lanes 0..9 a shape column, 10..12 the translation, 13 the residual, 14 and 15 zeros.
// A tile is 48 rows x 64 columns in LDS; the four waves then add the lower-triangle 16 x 16 blocks of its Gram matrix with
// v_mfma_f64_16x16x4_f64, ten blocks, each owned by one wave for the whole walk, tiles and rows in ascending order.  Both operands
// of a block are 16 consecutive doubles of a tile row, so one LDS read serves J^T and J.  The Gram matrix holds H's data part and
// g = J^T r (row 61); priors and damping go on as in fit.hip and solve() of fit_device.h factors.  A candidate costs one walk without
// the Jacobian; after an accepted step that evaluation is kept.  The set-up of the state and the stores the three fits share are
// the driver routines of fit_device.h; the iteration is this kernel's own copy of lm_stage with FREE_ALL: called through
// lm_stage the same arithmetic was 5 % slower (docs/EXPERIMENTS.md), so the text stays here until that is understood.
// Every sum has an order the code fixes: the butterflies (DPP row moves) add the same pairs on every lane, a vertex slot adds its
// 49 tiles in ascending order, one lane adds the 16 slots.  kinematics() of fit.hip is not used: it evaluates the tips from the tip pack;
// here joint_state() leaves the joints and the walk delivers the five tip vertices.  62 KB of LDS.
// State, block_sum, joint_state, row_move, sum16 and put_block are fit_mesh_device.h's: fit_surf.hip needs them too.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"
#include "fit_device.h"
#include "fit_mesh_device.h"

namespace {

constexpr int NV = 778;                          // vertices
constexpr int TV = 16, NTILE = (NV + TV - 1) / TV;       // vertices of a tile; 49 tiles
constexpr int TR = 3 * TV, TC = 64;              // rows and columns of a tile: 61 unknowns, the residual, two zero columns
constexpr int NVP = NTILE * TV;                  // 784
constexpr int RED = 2400;                        // where the reduction buffer starts in the tile, behind the 2334 rest coordinates

struct Mesh {                                    // what this fit keeps beside the state
  double T[TR * TC];                             // the tile; before the iteration the rest vertices and the reduction buffer
  double D[480];                                 // d p_i / d beta - Q_i S_i, (16, 3, 10)
  double part[TV];                               // the data cost per vertex slot
  double sumw;
  float w[NVP];                                  // w_n where it is > 0, else 0
};

enum { EVAL = 0, JAC = 1, REST = 2 };

__device__ __forceinline__ int tip_of(int n) {           // the tip slot of vertex n or -1
  return n == 744 ? 0 : (n == 320 ? 1 : (n == 443 ? 2 : (n == 554 ? 3 : (n == 671 ? 4 : -1))));
}

// One walk over the vertices at the state joint_state() saw last (state s).
// EVAL: the data cost per vertex slot into E.part and the five tips into S.joints.  REST: the vertices into E.T (778 x 3).
// JAC: the tiles and, in acc, the wave's blocks of their Gram matrix -- wave 0: (0,0) (1,0) (1,1); 1: (2,0) (2,1) (2,2);
// 2: (3,0) (3,1); 3: (3,2) (3,3) -- after shape_chain() and E.D.
template <int MODE>
__device__ __forceinline__ void walk(State& S, Mesh& E, const hands_mano_fit_verts_side& sd, long long b, int s, int tid, f64x4* acc) {
  const hands_mano_fit_verts_consts& C = sd.consts;
  const int g = tid >> 4, j = tid & 15, lane = tid & 63, wv = tid >> 6;
  double Qj[9], Fj[9], pj[3], Jj[3], tt[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    Qj[k] = S.Q[9 * j + k];
    Fj[k] = S.R[s][9 * j + k] - (k % 4 == 0 ? 1.0 : 0.0);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pj[c] = S.p[3 * j + c];
    Jj[c] = S.Jr[3 * j + c];
    tt[c] = S.t[s][c];
  }
  double cost = 0.0;
#pragma unroll 1
  for (int tile = 0; tile < NTILE; ++tile) {
    const int n = tile * TV + g;
    const bool present = n < NV;
    const int nn = present ? n : NV - 1;         // an absent vertex reads the last one and writes zeros
    // v~_n: lane 0 the template and the shape blend shapes, lane j >= 1 the nine pose features of joint j
    double a[3];
    float pd[27];
    if (j == 0) {
#pragma unroll
      for (int i = 0; i < 27; ++i) pd[i] = 0.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[c] = (double)C.v_template[nn * 3 + c];
#pragma unroll
        for (int l = 0; l < 10; ++l) a[c] += (double)C.shapedirs[(nn * 3 + c) * 10 + l] * S.beta[s][l];
      }
    } else {
      const float* q = C.posedirs_vm + (long long)nn * 405 + 27 * (j - 1);
#pragma unroll
      for (int i = 0; i < 27; ++i) pd[i] = q[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[c] = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) a[c] += Fj[k] * (double)pd[3 * k + c];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = sum16(a[c]);
    // x_{n,j} and v_n = sum_j W_nj x_{n,j}
    const double W = (double)C.lbs_weights[nn * 16 + j];
    const double e0 = a[0] - Jj[0], e1 = a[1] - Jj[1], e2 = a[2] - Jj[2];
    double wx[3], v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      wx[c] = W * (pj[c] + ((Qj[3 * c] * e0 + Qj[3 * c + 1] * e1) + Qj[3 * c + 2] * e2));
      v[c] = sum16(wx[c]);
    }
    const float wn = E.w[n];                     // 0 for an absent vertex
    const bool on = wn > 0.f;
    const double sw = sqrt((double)wn);

    if constexpr (MODE == REST) {
      if (j == 0 && present) {
#pragma unroll
        for (int c = 0; c < 3; ++c) E.T[3 * n + c] = v[c];
      }
    } else if constexpr (MODE == EVAL) {
      if (j == 0) {
        if (on) {                                // a vertex of weight 0 is never read
          const float* y = sd.verts + (b * NV + n) * 3;
          const double r0 = sw * ((v[0] + tt[0]) - (double)y[0]), r1 = sw * ((v[1] + tt[1]) - (double)y[1]);
          const double r2 = sw * ((v[2] + tt[2]) - (double)y[2]);
          cost += (r0 * r0 + r1 * r1) + r2 * r2;
        }
        const int m = present ? tip_of(n) : -1;
        if (m >= 0) {
#pragma unroll
          for (int c = 0; c < 3; ++c) S.joints[48 + 3 * m + c] = v[c];
        }
      }
    } else {
      // A_n = sum_i W_ni Q_i, and what joint j moves of the vertex: sum over i at or below j of W_ni (x_ni - p_j)
      double A[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) A[k] = sum16(W * Qj[k]);
      const double Wall = sum16(W);
      const int q = (j + 2) % 3;                 // the place in the finger of joint j >= 1: 0, 1, 2
      const double W1 = row_move<0x101>(W), W2 = row_move<0x102>(W);
      const double Ws = j == 0 ? Wall : (W + (q < 2 ? W1 : 0.0)) + (q < 1 ? W2 : 0.0);
      double sv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double x1 = row_move<0x101>(wx[c]), x2 = row_move<0x102>(wx[c]);
        const double sx = j == 0 ? v[c] : (wx[c] + (q < 2 ? x1 : 0.0)) + (q < 1 ? x2 : 0.0);
        sv[c] = sx - Ws * pj[c];
      }
      double B[9];
#pragma unroll
      for (int c = 0; c < 3; ++c) {              // column c of -[sv]x Q_j = (column c of Q_j) x sv
        const double q0 = Qj[c], q1 = Qj[3 + c], q2 = Qj[6 + c];
        B[c] = q1 * sv[2] - q2 * sv[1];
        B[3 + c] = q2 * sv[0] - q0 * sv[2];
        B[6 + c] = q0 * sv[1] - q1 * sv[0];
      }
      if (j >= 1) {                              // the pose blend shapes: A_n posedirs_n vec(R_j [e_a]x)
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
          double dR[9];
#pragma unroll
          for (int r = 0; r < 3; ++r) {          // R [e_a]x: columns (0, R2, -R1), (-R2, 0, R0), (R1, -R0, 0)
            const double R0 = Fj[3 * r] + (r == 0 ? 1.0 : 0.0), R1 = Fj[3 * r + 1] + (r == 1 ? 1.0 : 0.0);
            const double R2 = Fj[3 * r + 2] + (r == 2 ? 1.0 : 0.0);
            dR[3 * r] = ax == 0 ? 0.0 : (ax == 1 ? -R2 : R1);
            dR[3 * r + 1] = ax == 0 ? R2 : (ax == 1 ? 0.0 : -R0);
            dR[3 * r + 2] = ax == 0 ? -R1 : (ax == 1 ? R0 : 0.0);
          }
          double u[3] = {0.0, 0.0, 0.0};
#pragma unroll
          for (int f = 0; f < 9; ++f)
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c] += dR[f] * (double)pd[3 * f + c];
#pragma unroll
          for (int r = 0; r < 3; ++r) B[3 * r + ax] += (A[3 * r] * u[0] + A[3 * r + 1] * u[1]) + A[3 * r + 2] * u[2];
        }
      }
      // the lane's sixteenth column: shape l = j, translation, residual, zeros
      double col[3] = {0.0, 0.0, 0.0};
      if (j < 10) {
        double sdl[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) sdl[k] = (double)C.shapedirs[(nn * 3 + k) * 10 + j];
#pragma unroll
        for (int r = 0; r < 3; ++r) col[r] = (A[3 * r] * sdl[0] + A[3 * r + 1] * sdl[1]) + A[3 * r + 2] * sdl[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const double wi = (double)C.lbs_weights[nn * 16 + i];
#pragma unroll
          for (int r = 0; r < 3; ++r) col[r] += wi * E.D[(3 * i + r) * 10 + j];
        }
      } else if (j < 13) {
#pragma unroll
        for (int r = 0; r < 3; ++r) col[r] = j - 10 == r ? 1.0 : 0.0;
      } else if (j == 13 && on) {
        const float* y = sd.verts + (b * NV + n) * 3;
#pragma unroll
        for (int r = 0; r < 3; ++r) col[r] = (v[r] + tt[r]) - (double)y[r];
      }
      double* row = E.T + (3 * g) * TC;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) row[r * TC + 3 * j + c] = on ? sw * B[3 * r + c] : 0.0;
        row[r * TC + 48 + j] = on ? sw * col[r] : 0.0;
      }
      __syncthreads();
      const double* src = E.T + (lane >> 4) * TC + (lane & 15);
#pragma unroll 4
      for (int k = 0; k < TR / 4; ++k) {         // four rows a step: lane holds row 4 k + (lane >> 4), column lane & 15 of a block
        const double c0 = src[4 * k * TC], c1 = src[4 * k * TC + 16], c2 = src[4 * k * TC + 32], c3 = src[4 * k * TC + 48];
        if (wv == 0) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c0, c0, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, c0, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(c1, c1, acc[2], 0, 0, 0);
        } else if (wv == 1) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c2, c0, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c2, c1, acc[1], 0, 0, 0);
          acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(c2, c2, acc[2], 0, 0, 0);
        } else if (wv == 2) {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c3, c0, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c3, c1, acc[1], 0, 0, 0);
        } else {
          acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(c3, c2, acc[0], 0, 0, 0);
          acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(c3, c3, acc[1], 0, 0, 0);
        }
      }
      __syncthreads();
    }
  }
  if (MODE == EVAL && j == 0) E.part[g] = cost;
  __syncthreads();
}

// Cost and data cost of state s; leaves the joints, the tips and what the walks read of the state.
__device__ void evaluate_verts(State& S, Mesh& E, const hands_mano_fit_verts_side& sd, long long b, int s, double lb, double lp, int tid) {
  joint_state(S, sd.consts, s, tid);
  walk<EVAL>(S, E, sd, b, s, tid, nullptr);
  if (tid == 0) {
    double data = 0.0;
    for (int k = 0; k < TV; ++k) data += E.part[k];
    double all = data;
    for (int l = 0; l < 10; ++l) all += lb * (S.beta[s][l] * S.beta[s][l]);
    for (int k = 0; k < 45; ++k) all += lp * (S.lg[k] * S.lg[k]);
    S.c[0] = all;
    S.c[1] = data;
  }
  __syncthreads();
}

// g and the damped H at the state evaluate_verts() saw last (state s)
__device__ void linearise_verts(State& S, Mesh& E, const hands_mano_fit_verts_side& sd, long long b, int s, double lb, double lp,
                                double mu, int tid) {
  const hands_mano_fit_consts Cj = {sd.consts.pose_mean, sd.consts.J_template, sd.consts.J_shapedirs, nullptr, nullptr, nullptr, nullptr};
  shape_chain(S, Cj, tid);
  for (int it = tid; it < 480; it += NT) {
    const int i = it / 30, c = (it % 30) / 10, l = it % 10;
    const double* q = S.Q + 9 * i + 3 * c;
    const float* sj = sd.consts.J_shapedirs + (3 * i) * 10 + l;
    E.D[it] = S.dp[it] - ((q[0] * (double)sj[0] + q[1] * (double)sj[10]) + q[2] * (double)sj[20]);
  }
  __syncthreads();
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  f64x4 acc[3] = {zero, zero, zero};
  walk<JAC>(S, E, sd, b, s, tid, acc);
  const int lane = tid & 63, wv = tid >> 6;
  if (wv == 0) {
    put_block(S, acc[0], 0, 0, lane, s, lb, lp, mu);
    put_block(S, acc[1], 1, 0, lane, s, lb, lp, mu);
    put_block(S, acc[2], 1, 1, lane, s, lb, lp, mu);
  } else if (wv == 1) {
    put_block(S, acc[0], 2, 0, lane, s, lb, lp, mu);
    put_block(S, acc[1], 2, 1, lane, s, lb, lp, mu);
    put_block(S, acc[2], 2, 2, lane, s, lb, lp, mu);
  } else if (wv == 2) {
    put_block(S, acc[0], 3, 0, lane, s, lb, lp, mu);
    put_block(S, acc[1], 3, 1, lane, s, lb, lp, mu);
  } else {
    put_block(S, acc[0], 3, 2, lane, s, lb, lp, mu);
    put_block(S, acc[1], 3, 3, lane, s, lb, lp, mu);
  }
  __syncthreads();
}

struct SidesV {
  hands_mano_fit_verts_side s[2];
};

__global__ void __launch_bounds__(NT) mano_fit_verts_kernel(SidesV sides, hands_fit_cfg cfg) {
  __shared__ State S;
  __shared__ Mesh E;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const hands_mano_fit_verts_side& sd = sides.s[blockIdx.y];
  const hands_mano_fit_verts_consts& C = sd.consts;
  const double lb = cfg.lambda_beta, lp = cfg.lambda_pose;
  double* red = E.T + RED;

  // the target: a vertex of weight 0 (or of a weight that is no number) is never read
  bool bad = false;
  int nsel = 0;
  double wsum = 0.0;
#pragma unroll 1
  for (int r = 0; r < 4; ++r) {
    const int n = tid + NT * r;
    bool sel = false;
    if (n < NVP) {
      const float w = n < NV ? (sd.weights ? sd.weights[b * NV + n] : 1.f) : 0.f;
      sel = w > 0.f;
      E.w[n] = sel ? w : 0.f;
      if (sel) {
        wsum += (double)w;
        bad = bad || !isfinite(w);               // a selected weight of +inf: the row is not fitted
#pragma unroll
        for (int c = 0; c < 3; ++c) bad = bad || !isfinite(sd.verts[(b * NV + n) * 3 + c]);
      }
    }
    nsel += __syncthreads_count(sel);
  }
  mean_pose(S, C.pose_mean, tid);
  bad = read_init(S, sd, b, tid) || bad;         // a caller's initial state
  if (!row_fitted(sd, b, nsel, bad)) {           // the whole workgroup leaves; NaN in j3d
    store_unfitted(S, sd, b, tid);
    if (tid < 63) sd.j3d[b * 63 + tid] = __builtin_nanf("");
    return;
  }
  {
    const double sw = block_sum(wsum, red, tid);
    if (tid == 0) E.sumw = sw;
  }

  if (!sd.init_pose) {                           // the rest hand, its vertices aligned rigidly to the weighted target vertices
    rest_state(S, tid);
    joint_state(S, C, 0, tid);
    walk<REST>(S, E, sd, b, 0, tid, nullptr);
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int n = tid; n < NV; n += NT)
      if (E.w[n] > 0.f) {
        const double w = (double)E.w[n];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          m[c] += w * E.T[3 * n + c];
          m[3 + c] += w * (double)sd.verts[(b * NV + n) * 3 + c];
        }
      }
    const double sw = E.sumw;
#pragma unroll
    for (int c = 0; c < 6; ++c) m[c] = block_sum(m[c], red, tid) / sw;
    double k9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int n = tid; n < NV; n += NT)
      if (E.w[n] > 0.f) {
        const double w = (double)E.w[n];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double x1 = w * (E.T[3 * n + a] - m[a]);
#pragma unroll
          for (int c = 0; c < 3; ++c) k9[3 * a + c] += x1 * ((double)sd.verts[(b * NV + n) * 3 + c] - m[3 + c]);
        }
      }
#pragma unroll
    for (int c = 0; c < 9; ++c) k9[c] = block_sum(k9[c], red, tid);
    if (tid == 0) {
      double K[3][3], Rm[3][3], scale;
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) K[a][c] = k9[3 * a + c];
      procrustes_solve(K, 1.0, Rm, &scale);      // the scale is not used: the alignment is rigid
      place_rigid(S, Rm, m, m + 3);
    }
  }
  __syncthreads();

  // lm_stage of fit_device.h with FREE_ALL, written out (see the head of the file); `fresh`: what evaluate_verts() left in LDS
  // belongs to the current state
  double mu = cfg.mu0, c0 = 0.0;
  int steps = 0;
  bool fresh = false;
  for (int it = 0; it < cfg.iters; ++it) {
    if (!fresh) {
      evaluate_verts(S, E, sd, b, 0, lb, lp, tid);
      c0 = S.c[0];
    }
    linearise_verts(S, E, sd, b, 0, lb, lp, mu, tid);
    const bool ok = solve(S, tid);
    if (tid < 16) {                              // the candidate: R_j Exp(delta_j), beta + delta_beta, t + delta_t
      const double w[3] = {S.d[3 * tid], S.d[3 * tid + 1], S.d[3 * tid + 2]};
      double X[9], Rn[9];
      exp_so3(w, X);
      mul_nn(S.R[0] + 9 * tid, X, Rn);
#pragma unroll
      for (int k = 0; k < 9; ++k) S.R[1][9 * tid + k] = Rn[k];
    } else if (tid >= 64 && tid < 74) {
      S.beta[1][tid - 64] = S.beta[0][tid - 64] + S.d[UB + tid - 64];
    } else if (tid >= 74 && tid < 77) {
      S.t[1][tid - 74] = S.t[0][tid - 74] + S.d[UT + tid - 74];
    }
    __syncthreads();
    evaluate_verts(S, E, sd, b, 1, lb, lp, tid);
    const double c1 = S.c[0];
    const bool accept = ok && c1 < c0;           // strict, false for NaN; the same on every lane
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
  if (!fresh) evaluate_verts(S, E, sd, b, 0, lb, lp, tid);

  store_fitted(S, sd, b, steps, tid, [&] { return E.sumw; });
  if (tid < 63) sd.j3d[b * 63 + tid] = (float)(S.joints[tid] + S.t[0][tid % 3]);
}

}  // namespace

extern "C" int hands_mano_fit_verts_f32(const hands_mano_fit_verts_side* sides, int n_sides, const hands_fit_cfg* cfg, int B,
                                        hands_stream_t stream) {
  if (!sides || !cfg || n_sides < 1 || n_sides > 2 || B <= 0 || !fit_cfg_ok(*cfg)) return HANDS_EINVAL;
  SidesV k;
  for (int i = 0; i < 2; ++i) {
    const hands_mano_fit_verts_side& d = k.s[i] = sides[i < n_sides ? i : 0];
    const hands_mano_fit_verts_consts& c = d.consts;
    if (!fit_side_ok(d, {c.pose_mean, c.J_template, c.J_shapedirs, c.v_template, c.shapedirs, c.lbs_weights, c.posedirs_vm, d.verts,
                         d.pose, d.beta, d.transl, d.rmse, d.steps, d.j3d}))
      return HANDS_EINVAL;
  }
  hipLaunchKernelGGL(mano_fit_verts_kernel, dim3(B, n_sides), dim3(NT), 0, (hipStream_t)stream, k, *cfg);
  HANDS_LAUNCH_CHECK();
}
