// fit_surf.hip -- MANO fitting to surface correspondences (hands_mano_fit_surf_f32 of include/hands_hip.h): the Levenberg-Marquardt
// fit of fit_verts.hip -- the same 61 unknowns, damping, accept rule and priors -- whose P data rows are points ON FACES of the
// model: row k names a face f_k of the asset's face list and three coefficients b_k, c_k = sum_i b_ki v_{faces[f_k][i]}, and the
// residual is sqrt(w_k) A_k (c_k + t - y_k) with A_k = I or, with normals and tangent_weight tau != 1, n n^T + sqrt(tau) (I - n n^T).
// DESIGN.md section 7 "MANO fitting to surface correspondences and ICP registration" is the specification, tests/fit_surf_ref.py
// its fp64 restatement.  Launch as the siblings: grid (B, n_sides), one workgroup of four waves per hand, fp32 in, fp64
// arithmetic, one rounding per output, exactly `iters` iterations, no atomics, no allocation.
//
// The rows stream from global memory in tiles of 16, so P is not bounded by LDS.  Sixteen lanes share a row, lane j of them owns
// joint j as in fit_verts.hip; the row's three vertices are evaluated one after the other with that kernel's arithmetic -- v~_n,
// x_{n,j}, v_n, sum_i W_ni Q_i, the 3 x 3 block d v_n / d delta_j and the lane's shape column -- and added with the coefficients
// b_k0, b_k1, b_k2 in that order; the translation and residual columns belong to the row, not to a vertex.  A_k then multiplies
// the lane's four columns.  A tile is 48 rows x 64 columns in LDS and its Gram matrix is added by the four waves with
// v_mfma_f64_16x16x4_f64 exactly as there.  A tile whose sixteen weights are all zero is skipped by the whole workgroup; a row of
// weight 0 inside a tile writes zeros and reads nothing of its own.  The vertices are walked twice more, in 49 tiles of 16: at
// the rest state for the Kabsch start (into LDS) and at the end for `verts` and the five tips of j3d.
// The iteration is lm_stage of fit_device.h with FREE_ALL.  Every sum has an order the code fixes: a row slot adds its tiles in
// ascending order, one lane adds the 16 slots; the set-up sums go lane-strided and then through block_sum.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"
#include "fit_device.h"
#include "fit_mesh_device.h"

namespace {

constexpr int NV = 778, NF = 1538;               // vertices and faces of the asset
constexpr int TV = 16, NVT = (NV + TV - 1) / TV; // rows (or vertices) of a tile; 49 vertex tiles
constexpr int TR = 3 * TV, TC = 64;              // rows and columns of a tile: 61 unknowns, the residual, two zero columns
constexpr int RED = 2400;                        // where the reduction buffer starts in the tile, behind the 2334 rest coordinates

struct Surf {                                    // what this fit keeps beside the state
  double T[TR * TC];                             // the tile; before the iteration the rest vertices and the reduction buffer
  double D[480];                                 // d p_i / d beta - Q_i S_i, (16, 3, 10)
  double part[TV], data[TV];                     // per row slot: the cost of the data rows, and sum w |c + t - y|^2
  double sumw;
};

enum { EVAL = 0, JAC = 1, REST = 2, VERTS = 3 };

struct Joint {                                   // what lane j holds of joint j and of the state for a whole walk
  double Q[9], F[9], p[3], J[3], t[3];
};

__device__ __forceinline__ int tip_of(int n) {           // the tip slot of vertex n or -1
  return n == 744 ? 0 : (n == 320 ? 1 : (n == 443 ? 2 : (n == 554 ? 3 : (n == 671 ? 4 : -1))));
}

// Vertex nn at state s, the arithmetic of fit_verts.hip's walk: v = v_n on all sixteen lanes; with JACOBIAN also the lane's
// block B = d v_n / d delta_j (3 x 3, row-major) and, on lanes 0..9, its shape column col.
template <bool JACOBIAN>
__device__ __forceinline__ void vertex(const State& S, const Surf& E, const hands_mano_fit_verts_consts& C, const Joint& L, int s, int nn,
                                       int j, double* v, double* B, double* col) {
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
      for (int k = 0; k < 9; ++k) a[c] += L.F[k] * (double)pd[3 * k + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = sum16(a[c]);
  // x_{n,j} and v_n = sum_j W_nj x_{n,j}
  const double W = (double)C.lbs_weights[nn * 16 + j];
  const double e0 = a[0] - L.J[0], e1 = a[1] - L.J[1], e2 = a[2] - L.J[2];
  double wx[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    wx[c] = W * (L.p[c] + ((L.Q[3 * c] * e0 + L.Q[3 * c + 1] * e1) + L.Q[3 * c + 2] * e2));
    v[c] = sum16(wx[c]);
  }
  if constexpr (JACOBIAN) {
    // A_n = sum_i W_ni Q_i, and what joint j moves of the vertex: sum over i at or below j of W_ni (x_ni - p_j)
    double A[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = sum16(W * L.Q[k]);
    const double Wall = sum16(W);
    const int q = (j + 2) % 3;                   // the place in the finger of joint j >= 1: 0, 1, 2
    const double W1 = row_move<0x101>(W), W2 = row_move<0x102>(W);
    const double Ws = j == 0 ? Wall : (W + (q < 2 ? W1 : 0.0)) + (q < 1 ? W2 : 0.0);
    double sv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x1 = row_move<0x101>(wx[c]), x2 = row_move<0x102>(wx[c]);
      const double sx = j == 0 ? v[c] : (wx[c] + (q < 2 ? x1 : 0.0)) + (q < 1 ? x2 : 0.0);
      sv[c] = sx - Ws * L.p[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {                // column c of -[sv]x Q_j = (column c of Q_j) x sv
      const double q0 = L.Q[c], q1 = L.Q[3 + c], q2 = L.Q[6 + c];
      B[c] = q1 * sv[2] - q2 * sv[1];
      B[3 + c] = q2 * sv[0] - q0 * sv[2];
      B[6 + c] = q0 * sv[1] - q1 * sv[0];
    }
    if (j >= 1) {                                // the pose blend shapes: A_n posedirs_n vec(R_j [e_a]x)
#pragma unroll
      for (int ax = 0; ax < 3; ++ax) {
        double dR[9];
#pragma unroll
        for (int r = 0; r < 3; ++r) {            // R [e_a]x: columns (0, R2, -R1), (-R2, 0, R0), (R1, -R0, 0)
          const double R0 = L.F[3 * r] + (r == 0 ? 1.0 : 0.0), R1 = L.F[3 * r + 1] + (r == 1 ? 1.0 : 0.0);
          const double R2 = L.F[3 * r + 2] + (r == 2 ? 1.0 : 0.0);
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
#pragma unroll
    for (int r = 0; r < 3; ++r) col[r] = 0.0;
    if (j < 10) {                                // shape l = j
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
    }
  }
}

// x <- A x, A = n n^T + sq (I - n n^T)
__device__ __forceinline__ void apply_normal(const double* n, double sq, double* x) {
  const double d = (n[0] * x[0] + n[1] * x[1]) + n[2] * x[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) x[r] = n[r] * d + sq * (x[r] - n[r] * d);
}

// the tile's Gram matrix onto the wave's blocks -- wave 0: (0,0) (1,0) (1,1); 1: (2,0) (2,1) (2,2); 2: (3,0) (3,1); 3: (3,2) (3,3)
__device__ __forceinline__ void gram_tile(const double* T, int lane, int wv, f64x4* acc) {
  const double* src = T + (lane >> 4) * TC + (lane & 15);
#pragma unroll 4
  for (int k = 0; k < TR / 4; ++k) {             // four rows a step: lane holds row 4 k + (lane >> 4), column lane & 15 of a block
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
}

// One walk at the state joint_state() saw last (state s).
// EVAL: over the rows; the cost per row slot into E.part and sum w |c + t - y|^2 into E.data.
// JAC: over the rows; the tiles and, in acc, the wave's blocks of their Gram matrix -- after shape_chain() and E.D.
// REST: over the vertices; the vertices into E.T (778 x 3).  VERTS: over the vertices; vertices + t into sd.verts, the tips into S.joints.
// sq: sqrt(tangent_weight) where the normals are used, else a negative number.
template <int MODE>
__device__ __forceinline__ void walk(State& S, Surf& E, const hands_mano_fit_surf_side& sd, long long b, int P, int s, double sq, int tid,
                                     f64x4* acc) {
  const hands_mano_fit_verts_consts& C = sd.consts.mano;
  constexpr bool ROWS = MODE == EVAL || MODE == JAC;
  const int g = tid >> 4, j = tid & 15, lane = tid & 63, wv = tid >> 6;
  Joint L;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    L.Q[k] = S.Q[9 * j + k];
    L.F[k] = S.R[s][9 * j + k] - (k % 4 == 0 ? 1.0 : 0.0);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    L.p[c] = S.p[3 * j + c];
    L.J[c] = S.Jr[3 * j + c];
    L.t[c] = S.t[s][c];
  }
  double cost = 0.0, data = 0.0;
  const int ntile = ROWS ? (P + TV - 1) / TV : NVT;
#pragma unroll 1
  for (int tile = 0; tile < ntile; ++tile) {
    const int k = tile * TV + g;                 // the row, or the vertex
    if constexpr (ROWS) {
      const long long o = b * P + k;
      const float wk = k < P ? (sd.weights ? sd.weights[o] : 1.f) : 0.f;
      const bool on = wk > 0.f;                  // a row of weight 0 (or of a weight that is no number) is never read
      if (!__syncthreads_or(on)) continue;       // the whole workgroup: a tile without a weighted row
      const double sw = sqrt(on ? (double)wk : 0.0);
      int n0 = 0, n1 = 0, n2 = 0;
      double b0 = 0.0, b1 = 0.0, b2 = 0.0;
      if (on) {                                  // the set-up has checked the face and its three vertices
        const int32_t* fv = sd.consts.faces + 3 * sd.face_idx[o];
        n0 = fv[0]; n1 = fv[1]; n2 = fv[2];
        b0 = (double)sd.bary[3 * o]; b1 = (double)sd.bary[3 * o + 1]; b2 = (double)sd.bary[3 * o + 2];
      }
      double nr[3] = {0.0, 0.0, 0.0};
      bool useA = false;
      if (sq >= 0.0 && on) {
#pragma unroll
        for (int c = 0; c < 3; ++c) nr[c] = (double)sd.normals[3 * o + c];
        useA = nr[0] != 0.0 || nr[1] != 0.0 || nr[2] != 0.0;           // a zero normal: A = I
      }
      double vt[3] = {0.0, 0.0, 0.0}, Bt[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ct[3] = {0.0, 0.0, 0.0};
#pragma unroll 1
      for (int i = 0; i < 3; ++i) {
        const int nn = i == 0 ? n0 : (i == 1 ? n1 : n2);
        const double bi = i == 0 ? b0 : (i == 1 ? b1 : b2);
        double v[3], B[9], col[3];
        vertex<MODE == JAC>(S, E, C, L, s, nn, j, v, B, col);
#pragma unroll
        for (int c = 0; c < 3; ++c) vt[c] += bi * v[c];
        if constexpr (MODE == JAC) {
#pragma unroll
          for (int c = 0; c < 9; ++c) Bt[c] += bi * B[c];
#pragma unroll
          for (int c = 0; c < 3; ++c) ct[c] += bi * col[c];
        }
      }
      if constexpr (MODE == EVAL) {
        if (j == 0 && on) {
          const float* y = sd.points + 3 * o;
          double e[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) e[c] = sw * ((vt[c] + L.t[c]) - (double)y[c]);
          data += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
          if (useA) apply_normal(nr, sq, e);
          cost += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
        }
      } else {
        // the lane's sixteenth column: shape l = j (ct), translation, residual, zeros
        if (j >= 10 && j < 13) {
#pragma unroll
          for (int r = 0; r < 3; ++r) ct[r] = j - 10 == r ? 1.0 : 0.0;
        } else if (j == 13 && on) {
          const float* y = sd.points + 3 * o;
#pragma unroll
          for (int r = 0; r < 3; ++r) ct[r] = (vt[r] + L.t[r]) - (double)y[r];
        }
        if (useA) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            double x[3] = {Bt[c], Bt[3 + c], Bt[6 + c]};
            apply_normal(nr, sq, x);
            Bt[c] = x[0]; Bt[3 + c] = x[1]; Bt[6 + c] = x[2];
          }
          apply_normal(nr, sq, ct);
        }
        double* row = E.T + (3 * g) * TC;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
          for (int c = 0; c < 3; ++c) row[r * TC + 3 * j + c] = on ? sw * Bt[3 * r + c] : 0.0;
          row[r * TC + 48 + j] = on ? sw * ct[r] : 0.0;
        }
        __syncthreads();
        gram_tile(E.T, lane, wv, acc);
        __syncthreads();
      }
    } else {
      const bool present = k < NV;
      const int nn = present ? k : NV - 1;       // an absent vertex reads the last one and writes nothing
      double v[3];
      vertex<false>(S, E, C, L, s, nn, j, v, nullptr, nullptr);
      if (j == 0 && present) {
        if constexpr (MODE == REST) {
#pragma unroll
          for (int c = 0; c < 3; ++c) E.T[3 * k + c] = v[c];
        } else {
#pragma unroll
          for (int c = 0; c < 3; ++c) sd.verts[(b * NV + k) * 3 + c] = (float)(v[c] + L.t[c]);
          const int m = tip_of(k);
          if (m >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) S.joints[48 + 3 * m + c] = v[c];
          }
        }
      }
    }
  }
  if (MODE == EVAL && j == 0) {
    E.part[g] = cost;
    E.data[g] = data;
  }
  __syncthreads();
}

// Cost and sum w |c + t - y|^2 of state s; leaves the joints and what the walks read of the state.
__device__ void evaluate_surf(State& S, Surf& E, const hands_mano_fit_surf_side& sd, long long b, int P, int s, double sq, double lb,
                              double lp, int tid) {
  joint_state(S, sd.consts.mano, s, tid);
  walk<EVAL>(S, E, sd, b, P, s, sq, tid, nullptr);
  if (tid == 0) {
    double all = 0.0, data = 0.0;
    for (int k = 0; k < TV; ++k) {
      all += E.part[k];
      data += E.data[k];
    }
    for (int l = 0; l < 10; ++l) all += lb * (S.beta[s][l] * S.beta[s][l]);
    for (int k = 0; k < 45; ++k) all += lp * (S.lg[k] * S.lg[k]);
    S.c[0] = all;
    S.c[1] = data;
  }
  __syncthreads();
}

// g and the damped H at the state evaluate_surf() saw last (state s)
__device__ void linearise_surf(State& S, Surf& E, const hands_mano_fit_surf_side& sd, long long b, int P, int s, double sq, double lb,
                               double lp, double mu, int tid) {
  const hands_mano_fit_verts_consts& C = sd.consts.mano;
  const hands_mano_fit_consts Cj = {C.pose_mean, C.J_template, C.J_shapedirs, nullptr, nullptr, nullptr, nullptr};
  shape_chain(S, Cj, tid);
  for (int it = tid; it < 480; it += NT) {
    const int i = it / 30, c = (it % 30) / 10, l = it % 10;
    const double* q = S.Q + 9 * i + 3 * c;
    const float* sj = C.J_shapedirs + (3 * i) * 10 + l;
    E.D[it] = S.dp[it] - ((q[0] * (double)sj[0] + q[1] * (double)sj[10]) + q[2] * (double)sj[20]);
  }
  __syncthreads();
  const f64x4 zero = {0.0, 0.0, 0.0, 0.0};
  f64x4 acc[3] = {zero, zero, zero};
  walk<JAC>(S, E, sd, b, P, s, sq, tid, acc);
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

// the rest-state surface point of a weighted row from the rest vertices in E.T
__device__ __forceinline__ void rest_point(const Surf& E, const hands_mano_fit_surf_side& sd, long long o, double* c) {
  const int32_t* fv = sd.consts.faces + 3 * sd.face_idx[o];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    c[a] = ((double)sd.bary[3 * o] * E.T[3 * fv[0] + a] + (double)sd.bary[3 * o + 1] * E.T[3 * fv[1] + a]) +
           (double)sd.bary[3 * o + 2] * E.T[3 * fv[2] + a];
}

struct SidesS {
  hands_mano_fit_surf_side s[2];
};

__global__ void __launch_bounds__(NT) mano_fit_surf_kernel(SidesS sides, hands_fit_surf_cfg cfg, int P) {
  __shared__ State S;
  __shared__ Surf E;
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  const hands_mano_fit_surf_side& sd = sides.s[blockIdx.y];
  const hands_mano_fit_verts_consts& C = sd.consts.mano;
  const double lb = cfg.lambda_beta, lp = cfg.lambda_pose;
  const bool normals = sd.normals && cfg.tangent_weight != 1.0;        // tangent_weight 1 is A = I exactly: the normals are not read
  const double sq = normals ? sqrt(cfg.tangent_weight) : -1.0;
  double* red = E.T + RED;

  // the rows: one of weight 0 (or of a weight that is no number) is never read; the face index is checked before anything is
  // read through it, and so are the face's vertex indices
  bool bad = false;
  int cnt = 0;
  double wsum = 0.0;
#pragma unroll 1
  for (int k = tid; k < P; k += NT) {
    const long long o = b * P + k;
    const float w = sd.weights ? sd.weights[o] : 1.f;
    if (w > 0.f) {
      ++cnt;
      wsum += (double)w;
      bad = bad || !isfinite(w);                 // a selected weight of +inf: the hand is not fitted
      const int f = sd.face_idx[o];
      if (f < 0 || f >= NF) {
        bad = true;
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) bad = bad || (unsigned)sd.consts.faces[3 * f + c] >= (unsigned)NV;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        bad = bad || !isfinite(sd.points[3 * o + c]) || !isfinite(sd.bary[3 * o + c]);
        if (normals) bad = bad || !isfinite(sd.normals[3 * o + c]);
      }
    }
  }
  const int nsel = (int)block_sum((double)cnt, red, tid);              // exact: at most HANDS_FIT_SURF_MAX_P
  mean_pose(S, C.pose_mean, tid);
  bad = read_init(S, sd, b, tid) || bad;         // a caller's initial state
  if (!row_fitted(sd, b, nsel, bad)) {           // the whole workgroup leaves; NaN in j3d and verts
    store_unfitted(S, sd, b, tid);
    if (tid < 63) sd.j3d[b * 63 + tid] = __builtin_nanf("");
    for (int i = tid; i < NV * 3; i += NT) sd.verts[b * NV * 3 + i] = __builtin_nanf("");
    return;
  }
  {
    const double sw = block_sum(wsum, red, tid);
    if (tid == 0) E.sumw = sw;
  }

  if (!sd.init_pose) {                           // the rest hand, its surface points aligned rigidly to the weighted targets
    rest_state(S, tid);
    joint_state(S, C, 0, tid);
    walk<REST>(S, E, sd, b, P, 0, sq, tid, nullptr);
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = tid; k < P; k += NT) {
      const long long o = b * P + k;
      const float wf = sd.weights ? sd.weights[o] : 1.f;
      if (wf > 0.f) {
        const double w = (double)wf;
        double c[3];
        rest_point(E, sd, o, c);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          m[a] += w * c[a];
          m[3 + a] += w * (double)sd.points[3 * o + a];
        }
      }
    }
    const double sw = E.sumw;
#pragma unroll
    for (int c = 0; c < 6; ++c) m[c] = block_sum(m[c], red, tid) / sw;
    double k9[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int k = tid; k < P; k += NT) {
      const long long o = b * P + k;
      const float wf = sd.weights ? sd.weights[o] : 1.f;
      if (wf > 0.f) {
        const double w = (double)wf;
        double c[3];
        rest_point(E, sd, o, c);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          const double x1 = w * (c[a] - m[a]);
#pragma unroll
          for (int q = 0; q < 3; ++q) k9[3 * a + q] += x1 * ((double)sd.points[3 * o + q] - m[3 + q]);
        }
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

  double c0 = 0.0;
  int steps = 0;
  bool fresh = false;
  lm_stage(S, cfg.iters, FREE_ALL, cfg.mu0, c0, steps, fresh, tid,
           [&](int s) { evaluate_surf(S, E, sd, b, P, s, sq, lb, lp, tid); },
           [&](double mu, int) { linearise_surf(S, E, sd, b, P, 0, sq, lb, lp, mu, tid); });

  walk<VERTS>(S, E, sd, b, P, 0, sq, tid, nullptr);      // the vertices and the five tips of the state evaluate_surf() saw last
  store_fitted(S, sd, b, steps, tid, [&] { return E.sumw; });
  if (tid < 63) sd.j3d[b * 63 + tid] = (float)(S.joints[tid] + S.t[0][tid % 3]);
}

}  // namespace

extern "C" int hands_mano_fit_surf_f32(const hands_mano_fit_surf_side* sides, int n_sides, const hands_fit_surf_cfg* cfg, int B, int P,
                                       hands_stream_t stream) {
  if (!sides || !cfg || n_sides < 1 || n_sides > 2 || B <= 0 || P < 1 || P > HANDS_FIT_SURF_MAX_P || !fit_cfg_ok(*cfg))
    return HANDS_EINVAL;
  if (!(cfg->tangent_weight >= 0.0 && cfg->tangent_weight <= 1.0)) return HANDS_EINVAL;
  SidesS k;
  for (int i = 0; i < 2; ++i) {
    const hands_mano_fit_surf_side& d = k.s[i] = sides[i < n_sides ? i : 0];
    const hands_mano_fit_verts_consts& c = d.consts.mano;
    if (!fit_side_ok(d, {c.pose_mean, c.J_template, c.J_shapedirs, c.v_template, c.shapedirs, c.lbs_weights, c.posedirs_vm,
                         d.consts.faces, d.points, d.face_idx, d.bary, d.pose, d.beta, d.transl, d.rmse, d.steps, d.j3d, d.verts}))
      return HANDS_EINVAL;
  }
  hipLaunchKernelGGL(mano_fit_surf_kernel, dim3(B, n_sides), dim3(NT), 0, (hipStream_t)stream, k, *cfg, P);
  HANDS_LAUNCH_CHECK();
}
