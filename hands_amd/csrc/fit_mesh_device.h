// fit_mesh_device.h -- what the two MANO fits that walk the mesh share beside fit_device.h (fit_verts.hip: the fit to 778
// vertices; fit_surf.hip: the fit to surface correspondences): the state they keep, the sum over the workgroup, the joints of a
// state, the exchanges among the sixteen lanes of a vertex and the way a block of the Gram matrix becomes H and g.  The text is
// fit_verts.hip's own, moved here unchanged; DESIGN.md section 7 "MANO fitting to 778 vertices" specifies it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "fit_device.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef Lds<1> State;                            // the shared state; its data-row arrays (J, r, y, w, sw) are not used here

// the sum over the 256 lanes in a fixed order, on every lane; red: 257 doubles
__device__ double block_sum(double v, double* red, int tid) {
  red[tid] = v;
  __syncthreads();
  if (tid < 64) {
    double a = ((red[tid] + red[tid + 64]) + red[tid + 128]) + red[tid + 192];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if (tid == 0) red[256] = a;
  }
  __syncthreads();
  const double r = red[256];
  __syncthreads();
  return r;
}

// Rest joints, the pose prior's Log(M_j^T R_j), forward kinematics and the 16 joints of state s (the arithmetic of fit.hip's
// kinematics() without the tips).  Ends with a barrier.
__device__ void joint_state(State& S, const hands_mano_fit_verts_consts& C, int s, int tid) {
  const double* R = S.R[s];
  const double* be = S.beta[s];
  if (tid < 48) {
    double a = (double)C.J_template[tid];
#pragma unroll
    for (int l = 0; l < 10; ++l) a += (double)C.J_shapedirs[tid * 10 + l] * be[l];
    S.Jr[tid] = a;
  } else if (tid >= 128 && tid < 143) {
    const int j = tid - 127;
    double D[9], w[3];
    mul_tn(S.M + 9 * j, R + 9 * j, D);
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
      for (int c = 0; c < 3; ++c) S.p[3 * i + c] = S.joints[3 * i + c] = pa[c] = pi[c];
    }
  } else if (tid == 5) {
#pragma unroll
    for (int k = 0; k < 9; ++k) S.Q[k] = R[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) S.p[c] = S.joints[c] = S.Jr[c];
  }
  __syncthreads();
}

// The sixteen lanes of a vertex are one DPP row: their exchanges are DPP moves on the vector pipe, no trip through the LDS crossbar.
// CTRL: 0xB1 quad_perm [1,0,3,2], 0x4E quad_perm [2,3,0,1], 0x141 row_half_mirror, 0x140 row_mirror, 0x100 + n row_shl:n (lane i
// reads lane i + n of its row; a lane whose source lies outside the row reads 0).
template <int CTRL>
__device__ __forceinline__ double row_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// over the sixteen lanes of a vertex: pairs, quads, halves, the row -- every step adds the same two partial sums on both
// lanes of an exchange, so all sixteen end with the same bits
__device__ __forceinline__ double sum16(double v) {
  v += row_move<0xB1>(v);
  v += row_move<0x4E>(v);
  v += row_move<0x141>(v);
  v += row_move<0x140>(v);
  return v;
}

// one block of the Gram matrix into the damped H (rows below 61) and g (row 61), the priors added as in fit.hip
__device__ __forceinline__ void put_block(State& S, const f64x4& a, int bi, int bj, int lane, int s, double lb, double lp, double mu) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int ua = 16 * bi + (lane >> 4) + 4 * r, ub = 16 * bj + (lane & 15);
    double h = a[r];
    if (ua < NU && ub <= ua) {
      if (ua == ub) {
        if (ua >= 3 && ua < UB) h += lp;
        if (ua >= UB && ua < UT) h += lb;
        h += mu * h;
      }
      S.H[ua * (ua + 1) / 2 + ub] = h;
    } else if (ua == NU && ub < NU) {            // g = J^T r, the priors with d Log / d delta = I
      if (ub >= 3 && ub < UB) h += lp * S.lg[ub - 3];
      if (ub >= UB && ub < UT) h += lb * S.beta[s][ub - UB];
      S.g[ub] = h;
    }
  }
}

}  // namespace
