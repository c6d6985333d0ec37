// procrustes_device.h -- the rank-safe orthogonal-Procrustes solve shared by metrics.hip (21 or fewer joints per hand) and
// mesh_metrics.hip (V vertices per hand): cross-covariance K and variance var1 of the centred source points -> rotation R and
// scale of compute_similarity_transform (src/utils/eval_modules.py:136-187), all in fp64.
// Rank-deficient K: the rotation is V diag(1,1,det V) U^T with U an orthonormal frame whatever the rank of K.  Rank 2 (planar
// points): U_2 = U_0 x U_1.  Rank 1 (source or target points on a line): U_1 is completed from the unit axis least aligned
// with U_0; the error does not depend on the completion and equals the one of the reference's LAPACK SVD.  K = 0: constant
// source points give NaN (scale = 0 / 0, as the reference), constant target points give scale 0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// symmetric 3x3 eigen-decomposition by cyclic Jacobi (fp64): A = V diag(w) V^T
static __device__ void jacobi3(double A[3][3], double V[3][3], double w[3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
    if (off < 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; ++k) {           // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 3; ++k) {           // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// K[a][b] = sum_j X1[j][a] X2[j][b], var1 = sum_j |X1[j]|^2 of the centred points  ->  R, scale = trace(R K) / var1
static __device__ void procrustes_solve(const double K[3][3], double var1, double R[3][3], double* scale_out) {
  // K = U S V^T; eigen-decompose K^T K = V S^2 V^T
  double A[3][3], V[3][3], w[3];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) A[a][b] = K[0][a] * K[0][b] + K[1][a] * K[1][b] + K[2][a] * K[2][b];
  jacobi3(A, V, w);
  int o[3] = {0, 1, 2};                                  // sort singular values descending
  for (int i = 0; i < 2; ++i)
    for (int j = i + 1; j < 3; ++j)
      if (w[o[j]] > w[o[i]]) { const int t = o[i]; o[i] = o[j]; o[j] = t; }
  double Vs[3][3], U[3][3];
  for (int i = 0; i < 3; ++i)
    for (int r = 0; r < 3; ++r) Vs[r][i] = V[r][o[i]];
  // U is an orthonormal frame whatever the rank of K.  U_0 = K V_0 / |K V_0| (e_x when K = 0: scale is 0 or NaN then and the
  // frame does not matter).  U_1 = K V_1 made orthogonal to U_0; when what is left is below 1e-10 |K V_0| -- K has rank 1: the
  // source or the target points lie on a line, and K V_1 is zero or rounding noise parallel to U_0 -- the unit axis
  // least aligned with U_0 takes its place.  Any orthonormal completion gives the same error there, as for LAPACK's.
  double u0[3], u1[3], n0 = 0;
  for (int r = 0; r < 3; ++r) {
    u0[r] = K[r][0] * Vs[0][0] + K[r][1] * Vs[1][0] + K[r][2] * Vs[2][0];
    u1[r] = K[r][0] * Vs[0][1] + K[r][1] * Vs[1][1] + K[r][2] * Vs[2][1];
    n0 += u0[r] * u0[r];
  }
  n0 = sqrt(n0);
  for (int r = 0; r < 3; ++r) U[r][0] = n0 > 0 ? u0[r] / n0 : (r == 0 ? 1.0 : 0.0);
  for (int pass = 0; pass < 2; ++pass) {
    double n1 = 0;
    for (int again = 0; again < 2; ++again) {            // Gram-Schmidt twice: the first pass may cancel almost everything
      const double d = u1[0] * U[0][0] + u1[1] * U[1][0] + u1[2] * U[2][0];
      for (int r = 0; r < 3; ++r) u1[r] -= d * U[r][0];
    }
    for (int r = 0; r < 3; ++r) n1 += u1[r] * u1[r];
    n1 = sqrt(n1);
    if (pass == 1 || (n0 > 0 && n1 > 1e-10 * n0)) {
      for (int r = 0; r < 3; ++r) U[r][1] = u1[r] / n1;
      break;
    }
    int ax = 0;
    for (int r = 1; r < 3; ++r)
      if (fabs(U[r][0]) < fabs(U[ax][0])) ax = r;
    for (int r = 0; r < 3; ++r) u1[r] = r == ax ? 1.0 : 0.0;
  }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];      // U_3 = U_1 x U_2  (det U = +1)
  U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
  U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  const double detV = Vs[0][0] * (Vs[1][1] * Vs[2][2] - Vs[1][2] * Vs[2][1]) -
                      Vs[0][1] * (Vs[1][0] * Vs[2][2] - Vs[1][2] * Vs[2][0]) +
                      Vs[0][2] * (Vs[1][0] * Vs[2][1] - Vs[1][1] * Vs[2][0]);
  const double z = detV >= 0 ? 1.0 : -1.0;               // R = V diag(1,1,det V) U^T maximises trace(R K)
  double tr = 0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) R[a][b] = Vs[a][0] * U[b][0] + Vs[a][1] * U[b][1] + z * Vs[a][2] * U[b][2];
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) tr += R[a][b] * K[b][a];
  *scale_out = tr / var1;
}
