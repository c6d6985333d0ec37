// mesh_distance.hip -- distances from points to a triangle surface on device (include/hands_hip.h):
//   hands_mesh_closest_f32          per query point the closest point of a triangle mesh: distance, face, point;
//   hands_eval_surface_metrics_f32  point-to-surface error and Chamfer distance of both hands, root- and Procrustes-aligned.
// (hands_mesh_signed_f32, the same walk with the winding number beside it, is mesh_signed.hip; the point-triangle routines
// the two files share are mesh_distance_device.h.)
// Brute force over the faces, in the scheme of vertex_stage (mesh_metrics.hip): the target vertices (fp32) and the face list
// (16-bit indices, V <= 1024) sit in LDS, a lane owns QPL query points in registers and walks all faces, so that one face
// fetched from LDS -- every lane reads the same address, a broadcast -- and the quantities that depend on the face alone (edges,
// normal, reciprocals) feed QPL point-triangle evaluations.  The per-face work has no divergent exit: a face that is skipped
// (an index outside [0, V), a non-finite vertex) is skipped by the whole wave.  Squared distances and their comparison are
// fp32, one square root per query at the end.  Sums are fp64 through one fixed tree, no atomics: the bits depend neither on the
// run nor on the batch around a sample.
//
// Point to triangle a, b, c: the minimum of the three clamped segment distances (ab, ac, bc) and -- when the normal is not zero
// and the projection of the point falls inside the triangle -- of the distance to the plane.  A face with a repeated index or
// collinear vertices has an exactly zero normal in fp32 (ab x ab, products and differences of equal numbers: the library is
// built with -ffp-contract=off, a fused multiply-add would leave its rounding residue there) and is the segment
// or the point it collapses to without a special case; a zero edge has the parameter 0.  A NEARLY degenerate face -- thin: the
// sine of the angle at its first vertex is at most 1/64 -- takes "falls inside" and the plane distance in fp64 from its fp32
// vertices, because the fp32 barycentrics of such a face are rounding noise (mesh_distance_device.h has the reasoning and the
// threshold).  The flag belongs to the face, so a wave takes that branch together, once per face.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "procrustes_device.h"
#include "mesh_distance_device.h"

namespace {

constexpr int NW = NT / 64;
constexpr int QPL_CLOSEST = HANDS_SURF_CHUNK / NT;  // queries a lane owns: the primitive ...
constexpr int QPL_METRIC = MAXV / NT;            // ... and the metrics, where a workgroup holds a whole hand
constexpr int NJ = 21;
constexpr int NRED = 10;                         // widest reduction (K and var1)
static_assert(HANDS_SURF_CHUNK % NT == 0 && MAXV % NT == 0, "a lane owns a whole number of queries");

// One face against the lane's Q queries
template <int Q, bool IDX, int THIN>
__device__ __forceinline__ void scan_face(const Face& T, int f, const float (&p)[Q][3], float (&m)[Q], int (&mi)[Q]) {
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const float d = tri_dist2<false, THIN>(T, p[k], nullptr);
    if (d < m[k]) {
      m[k] = d;
      if (IDX) mi[k] = f;
    }
  }
}

// All faces against the lane's Q queries: m = smallest squared distance, mi = its face (strict <, ascending: the lowest index
// wins an exact tie).  Every lane of the wave reads the same addresses.
template <int Q, bool IDX>
__device__ __forceinline__ void scan_faces(const float* Vt, const unsigned short* Fc, int F, const float (&p)[Q][3], float (&m)[Q],
                                           int (&mi)[Q]) {
  for (int f = 0; f < F; ++f) {
    const unsigned i0 = Fc[3 * f];
    if (i0 == SKIP) continue;                    // the whole wave
    const Face T = make_face(Vt + 3 * i0, Vt + 3 * Fc[3 * f + 1], Vt + 3 * Fc[3 * f + 2]);
    if (T.thin)                                  // the whole wave
      scan_face<Q, IDX, 1>(T, f, p, m, mi);
    else
      scan_face<Q, IDX, 0>(T, f, p, m, mi);
  }
}

// ---- the primitive ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) mesh_closest_kernel(const float* __restrict__ points, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ faces, const float* __restrict__ valid,
                                                          float* __restrict__ dist, int32_t* __restrict__ face_idx,
                                                          float* __restrict__ closest, int P, int V, int F, int chunks) {
  __shared__ float Vt[MAXV * 3];
  __shared__ unsigned short Fc[MAXF * 3];
  const int b = blockIdx.x / chunks, q0 = (blockIdx.x % chunks) * HANDS_SURF_CHUNK, tid = threadIdx.x;
  const float NaN = __builtin_nanf("");
  const bool live = !valid || valid[b] != 0.f;   // the same for the whole workgroup
  if (live) {
    const float* v = verts + (long long)b * V * 3;
    for (int i = tid; i < V * 3; i += NT) Vt[i] = v[i];
    __syncthreads();
    load_faces(faces, F, V, Vt, true, Fc, tid);
    __syncthreads();
  }
  float p[QPL_CLOSEST][3], m[QPL_CLOSEST];
  int mi[QPL_CLOSEST];
#pragma unroll
  for (int k = 0; k < QPL_CLOSEST; ++k) {
    const int q = q0 + tid + k * NT;
    const float* src = points + ((long long)b * P + q) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[k][c] = live && q < P ? src[c] : 0.f;
    m[k] = INFINITY;
    mi[k] = -1;
  }
  if (live && q0 + (tid & ~63) < P) scan_faces<QPL_CLOSEST, true>(Vt, Fc, F, p, m, mi);   // a wave without a query has no work
#pragma unroll
  for (int k = 0; k < QPL_CLOSEST; ++k) {
    const int q = q0 + tid + k * NT;
    if (q >= P) continue;
    const long long o = (long long)b * P + q;
    const bool ok = live && isfinite(p[k][0]) && isfinite(p[k][1]) && isfinite(p[k][2]);
    const int f = ok ? mi[k] : -1;
    float c[3] = {NaN, NaN, NaN};
    if (f >= 0) {
      const Face T = make_face(Vt + 3 * Fc[3 * f], Vt + 3 * Fc[3 * f + 1], Vt + 3 * Fc[3 * f + 2]);
      tri_dist2<true>(T, p[k], c);
    }
    dist[o] = ok ? sqrtf(m[k]) : NaN;
    if (face_idx) face_idx[o] = f;
    if (closest)
      for (int a = 0; a < 3; ++a) closest[3 * o + a] = c[a];
  }
}

// ---- the metrics -----------------------------------------------------------------------------------------------------------
struct SurfLds {
  float X[MAXV * 3], Y[MAXV * 3];                // root-aligned prediction (pa: Procrustes-aligned) and ground truth
  unsigned short Fc[MAXF * 3];
  double red[NW][NRED];
  double xf[13];                                 // scale, R (9), t (3) of the vertex fit
  int any_face;
};

// sum over the NT lanes, valid on all of them: shuffle tree inside each wave, then the waves in order (half_sum of
// mesh_metrics.hip)
template <int N>
__device__ void block_sum(double (&v)[N], double (*red)[NRED], int tid) {
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

// One workgroup per (sample, hand, alignment): blockIdx.x = 4 b + 2 hand + (0: ra, 1: pa).  It writes p2s and chamfer of its
// hand and alignment; surface_h_kernel forms h afterwards.
__global__ void __launch_bounds__(NT) surface_metrics_kernel(hands_mesh_eval_in in, const int32_t* __restrict__ faces_r,
                                                             const int32_t* __restrict__ faces_l, int F_r, int F_l,
                                                             hands_surf_eval_out out, int V) {
  __shared__ SurfLds S;
  const int b = blockIdx.x >> 2, hand = (blockIdx.x >> 1) & 1, pa = blockIdx.x & 1, tid = threadIdx.x;
  const float NaN = __builtin_nanf("");
  float* const* o = reinterpret_cast<float* const*>(&out);
  float* o_p2s = o[3 * pa + hand] + b;           // quantities: p2s_ra, p2s_pa, chamfer_ra, chamfer_pa
  float* o_chamfer = o[3 * (2 + pa) + hand] + b;
  const bool live = in.is_valid[b] * (hand ? in.left_valid[b] : in.right_valid[b]) != 0.f;
  if (!live) {                                   // the whole workgroup: nothing of the hand is read
    if (tid == 0) *o_p2s = *o_chamfer = NaN;
    return;
  }
  const float* pv = (hand ? in.pred_v3d_l : in.pred_v3d_r) + (long long)b * V * 3;
  const float* gv = (hand ? in.gt_v3d_l : in.gt_v3d_r) + (long long)b * V * 3;
  const float* pj = (hand ? in.pred_j3d_l : in.pred_j3d_r) + (long long)b * NJ * 3;
  const float* gj = (hand ? in.gt_j3d_l : in.gt_j3d_r) + (long long)b * NJ * 3;
  const int32_t* faces = hand ? faces_l : faces_r;
  const int F = hand ? F_l : F_r;

  // ---- load and root-align in fp32, as mesh_metrics_kernel; `bad` counts the non-finite coordinates, the joints' included
  float pr0[3], gr0[3];
  for (int c = 0; c < 3; ++c) { pr0[c] = pj[c]; gr0[c] = gj[c]; }
  int bad = 0;
  for (int i = tid; i < V * 3; i += NT) {
    const float x = pv[i], y = gv[i];
    bad += (isfinite(x) ? 0 : 1) + (isfinite(y) ? 0 : 1);
    S.X[i] = x - pr0[i % 3];
    S.Y[i] = y - gr0[i % 3];
  }
  if (tid < NJ * 3) bad += (isfinite(pj[tid]) ? 0 : 1) + (isfinite(gj[tid]) ? 0 : 1);
  if (tid == 0) S.any_face = 0;
  __syncthreads();
  if (load_faces(faces, F, V, nullptr, false, S.Fc, tid) > 0) S.any_face = 1;   // every writer stores the same value

  float p[QPL_METRIC][3], g[QPL_METRIC][3];
  int n_own = 0;
#pragma unroll
  for (int k = 0; k < QPL_METRIC; ++k) {
    const int q = tid + k * NT;
    const bool own = q < V;
    n_own += own ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      p[k][c] = own ? S.X[3 * q + c] : 0.f;
      g[k][c] = own ? S.Y[3 * q + c] : 0.f;
    }
  }

  // ---- means (and the count of bad coordinates); pa: the similarity transform of mesh_metrics_kernel, operation by operation
  double m[7] = {0, 0, 0, 0, 0, 0, (double)bad};
#pragma unroll
  for (int k = 0; k < QPL_METRIC; ++k)
    if (k < n_own)
      for (int c = 0; c < 3; ++c) { m[c] += (double)p[k][c]; m[3 + c] += (double)g[k][c]; }
  block_sum(m, S.red, tid);                      // its barriers also close the face load
  const bool hand_bad = m[6] != 0.0;
  bool fit_finite = true;
  if (pa) {
    double mu1[3], mu2[3];
    for (int c = 0; c < 3; ++c) { mu1[c] = m[c] / (double)V; mu2[c] = m[3 + c] / (double)V; }
    double kv[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};                        // K row-major, var1
#pragma unroll
    for (int k = 0; k < QPL_METRIC; ++k)
      if (k < n_own)
        for (int a = 0; a < 3; ++a) {
          const double x1 = (double)p[k][a] - mu1[a];
          kv[9] += x1 * x1;
          for (int c = 0; c < 3; ++c) kv[3 * a + c] += x1 * ((double)g[k][c] - mu2[c]);
        }
    block_sum(kv, S.red, tid);
    if (tid < 64) {                                                        // wave 0: the fit, every lane the same
      double K[3][3], R[3][3], scale;
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) K[a][c] = kv[3 * a + c];
      procrustes_solve(K, kv[9], R, &scale);     // inlined: no stack, and the walks below still keep three waves per SIMD
      if (tid == 0) {
        S.xf[0] = scale;
        for (int a = 0; a < 3; ++a) {
          for (int c = 0; c < 3; ++c) S.xf[1 + 3 * a + c] = R[a][c];
          S.xf[10 + a] = mu2[a] - scale * (R[a][0] * mu1[0] + R[a][1] * mu1[1] + R[a][2] * mu1[2]);
        }
      }
    }
    __syncthreads();
    const double scale = S.xf[0];
#pragma unroll
    for (int k = 0; k < QPL_METRIC; ++k)
      if (k < n_own) {
        float h[3];
        for (int a = 0; a < 3; ++a)
          h[a] = (float)(scale * (S.xf[1 + 3 * a] * (double)p[k][0] + S.xf[2 + 3 * a] * (double)p[k][1] +
                                  S.xf[3 + 3 * a] * (double)p[k][2]) + S.xf[10 + a]);
        for (int a = 0; a < 3; ++a) S.X[3 * (tid + k * NT) + a] = p[k][a] = h[a];
      }
    for (int i = 0; i < 13; ++i) fit_finite = fit_finite && isfinite(S.xf[i]);
    __syncthreads();
  }

  // ---- Chamfer: nearest vertex, both directions in one walk (vertex_stage of mesh_metrics.hip)
  float c1[QPL_METRIC], c2[QPL_METRIC], s1[QPL_METRIC], s2[QPL_METRIC];
  int unused[QPL_METRIC];
#pragma unroll
  for (int k = 0; k < QPL_METRIC; ++k) c1[k] = c2[k] = s1[k] = s2[k] = INFINITY;
#pragma unroll 2
  for (int j = 0; j < V; ++j) {
    const float px = S.X[3 * j], py = S.X[3 * j + 1], pz = S.X[3 * j + 2];
    const float gx = S.Y[3 * j], gy = S.Y[3 * j + 1], gz = S.Y[3 * j + 2];
#pragma unroll
    for (int k = 0; k < QPL_METRIC; ++k) {
      const float ax = g[k][0] - px, ay = g[k][1] - py, az = g[k][2] - pz;
      const float bx = p[k][0] - gx, by = p[k][1] - gy, bz = p[k][2] - gz;
      c1[k] = fminf(c1[k], (ax * ax + ay * ay) + az * az);
      c2[k] = fminf(c2[k], (bx * bx + by * by) + bz * bz);
    }
  }
  // ---- point to surface: the prediction against the ground-truth surface, then the other way round.  A hand with a
  //      non-finite coordinate is NaN anyway and would only feed NaN through the walk
  if (!hand_bad) {
    scan_faces<QPL_METRIC, false>(S.Y, S.Fc, F, p, s1, unused);
    scan_faces<QPL_METRIC, false>(S.X, S.Fc, F, g, s2, unused);
  }
  double v[4] = {0, 0, 0, 0};                    // sums of: X -> nearest Y, Y -> nearest X, X -> surface(Y), Y -> surface(X)
#pragma unroll
  for (int k = 0; k < QPL_METRIC; ++k)
    if (k < n_own) {
      v[0] += (double)sqrtf(c2[k]);
      v[1] += (double)sqrtf(c1[k]);
      v[2] += (double)sqrtf(s1[k]);
      v[3] += (double)sqrtf(s2[k]);
    }
  block_sum(v, S.red, tid);
  if (tid == 0) {
    const double n = (double)V;
    const bool ok = !hand_bad && fit_finite;     // a constant prediction: scale = 0 / 0, NaN in the pa outputs
    *o_chamfer = ok ? (float)(1000.0 * (0.5 * (v[0] / n + v[1] / n))) : NaN;
    *o_p2s = ok && S.any_face ? (float)(1000.0 * (0.5 * (v[2] / n + v[3] / n))) : NaN;
  }
}

__device__ __forceinline__ float nanmean2(float a, float b) {
  const bool na = isnan(a), nb = isnan(b);
  return ((na ? 0.f : a) + (nb ? 0.f : b)) / (float)((na ? 0 : 1) + (nb ? 0 : 1));
}

__global__ void surface_h_kernel(hands_surf_eval_out out, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * HANDS_SURF_NQ) return;
  const int q = i / B, b = i % B;
  float* const* o = reinterpret_cast<float* const*>(&out);
  o[3 * q + 2][b] = nanmean2(o[3 * q][b], o[3 * q + 1][b]);
}

}  // namespace

extern "C" int hands_mesh_closest_f32(const float* points, const float* verts, const int32_t* faces, const float* valid,
                                      float* dist, int32_t* face_idx, float* closest, int B, int P, int V, int F,
                                      hands_stream_t stream) {
  if (!points || !verts || !dist || (!faces && F != 0)) return HANDS_EINVAL;
  if (B <= 0 || P <= 0 || V <= 0 || F < 0 || V > MAXV || F > MAXF) return HANDS_EINVAL;
  const long long chunks = ((long long)P + HANDS_SURF_CHUNK - 1) / HANDS_SURF_CHUNK;
  if (chunks * B > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(mesh_closest_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, (hipStream_t)stream, points, verts, faces,
                     valid, dist, face_idx, closest, P, V, F, (int)chunks);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_eval_surface_metrics_f32(const hands_mesh_eval_in* in, const int32_t* faces_r, const int32_t* faces_l,
                                              int F_r, int F_l, const hands_surf_eval_out* out, int B, int V,
                                              hands_stream_t stream) {
  static_assert(sizeof(hands_surf_eval_out) == 3 * HANDS_SURF_NQ * sizeof(void*), "three pointers per quantity");
  if (!in || !out || B <= 0 || B > 0x7fffffff / 4 || V < 1 || V > MAXV) return HANDS_EINVAL;
  if (F_r < 0 || F_l < 0 || F_r > MAXF || F_l > MAXF || (!faces_r && F_r != 0) || (!faces_l && F_l != 0)) return HANDS_EINVAL;
  const void* const* pi = reinterpret_cast<const void* const*>(in);
  for (size_t i = 0; i < sizeof(hands_mesh_eval_in) / sizeof(void*); ++i)
    if (!pi[i]) return HANDS_EINVAL;
  const void* const* po = reinterpret_cast<const void* const*>(out);
  for (size_t i = 0; i < sizeof(hands_surf_eval_out) / sizeof(void*); ++i)
    if (!po[i]) return HANDS_EINVAL;
  hipLaunchKernelGGL(surface_metrics_kernel, dim3(4 * B), dim3(NT), 0, (hipStream_t)stream, *in, faces_r, faces_l, F_r, F_l, *out, V);
  const int n = B * HANDS_SURF_NQ;
  hipLaunchKernelGGL(surface_h_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *out, B);
  HANDS_LAUNCH_CHECK();
}
