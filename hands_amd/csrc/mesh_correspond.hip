// mesh_correspond.hip -- closest point with what a fit needs (hands_mesh_correspond_f32 of include/hands_hip.h): the walk of
// hands_mesh_closest_f32 (mesh_distance.hip) over the faces -- vertices and 16-bit faces in LDS, a lane owns its queries in
// registers, squared distances and their comparison in fp32, strict < in ascending face order -- and, for the face that won, the
// coefficients of the closest point, the face's unit normal and the gated weight.  The distance, the face and the point come from
// tri_dist2 of mesh_distance_device.h with the template arguments mesh_distance.hip gives it, so they are that entry's bits.
// The coefficients repeat tri_dist2's choice of the candidate -- plane, then ab, ac, bc: the first of equal ones -- and are
// written in that candidate's own arithmetic, so a degenerate or a thin face needs no second rule.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "mesh_distance_device.h"

namespace {

constexpr int QPL = HANDS_SURF_CHUNK / NT;       // queries a lane owns
static_assert(HANDS_SURF_CHUNK % NT == 0, "a lane owns a whole number of queries");

// The coefficients of the point tri_dist2<true> returns for face f and query p.
__device__ __forceinline__ void tri_bary(const Face& f, const float* p, float* b) {
  float ap[3], bp[3], q1[3], q2[3], q3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ap[k] = p[k] - f.a[k]; bp[k] = p[k] - f.b[k]; }
  const float d1 = dot3(ap, f.ab), d2 = dot3(ap, f.ac), d3 = dot3(bp, f.bc);
  const float t1 = clamp01(d1 * f.iab), t2 = clamp01(d2 * f.iac), t3 = clamp01(d3 * f.ibc);
#pragma unroll
  for (int k = 0; k < 3; ++k) { q1[k] = fmaf(-t1, f.ab[k], ap[k]); q2[k] = fmaf(-t2, f.ac[k], ap[k]); q3[k] = fmaf(-t3, f.bc[k], bp[k]); }
  const float e1 = dot3(q1, q1), e2 = dot3(q2, q2), e3 = dot3(q3, q3);
  const float nv = fmaf(f.d11, d1, -(f.d01 * d2)), nw = fmaf(f.d00, d2, -(f.d01 * d1));
  const float dn = dot3(ap, f.n), s = dn * f.inn;
  float pl = dn * s;
  bool inside = f.plane && nv >= 0.f && nw >= 0.f && nv + nw <= f.den;
  float v = nv / f.den, w = nw / f.den;          // read only where inside holds: den > 0 there
  if (f.thin) {                                  // thin_plane's fp64 barycentrics from the fp32 vertices
    inside = thin_plane<false>(f, p, &pl, nullptr);
    double ab[3], ac[3], pa[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      ab[k] = (double)f.b[k] - (double)f.a[k];
      ac[k] = ab[k] + (double)f.bc[k];
      pa[k] = (double)p[k] - (double)f.a[k];
    }
    const double d00 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], d01 = ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2];
    const double d11 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
    const double g1 = pa[0] * ab[0] + pa[1] * ab[1] + pa[2] * ab[2], g2 = pa[0] * ac[0] + pa[1] * ac[1] + pa[2] * ac[2];
    const double den = d00 * d11 - d01 * d01;
    v = (float)((d11 * g1 - d01 * g2) / den);
    w = (float)((d00 * g2 - d01 * g1) / den);
  }
  const float e = fminf(fminf(e1, e2), e3);
  if (inside && pl <= e) {
    b[0] = (1.f - v) - w; b[1] = v; b[2] = w;
  } else if (e1 <= e) {
    b[0] = 1.f - t1; b[1] = t1; b[2] = 0.f;
  } else if (e2 <= e) {
    b[0] = 1.f - t2; b[1] = 0.f; b[2] = t2;
  } else {
    b[0] = 0.f; b[1] = 1.f - t3; b[2] = t3;
  }
}

__global__ void __launch_bounds__(NT) mesh_correspond_kernel(const float* __restrict__ points, const float* __restrict__ verts,
                                                             const int32_t* __restrict__ faces, const float* __restrict__ valid,
                                                             const float* __restrict__ w_in, float max_dist, float* __restrict__ dist,
                                                             int32_t* __restrict__ face_idx, float* __restrict__ closest,
                                                             float* __restrict__ bary, float* __restrict__ normal,
                                                             float* __restrict__ w_out, int P, int V, int F, int chunks) {
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
  float p[QPL][3], m[QPL], wq[QPL];
  int mi[QPL];
  bool read[QPL];
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int q = q0 + tid + k * NT;
    const long long o = (long long)b * P + q;
    wq[k] = q < P ? (w_in ? w_in[o] : 1.f) : 0.f;
    read[k] = live && q < P && wq[k] > 0.f;      // a query of weight 0 (or of a weight that is no number) is not read
#pragma unroll
    for (int c = 0; c < 3; ++c) p[k][c] = read[k] ? points[3 * o + c] : 0.f;
    m[k] = INFINITY;
    mi[k] = -1;
  }
  if (live && q0 + (tid & ~63) < P) {            // a wave without a query has no work
    for (int f = 0; f < F; ++f) {
      const unsigned i0 = Fc[3 * f];
      if (i0 == SKIP) continue;                  // the whole wave
      const Face T = make_face(Vt + 3 * i0, Vt + 3 * Fc[3 * f + 1], Vt + 3 * Fc[3 * f + 2]);
#pragma unroll
      for (int k = 0; k < QPL; ++k) {
        const float d = T.thin ? tri_dist2<false, 1>(T, p[k], nullptr) : tri_dist2<false, 0>(T, p[k], nullptr);   // the whole wave
        if (d < m[k]) {
          m[k] = d;
          mi[k] = f;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int q = q0 + tid + k * NT;
    if (q >= P) continue;
    const long long o = (long long)b * P + q;
    const bool ok = read[k] && isfinite(p[k][0]) && isfinite(p[k][1]) && isfinite(p[k][2]);
    const int f = ok ? mi[k] : -1;
    float c[3] = {NaN, NaN, NaN}, bc[3] = {NaN, NaN, NaN}, n[3] = {0.f, 0.f, 0.f};
    if (f >= 0) {
      const Face T = make_face(Vt + 3 * Fc[3 * f], Vt + 3 * Fc[3 * f + 1], Vt + 3 * Fc[3 * f + 2]);
      tri_dist2<true>(T, p[k], c);
      tri_bary(T, p[k], bc);
      if (T.plane) {
        const float r = 1.f / sqrtf(dot3(T.n, T.n));
#pragma unroll
        for (int a = 0; a < 3; ++a) n[a] = T.n[a] * r;
      }
    }
    const float d = ok ? sqrtf(m[k]) : NaN;
    dist[o] = d;
    face_idx[o] = f;
    const bool gate = wq[k] > 0.f && (max_dist <= 0.f || d <= max_dist);
    w_out[o] = gate ? wq[k] : 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      closest[3 * o + a] = c[a];
      bary[3 * o + a] = bc[a];
      normal[3 * o + a] = n[a];
    }
  }
}

}  // namespace

extern "C" int hands_mesh_correspond_f32(const float* points, const float* verts, const int32_t* faces, const float* valid,
                                         const float* w_in, float max_dist, float* dist, int32_t* face_idx, float* closest,
                                         float* bary, float* normal, float* w_out, int B, int P, int V, int F, hands_stream_t stream) {
  if (!points || !verts || !dist || !face_idx || !closest || !bary || !normal || !w_out || (!faces && F != 0)) return HANDS_EINVAL;
  if (B <= 0 || P <= 0 || V <= 0 || F < 0 || V > MAXV || F > MAXF || max_dist != max_dist) return HANDS_EINVAL;
  const long long chunks = ((long long)P + HANDS_SURF_CHUNK - 1) / HANDS_SURF_CHUNK;
  if (chunks * B > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(mesh_correspond_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, (hipStream_t)stream, points, verts, faces,
                     valid, w_in, max_dist, dist, face_idx, closest, bary, normal, w_out, P, V, F, (int)chunks);
  HANDS_LAUNCH_CHECK();
}
