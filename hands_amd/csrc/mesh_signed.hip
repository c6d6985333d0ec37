// mesh_signed.hip -- signed distance from points to a closed triangle surface on device (include/hands_hip.h):
//   hands_mesh_signed_f32   per query point the distance to the mesh, the generalised winding number of the mesh about it and
//                           the closest face; the distance is negative where |winding| >= 0.5.
// The scheme of hands_mesh_closest_f32 (mesh_distance.hip) and its device routines (mesh_distance_device.h): vertices (fp32) and
// faces (16-bit indices) in LDS, a lane owns its queries in registers and walks all faces, skipped faces are skipped by the
// whole wave.  No atomics, no allocation, no synchronisation with the host: the bits depend neither on the run nor on the batch
// around a sample.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"
#include "mesh_distance_device.h"

namespace {

constexpr int QPL_SIGNED = HANDS_SIGNED_CHUNK / NT;  // queries a lane owns: see mesh_signed_kernel
static_assert(HANDS_SIGNED_CHUNK % NT == 0, "a lane owns a whole number of queries");

__host__ __device__ __forceinline__ float root(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(x);              // 1 ulp; only the winding number's lengths, never a distance that is returned
#else
  return sqrtf(x);
#endif
}

// Half the solid angle the triangle v0 v1 v2 subtends at p (Van Oosterom & Strackee 1983): atan2(a . (b x c), |a||b||c| +
// (a.b)|c| + (b.c)|a| + (c.a)|b|) with a = v0 - p, ...; positive where p sees the face from behind (the inside of an outward
// mesh).  Both arguments zero -- p on a vertex of the face -- is 0, whatever the zeros' signs.
__host__ __device__ __forceinline__ float half_solid_angle(const float* v0, const float* v1, const float* v2, const float* p) {
  float a[3], b[3], c[3], x[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { a[k] = v0[k] - p[k]; b[k] = v1[k] - p[k]; c[k] = v2[k] - p[k]; }
  x[0] = b[1] * c[2] - b[2] * c[1];
  x[1] = b[2] * c[0] - b[0] * c[2];
  x[2] = b[0] * c[1] - b[1] * c[0];
  const float la = root(dot3(a, a)), lb = root(dot3(b, b)), lc = root(dot3(c, c));
  const float num = dot3(a, x);
  const float den = fmaf(dot3(c, a), lb, fmaf(dot3(b, c), la, fmaf(dot3(a, b), lc, la * lb * lc)));
  return num == 0.f && den == 0.f ? 0.f : atan2f(num, den);
}

// One face against the lane's queries: the distance, and the face's term of the winding number
template <int THIN>
__device__ __forceinline__ void signed_face(const Face& T, const float* v0, const float* v1, const float* v2, int f,
                                            const float (&p)[QPL_SIGNED][3], float (&m)[QPL_SIGNED], int (&mi)[QPL_SIGNED],
                                            float (&w)[QPL_SIGNED]) {
#pragma unroll
  for (int k = 0; k < QPL_SIGNED; ++k) {
    const float d = tri_dist2<false, THIN>(T, p[k], nullptr);
    if (d < m[k]) {
      m[k] = d;
      mi[k] = f;
    }
    // a face with an exactly zero normal subtends nothing; asked, it would return the rounding residue of a . (b x c)
    // over a denominator that vanishes along its line.  The same for the whole wave
    if (T.plane) w[k] += half_solid_angle(v0, v1, v2, p[k]);
  }
}

// hands_mesh_closest_f32's walk with one more quantity per (query, face).  The winding number costs three square roots and an
// atan2f per pair, about what the distance costs, so the walk stays bound by the vector pipe and a lane owns ONE query: 256 per
// workgroup leave a 778-vertex hand 7 % of idle lanes where 512 leave 24 %, and with 36 KB of LDS four workgroups share a CU
// either way.  The sum runs in ascending face order in the one lane that owns the query: bit-reproducible.
__global__ void __launch_bounds__(NT) mesh_signed_kernel(const float* __restrict__ points, const float* __restrict__ verts,
                                                         const int32_t* __restrict__ faces, const float* __restrict__ valid,
                                                         float* __restrict__ sdf, float* __restrict__ winding,
                                                         int32_t* __restrict__ face_idx, int P, int V, int F, int chunks) {
  __shared__ float Vt[MAXV * 3];
  __shared__ unsigned short Fc[MAXF * 3];
  const int b = blockIdx.x / chunks, q0 = (blockIdx.x % chunks) * HANDS_SIGNED_CHUNK, tid = threadIdx.x;
  const float NaN = __builtin_nanf("");
  const bool live = !valid || valid[b] != 0.f;   // the same for the whole workgroup
  if (live) {
    const float* v = verts + (long long)b * V * 3;
    for (int i = tid; i < V * 3; i += NT) Vt[i] = v[i];
    __syncthreads();
    load_faces(faces, F, V, Vt, true, Fc, tid);
    __syncthreads();
  }
  float p[QPL_SIGNED][3], m[QPL_SIGNED], w[QPL_SIGNED];
  int mi[QPL_SIGNED];
#pragma unroll
  for (int k = 0; k < QPL_SIGNED; ++k) {
    const int q = q0 + tid + k * NT;
    const float* src = points + ((long long)b * P + q) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[k][c] = live && q < P ? src[c] : 0.f;
    m[k] = INFINITY;
    mi[k] = -1;
    w[k] = 0.f;
  }
  if (live && q0 + (tid & ~63) < P)              // a wave without a query has no work
    for (int f = 0; f < F; ++f) {
      const unsigned i0 = Fc[3 * f];
      if (i0 == SKIP) continue;                  // the whole wave
      const float *v0 = Vt + 3 * i0, *v1 = Vt + 3 * Fc[3 * f + 1], *v2 = Vt + 3 * Fc[3 * f + 2];
      const Face T = make_face(v0, v1, v2);
      if (T.thin)                                // the whole wave: a thin face's plane test is fp64 (mesh_distance_device.h)
        signed_face<1>(T, v0, v1, v2, f, p, m, mi, w);
      else
        signed_face<0>(T, v0, v1, v2, f, p, m, mi, w);
    }
#pragma unroll
  for (int k = 0; k < QPL_SIGNED; ++k) {
    const int q = q0 + tid + k * NT;
    if (q >= P) continue;
    const long long o = (long long)b * P + q;
    const bool ok = live && isfinite(p[k][0]) && isfinite(p[k][1]) && isfinite(p[k][2]);
    const float wn = w[k] * 0.15915494309189535f;                          // sum of Omega / 4 pi = sum of the halves / 2 pi
    const float d = sqrtf(m[k]);
    sdf[o] = ok ? (fabsf(wn) >= 0.5f ? -d : d) : NaN;
    if (winding) winding[o] = ok ? wn : NaN;
    if (face_idx) face_idx[o] = ok ? mi[k] : -1;
  }
}

}  // namespace

extern "C" int hands_mesh_signed_f32(const float* points, const float* verts, const int32_t* faces, const float* valid, float* sdf,
                                     float* winding, int32_t* face_idx, int B, int P, int V, int F, hands_stream_t stream) {
  if (!points || !verts || !sdf || (!faces && F != 0)) return HANDS_EINVAL;
  if (B <= 0 || P <= 0 || V <= 0 || F < 0 || V > MAXV || F > MAXF) return HANDS_EINVAL;
  const long long chunks = ((long long)P + HANDS_SIGNED_CHUNK - 1) / HANDS_SIGNED_CHUNK;
  if (chunks * B > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(mesh_signed_kernel, dim3((unsigned)(chunks * B)), dim3(NT), 0, (hipStream_t)stream, points, verts, faces,
                     valid, sdf, winding, face_idx, P, V, F, (int)chunks);
  HANDS_LAUNCH_CHECK();
}
