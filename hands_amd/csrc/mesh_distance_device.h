// mesh_distance_device.h -- what mesh_distance.hip (closest point, surface metrics) and mesh_signed.hip (signed distance) share:
// the limits and the workgroup size, the per-face quantities, the point-triangle distance and the face load into LDS.  The
// definition of the distance and of a degenerate face is at the top of mesh_distance.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"

namespace {

constexpr int MAXV = HANDS_MESH_MAX_V;
constexpr int MAXF = HANDS_SURF_MAX_F;
constexpr int NT = 256;                          // lanes of a workgroup, every kernel
constexpr unsigned short SKIP = 0xFFFF;          // first index of a face that is not to be used
static_assert(MAXV <= 0xFFFF, "vertex indices are kept in 16 bits");

// The dot products and the points on a segment are written with fmaf: a third fewer instructions in the face walk, which runs at
// the rate of the fp32 vector pipe, and one rounding less each.  The normal is NOT: its exact zero (above) needs both products rounded.
__host__ __device__ __forceinline__ float dot3(const float* a, const float* b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
__host__ __device__ __forceinline__ float clamp01(float t) { return fminf(fmaxf(t, 0.f), 1.f); }   // NaN (0 * inf) gives 0
__host__ __device__ __forceinline__ float recip(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);               // 1 ulp: moves a distance by 1e-7 of itself at the most
#else
  return 1.0f / x;
#endif
}

// A face is THIN when the angle A at its first vertex has sin A <= 1/64 (within 0.9 degrees of 0 or of 180): den <= THIN_SIN2 x
// d00 d11, as den = d00 d11 sin^2 A.  The fp32 plane test of tri_dist2 forms nv, nw and den as differences of products that
// nearly cancel; their rounding, 2^-23 of a product, is 2^-23 |ap| / (|ab| sin^2 A) of the barycentric and moves the border of
// "inside" by about 2^-23 |ap| / sin A metres -- which is what a query in the face's plane beside that border then gets wrong.
// Above the threshold that stays small: 1.7e-7 m at the most over 27 million queries about faces with 0.1 m edges and heights
// of 0.2 % to 6 % of them, a tenth of that at a hand's size (docs/EXPERIMENTS.md).  Below it the noise grows until it decides
// the test for queries far outside the face, which then get the distance to the PLANE, up to 100 % too small.  A sliver or a
// cap is thin from whichever vertex it starts: its angles are all near 0 or 180 degrees.  A needle is thin only from its sharp
// vertex and exact from the other two.  A thin face takes the plane test in fp64 from its fp32 vertices (thin_plane): the
// same noise is 2^-52 / sin^2 A, under 1e-3 of the barycentric down to a height of 1e-6 of the edge.  The flag depends on the
// face alone, so a wave takes one side of the branch together.
constexpr float THIN_SIN2 = 1.f / 4096.f;

// What the queries of a lane share of one triangle
struct Face {
  float a[3], b[3], ab[3], ac[3], bc[3], n[3];
  float iab, iac, ibc, inn;                      // 1 / |ab|^2, ... (0 for a zero edge); 1 / |n|^2
  float d00, d01, d11, den;                      // ab.ab, ab.ac, ac.ac and d00 d11 - d01^2 of the barycentric test
  bool plane;                                    // the normal is not zero
  bool thin;                                     // ... and the face is thin (above)
};

__host__ __device__ __forceinline__ Face make_face(const float* a, const float* b, const float* c) {
  Face f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f.a[k] = a[k];
    f.b[k] = b[k];
    f.ab[k] = b[k] - a[k];
    f.ac[k] = c[k] - a[k];
    f.bc[k] = c[k] - b[k];
  }
  f.n[0] = f.ab[1] * f.ac[2] - f.ab[2] * f.ac[1];
  f.n[1] = f.ab[2] * f.ac[0] - f.ab[0] * f.ac[2];
  f.n[2] = f.ab[0] * f.ac[1] - f.ab[1] * f.ac[0];
  f.d00 = dot3(f.ab, f.ab);
  f.d01 = dot3(f.ab, f.ac);
  f.d11 = dot3(f.ac, f.ac);
  const float d22 = dot3(f.bc, f.bc), nn = dot3(f.n, f.n);
  f.den = fmaf(f.d00, f.d11, -(f.d01 * f.d01));
  f.iab = f.d00 > 0.f ? recip(f.d00) : 0.f;
  f.iac = f.d11 > 0.f ? recip(f.d11) : 0.f;
  f.ibc = d22 > 0.f ? recip(d22) : 0.f;
  f.plane = nn > 0.f;
  f.inn = f.plane ? recip(nn) : 0.f;
  f.thin = f.plane && f.den <= THIN_SIN2 * (f.d00 * f.d11);
  return f;
}

// The plane test of a thin face in fp64.  The vertices are read back from the edges' ends: a and b as they are, c = b + bc
// exactly wherever the fp32 difference bc was exact, and within its rounding -- 2^-24 |bc|, in the face's plane and across it
// alike -- where it was not.  Returns "the projection of p falls inside the face"; *pl the squared distance to the plane, cp
// the projection.  A normal that is zero in fp64 is outside (0 / 0 is not compared).
template <bool POINT>
__host__ __device__ __forceinline__ bool thin_plane(const Face& f, const float* p, float* pl, float* cp) {
  double ab[3], ac[3], ap[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ab[k] = (double)f.b[k] - (double)f.a[k];
    ac[k] = ab[k] + (double)f.bc[k];
    ap[k] = (double)p[k] - (double)f.a[k];
  }
  n[0] = ab[1] * ac[2] - ab[2] * ac[1];
  n[1] = ab[2] * ac[0] - ab[0] * ac[2];
  n[2] = ab[0] * ac[1] - ab[1] * ac[0];
  const double d00 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2], d01 = ab[0] * ac[0] + ab[1] * ac[1] + ab[2] * ac[2];
  const double d11 = ac[0] * ac[0] + ac[1] * ac[1] + ac[2] * ac[2];
  const double d1 = ap[0] * ab[0] + ap[1] * ab[1] + ap[2] * ab[2], d2 = ap[0] * ac[0] + ap[1] * ac[1] + ap[2] * ac[2];
  const double nv = d11 * d1 - d01 * d2, nw = d00 * d2 - d01 * d1, den = d00 * d11 - d01 * d01;
  const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2], dn = ap[0] * n[0] + ap[1] * n[1] + ap[2] * n[2];
  const double s = dn / nn;
  *pl = (float)(dn * s);
  if (POINT) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = (float)((double)p[k] - s * n[k]);
  }
  return nn > 0.0 && nv >= 0.0 && nw >= 0.0 && nv + nw <= den;
}

// Squared distance from p to the closed triangle; with `c` also the closest point, from the candidate that gave the minimum
// (plane, then ab, ac, bc: the first of equal ones).  THIN: 0 / 1 where the caller has asked f.thin already -- the face walks,
// which branch once per face and so keep the fp64 registers out of their fp32 side -- and -1 to ask it here.
template <bool POINT, int THIN = -1>
__host__ __device__ __forceinline__ float tri_dist2(const Face& f, const float* p, float* c) {
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
  float pl = dn * s, cp[3];
  bool inside = f.plane && nv >= 0.f && nw >= 0.f && nv + nw <= f.den;
  if (POINT) {
#pragma unroll
    for (int k = 0; k < 3; ++k) cp[k] = fmaf(-s, f.n[k], p[k]);
  }
  if (THIN < 0 ? f.thin : THIN != 0) inside = thin_plane<POINT>(f, p, &pl, cp);   // the whole wave
  const float e = fminf(fminf(e1, e2), e3);
  const float d = inside ? fminf(pl, e) : e;
  if (POINT) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      c[k] = inside && pl <= e ? cp[k]
                               : (e1 <= e ? fmaf(t1, f.ab[k], f.a[k]) : (e2 <= e ? fmaf(t2, f.ac[k], f.a[k]) : fmaf(t3, f.bc[k], f.b[k])));
  }
  return d;
}

// Faces of the batch-shared list into LDS as 16-bit triples; a face with an index outside [0, V) or -- with `finite_check` --
// a non-finite vertex among Vt (already in LDS) gets SKIP as its first index.  Returns the lane's count of usable faces.
__device__ int load_faces(const int32_t* faces, int F, int V, const float* Vt, bool finite_check, unsigned short* Fc, int tid) {
  int usable = 0;
  for (int f = tid; f < F; f += NT) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
    if (ok && finite_check)
      for (int k = 0; k < 3; ++k) ok = ok && isfinite(Vt[3 * i0 + k]) && isfinite(Vt[3 * i1 + k]) && isfinite(Vt[3 * i2 + k]);
    Fc[3 * f] = ok ? (unsigned short)i0 : SKIP;
    Fc[3 * f + 1] = ok ? (unsigned short)i1 : 0;
    Fc[3 * f + 2] = ok ? (unsigned short)i2 : 0;
    usable += ok ? 1 : 0;
  }
  return usable;
}

}  // namespace
