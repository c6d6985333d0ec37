// render.hip -- forward-only soft-silhouette rasteriser for the predicted MANO meshes (hands_render_silhouette_f32).
// Reference: src/models/hands_light/renderer.py:112-207 (DiffRenderer / MANORenderer), used at hands_light/model.py:413-420,
// hamer_light/model.py:143-148.  The reference delegates to pytorch3d (MeshRasterizer with blur_radius > 0, faces_per_pixel = 10,
// perspective_correct = False, then SoftSilhouetteShader); pytorch3d is third party and absent, so this file restates the
// published algorithm -- rasterize_meshes' naive per-pixel path and sigmoid_alpha_blend -- "parity unpinned" (DESIGN.md section 2).
//
// Per hand: vertices (N, 3) in the camera frame, faces (F, 3) shared by the batch, K (3, 3), image S x S.
//   u = K00 X / Z + K02, v = K11 Y / Z + K12 (skew ignored: the reference takes the diagonal and K[:2, 2]),
//   xn = 2u/S - 1, yn = 2v/S - 1, depth Z.  Output pixel (r, c) samples xn = (2c+1)/S - 1, yn = (2r+1)/S - 1 -- the image point
//   (c + 0.5, r + 0.5): what intrx_to_ndc, pytorch3d's +X-left / +Y-up grid and flip_transpose_canvas compose to.
//   edge(p, a, b) = (p.x-a.x)(b.y-a.y) - (p.y-a.y)(b.x-a.x), area = edge(v2, v0, v1).  A face is a candidate at a pixel when
//   |area| > 1e-8, dist < blur_radius and pz >= 0, where the barycentrics are w0 = edge(p, v1, v2) / (area + 1e-8) etc.,
//   pz = w0 z0 + w1 z1 + w2 z2 (screen-space, not clipped), d2 = the smallest squared distance to the three edge segments (a
//   segment of squared length <= 1e-8 counts as its end point) and dist = -d2 if w0, w1, w2 > 0, else d2.  The faces_per_pixel
//   candidates of smallest pz are kept (ties: lower face index) and alpha = 1 - prod (1 - sigmoid(-dist / sigma)).
//   face_idx / zbuf: the nearest candidate that CONTAINS the pixel (-1 / 0 where none).
// Stated deviation: a face with a vertex at Z <= 0 is skipped (pytorch3d projects such a vertex through the camera centre and
// rasterises the mirrored triangle); predicted hands are in front of the camera.
// The barycentrics are multiplied by 1 / (area + 1e-8) and the segment parameter by 1 / |e|^2 (computed once per face) where
// the published code divides per pixel: one rounding of difference.
//
// The tile geometry, the projection, the cull of a face against the tile, the ordered face list in LDS with its barrier
// protocol and the per-pixel edge functions are raster_tile.h's, shared with shade.hip.  This file's own part:
//   1. the N vertices are projected into LDS (dynamic: 12 N bytes);
//   2. a face's box is grown by sqrt(blur_radius) for the cull, and its 64-byte record carries the depth coefficients of pz
//      and the three edge-length reciprocals;
//   3. in the walk every lane keeps a sorted top-10 of (pz, dist) in registers -- unrolled compare-and-swap with static
//      indices, strict '<' so that a later (higher) face never overtakes an equal depth -- carried across the chunks of an
//      over-full tile;
//   4. blend, store.  No allocation, no synchronisation: capturable in a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "hands_hip.h"
#include "common.h"
#include "raster_tile.h"

using namespace raster_tile;

namespace {

constexpr int MAX_K = 10;                          // faces_per_pixel the register top-K holds
constexpr int RENDER_MAX_LDS = 64 * 1024;          // static + dynamic LDS a launch may ask for without an attribute

// The record, four float4:  x0 y0 x1 y1 | x2 y2 zc z1-z0 | z2-z0 inv_area il0 il1 | il2 idx ylo yhi
//   zc = z0 area / (area + 1e-8) (see pz below); il_i = 1 / |edge i|^2, < 0 for a degenerate edge; [ylo, yhi]: the grown box.

// squared distance from q = p - a to the segment a -> a + e; il = 1 / |e|^2, or < 0: the segment is its end point a + e
__device__ __forceinline__ float seg_d2(float qx, float qy, float ex, float ey, float il) {
  float t = (ex * qx + ey * qy) * il;
  t = fminf(fmaxf(t, 0.f), 1.f);
  t = il < 0.f ? 1.f : t;
  const float dx = qx - t * ex, dy = qy - t * ey;
  return dx * dx + dy * dy;
}

__global__ __launch_bounds__(THREADS) void render_silhouette_kernel(
    const float* __restrict__ verts, int ld_verts, int n_verts, const int32_t* __restrict__ faces, int n_faces,
    const float* __restrict__ Kmat, int S, int tiles_x, int tiles, float sigma, float blur_radius, float grow,
    int faces_per_pixel, float* __restrict__ mask, int32_t* __restrict__ face_idx, float* __restrict__ zbuf) {
  extern __shared__ float s_v[];                   // projected vertices: xn, yn, z
  __shared__ FaceList s_list;

  const int tid = threadIdx.x;
  const TileGeom g = tile_geom(blockIdx.x, tiles, tiles_x, S);
  const int b = g.b, r = g.r, c = g.c;

  // 1. projection
  {
    const float* Kb = Kmat + (size_t)b * 9;
    const float* vb = verts + (size_t)b * ld_verts;
    for (int i = tid; i < n_verts; i += THREADS) {
      const float Z = vb[3 * i + 2];
      const float2 p = project_ndc(Kb, vb[3 * i], vb[3 * i + 1], Z, (float)S);
      s_v[3 * i] = p.x;
      s_v[3 * i + 1] = p.y;
      s_v[3 * i + 2] = Z;
    }
  }
  __syncthreads();

  float tz[MAX_K], td[MAX_K];                      // sorted by depth; empty slots: depth +inf
#pragma unroll
  for (int k = 0; k < MAX_K; ++k) { tz[k] = INFINITY; td[k] = INFINITY; }
  float best_z = INFINITY;
  int best_f = -1;

  int count = 0;
  for (int base = 0, pass = 0; base < n_faces; base += THREADS, ++pass) {
    // 2. one face per lane against the tile
    const int f = base + tid;
    Tri v;                                         // v and the rest of t: read only where t.keep
    TriCull t;
    t.keep = false;
    if (f < n_faces) {
      const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if (face_in_range(i0, i1, i2, n_verts)) {
        v.x0 = s_v[3 * i0]; v.y0 = s_v[3 * i0 + 1]; v.z0 = s_v[3 * i0 + 2];
        v.x1 = s_v[3 * i1]; v.y1 = s_v[3 * i1 + 1]; v.z1 = s_v[3 * i1 + 2];
        v.x2 = s_v[3 * i2]; v.y2 = s_v[3 * i2 + 1]; v.z2 = s_v[3 * i2 + 2];
        t = tri_cull(g, grow, v);
      }
    }
    bool flush;
    const int at = list_append(s_list, t.keep, pass, base + THREADS >= n_faces, count, flush);
    if (t.keep) {
      const float inv_area = 1.f / (t.area + K_EPS);
      const float e0x = v.x1 - v.x0, e0y = v.y1 - v.y0, e1x = v.x2 - v.x1, e1y = v.y2 - v.y1, e2x = v.x0 - v.x2, e2y = v.y0 - v.y2;
      const float l0 = e0x * e0x + e0y * e0y, l1 = e1x * e1x + e1y * e1y, l2 = e2x * e2x + e2y * e2y;
      float4* dst = s_list.rec + 4 * at;
      dst[0] = make_float4(v.x0, v.y0, v.x1, v.y1);
      dst[1] = make_float4(v.x2, v.y2, v.z0 * (t.area * inv_area), v.z1 - v.z0);
      dst[2] = make_float4(v.z2 - v.z0, inv_area, l0 <= K_EPS ? -1.f : 1.f / l0, l1 <= K_EPS ? -1.f : 1.f / l1);
      dst[3] = make_float4(l2 <= K_EPS ? -1.f : 1.f / l2, __int_as_float(f), t.ylo, t.yhi);
    }
    if (!flush) continue;                          // uniform over the workgroup

    // 3. every lane walks the list for its own pixel
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float4 a = s_list.rec[4 * j], bq = s_list.rec[4 * j + 1], cq = s_list.rec[4 * j + 2], dq = s_list.rec[4 * j + 3];
      if (!RASTER_TILE_ROW_HITS(g.py, dq.z, dq.w)) continue;
      const PixelTri p = pixel_tri(g.px, g.py, a.x, a.y, a.z, a.w, bq.x, bq.y, cq.y);
      // w0 z0 + w1 z1 + w2 z2 with w0 = area / (area + eps) - w1 - w2: the rounding errors of the barycentrics then scale with
      // the face's depth RANGE, not with its depth (float32 holds the z-buffer to 1e-6 m this way, the plain sum does not)
      const float pz = bq.z + p.w1 * bq.w + p.w2 * cq.x;
      const float d2 = fminf(fminf(seg_d2(p.q0x, p.q0y, p.e0x, p.e0y, cq.z), seg_d2(p.q1x, p.q1y, p.e1x, p.e1y, cq.w)),
                             seg_d2(p.q2x, p.q2y, p.e2x, p.e2y, dq.x));
      const bool inside = p.w0 > 0.f && p.w1 > 0.f && p.w2 > 0.f;
      const float dist = inside ? -d2 : d2;
      if (dist < blur_radius && pz >= 0.f) {
        if (inside && pz < best_z) { best_z = pz; best_f = __float_as_int(dq.y); }
        float z = pz, d = dist;
#pragma unroll
        for (int k = 0; k < MAX_K; ++k) {          // static indices: the arrays stay in registers
          const bool sw = z < tz[k];
          const float oz = tz[k], od = td[k];
          tz[k] = sw ? z : oz; td[k] = sw ? d : od;
          z = sw ? oz : z;     d = sw ? od : d;
        }
      }
    }
    count = 0;
  }

  // 4. blend
  if (r < S && c < S) {
    float keep_prod = 1.f;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k)
      if (k < faces_per_pixel && tz[k] < INFINITY) keep_prod *= 1.f - 1.f / (1.f + expf(td[k] / sigma));   // 1 - sigmoid(-dist / sigma)
    const size_t o = ((size_t)b * S + r) * S + c;
    mask[o] = 1.f - keep_prod;
    if (face_idx) face_idx[o] = best_f;
    if (zbuf) zbuf[o] = best_f >= 0 ? best_z : 0.f;
  }
}

}  // namespace

extern "C" int hands_render_silhouette_f32(const float* verts, int ld_verts, int n_verts, const int32_t* faces, int n_faces, const float* K, int B, int S, float sigma, float blur_radius, int faces_per_pixel, float* mask, int32_t* face_idx, float* zbuf, hands_stream_t stream) {
  if (!verts || !faces || !K || !mask || B <= 0 || S < 1 || S > 16384 || n_verts < 1 || n_faces < 0 || ld_verts < 3 * n_verts) return HANDS_EINVAL;
  if (faces_per_pixel < 1 || faces_per_pixel > MAX_K || !(sigma > 0.f) || !(blur_radius >= 0.f)) return HANDS_EINVAL;
  const size_t lds_static = sizeof(FaceList);
  const size_t lds_verts = (size_t)n_verts * 3 * sizeof(float);
  if (lds_verts + lds_static > (size_t)RENDER_MAX_LDS) return HANDS_EINVAL;          // the vertex block must fit in LDS
  const int tiles_x = (S + TILE_W - 1) / TILE_W, tiles_y = (S + TILE_H - 1) / TILE_H;
  const long long blocks = (long long)tiles_x * tiles_y * B;
  if (blocks > 0x7fffffffLL) return HANDS_EINVAL;
  // the box grows by a little more than sqrt(blur_radius): the cull must never lose a face the per-pixel test would keep
  const float grow = sqrtf(blur_radius) * 1.001f + 1e-6f;
  hipLaunchKernelGGL(render_silhouette_kernel, dim3((unsigned)blocks), dim3(THREADS), lds_verts, (hipStream_t)stream,
                     verts, ld_verts, n_verts, faces, n_faces, K, S, tiles_x, tiles_x * tiles_y, sigma, blur_radius, grow,
                     faces_per_pixel, mask, face_idx, zbuf);
  HANDS_LAUNCH_CHECK();
}
