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
// One workgroup of 256 lanes per (hand, 32 x 8 pixel tile); a wave's 64 pixels are two full rows of the tile.
//   1. the N vertices are projected into LDS (dynamic: 12 N bytes);
//   2. 256 faces at a time, each lane tests one face's box (grown by sqrt(blur_radius)) against the tile; the survivors are
//      compacted IN FACE ORDER (ballot + prefix inside a wave, four wave counts through LDS) into a list of 64-byte records;
//   3. when another 256 faces might not fit (or at the end) every lane walks the list for its own pixel and keeps a sorted
//      top-10 of (pz, dist) in registers -- unrolled compare-and-swap with static indices, strict '<' so that a later (higher)
//      face never overtakes an equal depth -- then the list restarts: an over-full tile is processed in chunks, the top-10
//      carried across them, no face dropped;
//   4. blend, store.  No allocation, no synchronisation: capturable in a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "hands_hip.h"
#include "common.h"

namespace {

constexpr int RENDER_THREADS = 256;
constexpr int TILE_W = 32, TILE_H = 8;             // TILE_W * TILE_H == RENDER_THREADS
constexpr int LIST_CAP = 384;                      // face records per chunk: 24 KB
constexpr int MAX_K = 10;                          // faces_per_pixel the register top-K holds
constexpr int RENDER_MAX_LDS = 64 * 1024;          // static + dynamic LDS a launch may ask for without an attribute
constexpr float K_EPS = 1e-8f;

struct FaceRec {                                   // 16 dwords, read as four broadcast 16-byte loads
  float x0, y0, x1, y1;
  float x2, y2, z0, z1;                            // in the list: z0 area / (area + 1e-8), z1 - z0, z2 - z0 (see pz below)
  float z2, inv_area, il0, il1;                    // il_i = 1 / |edge i|^2, < 0 for a degenerate edge (edge 0 = v0v1, 1 = v1v2, 2 = v2v0)
  float il2; int idx; float ylo, yhi;              // y extent of the grown box: a wave (two pixel rows) skips the faces that miss both
};
static_assert(sizeof(FaceRec) == 64, "FaceRec is four float4");

// squared distance from q = p - a to the segment a -> a + e; il = 1 / |e|^2, or < 0: the segment is its end point a + e
__device__ __forceinline__ float seg_d2(float qx, float qy, float ex, float ey, float il) {
  float t = (ex * qx + ey * qy) * il;
  t = fminf(fmaxf(t, 0.f), 1.f);
  t = il < 0.f ? 1.f : t;
  const float dx = qx - t * ex, dy = qy - t * ey;
  return dx * dx + dy * dy;
}

__global__ __launch_bounds__(RENDER_THREADS) void render_silhouette_kernel(
    const float* __restrict__ verts, int ld_verts, int n_verts, const int32_t* __restrict__ faces, int n_faces,
    const float* __restrict__ Kmat, int S, int tiles_x, int tiles, float sigma, float blur_radius, float grow,
    int faces_per_pixel, float* __restrict__ mask, int32_t* __restrict__ face_idx, float* __restrict__ zbuf) {
  extern __shared__ float s_v[];                   // projected vertices: xn, yn, z
  __shared__ float4 s_face[LIST_CAP * 4];
  __shared__ int s_wc[2][RENDER_THREADS / 64];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const float fS = (float)S;

  // 1. projection
  {
    const float* Kb = Kmat + (size_t)b * 9;
    const float k00 = Kb[0], k02 = Kb[2], k11 = Kb[4], k12 = Kb[5];
    const float* vb = verts + (size_t)b * ld_verts;
    for (int i = tid; i < n_verts; i += RENDER_THREADS) {
      const float X = vb[3 * i], Y = vb[3 * i + 1], Z = vb[3 * i + 2];
      const float u = k00 * X / Z + k02, v = k11 * Y / Z + k12;
      s_v[3 * i] = 2.f * u / fS - 1.f;
      s_v[3 * i + 1] = 2.f * v / fS - 1.f;
      s_v[3 * i + 2] = Z;
    }
  }
  __syncthreads();

  const int r = ty * TILE_H + (tid >> 5), c = tx * TILE_W + (tid & 31);
  const float px = (float)(2 * c + 1) / fS - 1.f, py = (float)(2 * r + 1) / fS - 1.f;
  // sample points of the tile's first and last pixel
  const float tx0 = (float)(2 * tx * TILE_W + 1) / fS - 1.f, tx1 = (float)(2 * (tx * TILE_W + TILE_W - 1) + 1) / fS - 1.f;
  const float ty0 = (float)(2 * ty * TILE_H + 1) / fS - 1.f, ty1 = (float)(2 * (ty * TILE_H + TILE_H - 1) + 1) / fS - 1.f;

  float tz[MAX_K], td[MAX_K];                      // sorted by depth; empty slots: depth +inf
#pragma unroll
  for (int k = 0; k < MAX_K; ++k) { tz[k] = INFINITY; td[k] = INFINITY; }
  float best_z = INFINITY;
  int best_f = -1;

  int count = 0;
  for (int base = 0, pass = 0; base < n_faces; base += RENDER_THREADS, ++pass) {
    // 2. one face per lane against the tile
    const int f = base + tid;
    bool keep = false;
    FaceRec rec;
    if (f < n_faces) {
      const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if ((unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts) {
        rec.x0 = s_v[3 * i0]; rec.y0 = s_v[3 * i0 + 1]; rec.z0 = s_v[3 * i0 + 2];
        rec.x1 = s_v[3 * i1]; rec.y1 = s_v[3 * i1 + 1]; rec.z1 = s_v[3 * i1 + 2];
        rec.x2 = s_v[3 * i2]; rec.y2 = s_v[3 * i2 + 1]; rec.z2 = s_v[3 * i2 + 2];
        const float area = (rec.x2 - rec.x0) * (rec.y1 - rec.y0) - (rec.y2 - rec.y0) * (rec.x1 - rec.x0);
        const float xlo = fminf(fminf(rec.x0, rec.x1), rec.x2) - grow, xhi = fmaxf(fmaxf(rec.x0, rec.x1), rec.x2) + grow;
        rec.ylo = fminf(fminf(rec.y0, rec.y1), rec.y2) - grow;
        rec.yhi = fmaxf(fmaxf(rec.y0, rec.y1), rec.y2) + grow;
        // every comparison is false for a NaN: such a face is dropped
        keep = rec.z0 > 0.f && rec.z1 > 0.f && rec.z2 > 0.f && fabsf(area) > K_EPS && xlo <= tx1 && xhi >= tx0 &&
               rec.ylo <= ty1 && rec.yhi >= ty0;
        if (keep) {
          rec.inv_area = 1.f / (area + K_EPS);
          rec.z1 -= rec.z0;
          rec.z2 -= rec.z0;
          rec.z0 *= area * rec.inv_area;
          const float e0x = rec.x1 - rec.x0, e0y = rec.y1 - rec.y0, e1x = rec.x2 - rec.x1, e1y = rec.y2 - rec.y1;
          const float e2x = rec.x0 - rec.x2, e2y = rec.y0 - rec.y2;
          const float l0 = e0x * e0x + e0y * e0y, l1 = e1x * e1x + e1y * e1y, l2 = e2x * e2x + e2y * e2y;
          rec.il0 = l0 <= K_EPS ? -1.f : 1.f / l0;
          rec.il1 = l1 <= K_EPS ? -1.f : 1.f / l1;
          rec.il2 = l2 <= K_EPS ? -1.f : 1.f / l2;
          rec.idx = f;
        }
      }
    }
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_wc[pass & 1][wave] = __popcll(bal);
    __syncthreads();
    int off = count, total = 0;
#pragma unroll
    for (int w = 0; w < RENDER_THREADS / 64; ++w) {
      const int n = s_wc[pass & 1][w];
      off += w < wave ? n : 0;
      total += n;
    }
    if (keep) {                                    // count + total <= LIST_CAP: a flush leaves count <= LIST_CAP - 256
      const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
      float4* dst = s_face + 4 * at;
      dst[0] = make_float4(rec.x0, rec.y0, rec.x1, rec.y1);
      dst[1] = make_float4(rec.x2, rec.y2, rec.z0, rec.z1);
      dst[2] = make_float4(rec.z2, rec.inv_area, rec.il0, rec.il1);
      dst[3] = make_float4(rec.il2, __int_as_float(rec.idx), rec.ylo, rec.yhi);
    }
    count += total;
    const bool last = base + RENDER_THREADS >= n_faces;
    if (count <= LIST_CAP - RENDER_THREADS && !last) continue;          // uniform over the workgroup

    // 3. every lane walks the list for its own pixel
    __syncthreads();
    for (int j = 0; j < count; ++j) {
      const float4 a = s_face[4 * j], bq = s_face[4 * j + 1], cq = s_face[4 * j + 2], dq = s_face[4 * j + 3];
      if (!(py >= dq.z && py <= dq.w)) continue;
      const float x0 = a.x, y0 = a.y, x1 = a.z, y1 = a.w, x2 = bq.x, y2 = bq.y;
      const float q0x = px - x0, q0y = py - y0, q1x = px - x1, q1y = py - y1, q2x = px - x2, q2y = py - y2;
      const float e0x = x1 - x0, e0y = y1 - y0, e1x = x2 - x1, e1y = y2 - y1, e2x = x0 - x2, e2y = y0 - y2;
      const float w0 = (q1x * e1y - q1y * e1x) * cq.y;     // edge(p, v1, v2) / (area + eps)
      const float w1 = (q2x * e2y - q2y * e2x) * cq.y;     // edge(p, v2, v0)
      const float w2 = (q0x * e0y - q0y * e0x) * cq.y;     // edge(p, v0, v1)
      // w0 z0 + w1 z1 + w2 z2 with w0 = area / (area + eps) - w1 - w2: the rounding errors of the barycentrics then scale with
      // the face's depth RANGE, not with its depth (float32 holds the z-buffer to 1e-6 m this way, the plain sum does not)
      const float pz = bq.z + w1 * bq.w + w2 * cq.x;
      const float d2 = fminf(fminf(seg_d2(q0x, q0y, e0x, e0y, cq.z), seg_d2(q1x, q1y, e1x, e1y, cq.w)),
                             seg_d2(q2x, q2y, e2x, e2y, dq.x));
      const bool inside = w0 > 0.f && w1 > 0.f && w2 > 0.f;
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
    if (!last) __syncthreads();                    // the list is rewritten by the next pass
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
  const size_t lds_static = sizeof(float4) * 4 * LIST_CAP + sizeof(int) * 2 * (RENDER_THREADS / 64);
  const size_t lds_verts = (size_t)n_verts * 3 * sizeof(float);
  if (lds_verts + lds_static > (size_t)RENDER_MAX_LDS) return HANDS_EINVAL;          // the vertex block must fit in LDS
  const int tiles_x = (S + TILE_W - 1) / TILE_W, tiles_y = (S + TILE_H - 1) / TILE_H;
  const long long blocks = (long long)tiles_x * tiles_y * B;
  if (blocks > 0x7fffffffLL) return HANDS_EINVAL;
  // the box grows by a little more than sqrt(blur_radius): the cull must never lose a face the per-pixel test would keep
  const float grow = sqrtf(blur_radius) * 1.001f + 1e-6f;
  hipLaunchKernelGGL(render_silhouette_kernel, dim3((unsigned)blocks), dim3(RENDER_THREADS), lds_verts, (hipStream_t)stream,
                     verts, ld_verts, n_verts, faces, n_faces, K, S, tiles_x, tiles_x * tiles_y, sigma, blur_radius, grow,
                     faces_per_pixel, mask, face_idx, zbuf);
  HANDS_LAUNCH_CHECK();
}
