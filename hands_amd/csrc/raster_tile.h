// raster_tile.h -- the tile-binning core of the two mesh rasterisers: render.hip (soft silhouette) and shade.hip (shaded
// overlays and side views).  Device only.  It holds what both kernels do in the same way and nothing that would branch on
// the caller: the tile's geometry, the NDC projection, the face's cull against the tile, the ordered face list in LDS and
// the per-pixel edge functions.  Each kernel keeps its own record fields, its own per-pixel state and its own epilogue.
//
// One workgroup of THREADS = 256 lanes per (image, TILE_W x TILE_H pixel tile), one lane per pixel; a wave's 64 pixels are
// two full rows of the tile.  THREADS faces at a time ("a pass"), one per lane, are tested against the tile (tri_cull); the
// survivors are appended IN FACE ORDER (list_append) to a list of 64-byte records in LDS; when another pass might not fit, or
// after the last pass, every lane walks the list for its own pixel (RASTER_TILE_ROW_HITS, pixel_tri) and the list restarts:
// an over-full tile is processed in chunks, the per-pixel state carried across them, no face dropped.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "hands_hip.h"

namespace raster_tile {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int TILE_W = HANDS_SHADE_TILE_W, TILE_H = HANDS_SHADE_TILE_H;
constexpr int LIST_CAP = HANDS_SHADE_LIST_CAP;     // face records per chunk: 24 KB
constexpr float K_EPS = 1e-8f;
static_assert(TILE_W * TILE_H == THREADS, "one lane per pixel of the tile");
static_assert(LIST_CAP >= THREADS, "a pass of 256 faces must fit after a flush");

// The list, __shared__ in the kernel: record j is rec[4 j .. 4 j + 3], read as four broadcast 16-byte loads.
//
// Barrier protocol.  A pass costs ONE barrier, inside list_append, between the wave counts' stores and their loads.  A flush
// costs one more, in the kernel, between the pass's record stores and the walk.  Nothing follows the walk: a lane stores the
// next records only after it has crossed the next pass's barrier, and every lane reaches that barrier only after its walk has
// ended.  wc is double-buffered by the pass's parity for the same reason: the lanes that are still reading wc[p & 1] have
// not crossed barrier p + 1, and wc[p & 1] is stored again only by a lane that has.
struct FaceList {
  float4 rec[LIST_CAP * 4];
  int wc[2][WAVES];
};

// This lane's pixel (r, c) of image b, its sample point (px, py) -- the image point (c + 0.5, r + 0.5) in NDC -- and the
// sample points of the tile's first and last pixel.  r >= S or c >= S in a partial tile: such a lane bins but does not store.
struct TileGeom { int b, r, c; float px, py, tx0, tx1, ty0, ty1; };
__device__ __forceinline__ TileGeom tile_geom(int block, int tiles, int tiles_x, int S) {
  const int tid = threadIdx.x, b = block / tiles, tile = block - b * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const float fS = (float)S;
  TileGeom g;
  g.b = b; g.r = ty * TILE_H + tid / TILE_W; g.c = tx * TILE_W + tid % TILE_W;
  g.px = (float)(2 * g.c + 1) / fS - 1.f; g.py = (float)(2 * g.r + 1) / fS - 1.f;
  g.tx0 = (float)(2 * tx * TILE_W + 1) / fS - 1.f; g.tx1 = (float)(2 * (tx * TILE_W + TILE_W - 1) + 1) / fS - 1.f;
  g.ty0 = (float)(2 * ty * TILE_H + 1) / fS - 1.f; g.ty1 = (float)(2 * (ty * TILE_H + TILE_H - 1) + 1) / fS - 1.f;
  return g;
}

// u = K00 X / Z + K02, v = K11 Y / Z + K12 (skew ignored), xn = 2u/S - 1, yn = 2v/S - 1.  Kb: one image's (3, 3).
__device__ __forceinline__ float2 project_ndc(const float* __restrict__ Kb, float X, float Y, float Z, float fS) {
  const float u = Kb[0] * X / Z + Kb[2], v = Kb[4] * Y / Z + Kb[5];
  return make_float2(2.f * u / fS - 1.f, 2.f * v / fS - 1.f);
}

__device__ __forceinline__ bool face_in_range(int i0, int i1, int i2, int n_verts) {
  return (unsigned)i0 < (unsigned)n_verts && (unsigned)i1 < (unsigned)n_verts && (unsigned)i2 < (unsigned)n_verts;
}

// edge(p, a, b) = (p.x-a.x)(b.y-a.y) - (p.y-a.y)(b.x-a.x), area = edge(v2, v0, v1).  A face is kept when all Z > 0,
// |area| > 1e-8 and its box, grown by `grow` on every side, meets the tile's sample points.  [ylo, yhi] is the grown box's
// y extent, stored in the record for RASTER_TILE_ROW_HITS.
struct Tri { float x0, y0, z0, x1, y1, z1, x2, y2, z2; };          // projected: xn, yn and the depth Z of the three vertices
struct TriCull { float area, ylo, yhi; bool keep; };
__device__ __forceinline__ TriCull tri_cull(const TileGeom& g, float grow, const Tri& v) {
  TriCull t;
  t.area = (v.x2 - v.x0) * (v.y1 - v.y0) - (v.y2 - v.y0) * (v.x1 - v.x0);
  const float xlo = fminf(fminf(v.x0, v.x1), v.x2) - grow, xhi = fmaxf(fmaxf(v.x0, v.x1), v.x2) + grow;
  t.ylo = fminf(fminf(v.y0, v.y1), v.y2) - grow; t.yhi = fmaxf(fmaxf(v.y0, v.y1), v.y2) + grow;
  // every comparison is false for a NaN: such a face is dropped
  t.keep = v.z0 > 0.f && v.z1 > 0.f && v.z2 > 0.f && fabsf(t.area) > K_EPS && xlo <= g.tx1 && xhi >= g.tx0 &&
           t.ylo <= g.ty1 && t.yhi >= g.ty0;
  return t;
}

// Called by all 256 lanes once per pass (pass = 0, 1, 2, ... over the whole kernel).  Returns the record slot of a lane
// that keeps its face: the survivors of a pass follow the list's `count` records in lane order.  count becomes the new
// length; it never exceeds LIST_CAP, because a flush leaves count <= LIST_CAP - THREADS.  flush (uniform over the
// workgroup): walk the list now, after the records are stored and a __syncthreads(), then set count = 0.
__device__ __forceinline__ int list_append(FaceList& L, bool keep, int pass, bool last, int& count, bool& flush) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) L.wc[pass & 1][wave] = __popcll(bal);
  __syncthreads();
  int off = count, total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) {
    const int n = L.wc[pass & 1][w];
    off += w < wave ? n : 0;
    total += n;
  }
  count += total;
  flush = count > LIST_CAP - THREADS || last;
  return off + __popcll(bal & ((1ull << lane) - 1ull));
}

// A wave (two pixel rows) skips the faces whose grown box misses both.  A macro for what this compiler (hipcc of ROCm 7) makes
// of it, nothing else: as an inline function the two comparisons are merged into one condition, the silhouette kernel's walk
// is then allocated five more register copies per face and was measured slower (docs/EXPERIMENTS.md has the figures).
#define RASTER_TILE_ROW_HITS(py, ylo, yhi) ((py) >= (ylo) && (py) <= (yhi))

// q_i = p - v_i, e_i = the edge that leaves v_i (e0 = v0v1, e1 = v1v2, e2 = v2v0) and the barycentrics
// w0 = edge(p, v1, v2) / (area + 1e-8), w1 = edge(p, v2, v0) / .., w2 = edge(p, v0, v1) / .., as products with
// inv_area = 1 / (area + 1e-8), computed once per face.  p is inside the face when w0, w1, w2 > 0 (both windings).
struct PixelTri { float q0x, q0y, q1x, q1y, q2x, q2y, e0x, e0y, e1x, e1y, e2x, e2y, w0, w1, w2; };
__device__ __forceinline__ PixelTri pixel_tri(float px, float py, float x0, float y0, float x1, float y1, float x2, float y2,
                                              float inv_area) {
  PixelTri t;
  t.q0x = px - x0; t.q0y = py - y0; t.q1x = px - x1; t.q1y = py - y1; t.q2x = px - x2; t.q2y = py - y2;
  t.e0x = x1 - x0; t.e0y = y1 - y0; t.e1x = x2 - x1; t.e1y = y2 - y1; t.e2x = x0 - x2; t.e2y = y0 - y2;
  t.w0 = (t.q1x * t.e1y - t.q1y * t.e1x) * inv_area;
  t.w1 = (t.q2x * t.e2y - t.q2y * t.e2x) * inv_area;
  t.w2 = (t.q0x * t.e0y - t.q0y * t.e0x) * inv_area;
  return t;
}

}  // namespace raster_tile
