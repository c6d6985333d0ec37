// shade.hip -- forward-only hard z-buffer rasteriser with smooth shading for up to four meshes per image
// (hands_mesh_prepare_f32, hands_render_shaded_f32): the overlay and side-view pictures of common/rend_utils.py::Renderer,
// driven by src/callbacks/vis/visualize_arctic.py:199-271.  The reference draws them with pyrender on OpenGL, one image at a
// time; pyrender is third party and absent, so the semantics are DEFINED in DESIGN.md section 7 and restated in fp64 in
// tests/shade_ref.py -- "parity unpinned" (DESIGN.md section 2).
//
// Per image: M <= 4 meshes in the camera frame (+x right, +y down, +z forward), each with a base colour and a metallic factor,
// an optional rigid transform T applied to every vertex first, K (3, 3), image S x S.
//   pre-pass   P' = R P + t; n_v = normalise(sum over the faces that hold v, ascending, of (P'1 - P'0) x (P'2 - P'0)), the zero
//              vector when the squared sum is <= 1e-30; projection: raster_tile.h's, xn = 2 (K00 X / Z + K02) / S - 1.
//   coverage   raster_tile.h's rule, the silhouette rasteriser's: all Z > 0, |area| > 1e-8, w0, w1, w2 > 0 with
//              w_i = edge_i / (area + 1e-8); both windings (no back-face culling: the MANO mesh is open at the wrist).
//   depth      perspective-correct, 1 / z = sum w_i / z_i, b_i = (w_i / z_i) z; the nearest z wins, ties to the lower
//              (mesh, face): the faces are visited in that order and the comparison is a strict '<'.
//   shading    P = sum b_i P'_i, n = normalise(sum b_i n_i), v = normalise(-P); n = v if n is zero, n = -n if n.v < 0;
//              glTF 2.0 metallic-roughness with ONE directional light towards l = (0, 0, -1), intensity 3 (rend_utils.py:128-142
//              gives its three lights translations only: all three shine along the view axis), ambient 0.5.
//   composite  covered: the clamped colour; uncovered: the background image, or 1.0.  8 bit: floor(255 x).
//
// hands_mesh_prepare_f32: one lane per (image, vertex); the normal is GATHERED through a CSR vertex -> face table (no float
// atomics: bit-reproducible).  8 floats per vertex: P'x P'y P'z nx | ny nz xn yn.
// hands_render_shaded_f32: the tile geometry, the cull of a face against the tile (its box not grown), the ordered face list in
// LDS with its barrier protocol and the per-pixel edge functions are raster_tile.h's, shared with render.hip.  This file's
// own part: the faces of the valid meshes are binned in (mesh, face) order, a record carries 1/z coefficients, and in the
// walk every lane keeps the nearest hit only -- z, global face id, two barycentrics.  The epilogue fetches the winner's
// three vertex records from the workspace (L2-resident), shades, composites and stores.  No allocation, no
// synchronisation: capturable in a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "hands_hip.h"
#include "common.h"
#include "raster_tile.h"

using namespace raster_tile;

namespace {

constexpr int WS = 8;                              // workspace floats per vertex
constexpr float PI_F = 3.14159265358979323846f;

struct Vec3 { float x, y, z; };
__device__ __forceinline__ Vec3 xform(const float* T, float X, float Y, float Z) {
  if (!T) return {X, Y, Z};
  return {T[0] * X + T[1] * Y + T[2] * Z + T[3], T[4] * X + T[5] * Y + T[6] * Z + T[7], T[8] * X + T[9] * Y + T[10] * Z + T[11]};
}

__global__ __launch_bounds__(256) void mesh_prepare_kernel(
    const float* __restrict__ verts, int ld_verts, int n_verts, const int32_t* __restrict__ faces, int n_faces,
    const int32_t* __restrict__ csr_off, const int32_t* __restrict__ csr_face, const float* __restrict__ Kmat,
    const float* __restrict__ Tmat, int B, int S, float* __restrict__ ws) {
  const long long total = (long long)B * n_verts;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int b = (int)(i / n_verts), v = (int)(i - (long long)b * n_verts);
    const float* vb = verts + (size_t)b * ld_verts;
    const float* T = Tmat ? Tmat + (size_t)b * 12 : nullptr;
    const Vec3 P = xform(T, vb[3 * v], vb[3 * v + 1], vb[3 * v + 2]);
    float sx = 0.f, sy = 0.f, sz = 0.f;
    const int j1 = csr_off[v + 1];
    for (int j = csr_off[v]; j < j1; ++j) {
      const int f = csr_face[j];
      if ((unsigned)f >= (unsigned)n_faces) continue;
      const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
      if (!face_in_range(i0, i1, i2, n_verts)) continue;
      const Vec3 a = xform(T, vb[3 * i0], vb[3 * i0 + 1], vb[3 * i0 + 2]);
      const Vec3 p = xform(T, vb[3 * i1], vb[3 * i1 + 1], vb[3 * i1 + 2]);
      const Vec3 q = xform(T, vb[3 * i2], vb[3 * i2 + 1], vb[3 * i2 + 2]);
      const float ux = p.x - a.x, uy = p.y - a.y, uz = p.z - a.z, wx = q.x - a.x, wy = q.y - a.y, wz = q.z - a.z;
      const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
      if (fabsf(cx) <= 3.0e38f && fabsf(cy) <= 3.0e38f && fabsf(cz) <= 3.0e38f) { sx += cx; sy += cy; sz += cz; }   // false for a NaN
    }
    const float s2 = sx * sx + sy * sy + sz * sz;
    const float inv = s2 > 1e-30f ? 1.f / sqrtf(s2) : 0.f;
    const float2 ndc = project_ndc(Kmat + (size_t)b * 9, P.x, P.y, P.z, (float)S);
    float4* dst = reinterpret_cast<float4*>(ws + (size_t)i * WS);
    dst[0] = make_float4(P.x, P.y, P.z, inv > 0.f ? sx * inv : 0.f);
    dst[1] = make_float4(inv > 0.f ? sy * inv : 0.f, inv > 0.f ? sz * inv : 0.f, ndc.x, ndc.y);
  }
}

__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float smith_g1(float nd, float a2) { return 2.f * nd / (nd + sqrtf(a2 + (1.f - a2) * nd * nd)); }

// glTF 2.0 metallic-roughness under one directional light towards l = (0, 0, -1) of intensity 3, plus the ambient term 0.5 c
__device__ __forceinline__ float shade_channel(float c, float m, float a2, float NdotL, float NdotV, float NdotH, float VdotH) {
  const float f0 = 0.04f * (1.f - m) + c * m;
  const float c_diff = 0.96f * c * (1.f - m);
  const float t = 1.f - VdotH, t2 = t * t;
  const float F = f0 + (1.f - f0) * (t2 * t2 * t);
  const float dd = NdotH * NdotH * (a2 - 1.f) + 1.f;
  const float D = a2 / (PI_F * (dd * dd));
  const float G = smith_g1(NdotL, a2) * smith_g1(NdotV, a2);
  const float col = 3.0f * NdotL * ((1.f - F) * c_diff / PI_F + F * G * D / (4.f * NdotL * NdotV)) + 0.5f * c;
  return clamp01(col);
}

__global__ __launch_bounds__(THREADS) void render_shaded_kernel(
    const hands_shade_scene sc, const float* __restrict__ image, int S, int tiles_x, int tiles,
    float* __restrict__ rgb, unsigned char* __restrict__ rgb8, float* __restrict__ depth, int32_t* __restrict__ face_id) {
  __shared__ FaceList s_list;

  const int tid = threadIdx.x;
  const TileGeom g = tile_geom(blockIdx.x, tiles, tiles_x, S);
  const int b = g.b, r = g.r, c = g.c;

  float best_z = INFINITY, best_b1 = 0.f, best_b2 = 0.f;
  int best_m = -1, best_f = -1;

  int last_m = -1;                                   // the last mesh that has faces to bin for this image (uniform)
  for (int m = 0; m < sc.n_meshes; ++m)
    if (sc.mesh[m].n_faces > 0 && (!sc.mesh[m].valid || sc.mesh[m].valid[b] != 0.f)) last_m = m;

  int count = 0, pass = 0;
  for (int m = 0; m <= last_m; ++m) {
    const hands_shade_mesh& M = sc.mesh[m];
    if (M.n_faces <= 0 || (M.valid && M.valid[b] == 0.f)) continue;          // uniform over the workgroup
    const float* wsb = M.workspace + (size_t)b * M.n_verts * WS;
    for (int base = 0; base < M.n_faces; base += THREADS, ++pass) {
      // one face per lane against the tile
      const int f = base + tid;
      Tri v = {};                                    // zeroed: undefined, this compiler gives the kernel 56 VGPRs, not 48
      TriCull t;
      t.keep = false;
      if (f < M.n_faces) {
        const int i0 = M.faces[3 * f], i1 = M.faces[3 * f + 1], i2 = M.faces[3 * f + 2];
        if (face_in_range(i0, i1, i2, M.n_verts)) {
          const float* a0 = wsb + (size_t)i0 * WS; const float* a1 = wsb + (size_t)i1 * WS; const float* a2 = wsb + (size_t)i2 * WS;
          v.x0 = a0[6]; v.y0 = a0[7]; v.z0 = a0[2];
          v.x1 = a1[6]; v.y1 = a1[7]; v.z1 = a1[2];
          v.x2 = a2[6]; v.y2 = a2[7]; v.z2 = a2[2];
          t = tri_cull(g, 0.f, v);
        }
      }
      bool flush;
      const int at = list_append(s_list, t.keep, pass, m == last_m && base + THREADS >= M.n_faces, count, flush);
      if (t.keep) {
        const float inv_area = 1.f / (t.area + K_EPS);
        const float iz0 = 1.f / v.z0, iz1 = 1.f / v.z1, iz2 = 1.f / v.z2;
        float4* dst = s_list.rec + 4 * at;
        dst[0] = make_float4(v.x0, v.y0, v.x1, v.y1);
        // 1/z = W / z0 + w1 (1/z1 - 1/z0) + w2 (1/z2 - 1/z0) with W = w0 + w1 + w2 = area / (area + eps): the rounding errors of
        // the barycentrics then scale with the face's RANGE of 1/z, not with 1/z itself (render.hip does the same for pz)
        dst[1] = make_float4(v.x2, v.y2, inv_area, t.area * inv_area * iz0);
        dst[2] = make_float4(iz1 - iz0, iz2 - iz0, iz1, iz2);
        dst[3] = make_float4(__int_as_float(m), __int_as_float(f), t.ylo, t.yhi);
      }
      if (!flush) continue;                          // uniform over the workgroup

      // every lane walks the list for its own pixel
      __syncthreads();
      for (int j = 0; j < count; ++j) {
        const float4 a = s_list.rec[4 * j], bq = s_list.rec[4 * j + 1], cq = s_list.rec[4 * j + 2], dq = s_list.rec[4 * j + 3];
        if (!RASTER_TILE_ROW_HITS(g.py, dq.z, dq.w)) continue;
        const PixelTri p = pixel_tri(g.px, g.py, a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z);
        if (p.w0 > 0.f && p.w1 > 0.f && p.w2 > 0.f) {
          const float iz = bq.w + p.w1 * cq.x + p.w2 * cq.y;
          const float z = 1.f / iz;
          if (z < best_z) {                          // strict: a later (higher) face never overtakes an equal depth
            best_z = z;
            best_m = __float_as_int(dq.x);
            best_f = __float_as_int(dq.y);
            best_b1 = p.w1 * cq.z * z;
            best_b2 = p.w2 * cq.w * z;
          }
        }
      }
      count = 0;
    }
  }

  // shade, composite, store
  if (r >= S || c >= S) return;
  const size_t o = ((size_t)b * S + r) * S + c;
  float out[3];
  if (best_m >= 0) {
    // static indexing of the by-value scene: a runtime index would put it in scratch
    hands_shade_mesh M = sc.mesh[0];
    if (best_m == 1) M = sc.mesh[1];
    if (best_m == 2) M = sc.mesh[2];
    if (best_m == 3) M = sc.mesh[3];
    const float* wsb = M.workspace + (size_t)b * M.n_verts * WS;
    const int i0 = M.faces[3 * best_f], i1 = M.faces[3 * best_f + 1], i2 = M.faces[3 * best_f + 2];
    const float4* r0 = reinterpret_cast<const float4*>(wsb + (size_t)i0 * WS);
    const float4* r1 = reinterpret_cast<const float4*>(wsb + (size_t)i1 * WS);
    const float4* r2 = reinterpret_cast<const float4*>(wsb + (size_t)i2 * WS);
    const float4 p0 = r0[0], n0 = r0[1], p1 = r1[0], n1 = r1[1], p2 = r2[0], n2 = r2[1];
    const float b1 = best_b1, b2 = best_b2, b0 = 1.f - b1 - b2;
    const float Px = b0 * p0.x + b1 * p1.x + b2 * p2.x, Py = b0 * p0.y + b1 * p1.y + b2 * p2.y, Pz = b0 * p0.z + b1 * p1.z + b2 * p2.z;
    float nx = b0 * p0.w + b1 * p1.w + b2 * p2.w, ny = b0 * n0.x + b1 * n1.x + b2 * n2.x, nz = b0 * n0.y + b1 * n1.y + b2 * n2.y;
    const float ip = 1.f / sqrtf(Px * Px + Py * Py + Pz * Pz);
    const float vx = -Px * ip, vy = -Py * ip, vz = -Pz * ip;
    const float n2s = nx * nx + ny * ny + nz * nz;
    if (n2s > 1e-30f) {
      const float in = 1.f / sqrtf(n2s);
      nx *= in; ny *= in; nz *= in;
    } else {
      nx = vx; ny = vy; nz = vz;
    }
    float ndv = nx * vx + ny * vy + nz * vz;
    if (ndv < 0.f) { nx = -nx; ny = -ny; nz = -nz; ndv = -ndv; }
    // l = (0, 0, -1); h = normalise(l + v)
    const float hx = vx, hy = vy, hz = vz - 1.f;
    const float ih = 1.f / sqrtf(hx * hx + hy * hy + hz * hz);
    const float NdotL = fminf(fmaxf(-nz, 0.001f), 1.f);
    const float NdotV = fminf(fmaxf(ndv, 0.001f), 1.f);
    const float NdotH = clamp01((nx * hx + ny * hy + nz * hz) * ih);
    const float VdotH = clamp01((vx * hx + vy * hy + vz * hz) * ih);
    const float al = M.roughness * M.roughness, a2 = al * al;
    out[0] = shade_channel(M.color[0], M.metallic, a2, NdotL, NdotV, NdotH, VdotH);
    out[1] = shade_channel(M.color[1], M.metallic, a2, NdotL, NdotV, NdotH, VdotH);
    out[2] = shade_channel(M.color[2], M.metallic, a2, NdotL, NdotV, NdotH, VdotH);
    if (depth) depth[o] = best_z;
    if (face_id) face_id[o] = best_f + M.face_offset;
  } else {
    const size_t plane = (size_t)S * S, io = (size_t)b * 3 * plane + (size_t)r * S + c;
    out[0] = image ? image[io] : 1.f;
    out[1] = image ? image[io + plane] : 1.f;
    out[2] = image ? image[io + 2 * plane] : 1.f;
    if (depth) depth[o] = 0.f;
    if (face_id) face_id[o] = -1;
  }
  if (rgb) { rgb[3 * o] = out[0]; rgb[3 * o + 1] = out[1]; rgb[3 * o + 2] = out[2]; }
  if (rgb8) {
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb8[3 * o + k] = (unsigned char)floorf(fminf(fmaxf(255.f * out[k], 0.f), 255.f));
  }
}

}  // namespace

extern "C" long long hands_mesh_workspace_floats(int B, int n_verts) {
  if (B < 0 || n_verts < 0) return 0;
  return (long long)WS * B * n_verts;
}

extern "C" int hands_mesh_prepare_f32(const float* verts, int ld_verts, int n_verts, const int32_t* faces, int n_faces, const int32_t* csr_off, const int32_t* csr_face, const float* K, const float* T, int B, int S, float* workspace, hands_stream_t stream) {
  if (!verts || !faces || !csr_off || !csr_face || !K || !workspace || B <= 0 || S < 1 || S > 16384 || n_verts < 1 || n_faces < 0 ||
      ld_verts < 3 * n_verts)
    return HANDS_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return HANDS_EINVAL;       // written as float4
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3(hands_grid_1d((long long)B * n_verts, 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream,
                     verts, ld_verts, n_verts, faces, n_faces, csr_off, csr_face, K, T, B, S, workspace);
  HANDS_LAUNCH_CHECK();
}

extern "C" int hands_render_shaded_f32(const hands_shade_scene* scene, const float* image, int B, int S, float* rgb, unsigned char* rgb8, float* depth, int32_t* face_id, hands_stream_t stream) {
  if (!scene || B <= 0 || S < 1 || S > 16384 || scene->n_meshes < 1 || scene->n_meshes > HANDS_SHADE_MAX_MESHES) return HANDS_EINVAL;
  if (!rgb && !rgb8 && !depth && !face_id) return HANDS_EINVAL;
  hands_shade_scene sc = *scene;
  for (int m = 0; m < HANDS_SHADE_MAX_MESHES; ++m) {
    hands_shade_mesh& M = sc.mesh[m];
    if (m >= sc.n_meshes) { M = hands_shade_mesh{}; continue; }
    if (!M.workspace || !M.faces || M.n_verts < 1 || M.n_faces < 0 || (reinterpret_cast<uintptr_t>(M.workspace) & 15) != 0) return HANDS_EINVAL;
  }
  const int tiles_x = (S + TILE_W - 1) / TILE_W, tiles_y = (S + TILE_H - 1) / TILE_H;
  const long long blocks = (long long)tiles_x * tiles_y * B;
  if (blocks > 0x7fffffffLL) return HANDS_EINVAL;
  hipLaunchKernelGGL(render_shaded_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, sc, image, S, tiles_x,
                     tiles_x * tiles_y, rgb, rgb8, depth, face_id);
  HANDS_LAUNCH_CHECK();
}
