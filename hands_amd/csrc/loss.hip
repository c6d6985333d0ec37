// loss.hip -- the reference's validation loss dict (src/callbacks/loss/loss_arctic_sf.py:20-206 with
// src/utils/loss_modules.py:97-152 and the weighting / total of src/models/generic/wrapper.py:19-23,100-115), forward only,
// in two launches on the caller's stream:
//   A  loss_partials_kernel   grid = (term, chunk).  The mask / depth L1 terms are streamed as flat arrays, LARGE_CHUNK
//                             elements per workgroup with 16-byte loads; every other term takes SMALL_SAMPLES samples per
//                             workgroup.  Elements are formed in fp32 in the reference's operation order (difference -> square
//                             or abs -> x validity -> x is_*_loss), summed in fp64 (thread, wave shuffle, LDS) and the
//                             workgroup's partial goes to its own workspace slot with a plain store.  Three more "terms" sum
//                             the validity vectors the all-invalid rule needs.
//   B  loss_finish_kernel     one workgroup: sums every term's partials in a fixed order in fp64, divides by the element
//                             count, applies the all-invalid rule (loss_modules.py:101-105: a vector_loss term whose validity
//                             sums to zero is exactly 0, NaNs included -- the reference decides that with a host sync, here it
//                             is a select), and writes the 21 means, the 21 weighted values and their total as fp32.
// No atomics and no hand-off between workgroups inside a launch: the result is bit-reproducible from run to run.
// Grasp labels are assumed to lie in [0, 9); they are NOT checked on the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <initializer_list>
#include "hands_hip.h"
#include "common.h"
#include "rot_device.h"

namespace {

constexpr int NT = 256;               // threads per workgroup (4 waves)
constexpr int LARGE_CHUNK = 8192;     // elements of a streamed term per workgroup: 8 float4 per thread and tensor;
                                      // bz = 256, S = 224 -> 1568 chunks per tensor pair, 6272 workgroups on 256 CUs
                                      // (docs/EXPERIMENTS.md: 4096 / 8192 / 16384 measured)
constexpr int SMALL_SAMPLES = 32;     // samples of a small term per workgroup
constexpr int NJ = 21;
constexpr int NCLS = 9;               // grasp classes

// output keys in the reference's dict order, then the three validity sums
enum {
  K_CAMT_R = 0, K_CAMT_L, K_KP2D_R, K_KP3D_R, K_POSE_R, K_BETA_R, K_KP2D_L, K_KP3D_L, K_POSE_L, K_TRANSL_L, K_BETA_L,
  K_GRASP_R, K_GRASP_L, K_MASK_R, K_MASK_L, K_DEPTH_R, K_DEPTH_L, K_CENTER_R, K_CENTER_L, K_CORNER_R, K_CORNER_L,
  NKEY,
  V_R = NKEY, V_L, V_RL, NSLOT
};
static_assert(NKEY == HANDS_LOSS_NKEYS, "key count of hands_hip.h");

struct Layout { int nS, nM, nD; };    // chunks per small / mask / depth slot

__host__ __device__ inline bool is_mask_slot(int s) { return s == K_MASK_R || s == K_MASK_L; }
__host__ __device__ inline bool is_depth_slot(int s) { return s == K_DEPTH_R || s == K_DEPTH_L; }
__host__ __device__ inline int slot_chunks(int s, Layout L) { return is_mask_slot(s) ? L.nM : (is_depth_slot(s) ? L.nD : L.nS); }
__host__ __device__ inline long long slot_offset(int s, Layout L) {
  long long o = 0;
  for (int i = 0; i < s; ++i) o += slot_chunks(i, L);
  return o;
}

static inline long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// sum over the workgroup, valid on thread 0: shuffle tree inside each wave, then the waves in order
__device__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();                      // lds may still be read from the previous call
  if (lane == 0) lds[wave] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NT / 64; ++w) s += lds[w];
  return s;
}

// ---- the streamed terms: sum over [start, end) of |p - g| (* valid[b]) * flag[b], b = index / S2 ------------------------------
template <bool VEC>
__device__ double stream_l1(const float* __restrict__ p, const float* __restrict__ g, const float* __restrict__ valid,
                            const float* __restrict__ flag, long long start, long long end, int S2) {
  double acc = 0.0;
  long long i = start + (long long)threadIdx.x * 4;
  int b = (int)(i / S2);
  int r = (int)(i - (long long)b * S2);
  int cb = -1;                          // sample whose weights are in cv / cf
  float cv = 1.f, cf = 0.f;
#pragma unroll 2
  for (; i < end; i += NT * 4) {
    float pv[4], gv[4];
    int n = 4;
    if (VEC && i + 4 <= end) {
      const float4 P = *reinterpret_cast<const float4*>(p + i), G = *reinterpret_cast<const float4*>(g + i);
      pv[0] = P.x; pv[1] = P.y; pv[2] = P.z; pv[3] = P.w;
      gv[0] = G.x; gv[1] = G.y; gv[2] = G.z; gv[3] = G.w;
    } else {
      n = (int)(end - i < 4 ? end - i : 4);
      for (int k = 0; k < 4; ++k) {
        pv[k] = k < n ? p[i + k] : 0.f;
        gv[k] = k < n ? g[i + k] : 0.f;
      }
    }
    int bk = b, rk = r;                 // a vector may straddle two samples (or more, for S2 < 4)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        if (bk != cb) {
          cb = bk;
          cv = valid ? valid[bk] : 1.f;
          cf = flag[bk];
        }
        float e = fabsf(pv[k] - gv[k]);
        if (valid) e = e * cv;
        e = e * cf;
        acc += (double)e;
        if (++rk == S2) { rk = 0; ++bk; }
      }
    }
    r += NT * 4;
    if (r >= S2) {
      const int q = r / S2;
      b += q;
      r -= q * S2;
    }
  }
  return acc;
}

// ---- the small terms ------------------------------------------------------------------------------------------------------
// mse * valid[b] * flag[b] over D values per sample (vector_loss: beta, center, corner)
__device__ double vec_term(const float* p, const float* g, const float* valid, const float* flag, int D, int b0, int b1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < (b1 - b0) * D; i += NT) {
    const int b = b0 + i / D;
    const long long at = (long long)b0 * D + i;
    const float d = p[at] - g[at];
    float e = (d * d) * valid[b];
    if (flag) e = e * flag[b];
    acc += (double)e;
  }
  return acc;
}

// cam_t: the cam_t.wp and cam_t.wp.init terms against the same GT, summed per element, then x is_cam_loss
__device__ double camt_term(const float* p, const float* pi, const float* g, const float* valid, const float* flag, int b0,
                            int b1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < (b1 - b0) * 3; i += NT) {
    const int b = b0 + i / 3;
    const long long at = (long long)b0 * 3 + i;
    const float d0 = p[at] - g[at], d1 = pi[at] - g[at];
    const float e = ((d0 * d0) * valid[b] + (d1 * d1) * valid[b]) * flag[b];
    acc += (double)e;
  }
  return acc;
}

// transl/l: (cam_l - cam_r) of pred against the same of gt, under right_valid * left_valid
__device__ double transl_term(const hands_loss_in& in, int b0, int b1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < (b1 - b0) * 3; i += NT) {
    const int b = b0 + i / 3;
    const long long at = (long long)b0 * 3 + i;
    const float d = (in.pred_cam_wp_l[at] - in.pred_cam_wp_r[at]) - (in.gt_cam_wp_l[at] - in.gt_cam_wp_r[at]);
    const float e = ((d * d) * (in.right_valid[b] * in.left_valid[b])) * in.is_cam_loss[b];
    acc += (double)e;
  }
  return acc;
}

// kp2d (C = 2) and the root-relative kp3d (C = 3): joints_loss, x joints_valid[b, j] x flag[b]
template <int C, bool ROOT_REL>
__device__ double joints_term(const float* p, const float* g, const float* jvalid, const float* flag, int b0, int b1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < (b1 - b0) * NJ * C; i += NT) {
    const int b = b0 + i / (NJ * C), jc = i % (NJ * C), j = jc / C, c = jc % C;
    const long long row = (long long)b * NJ * C;
    float pv = p[row + jc], gv = g[row + jc];
    if (ROOT_REL) {                     // hand_kp3d_loss subtracts joint 0 twice; the second time it is 0
      pv = pv - p[row + c];
      gv = gv - g[row + c];
    }
    const float d = pv - gv;
    const float e = ((d * d) * jvalid[(long long)b * NJ + j]) * flag[b];
    acc += (double)e;
  }
  return acc;
}

// pose: pred rotation matrices (B,16,3,3) against GT axis-angle (B,48) turned into matrices; one thread per joint
__device__ double pose_term(const float* p, const float* g_aa, const float* valid, const float* flag, int b0, int b1) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < (b1 - b0) * 16; i += NT) {
    const int b = b0 + i / 16;
    const long long at = (long long)b0 * 16 + i;
    float R[9];
    hands::axis_angle_to_matrix(g_aa + at * 3, R);
    const float v = valid[b], f = flag[b];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float d = p[at * 9 + k] - R[k];
      const float e = ((d * d) * v) * f;
      acc += (double)e;
    }
  }
  return acc;
}

// grasp: 9-way cross-entropy (stable log-sum-exp) x grasp_valid x is_grasp_loss.  The label is not range-checked.
__device__ double grasp_term(const float* logits, const long long* label, const float* valid, const float* flag, int b0,
                             int b1) {
  double acc = 0.0;
  for (int b = b0 + threadIdx.x; b < b1; b += NT) {
    const float* x = logits + (long long)b * NCLS;
    float m = x[0];
    for (int k = 1; k < NCLS; ++k) m = fmaxf(m, x[k]);
    float s = 0.f;
    for (int k = 0; k < NCLS; ++k) s += expf(x[k] - m);
    const float ce = logf(s) - (x[label[b]] - m);
    const float e = (ce * valid[b]) * flag[b];
    acc += (double)e;
  }
  return acc;
}

__device__ double valid_sum(const float* a, const float* b2, int b0, int b1) {
  double acc = 0.0;
  for (int b = b0 + threadIdx.x; b < b1; b += NT) acc += (double)(b2 ? a[b] * b2[b] : a[b]);
  return acc;
}

// the small slots in launch order
__constant__ const int SMALL_SLOTS[] = {K_CAMT_R, K_CAMT_L, K_KP2D_R, K_KP3D_R, K_POSE_R, K_BETA_R, K_KP2D_L, K_KP3D_L,
                                        K_POSE_L, K_TRANSL_L, K_BETA_L, K_GRASP_R, K_GRASP_L, K_CENTER_R, K_CENTER_L,
                                        K_CORNER_R, K_CORNER_L, V_R, V_L, V_RL};
constexpr int NSMALL = 20;

template <bool VEC>
__global__ __launch_bounds__(NT) void loss_partials_kernel(hands_loss_in in, int B, int S2m, int S2d, Layout L,
                                                           double* __restrict__ ws) {
  __shared__ double lds[NT / 64];
  const int blk = blockIdx.x;
  int slot, chunk;
  double acc;
  if (blk < 2 * L.nM + 2 * L.nD) {
    const bool mask = blk < 2 * L.nM;
    const int t = mask ? blk : blk - 2 * L.nM, per = mask ? L.nM : L.nD;
    const bool left = t >= per;
    chunk = left ? t - per : t;
    slot = mask ? (left ? K_MASK_L : K_MASK_R) : (left ? K_DEPTH_L : K_DEPTH_R);
    const int S2 = mask ? S2m : S2d;
    const long long n = (long long)B * S2, start = (long long)chunk * LARGE_CHUNK;
    const long long end = start + LARGE_CHUNK < n ? start + LARGE_CHUNK : n;
    const float* p = mask ? (left ? in.pred_mask_l : in.pred_mask_r) : (left ? in.pred_depth_l : in.pred_depth_r);
    const float* g = mask ? (left ? in.gt_mask_l : in.gt_mask_r) : (left ? in.gt_depth_l : in.gt_depth_r);
    const float* valid = mask ? (left ? in.render_valid_l : in.render_valid_r) : nullptr;   // depth: a plain L1
    acc = stream_l1<VEC>(p, g, valid, mask ? in.is_mask_loss : in.is_depth_loss, start, end, S2);
  } else {
    const int t = blk - (2 * L.nM + 2 * L.nD);
    slot = SMALL_SLOTS[t / L.nS];
    chunk = t % L.nS;
    const int b0 = chunk * SMALL_SAMPLES, b1 = b0 + SMALL_SAMPLES < B ? b0 + SMALL_SAMPLES : B;
    switch (slot) {
      case K_CAMT_R: acc = camt_term(in.pred_cam_wp_r, in.pred_cam_wp_init_r, in.gt_cam_wp_r, in.right_valid, in.is_cam_loss, b0, b1); break;
      case K_CAMT_L: acc = camt_term(in.pred_cam_wp_l, in.pred_cam_wp_init_l, in.gt_cam_wp_l, in.left_valid, in.is_cam_loss, b0, b1); break;
      case K_KP2D_R: acc = joints_term<2, false>(in.pred_j2d_r, in.gt_j2d_r, in.joints_valid_r, in.is_j2d_loss, b0, b1); break;
      case K_KP2D_L: acc = joints_term<2, false>(in.pred_j2d_l, in.gt_j2d_l, in.joints_valid_l, in.is_j2d_loss, b0, b1); break;
      case K_KP3D_R: acc = joints_term<3, true>(in.pred_j3d_r, in.gt_j3d_r, in.joints_valid_r, in.is_j3d_loss, b0, b1); break;
      case K_KP3D_L: acc = joints_term<3, true>(in.pred_j3d_l, in.gt_j3d_l, in.joints_valid_l, in.is_j3d_loss, b0, b1); break;
      case K_POSE_R: acc = pose_term(in.pred_pose_r, in.gt_pose_r, in.right_valid, in.is_pose_loss, b0, b1); break;
      case K_POSE_L: acc = pose_term(in.pred_pose_l, in.gt_pose_l, in.left_valid, in.is_pose_loss, b0, b1); break;
      case K_BETA_R: acc = vec_term(in.pred_beta_r, in.gt_beta_r, in.right_valid, in.is_beta_loss, 10, b0, b1); break;
      case K_BETA_L: acc = vec_term(in.pred_beta_l, in.gt_beta_l, in.left_valid, in.is_beta_loss, 10, b0, b1); break;
      case K_TRANSL_L: acc = transl_term(in, b0, b1); break;
      case K_GRASP_R:
        if (!in.pred_grasp_r) return;
        acc = grasp_term(in.pred_grasp_r, in.gt_grasp_r, in.grasp_valid_r, in.is_grasp_loss, b0, b1); break;
      case K_GRASP_L:
        if (!in.pred_grasp_r) return;
        acc = grasp_term(in.pred_grasp_l, in.gt_grasp_l, in.grasp_valid_l, in.is_grasp_loss, b0, b1); break;
      case K_CENTER_R:
        if (!in.pred_center_r) return;
        acc = vec_term(in.pred_center_r, in.gt_center_r, in.right_valid, nullptr, 2, b0, b1); break;
      case K_CENTER_L:
        if (!in.pred_center_r) return;
        acc = vec_term(in.pred_center_l, in.gt_center_l, in.left_valid, nullptr, 2, b0, b1); break;
      case K_CORNER_R:
        if (!in.pred_center_r) return;
        acc = vec_term(in.pred_corner_r, in.gt_corner_r, in.right_valid, nullptr, 8, b0, b1); break;
      case K_CORNER_L:
        if (!in.pred_center_r) return;
        acc = vec_term(in.pred_corner_l, in.gt_corner_l, in.left_valid, nullptr, 8, b0, b1); break;
      case V_R: acc = valid_sum(in.right_valid, nullptr, b0, b1); break;
      case V_L: acc = valid_sum(in.left_valid, nullptr, b0, b1); break;
      default: acc = valid_sum(in.right_valid, in.left_valid, b0, b1); break;      // V_RL
    }
  }
  const double s = block_sum(acc, lds);      // every early return above is uniform over the workgroup
  if (threadIdx.x == 0) ws[slot_offset(slot, L) + chunk] = s;
}

__global__ __launch_bounds__(NT) void loss_finish_kernel(const double* __restrict__ ws, int B, int S2m, int S2d, Layout L,
                                                         unsigned present, float* __restrict__ out_unweighted,
                                                         float* __restrict__ out_weighted, float* __restrict__ out_total) {
  __shared__ double sums[NSLOT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // one wave per slot: lane i adds the partials of its contiguous segment in index order, a shuffle tree adds the 64 segment
  // sums -- a fixed association, the same in every run
  for (int s = wave; s < NSLOT; s += NT / 64) {
    const int n = slot_chunks(s, L);
    const bool on = s >= NKEY || ((present >> s) & 1u);
    const double* part = ws + slot_offset(s, L);
    const int seg = (n + 63) / 64;
    double a = 0.0;
    if (on)
      for (int i = lane * seg; i < n && i < (lane + 1) * seg; ++i) a += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if (lane == 0) sums[s] = a;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // elements per sample, weight, and the validity sum the all-invalid rule reads (-1: the term has no such rule)
  const double per_sample[NKEY] = {3, 3, 42, 63, 144, 10, 42, 63, 144, 3, 10, 1, 1, (double)S2m, (double)S2m, (double)S2d,
                                   (double)S2d, 2, 2, 8, 8};
  const float weight[NKEY] = {1.0f, 1.0f, 5.0f, 5.0f, 10.0f, 0.001f, 5.0f, 5.0f, 10.0f, 1.0f, 0.001f, 0.1f, 0.1f, 10.0f,
                              10.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
  const int rule[NKEY] = {V_R, V_L, -1, -1, V_R, V_R, -1, -1, V_L, V_RL, V_L, -1, -1, -1, -1, -1, -1, V_R, V_L, V_R, V_L};
  float total = 0.0f;
  for (int k = 0; k < NKEY; ++k) {
    float u = 0.0f, w = 0.0f;
    if ((present >> k) & 1u) {
      u = (float)(sums[k] / ((double)B * per_sample[k]));
      if (rule[k] >= 0 && sums[rule[k]] == 0.0) u = 0.0f;
      w = u * weight[k];
      total += w;
    }
    out_unweighted[k] = u;
    out_weighted[k] = w;
  }
  out_total[0] = total;
}

bool layout_of(int B, int S_mask, int S_depth, Layout* L) {
  if (B <= 0 || S_mask < 0 || S_depth < 0 || S_mask > 32768 || S_depth > 32768) return false;
  const long long nM = ceil_div((long long)B * S_mask * S_mask, LARGE_CHUNK);
  const long long nD = ceil_div((long long)B * S_depth * S_depth, LARGE_CHUNK);
  const long long nS = ceil_div(B, SMALL_SAMPLES);
  if (2 * nM + 2 * nD + NSMALL * nS > 0x7fffffffLL) return false;
  L->nS = (int)nS; L->nM = (int)nM; L->nD = (int)nD;
  return true;
}

}  // namespace

extern "C" long long hands_loss_workspace_bytes(int B, int S_mask, int S_depth) {
  Layout L;
  if (!layout_of(B, S_mask, S_depth, &L)) return 0;
  return (long long)sizeof(double) * slot_offset(NSLOT, L);
}

extern "C" int hands_loss_light_f32(const hands_loss_in* in, int B, int S_mask, int S_depth, void* workspace,
                                    float* out_unweighted21, float* out_weighted21, float* out_total, hands_stream_t stream) {
  if (!in || !workspace || !out_unweighted21 || !out_weighted21 || !out_total || B <= 0) return HANDS_EINVAL;
  if (((uintptr_t)workspace & 7u) != 0) return HANDS_EINVAL;
  const void* const* p = reinterpret_cast<const void* const*>(in);
  for (int i = 0; i < HANDS_LOSS_N_MANDATORY; ++i)
    if (!p[i]) return HANDS_EINVAL;
  // an optional group is all there or all absent
  auto group = [&](std::initializer_list<const void*> g, bool* on) {
    size_t n = 0;
    for (const void* q : g) n += q != nullptr;
    *on = n == g.size();
    return n == 0 || n == g.size();
  };
  bool grasp, mask, depth, cc;
  if (!group({in->pred_grasp_r, in->pred_grasp_l, in->gt_grasp_r, in->gt_grasp_l, in->grasp_valid_r, in->grasp_valid_l,
              in->is_grasp_loss}, &grasp) ||
      !group({in->pred_mask_r, in->pred_mask_l, in->gt_mask_r, in->gt_mask_l, in->render_valid_r, in->render_valid_l,
              in->is_mask_loss}, &mask) ||
      !group({in->pred_depth_r, in->pred_depth_l, in->gt_depth_r, in->gt_depth_l, in->is_depth_loss}, &depth) ||
      !group({in->pred_center_r, in->pred_center_l, in->gt_center_r, in->gt_center_l, in->pred_corner_r, in->pred_corner_l,
              in->gt_corner_r, in->gt_corner_l}, &cc))
    return HANDS_EINVAL;
  if ((mask && S_mask <= 0) || (depth && S_depth <= 0)) return HANDS_EINVAL;
  Layout L;
  if (!layout_of(B, mask ? S_mask : 0, depth ? S_depth : 0, &L)) return HANDS_EINVAL;
  unsigned present = (1u << K_GRASP_R) - 1u;                      // the 11 base keys
  if (grasp) present |= (1u << K_GRASP_R) | (1u << K_GRASP_L);
  if (mask) present |= (1u << K_MASK_R) | (1u << K_MASK_L);
  if (depth) present |= (1u << K_DEPTH_R) | (1u << K_DEPTH_L);
  if (cc) present |= (1u << K_CENTER_R) | (1u << K_CENTER_L) | (1u << K_CORNER_R) | (1u << K_CORNER_L);
  bool vec = true;                                                // 16-byte loads need 16-byte aligned tensors
  for (const void* q : {(const void*)in->pred_mask_r, (const void*)in->pred_mask_l, (const void*)in->gt_mask_r,
                        (const void*)in->gt_mask_l, (const void*)in->pred_depth_r, (const void*)in->pred_depth_l,
                        (const void*)in->gt_depth_r, (const void*)in->gt_depth_l})
    vec = vec && ((uintptr_t)q & 15u) == 0;
  const int grid = 2 * L.nM + 2 * L.nD + NSMALL * L.nS;
  const int S2m = mask ? S_mask * S_mask : 0, S2d = depth ? S_depth * S_depth : 0;
  double* ws = static_cast<double*>(workspace);
  if (vec)
    hipLaunchKernelGGL(loss_partials_kernel<true>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, *in, B, S2m, S2d, L, ws);
  else
    hipLaunchKernelGGL(loss_partials_kernel<false>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, *in, B, S2m, S2d, L, ws);
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, ws, B, S2m, S2d, L, present,
                     out_unweighted21, out_weighted21, out_total);
  HANDS_LAUNCH_CHECK();
}
