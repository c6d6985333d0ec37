// smooth.hip -- temporal smoothing on device (hands_smooth_mano_f32, hands_smooth_state_bytes of include/hands_hip.h): the
// One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) over the MANO parameters of a stream of frames, rotations filtered on SO(3).
// DESIGN.md section 7 "Temporal smoothing" is the specification, tests/smooth_ref.py its fp64 restatement.
// One launch filters every hand-stream of a call: one wave per (side, stream), grid (S, nsides).  Lanes 0..15 own the 16
// rotation channels, lane 16 the shape vector, lane 17 the camera vector; the other lanes idle.  Time is a serial loop of T steps
// inside the kernel -- the recurrence is non-linear -- with the inputs of step t + 1 loaded before the arithmetic of step t.
// A lane keeps its channel's state in registers (fp64, at most 40 values, constant indices only: no scratch), checks the
// finiteness of the inputs it loaded, and the wave agrees on "all 157 finite" with one vote.  fp32 in, fp64 arithmetic, one
// rounding per output; a frame that is passed through is copied as bits.  No atomics, no inter-workgroup synchronisation,
// every loop is bounded by T.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hands_hip.h"
#include "common.h"

namespace {

constexpr int NROT = 16;
constexpr int ROT_ST = 21;                       // raw (9), hat (9), derivative estimate (3)
constexpr int SHAPE_ST = 40;                     // raw, hat, derivative estimate, sum (10 each)
constexpr int CAM_ST = 9;                        // raw, hat, derivative estimate (3 each)
constexpr int ST_SHAPE = NROT * ROT_ST;          // 336
constexpr int ST_CAM = ST_SHAPE + SHAPE_ST;      // 376
constexpr int ST_ID = ST_CAM + CAM_ST;           // 385: the id, then the live flag, then the count, int64 each
constexpr int ST_WORDS = ST_ID + 3;              // 388 words of 8 bytes
constexpr int MAXV = 10;                         // floats a lane reads and writes per frame, at most
constexpr int MAXST = SHAPE_ST;

constexpr double PI = 3.14159265358979323846;

__device__ __forceinline__ double alpha(double f, double dt) {
  const double r = 2.0 * PI * f * dt;
  return r / (r + 1.0);
}

// D = A^T B, row-major 3x3
__device__ __forceinline__ void mul_tn(const double* A, const double* B, double* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}

__device__ __forceinline__ void mul_nn(const double* A, const double* B, double* D) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) D[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ void log_so3(const double* D, double* w) {
  const double v0 = 0.5 * (D[7] - D[5]), v1 = 0.5 * (D[2] - D[6]), v2 = 0.5 * (D[3] - D[1]);
  const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  const double c = 0.5 * (((D[0] + D[4]) + D[8]) - 1.0);
  if (s >= 1e-9) {
    const double k = atan2(s, c) / s;
    w[0] = v0 * k; w[1] = v1 * k; w[2] = v2 * k;
  } else if (c >= 0.0) {
    w[0] = v0; w[1] = v1; w[2] = v2;
  } else {                                       // a half turn: the axis from the symmetric part
    double u0 = sqrt(fmax(0.0, (D[0] - c) / (1.0 - c)));
    double u1 = sqrt(fmax(0.0, (D[4] - c) / (1.0 - c)));
    double u2 = sqrt(fmax(0.0, (D[8] - c) / (1.0 - c)));
    const double s01 = D[1] + D[3], s02 = D[2] + D[6], s12 = D[5] + D[7];
    if (u0 >= u1 && u0 >= u2) {                  // the largest, the lowest index on a tie
      u1 = s01 < 0.0 ? -u1 : u1;
      u2 = s02 < 0.0 ? -u2 : u2;
    } else if (u1 >= u2) {
      u0 = s01 < 0.0 ? -u0 : u0;
      u2 = s12 < 0.0 ? -u2 : u2;
    } else {
      u0 = s02 < 0.0 ? -u0 : u0;
      u1 = s12 < 0.0 ? -u1 : u1;
    }
    const double k = PI / sqrt((u0 * u0 + u1 * u1) + u2 * u2);
    w[0] = u0 * k; w[1] = u1 * k; w[2] = u2 * k;
  }
}

__device__ __forceinline__ void exp_so3(const double* w, double* E) {
  const double theta = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double K2[9];
  mul_nn(K, K, K2);
  double a = 1.0, b = 0.5;
  if (theta >= 1e-6) {
    double sn, cs;
    sincos(theta, &sn, &cs);
    a = sn / theta;
    b = (1.0 - cs) / (theta * theta);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * K[i]) + b * K2[i];
}

// st: raw [0, 9), hat [9, 18), derivative estimate [18, 21)
__device__ __forceinline__ void rotation_update(double* st, const float* x, float* o, double dt, double mc, double be, double dc) {
  double R[9], D[9], w[3], E[9], H[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (double)x[i];
  mul_tn(st, R, D);
  log_so3(D, w);
  const double ad = alpha(dc, dt);
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    st[18 + i] += ad * (w[i] / dt - st[18 + i]);
    n2 += st[18 + i] * st[18 + i];
  }
  const double a = alpha(mc + be * sqrt(n2), dt);
  mul_tn(st + 9, R, D);
  log_so3(D, w);
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] *= a;
  exp_so3(w, E);
  mul_nn(st + 9, E, H);
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    st[9 + i] = H[i];
    st[i] = R[i];
    o[i] = (float)H[i];
  }
}

// st: raw [0, N), hat [N, 2N), derivative estimate [2N, 3N)
template <int N>
__device__ __forceinline__ void vector_update(double* st, const float* x, float* o, double dt, double mc, double be, double dc) {
  const double ad = alpha(dc, dt);
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double d = ((double)x[i] - st[i]) / dt;
    st[2 * N + i] += ad * (d - st[2 * N + i]);
    n2 += st[2 * N + i] * st[2 * N + i];
  }
  const double a = alpha(mc + be * sqrt(n2), dt);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    st[N + i] += a * ((double)x[i] - st[N + i]);
    st[i] = (double)x[i];
    o[i] = (float)st[N + i];
  }
}

struct Sides {
  hands_smooth_side s[2];
};

__global__ void __launch_bounds__(64) smooth_kernel(Sides sides, const long long* __restrict__ seq, int T, int S, double dt,
                                                    hands_smooth_cfg cfg) {
  const int lane = threadIdx.x, s = blockIdx.x;
  const hands_smooth_side& sd = sides.s[blockIdx.y];
  // what this lane owns: nv floats of a frame at in / out + row * ld, nst state values from word st_off on
  const bool is_rot = lane < NROT, is_shape = lane == NROT, is_cam = lane == NROT + 1;
  const int nv = is_rot ? 9 : (is_shape ? 10 : (is_cam ? 3 : 0));
  const int ld = is_rot ? 144 : (is_shape ? 10 : 3);
  const int nst = is_rot ? ROT_ST : (is_shape ? SHAPE_ST : (is_cam ? CAM_ST : 0));
  const int st_off = is_rot ? lane * ROT_ST : (is_shape ? ST_SHAPE : ST_CAM);
  const float* in = is_rot ? sd.pose + 9 * lane : (is_shape ? sd.beta : sd.cam);
  float* out = is_rot ? sd.pose_out + 9 * lane : (is_shape ? sd.beta_out : sd.cam_out);
  double* state = sd.state ? reinterpret_cast<double*>(sd.state) + (long long)s * ST_WORDS : nullptr;

  double st[MAXST];
  long long id = 0, live = 0, count = 0;         // id and live are the same on every lane; the count is the shape lane's
#pragma unroll
  for (int i = 0; i < MAXST; ++i) st[i] = (state && i < nst) ? state[st_off + i] : 0.0;
  if (state) {
    const long long* w = reinterpret_cast<const long long*>(state + ST_ID);
    id = w[0]; live = w[1]; count = w[2];
  }

  float nxt[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) nxt[i] = i < nv ? in[(long long)s * ld + i] : 0.f;
  for (int t = 0; t < T; ++t) {
    const long long row = (long long)t * S + s;
    float x[MAXV], o[MAXV];
    bool fin = true;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      x[i] = nxt[i];
      o[i] = x[i];
      fin = fin && isfinite(x[i]);
    }
    if (t + 1 < T) {
#pragma unroll
      for (int i = 0; i < MAXV; ++i) nxt[i] = i < nv ? in[(row + S) * ld + i] : 0.f;
    }
    const bool usable = (sd.valid ? sd.valid[row] != 0.f : true) && __all(fin);
    const long long sid = seq ? seq[row] : id;
    if (!usable) {
      live = 0;
    } else if (!(live && sid == id)) {           // a stream starts here: raw = hat = input, the estimates 0, sum = beta, count 1
      live = 1; id = sid; count = 1;
      if (is_rot) {
#pragma unroll
        for (int i = 0; i < 9; ++i) st[i] = st[9 + i] = (double)x[i];
        st[18] = st[19] = st[20] = 0.0;
      } else if (is_shape) {
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          st[i] = st[10 + i] = st[30 + i] = (double)x[i];
          st[20 + i] = 0.0;
        }
      } else if (is_cam) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          st[i] = st[3 + i] = (double)x[i];
          st[6 + i] = 0.0;
        }
      }
    } else {
      if (is_rot) {
        rotation_update(st, x, o, dt, cfg.min_cutoff[0], cfg.beta[0], cfg.d_cutoff[0]);
      } else if (is_shape) {
        if (cfg.shape_mode == HANDS_SMOOTH_SHAPE_FILTER) {
          vector_update<10>(st, x, o, dt, cfg.min_cutoff[1], cfg.beta[1], cfg.d_cutoff[1]);
        } else if (cfg.shape_mode == HANDS_SMOOTH_SHAPE_MEAN) {
          count += 1;
#pragma unroll
          for (int i = 0; i < 10; ++i) {
            st[30 + i] += (double)x[i];
            o[i] = (float)(st[30 + i] / (double)count);
          }
        }
      } else if (is_cam) {
        vector_update<3>(st, x, o, dt, cfg.min_cutoff[2], cfg.beta[2], cfg.d_cutoff[2]);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXV; ++i)
      if (i < nv) out[row * ld + i] = o[i];
  }

  if (state) {
#pragma unroll
    for (int i = 0; i < MAXST; ++i)
      if (i < nst) state[st_off + i] = st[i];
    if (is_shape) {                              // the count moves on this lane alone
      long long* w = reinterpret_cast<long long*>(state + ST_ID);
      w[0] = id; w[1] = live; w[2] = count;
    }
  }
}

bool positive(double v) { return isfinite(v) && v > 0.0; }

}  // namespace

extern "C" long long hands_smooth_state_bytes(void) { return (long long)ST_WORDS * 8; }

extern "C" int hands_smooth_mano_f32(const hands_smooth_side* sides, int nsides, const long long* seq_id, int T, int S, float fps,
                                     const hands_smooth_cfg* cfg, hands_stream_t stream) {
  if (!sides || !cfg || nsides < 1 || nsides > 2 || T < 1 || S < 1 || !positive((double)fps)) return HANDS_EINVAL;
  for (int g = 0; g < 3; ++g)
    if (!positive(cfg->min_cutoff[g]) || !positive(cfg->d_cutoff[g]) || !isfinite(cfg->beta[g]) || cfg->beta[g] < 0.0)
      return HANDS_EINVAL;
  if (cfg->shape_mode != HANDS_SMOOTH_SHAPE_FILTER && cfg->shape_mode != HANDS_SMOOTH_SHAPE_MEAN &&
      cfg->shape_mode != HANDS_SMOOTH_SHAPE_NONE)
    return HANDS_EINVAL;
  Sides k;
  for (int i = 0; i < 2; ++i) {
    k.s[i] = sides[i < nsides ? i : 0];
    const hands_smooth_side& d = k.s[i];
    if (!d.pose || !d.beta || !d.cam || !d.pose_out || !d.beta_out || !d.cam_out) return HANDS_EINVAL;
  }
  hipLaunchKernelGGL(smooth_kernel, dim3(S, nsides), dim3(64), 0, (hipStream_t)stream, k, seq_id, T, S, 1.0 / (double)fps, *cfg);
  HANDS_LAUNCH_CHECK();
}
