// common.h -- shared helpers for the gfx950 kernels of libhands_hip.so
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define HANDS_LAUNCH_CHECK() return (int)hipGetLastError()

static inline int hands_grid_1d(long long work, int block, int cap = 256 * 8) {
  long long g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// vit_b.hip: the (T, head_dim) = (197, 64) launch behind hands_attention_f32 (transformer.hip)
__attribute__((visibility("hidden"))) int hands_detail_attention_t197_d64(const float* qkv, float* out, int B, int heads, float scale, hipStream_t stream);
