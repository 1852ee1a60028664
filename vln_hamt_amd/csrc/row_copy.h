// What the gather kernels share (obs.hip, pretrain_gather.hip): one wave copies one row, and a wave-wide OR builds the mask of the views
// a viewpoint's candidates point to.  Wave shuffles only; no arithmetic touches a copied value.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t wave_or_u(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// dst[0..n) = src[0..n), or zeros for a NULL src
__device__ __forceinline__ void copy_row(float* __restrict__ dst, const float* __restrict__ src, int n, bool vec, int lane) {
  if (vec) {
    f32x4* __restrict__ d = reinterpret_cast<f32x4*>(dst);
    const f32x4* __restrict__ s = reinterpret_cast<const f32x4*>(src);
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = lane; i < (n >> 2); i += 64) d[i] = src ? s[i] : zero;
  } else {
    for (int i = lane; i < n; i += 64) dst[i] = src ? src[i] : 0.0f;
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
