// PIL's 8-bit two-pass resample (Resample.c), the arithmetic that image_prep.hip (crop box -> 224 x 224, bicubic, taps made on the
// device) and image_resample.hip (whole view -> window of (OH, OW), bicubic | Lanczos, taps made on the host) share.  Both are PIL's
// bit for bit, so this is PIL's order of operations, not an approximation of it:
//  * taps (precompute_coeffs + normalize_coeffs_8bpc): in double; bounds (int)(center -+ support + 0.5) clamped to [0, in], the
//    sequential sum ww, w / ww when ww != 0, (int)(-+0.5 + w * 2^22).  A contracted multiply-add would change taps: this header
//    turns FMA contraction off for itself and for the file that includes it.
//  * a pass: clip8((2^21 + sum k p) >> 22) in int32; the horizontal pass's uint8 result feeds the vertical pass.
// The bicubic filter is pure arithmetic and runs on either side.  Lanczos needs sin(): the host's libm is what PIL calls, the
// device's sin is not, so the Lanczos filter is a host function and no tap that needs it is ever computed on the device.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

#define PIL_ONE (1 << 22)                // 1.0 in the 22-bit fixed point of the taps

struct pil_bicubic {                     // PIL's bicubic_filter (a = -0.5)
  static constexpr double support = 2.0;
  __host__ __device__ static inline double eval(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((1.5 * x - 2.5) * x) * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5;
    return 0.0;
  }
};

struct pil_lanczos {                     // PIL's lanczos_filter: truncated sinc.  Host only (libm's sin)
  static constexpr double support = 3.0;
  static inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * 3.14159265358979323846;
    return sin(x) / x;
  }
  static inline double eval(double x) {
    if (-3.0 <= x && x < 3.0) return sinc(x) * sinc(x / 3);
    return 0.0;
  }
};

// taps per output coordinate of an axis in -> out
__host__ __device__ static inline int pil_ksize(int in, int out, double support) {
  const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale;
  return (int)ceil(support * fs) * 2 + 1;
}

// the taps of output coordinate xx of an axis in -> out (box origin 0): k[0 .. *xcnt) weigh input [*xmin, *xmin + *xcnt).  The count
// is clamped to `cap`, the entries of k the caller has; k beyond the count is not written.  The filter is evaluated once for the
// sum and once for the weight (the same value: a pure function of the same argument), so that no array of weights is needed.
template <class F>
__host__ __device__ static inline void pil_taps(int xx, int in, int out, int* __restrict__ k, int cap, int* xmin, int* xcnt) {
  const double scale = (double)in / out;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = F::support * fs, ss = 1.0 / fs;
  const double center = (xx + 0.5) * scale;
  int x0 = (int)(center - support + 0.5);
  if (x0 < 0) x0 = 0;
  int x1 = (int)(center + support + 0.5);
  if (x1 > in) x1 = in;
  int cnt = x1 - x0;
  if (cnt > cap) cnt = cap;
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww += F::eval((x + x0 - center + 0.5) * ss);
  for (int x = 0; x < cnt; ++x) {
    double w = F::eval((x + x0 - center + 0.5) * ss);
    if (ww != 0.0) w /= ww;
    k[x] = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
  }
  *xmin = x0;
  *xcnt = cnt;
}

__host__ __device__ __forceinline__ int pil_clip8(int acc) {
  const int v = acc >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// one output sample of a pass: clip8(2^21 + sum_t k[t] * p[t * stride]), for one channel and for the three interleaved channels of a
// pixel.  Plain scalar accumulators: with an array of them the compiler merges the byte loads of neighbouring taps into wide
// unaligned ones, which measured 13-15 % slower on both resize kernels (profiles/pil_resample_refactor_resources.txt).
#define PIL_HALF (1 << 21)
__host__ __device__ __forceinline__ int pil_sample1(const uint8_t* p, int stride, const int* k, int n) {
  int acc = PIL_HALF;
  for (int t = 0; t < n; ++t) acc += (int)p[t * stride] * k[t];
  return pil_clip8(acc);
}
__host__ __device__ __forceinline__ void pil_sample3(const uint8_t* p, int stride, const int* k, int n, int& r, int& g, int& b) {
  int a0 = PIL_HALF, a1 = PIL_HALF, a2 = PIL_HALF;
  for (int t = 0; t < n; ++t) {
    const int kt = k[t];
    a0 += (int)p[t * stride] * kt; a1 += (int)p[t * stride + 1] * kt; a2 += (int)p[t * stride + 2] * kt;
  }
  r = pil_clip8(a0); g = pil_clip8(a1); b = pil_clip8(a2);
}
