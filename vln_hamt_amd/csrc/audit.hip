// Range watch on a dense layer's output (include/hamt.h: hamt_range_audit): one pass over the [M, N] elements the GEMM in front just
// wrote, folded into a four-word device record --
//   rec[0] += elements AT HALF'S LIMIT, |x| == 65504 (bits 0x7BFF under the sign), HAMT_F16 only.  The half store (common.h: pack_h2)
//             clamps at +-65504, so every overflow arrives as exactly this value; a result that rounds to 65504 by itself (65488 < |v|
//             <= 65504 before the rounding) is counted as well: the count is an upper bound on the clamps, and 0 proves there were none.
//   rec[1] += non-finite elements (exponent field all ones: inf and NaN)
//   rec[2]  = max(rec[2], float32 bits of the largest FINITE |x|), widened exactly from half / bf16
//   rec[3] += 1 per call
// Nothing is converted per element: with the sign dropped, the bit patterns of one format order like the magnitudes they encode, so a
// lane keeps the largest finite PATTERN and thread 0 of the workgroup widens that one value.  Integer atomics only (add, max): the
// record is the same whatever order the workgroups retire in.  At most one atomic per field per workgroup, none for a contribution
// of zero (the normal case for rec[0] / rec[1]) nor for a maximum the record already holds.
//
// Work is cut into UNITS: a row is N / V 16-byte vectors (V = 8 half / bf16, 4 fp32 elements) plus, when N % V != 0, one unit that walks
// the N % V tail elements one by one -- the element-wise path is the same kernel with V = 1.  Units are numbered row-major and taken
// grid-stride, 256 lanes per workgroup, at most kMaxBlocks workgroups (4 per CU of a 256-CU part), the (row, unit-in-row) pair advanced
// by the stride without a division.  Only the M x N elements named are ever read.  LDS: the 4-wave hand-off; no scratch.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

typedef unsigned long long u64;

// the format's view of one element's bits: magnitude pattern, where non-finite starts, the at-the-limit pattern (0: none)
struct FmtF16 { typedef uint16_t raw; static constexpr uint32_t kAbs = 0x7fffu, kInf = 0x7c00u, kLimit = 0x7bffu; };
struct FmtBF16 { typedef uint16_t raw; static constexpr uint32_t kAbs = 0x7fffu, kInf = 0x7f80u, kLimit = 0u; };
struct FmtF32 { typedef uint32_t raw; static constexpr uint32_t kAbs = 0x7fffffffu, kInf = 0x7f800000u, kLimit = 0u; };

__device__ __forceinline__ uint32_t widen_bits(FmtF16, uint32_t a) { return __float_as_uint((float)__builtin_bit_cast(_Float16, (uint16_t)a)); }
__device__ __forceinline__ uint32_t widen_bits(FmtBF16, uint32_t a) { return a << 16; }
__device__ __forceinline__ uint32_t widen_bits(FmtF32, uint32_t a) { return a; }

struct Tally { uint32_t limit, nonfinite, amax; };

template <class F>
__device__ __forceinline__ void tally(uint32_t bits, Tally& t) {
  const uint32_t a = bits & F::kAbs;
  const bool fin = a < F::kInf;
  if (F::kLimit != 0u) t.limit += (a == F::kLimit) ? 1u : 0u;
  t.nonfinite += fin ? 0u : 1u;
  t.amax = max(t.amax, fin ? a : 0u);
}
template <class F>
__device__ __forceinline__ void tally_word(uint32_t w, Tally& t) {       // one 32-bit word of a 16-byte vector: one or two elements
  if (sizeof(typename F::raw) == 2) { tally<F>(w & 0xffffu, t); tally<F>(w >> 16, t); }
  else tally<F>(w, t);
}

// V: elements per vector unit (16 / sizeof(raw)), or 1 for the element-wise path
template <class F, int V>
__global__ __launch_bounds__(kThreads) void range_audit_kernel(const typename F::raw* __restrict__ x, int64_t M, int64_t N, int64_t ld,
                                                              u64* __restrict__ rec) {
  __shared__ u64 red_cnt[4][2];
  __shared__ uint32_t red_max[4];
  const int64_t nvec = N / V, tail = N - nvec * V;
  const int64_t upr = nvec + (tail ? 1 : 0);                    // units per row
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t drow = stride / upr, dcol = stride - drow * upr;
  const int64_t first = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int64_t row = first / upr, col = first - row * upr;
  Tally t = {0u, 0u, 0u};
  while (row < M) {
    const typename F::raw* p = x + row * ld + col * V;
    if (V > 1 && col < nvec) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      tally_word<F>(v.x, t); tally_word<F>(v.y, t); tally_word<F>(v.z, t); tally_word<F>(v.w, t);
    } else {
      const int n = V > 1 ? (int)tail : 1;
      for (int j = 0; j < n; ++j) tally<F>((uint32_t)p[j], t);
    }
    row += drow; col += dcol;
    if (col >= upr) { col -= upr; ++row; }
  }
  // wave, then workgroup: counts as 64-bit sums (a lane's 32 bits hold whatever one lane can walk), the maximum as a pattern
  u64 c0 = t.limit, c1 = t.nonfinite;
  uint32_t m = t.amax;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    c0 += __shfl_xor(c0, o, 64); c1 += __shfl_xor(c1, o, 64);
    m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red_cnt[w][0] = c0; red_cnt[w][1] = c1; red_max[w] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    c0 = (red_cnt[0][0] + red_cnt[1][0]) + (red_cnt[2][0] + red_cnt[3][0]);
    c1 = (red_cnt[0][1] + red_cnt[1][1]) + (red_cnt[2][1] + red_cnt[3][1]);
    m = max(max(red_max[0], red_max[1]), max(red_max[2], red_max[3]));
    if (c0) atomicAdd(&rec[0], c0);
    if (c1) atomicAdd(&rec[1], c1);
    if (m) {
      const u64 wide = widen_bits(F(), m);
      // the record's maximum only grows while kernels run: a stale read can only send an atomic that was not needed
      if (__atomic_load_n(&rec[2], __ATOMIC_RELAXED) < wide) atomicMax(&rec[2], wide);
    }
    if (blockIdx.x == 0) atomicAdd(&rec[3], 1ull);
  }
}

template <class F>
void launch(const void* x, int64_t M, int64_t N, int64_t ld, int64_t* rec, hipStream_t s) {
  typedef typename F::raw raw;
  constexpr int V = 16 / (int)sizeof(raw);
  if (ld == N && M > 1) { N *= M; ld = N; M = 1; }              // contiguous: one long row (its tail is the only ragged end)
  const bool vec = N >= V && ((uintptr_t)x & 15u) == 0 && (M <= 1 || (ld * (int64_t)sizeof(raw)) % 16 == 0);
  const int64_t upr = vec ? N / V + (N % V ? 1 : 0) : N;
  const int64_t need = (M * upr + kThreads - 1) / kThreads;
  const int grid = (int)(need < 1 ? 1 : (need > kMaxBlocks ? kMaxBlocks : need));
  if (vec) hipLaunchKernelGGL((range_audit_kernel<F, V>), dim3(grid), dim3(kThreads), 0, s, (const raw*)x, M, N, ld, (u64*)rec);
  else hipLaunchKernelGGL((range_audit_kernel<F, 1>), dim3(grid), dim3(kThreads), 0, s, (const raw*)x, M, N, ld, (u64*)rec);
}

}  // namespace

extern "C" int hamt_range_audit(const void* x, int dtype, int M, int N, int64_t ld, int64_t* rec, void* stream) {
  HAMT_CHECK_ARG(x && rec, "hamt_range_audit: null pointer");
  HAMT_CHECK_ARG(dtype == HAMT_F16 || dtype == HAMT_BF16 || dtype == HAMT_F32, "hamt_range_audit: dtype %d is not HAMT_F16 / HAMT_BF16 / HAMT_F32", dtype);
  HAMT_CHECK_ARG(M >= 0 && N > 0 && ld >= N, "hamt_range_audit: bad shape M=%d N=%d ld=%lld (M >= 0, N > 0, ld >= N)", M, N, (long long)ld);
  const hipStream_t s = as_stream(stream);
  switch (dtype) {
    case HAMT_F16: launch<FmtF16>(x, M, N, ld, rec, s); break;
    case HAMT_BF16: launch<FmtBF16>(x, M, N, ld, rec, s); break;
    default: launch<FmtF32>(x, M, N, ld, rec, s); break;
  }
  HAMT_CHECK_LAUNCH("hamt_range_audit");
  return HAMT_OK;
}
