// The loss / accuracy side of the proxy-task validation pass (pretrain_src/main_r2r.py:344-511), accumulated on the device:
//   validate_mlm / _sap / _itm   F.cross_entropy(scores, labels, reduction='sum'), (scores.max(-1)[1] == labels).sum(), labels.numel()
//   validate_mrc                 F.kl_div(log_softmax(x), t, reduction='sum'), the arg-max agreement of compute_accuracy_for_soft_targets
//   validate_sar / _sprel        F.mse_loss(scores[:, c], targets[:, c], reduction='sum') per column
// Every call ADDS into the caller's accumulators (double sums[4], int64 counts[4]) and reads nothing from the host, so a pass over a
// loader needs one device-to-host copy at its end.  The row terms are fp32, computed as loss.hip computes them; they are folded in
// fp64 by ONE workgroup in a fixed order (thread t takes rows t, t + 256, ...; lanes, then waves, are combined as a fixed tree), with
// no floating-point atomics: the totals are bit-identical from run to run.
#include "common.h"

namespace {

constexpr int kNoCol = 0x7fffffff;

// loss.hip's reductions (same order of operations: the row terms below are bit-equal to ce_fwd_kernel's / kl_fwd_kernel's)
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return v;
}

// Maximum of a row AND the lowest column that holds it (what scores.max(dim=-1)[1] returns, and policy.hip's row_argmax), in the one
// pass that row_lse spends on the maximum.  A thread walks its columns upwards and moves on a strictly larger value only, so it keeps
// the lowest of its own; the workgroup's maximum is then compared back and the lowest candidate column wins.  -inf entries count (a
// row of nothing but -inf answers column 0, as torch does); NaN entries are skipped by the maximum, as fmaxf skips them in row_lse,
// and reported through `has_nan`.  red: 4 floats, redi: 8 ints.
__device__ __forceinline__ float row_max_arg(const float* __restrict__ x, int C, float* red, int* redi, int& arg, bool& has_nan) {
  float m = -INFINITY;
  int idx = kNoCol;
  bool nan = false;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float v = x[c];
    if (v != v) nan = true;
    else if (v > m || idx == kNoCol) { m = v; idx = c; }
  }
  const float wm = wave_max(m);
  const bool wnan = __ballot(nan) != 0ull;
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[w] = wm; redi[4 + w] = wnan ? 1 : 0; }
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  has_nan = (redi[4] | redi[5] | redi[6] | redi[7]) != 0;
  const int cand = wave_min_i((idx != kNoCol && m == bm) ? idx : kNoCol);
  if ((threadIdx.x & 63) == 0) redi[w] = cand;
  __syncthreads();
  arg = min(min(redi[0], redi[1]), min(redi[2], redi[3]));
  __syncthreads();
  return bm;
}
__device__ __forceinline__ float row_lse_from_max(const float* __restrict__ x, int C, float m, float* red) {
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) s += expf(x[c] - m);
  s = block_sum(s, red);
  return m + logf(s);
}

// workspace of the row kernels: ws[r] = the row's loss term (fp32), ws[R + r] = its flags (bit 0: the row counts, bit 1: correct)
constexpr uint32_t kCounts = 1u, kCorrect = 2u;

__global__ __launch_bounds__(256) void eval_ce_rows_kernel(int R, int C, const float* __restrict__ x, int ldx, const int64_t* __restrict__ label,
                                                           float* __restrict__ ws) {
  __shared__ float red[4];
  __shared__ int redi[8];
  const int r = blockIdx.x;
  const float* xr = x + (size_t)r * ldx;
  int arg;
  bool has_nan;
  const float m = row_max_arg(xr, C, red, redi, arg, has_nan);
  const float l = row_lse_from_max(xr, C, m, red);
  if (threadIdx.x == 0) {
    // ce_fwd_kernel's rules: a negative label is an ignored row (no loss, not counted), a label >= C a corrupted one (NaN, never an
    // out-of-bounds read).  A NaN logit makes l NaN by itself; such a row is never correct, wherever torch would point its arg-max.
    const int64_t lab = label[r];
    ws[r] = lab < 0 ? 0.f : (lab < C ? l - xr[lab] : __builtin_nanf(""));
    const uint32_t f = lab < 0 ? 0u : (kCounts | ((!has_nan && lab == (int64_t)arg) ? kCorrect : 0u));
    ws[R + r] = __uint_as_float(f);
  }
}

// The reference takes the arg-max of log_softmax(x) (main_r2r.py:469-471); this one takes it of x.  x - lse is monotone in x, so the
// index is the same unless the fp32 rounding of x - lse merges the row's top two values into one, where the reference's answer is the
// lower column of the two and not the mathematical arg-max.
__global__ __launch_bounds__(256) void eval_kl_rows_kernel(int R, int C, const float* __restrict__ x, int ldx, const float* __restrict__ t, int ldt,
                                                           float* __restrict__ ws) {
  __shared__ float red[4];
  __shared__ int redi[8];
  const int r = blockIdx.x;
  const float* xr = x + (size_t)r * ldx;
  const float* tr = t + (size_t)r * ldt;
  int ax, at;
  bool nan_x, nan_t;
  const float m = row_max_arg(xr, C, red, redi, ax, nan_x);
  (void)row_max_arg(tr, C, red, redi, at, nan_t);
  const float l = row_lse_from_max(xr, C, m, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float tv = tr[c];
    s += (tv > 0.f ? tv * logf(tv) : 0.f) - tv * (xr[c] - l);  // xlogy(t,t) - t*log_softmax(x), as kl_fwd_kernel
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    ws[r] = s;
    ws[R + r] = __uint_as_float(kCounts | ((!nan_x && !nan_t && ax == at) ? kCorrect : 0u));
  }
}

// fixed-order fp64 sum over the 256 threads of the one workgroup: lanes by xor shuffles, the four waves as (0 + 1) + (2 + 3)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void eval_fold_kernel(int R, const float* __restrict__ ws, double* __restrict__ sums, int64_t* __restrict__ counts) {
  __shared__ double reds[4];
  __shared__ long long redc[4][2];
  double s = 0.0;
  long long n = 0, k = 0;
  for (int r = threadIdx.x; r < R; r += 256) {
    const uint32_t f = __float_as_uint(ws[R + r]);
    if (f & kCounts) { s += (double)ws[r]; ++n; }
    if (f & kCorrect) ++k;
  }
  s = wave_sum_f64(s);
  n = wave_sum_i64(n);
  k = wave_sum_i64(k);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { reds[w] = s; redc[w][0] = k; redc[w][1] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    sums[0] += (reds[0] + reds[1]) + (reds[2] + reds[3]);
    counts[0] += (redc[0][0] + redc[1][0]) + (redc[2][0] + redc[3][0]);
    counts[1] += (redc[0][1] + redc[1][1]) + (redc[2][1] + redc[3][1]);
  }
}

// sums[c] += sum_r (x[r,c] - t[r,c])^2, c < NC <= 4: each term d * d rounded once in fp32 (mse_fwd_kernel), summed in fp64 by one
// workgroup in the order of eval_fold_kernel
template <int NC>
__global__ __launch_bounds__(256) void eval_mse_cols_kernel(int R, const float* __restrict__ x, int ldx, const float* __restrict__ t, int ldt,
                                                            double* __restrict__ sums) {
  __shared__ double reds[4][NC];
  double s[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = 0.0;
  for (int r = threadIdx.x; r < R; r += 256) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float d = x[(size_t)r * ldx + c] - t[(size_t)r * ldt + c];
      s[c] += (double)__fmul_rn(d, d);
    }
  }
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    s[c] = wave_sum_f64(s[c]);
    if ((threadIdx.x & 63) == 0) reds[w][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < NC) {
    const int c = threadIdx.x;
    sums[c] += (reds[0][c] + reds[1][c]) + (reds[2][c] + reds[3][c]);
  }
}

}  // namespace

extern "C" int hamt_eval_ce(int R, int C, const float* x, int ldx, const int64_t* label, float* ws, double* sums, int64_t* counts,
                            void* stream) {
  if (R == 0) return HAMT_OK;
  HAMT_CHECK_ARG(R > 0 && C > 0 && ldx >= C && x && label && ws && sums && counts, "hamt_eval_ce: bad argument");
  hipLaunchKernelGGL(eval_ce_rows_kernel, dim3(R), dim3(256), 0, as_stream(stream), R, C, x, ldx, label, ws);
  HAMT_CHECK_LAUNCH("hamt_eval_ce");
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, as_stream(stream), R, ws, sums, counts);
  HAMT_CHECK_LAUNCH("hamt_eval_ce (fold)");
  return HAMT_OK;
}

extern "C" int hamt_eval_kl(int R, int C, const float* x, int ldx, const float* t, int ldt, float* ws, double* sums, int64_t* counts,
                            void* stream) {
  if (R == 0) return HAMT_OK;
  HAMT_CHECK_ARG(R > 0 && C > 0 && ldx >= C && ldt >= C && x && t && ws && sums && counts, "hamt_eval_kl: bad argument");
  hipLaunchKernelGGL(eval_kl_rows_kernel, dim3(R), dim3(256), 0, as_stream(stream), R, C, x, ldx, t, ldt, ws);
  HAMT_CHECK_LAUNCH("hamt_eval_kl");
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, as_stream(stream), R, ws, sums, counts);
  HAMT_CHECK_LAUNCH("hamt_eval_kl (fold)");
  return HAMT_OK;
}

extern "C" int hamt_eval_mse_cols(int R, int C, const float* x, int ldx, const float* t, int ldt, double* sums, void* stream) {
  if (R == 0) return HAMT_OK;
  HAMT_CHECK_ARG(R > 0 && C >= 1 && C <= 4 && ldx >= C && ldt >= C && x && t && sums, "hamt_eval_mse_cols: bad argument (1 <= C <= 4)");
  const hipStream_t s = as_stream(stream);
  switch (C) {
    case 1: hipLaunchKernelGGL(eval_mse_cols_kernel<1>, dim3(1), dim3(256), 0, s, R, x, ldx, t, ldt, sums); break;
    case 2: hipLaunchKernelGGL(eval_mse_cols_kernel<2>, dim3(1), dim3(256), 0, s, R, x, ldx, t, ldt, sums); break;
    case 3: hipLaunchKernelGGL(eval_mse_cols_kernel<3>, dim3(1), dim3(256), 0, s, R, x, ldx, t, ldt, sums); break;
    default: hipLaunchKernelGGL(eval_mse_cols_kernel<4>, dim3(1), dim3(256), 0, s, R, x, ldx, t, ldt, sums); break;
  }
  HAMT_CHECK_LAUNCH("hamt_eval_mse_cols");
  return HAMT_OK;
}
