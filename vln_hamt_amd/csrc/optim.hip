// Optimiser-side kernels over flat fp32 arenas (pure HBM streaming, 16-byte accesses):
//   hamt_sumsq       global L2 norm of the gradient arena (torch clip_grad_norm_, main_r2r.py:271-273)
//   hamt_adamw_flat  the reference's HF AdamW (optim/adamw.py:85-110) fused with the clip scaling, the
//                    bf16 shadow refresh used by the MFMA GEMMs, and optimizer.zero_grad (main_r2r.py:280)
//   hamt_optim_table torch.optim's AdamW / Adam / RMSprop / SGD, the finetune agents' optimisers (agent_cmt.py:62-77), same fusions
// Traffic per parameter: read p,g,m,v (16 B) + write p,m,v (12 B) + g zero (4 B) + bf16 shadow (2 B) = 34 B.
#include "common.h"

namespace {

// The sum of `s` over a block of 256 threads, in a fixed order: the butterfly inside each wave, then (w0 + w1) + (w2 + w3).  Every thread
// gets it; one call per kernel (one LDS buffer, no barrier behind the read).
__device__ __forceinline__ float block_sum(float s) {
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void sumsq_partial_kernel(size_t n, const float* __restrict__ g, float* __restrict__ ws) {
  float s = 0.f;
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = ((const float4*)g)[i];
    s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[n4 * 4 + threadIdx.x]; s += v * v; }
  s = block_sum(s);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(int nb, const float* __restrict__ ws, float* __restrict__ out, int accumulate) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += 256) s += ws[i];
  s = block_sum(s);
  if (threadIdx.x == 0) *out = accumulate ? *out + s : s;
}
__device__ __forceinline__ float clip_coef(const float* gnorm_sq, float max_norm) {
  if (!gnorm_sq || max_norm <= 0.f) return 1.0f;
  return fminf(1.0f, max_norm / (sqrtf(*gnorm_sq) + 1e-6f));
}
// avg * beta + w * x, the step of an exponential average, with the FMA spelled out.  As `avg * beta + w * x` the compiler fuses whichever
// product the operand order of the add offers first, and that order is canonicalised anew in every function the expression is inlined
// through: moving the sweep body into a shared function changed the rounding of v.  So the choice is made here.  FUSE_DECAY false:
// avg * beta is rounded on its own, as the references' mul_ does; true: w * x is.
template <bool FUSE_DECAY>
__device__ __forceinline__ float ema(float avg, float beta, float w, float x) {
  return FUSE_DECAY ? fmaf(avg, beta, w * x) : fmaf(w, x, avg * beta);
}
__device__ __forceinline__ void adamw_one(float& p, float& g, float& m, float& v, float coef, float lr, float step, float b1,
                                          float b2, float eps, float wd) {
  const float gg = g * coef;
  m = ema<false>(m, b1, 1.0f - b1, gg);             // exp_avg.mul_(b1).add_(grad, alpha=1-b1)           adamw.py:89
  v = ema<false>(v, b2, gg, (1.0f - b2) * gg);      // exp_avg_sq.mul_(b2).addcmul_(grad, grad, 1-b2)    adamw.py:90
  p = p - step * (m / (sqrtf(v) + eps));            // denom = sqrt(v)+eps; p.addcdiv_(m, denom, -step)  adamw.py:91-99
  if (wd > 0.f) p = p - lr * wd * p;                // decoupled decay AFTER the update                   adamw.py:109-110
}
__global__ __launch_bounds__(256) void adamw_kernel(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, bf16_t* __restrict__ p16, const float* __restrict__ hyper,
                                                    const float* __restrict__ gnorm_sq, float b1, float b2, float eps, float wd,
                                                    int zero_grad) {
  const float lr = hyper[0], step = hyper[1], coef = clip_coef(gnorm_sq, hyper[2]);
  const size_t n4 = n >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    float4 P = ((float4*)p)[i], G = ((float4*)g)[i], M = ((float4*)m)[i], V = ((float4*)v)[i];
    adamw_one(P.x, G.x, M.x, V.x, coef, lr, step, b1, b2, eps, wd);
    adamw_one(P.y, G.y, M.y, V.y, coef, lr, step, b1, b2, eps, wd);
    adamw_one(P.z, G.z, M.z, V.z, coef, lr, step, b1, b2, eps, wd);
    adamw_one(P.w, G.w, M.w, V.w, coef, lr, step, b1, b2, eps, wd);
    ((float4*)p)[i] = P; ((float4*)m)[i] = M; ((float4*)v)[i] = V;
    if (zero_grad) ((float4*)g)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (p16) ((uint2*)p16)[i] = make_uint2(pack_bf2(P.x, P.y), pack_bf2(P.z, P.w));
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const size_t i = n4 * 4 + threadIdx.x;
    float P = p[i], G = g[i], M = m[i], V = v[i];
    adamw_one(P, G, M, V, coef, lr, step, b1, b2, eps, wd);
    p[i] = P; m[i] = M; v[i] = V;
    if (zero_grad) g[i] = 0.f;
    if (p16) p16[i] = f2bf(P);
  }
}
// One launch for the whole arena: per-parameter hyper-parameters come from a device table
// (ends[i] = exclusive end offset of parameter i, hyp[i] = {lr, step_size, weight_decay, active}); parameters with
// active == 0 (grad is None this step -- the reference's `continue`, adamw.py:70-71) are left untouched.  active == 2: updated
// like 1, but the gradient slot is NOT zeroed (its producer overwrites it: the grouped weight-gradient launch stores, it does
// not accumulate) -- 30 instead of 34 bytes per parameter; hamt_sumsq_table skips inactive slots, whatever they hold.
// Offsets are multiples of 8, so a 4-element chunk never straddles two parameters.
// The blocks SWEEP the arena together: block b takes the 256 * U float4 chunks b, b + gridDim, b + 2 gridDim, ... -- at any moment the whole
// grid works inside one window of gridDim * 16 KiB of each of the five arrays (2 048 blocks: 32 MiB), U float4 of each of p, g, m, v in flight
// per thread, stores non-temporal (nothing re-reads p, m, v before the next step; the bf16 shadow is re-read by the next forward and keeps the
// default policy).  Rounds 2-4 gave every block ONE contiguous range of the arena (2 048 places spread over all 700 MB of each array, the
// hyper-parameters of its one or two parameters in registers): that form's time moved 945 -> 1 140 us from PROCESS to process (and so from
// box to box: VERDICT r4 weak 11) while a plain 1-GiB copy held 5.35 - 5.46 TB/s in every one of them -- ten thousand concurrently streamed
// regions depend on how the driver happened to back the arenas (translation reach), a narrow moving window does not: 968 - 983 us in every
// process (tools/r5_adamw2.sh; 1 024 blocks the same, 4 096 blocks 1 016 - 1 024 us).  table_sweep below is that kernel body.
//
// The segment walk of the table kernels.  A block's chunk [lo, hi) (float4 offsets inside the launch's range, which starts at float4
// `first4` of the arena and may start and end inside parameters) is cut into the segments of the parameters it touches:
//     int q = walk.seek(lo);
//     for (size_t seg = lo; seg < hi; ++q) { const size_t pend = walk.end(q, hi);  ... [seg, pend) is of parameter q ...  seg = pend; }
// A chunk may hold dozens of parameters; the last parameter owns the padding behind it.
struct SegWalk {
  const int* __restrict__ ends;
  int nparams;
  size_t first4;
  int pi;
  __device__ __forceinline__ SegWalk(const int* __restrict__ ends_, int nparams_, size_t first4_) : ends(ends_), nparams(nparams_), first4(first4_), pi(-1) {}
  // the parameter that holds the chunk's first element: the first one whose end is beyond it
  __device__ __forceinline__ int seek(size_t lo) {
    const long e0 = (long)(lo + first4) * 4;
    if (pi < 0) {   // binary search once
      int a = 0, b = nparams - 1;
      while (a < b) { const int mid = (a + b) >> 1; if ((long)ends[mid] > e0) b = mid; else a = mid + 1; }
      pi = a;
    } else {
      while (pi < nparams - 1 && (long)ends[pi] <= e0) ++pi;       // (the chunks of a block only move forward)
    }
    return pi;
  }
  __device__ __forceinline__ size_t end(int q, size_t hi) const { return q < nparams - 1 ? min(hi, ((size_t)ends[q] >> 2) - first4) : hi; }
};
// The per-element rules of the sweep: the reference's HF AdamW (adamw_one; an internal rule, not one of hamt_opt_rule) and torch.optim's
// AdamW / Adam / RMSprop (momentum 0, not centered) / SGD (momentum 0) -- what the finetune agents run (finetune_src/r2r/agent_cmt.py:62-77).
// The rule is a template parameter: a rule's unused arenas are neither loaded nor stored (34 / 34 / 26 / 18 bytes per element with the
// gradient slot zeroed), and the per-element code has no rule branch.
// HF AdamW: hyp[q] = {lr, step_size, weight_decay, active}, no aux.
// torch's:  hyp[q] = {lr, lr / (1 - b1^t), weight_decay, active}, aux[q] = {1 / sqrt(1 - b2^t), 1 - lr * wd, 0, 0}; t is the parameter's own count.
constexpr int RULE_HF_ADAMW = -1;
static_assert(HAMT_OPT_ADAMW >= 0, "RULE_HF_ADAMW must not collide with hamt_opt_rule");
template <int RULE>
__device__ __forceinline__ void optim_one(float& p, float g, float& m, float& v, float coef, const float4& h, const float4& a, float b1,
                                          float b2, float eps) {
  if constexpr (RULE == RULE_HF_ADAMW) {
    adamw_one(p, g, m, v, coef, h.x, h.y, b1, b2, eps, h.z);
    return;
  }
  constexpr bool L2 = RULE != HAMT_OPT_ADAMW;                      // (the rules with the L2 term fuse the decay product of m and v, AdamW the
  float gg = g * coef;                                             //  other one: how each kernel was first compiled, kept bit for bit -- see ema)
  if constexpr (RULE == HAMT_OPT_ADAMW) p = p * a.y;               // param.mul_(1 - lr * wd), BEFORE the update   torch/optim/adamw.py
  else gg = gg + h.z * p;                                          // grad = grad.add(param, alpha=wd)            (L2)
  if constexpr (RULE == HAMT_OPT_ADAMW || RULE == HAMT_OPT_ADAM) {
    m = ema<L2>(m, b1, 1.0f - b1, gg);                             // exp_avg.lerp_(grad, 1 - b1)
    v = ema<L2>(v, b2, gg, (1.0f - b2) * gg);                      // exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    p = p - h.y * (m / (sqrtf(v) * a.x + eps));                    // denom = sqrt(v) / sqrt(1 - b2^t) + eps; p.addcdiv_(m, denom, -lr / (1 - b1^t))
  } else if constexpr (RULE == HAMT_OPT_RMSPROP) {
    v = ema<L2>(v, b2, gg, (1.0f - b2) * gg);                      // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    p = p - h.x * (gg / (sqrtf(v) + eps));                         // p.addcdiv_(grad, sqrt(square_avg) + eps, -lr)
  } else {
    p = p - h.x * gg;                                              // p.add_(grad, alpha=-lr)
  }
}
// The sweep body of adamw_table_kernel and optim_table_kernel (see the comment above): U float4 of each arena the rule owns in flight
// per thread, p / m / v and the zeroed gradient slot stored non-temporally, the bf16 shadow at the default policy.
template <int RULE, int U>
__device__ __forceinline__ void table_sweep(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            bf16_t* __restrict__ p16, const int* __restrict__ ends, const float4* __restrict__ hyp,
                                            const float4* __restrict__ aux, int nparams, const float* __restrict__ gnorm_sq, float max_norm,
                                            float b1, float b2, float eps, int zero_grad, size_t first4) {
  constexpr bool HF = RULE == RULE_HF_ADAMW;
  constexpr bool HAS_M = HF || RULE == HAMT_OPT_ADAMW || RULE == HAMT_OPT_ADAM, HAS_V = RULE != HAMT_OPT_SGD;
  const float coef = clip_coef(gnorm_sq, max_norm);
  const size_t n4 = n >> 2;
  constexpr size_t CH = 256 * U;
  typedef float f4 __attribute__((ext_vector_type(4)));
  SegWalk walk(ends, nparams, first4);
  for (size_t lo = (size_t)blockIdx.x * CH; lo < n4; lo += (size_t)gridDim.x * CH) {
    const size_t hi = min(n4, lo + CH);
    int q = walk.seek(lo);
    for (size_t seg = lo; seg < hi; ++q) {
      const size_t pend = walk.end(q, hi);
      const float4 h = hyp[q];
      if (h.w != 0.f) {
        const float4 ax = HF ? make_float4(0.f, 0.f, 0.f, 0.f) : aux[q];
        const bool zg = zero_grad && h.w == 1.f;
        const size_t i = seg + threadIdx.x;
        f4 P[U], G[U], M[U], V[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const size_t j = i + (size_t)u * 256;
          if (j < pend) {
            P[u] = ((const f4*)p)[j]; G[u] = ((const f4*)g)[j];
            if constexpr (HAS_M) M[u] = ((const f4*)m)[j];
            if constexpr (HAS_V) V[u] = ((const f4*)v)[j];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const size_t j = i + (size_t)u * 256;
          if (j < pend) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              float pp = P[u][c], mm = HAS_M ? M[u][c] : 0.f, vv = HAS_V ? V[u][c] : 0.f;
              optim_one<RULE>(pp, G[u][c], mm, vv, coef, h, ax, b1, b2, eps);
              P[u][c] = pp;
              if constexpr (HAS_M) M[u][c] = mm;
              if constexpr (HAS_V) V[u][c] = vv;
            }
            __builtin_nontemporal_store(P[u], (f4*)p + j);
            if constexpr (HAS_M) __builtin_nontemporal_store(M[u], (f4*)m + j);
            if constexpr (HAS_V) __builtin_nontemporal_store(V[u], (f4*)v + j);
            if (zg) __builtin_nontemporal_store((f4){0.f, 0.f, 0.f, 0.f}, (f4*)g + j);
            if (p16) ((uint2*)p16)[j] = make_uint2(pack_bf2(P[u][0], P[u][1]), pack_bf2(P[u][2], P[u][3]));
          }
        }
      }
      seg = pend;
    }
  }
}
template <int U>
__global__ __launch_bounds__(256) void adamw_table_kernel(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16_t* __restrict__ p16, const int* __restrict__ ends,
                                                          const float4* __restrict__ hyp, int nparams, const float* __restrict__ gnorm_sq,
                                                          float max_norm, float b1, float b2, float eps, int zero_grad, size_t first4) {
  table_sweep<RULE_HF_ADAMW, U>(n, p, g, m, v, p16, ends, hyp, nullptr, nparams, gnorm_sq, max_norm, b1, b2, eps, zero_grad, first4);
}
template <int RULE, int U>
__global__ __launch_bounds__(256) void optim_table_kernel(size_t n, float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, bf16_t* __restrict__ p16, const int* __restrict__ ends,
                                                          const float4* __restrict__ hyp, const float4* __restrict__ aux, int nparams,
                                                          const float* __restrict__ gnorm_sq, float max_norm, float b1, float b2, float eps,
                                                          int zero_grad) {
  table_sweep<RULE, U>(n, p, g, m, v, p16, ends, hyp, aux, nparams, gnorm_sq, max_norm, b1, b2, eps, zero_grad, 0);
}
// sum(g^2) over the ACTIVE parameters of an arena range: slots of inactive parameters are not read (they may hold a stale gradient,
// see active == 2 above).  One partial per block, summed in block order by sumsq_final_kernel: deterministic.
__global__ __launch_bounds__(256) void sumsq_table_partial_kernel(size_t n, const float* __restrict__ g, const int* __restrict__ ends,
                                                                  const float4* __restrict__ hyp, int nparams, size_t first4,
                                                                  float* __restrict__ ws) {
  // (the blocks sweep the range together, 16-KiB chunks b, b + gridDim, ...: the pattern of table_sweep; a block's partial is the sum over ITS
  // chunks in order, the partials are summed in block order: a fixed partition for a given grid, deterministic)
  const size_t n4 = n >> 2;
  constexpr size_t CH = 256 * 4;
  float s = 0.f;
  SegWalk walk(ends, nparams, first4);
  for (size_t lo = (size_t)blockIdx.x * CH; lo < n4; lo += (size_t)gridDim.x * CH) {
    const size_t hi = min(n4, lo + CH);
    int q = walk.seek(lo);
    for (size_t seg = lo; seg < hi; ++q) {
      const size_t pend = walk.end(q, hi);
      const float act = hyp[q].w;
      if (act != 0.f && act != 3.f) {      // 3: accounted for by the weight-gradient tiles (hamt_wgrad_desc.ss)
        const size_t i = seg + threadIdx.x;
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + (size_t)u * 256 < pend ? ((const float4*)g)[i + (size_t)u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
      }
      seg = pend;
    }
  }
  s = block_sum(s);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
// The same sum with the ACTIVE elements spread evenly over the blocks.  When most of a range is skipped (the GEMM-weight region once the
// weight-gradient tiles carry their own sums: what is left are the few weights written twice in a pass, ~6 % of the range in a handful
// of places) the uniform element ranges above leave ~60 of 1024 blocks with all the reading: 42 us for 38 MB.  Here every block builds
// the prefix sums of the active lengths (nparams <= SS_NP_MAX entries, LDS), takes an equal share of the active float4s and maps it
// back to arena offsets.  Same determinism: a fixed partition for a given table, partials summed in block order.
constexpr int SS_NP_MAX = 2048;
__global__ __launch_bounds__(256) void sumsq_table_balanced_kernel(size_t n, const float* __restrict__ g, const int* __restrict__ ends,
                                                                   const float4* __restrict__ hyp, int nparams, size_t first4,
                                                                   float* __restrict__ ws) {
  __shared__ unsigned pref[SS_NP_MAX + 1];      // pref[i] = active float4s of parameters [0, i) inside the range
  __shared__ unsigned tsum[256];
  const size_t n4 = n >> 2, r_lo = first4, r_hi = first4 + n4;
  const int t = threadIdx.x, per = (nparams + 255) / 256;
  unsigned loc = 0;
  for (int k = 0; k < per; ++k) {
    const int pi = t * per + k;
    unsigned len = 0;
    if (pi < nparams) {
      const size_t a = pi ? (size_t)ends[pi - 1] >> 2 : 0, b = (size_t)ends[pi] >> 2;
      const size_t lo = a > r_lo ? a : r_lo, hi = b < r_hi ? b : r_hi;
      const float act = hyp[pi].w;
      if (hi > lo && act != 0.f && act != 3.f) len = (unsigned)(hi - lo);
      pref[pi + 1] = len;                       // (own length for now)
    }
    loc += len;
  }
  tsum[t] = loc;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {           // inclusive scan of the 256 thread sums
    const unsigned v = t >= o ? tsum[t - o] : 0u;
    __syncthreads();
    tsum[t] += v;
    __syncthreads();
  }
  unsigned run = t ? tsum[t - 1] : 0u;
  if (t == 0) pref[0] = 0;
  for (int k = 0; k < per; ++k) {
    const int pi = t * per + k;
    if (pi < nparams) { run += pref[pi + 1]; pref[pi + 1] = run; }
  }
  __syncthreads();
  const unsigned total = pref[nparams];
  const unsigned share = (total + gridDim.x - 1) / gridDim.x;
  const unsigned lo = min(total, blockIdx.x * share), hi = min(total, lo + share);
  float s = 0.f;
  if (hi > lo) {
    int a = 0, b = nparams - 1;                 // first parameter whose prefix end lies behind lo
    while (a < b) { const int mid = (a + b) >> 1; if (pref[mid + 1] > lo) b = mid; else a = mid + 1; }
    for (int pi = a; pi < nparams && pref[pi] < hi; ++pi) {
      if (pref[pi + 1] == pref[pi]) continue;
      const size_t pa = pi ? (size_t)ends[pi - 1] >> 2 : 0;
      const size_t base = (pa > r_lo ? pa : r_lo) - r_lo;                 // float4 offset of the parameter's first in-range element in g
      const unsigned o0 = max(lo, pref[pi]) - pref[pi], o1 = min(hi, pref[pi + 1]) - pref[pi];
      for (size_t i = base + o0 + t; i < base + o1; i += 256 * 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + (size_t)u * 256 < base + o1 ? ((const float4*)g)[i + (size_t)u * 256] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u].x * v[u].x + v[u].y * v[u].y + v[u].z * v[u].z + v[u].w * v[u].w;
      }
    }
  }
  s = block_sum(s);
  if (t == 0) ws[blockIdx.x] = s;
}
// That sum fused with the widening of a reduce-scattered bf16 gradient chunk: g[i] = float(y16[i]) for EVERY element of the
// chunk, sum of squares over the active parameters only -- one pass instead of hamt_wire_unpack_bf16 followed by hamt_sumsq_table
// (the exchange of a data-parallel step runs this once per arena range, behind the range's reduce-scatter).
__global__ __launch_bounds__(256) void unpack_sumsq_partial_kernel(size_t n, const bf16_t* __restrict__ y, float* __restrict__ g,
                                                                   const int* __restrict__ ends, const float4* __restrict__ hyp, int nparams,
                                                                   size_t first4, float* __restrict__ ws) {
  const size_t n4 = n >> 2;
  constexpr size_t CH = 256 * 4;
  float s = 0.f;
  SegWalk walk(ends, nparams, first4);
  for (size_t lo = (size_t)blockIdx.x * CH; lo < n4; lo += (size_t)gridDim.x * CH) {
    const size_t hi = min(n4, lo + CH);
    int k = walk.seek(lo);
    for (size_t seg = lo; seg < hi; ++k) {
      const size_t pend = walk.end(k, hi);
      const bool act = hyp[k].w != 0.f && hyp[k].w != 3.f;
      const size_t i = seg + threadIdx.x;
      uint2 u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) u[q] = i + (size_t)q * 256 < pend ? ((const uint2*)y)[i + (size_t)q * 256] : make_uint2(0u, 0u);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (i + (size_t)q * 256 < pend) {
          const float4 v = make_float4(__uint_as_float(u[q].x << 16), __uint_as_float(u[q].x & 0xffff0000u), __uint_as_float(u[q].y << 16), __uint_as_float(u[q].y & 0xffff0000u));
          ((float4*)g)[i + (size_t)q * 256] = v;
          if (act) s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
      }
      seg = pend;
    }
  }
  s = block_sum(s);
  if (threadIdx.x == 0) ws[blockIdx.x] = s;
}
__global__ void clip_scale_kernel(size_t n, float* __restrict__ g, const float* __restrict__ gnorm_sq, float max_norm) {
  const float coef = clip_coef(gnorm_sq, max_norm);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) g[i] *= coef;
}

}  // namespace

// blocks for a range of n floats in 16-KiB chunks (256 threads x 4 float4), 1 .. cap: beyond cap the grid sweeps the chunks together
static inline int chunk_grid(size_t n, size_t cap) {
  const size_t b = (n / 4 + 1023) / 1024;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

extern "C" int hamt_sumsq(size_t n, const float* g, float* out, int accumulate, float* ws, void* stream) {
  HAMT_CHECK_ARG(g && out && ws && ((uintptr_t)g % 16) == 0, "hamt_sumsq: bad argument (ws needs 1024 floats, g 16-byte aligned)");
  size_t b = (n / 4 + 255) / 256;
  int nb = (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
  hipStream_t s = as_stream(stream);
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, n, g, ws);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, nb, ws, out, accumulate);
  HAMT_CHECK_LAUNCH("hamt_sumsq");
  return HAMT_OK;
}
extern "C" int hamt_sumsq_table(size_t first, size_t n, const float* g, const int* ends, const float* hyp, int nparams, float* out,
                               int accumulate, float* ws, void* stream) {
  HAMT_CHECK_ARG(g && out && ws && ends && hyp && nparams > 0 && n % 4 == 0 && first % 4 == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)hyp % 16) == 0,
                 "hamt_sumsq_table: bad argument (ws needs 1024 floats, g / hyp 16-byte aligned, first and n multiples of 4)");
  hipStream_t s = as_stream(stream);
  int nb = chunk_grid(n, 1024);
  static const bool balanced = getenv("HAMT_SUMSQ_UNBALANCED") == nullptr;
  const bool sparse = (accumulate & HAMT_SUMSQ_SPARSE) != 0;
  accumulate &= 1;
  if (sparse && balanced && nparams <= SS_NP_MAX && n / 4 < ((size_t)1 << 32)) {
    nb = nb < 512 ? nb : 512;
    hipLaunchKernelGGL(sumsq_table_balanced_kernel, dim3(nb), dim3(256), 0, s, n, g, ends, (const float4*)hyp, nparams, first / 4, ws);
  } else
    hipLaunchKernelGGL(sumsq_table_partial_kernel, dim3(nb), dim3(256), 0, s, n, g, ends, (const float4*)hyp, nparams, first / 4, ws);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, nb, ws, out, accumulate);
  HAMT_CHECK_LAUNCH("hamt_sumsq_table");
  return HAMT_OK;
}
extern "C" int hamt_wire_unpack_sumsq(size_t first, size_t n, const void* y16, float* g, const int* ends, const float* hyp, int nparams,
                                     float* out, int accumulate, float* ws, void* stream) {
  HAMT_CHECK_ARG(y16 && g && out && ws && ends && hyp && nparams > 0 && n % 4 == 0 && first % 4 == 0 && ((uintptr_t)g % 16) == 0 &&
                 ((uintptr_t)y16 % 8) == 0 && ((uintptr_t)hyp % 16) == 0,
                 "hamt_wire_unpack_sumsq: bad argument (ws needs 1024 floats, g / hyp 16-byte and y16 8-byte aligned, first and n multiples of 4)");
  hipStream_t s = as_stream(stream);
  const int nb = chunk_grid(n, 1024);
  hipLaunchKernelGGL(unpack_sumsq_partial_kernel, dim3(nb), dim3(256), 0, s, n, (const bf16_t*)y16, g, ends, (const float4*)hyp, nparams, first / 4, ws);
  hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, s, nb, ws, out, accumulate);
  HAMT_CHECK_LAUNCH("hamt_wire_unpack_sumsq");
  return HAMT_OK;
}
// out (+)= sum of n floats, one block of 1024 threads, four independent 16-byte loads in flight per thread (the ~18 k tile
// slots of a step's weight gradients: 4 us instead of 15 with the 256-thread scalar loop); fixed order: deterministic
__global__ __launch_bounds__(1024) void sum_partials_kernel(size_t n, const float* __restrict__ x, float* __restrict__ out, int accumulate) {
  float s = 0.f;
  const size_t n4 = n >> 2;
  for (size_t i = threadIdx.x; i < n4; i += 4096) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = i + (size_t)u * 1024 < n4 ? ((const float4*)x)[i + (size_t)u * 1024] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 4; ++u) s += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  if (threadIdx.x < (n & 3)) s += x[n4 * 4 + threadIdx.x];
  __shared__ float red[16];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int i = 0; i < 16; ++i) t += red[i];
    *out = accumulate ? *out + t : t;
  }
}
extern "C" int hamt_sumsq_partials(size_t n, const float* partials, float* out, int accumulate, void* stream) {
  HAMT_CHECK_ARG(partials && out && n < (size_t)1 << 30 && ((uintptr_t)partials % 16) == 0, "hamt_sumsq_partials: bad argument");
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(1024), 0, as_stream(stream), n, partials, out, accumulate);
  HAMT_CHECK_LAUNCH("hamt_sumsq_partials");
  return HAMT_OK;
}
extern "C" int hamt_adamw_flat(size_t n, float* p, float* g, float* m, float* v, void* p16, const float* hyper,
                               const float* gnorm_sq, float beta1, float beta2, float eps, float weight_decay, int zero_grad,
                               void* stream) {
  HAMT_CHECK_ARG(p && g && m && v && hyper, "hamt_adamw_flat: null pointer");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                 ((uintptr_t)p16 % 8) == 0, "hamt_adamw_flat: arenas must be 16-byte aligned");
  if (n == 0) return HAMT_OK;
  size_t b = (n / 4 + 255) / 256;
  int nb = (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
  hipLaunchKernelGGL(adamw_kernel, dim3(nb), dim3(256), 0, as_stream(stream), n, p, g, m, v, (bf16_t*)p16, hyper, gnorm_sq, beta1, beta2, eps, weight_decay, zero_grad);
  HAMT_CHECK_LAUNCH("hamt_adamw_flat");
  return HAMT_OK;
}
extern "C" int hamt_adamw_table_range(size_t first, size_t n, float* p, float* g, float* m, float* v, void* p16, const int* ends, const float* hyp,
                                      int nparams, const float* gnorm_sq, float max_norm, float beta1, float beta2, float eps,
                                      int zero_grad, void* stream) {
  HAMT_CHECK_ARG(p && g && m && v && ends && hyp && nparams > 0 && n % 4 == 0 && first % 4 == 0, "hamt_adamw_table: bad argument");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                 ((uintptr_t)p16 % 8) == 0 && ((uintptr_t)hyp % 16) == 0, "hamt_adamw_table: arenas must be 16-byte aligned");
  if (n == 0) return HAMT_OK;
  const int nb = chunk_grid(n, 2048);
  hipLaunchKernelGGL((adamw_table_kernel<4>), dim3(nb), dim3(256), 0, as_stream(stream), n, p, g, m, v, (bf16_t*)p16, ends,
                     (const float4*)hyp, nparams, gnorm_sq, max_norm, beta1, beta2, eps, zero_grad, first / 4);
  HAMT_CHECK_LAUNCH("hamt_adamw_table");
  return HAMT_OK;
}
extern "C" int hamt_adamw_table(size_t n, float* p, float* g, float* m, float* v, void* p16, const int* ends, const float* hyp,
                                int nparams, const float* gnorm_sq, float max_norm, float beta1, float beta2, float eps,
                                int zero_grad, void* stream) {
  return hamt_adamw_table_range(0, n, p, g, m, v, p16, ends, hyp, nparams, gnorm_sq, max_norm, beta1, beta2, eps, zero_grad, stream);
}
extern "C" int hamt_optim_table(int rule, size_t n, float* p, float* g, float* m, float* v, void* p16, const int* ends, const float* hyp,
                                const float* aux, int nparams, const float* gnorm_sq, float max_norm, float beta1, float beta2, float eps,
                                int zero_grad, void* stream) {
  HAMT_CHECK_ARG(rule >= HAMT_OPT_ADAMW && rule <= HAMT_OPT_SGD, "hamt_optim_table: unknown rule");
  const bool has_m = rule == HAMT_OPT_ADAMW || rule == HAMT_OPT_ADAM, has_v = rule != HAMT_OPT_SGD;
  HAMT_CHECK_ARG(p && g && (m || !has_m) && (v || !has_v) && ends && hyp && aux && nparams > 0 && n % 4 == 0,
                 "hamt_optim_table: bad argument (an arena the rule needs, ends, hyp or aux is NULL, or n is no multiple of 4)");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && (!has_m || ((uintptr_t)m % 16) == 0) &&
                 (!has_v || ((uintptr_t)v % 16) == 0) && ((uintptr_t)p16 % 8) == 0 && ((uintptr_t)hyp % 16) == 0 && ((uintptr_t)aux % 16) == 0,
                 "hamt_optim_table: arenas and tables must be 16-byte aligned");
  if (n == 0) return HAMT_OK;
  const int nb = chunk_grid(n, 2048);
  hipStream_t s = as_stream(stream);
#define HAMT_OPTIM_LAUNCH(R)                                                                                                          \
  hipLaunchKernelGGL((optim_table_kernel<R, 4>), dim3(nb), dim3(256), 0, s, n, p, g, m, v, (bf16_t*)p16, ends, (const float4*)hyp,     \
                     (const float4*)aux, nparams, gnorm_sq, max_norm, beta1, beta2, eps, zero_grad)
  switch (rule) {
    case HAMT_OPT_ADAMW: HAMT_OPTIM_LAUNCH(HAMT_OPT_ADAMW); break;
    case HAMT_OPT_ADAM: HAMT_OPTIM_LAUNCH(HAMT_OPT_ADAM); break;
    case HAMT_OPT_RMSPROP: HAMT_OPTIM_LAUNCH(HAMT_OPT_RMSPROP); break;
    default: HAMT_OPTIM_LAUNCH(HAMT_OPT_SGD); break;
  }
#undef HAMT_OPTIM_LAUNCH
  HAMT_CHECK_LAUNCH("hamt_optim_table");
  return HAMT_OK;
}
extern "C" int hamt_clip_scale(size_t n, float* g, const float* gnorm_sq, float max_norm, void* stream) {
  HAMT_CHECK_ARG(g && gnorm_sq, "hamt_clip_scale: null pointer");
  if (n == 0) return HAMT_OK;
  size_t b = (n + 255) / 256;
  hipLaunchKernelGGL(clip_scale_kernel, dim3((int)(b > 4096 ? 4096 : b)), dim3(256), 0, as_stream(stream), n, g, gnorm_sq, max_norm);
  HAMT_CHECK_LAUNCH("hamt_clip_scale");
  return HAMT_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Ralamb (RAdam + a LARS-style per-tensor trust ratio, pretrain_src/optim/ralamb.py) with the Lookahead wrapper (lookahead.py), as
// three static launches over the flat arenas:
//   1. ralamb_moments_kernel: m, v of every active element (clip fused as in adamw_table_kernel; gradient slot zeroed where the table
//      says so) and, per ITEM, the two partial sums  sum(p_dec^2)  and  sum((p_dec - s*lr*u)^2)  -- the decayed weights and the
//      candidate weights whose norms make the trust ratio (ralamb.py:70-82);
//   2. ralamb_trust_kernel: per parameter, its items' partials summed in a fixed order -> {weight_norm, adam_norm, trust};
//   3. ralamb_apply_kernel: p = p_dec - (s*lr*trust)*u, recomputed from p, m, v; the Lookahead sync (create / interpolate the slow
//      weights) of this step; the bf16 shadow from the final value.
// Items: a static host-built table, each item inside one parameter and at most one 16-KiB chunk (256 threads x 4 float4), in arena
// order, each with its own partial slot.  The grid sweeps the items together (block b: items b, b + gridDim, ...), the access
// pattern of adamw_table_kernel; every partial is a block reduction of a fixed shape, so the sums (and everything after them) are
// bit-identical from launch to launch and independent of the grid size.  No float atomics.
// Traffic per element: pass 1 reads p, g, m, v and writes m, v (24 B; + 4 B where the gradient slot is zeroed), pass 3 reads p, m, v and
// writes p and the bf16 shadow (18 B; + 8 B for the slow weights on a Lookahead sync).
namespace {

constexpr int RL_U = 4;     // float4 per thread per item: items are at most 256 * RL_U float4

struct RalambCoef {
  float coef, b1, b2, omb1, omb2, eps;
};

// The reference's statements in its own operation order (torch CPU kernels): mul_ then add_(alpha) = fma, addcmul_ = self + (value*t1)*t2,
// add_(p, alpha) = fma, addcdiv_ = self + (value*t1)/t2.  Contraction off, so that nothing else is fused.
__device__ __forceinline__ void ralamb_moments(float p, float g, float& m, float& v, const RalambCoef& c, float dec, float nslr, bool rect,
                                               float& pd, float& cand) {
#pragma clang fp contract(off)
  const float gg = g * c.coef;
  m = fmaf(gg, c.omb1, m * c.b1);                   // exp_avg.mul_(b1).add_(grad, alpha=1-b1)               ralamb.py:47
  v = v * c.b2 + (c.omb2 * gg) * gg;                // exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1-b2)  ralamb.py:49
  pd = dec != 0.f ? fmaf(p, dec, p) : p;            // p.add_(p, alpha=-wd*lr), BEFORE the norms              ralamb.py:70-71
  cand = rect ? pd + (nslr * m) / (sqrtf(v) + c.eps) // radam_step = p_dec - s*lr*m/(sqrt(v)+eps)             ralamb.py:74-79
              : fmaf(m, nslr, pd);                  //             p_dec - s*lr*m  (N_sma < 5)
}
__device__ __forceinline__ float ralamb_new_p(float p, float m, float v, float eps, float dec, float c, bool rect) {
#pragma clang fp contract(off)
  const float pd = dec != 0.f ? fmaf(p, dec, p) : p;
  return rect ? pd + (c * m) / (sqrtf(v) + eps) : fmaf(m, c, pd);      // ralamb.py:92-95
}

__global__ __launch_bounds__(256) void ralamb_moments_kernel(const float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, const int* __restrict__ items, int nitems,
                                                             const float4* __restrict__ hyp, const float4* __restrict__ rl,
                                                             const float* __restrict__ gnorm_sq, float max_norm, float b1, float b2,
                                                             float omb1, float omb2, float eps, int zero_grad, float2* __restrict__ partials,
                                                             int item_first, int item_count) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const RalambCoef c{clip_coef(gnorm_sq, max_norm), b1, b2, omb1, omb2, eps};
  const int* item_param = items + nitems + 1;
  const int item_end = item_first + item_count;     // the launch's items [item_first, item_end): nothing of any other item is touched
  __shared__ float red[2][4][2];
  int par = 0;
  for (int j = item_first + blockIdx.x; j < item_end; j += gridDim.x) {
    const int q = item_param[j];
    const float4 h = hyp[q];
    if (h.w == 0.f) continue;                       // (uniform over the block: no barrier is skipped by part of it)
    const float4 r = rl[q];                         // {N_sma >= 5, Lookahead action, alpha, -wd*lr}
    const size_t lo = (size_t)items[j], hi = (size_t)items[j + 1];
    const bool zg = zero_grad && h.w == 1.f, rect = r.x != 0.f;
    const float nslr = -h.y;
    float sa = 0.f, sb = 0.f;
    f4 P[RL_U], G[RL_U], M[RL_U], V[RL_U];
#pragma unroll
    for (int u = 0; u < RL_U; ++u) {
      const size_t i = lo + threadIdx.x + (size_t)u * 256;
      if (i < hi) { P[u] = ((const f4*)p)[i]; G[u] = ((const f4*)g)[i]; M[u] = ((const f4*)m)[i]; V[u] = ((const f4*)v)[i]; }
    }
#pragma unroll
    for (int u = 0; u < RL_U; ++u) {
      const size_t i = lo + threadIdx.x + (size_t)u * 256;
      if (i < hi) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float mm = M[u][k], vv = V[u][k], pd, cand;
          ralamb_moments(P[u][k], G[u][k], mm, vv, c, r.w, nslr, rect, pd, cand);
          M[u][k] = mm; V[u][k] = vv;
          sa += pd * pd;
          sb += cand * cand;
        }
        __builtin_nontemporal_store(M[u], (f4*)m + i);
        __builtin_nontemporal_store(V[u], (f4*)v + i);
        if (zg) __builtin_nontemporal_store((f4){0.f, 0.f, 0.f, 0.f}, (f4*)g + i);
      }
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if ((threadIdx.x & 63) == 0) { red[par][threadIdx.x >> 6][0] = sa; red[par][threadIdx.x >> 6][1] = sb; }
    __syncthreads();                                // (two LDS buffers: the next item's writes cannot overtake this read)
    if (threadIdx.x == 0)
      partials[j] = make_float2((red[par][0][0] + red[par][1][0]) + (red[par][2][0] + red[par][3][0]),
                                (red[par][0][1] + red[par][1][1]) + (red[par][2][1] + red[par][3][1]));
    par ^= 1;
  }
}

// one wave per parameter: its items' partials in a fixed order (lane l: items l, l + 64, ...; then the fixed butterfly)
__global__ __launch_bounds__(256) void ralamb_trust_kernel(const int* __restrict__ items, int nitems, const float4* __restrict__ hyp, int nparams,
                                                           const float2* __restrict__ partials, float4* __restrict__ stats) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= nparams || hyp[q].w == 0.f) return;      // inactive: its last statistics stay (the reference keeps them in its state)
  const int* first = items + 2 * nitems + 1;
  float a = 0.f, b = 0.f;
  for (int j = first[q] + lane; j < first[q + 1]; j += 64) { const float2 t = partials[j]; a += t.x; b += t.y; }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    const float ws = sqrtf(a), an = sqrtf(b);
    const float wn = ws > 10.f ? 10.f : ws;         // .clamp(0, 10) (a NaN stays a NaN)   ralamb.py:82
    const float tr = (wn == 0.f || an == 0.f) ? 1.f : wn / an;                               // ralamb.py:83-86
    stats[q] = make_float4(wn, an, tr, 0.f);
  }
}

__global__ __launch_bounds__(256) void ralamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                                           bf16_t* __restrict__ p16, float* __restrict__ slow, const int* __restrict__ items,
                                                           int nitems, const float4* __restrict__ hyp, const float4* __restrict__ rl,
                                                           const float4* __restrict__ stats, float eps, int item_first, int item_count) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const int* item_param = items + nitems + 1;
  const int item_end = item_first + item_count;
  for (int j = item_first + blockIdx.x; j < item_end; j += gridDim.x) {
    const int q = item_param[j];
    const float4 h = hyp[q];
    if (h.w == 0.f) continue;
    const float4 r = rl[q];
    const size_t lo = (size_t)items[j], hi = (size_t)items[j + 1];
    const bool rect = r.x != 0.f;
    const int act = slow ? (int)r.y : 0;            // 1: create the slow weights (= the new weights), 2: slow += alpha (p - slow), p = slow
    const float cs = -(h.y * stats[q].z);           // -s*lr*trust_ratio (ralamb.py:92-95)
    f4 P[RL_U], M[RL_U], V[RL_U], S[RL_U];
#pragma unroll
    for (int u = 0; u < RL_U; ++u) {
      const size_t i = lo + threadIdx.x + (size_t)u * 256;
      if (i < hi) {
        P[u] = ((const f4*)p)[i]; M[u] = ((const f4*)m)[i]; V[u] = ((const f4*)v)[i];
        if (act == 2) S[u] = ((const f4*)slow)[i];
      }
    }
#pragma unroll
    for (int u = 0; u < RL_U; ++u) {
      const size_t i = lo + threadIdx.x + (size_t)u * 256;
      if (i < hi) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float pn = ralamb_new_p(P[u][k], M[u][k], V[u][k], eps, r.w, cs, rect);
          if (act == 2) pn = fmaf(pn - S[u][k], r.z, S[u][k]);      // slow.add_(alpha, fast - slow); fast.copy_(slow)   lookahead.py:37-39
          P[u][k] = pn;
        }
        __builtin_nontemporal_store(P[u], (f4*)p + i);
        if (act) __builtin_nontemporal_store(P[u], (f4*)slow + i);
        if (p16) ((uint2*)p16)[i] = make_uint2(pack_bf2(P[u][0], P[u][1]), pack_bf2(P[u][2], P[u][3]));
      }
    }
  }
}

}  // namespace

// The three passes as entry points of their own: a rank of a sharded optimizer (parallel.ShardedItemSync) runs passes 1 and 3 over the
// items it owns and pass 2 over all parameters, once the ranks have summed their partial slots.  The grid sweeps the launch's items
// as the whole-table launch sweeps all of them; a partial is a block reduction of a fixed shape, so an item's result does not depend
// on the range it is run in.
static inline bool ralamb_item_range_ok(int nitems, int item_first, int item_count) {
  return nitems > 0 && item_first >= 0 && item_count >= 0 && item_first <= nitems && item_count <= nitems - item_first;
}
extern "C" int hamt_ralamb_moments_items(float* p, float* g, float* m, float* v, const int* items, int nitems, int item_first,
                                         int item_count, const float* hyp, const float* rl, int nparams, float* partials,
                                         const float* gnorm_sq, float max_norm, float beta1, float beta2, float one_minus_beta1,
                                         float one_minus_beta2, float eps, int zero_grad, void* stream) {
  HAMT_CHECK_ARG(p && g && m && v && items && hyp && rl && partials && nparams > 0 && ralamb_item_range_ok(nitems, item_first, item_count),
                 "hamt_ralamb_moments_items: bad argument (a NULL arena or table, or an item range outside [0, nitems])");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                 ((uintptr_t)hyp % 16) == 0 && ((uintptr_t)rl % 16) == 0 && ((uintptr_t)partials % 8) == 0,
                 "hamt_ralamb_moments_items: arenas / tables must be 16-byte aligned (partials 8)");
  if (item_count == 0) return HAMT_OK;
  const int nb = item_count < 2048 ? item_count : 2048;     // (the grid sweeps the items together: see adamw_table_kernel)
  hipLaunchKernelGGL(ralamb_moments_kernel, dim3(nb), dim3(256), 0, as_stream(stream), p, g, m, v, items, nitems, (const float4*)hyp,
                     (const float4*)rl, gnorm_sq, max_norm, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, zero_grad,
                     (float2*)partials, item_first, item_count);
  HAMT_CHECK_LAUNCH("hamt_ralamb_moments_items");
  return HAMT_OK;
}
extern "C" int hamt_ralamb_trust(const int* items, int nitems, const float* hyp, int nparams, const float* partials, float* stats,
                                 void* stream) {
  HAMT_CHECK_ARG(items && hyp && partials && stats && nitems > 0 && nparams > 0, "hamt_ralamb_trust: bad argument");
  HAMT_CHECK_ARG(((uintptr_t)hyp % 16) == 0 && ((uintptr_t)stats % 16) == 0 && ((uintptr_t)partials % 8) == 0,
                 "hamt_ralamb_trust: tables must be 16-byte aligned (partials 8)");
  hipLaunchKernelGGL(ralamb_trust_kernel, dim3((nparams + 3) / 4), dim3(256), 0, as_stream(stream), items, nitems, (const float4*)hyp,
                     nparams, (const float2*)partials, (float4*)stats);
  HAMT_CHECK_LAUNCH("hamt_ralamb_trust");
  return HAMT_OK;
}
extern "C" int hamt_ralamb_apply_items(float* p, const float* m, const float* v, void* p16, float* slow, const int* items, int nitems,
                                       int item_first, int item_count, const float* hyp, const float* rl, int nparams,
                                       const float* stats, float eps, void* stream) {
  HAMT_CHECK_ARG(p && m && v && items && hyp && rl && stats && nparams > 0 && ralamb_item_range_ok(nitems, item_first, item_count),
                 "hamt_ralamb_apply_items: bad argument (a NULL arena or table, or an item range outside [0, nitems])");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 && ((uintptr_t)slow % 16) == 0 &&
                 ((uintptr_t)p16 % 8) == 0 && ((uintptr_t)hyp % 16) == 0 && ((uintptr_t)rl % 16) == 0 && ((uintptr_t)stats % 16) == 0,
                 "hamt_ralamb_apply_items: arenas / tables must be 16-byte aligned");
  if (item_count == 0) return HAMT_OK;
  const int nb = item_count < 2048 ? item_count : 2048;
  hipLaunchKernelGGL(ralamb_apply_kernel, dim3(nb), dim3(256), 0, as_stream(stream), p, m, v, (bf16_t*)p16, slow, items, nitems,
                     (const float4*)hyp, (const float4*)rl, (const float4*)stats, eps, item_first, item_count);
  HAMT_CHECK_LAUNCH("hamt_ralamb_apply_items");
  return HAMT_OK;
}
extern "C" int hamt_ralamb_table(float* p, float* g, float* m, float* v, void* p16, float* slow, const int* items, int nitems,
                                 const float* hyp, const float* rl, int nparams, float* partials, float* stats, const float* gnorm_sq,
                                 float max_norm, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                                 int zero_grad, void* stream) {
  HAMT_CHECK_ARG(p && g && m && v && items && hyp && rl && partials && stats && nitems > 0 && nparams > 0, "hamt_ralamb_table: bad argument");
  HAMT_CHECK_ARG(((uintptr_t)p % 16) == 0 && ((uintptr_t)g % 16) == 0 && ((uintptr_t)m % 16) == 0 && ((uintptr_t)v % 16) == 0 &&
                 ((uintptr_t)slow % 16) == 0 && ((uintptr_t)p16 % 8) == 0 && ((uintptr_t)hyp % 16) == 0 && ((uintptr_t)rl % 16) == 0 &&
                 ((uintptr_t)stats % 16) == 0 && ((uintptr_t)partials % 8) == 0,
                 "hamt_ralamb_table: arenas / tables must be 16-byte aligned (partials 8)");
  // every argument is checked above, before the first launch: the three calls cannot refuse after one of them has run
  int rc = hamt_ralamb_moments_items(p, g, m, v, items, nitems, 0, nitems, hyp, rl, nparams, partials, gnorm_sq, max_norm, beta1, beta2,
                                     one_minus_beta1, one_minus_beta2, eps, zero_grad, stream);
  if (rc == HAMT_OK) rc = hamt_ralamb_trust(items, nitems, hyp, nparams, partials, stats, stream);
  if (rc == HAMT_OK) rc = hamt_ralamb_apply_items(p, m, v, p16, slow, items, nitems, 0, nitems, hyp, rl, nparams, stats, eps, stream);
  return rc;
}
