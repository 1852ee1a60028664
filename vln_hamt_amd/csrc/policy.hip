// The decision and loss side of ONE rollout step of the finetune agents, for all B episodes in one launch.  Three parts:
//   1. the shared row core: what every agent's step does to a row of logits -- the draw, the inverse-CDF sampler, the arg-max, log pi(a_t),
//      the entropy, the book-keeping stores, and the backward's log-probability and entropy terms.  Each exists once, here.
//   2. the R2R-family step (finetune_src/r2r/agent_cmt.py:336-401, repeated verbatim by the R2R-back and CVDN agents):
//      imitation cross-entropy on the raw logits (:339)  ->  back-track mask (:350)  ->  teacher / argmax / sample choice with its
//      log-probability and entropy (:353-366)  ->  environment action (:372-375), the chosen candidate's angle feature (:382-385),
//      `ended` (:447), the A2C mask (:418-420) and the history lengths (:399-401).
//   3. REVERIE's step (finetune_src/reverie/agent.py:253-307): the same with one more action column, STOP, made from the object logits,
//      the cross-entropy AFTER the mask, and a second cross-entropy that grounds the object.
// One wave per row, lanes strided over the <= 256 columns (4 per lane, held in registers), wave reductions only: no LDS, no atomics,
// no hand-off between rows.  Every per-row result is stored by lane 0 with ordinary (vector) stores.
#include "common.h"
#include <float.h>

namespace {

constexpr int kCols = 4;                 // columns per lane: at most 64 * kCols columns in a row
constexpr int kRowsPerBlock = 4;         // waves per 256-thread workgroup
constexpr int kNone = 0x7fffffff;        // "no slot" under wave_min_i

// ---------------------------------------------------------------------------------------------------------------- 1. the shared row core
// exp(x - ref) with exp(-inf - anything) = 0 (never -inf - -inf = NaN)
__device__ __forceinline__ float exp_rel(float x, float ref) { return x == -INFINITY ? 0.f : expf(x - ref); }

// max and sum of exp(x - max) over the row; a row of -inf gives m = -inf, s = 0
__device__ __forceinline__ void row_max_sum(const float (&x)[kCols], float& m, float& s) {
  m = wave_max(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])));
  s = 0.f;
#pragma unroll
  for (int k = 0; k < kCols; ++k) s += exp_rel(x[k], m);
  s = wave_sum(s);
}
__device__ __forceinline__ float lse_of(float m, float s) { return m == -INFINITY ? -INFINITY : m + logf(s); }

// lowest index among the columns c < n whose value equals m, the wave's maximum over them (torch.max's tie rule on one device); n <= 0: -1.
// A dead row (all -inf) has every column equal to the maximum: slot 0.  A row where nothing compares equal (all NaN): slot 0 too.
__device__ __forceinline__ int row_argmax(const float (&x)[kCols], int n, int lane, float m) {
  int first = kNone;
#pragma unroll
  for (int k = kCols - 1; k >= 0; --k)
    if (lane + 64 * k < n && x[k] == m) first = lane + 64 * k;
  first = wave_min_i(first);
  return first == kNone ? (n > 0 ? 0 : -1) : first;
}
// ... for a caller that has no maximum over exactly those columns yet
__device__ __forceinline__ int row_argmax(const float (&x)[kCols], int n, int lane) {
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < kCols; ++k)
    if (lane + 64 * k < n) m = fmaxf(m, x[k]);
  return row_argmax(x, n, lane, wave_max(m));
}

// the draw of 'sample': the injected value, or a counter hash of (seed, epoch, call_id, row) as a 24-bit uniform in [0, 1)
__device__ __forceinline__ float step_uniform(const float* __restrict__ uniform, const uint64_t* __restrict__ rng, uint32_t call_id, int b) {
  if (uniform) return uniform[b];
  const RngKey key = rng_key(rng, call_id);
  uint32_t h = hamt_mix32((uint32_t)b ^ key.k0);
  h = hamt_mix32(h + key.k1);
  return (float)(h >> 8) * (1.0f / 16777216.0f);
}

// inverse CDF over the first n columns of a row with maximum m and sum s: the first slot of non-zero probability whose inclusive
// cumulative probability exceeds u (the fp32 wave scan is not guaranteed monotone to the last bit: a slot of probability 0 is never
// taken, whatever its rounded sum says); none: the last such slot; a dead row: slot 0
__device__ __forceinline__ int sample_slot(const float (&xm)[kCols], int n, float m, float s, bool dead, float u, int lane) {
  const float inv_s = dead ? 0.f : 1.0f / s;
  float base = 0.f;
  int first = kNone, last = -1;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    if (64 * k < n) {                                       // (wave-uniform)
      const int v = lane + 64 * k;
      const float e = exp_rel(xm[k], m);
      float scan = e;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(scan, o, 64);
        if (lane >= o) scan += up;
      }
      if (e > 0.f) {
        last = v;
        if (first == kNone && (base + scan) * inv_s > u) first = v;
      }
      base += __shfl(scan, 63, 64);
    }
  }
  first = wave_min_i(first);
  last = wave_max_i(last);
  const int a = first != kNone ? first : last;
  return a < 0 ? 0 : a;
}

// a_t over the first n columns of the masked row (m, s: their maximum and sum of exp(x - m); the columns behind them hold -inf):
// forced, the teacher's target, the arg-max or a sample (:353-366)
__device__ __forceinline__ long long choose_action(int mode, const int64_t* __restrict__ forced, long long tgt, const float (&xm)[kCols], int n,
                                                   float m, float s, bool dead, const float* __restrict__ uniform,
                                                   const uint64_t* __restrict__ rng, uint32_t call_id, int b, int lane) {
  if (forced) return (long long)forced[b];
  if (mode == HAMT_POLICY_TEACHER) return tgt;
  if (mode == HAMT_POLICY_ARGMAX) return row_argmax(xm, n, lane, m);
  return sample_slot(xm, n, m, s, dead, step_uniform(uniform, rng, call_id, b), lane);
}

// log pi(a) of the masked row as the reference takes it: log_softmax(...).gather (argmax, :358-359) or Categorical(probs).log_prob
// (sample, :361-366: probabilities clamped to [eps, 1 - eps] before the log).  `live` = the gradient flows (no clamp, a real slot).
__device__ __forceinline__ float chosen_logp(int mode, float xa, float lse1, bool a_ok, bool& live) {
  live = false;
  if (mode == HAMT_POLICY_TEACHER || !a_ok || lse1 == -INFINITY) return 0.f;
  float lp = xa == -INFINITY ? -INFINITY : xa - lse1;
  live = xa != -INFINITY;
  if (mode == HAMT_POLICY_SAMPLE) {
    const float lo = logf(FLT_EPSILON), hi = logf(1.0f - FLT_EPSILON);
    if (lp < lo) { lp = lo; live = false; }
    if (lp > hi) { lp = hi; live = false; }
  }
  return lp;
}

// entropy of the masked row ('sample' only: Categorical(probs).entropy(), :364); a dead row: 0
__device__ __forceinline__ float row_entropy(const float (&xm)[kCols], float lse, bool dead) {
  float H = 0.f;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const float p = exp_rel(xm[k], lse);
    if (p > 0.f) H -= p * (xm[k] - lse);                     // 0 log 0 = 0
  }
  H = wave_sum(H);
  return dead ? 0.f : H;
}

// the step's tail: the chosen candidate's angle feature (all lanes) and the per-row results and in-place state (lane 0); env < 0 = no move
__device__ __forceinline__ void store_step(int b, int lane, int V, int A, int mode, bool was_ended, int env, float ml_b, long long a, float lp,
                                           float H, const float* __restrict__ ob_ang, float* __restrict__ prev_angle, float* __restrict__ ml,
                                           int64_t* __restrict__ action, float* __restrict__ logp, float* __restrict__ ent,
                                           float* __restrict__ mask, int32_t* __restrict__ env_action, uint8_t* ended, int32_t* hist_len) {
  if (prev_angle) {
    for (int j = lane; j < A; j += 64)
      prev_angle[(size_t)b * A + j] = (env >= 0 && ob_ang) ? ob_ang[((size_t)b * V + env) * A + j] : 0.f;
  }
  if (lane == 0) {
    ml[b] = ml_b;
    action[b] = (int64_t)a;
    logp[b] = lp;
    if (mode == HAMT_POLICY_SAMPLE && ent) ent[b] = H;
    mask[b] = was_ended ? 0.f : 1.f;
    env_action[b] = env;
    ended[b] = (was_ended || env < 0) ? 1 : 0;
    if (hist_len && !was_ended) hist_len[b] += 1;
  }
}

// The backward's policy terms of one row: d(g_logp * log pi(a) + g_ent * H) / d(masked logit).  `p[]` doubles as the softmax of the
// masked row for the caller's cross-entropy term.
struct PolicyGrad {
  float gl, ge, H, lse1, p[kCols];
  bool with_ent;
  // column k holding masked logit x (not -inf: such positions take nothing), added to d; `chosen` = this column is a_t
  __device__ __forceinline__ float add(float d, int k, float x, bool chosen) const {
    if (gl != 0.f) d += gl * ((chosen ? 1.f : 0.f) - p[k]);
    if (with_ent && p[k] > 0.f) d += ge * (-p[k] * ((x - lse1) + H));
    return d;
  }
};
__device__ __forceinline__ PolicyGrad policy_grad_row(int mode, const float (&xm)[kCols], float xa, bool a_ok, float lse1, int b,
                                                      const float* __restrict__ g_logp, const float* __restrict__ g_ent, int gs_logp,
                                                      int gs_ent) {
  PolicyGrad g;
  bool live;
  chosen_logp(mode, xa, lse1, a_ok, live);
  const bool dead = lse1 == -INFINITY;
  g.lse1 = lse1;
  g.gl = (g_logp && live && mode != HAMT_POLICY_TEACHER) ? g_logp[(size_t)b * gs_logp] : 0.f;
  g.with_ent = g_ent && mode == HAMT_POLICY_SAMPLE && !dead;
  g.ge = g.with_ent ? g_ent[(size_t)b * gs_ent] : 0.f;
  g.H = 0.f;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    g.p[k] = dead ? 0.f : exp_rel(xm[k], lse1);
    if (g.p[k] > 0.f) g.H -= g.p[k] * (xm[k] - lse1);
  }
  if (g.with_ent) g.H = wave_sum(g.H);                      // (wave-uniform condition)
  return g;
}

// ---------------------------------------------------------------------------------------------------- 2. the R2R-family step
__device__ __forceinline__ void load_row(const float* __restrict__ xr, const uint8_t* __restrict__ mr, int V, int lane,
                                         float (&x)[kCols], float (&xm)[kCols]) {
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int v = lane + 64 * k;
    x[k] = v < V ? xr[v] : -INFINITY;
    xm[k] = (mr && v < V && mr[v]) ? -INFINITY : x[k];
  }
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void policy_step_fwd_kernel(
    int B, int V, int A, int mode, long long ignoreid, const float* __restrict__ logit, int ld, const int64_t* __restrict__ target,
    const uint8_t* __restrict__ bt_mask, const int32_t* __restrict__ cand_len, uint8_t* ended, const float* __restrict__ ob_ang,
    const int64_t* __restrict__ forced, const float* __restrict__ uniform, const uint64_t* __restrict__ rng, uint32_t call_id,
    float* __restrict__ ml, int64_t* __restrict__ action, float* __restrict__ logp, float* __restrict__ ent, float* __restrict__ mask,
    int32_t* __restrict__ env_action, float* __restrict__ prev_angle, int32_t* hist_len, float* __restrict__ lse) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;                                       // (whole waves leave: nothing below synchronises a workgroup)
  const float* xr = logit + (size_t)b * ld;
  const uint8_t* mr = bt_mask ? bt_mask + (size_t)b * V : nullptr;
  float x[kCols], xm[kCols];
  load_row(xr, mr, V, lane, x, xm);

  // ---- imitation cross-entropy on the UNMASKED row (:339 precedes :350; REVERIE's follows the mask)
  float m0, s0;
  row_max_sum(x, m0, s0);
  const float lse0 = lse_of(m0, s0);
  const long long tgt = target ? (long long)target[b] : ignoreid;
  float ml_b = 0.f;
  if (tgt != ignoreid) ml_b = (tgt >= 0 && tgt < V) ? lse0 - xr[tgt] : __builtin_nanf("");    // (a target behind the row: NaN, as hamt_ce_fwd)

  // ---- the distribution the action comes from: the back-track-masked row
  float m1 = m0, s1 = s0;
  if (mr) row_max_sum(xm, m1, s1);
  const float lse1 = lse_of(m1, s1);
  const bool dead = m1 == -INFINITY;                        // every slot masked: cannot occur on the path (the STOP slot is never visited)
  const long long a = choose_action(mode, forced, tgt, xm, V, m1, s1, dead, uniform, rng, call_id, b, lane);

  // ---- log pi(a_t), entropy
  const bool a_ok = a >= 0 && a < V;
  float xa = -INFINITY;
  if (a_ok) xa = (mr && mr[a]) ? -INFINITY : xr[a];
  bool live;
  const float lp = chosen_logp(mode, xa, lse1, a_ok, live);
  const float H = mode == HAMT_POLICY_SAMPLE ? row_entropy(xm, lse1, dead) : 0.f;

  // ---- environment action (STOP is slot cand_len - 1 here; REVERIE's is column V), previous-action angle, book-keeping
  const bool was_ended = ended[b] != 0;
  const int cl = cand_len[b];
  int env = -1;
  if (a_ok && !dead && !was_ended && a != ignoreid && a != (long long)cl - 1) env = (int)a;
  store_step(b, lane, V, A, mode, was_ended, env,           // the row, the shapes, the state before the step, the move
             ml_b, a, lp, H,                                // the values, in the order of their destinations two lines down
             ob_ang, prev_angle,                            // the angle feature: from, to
             ml, action, logp, ent,                         // the destinations of the values
             mask, env_action, ended, hist_len);            // derived from was_ended and env
  if (lane == 0) {                                          // (2 floats per row; REVERIE keeps 3)
    lse[2 * b] = lse0;
    lse[2 * b + 1] = lse1;
  }
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void policy_step_bwd_kernel(
    int B, int V, int mode, long long ignoreid, const float* __restrict__ logit, int ld, const int64_t* __restrict__ target,
    const uint8_t* __restrict__ bt_mask, const int64_t* __restrict__ action, const float* __restrict__ lse, const float* __restrict__ g_ml,
    const float* __restrict__ g_logp, const float* __restrict__ g_ent, int gs_ml, int gs_logp, int gs_ent, float* __restrict__ dlogit, int ldd) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;
  const float* xr = logit + (size_t)b * ld;
  const uint8_t* mr = bt_mask ? bt_mask + (size_t)b * V : nullptr;
  float x[kCols], xm[kCols];
  load_row(xr, mr, V, lane, x, xm);
  const float lse0 = lse[2 * b], lse1 = lse[2 * b + 1];
  const long long tgt = target ? (long long)target[b] : ignoreid;
  const long long a = (long long)action[b];
  const bool a_ok = a >= 0 && a < V;
  float xa = -INFINITY;
  if (a_ok) xa = (mr && mr[a]) ? -INFINITY : xr[a];
  const PolicyGrad g = policy_grad_row(mode, xm, xa, a_ok, lse1, b, g_logp, g_ent, gs_logp, gs_ent);
  const float gm = (g_ml && tgt != ignoreid) ? g_ml[(size_t)b * gs_ml] : 0.f;
  const float bad = (tgt != ignoreid && !(tgt >= 0 && tgt < V)) ? __builtin_nanf("") : 0.f;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int v = lane + 64 * k;
    if (v < V) {
      float d = 0.f;                                        // the cross-entropy term is taken on the UNMASKED row here
      if (tgt != ignoreid) d = gm * (exp_rel(x[k], lse0) - (v == tgt ? 1.f : 0.f)) + bad;
      if (xm[k] != -INFINITY) d = g.add(d, k, xm[k], v == a);   // masked (and -inf) positions take nothing from the policy terms
      dlogit[(size_t)b * ldd + v] = d;
    }
  }
}

}  // namespace

extern "C" int hamt_policy_step_fwd(int B, int V, int A, int mode, int64_t ignoreid, const float* logit, int ld_logit,
                                    const int64_t* target, const uint8_t* bt_mask, const int32_t* cand_len, uint8_t* ended,
                                    const float* ob_ang, const int64_t* forced_action, const float* uniform, const uint64_t* rng,
                                    uint32_t call_id, float* ml, int64_t* action, float* logp, float* ent, float* mask,
                                    int32_t* env_action, float* prev_angle, int32_t* hist_len, float* lse, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && V <= 64 * kCols && A >= 0 && ld_logit >= V, "hamt_policy_step_fwd: need 0 < V <= 256, ld_logit >= V");
  HAMT_CHECK_ARG(mode == HAMT_POLICY_TEACHER || mode == HAMT_POLICY_ARGMAX || mode == HAMT_POLICY_SAMPLE, "hamt_policy_step_fwd: bad mode");
  HAMT_CHECK_ARG(logit && cand_len && ended && ml && action && logp && mask && env_action && lse, "hamt_policy_step_fwd: null pointer");
  HAMT_CHECK_ARG(mode != HAMT_POLICY_SAMPLE || ent, "hamt_policy_step_fwd: sample mode writes ent");
  HAMT_CHECK_ARG(mode != HAMT_POLICY_TEACHER || target || forced_action, "hamt_policy_step_fwd: teacher mode needs a target");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(policy_step_fwd_kernel, dim3((B + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, as_stream(stream),
                     B, V, A, mode, (long long)ignoreid, logit, ld_logit, target, bt_mask, cand_len, ended, ob_ang, forced_action, uniform,
                     rng, call_id, ml, action, logp, ent, mask, env_action, prev_angle, hist_len, lse);
  HAMT_CHECK_LAUNCH("hamt_policy_step_fwd");
  return HAMT_OK;
}

extern "C" int hamt_policy_step_bwd(int B, int V, int mode, int64_t ignoreid, const float* logit, int ld_logit, const int64_t* target,
                                    const uint8_t* bt_mask, const int64_t* action, const float* lse, const float* g_ml,
                                    const float* g_logp, const float* g_ent, int gs_ml, int gs_logp, int gs_ent, float* dlogit, int ld_dlogit,
                                    void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && V <= 64 * kCols && ld_logit >= V && ld_dlogit >= V, "hamt_policy_step_bwd: need 0 < V <= 256, ld >= V");
  HAMT_CHECK_ARG(logit && action && lse && dlogit, "hamt_policy_step_bwd: null pointer");
  HAMT_CHECK_ARG(gs_ml >= 0 && gs_logp >= 0 && gs_ent >= 0, "hamt_policy_step_bwd: negative gradient stride");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(policy_step_bwd_kernel, dim3((B + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, as_stream(stream),
                     B, V, mode, (long long)ignoreid, logit, ld_logit, target, bt_mask, action, lse, g_ml, g_logp, g_ent, gs_ml, gs_logp, gs_ent, dlogit, ld_dlogit);
  HAMT_CHECK_LAUNCH("hamt_policy_step_bwd");
  return HAMT_OK;
}

// ---------------------------------------------------------------------------------------------------- 3. REVERIE's step
// The action row has ONE more column, V = ob_img_max_len, that stands for STOP and is made from the object logits
// (finetune_src/reverie/agent.py:253-254) -- the best object's INDEX as the reference writes it, or its value (`stop_logit`); the imitation
// cross-entropy is taken AFTER the back-track mask (:269 precedes :274); a second cross-entropy grounds the object (:275); STOP is
// a_t >= V (:306), not slot cand_len - 1; a step that stops, or the rollout's last one, predicts the object (:299-304).  The V + 1 <= 256
// action columns and the O <= 256 object columns lie 4 per lane in registers, and the row core of part 1 runs on V + 1 columns.
namespace {

constexpr int kSavedInts = 3;            // per row: obj arg-max, effective ref target, effective action target (kIgnored / kBadTarget)
constexpr int kIgnored = -1, kBadTarget = -2;

// the masked action row of V + 1 columns: act_logit, then the STOP column
__device__ __forceinline__ void load_ref_row(const float* __restrict__ xr, const uint8_t* __restrict__ mr, int V, float stop, int lane,
                                             float (&xm)[kCols]) {
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int v = lane + 64 * k;
    float x = v < V ? xr[v] : (v == V ? stop : -INFINITY);
    if (mr && v < V && mr[v]) x = -INFINITY;                 // (the mask is never set on column V: agent.py:262-267 walks the candidates)
    xm[k] = x;
  }
}

__device__ __forceinline__ float ref_row_at(const float* __restrict__ xr, const uint8_t* __restrict__ mr, int V, float stop, long long c) {
  if (c == V) return stop;
  return (mr && mr[c]) ? -INFINITY : xr[c];
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void policy_ref_fwd_kernel(
    int B, int V, int O, int A, int mode, int stop_logit, int last_step, long long ignoreid, const float* __restrict__ act, int ld_act,
    const float* __restrict__ obj, int ld_obj, const int32_t* __restrict__ obj_len, const int32_t* __restrict__ cand_len,
    const int64_t* __restrict__ target, const int64_t* __restrict__ ref_target, const int32_t* __restrict__ obj_id,
    const int32_t* __restrict__ goal_obj, const uint8_t* __restrict__ bt_mask, uint8_t* ended, const float* __restrict__ ob_ang,
    const int64_t* __restrict__ forced, const float* __restrict__ uniform, const uint64_t* __restrict__ rng, uint32_t call_id,
    float* __restrict__ ml, float* __restrict__ ref, int64_t* __restrict__ action, float* __restrict__ logp, float* __restrict__ ent,
    float* __restrict__ mask, int32_t* __restrict__ env_action, float* __restrict__ prev_angle, int32_t* hist_len, int32_t* pred_obj,
    int32_t* pred_obj_id, float* __restrict__ lse, int32_t* __restrict__ saved) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;                                       // (whole waves leave: nothing below synchronises a workgroup)
  const int Vp = V + 1;
  const float* xr = act + (size_t)b * ld_act;
  const float* orow = obj + (size_t)b * ld_obj;
  const uint8_t* mr = bt_mask ? bt_mask + (size_t)b * V : nullptr;
  const bool was_ended = ended[b] != 0;
  const int cl = cand_len[b];
  const int ol = min(max(obj_len[b], 0), O);

  // ---- the object row: its log-sum-exp, its best entry (:253) and the best among the true objects (:303)
  float xo[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) xo[k] = lane + 64 * k < O ? orow[lane + 64 * k] : -INFINITY;
  float mo, so;
  row_max_sum(xo, mo, so);
  const float lse_o = lse_of(mo, so);
  const int best = row_argmax(xo, O, lane);
  const int best_true = row_argmax(xo, ol, lane);
  const float stop = stop_logit == HAMT_STOP_LOGIT_VALUE ? mo : (float)best;

  // ---- the action row of V + 1 columns, back-track-masked BEFORE the imitation cross-entropy (:269, :274; the other agents mask after it)
  float xm[kCols];
  load_ref_row(xr, mr, V, stop, lane, xm);
  float m1, s1;
  row_max_sum(xm, m1, s1);
  const float lse1 = lse_of(m1, s1);
  const bool dead = m1 == -INFINITY;                        // ('value' with an object row of -inf, and nothing else left)

  long long tgt = target ? (long long)target[b] : ignoreid;
  if (tgt != ignoreid && tgt >= (long long)cl - 1) tgt = V;  // STOP, whether written as V (the reference) or as cand_len - 1 (hamt_nav_observe)
  int tgt_s = kIgnored;
  float ml_b = 0.f;
  if (tgt != ignoreid) {
    const bool ok = tgt >= 0 && tgt <= V;                    // (a target outside the row: NaN, as hamt_ce_fwd)
    tgt_s = ok ? (int)tgt : kBadTarget;
    ml_b = ok ? lse1 - ref_row_at(xr, mr, V, stop, tgt) : __builtin_nanf("");
  }

  // ---- the object cross-entropy (:275): the goal object's slot, only where the teacher says STOP (_teacher_action, :150-160)
  long long rt = ignoreid;
  if (ref_target) {
    rt = (long long)ref_target[b];
  } else if (obj_id && goal_obj && tgt == V && !was_ended) {
    const int goal = goal_obj[b];
    int first = kNone;
#pragma unroll
    for (int k = kCols - 1; k >= 0; --k) {
      const int c = lane + 64 * k;
      if (c < ol && obj_id[(size_t)b * O + c] == goal) first = c;
    }
    first = wave_min_i(first);
    if (first != kNone) rt = first;
  }
  int rt_s = kIgnored;
  float ref_b = 0.f;
  if (rt != ignoreid) {
    const bool ok = rt >= 0 && rt < O;
    rt_s = ok ? (int)rt : kBadTarget;
    ref_b = ok ? lse_o - orow[rt] : __builtin_nanf("");
  }

  const long long a = choose_action(mode, forced, tgt, xm, Vp, m1, s1, dead, uniform, rng, call_id, b, lane);

  // ---- log pi(a_t), entropy
  const bool a_ok = a >= 0 && a < Vp;
  const float xa = a_ok ? ref_row_at(xr, mr, V, stop, a) : -INFINITY;
  bool live;
  const float lp = chosen_logp(mode, xa, lse1, a_ok, live);
  const float H = mode == HAMT_POLICY_SAMPLE ? row_entropy(xm, lse1, dead) : 0.f;

  // ---- environment action (:306-307: STOP is a_t >= V, no cand_len - 1 rule), previous-action angle, book-keeping
  int env = -1;
  if (a >= 0 && a < V && !dead && !was_ended && a != ignoreid) env = (int)a;
  store_step(b, lane, V, A, mode, was_ended, env,           // the row, the shapes, the state before the step, the move
             ml_b, a, lp, H,                                // the values, in the order of their destinations two lines down
             ob_ang, prev_angle,                            // the angle feature: from, to
             ml, action, logp, ent,                         // the destinations of the values
             mask, env_action, ended, hist_len);            // derived from was_ended and env
  if (lane == 0) {                                          // ---- what only this agent keeps: ref loss, predicted object (:299-304), 3 + 3 saved
    ref[b] = ref_b;
    if ((a >= V || last_step) && !was_ended) {              // just stopped, or stopped by the step limit; no object in view: None
      if (pred_obj) pred_obj[b] = best_true;
      if (pred_obj_id) pred_obj_id[b] = (best_true >= 0 && obj_id) ? obj_id[(size_t)b * O + best_true] : -1;
    }
    lse[3 * b] = lse1;
    lse[3 * b + 1] = lse_o;
    lse[3 * b + 2] = stop;
    saved[kSavedInts * b] = best;
    saved[kSavedInts * b + 1] = rt_s;
    saved[kSavedInts * b + 2] = tgt_s;
  }
}

__global__ __launch_bounds__(64 * kRowsPerBlock) void policy_ref_bwd_kernel(
    int B, int V, int O, int mode, int stop_logit, const float* __restrict__ act, int ld_act, const float* __restrict__ obj, int ld_obj,
    const uint8_t* __restrict__ bt_mask, const int64_t* __restrict__ action, const float* __restrict__ lse, const int32_t* __restrict__ saved,
    const float* __restrict__ g_ml, const float* __restrict__ g_ref, const float* __restrict__ g_logp, const float* __restrict__ g_ent,
    int gs_ml, int gs_ref, int gs_logp, int gs_ent, float* __restrict__ dact, int ld_dact, float* __restrict__ dobj, int ld_dobj) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;
  const int Vp = V + 1;
  const float* xr = act + (size_t)b * ld_act;
  const float* orow = obj + (size_t)b * ld_obj;
  const uint8_t* mr = bt_mask ? bt_mask + (size_t)b * V : nullptr;
  const float lse1 = lse[3 * b], lse_o = lse[3 * b + 1], stop = lse[3 * b + 2];
  const int best = saved[kSavedInts * b], rt = saved[kSavedInts * b + 1], tgt = saved[kSavedInts * b + 2];
  float xm[kCols];
  load_ref_row(xr, mr, V, stop, lane, xm);
  const long long a = (long long)action[b];
  const bool a_ok = a >= 0 && a < Vp;
  const float xa = a_ok ? ref_row_at(xr, mr, V, stop, a) : -INFINITY;
  const PolicyGrad g = policy_grad_row(mode, xm, xa, a_ok, lse1, b, g_logp, g_ent, gs_logp, gs_ent);
  const float gm = (g_ml && tgt != kIgnored) ? g_ml[(size_t)b * gs_ml] : 0.f;
  const float bad = tgt == kBadTarget ? __builtin_nanf("") : 0.f;
  float d_stop = 0.f;                                       // column V's gradient: it lies in exactly one lane
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int v = lane + 64 * k;
    if (v < Vp) {
      float d = 0.f;
      if (xm[k] != -INFINITY) {                             // masked (and -inf) positions take nothing: the cross-entropy follows the mask here
        if (tgt != kIgnored) d = gm * (g.p[k] - (v == tgt ? 1.f : 0.f)) + bad;
        d = g.add(d, k, xm[k], v == a);
      }
      if (v < V) dact[(size_t)b * ld_dact + v] = d;
      else d_stop = d;
    }
  }
  // 'value': the STOP column is the object row's maximum, its gradient lands on the arg-max; 'index': an integer, no gradient (:253)
  d_stop = stop_logit == HAMT_STOP_LOGIT_VALUE ? __shfl(d_stop, V & 63, 64) : 0.f;
  const float gr = (g_ref && rt != kIgnored) ? g_ref[(size_t)b * gs_ref] : 0.f;
  const float bad_r = rt == kBadTarget ? __builtin_nanf("") : 0.f;
#pragma unroll
  for (int k = 0; k < kCols; ++k) {
    const int c = lane + 64 * k;
    if (c < O) {
      const float x = orow[c];
      float d = 0.f;
      if (x != -INFINITY) {
        if (rt != kIgnored) d = gr * (exp_rel(x, lse_o) - (c == rt ? 1.f : 0.f)) + bad_r;
        if (c == best) d += d_stop;
      }
      dobj[(size_t)b * ld_dobj + c] = d;
    }
  }
}

}  // namespace

extern "C" int hamt_policy_ref_step_fwd(int B, int V, int O, int A, int mode, int stop_logit, int last_step, int64_t ignoreid,
                                        const float* act_logit, int ld_act, const float* obj_logit, int ld_obj, const int32_t* obj_len,
                                        const int32_t* cand_len, const int64_t* target, const int64_t* ref_target, const int32_t* obj_id,
                                        const int32_t* goal_obj, const uint8_t* bt_mask, uint8_t* ended, const float* ob_ang,
                                        const int64_t* forced_action, const float* uniform, const uint64_t* rng, uint32_t call_id,
                                        float* ml, float* ref, int64_t* action, float* logp, float* ent, float* mask, int32_t* env_action,
                                        float* prev_angle, int32_t* hist_len, int32_t* pred_obj, int32_t* pred_obj_id, float* lse,
                                        int32_t* saved, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && V + 1 <= 64 * kCols && O > 0 && O <= 64 * kCols && A >= 0 && ld_act >= V && ld_obj >= O,
                 "hamt_policy_ref_step_fwd: need 0 < V, V + 1 <= 256, 0 < O <= 256, ld_act >= V, ld_obj >= O");
  HAMT_CHECK_ARG(mode == HAMT_POLICY_TEACHER || mode == HAMT_POLICY_ARGMAX || mode == HAMT_POLICY_SAMPLE, "hamt_policy_ref_step_fwd: bad mode");
  HAMT_CHECK_ARG(stop_logit == HAMT_STOP_LOGIT_INDEX || stop_logit == HAMT_STOP_LOGIT_VALUE, "hamt_policy_ref_step_fwd: bad stop_logit");
  HAMT_CHECK_ARG(act_logit && obj_logit && obj_len && cand_len && ended && ml && ref && action && logp && mask && env_action && lse && saved,
                 "hamt_policy_ref_step_fwd: null pointer");
  HAMT_CHECK_ARG(mode != HAMT_POLICY_SAMPLE || ent, "hamt_policy_ref_step_fwd: sample mode writes ent");
  HAMT_CHECK_ARG(mode != HAMT_POLICY_TEACHER || target || forced_action, "hamt_policy_ref_step_fwd: teacher mode needs a target");
  HAMT_CHECK_ARG(!pred_obj_id || obj_id, "hamt_policy_ref_step_fwd: pred_obj_id needs obj_id");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(policy_ref_fwd_kernel, dim3((B + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, as_stream(stream),
                     B, V, O, A, mode, stop_logit, last_step, (long long)ignoreid, act_logit, ld_act, obj_logit, ld_obj, obj_len, cand_len,
                     target, ref_target, obj_id, goal_obj, bt_mask, ended, ob_ang, forced_action, uniform, rng, call_id, ml, ref, action, logp,
                     ent, mask, env_action, prev_angle, hist_len, pred_obj, pred_obj_id, lse, saved);
  HAMT_CHECK_LAUNCH("hamt_policy_ref_step_fwd");
  return HAMT_OK;
}

extern "C" int hamt_policy_ref_step_bwd(int B, int V, int O, int mode, int stop_logit, const float* act_logit, int ld_act,
                                        const float* obj_logit, int ld_obj, const uint8_t* bt_mask, const int64_t* action, const float* lse,
                                        const int32_t* saved, const float* g_ml, const float* g_ref, const float* g_logp, const float* g_ent,
                                        int gs_ml, int gs_ref, int gs_logp, int gs_ent, float* dact, int ld_dact, float* dobj, int ld_dobj,
                                        void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && V + 1 <= 64 * kCols && O > 0 && O <= 64 * kCols && ld_act >= V && ld_obj >= O && ld_dact >= V && ld_dobj >= O,
                 "hamt_policy_ref_step_bwd: need 0 < V, V + 1 <= 256, 0 < O <= 256, ld >= the row");
  HAMT_CHECK_ARG(stop_logit == HAMT_STOP_LOGIT_INDEX || stop_logit == HAMT_STOP_LOGIT_VALUE, "hamt_policy_ref_step_bwd: bad stop_logit");
  HAMT_CHECK_ARG(act_logit && obj_logit && action && lse && saved && dact && dobj, "hamt_policy_ref_step_bwd: null pointer");
  HAMT_CHECK_ARG(gs_ml >= 0 && gs_ref >= 0 && gs_logp >= 0 && gs_ent >= 0, "hamt_policy_ref_step_bwd: negative gradient stride");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(policy_ref_bwd_kernel, dim3((B + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0, as_stream(stream),
                     B, V, O, mode, stop_logit, act_logit, ld_act, obj_logit, ld_obj, bt_mask, action, lse, saved, g_ml, g_ref, g_logp, g_ent,
                     gs_ml, gs_ref, gs_logp, gs_ent, dact, ld_dact, dobj, ld_dobj);
  HAMT_CHECK_LAUNCH("hamt_policy_ref_step_bwd");
  return HAMT_OK;
}
