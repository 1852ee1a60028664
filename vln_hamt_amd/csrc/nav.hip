// What the finetune agents read from the navigation graph around one rollout step, and the evaluation metrics, on the device:
//   nav_observe  the teacher's slot (finetune_src/r2r/agent_cmt.py:199-211 over env.py::_teacher_path_action) and the back-track mask
//                (:342-349), before the policy step;
//   nav_advance  the move, the distance to the goal, the nDTW of the grown path and the shaped reward (:407-445), after it;
//   nav_eval     env.py::_eval_item (with eval_utils.py::cal_dtw / cal_cls) for N finished trajectories.
// and the same for the reference's other three agents on this model:
//   nav_goals_step / nav_goals_eval   CVDN and REVERIE: the goal is a SET of nodes, the distance the minimum over it (cvdn/agent.py:174-203,
//                                     reverie/agent.py:337-366; cvdn/env.py and reverie/env.py::_eval_item);
//   nav_back_step / nav_back_eval     R2R-Back: two legs, the first STOP records the mid-stop and switches the reward's distance to the
//                                     path's end (r2r/agent_r2rback.py:192-198, :227-276; env.py::R2RBackBatch._eval_item).
// All three read one arena of per-scan tables: dist fp64 [n, n] (all-pairs shortest distances) and nxt int32 [n, n] (next hop), scan s
// at element scan_off[s].  One wave per episode / trajectory, lanes strided over the ground-truth path (j = 64 k + lane + 1, at most
// kChunks per lane held in registers), wave shuffles only: no LDS, no hand-off between waves; the only atomics are the two anomaly
// counters.  Every per-episode result is stored by lane 0 with ordinary (vector) stores.  All arithmetic on the tables is fp64 and
// uncontracted (an fma would round differently from the reference's separate multiply and add).
#include "common.h"
#pragma clang fp contract(off)

namespace {

constexpr int kWaves = 4;                          // episodes per 256-thread workgroup
constexpr int kChunks = HAMT_NAV_MAX_GT / 64;      // ground-truth nodes per lane
constexpr int kGoalChunks = HAMT_NAV_MAX_GOALS / 64;   // goal nodes per lane
constexpr double kInf = __builtin_huge_val();
constexpr double kMargin = 3.0;                    // ERROR_MARGIN of env.py, `threshold` of cal_dtw / cal_cls

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One row of cal_dtw's matrix from the row above it, in place: row[j] = cost[j] + min(above[j], row[j-1], above[j-1]), j = 1..G,
// with row[0] = inf and above[0] = `above0` (0 for the first row, inf after it).  The dependence along j is the map
// x -> min(a_j, b_j + x), a_j = cost[j] + min(above[j], above[j-1]), b_j = cost[j]; maps of that form compose to
// (min(a2, b2 + a1), b2 + b1), so 64 of them are an inclusive wave scan of six steps, and chunk k + 1 starts from chunk k's last value.
__device__ __forceinline__ void dtw_next_row(double (&row)[kChunks], double above0, const double (&cost)[kChunks], int G, int lane) {
  double carry = kInf, left = above0;
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    if (64 * k < G) {                                       // (wave-uniform)
      const bool in = 64 * k + lane < G;
      double diag = __shfl_up(row[k], 1, 64);
      if (lane == 0) diag = left;
      left = __shfl(row[k], 63, 64);
      double a = in ? cost[k] + fmin(row[k], diag) : kInf;  // (past G: the identity map)
      double b = in ? cost[k] : 0.0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double au = __shfl_up(a, o, 64), bu = __shfl_up(b, o, 64);
        if (lane >= o) { a = fmin(a, b + au); b = b + bu; }
      }
      const double v = fmin(a, b + carry);
      carry = __shfl(v, 63, 64);
      row[k] = in ? v : kInf;
    }
  }
}

// row[G] in every lane
__device__ __forceinline__ double dtw_last(const double (&row)[kChunks], int G) {
  double v = kInf;
#pragma unroll
  for (int k = 0; k < kChunks; ++k)
    if ((G - 1) >> 6 == k) v = __shfl(row[k], (G - 1) & 63, 64);
  return v;
}

// The move of a step (make_equiv_action appends to traj only then): the new viewpoint is the chosen candidate's.  -> moved
__device__ __forceinline__ bool take_move(int act, int V, int n, const int32_t* __restrict__ cand_row, int& here) {
  if (act >= 0 && act < V) {
    const int node = cand_row[act];
    if (node >= 0 && node < n) { here = node; return true; }
  }
  return false;
}

// lane 0, after a move: the episode stands on `here`, appended to its path
__device__ __forceinline__ void store_move(int b, int here, int path_cap, int32_t* cur, int32_t* path, int32_t* path_len) {
  cur[b] = here;
  const int pl = path_len[b];
  if (pl >= 0 && pl < path_cap) { path[(size_t)b * path_cap + pl] = here; path_len[b] = pl + 1; }
}

// cal_dtw's last value for the path so far (every lane); after a move the stored row advances by the appended node `here` alone
__device__ __forceinline__ double step_dtw(const double* __restrict__ D, int n, int here, bool moved, const int32_t* __restrict__ g, int G,
                                           double* rowp, int lane) {
  double row[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int j = 64 * k + lane;
    row[k] = j < G ? rowp[j + 1] : kInf;
  }
  if (moved) {                                              // (wave-uniform) the DTW row of the appended node only
    double cost[kChunks];
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int j = 64 * k + lane;
      cost[k] = j < G ? D[(int64_t)here * n + min(max(g[j], 0), n - 1)] : 0.0;
    }
    dtw_next_row(row, rowp[0], cost, G, lane);
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      const int j = 64 * k + lane;
      if (j < G) rowp[j + 1] = row[k];
    }
  }
  return dtw_last(row, G);
}

// The shaped reward of agent_cmt.py:418-441 (agent_r2rback.py:241-265 is the same block), fp32 as the reference's arrays
__device__ __forceinline__ float shaped_reward(bool live, int act, float d, float ld, float ndtw, float ln, int32_t* anomalies) {
  float r = 0.0f;
  if (live) {                                               // (not ended before the step)
    if (act < 0) {
      r = d < 3.0f ? 2.0f + ndtw * 2.0f : -2.0f;
    } else {
      const float gain = -(d - ld);
      const float ndtw_reward = ndtw - ln;
      if (gain > 0.0f) r = 1.0f + ndtw_reward;
      else if (gain < 0.0f) r = -1.0f + ndtw_reward;
      else { r = ndtw_reward; atomicAdd(&anomalies[1], 1); }           // (the reference raises NameError here)
      if (ld <= 1.0f && d - ld > 0.0f) r -= (1.0f - ld) * 2.0f;
    }
  }
  return r;
}

// sum of dist along a node list (every lane)
__device__ __forceinline__ double walk_length(const double* __restrict__ D, int n, const int32_t* __restrict__ p, int P, int lane) {
  double len = 0.0;
  for (int j = lane; j + 1 < P; j += 64) len += D[(int64_t)p[j] * n + p[j + 1]];
  return wave_sum_d(len);
}

// 1 in every lane if a length or a node lies outside its table
__device__ __forceinline__ int bad_list(const int32_t* __restrict__ p, int P, int p_max, int n, int lane) {
  int bad = (P < 1 || P > p_max) ? 1 : 0;
  if (!bad)
    for (int j = lane; j < P; j += 64) bad |= (p[j] < 0 || p[j] >= n) ? 1 : 0;
  return __any(bad);
}

// cal_dtw's DTW of path p against ground truth g, row by row (every lane), and cal_cls's coverage: the mean over g of
// exp(-(distance to the nearest path node) / 3)
__device__ __forceinline__ void dtw_and_cover(const double* __restrict__ D, int n, const int32_t* __restrict__ p, int P,
                                              const int32_t* __restrict__ g, int G, int lane, double& dtw, double& cover) {
  int gj[kChunks];
  double row[kChunks], nearest[kChunks], cost[kChunks];
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const int j = 64 * k + lane;
    gj[k] = j < G ? g[j] : 0;
    row[k] = kInf;
    nearest[k] = kInf;
  }
  for (int r = 0; r < P; ++r) {
    const int node = p[r];
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
      if (64 * k < G) {
        cost[k] = D[(int64_t)node * n + gj[k]];
        nearest[k] = fmin(nearest[k], D[(int64_t)gj[k] * n + node]);
      }
    }
    dtw_next_row(row, r == 0 ? 0.0 : kInf, cost, G, lane);
  }
  dtw = dtw_last(row, G);
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < kChunks; ++k)
    if (64 * k + lane < G) c += exp(-nearest[k] / kMargin);
  cover = wave_sum_d(c) / (double)G;
}

// cal_cls from its coverage and the two lengths (0 / 0 = NaN for one node against one node, as the reference)
__device__ __forceinline__ double cls_score(double cover, double glen, double plen) {
  const double expected = cover * glen;
  return cover * (expected / (expected + fabs(expected - plen)));
}

// min over the goal set of dist[from, goal] (every lane); inf for an empty set
__device__ __forceinline__ double goals_min(const double* __restrict__ D, int n, int from, const int32_t* __restrict__ goals, int E, int lane) {
  double m = kInf;
  for (int e = lane; e < E; e += 64) m = fmin(m, D[(int64_t)from * n + min(max(goals[e], 0), n - 1)]);
  return wave_min_d(m);
}

__global__ __launch_bounds__(64 * kWaves) void nav_observe_kernel(
    int B, int V, int mode, int t, long long ignoreid, int g_max, int path_cap, const int32_t* __restrict__ nxt,
    const int64_t* __restrict__ scan_off, const int32_t* __restrict__ scan_n, const int32_t* __restrict__ ep_scan,
    const int32_t* __restrict__ cand_node, const int32_t* __restrict__ cand_len, const uint8_t* __restrict__ ended,
    const int32_t* __restrict__ cur, const int32_t* __restrict__ goal, const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len,
    const int32_t* __restrict__ path, const int32_t* __restrict__ path_len, int32_t* anomalies, int64_t* __restrict__ target,
    uint8_t* __restrict__ bt_mask) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;                                       // (whole waves leave: nothing below synchronises a workgroup)
  const int s = ep_scan[b], n = scan_n[s];
  const int G = min(max(gt_len[b], 1), g_max), plen = min(max(path_len[b], 0), path_cap);
  const int here = cur[b];
  const int cl = cand_len[b];
  const int nav = min(max(cl - 1, 0), V);                   // the navigable slots; slot cl - 1 is STOP
  const int32_t* cn = cand_node + (size_t)b * V;
  const int32_t* g = gt + (size_t)b * g_max;

  if (target) {
    int tv = -1;                                            // the teacher's viewpoint (env.py::_teacher_path_action); -1: none
    if (mode == HAMT_NAV_PATH_STEP) {
      tv = t < G - 1 ? g[t + 1] : here;
    } else if (mode == HAMT_NAV_PATH_INDEX) {
      int first = 0x7fffffff;                               // path.index(here)
      for (int j = lane; j < G; j += 64)
        if (g[j] == here) first = min(first, j);
      first = wave_min_i(first);
      if (first != 0x7fffffff) tv = first == G - 1 ? here : g[first + 1];
    } else {
      const int to = goal[b];
      if (here >= 0 && here < n && to >= 0 && to < n) tv = nxt[scan_off[s] + (int64_t)here * n + to];     // (nxt[x, x] = x: "just stop here")
    }
    int slot = 0x7fffffff;                                  // the first candidate that is the teacher's viewpoint (:204-207)
    if (tv >= 0)
      for (int c = lane; c < nav; c += 64)
        if (cn[c] == tv) slot = min(slot, c);
    slot = wave_min_i(slot);
    if (lane == 0) {
      long long a = ignoreid;
      if (!ended[b]) {
        if (slot != 0x7fffffff) a = slot;
        else if (tv >= 0 && tv == here) a = (long long)cl - 1;
        else atomicAdd(&anomalies[0], 1);                   // (where the reference's assert fires)
      }
      target[b] = (int64_t)a;
    }
  }
  if (bt_mask) {
    const int32_t* p = path + (size_t)b * path_cap;
    for (int c = lane; c < V; c += 64) {
      uint8_t m = 0;
      if (c < nav) {
        const int node = cn[c];
        if (node >= 0)
          for (int i = 0; i < plen; ++i) m |= p[i] == node ? 1 : 0;
      }
      bt_mask[(size_t)b * V + c] = m;
    }
  }
}

__global__ __launch_bounds__(64 * kWaves) void nav_advance_kernel(
    int B, int V, int g_max, int path_cap, const double* __restrict__ dist, const int64_t* __restrict__ scan_off,
    const int32_t* __restrict__ scan_n, const int32_t* __restrict__ ep_scan, const int32_t* __restrict__ cand_node,
    const int32_t* __restrict__ env_action, const float* __restrict__ mask_row, int32_t* cur, const int32_t* __restrict__ goal,
    const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len, int32_t* path, int32_t* path_len, double* dtw_row,
    float* last_dist, float* last_ndtw, int32_t* anomalies, float* __restrict__ reward_row) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int s = ep_scan[b], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int G = min(max(gt_len[b], 1), g_max);
  const int32_t* g = gt + (size_t)b * g_max;
  double* rowp = dtw_row + (size_t)b * (g_max + 1);
  int here = min(max(cur[b], 0), n - 1);
  const int act = env_action[b];
  const bool moved = take_move(act, V, n, cand_node + (size_t)b * V, here);
  const double dtw = step_dtw(D, n, here, moved, g, G, rowp, lane);
  if (lane != 0) return;
  const float ndtw = (float)exp(-dtw / (kMargin * (double)G));
  const float d = (float)D[(int64_t)here * n + min(max(goal[b], 0), n - 1)];
  reward_row[b] = shaped_reward(mask_row[b] != 0.0f, act, d, last_dist[b], ndtw, last_ndtw[b], anomalies);
  last_dist[b] = d;
  last_ndtw[b] = ndtw;
  if (moved) store_move(b, here, path_cap, cur, path, path_len);
}

__global__ __launch_bounds__(64 * kWaves) void nav_eval_kernel(
    int N, int p_max, int g_max, const double* __restrict__ dist, const int64_t* __restrict__ scan_off, const int32_t* __restrict__ scan_n,
    const int32_t* __restrict__ scan, const int32_t* __restrict__ path, const int32_t* __restrict__ path_len,
    const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= N) return;
  const int s = scan[i], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int P = path_len[i], G = gt_len[i];
  const int32_t* p = path + (size_t)i * p_max;
  const int32_t* g = gt + (size_t)i * g_max;
  double* o = out + (size_t)i * HAMT_NAV_EVAL_COLS;

  // ---- a length or a node outside its table: a row of NaN, nothing read
  if (bad_list(p, P, p_max, n, lane) | bad_list(g, G, g_max, n, lane)) {
    if (lane < HAMT_NAV_EVAL_COLS) o[lane] = __builtin_nan("");
    return;
  }
  const int to = g[G - 1];

  // ---- errors and lengths
  double near_d = kInf;
  for (int j = lane; j < P; j += 64) near_d = fmin(near_d, D[(int64_t)p[j] * n + to]);      // (_get_nearest's first minimum: only its distance is scored)
  near_d = wave_min_d(near_d);
  const double plen = walk_length(D, n, p, P, lane), glen = walk_length(D, n, g, G, lane);
  const double nav_error = D[(int64_t)p[P - 1] * n + to];
  const double success = nav_error < kMargin ? 1.0 : 0.0;
  double dtw, cover;
  dtw_and_cover(D, n, p, P, g, G, lane, dtw, cover);
  if (lane != 0) return;
  const double ndtw = exp(-dtw / (kMargin * (double)G));
  o[0] = nav_error;
  o[1] = near_d;
  o[2] = (double)(P - 1);
  o[3] = plen;
  o[4] = success;
  o[5] = success * glen / fmax(fmax(plen, glen), 0.01);
  o[6] = near_d < kMargin ? 1.0 : 0.0;
  o[7] = dtw;
  o[8] = ndtw;
  o[9] = success * ndtw;
  o[10] = cls_score(cover, glen, plen);
}

// ------------------------------------------------------------------------------------------------ goal sets (CVDN, REVERIE)
__global__ __launch_bounds__(64 * kWaves) void nav_goals_step_kernel(
    int B, int V, int e_max, int path_cap, const double* __restrict__ dist, const int64_t* __restrict__ scan_off,
    const int32_t* __restrict__ scan_n, const int32_t* __restrict__ ep_scan, const int32_t* __restrict__ cand_node,
    const int32_t* __restrict__ env_action, const float* __restrict__ mask_row, int32_t* cur, const int32_t* __restrict__ goals,
    const int32_t* __restrict__ goal_len, int32_t* path, int32_t* path_len, float* last_dist, float* __restrict__ reward_row) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int s = ep_scan[b], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int E = min(max(goal_len[b], 0), e_max);
  int here = min(max(cur[b], 0), n - 1);
  const int act = env_action[b];
  const bool moved = take_move(act, V, n, cand_node + (size_t)b * V, here);
  const double nearest = goals_min(D, n, here, goals + (size_t)b * e_max, E, lane);
  if (lane != 0) return;
  const float d = E > 0 ? (float)nearest : 0.0f;            // (no end_panos: cvdn/env.py:85-86)
  const float ld = last_dist[b];

  // ---- the reward (cvdn/agent.py:181-200, reverie/agent.py:344-363): constants only
  float r = 0.0f;
  if (mask_row[b] != 0.0f) {
    if (act < 0) {
      r = d == 0.0f ? 2.0f : -2.0f;
    } else {
      const float gain = -(d - ld);
      r = gain > 0.0f ? 1.0f : gain < 0.0f ? -1.0f : 0.0f;
    }
  }
  reward_row[b] = r;
  last_dist[b] = d;
  if (moved) store_move(b, here, path_cap, cur, path, path_len);
}

__global__ __launch_bounds__(64 * kWaves) void nav_goals_eval_kernel(
    int N, int p_max, int e_max, int g_max, const double* __restrict__ dist, const int64_t* __restrict__ scan_off,
    const int32_t* __restrict__ scan_n, const int32_t* __restrict__ scan, const int32_t* __restrict__ path,
    const int32_t* __restrict__ path_len, const int32_t* __restrict__ goals, const int32_t* __restrict__ goal_len,
    const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= N) return;
  const int s = scan[i], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int P = path_len[i], E = goal_len[i], G = gt ? gt_len[i] : 1;
  const int32_t* p = path + (size_t)i * p_max;
  const int32_t* ge = goals + (size_t)i * e_max;
  const int32_t* g = gt ? gt + (size_t)i * g_max : p;
  double* o = out + (size_t)i * HAMT_NAV_GOALS_EVAL_COLS;
  if (bad_list(p, P, p_max, n, lane) | bad_list(ge, E, e_max, n, lane) | bad_list(g, G, gt ? g_max : 1, n, lane)) {
    if (lane < HAMT_NAV_GOALS_EVAL_COLS) o[lane] = __builtin_nan("");
    return;
  }
  const int last = p[P - 1];

  // ---- membership: each lane holds its goals, the path goes by once
  int mine[kGoalChunks];
#pragma unroll
  for (int k = 0; k < kGoalChunks; ++k) mine[k] = 64 * k + lane < E ? ge[64 * k + lane] : -1;
  int on_path = 0, at_end = 0;
  for (int r = 0; r < P; ++r) {
    const int node = p[r];
#pragma unroll
    for (int k = 0; k < kGoalChunks; ++k) on_path |= mine[k] == node ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < kGoalChunks; ++k) at_end |= mine[k] == last ? 1 : 0;
  const double success = __any(at_end) ? 1.0 : 0.0, oracle = __any(on_path) ? 1.0 : 0.0;

  // ---- lengths: the ground-truth path's own (REVERIE), or the start's distance to the nearest goal (CVDN)
  const double plen = walk_length(D, n, p, P, lane);
  const double gtl = gt ? walk_length(D, n, g, G, lane) : goals_min(D, n, p[0], ge, E, lane);
  const double end_d = goals_min(D, n, last, ge, E, lane);
  if (lane != 0) return;
  const double longest = fmax(fmax(plen, gtl), 0.01);
  o[0] = (double)(P - 1);
  o[1] = plen;
  o[2] = success;
  o[3] = oracle;
  o[4] = success * gtl / longest;
  o[5] = gtl - end_d;
  o[6] = gtl / longest;
}

// ------------------------------------------------------------------------------------------------ return trips (R2R-Back)
__global__ __launch_bounds__(64 * kWaves) void nav_back_step_kernel(
    int B, int V, int g_max, int path_cap, int end_on_miss, const double* __restrict__ dist, const int64_t* __restrict__ scan_off,
    const int32_t* __restrict__ scan_n, const int32_t* __restrict__ ep_scan, const int32_t* __restrict__ cand_node,
    const int32_t* __restrict__ env_action, const float* __restrict__ mask_row, int32_t* cur, const int32_t* __restrict__ goal,
    const int32_t* __restrict__ midstop, const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len, int32_t* path,
    int32_t* path_len, double* dtw_row, float* last_dist, float* last_ndtw, uint8_t* first_ended, int32_t* midstop_at, uint8_t* ended,
    int32_t* anomalies, float* __restrict__ reward_row) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (b >= B) return;
  const int s = ep_scan[b], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int G = min(max(gt_len[b], 1), g_max);
  int here = min(max(cur[b], 0), n - 1);
  const int act = env_action[b];
  const bool moved = take_move(act, V, n, cand_node + (size_t)b * V, here);
  const double dtw = step_dtw(D, n, here, moved, gt + (size_t)b * g_max, G, dtw_row + (size_t)b * (g_max + 1), lane);
  if (lane != 0) return;
  const float ndtw = (float)exp(-dtw / (kMargin * (double)G));
  const float d0 = (float)D[(int64_t)here * n + min(max(midstop[b], 0), n - 1)];
  const float d1 = (float)D[(int64_t)here * n + min(max(goal[b], 0), n - 1)];
  const bool second_leg = first_ended[b] != 0, live = mask_row[b] != 0.0f;
  const float d = second_leg ? d1 : d0;                     // (agent_r2rback.py:234-237)
  reward_row[b] = shaped_reward(live, act, d, last_dist[b], ndtw, last_ndtw[b], anomalies);
  float ld = d;
  if (live && act < 0 && !second_leg) {                     // the first STOP: the mid-stop (:197-198), the distance from here on (:271-273)
    midstop_at[b] = here;
    first_ended[b] = 1;
    ld = d1;
    ended[b] = (end_on_miss && !(d < 3.0f)) ? 1 : 0;        // (:252; the policy step had set 1; :275 keeps the episode alive)
  } else if (!live) {
    first_ended[b] = 1;                                     // (:276, cpu_a_t = -1 for an ended episode)
  }
  last_dist[b] = ld;
  last_ndtw[b] = ndtw;
  if (moved) store_move(b, here, path_cap, cur, path, path_len);
}

__global__ __launch_bounds__(64 * kWaves) void nav_back_eval_kernel(
    int N, int p_max, int g_max, const double* __restrict__ dist, const int64_t* __restrict__ scan_off, const int32_t* __restrict__ scan_n,
    const int32_t* __restrict__ scan, const int32_t* __restrict__ path, const int32_t* __restrict__ path_len,
    const int32_t* __restrict__ gt, const int32_t* __restrict__ gt_len, const int32_t* __restrict__ midstop,
    const int32_t* __restrict__ gt_midstop, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= N) return;
  const int s = scan[i], n = scan_n[s];
  const double* D = dist + scan_off[s];
  const int P = path_len[i], G = gt_len[i], mid = midstop[i], gmid = gt_midstop[i];
  const int32_t* p = path + (size_t)i * p_max;
  const int32_t* g = gt + (size_t)i * g_max;
  double* o = out + (size_t)i * HAMT_NAV_BACK_EVAL_COLS;
  if (bad_list(p, P, p_max, n, lane) | bad_list(g, G, g_max, n, lane) | (mid < -1 || mid >= n || gmid < 0 || gmid >= n)) {
    if (lane < HAMT_NAV_BACK_EVAL_COLS) o[lane] = __builtin_nan("");
    return;
  }
  const double plen = walk_length(D, n, p, P, lane), glen = walk_length(D, n, g, G, lane);
  const double nav_error = D[(int64_t)p[P - 1] * n + g[G - 1]];
  const bool hit = mid >= 0 && D[(int64_t)mid * n + gmid] <= kMargin && nav_error <= kMargin;      // (<=, where _eval_item of R2R has <)
  const double success = hit ? 1.0 : 0.0;
  double dtw, cover;
  dtw_and_cover(D, n, p, P, g, G, lane, dtw, cover);
  if (lane != 0) return;
  const double ndtw = exp(-dtw / (kMargin * (double)G));
  o[0] = nav_error;
  o[1] = (double)(P - 1);
  o[2] = plen;
  o[3] = success;
  o[4] = success * glen / fmax(fmax(plen, glen), 0.01);
  o[5] = dtw;
  o[6] = ndtw;
  o[7] = success * ndtw;
  o[8] = cls_score(cover, glen, plen);
}

}  // namespace

#define NAV_CHECK_SIZE(cond, ...)                      \
  do {                                                 \
    if (!(cond)) {                                     \
      hamt_set_error(__VA_ARGS__);                     \
      return HAMT_ERR_UNSUPPORTED;                     \
    }                                                  \
  } while (0)

extern "C" int hamt_nav_observe(int B, int V, int mode, int t, int64_t ignoreid, int g_max, int path_cap, const int32_t* nxt,
                                const int64_t* scan_off, const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node,
                                const int32_t* cand_len, const uint8_t* ended, const int32_t* cur, const int32_t* goal, const int32_t* gt,
                                const int32_t* gt_len, const int32_t* path, const int32_t* path_len, int32_t* anomalies, int64_t* target,
                                uint8_t* bt_mask, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && t >= 0 && g_max > 0 && path_cap > 0, "hamt_nav_observe: need V, g_max, path_cap > 0 and t >= 0");
  HAMT_CHECK_ARG(mode == HAMT_NAV_PATH_STEP || mode == HAMT_NAV_PATH_INDEX || mode == HAMT_NAV_SHORTEST, "hamt_nav_observe: bad teacher mode");
  NAV_CHECK_SIZE(g_max <= HAMT_NAV_MAX_GT && path_cap <= HAMT_NAV_MAX_PATH, "hamt_nav_observe: g_max %d / path_cap %d above %d / %d", g_max,
                 path_cap, HAMT_NAV_MAX_GT, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(nxt && scan_off && scan_n && ep_scan && cand_node && cand_len && ended && cur && goal && gt && gt_len && path && path_len && anomalies,
                 "hamt_nav_observe: null pointer");
  if (B == 0 || (!target && !bt_mask)) return HAMT_OK;
  hipLaunchKernelGGL(nav_observe_kernel, dim3((B + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), B, V, mode, t,
                     (long long)ignoreid, g_max, path_cap, nxt, scan_off, scan_n, ep_scan, cand_node, cand_len, ended, cur, goal, gt, gt_len, path,
                     path_len, anomalies, target, bt_mask);
  HAMT_CHECK_LAUNCH("hamt_nav_observe");
  return HAMT_OK;
}

extern "C" int hamt_nav_advance(int B, int V, int g_max, int path_cap, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                                const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action, const float* mask_row,
                                int32_t* cur, const int32_t* goal, const int32_t* gt, const int32_t* gt_len, int32_t* path, int32_t* path_len,
                                double* dtw_row, float* last_dist, float* last_ndtw, int32_t* anomalies, float* reward_row, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && g_max > 0 && path_cap > 0, "hamt_nav_advance: need V, g_max, path_cap > 0");
  NAV_CHECK_SIZE(g_max <= HAMT_NAV_MAX_GT && path_cap <= HAMT_NAV_MAX_PATH, "hamt_nav_advance: g_max %d / path_cap %d above %d / %d", g_max,
                 path_cap, HAMT_NAV_MAX_GT, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && ep_scan && cand_node && env_action && mask_row && cur && goal && gt && gt_len && path && path_len &&
                     dtw_row && last_dist && last_ndtw && anomalies && reward_row, "hamt_nav_advance: null pointer");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_advance_kernel, dim3((B + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), B, V, g_max, path_cap, dist,
                     scan_off, scan_n, ep_scan, cand_node, env_action, mask_row, cur, goal, gt, gt_len, path, path_len, dtw_row, last_dist,
                     last_ndtw, anomalies, reward_row);
  HAMT_CHECK_LAUNCH("hamt_nav_advance");
  return HAMT_OK;
}

extern "C" int hamt_nav_eval(int N, int p_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                             const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* gt, const int32_t* gt_len,
                             double* out, void* stream) {
  HAMT_CHECK_ARG(N >= 0 && p_max > 0 && g_max > 0, "hamt_nav_eval: need p_max, g_max > 0");
  NAV_CHECK_SIZE(g_max <= HAMT_NAV_MAX_GT && p_max <= HAMT_NAV_MAX_PATH, "hamt_nav_eval: g_max %d / p_max %d above %d / %d", g_max, p_max,
                 HAMT_NAV_MAX_GT, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && scan && path && path_len && gt && gt_len && out, "hamt_nav_eval: null pointer");
  if (N == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_eval_kernel, dim3((N + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), N, p_max, g_max, dist, scan_off,
                     scan_n, scan, path, path_len, gt, gt_len, out);
  HAMT_CHECK_LAUNCH("hamt_nav_eval");
  return HAMT_OK;
}

extern "C" int hamt_nav_advance_goals(int B, int V, int e_max, int path_cap, const double* dist, const int64_t* scan_off,
                                      const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action,
                                      const float* mask_row, int32_t* cur, const int32_t* goals, const int32_t* goal_len, int32_t* path,
                                      int32_t* path_len, float* last_dist, float* reward_row, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && e_max > 0 && path_cap > 0, "hamt_nav_advance_goals: need V, e_max, path_cap > 0");
  NAV_CHECK_SIZE(e_max <= HAMT_NAV_MAX_GOALS && path_cap <= HAMT_NAV_MAX_PATH, "hamt_nav_advance_goals: e_max %d / path_cap %d above %d / %d",
                 e_max, path_cap, HAMT_NAV_MAX_GOALS, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && ep_scan && cand_node && env_action && mask_row && cur && goals && goal_len && path && path_len &&
                     last_dist && reward_row, "hamt_nav_advance_goals: null pointer");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_goals_step_kernel, dim3((B + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), B, V, e_max, path_cap,
                     dist, scan_off, scan_n, ep_scan, cand_node, env_action, mask_row, cur, goals, goal_len, path, path_len, last_dist,
                     reward_row);
  HAMT_CHECK_LAUNCH("hamt_nav_advance_goals");
  return HAMT_OK;
}

extern "C" int hamt_nav_advance_back(int B, int V, int g_max, int path_cap, int end_on_miss, const double* dist, const int64_t* scan_off,
                                     const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action,
                                     const float* mask_row, int32_t* cur, const int32_t* goal, const int32_t* midstop, const int32_t* gt,
                                     const int32_t* gt_len, int32_t* path, int32_t* path_len, double* dtw_row, float* last_dist,
                                     float* last_ndtw, uint8_t* first_ended, int32_t* midstop_at, uint8_t* ended, int32_t* anomalies,
                                     float* reward_row, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && V > 0 && g_max > 0 && path_cap > 0, "hamt_nav_advance_back: need V, g_max, path_cap > 0");
  NAV_CHECK_SIZE(g_max <= HAMT_NAV_MAX_GT && path_cap <= HAMT_NAV_MAX_PATH, "hamt_nav_advance_back: g_max %d / path_cap %d above %d / %d", g_max,
                 path_cap, HAMT_NAV_MAX_GT, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && ep_scan && cand_node && env_action && mask_row && cur && goal && midstop && gt && gt_len && path &&
                     path_len && dtw_row && last_dist && last_ndtw && first_ended && midstop_at && ended && anomalies && reward_row,
                 "hamt_nav_advance_back: null pointer");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_back_step_kernel, dim3((B + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), B, V, g_max, path_cap,
                     end_on_miss, dist, scan_off, scan_n, ep_scan, cand_node, env_action, mask_row, cur, goal, midstop, gt, gt_len, path, path_len,
                     dtw_row, last_dist, last_ndtw, first_ended, midstop_at, ended, anomalies, reward_row);
  HAMT_CHECK_LAUNCH("hamt_nav_advance_back");
  return HAMT_OK;
}

extern "C" int hamt_nav_eval_goals(int N, int p_max, int e_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                                   const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* goals,
                                   const int32_t* goal_len, const int32_t* gt, const int32_t* gt_len, double* out, void* stream) {
  HAMT_CHECK_ARG(N >= 0 && p_max > 0 && e_max > 0 && (!gt || g_max > 0), "hamt_nav_eval_goals: need p_max, e_max (and, with gt, g_max) > 0");
  NAV_CHECK_SIZE(e_max <= HAMT_NAV_MAX_GOALS && p_max <= HAMT_NAV_MAX_PATH && (!gt || g_max <= HAMT_NAV_MAX_PATH),
                 "hamt_nav_eval_goals: e_max %d / p_max %d / g_max %d above %d / %d / %d", e_max, p_max, g_max, HAMT_NAV_MAX_GOALS,
                 HAMT_NAV_MAX_PATH, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && scan && path && path_len && goals && goal_len && out && (!gt == !gt_len),
                 "hamt_nav_eval_goals: null pointer (gt and gt_len come together)");
  if (N == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_goals_eval_kernel, dim3((N + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), N, p_max, e_max, g_max, dist,
                     scan_off, scan_n, scan, path, path_len, goals, goal_len, gt, gt_len, out);
  HAMT_CHECK_LAUNCH("hamt_nav_eval_goals");
  return HAMT_OK;
}

extern "C" int hamt_nav_eval_back(int N, int p_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                                  const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* gt, const int32_t* gt_len,
                                  const int32_t* midstop, const int32_t* gt_midstop, double* out, void* stream) {
  HAMT_CHECK_ARG(N >= 0 && p_max > 0 && g_max > 0, "hamt_nav_eval_back: need p_max, g_max > 0");
  NAV_CHECK_SIZE(g_max <= HAMT_NAV_MAX_GT && p_max <= HAMT_NAV_MAX_PATH, "hamt_nav_eval_back: g_max %d / p_max %d above %d / %d", g_max, p_max,
                 HAMT_NAV_MAX_GT, HAMT_NAV_MAX_PATH);
  HAMT_CHECK_ARG(dist && scan_off && scan_n && scan && path && path_len && gt && gt_len && midstop && gt_midstop && out,
                 "hamt_nav_eval_back: null pointer");
  if (N == 0) return HAMT_OK;
  hipLaunchKernelGGL(nav_back_eval_kernel, dim3((N + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, as_stream(stream), N, p_max, g_max, dist, scan_off,
                     scan_n, scan, path, path_len, gt, gt_len, midstop, gt_midstop, out);
  HAMT_CHECK_LAUNCH("hamt_nav_eval_back");
  return HAMT_OK;
}
