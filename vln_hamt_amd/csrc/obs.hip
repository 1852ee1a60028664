// The observations a finetune rollout step feeds the model, gathered on the device from a viewpoint store:
//   obs_gather  what finetune_src/r2r/env.py::_get_obs (make_candidate's cached branch, :239-252) and the agent's
//               _cand_pano_feature_variable (agent_cmt.py:104-151), _candidate_variable (:153-171) and _history_variable (:173-190)
//               build on the host: candidates first, STOP, then (HAMT_OBS_PANO) the views no candidate points to, padding after them;
//   obs_turn    the view index after a move: the chosen candidate's pointId (make_equiv_action, :213-246);
//   obj_gather  REVERIE's candidate objects of the viewpoint stood on (finetune_src/reverie/env.py:181-215 and the agent's
//               _object_variable, reverie/agent.py:125-139), from a CSR object store over the same arena rows: features, the angle
//               feature of the view each object was seen in, normalised boxes, mask, true count and ids, zeros and -1 in the padding.
// With discretised viewing angles an observation is a pure function of (scan, viewpoint, view index): the store holds every viewpoint of
// every scan in the arena order of the navigation graphs, row = vp_base[scan] + local node.  A pure gather: no arithmetic on a feature
// value, so every output is exact.  One wave per output row; each wave builds its episode's slot-to-source map itself (the 36-bit mask of
// candidate views by an OR over lanes, the rank of a free view by a population count) and copies the row with 16 bytes per lane when
// F % 4 == 0 and the bases are aligned, element by element otherwise (and for the A-wide angle rows).  Wave shuffles only: no LDS, no
// hand-off between waves; the only atomic is the anomaly counter.  Offsets into feat are 64-bit.
#include "row_copy.h"          // wave_or_u, copy_row, aligned16

namespace {

constexpr int kWaves = 4;                          // rows per 256-thread workgroup
constexpr int kViews = 36;
constexpr int kHeadings = 12;
constexpr int kMaxRowBlocks = 64;                  // row blocks per episode; more rows than 64 * kWaves are strided over

__global__ __launch_bounds__(64 * kWaves) void obs_gather_kernel(
    int B, int W, int F, int A, int C, int layout, int vec, const float* __restrict__ feat, const float* __restrict__ ang36,
    const int32_t* __restrict__ cand_cnt, const int32_t* __restrict__ cand_point, const int32_t* __restrict__ cand_node,
    const float* __restrict__ cand_ang, const int64_t* __restrict__ vp_base, const int32_t* __restrict__ scan_n,
    const int32_t* __restrict__ ep_scan, const int32_t* __restrict__ cur, const int32_t* __restrict__ view, float* __restrict__ ob_img,
    float* __restrict__ ob_ang, int64_t* __restrict__ ob_nav, uint8_t* __restrict__ ob_mask, int32_t* __restrict__ ob_len,
    int32_t* __restrict__ cand_len, int32_t* __restrict__ cand_node_out, int32_t* __restrict__ cand_point_out, float* __restrict__ hist_img,
    float* __restrict__ hist_pano_img, float* __restrict__ hist_pano_ang, int32_t* anomalies) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x;
  const int rows = W + ((hist_img || hist_pano_img || hist_pano_ang) ? 1 + kViews : 0);

  // ---- the episode's slot-to-source map (every wave, in registers)
  const int s = ep_scan[b], here = cur[b], vw = view[b];
  const bool ok = here >= 0 && here < scan_n[s] && vw >= 0 && vw < kViews;
  const int64_t row = ok ? vp_base[s] + (int64_t)here : 0;
  const int n = ok ? min(max(cand_cnt[row], 0), min(C, W - 1)) : 0;                  // navigable candidates; slot n is STOP
  const int pt = lane < n ? min(max(cand_point[row * C + lane], 0), kViews - 1) : -1;  // candidate `lane`'s view
  const uint32_t lo = wave_or_u(pt >= 0 && pt < 32 ? 1u << pt : 0u), hi = wave_or_u(pt >= 32 ? 1u << (pt - 32) : 0u);
  const uint64_t taken = ((uint64_t)hi << 32) | lo;                                  // (two candidates may share a view: one bit)
  const uint64_t free_views = (ok && layout == HAMT_OBS_PANO) ? ~taken & ((1ull << kViews) - 1) : 0ull;
  const int len = min(n + 1 + __popcll(free_views), W);
  const bool is_free = lane < kViews && ((free_views >> lane) & 1ull);
  const int rank = __popcll(free_views & ((1ull << lane) - 1ull));                    // free views below view `lane`
  const float* frow = feat + row * (int64_t)kViews * F;                               // feat[row]

  for (int r = blockIdx.y * kWaves + (threadIdx.x >> 6); r < rows; r += gridDim.y * kWaves) {      // (r is wave-uniform)
    if (r < W) {
      const int64_t o = (int64_t)b * W + r;
      const float *img = nullptr, *ang = nullptr;
      int nav = 0, node = -1, point = -1;
      if (r < n) {                                                                   // a candidate, in table order
        point = __shfl(pt, r, 64);
        node = cand_node[row * C + r];
        img = frow + (int64_t)point * F;
        ang = cand_ang + ((row * C + r) * kHeadings + vw % kHeadings) * A;
        nav = 1;
      } else if (r == n) {                                                           // STOP: zeros
        nav = 2;
      } else if (r < len) {                                                          // the (r - n - 1)-th view no candidate points to
        const int v = max(__ffsll((unsigned long long)__ballot(is_free && rank == r - n - 1)) - 1, 0);
        img = frow + (int64_t)v * F;
        ang = ang36 + ((int64_t)vw * kViews + v) * A;
      }
      copy_row(ob_img + o * F, img, F, vec != 0, lane);
      copy_row(ob_ang + o * A, ang, A, false, lane);
      if (lane == 0) {
        ob_nav[o] = nav;
        ob_mask[o] = r < len ? 1 : 0;
        cand_node_out[o] = node;
        cand_point_out[o] = point;
        if (r == 0) {
          ob_len[b] = len;
          cand_len[b] = n + 1;
          if (!ok) atomicAdd(&anomalies[0], 1);
        }
      }
    } else if (r == W) {                                                             // the view looked at (_history_variable)
      if (hist_img) copy_row(hist_img + (int64_t)b * F, ok ? frow + (int64_t)vw * F : nullptr, F, vec != 0, lane);
    } else {                                                                         // the whole panorama, relative to that view
      const int v = r - W - 1;
      const int64_t o = (int64_t)b * kViews + v;
      if (hist_pano_img) copy_row(hist_pano_img + o * F, ok ? frow + (int64_t)v * F : nullptr, F, vec != 0, lane);
      if (hist_pano_ang) copy_row(hist_pano_ang + o * A, ok ? ang36 + ((int64_t)vw * kViews + v) * A : nullptr, A, false, lane);
    }
  }
}

__global__ __launch_bounds__(256) void obs_turn_kernel(int B, int W, const int32_t* __restrict__ cand_point_out,
                                                       const int32_t* __restrict__ env_action, int32_t* __restrict__ view,
                                                       int32_t* __restrict__ view_log_row) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const int a = env_action[b];
  int v = view[b];
  if (a >= 0 && a < W) {
    const int p = cand_point_out[(int64_t)b * W + a];
    if (p >= 0 && p < kViews) v = p;                        // (a padding slot: no move, the view stays)
  }
  view[b] = v;
  if (view_log_row) view_log_row[b] = v;
}

// One wave per output row (b, k): object k of the viewpoint episode b stands on, or a padding row.
__global__ __launch_bounds__(64 * kWaves) void obj_gather_kernel(
    int B, int Ow, int Fo, int A, int S, int64_t NV, int64_t NObj, int vec, const int64_t* __restrict__ obj_off,
    const float* __restrict__ obj_feat, const int32_t* __restrict__ obj_view, const float* __restrict__ obj_pos,
    const int32_t* __restrict__ obj_id, const float* __restrict__ ang36, const int64_t* __restrict__ vp_base,
    const int32_t* __restrict__ scan_n, const int32_t* __restrict__ ep_scan, const int32_t* __restrict__ cur,
    const int32_t* __restrict__ view, float* __restrict__ obj_feats, float* __restrict__ obj_angles, float* __restrict__ obj_poses,
    uint8_t* __restrict__ obj_masks, int32_t* __restrict__ obj_lens, int32_t* __restrict__ obj_ids, int32_t* anomalies) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x;

  // ---- the episode's slice of the store (every wave, in registers)
  const int s = ep_scan[b], here = cur[b], vw = view[b];
  bool ok = s >= 0 && s < S && vw >= 0 && vw < kViews;
  ok = ok && here >= 0 && here < scan_n[s];
  const int64_t row = ok ? vp_base[s] + (int64_t)here : 0;
  ok = ok && row >= 0 && row < NV;
  const int64_t first = ok ? obj_off[row] : 0, last = ok ? obj_off[row + 1] : 0;
  ok = ok && first >= 0 && first <= last && last <= NObj;                            // (a store that contradicts itself: an anomaly too)
  const int n = ok ? (int)min(last - first, (int64_t)Ow) : 0;                        // the true count
  const int live = max(n, 1);                                                        // (_object_variable: an empty viewpoint keeps one zero slot)

  for (int k = blockIdx.y * kWaves + (threadIdx.x >> 6); k < Ow; k += gridDim.y * kWaves) {      // (k is wave-uniform)
    const int64_t o = (int64_t)b * Ow + k, src = first + k;
    const float *fts = nullptr, *ang = nullptr, *pos = nullptr;
    int id = -1;
    if (k < n) {
      fts = obj_feat + src * Fo;
      ang = ang36 + ((int64_t)vw * kViews + min(max(obj_view[src], 0), kViews - 1)) * A;
      pos = obj_pos + src * 5;
      id = obj_id[src];
    }
    copy_row(obj_feats + o * Fo, fts, Fo, vec != 0, lane);
    copy_row(obj_angles + o * A, ang, A, false, lane);
    copy_row(obj_poses + o * 5, pos, 5, false, lane);
    if (lane == 0) {
      obj_masks[o] = k < live ? 1 : 0;
      obj_ids[o] = id;
      if (k == 0) {
        obj_lens[b] = n;
        if (!ok) atomicAdd(&anomalies[0], 1);
      }
    }
  }
}

}  // namespace

extern "C" int hamt_obj_gather(int B, int Ow, int Fo, int A, int S, int64_t NV, int64_t NObj, const int64_t* obj_off, const float* obj_feat,
                               const int32_t* obj_view, const float* obj_pos, const int32_t* obj_id, const float* ang36,
                               const int64_t* vp_base, const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cur,
                               const int32_t* view, float* obj_feats, float* obj_angles, float* obj_poses, uint8_t* obj_masks,
                               int32_t* obj_lens, int32_t* obj_ids, int32_t* anomalies, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && Ow > 0 && Fo > 0 && A > 0 && S > 0 && NV >= 0 && NObj >= 0, "hamt_obj_gather: need Ow, Fo, A, S > 0");
  if (Ow > HAMT_OBJ_MAX_WIDTH) {
    hamt_set_error("hamt_obj_gather: Ow %d above %d", Ow, HAMT_OBJ_MAX_WIDTH);
    return HAMT_ERR_UNSUPPORTED;
  }
  HAMT_CHECK_ARG(obj_off && (obj_feat || NObj == 0) && (obj_view || NObj == 0) && (obj_pos || NObj == 0) && (obj_id || NObj == 0) && ang36 &&
                     vp_base && scan_n && ep_scan && cur && view && obj_feats && obj_angles && obj_poses && obj_masks && obj_lens && obj_ids &&
                     anomalies,
                 "hamt_obj_gather: null pointer");
  if (B == 0) return HAMT_OK;
  const int row_blocks = (Ow + kWaves - 1) / kWaves;
  const int vec = Fo % 4 == 0 && aligned16(obj_feat) && aligned16(obj_feats);
  hipLaunchKernelGGL(obj_gather_kernel, dim3(B, row_blocks < kMaxRowBlocks ? row_blocks : kMaxRowBlocks), dim3(64 * kWaves), 0,
                     as_stream(stream), B, Ow, Fo, A, S, NV, NObj, vec, obj_off, obj_feat, obj_view, obj_pos, obj_id, ang36, vp_base, scan_n,
                     ep_scan, cur, view, obj_feats, obj_angles, obj_poses, obj_masks, obj_lens, obj_ids, anomalies);
  HAMT_CHECK_LAUNCH("hamt_obj_gather");
  return HAMT_OK;
}

extern "C" int hamt_obs_gather(int B, int W, int F, int A, int C, int layout, const float* feat, const float* ang36, const int32_t* cand_cnt,
                               const int32_t* cand_point, const int32_t* cand_node, const float* cand_ang, const int64_t* vp_base,
                               const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cur, const int32_t* view, float* ob_img,
                               float* ob_ang, int64_t* ob_nav, uint8_t* ob_mask, int32_t* ob_len, int32_t* cand_len, int32_t* cand_node_out,
                               int32_t* cand_point_out, float* hist_img, float* hist_pano_img, float* hist_pano_ang, int32_t* anomalies,
                               void* stream) {
  HAMT_CHECK_ARG(B >= 0 && W > 0 && F > 0 && A > 0 && C > 0, "hamt_obs_gather: need W, F, A, C > 0");
  HAMT_CHECK_ARG(layout == HAMT_OBS_PANO || layout == HAMT_OBS_CAND, "hamt_obs_gather: bad layout");
  if (C > HAMT_OBS_MAX_CAND) {
    hamt_set_error("hamt_obs_gather: C %d above %d", C, HAMT_OBS_MAX_CAND);
    return HAMT_ERR_UNSUPPORTED;
  }
  HAMT_CHECK_ARG(feat && ang36 && cand_cnt && cand_point && cand_node && cand_ang && vp_base && scan_n && ep_scan && cur && view && ob_img &&
                     ob_ang && ob_nav && ob_mask && ob_len && cand_len && cand_node_out && cand_point_out && anomalies,
                 "hamt_obs_gather: null pointer");
  if (B == 0) return HAMT_OK;
  const int rows = W + ((hist_img || hist_pano_img || hist_pano_ang) ? 1 + 36 : 0);
  const int row_blocks = (rows + kWaves - 1) / kWaves;
  const int vec = F % 4 == 0 && aligned16(feat) && aligned16(ob_img) && aligned16(hist_img) && aligned16(hist_pano_img);
  hipLaunchKernelGGL(obs_gather_kernel, dim3(B, row_blocks < kMaxRowBlocks ? row_blocks : kMaxRowBlocks), dim3(64 * kWaves), 0,
                     as_stream(stream), B, W, F, A, C, layout, vec, feat, ang36, cand_cnt, cand_point, cand_node, cand_ang, vp_base, scan_n,
                     ep_scan, cur, view, ob_img, ob_ang, ob_nav, ob_mask, ob_len, cand_len, cand_node_out, cand_point_out, hist_img,
                     hist_pano_img, hist_pano_ang, anomalies);
  HAMT_CHECK_LAUNCH("hamt_obs_gather");
  return HAMT_OK;
}

extern "C" int hamt_obs_turn(int B, int W, const int32_t* cand_point_out, const int32_t* env_action, int32_t* view, int32_t* view_log_row,
                             void* stream) {
  HAMT_CHECK_ARG(B >= 0 && W > 0, "hamt_obs_turn: need W > 0");
  HAMT_CHECK_ARG(cand_point_out && env_action && view, "hamt_obs_turn: null pointer");
  if (B == 0) return HAMT_OK;
  hipLaunchKernelGGL(obs_turn_kernel, dim3((B + 255) / 256), dim3(256), 0, as_stream(stream), B, W, cand_point_out, env_action, view,
                     view_log_row);
  HAMT_CHECK_LAUNCH("hamt_obs_turn");
  return HAMT_OK;
}
