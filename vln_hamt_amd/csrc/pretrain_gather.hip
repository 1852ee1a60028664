// The batch a pretraining step consumes, built on the device from resident tables in one launch: what MultiStepNavData.get_input
// (pretrain_src/data/r2r_data.py:147-315), the six task datasets' corruption (r2r_tasks.py) and their collate functions' padding build on
// the host per sample, from a 32-byte record per sample (data/device_store.py holds the tables, data/device_tasks.py draws the records).
// A view feature is a pure function of (viewpoint, view); a trajectory's per-step values (viewpoint row, view looked at, action angle
// feature, action label, action angles, progress) are a function of (trajectory, step): both sit in HBM once.  A pure gather: no arithmetic
// on a value, so every output is exact.
//
// One wave per output row, rows of sample b in this order: Hmax history steps; Hmax x 36 panorama views (when the panorama outputs are
// given); Omax observation slots (when the observation outputs are given); one row for the masks, lengths and labels.  Every wave reads its
// sample's record and checks it (and, one step per lane, the step rows it reaches) before any table load, so a record pointing outside the
// tables touches nothing: the sample is written as zeros and counted.  Rows are copied 16 bytes per lane where the width and the bases
// allow, element by element otherwise (row_copy.h, shared with obs.hip).  Wave shuffles only: no LDS, no hand-off between waves; the only
// atomic is the anomaly counter.  Offsets into feat and prob are 64-bit.
#include "row_copy.h"

namespace {

constexpr int kWaves = 4;                          // rows per 256-thread workgroup
constexpr int kViews = 36;
constexpr int kHeadings = 12;
constexpr int kMaxOb = kViews + 1 + HAMT_PRETRAIN_MAX_CAND;      // the longest observation there is (rows per sample <= 32 * 37 + 101 + 1)

struct Tables {
  const float* feat;        // [NV, 36, F]
  const float* prob;        // [NV, 36, P] or NULL
  const float* ang36;       // [36, 36, A]
  const int32_t* cand_cnt;  // [NV]
  const int32_t* cand_view; // [NV, C]
  const float* cand_ang;    // [NV, C, 12, A]
  const int32_t* step_idx;  // [NS, 4]
  const float* step_val;    // [NS, A + 5]
  const float* sp_table;    // [36, 36, 2]
  const int32_t* records;   // [B, 8]
};

struct Outputs {
  float *hist_img, *hist_ang, *hist_pano_img, *hist_pano_ang, *hist_prob;
  uint8_t *hist_mrc, *hist_masks;
  int64_t* hist_lens;
  float *ob_img, *ob_ang;
  int64_t* ob_nav;
  uint8_t* ob_masks;
  int64_t *ob_lens, *act_view;
  float *act_ang, *progress;
  int64_t* anchor;
  float* sp_targets;
  int32_t* anomalies;
};

__global__ __launch_bounds__(64 * kWaves) void pretrain_gather_kernel(int B, int Hmax, int Omax, int F, int A, int P, int C, int layout,
                                                                      int64_t NV, int64_t NS, int vecF, int vecP, Tables T, Outputs O) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x;
  const bool has_ob = O.ob_img != nullptr, has_pano = O.hist_pano_img != nullptr;
  const int pano_rows = has_pano ? Hmax * kViews : 0, ob_rows = has_ob ? Omax : 0;
  const int rows = Hmax + pano_rows + ob_rows + 1;

  // ---- the sample's record, checked before anything it points to is read (every wave, in registers)
  const int32_t* rec = T.records + (int64_t)b * HAMT_PRETRAIN_RECORD;
  const int base = rec[0], t_rec = rec[1], flags = rec[2], anchor = rec[4];
  const uint32_t mrc = (uint32_t)rec[3];
  const int need = t_rec + (has_ob ? 1 : 0);                                          // step rows base .. base + need - 1
  bool ok = base >= 0 && t_rec >= 0 && t_rec <= Hmax && t_rec <= HAMT_PRETRAIN_MAX_HIST && (int64_t)base + need <= NS;
  ok = ok && (!O.sp_targets || (anchor >= 0 && anchor < kViews));
  int vp = -1, vw = -1;                                                               // lane s: viewpoint row and view of step s
  if (ok && lane < need) {
    vp = T.step_idx[((int64_t)base + lane) * 4 + 0];
    vw = T.step_idx[((int64_t)base + lane) * 4 + 1];
  }
  const bool lane_bad = ok && lane < need && !(vp >= 0 && (int64_t)vp < NV && vw >= 0 && vw < kViews);
  ok = ok && __ballot(lane_bad) == 0ull;
  const int t_cur = ok ? t_rec : 0;                                                   // history length

  const int r = blockIdx.y * kWaves + (threadIdx.x >> 6);                             // this wave's row (wave-uniform); no loop, so that
  if (r < rows) {                                                                     // each kind of row loads only the pointers it uses
    if (r < Hmax + pano_rows) {                                                       // ---- a history step, or one view of its panorama
      const bool whole = r >= Hmax;
      const int t = whole ? (r - Hmax) / kViews : r, v = whole ? (r - Hmax) % kViews : 0;
      const bool live = t < t_cur;
      const int svp = __shfl(vp, live ? t : 0, 64), svw = __shfl(vw, live ? t : 0, 64);
      const bool masked = live && ((mrc >> t) & 1u);
      const int64_t o = (int64_t)b * Hmax + t;
      const float* frow = T.feat + (int64_t)(live ? svp : 0) * kViews * F;
      if (whole) {
        const int64_t ov = o * kViews + v;
        copy_row(O.hist_pano_img + ov * F, live && !masked ? frow + (int64_t)v * F : nullptr, F, vecF != 0, lane);
        if (O.hist_pano_ang) copy_row(O.hist_pano_ang + ov * A, live ? T.ang36 + ((int64_t)svw * kViews + v) * A : nullptr, A, false, lane);
      } else {
        if (O.hist_img) copy_row(O.hist_img + o * F, live && !masked ? frow + (int64_t)svw * F : nullptr, F, vecF != 0, lane);
        if (O.hist_ang) copy_row(O.hist_ang + o * A, live ? T.step_val + ((int64_t)base + t) * (A + 5) : nullptr, A, false, lane);
        if (O.hist_prob)
          copy_row(O.hist_prob + o * P, live && T.prob ? T.prob + ((int64_t)svp * kViews + svw) * P : nullptr, P, vecP != 0, lane);
        if (O.hist_mrc && lane == 0) O.hist_mrc[o] = masked ? 1 : 0;
      }
    } else if (r < rows - 1) {                                                        // ---- an observation slot
      const int k = r - Hmax - pano_rows;
      const int cvp = __shfl(vp, t_cur, 64), cvw = __shfl(vw, t_cur, 64);             // (need = t_cur + 1 lanes hold a step when ok)
      const int64_t row = ok ? cvp : 0;
      const int n = ok ? min(max(T.cand_cnt[row], 0), min(C, layout == HAMT_PRETRAIN_CANDS_FIRST ? Omax - 1 : C)) : 0;
      const int pt = lane < n ? min(max(T.cand_view[row * C + lane], 0), kViews - 1) : -1;
      const uint32_t lo = wave_or_u(pt >= 0 && pt < 32 ? 1u << pt : 0u), hi = wave_or_u(pt >= 32 ? 1u << (pt - 32) : 0u);
      const uint64_t taken = ((uint64_t)hi << 32) | lo;                               // the views a candidate points to
      const float* frow = T.feat + row * kViews * F;
      const float *img = nullptr, *ang = nullptr;
      int nav = 0, len = 0;
      if (ok && layout == HAMT_PRETRAIN_CANDS_FIRST) {                                // candidates, STOP, the views no candidate points to
        const uint64_t free_views = ~taken & ((1ull << kViews) - 1);
        len = min(n + 1 + __popcll(free_views), Omax);
        const bool is_free = lane < kViews && ((free_views >> lane) & 1ull);
        const int rank = __popcll(free_views & ((1ull << lane) - 1ull));
        if (k < n) {
          const int point = __shfl(pt, k, 64);
          img = frow + (int64_t)point * F;
          ang = T.cand_ang + ((row * C + k) * kHeadings + cvw % kHeadings) * A;
          nav = 1;
        } else if (k == n) {
          nav = 2;
        } else if (k < len) {
          const int v = max(__ffsll((unsigned long long)__ballot(is_free && rank == k - n - 1)) - 1, 0);
          img = frow + (int64_t)v * F;
          ang = T.ang36 + ((int64_t)cvw * kViews + v) * A;
        }
      } else if (ok) {                                                                // the 36 views in their own order, then STOP
        len = min(kViews + 1, Omax);
        if (k < kViews && k < len) {
          img = frow + (int64_t)k * F;
          ang = T.ang36 + ((int64_t)cvw * kViews + k) * A;
          nav = (int)((taken >> k) & 1ull);
        } else if (k == kViews && k < len) {
          nav = 2;
        }
      }
      const int64_t o = (int64_t)b * Omax + k;
      copy_row(O.ob_img + o * F, (flags & HAMT_PRETRAIN_KILL_V) ? nullptr : img, F, vecF != 0, lane);
      copy_row(O.ob_ang + o * A, (flags & HAMT_PRETRAIN_KILL_A) ? nullptr : ang, A, false, lane);
      if (lane == 0) {
        O.ob_nav[o] = nav;
        O.ob_masks[o] = k < len ? 1 : 0;
      }
    } else {                                                                          // ---- masks, lengths, labels
      for (int i = lane; i <= Hmax; i += 64) O.hist_masks[(int64_t)b * (Hmax + 1) + i] = i <= t_cur ? 1 : 0;      // (+ 1: the cls slot)
      const int64_t cur = (int64_t)base + t_cur;                                      // the step stood on (read only when ok && has_ob)
      const bool lab = ok && has_ob;
      if (O.sp_targets)
        for (int i = lane; i < kViews * 2; i += 64) O.sp_targets[(int64_t)b * kViews * 2 + i] = ok ? T.sp_table[anchor * kViews * 2 + i] : 0.0f;
      if (O.act_ang && lane < 2) O.act_ang[(int64_t)b * 2 + lane] = lab ? T.step_val[cur * (A + 5) + A + 2 * layout + lane] : 0.0f;
      if (has_ob) {                                                                   // the observation's length (as its rows derive it)
        const int cvp = __shfl(vp, t_cur, 64);
        const int64_t row = ok ? cvp : 0;
        int len = 0;
        if (ok && layout == HAMT_PRETRAIN_CANDS_FIRST) {
          const int n = min(max(T.cand_cnt[row], 0), min(C, Omax - 1));
          const int pt = lane < n ? min(max(T.cand_view[row * C + lane], 0), kViews - 1) : -1;
          const uint32_t lo = wave_or_u(pt >= 0 && pt < 32 ? 1u << pt : 0u), hi = wave_or_u(pt >= 32 ? 1u << (pt - 32) : 0u);
          const uint64_t taken = ((uint64_t)hi << 32) | lo;
          len = min(n + 1 + kViews - __popcll(taken), Omax);
        } else if (ok) {
          len = min(kViews + 1, Omax);
        }
        if (lane == 0) O.ob_lens[b] = len;
      }
      if (lane == 0) {
        O.hist_lens[b] = t_cur + 1;
        if (O.act_view) O.act_view[b] = lab ? T.step_idx[cur * 4 + 2 + layout] : 0;
        if (O.progress) O.progress[b] = lab ? T.step_val[cur * (A + 5) + A + 4] : 0.0f;
        if (O.anchor) O.anchor[b] = ok ? anchor : 0;
        if (!ok) atomicAdd(&O.anomalies[0], 1);
      }
    }
  }
}

}  // namespace

extern "C" int hamt_pretrain_gather(int B, int Hmax, int Omax, int F, int A, int P, int C, int layout, int64_t NV, int64_t NS,
                                    const float* feat, const float* prob, const float* ang36, const int32_t* cand_cnt,
                                    const int32_t* cand_view, const float* cand_ang, const int32_t* step_idx, const float* step_val,
                                    const float* sp_table, const int32_t* records, float* hist_img, float* hist_ang, float* hist_pano_img,
                                    float* hist_pano_ang, float* hist_prob, uint8_t* hist_mrc, uint8_t* hist_masks, int64_t* hist_lens,
                                    float* ob_img, float* ob_ang, int64_t* ob_nav, uint8_t* ob_masks, int64_t* ob_lens, int64_t* act_view,
                                    float* act_ang, float* progress, int64_t* anchor, float* sp_targets, int32_t* anomalies, void* stream) {
  HAMT_CHECK_ARG(B >= 0 && Hmax >= 0 && Omax >= 0 && F > 0 && A > 0 && P >= 0 && C > 0 && NV >= 0 && NS >= 0,
                 "hamt_pretrain_gather: need F, A, C > 0 and no negative size");
  HAMT_CHECK_ARG(layout == HAMT_PRETRAIN_VIEWS36 || layout == HAMT_PRETRAIN_CANDS_FIRST, "hamt_pretrain_gather: bad layout");
  if (Hmax > HAMT_PRETRAIN_MAX_HIST || C > HAMT_PRETRAIN_MAX_CAND || Omax > kMaxOb) {
    hamt_set_error("hamt_pretrain_gather: Hmax %d above %d, C %d above %d or Omax %d above %d", Hmax, HAMT_PRETRAIN_MAX_HIST, C,
                   HAMT_PRETRAIN_MAX_CAND, Omax, kMaxOb);
    return HAMT_ERR_UNSUPPORTED;
  }
  HAMT_CHECK_ARG(feat && ang36 && cand_cnt && cand_view && cand_ang && step_idx && step_val && records && hist_masks && hist_lens && anomalies,
                 "hamt_pretrain_gather: null pointer");
  HAMT_CHECK_ARG(Hmax == 0 || (hist_img && hist_ang), "hamt_pretrain_gather: Hmax > 0 needs hist_img and hist_ang");
  HAMT_CHECK_ARG(!hist_pano_img == !hist_pano_ang, "hamt_pretrain_gather: hist_pano_img and hist_pano_ang come together");
  HAMT_CHECK_ARG(!hist_prob || (prob && P > 0), "hamt_pretrain_gather: hist_prob needs the prob table");
  HAMT_CHECK_ARG(ob_img ? (Omax > 0 && ob_ang && ob_nav && ob_masks && ob_lens) : (!ob_ang && !ob_nav && !ob_masks && !ob_lens),
                 "hamt_pretrain_gather: the observation outputs come together, with Omax > 0");
  HAMT_CHECK_ARG(ob_img || (!act_view && !act_ang && !progress), "hamt_pretrain_gather: action labels need the observation outputs");
  HAMT_CHECK_ARG(!sp_targets || sp_table, "hamt_pretrain_gather: sp_targets needs sp_table");
  if (B == 0) return HAMT_OK;
  const int rows = Hmax * (1 + (hist_pano_img ? 36 : 0)) + (ob_img ? Omax : 0) + 1;
  const int row_blocks = (rows + kWaves - 1) / kWaves;
  const int vecF = F % 4 == 0 && aligned16(feat) && aligned16(hist_img) && aligned16(hist_pano_img) && aligned16(ob_img);
  const int vecP = P > 0 && P % 4 == 0 && aligned16(prob) && aligned16(hist_prob);
  Tables T{feat, prob, ang36, cand_cnt, cand_view, cand_ang, step_idx, step_val, sp_table, records};
  Outputs O{hist_img, hist_ang, hist_pano_img, hist_pano_ang, hist_prob, hist_mrc, hist_masks, hist_lens, ob_img,  ob_ang,
            ob_nav,   ob_masks, ob_lens,       act_view,      act_ang,   progress, anchor,     sp_targets, anomalies};
  hipLaunchKernelGGL(pretrain_gather_kernel, dim3(B, row_blocks), dim3(64 * kWaves), 0, as_stream(stream), B, Hmax, Omax, F, A, P, C, layout, NV, NS, vecF, vecP, T, O);
  HAMT_CHECK_LAUNCH("hamt_pretrain_gather");
  return HAMT_OK;
}
