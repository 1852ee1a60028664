// PIL's antialiased 8-bit resample (Resample.c: Image.resize(size, BICUBIC | LANCZOS)) of whole uint8 views at a real scale factor,
// one launch for a batch: what the reference's preprocessing does on the host in front of everything else, render by render
// (build_image_lmdb.py:78 `resize((330, 248), Image.ANTIALIAS)`; precompute_img_features_vit.py:51-52, 96: timm's Resize(248) +
// CenterCrop(224)).  hamt_image_prep (image_prep.hip) resizes a crop BOX to 224 x 224; this file resizes the whole view to
// (OH, OW) and writes only a window of the result, so that "resize, then cut the centre" never computes what the cut drops.
//
// The result is PIL's bit for bit.  The tap function and the arithmetic of a pass are pil_resample.h's, shared with image_prep.hip:
//  * taps: hamt_image_resample_taps, on the HOST.  Lanczos needs sin(): the host's libm is what PIL calls, the device's sin is not,
//    so no tap is ever computed on the device; the kernel loads the caller's host-made tables.
//  * passes: horizontal first, the uint8 result feeds the vertical pass.
//  * an axis whose input and output sizes are equal is not resampled (PIL skips that pass): the kernel gives it the table
//    (xmin = coordinate, one tap of 1.0 = PIL_ONE), with which the pass arithmetic returns the byte it reads.
//
// kernel (one workgroup per view and tile of TR output rows): both tables -> LDS; horizontal pass of exactly the input rows the
// tile's vertical taps cover, window columns only, into LDS as uint8; vertical pass out of LDS -> the window.  No scratch, no atomics.
#include "common.h"
#include "pil_resample.h"

#define IR_TR 16                         // output rows per tile, halved by the launcher until the request fits
#define IR_LDS_MAX (160 * 1024)          // LDS of one CU

// ------------------------------------------------------------------------------------------------ taps (host)
static int ir_ksize(int in, int out, int filter) {
  return pil_ksize(in, out, filter == HAMT_RESAMPLE_LANCZOS ? pil_lanczos::support : pil_bicubic::support);
}

extern "C" int hamt_image_resample_taps(int in, int out, int filter, int first, int count, int32_t* xmin, int32_t* xcnt, int32_t* k, int ksize) {
  HAMT_CHECK_ARG(in > 0 && out > 0, "hamt_image_resample_taps: sizes %d -> %d", in, out);
  HAMT_CHECK_ARG(filter == HAMT_RESAMPLE_BICUBIC || filter == HAMT_RESAMPLE_LANCZOS, "hamt_image_resample_taps: unknown filter %d", filter);
  HAMT_CHECK_ARG((double)in / out <= 4096.0, "hamt_image_resample_taps: %d -> %d is a reduction of more than 4096", in, out);
  const int need = ir_ksize(in, out, filter);
  if (!xmin && !xcnt && !k) return need;
  HAMT_CHECK_ARG(xmin && xcnt && k, "hamt_image_resample_taps: null pointer");
  HAMT_CHECK_ARG(first >= 0 && count >= 0 && (long long)first + count <= out, "hamt_image_resample_taps: coordinates [%d, %d + %d) of %d", first, first, count, out);
  HAMT_CHECK_ARG(ksize >= need, "hamt_image_resample_taps: ksize %d < %d", ksize, need);
  for (int i = 0; i < count; ++i) {
    int32_t* kk = k + (size_t)i * ksize;
    if (filter == HAMT_RESAMPLE_LANCZOS) pil_taps<pil_lanczos>(first + i, in, out, kk, ksize, xmin + i, xcnt + i);
    else pil_taps<pil_bicubic>(first + i, in, out, kk, ksize, xmin + i, xcnt + i);
    for (int x = xcnt[i]; x < ksize; ++x) kk[x] = 0;
  }
  return need;
}

// ------------------------------------------------------------------------------------------------ kernel
// table of one axis as the caller lays it out: xmin[cnt_out] | xcnt[cnt_out] | k[cnt_out][K]; a null table (K == 0) is the skipped
// axis.  Copies entries [first, first + m) into LDS with the bounds clamped to the input side, so that no table content can make
// a pass read outside its view.
__device__ __forceinline__ void ir_load_table(const int32_t* __restrict__ tab, int cnt_out, int K, int first, int m, int origin, int in,
                                              int* __restrict__ sk, int* __restrict__ smin, int* __restrict__ scnt, int tid) {
  const int KS = K > 0 ? K : 1;
  for (int i = tid; i < m; i += 256) {
    int lo, c;
    if (K > 0) {
      lo = tab[first + i];
      c = tab[cnt_out + first + i];
    } else {
      lo = origin + first + i;
      c = 1;
    }
    lo = lo < 0 ? 0 : (lo > in - 1 ? in - 1 : lo);
    c = c < 0 ? 0 : (c > KS ? KS : c);
    if (c > in - lo) c = in - lo;
    smin[i] = lo;
    scnt[i] = c;
  }
  for (int i = tid; i < m * KS; i += 256) sk[i] = K > 0 ? tab[2 * (size_t)cnt_out + (size_t)first * K + i] : PIL_ONE;
}

__global__ __launch_bounds__(256) void image_resample_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int32_t* __restrict__ xtab,
                                                             const int32_t* __restrict__ ytab, int H, int W, int x0, int y0, int w, int h, int KX, int KY,
                                                             int TR, int rows_cap, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) int ir_smem[];
  const int view = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, tid = threadIdx.x;
  const int KXS = KX > 0 ? KX : 1, KYS = KY > 0 ? KY : 1;
  const int row0 = tile * TR, tr = h - row0 < TR ? h - row0 : TR;
  int* xk = ir_smem;
  int* xmin = xk + w * KXS;
  int* xcnt = xmin + w;
  int* yk = xcnt + w;
  int* ymin = yk + TR * KYS;
  int* ycnt = ymin + TR;
  uint8_t* tmp = (uint8_t*)(ycnt + TR);
  ir_load_table(xtab, w, KX, 0, w, x0, W, xk, xmin, xcnt, tid);
  ir_load_table(ytab, h, KY, row0, tr, y0, H, yk, ymin, ycnt, tid);
  __syncthreads();
  const int r_lo = ymin[0];
  int rows = ymin[tr - 1] + ycnt[tr - 1] - r_lo;
  if (rows > rows_cap) rows = rows_cap;            // (the host sized rows_cap from the same bounds: never taken)
  if (rows > H - r_lo) rows = H - r_lo;
  // ---- horizontal pass of input rows [r_lo, r_lo + rows), window columns
  const uint8_t* img = src + ((size_t)view * H + r_lo) * W * 3;
  for (int i = tid; i < rows * w; i += 256) {
    const int r = i / w, x = i % w;
    int c0, c1, c2;
    pil_sample3(img + ((size_t)r * W + xmin[x]) * 3, 3, xk + x * KXS, xcnt[x], c0, c1, c2);
    uint8_t* q = tmp + (size_t)i * 3;
    q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
  }
  __syncthreads();
  // ---- vertical pass
  uint8_t* out = dst + ((size_t)view * h + row0) * w * 3;
  for (int i = tid; i < tr * w; i += 256) {
    const int yy = i / w, x = i % w;
    int yl = ymin[yy] - r_lo;
    int n = ycnt[yy];
    if (yl < 0) yl = 0;                            // (tables with decreasing bounds: PIL's never are)
    if (yl + n > rows) n = rows - yl;
    int c0, c1, c2;
    pil_sample3(tmp + ((size_t)yl * w + x) * 3, w * 3, yk + yy * KYS, n, c0, c1, c2);
    uint8_t* q = out + (size_t)i * 3;
    q[0] = (uint8_t)c0; q[1] = (uint8_t)c1; q[2] = (uint8_t)c2;
  }
}

// ------------------------------------------------------------------------------------------------ launcher
// the host copy of one axis table against its geometry: every bound inside the input side, every count inside the table
static bool ir_table_ok(const int32_t* tab, int cnt_out, int K, int in) {
  for (int i = 0; i < cnt_out; ++i) {
    const int lo = tab[i], c = tab[cnt_out + i];
    if (lo < 0 || c < 1 || c > K || (long long)lo + c > in) return false;
    if (i && (lo < tab[i - 1] || lo + c < tab[i - 1] + tab[cnt_out + i - 1])) return false;      // both ends never move backwards
  }
  return true;
}

extern "C" int hamt_image_resample(const hamt_image_resample_desc* d, const int32_t* xtab_host, const int32_t* ytab_host, const int32_t* xtab_dev,
                                   const int32_t* ytab_dev, const uint8_t* src, uint8_t* dst, void* stream) {
  HAMT_CHECK_ARG(d && d->n >= 0 && d->H > 0 && d->W > 0 && d->OH > 0 && d->OW > 0, "hamt_image_resample: bad descriptor");
  HAMT_CHECK_ARG(d->filter == HAMT_RESAMPLE_BICUBIC || d->filter == HAMT_RESAMPLE_LANCZOS, "hamt_image_resample: unknown filter %d", d->filter);
  HAMT_CHECK_ARG(d->w >= 1 && d->h >= 1 && d->x0 >= 0 && d->y0 >= 0 && (long long)d->x0 + d->w <= d->OW && (long long)d->y0 + d->h <= d->OH,
                 "hamt_image_resample: window (%d, %d, %d, %d) empty or outside the %d x %d result", d->x0, d->y0, d->w, d->h, d->OH, d->OW);
  const bool skip_x = d->W == d->OW, skip_y = d->H == d->OH;
  const int KX = skip_x ? 0 : d->kx, KY = skip_y ? 0 : d->ky;
  if (!skip_x) {
    HAMT_CHECK_ARG(xtab_host && xtab_dev, "hamt_image_resample: null column table");
    HAMT_CHECK_ARG(d->kx >= 1 && d->kx <= 1 << 16 && ir_table_ok(xtab_host, d->w, d->kx, d->W), "hamt_image_resample: column table does not fit %d -> %d columns with %d taps", d->W, d->w, d->kx);
  }
  if (!skip_y) {
    HAMT_CHECK_ARG(ytab_host && ytab_dev, "hamt_image_resample: null row table");
    HAMT_CHECK_ARG(d->ky >= 1 && d->ky <= 1 << 16 && ir_table_ok(ytab_host, d->h, d->ky, d->H), "hamt_image_resample: row table does not fit %d -> %d rows with %d taps", d->H, d->h, d->ky);
  }
  if (d->n == 0) return HAMT_OK;
  HAMT_CHECK_ARG(src && dst, "hamt_image_resample: null pointer");
  // tile height: the largest of 16, 8, .. 1 whose tables and horizontal-pass rows fit in the LDS of a CU
  const size_t KXS = KX > 0 ? KX : 1, KYS = KY > 0 ? KY : 1;
  int TR = IR_TR, rows_cap = 0;
  size_t lds = 0;
  for (;; TR >>= 1) {
    rows_cap = 0;
    for (int r0 = 0; r0 < d->h; r0 += TR) {
      const int r1 = (r0 + TR < d->h ? r0 + TR : d->h) - 1;
      const int rows = skip_y ? r1 - r0 + 1 : ytab_host[r1] + ytab_host[d->h + r1] - ytab_host[r0];
      if (rows > rows_cap) rows_cap = rows;
    }
    lds = ((size_t)d->w * (KXS + 2) + (size_t)TR * (KYS + 2)) * 4 + (size_t)rows_cap * d->w * 3;
    if (lds <= IR_LDS_MAX || TR == 1) break;
  }
  HAMT_CHECK_ARG(lds <= IR_LDS_MAX, "hamt_image_resample: %d x %d -> window %d x %d of %d x %d needs %zu bytes of LDS at one output row per workgroup (%d at most)",
                 d->H, d->W, d->h, d->w, d->OH, d->OW, lds, IR_LDS_MAX);
  const int ntiles = (d->h + TR - 1) / TR;
  HAMT_CHECK_ARG((long long)d->n * ntiles < (1ll << 31), "hamt_image_resample: %d views x %d tiles", d->n, ntiles);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&image_resample_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, IR_LDS_MAX);
  hipLaunchKernelGGL(image_resample_kernel, dim3((unsigned)(d->n * ntiles)), dim3(256), lds, as_stream(stream), src, dst, skip_x ? nullptr : xtab_dev,
                     skip_y ? nullptr : ytab_dev, d->H, d->W, d->x0, d->y0, d->w, d->h, KX, KY, TR, rows_cap, ntiles);
  HAMT_CHECK_LAUNCH("hamt_image_resample");
  return HAMT_OK;
}
