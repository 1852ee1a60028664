// Panorama view transform (image_data.py:70-80, 225-237: timm's create_transform per view on the host) as two launches for a whole
// batch of uint8 views: crop -> PIL-BICUBIC resize to 224 x 224 -> flip -> colour jitter -> x / 255 -> (x - 0.5) / 0.5.
//
// The result is PIL's bit for bit, so the arithmetic is PIL's (Resample.c, Blend.c, Convert.c), not an approximation of it:
//  * resize: two passes of 8-bit resampling over the CROPPED view, bicubic.  The tap function and the arithmetic of a pass are
//    pil_resample.h's, shared with image_resample.hip; the taps are made here on the device, per view slot.
//  * jitter: Image.blend(degenerate, image, factor) in float32, truncated (clipped when the factor is outside [0, 1]), rounded
//    to uint8 after every op.  The contrast op needs the mean grey value of the whole image as it is when the op runs: the
//    first kernel stops in front of it and leaves one integer partial sum per row tile, the second kernel adds the 14 partials
//    (integers: exact, order independent) and goes on.
//  * normalisation through the caller's 256-entry table.
//
// kernel 1 (one workgroup per view slot and tile of 16 output rows): taps -> horizontal pass of the rows the tile needs into LDS
//   -> vertical pass -> flip -> ops in front of contrast -> uint8 HWC scratch image + grey partial sum.
// kernel 2 (grid stride over 4-pixel groups): contrast and the ops after it -> table -> NCHW fp32, or the rows hamt_patchify
//   would make of that tensor (fp32 / bf16).
#include "common.h"
#include "pil_resample.h"

#define IP_OUT 224
#define IP_TR 16                         // output rows per tile
#define IP_NT (IP_OUT / IP_TR)           // 14 tiles per view
#define IP_KMAX 16                       // taps per output coordinate the tables hold (box side <= 3.5 x 224)
#define IP_ROWB (IP_OUT * 3)             // bytes of one resized row
#define IP_IMG (IP_OUT * IP_OUT * 3)
#define IP_SLOT (IP_IMG + 64)            // scratch per slot: the uint8 image + 14 int32 partial sums (padded to 64 bytes)
#define IP_P 16                          // ViT patch
#define IP_PG (IP_OUT / IP_P)            // 14 patches per side
#define IP_PK (3 * IP_P * IP_P)          // 768 columns of a patch row

size_t hamt_image_prep_ws_bytes(int n) { return (size_t)(n > 0 ? n : 0) * IP_SLOT; }

static inline int ip_ksize(int in) { return pil_ksize(in, IP_OUT, pil_bicubic::support); }

__device__ __forceinline__ int ip_grey(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
// Image.blend(degenerate d, image p, factor f)
__device__ __forceinline__ int ip_blend(int d, int p, float f) {
  const float t = (float)d + f * (float)(p - d);
  if (f >= 0.0f && f <= 1.0f) return (int)t;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}
__device__ __forceinline__ void ip_apply(int op, const hamt_image_view& v, int mean, int& r, int& g, int& b) {
  if (op == HAMT_JIT_BRIGHTNESS) {
    r = ip_blend(0, r, v.brightness); g = ip_blend(0, g, v.brightness); b = ip_blend(0, b, v.brightness);
  } else if (op == HAMT_JIT_CONTRAST) {
    r = ip_blend(mean, r, v.contrast); g = ip_blend(mean, g, v.contrast); b = ip_blend(mean, b, v.contrast);
  } else if (op == HAMT_JIT_SATURATION) {
    const int l = ip_grey(r, g, b);
    r = ip_blend(l, r, v.saturation); g = ip_blend(l, g, v.saturation); b = ip_blend(l, b, v.saturation);
  }
}
// position (0..2) of the contrast op in the chain, 3 when there is none
__device__ __forceinline__ int ip_contrast_pos(int order) {
  for (int j = 0; j < 3; ++j)
    if (((order >> (2 * j)) & 3) == HAMT_JIT_CONTRAST) return j;
  return 3;
}

__global__ __launch_bounds__(256) void image_prep_resize_kernel(const hamt_image_view* __restrict__ views, const uint8_t* __restrict__ src,
                                                                int H, int W, int KX, int rows_cap, uint8_t* __restrict__ ws) {
  extern __shared__ int ip_smem[];
  const int slot = blockIdx.x / IP_NT, tile = blockIdx.x % IP_NT, tid = threadIdx.x;
  const hamt_image_view v = views[slot];
  if (v.zero || v.src < 0) return;
  int* xk = ip_smem;
  int* xmin = xk + IP_OUT * KX;
  int* xcnt = xmin + IP_OUT;
  int* yk = xcnt + IP_OUT;
  int* ymin = yk + IP_TR * IP_KMAX;
  int* ycnt = ymin + IP_TR;
  int* red = ycnt + IP_TR;
  uint8_t* tmp = (uint8_t*)(red + 4);
  if (tid < IP_OUT) pil_taps<pil_bicubic>(tid, v.width, IP_OUT, xk + tid * KX, KX, xmin + tid, xcnt + tid);
  else if (tid < IP_OUT + IP_TR) pil_taps<pil_bicubic>(tile * IP_TR + tid - IP_OUT, v.height, IP_OUT, yk + (tid - IP_OUT) * IP_KMAX, IP_KMAX, ymin + tid - IP_OUT, ycnt + tid - IP_OUT);
  __syncthreads();
  const int r_lo = ymin[0];
  int rows = ymin[IP_TR - 1] + ycnt[IP_TR - 1] - r_lo;
  if (rows > rows_cap) rows = rows_cap;            // (the host sized rows_cap from the same bounds: never taken)
  // ---- horizontal pass of input rows [r_lo, r_lo + rows) of the box
  const uint8_t* img = src + (size_t)v.src * H * W * 3 + ((size_t)(v.top + r_lo) * W + v.left) * 3;
  for (int i = tid; i < rows * IP_ROWB; i += 256) {
    const int r = i / IP_ROWB, rem = i % IP_ROWB, x = rem / 3, c = rem % 3;
    tmp[i] = (uint8_t)pil_sample1(img + (size_t)r * W * 3 + xmin[x] * 3 + c, 3, xk + x * KX, xcnt[x]);
  }
  __syncthreads();
  // ---- vertical pass, flip, the ops in front of contrast, grey sum
  const int cpos = ip_contrast_pos(v.order);
  uint8_t* out = ws + (size_t)slot * IP_SLOT;
  int gsum = 0;
  for (int i = tid; i < IP_TR * IP_OUT; i += 256) {
    const int yy = i / IP_OUT, x = i % IP_OUT;
    const int y0 = ymin[yy] - r_lo;
    int n = ycnt[yy];
    if (y0 + n > rows) n = rows - y0;
    int r, g, b;
    pil_sample3(tmp + (y0 * IP_OUT + x) * 3, IP_ROWB, yk + yy * IP_KMAX, n, r, g, b);
    for (int j = 0; j < cpos && j < 3; ++j) ip_apply((v.order >> (2 * j)) & 3, v, 0, r, g, b);
    if (cpos < 3) gsum += ip_grey(r, g, b);
    const int xo = v.flip ? IP_OUT - 1 - x : x;
    uint8_t* q = out + ((size_t)(tile * IP_TR + yy) * IP_OUT + xo) * 3;
    q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
  }
  if (cpos < 3) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) gsum += __shfl_xor(gsum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = gsum;
    __syncthreads();
    if (tid == 0) ((int*)(out + IP_IMG))[tile] = red[0] + red[1] + red[2] + red[3];
  }
}

template <typename TO, bool PATCH>
__global__ __launch_bounds__(256) void image_prep_store_kernel(const hamt_image_view* __restrict__ views, int n, const uint8_t* __restrict__ ws,
                                                               const float* __restrict__ lut, TO* __restrict__ y, int ldy, int Rpad) {
  const size_t per = (size_t)IP_OUT * (IP_OUT / 4), real = (size_t)n * per;
  const size_t total = real + (PATCH ? (size_t)(Rpad - n * IP_PG * IP_PG) * (IP_PK / 4) : 0);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    if (i >= real) {                               // patch rows beyond the views: zero, as hamt_patchify leaves them
      const size_t j = i - real;
      TO* q = y + ((size_t)n * IP_PG * IP_PG + j / (IP_PK / 4)) * ldy + (j % (IP_PK / 4)) * 4;
      if constexpr (sizeof(TO) == 2) *(uint2*)q = make_uint2(0u, 0u);
      else *(float4*)q = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int slot = (int)(i / per), rem = (int)(i % per), yy = rem / (IP_OUT / 4), x = (rem % (IP_OUT / 4)) * 4;
    const hamt_image_view v = views[slot];
    float o[3][4];
    if (v.zero || v.src < 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) o[c][p] = 0.0f;
    } else {
      const uint8_t* img = ws + (size_t)slot * IP_SLOT;
      const uint32_t* w = (const uint32_t*)(img + ((size_t)yy * IP_OUT + x) * 3);
      const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
      const int cpos = ip_contrast_pos(v.order);
      int mean = 0;
      if (cpos < 3) {
        const int* part = (const int*)(img + IP_IMG);
        int s = 0;
#pragma unroll
        for (int t = 0; t < IP_NT; ++t) s += part[t];
        mean = (2 * s + IP_OUT * IP_OUT) / (2 * IP_OUT * IP_OUT);        // int(sum / N + 0.5)
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int bi = 3 * p;                        // byte index of the pixel's R in the 12 bytes
        auto byte = [&](int j) { return (int)(((j < 4 ? w0 : (j < 8 ? w1 : w2)) >> (8 * (j & 3))) & 0xffu); };
        int r = byte(bi), g = byte(bi + 1), b = byte(bi + 2);
        for (int j = cpos; j < 3; ++j) ip_apply((v.order >> (2 * j)) & 3, v, mean, r, g, b);
        o[0][p] = lut[r]; o[1][p] = lut[g]; o[2][p] = lut[b];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      TO* q;
      if constexpr (PATCH) q = y + ((size_t)slot * IP_PG * IP_PG + (yy / IP_P) * IP_PG + x / IP_P) * ldy + c * IP_P * IP_P + (yy % IP_P) * IP_P + x % IP_P;
      else q = y + (((size_t)slot * 3 + c) * IP_OUT + yy) * IP_OUT + x;
      if constexpr (sizeof(TO) == 2) *(uint2*)q = make_uint2(pack_bf2(o[c][0], o[c][1]), pack_bf2(o[c][2], o[c][3]));
      else *(float4*)q = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    }
  }
}

extern "C" int hamt_image_prep(const hamt_image_prep_desc* d, const hamt_image_view* views_host, const hamt_image_view* views_dev,
                               const uint8_t* src, const float* lut, void* y, void* ws, size_t ws_bytes, void* stream) {
  HAMT_CHECK_ARG(d && d->n >= 0 && d->n_src >= 0 && d->H > 0 && d->W > 0, "hamt_image_prep: bad descriptor");
  HAMT_CHECK_ARG(d->layout == HAMT_IMAGE_NCHW || d->layout == HAMT_IMAGE_PATCHES, "hamt_image_prep: unknown layout %d", d->layout);
  HAMT_CHECK_ARG(y && ((uintptr_t)y % 16) == 0, "hamt_image_prep: output must be 16-byte aligned");
  HAMT_CHECK_ARG(lut && (d->n == 0 || (views_host && views_dev)), "hamt_image_prep: null pointer");
  if (d->layout == HAMT_IMAGE_NCHW) {
    HAMT_CHECK_ARG(d->dtype_y == HAMT_F32, "hamt_image_prep: the nchw layout is fp32");
  } else {
    HAMT_CHECK_ARG(d->dtype_y == HAMT_F32 || d->dtype_y == HAMT_BF16, "hamt_image_prep: patch rows are fp32 or bf16");
    HAMT_CHECK_ARG(d->ldy >= IP_PK && (d->ldy * (d->dtype_y == HAMT_BF16 ? 2 : 4)) % 16 == 0, "hamt_image_prep: ldy %d (>= %d, rows 16-byte aligned)", d->ldy, IP_PK);
    HAMT_CHECK_ARG((long long)d->Rpad >= (long long)d->n * IP_PG * IP_PG, "hamt_image_prep: Rpad %d < %d views x %d patches", d->Rpad, d->n, IP_PG * IP_PG);
  }
  int active = 0, kx = 5, rows_cap = 1;
  for (int i = 0; i < d->n; ++i) {
    const hamt_image_view& v = views_host[i];
    if (v.zero || v.src < 0) continue;
    HAMT_CHECK_ARG(v.src < d->n_src, "hamt_image_prep: slot %d: source view %d of %d", i, v.src, d->n_src);
    HAMT_CHECK_ARG(v.width >= 1 && v.height >= 1, "hamt_image_prep: slot %d: empty crop box %d x %d", i, v.width, v.height);
    HAMT_CHECK_ARG(v.left >= 0 && v.top >= 0 && (long long)v.left + v.width <= d->W && (long long)v.top + v.height <= d->H,
                   "hamt_image_prep: slot %d: crop box (%d, %d, %d, %d) outside the %d x %d view", i, v.left, v.top, v.width, v.height, d->W, d->H);
    HAMT_CHECK_ARG((v.order & ~63) == 0 && ((v.order & 3) == HAMT_JIT_CONTRAST) + (((v.order >> 2) & 3) == HAMT_JIT_CONTRAST) + (((v.order >> 4) & 3) == HAMT_JIT_CONTRAST) <= 1,
                   "hamt_image_prep: slot %d: bad jitter order %d (three 2-bit ops, contrast at most once)", i, v.order);
    if (ip_ksize(v.width) > IP_KMAX || ip_ksize(v.height) > IP_KMAX) {
      hamt_set_error("hamt_image_prep: slot %d: crop box %d x %d needs more than %d taps (side <= %d)", i, v.width, v.height, IP_KMAX, IP_OUT * 7 / 2);
      return HAMT_ERR_UNSUPPORTED;
    }
    if (ip_ksize(v.width) > kx) kx = ip_ksize(v.width);
    const double sc = (double)v.height / IP_OUT, fs = sc > 1.0 ? sc : 1.0;
    const int rc = (int)ceil((IP_TR - 1) * sc + 4.0 * fs) + 2;       // last tap end - first tap start of a 16-row tile, rounded up
    if (rc > rows_cap) rows_cap = rc;
    ++active;
  }
  if (active) {
    HAMT_CHECK_ARG(src && ws && ((uintptr_t)ws % 16) == 0 && ws_bytes >= hamt_image_prep_ws_bytes(d->n),
                   "hamt_image_prep: scratch of %zu bytes needed (HAMT_WS_IMAGE_PREP), 16-byte aligned", hamt_image_prep_ws_bytes(d->n));
    const size_t lds = (size_t)(IP_OUT * kx + 2 * IP_OUT + IP_TR * IP_KMAX + 2 * IP_TR + 4) * 4 + (size_t)rows_cap * IP_ROWB;
    hipLaunchKernelGGL(image_prep_resize_kernel, dim3(d->n * IP_NT), dim3(256), lds, as_stream(stream), views_dev, src, d->H, d->W, kx, rows_cap, (uint8_t*)ws);
    HAMT_CHECK_LAUNCH("hamt_image_prep (resize)");
  }
  const bool patch = d->layout == HAMT_IMAGE_PATCHES;
  const size_t total = (size_t)d->n * IP_OUT * (IP_OUT / 4) + (patch ? (size_t)(d->Rpad - d->n * IP_PG * IP_PG) * (IP_PK / 4) : 0);
  if (total == 0) return HAMT_OK;
  const size_t nb = (total + 255) / 256;
  const dim3 grid((unsigned)(nb < 65536 ? nb : 65536));
  const uint8_t* w8 = (const uint8_t*)ws;
  if (!patch) hipLaunchKernelGGL((image_prep_store_kernel<float, false>), grid, dim3(256), 0, as_stream(stream), views_dev, d->n, w8, lut, (float*)y, 0, 0);
  else if (d->dtype_y == HAMT_BF16) hipLaunchKernelGGL((image_prep_store_kernel<bf16_t, true>), grid, dim3(256), 0, as_stream(stream), views_dev, d->n, w8, lut, (bf16_t*)y, d->ldy, d->Rpad);
  else hipLaunchKernelGGL((image_prep_store_kernel<float, true>), grid, dim3(256), 0, as_stream(stream), views_dev, d->n, w8, lut, (float*)y, d->ldy, d->Rpad);
  HAMT_CHECK_LAUNCH("hamt_image_prep (store)");
  return HAMT_OK;
}
