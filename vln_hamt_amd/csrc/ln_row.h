// The one-wave-per-row LayerNorm skeleton shared by norm.hip, vis_embed.hip and obj_embed.hip (gfx950).
//
// A row of H <= 1024 elements lives in one 64-lane wave as `float4 v[NV]`, NV = ceil(H / 256): lane l holds columns
// c = (i * 64 + l) * 4 .. c + 3 of vector i (live while c < H).  Statistics are fp32 wave-shuffle sums (wave_sum* of common.h).
// Column sums over rows leave a block as partials ws[block][v][H] (block_partial), and a second kernel sums the partials of one
// float4 column group in 16 phases (reduce_partials).
//
// The helpers return SUMS, never means: norm.hip and vis_embed.hip divide by (float)H, obj_embed.hip multiplies by 1 / (float)H,
// and the two round differently.  Every helper is a plain expression that inlines into its caller, so what the compiler may
// contract into an FMA is what it could contract when the expression was written out in place; none of them reassociates.
// One caveat: the compiler optimises a helper on its own before it inlines it and may swap the operands of a commutative add
// there.  That is exact in itself, but it can change how the SLP vectoriser pairs neighbouring sums, and with it which products
// become FMAs (ln_bwd_kernel in norm.hip keeps two sums spelled out for this reason).  After an edit here, compare the kernels'
// FMA / multiply / add counts with the previous build (profiles/ln_row_refactor_resources.txt shows how).
#pragma once
#include "common.h"

enum { LN_F32 = 0, LN_BF16 = 1, LN_F16 = 4 };     // element format of a row in memory (hamt_ln_desc.io16 names x's with these bits)
constexpr int LN_ANGLE_K = 4;                     // angle features (angle_feat_size is 4 everywhere in the reference)

// ---- row I/O
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
// elements o .. o+3 of a row-major image (o % 4 == 0)
__device__ __forceinline__ float4 load_row4(const void* xv, size_t o, int fmt) {
  float4 a;
  if (fmt & LN_F16) {
    const uint2 u = *(const uint2*)((const bf16_t*)xv + o);
    unpack_h2(u.x, a.x, a.y); unpack_h2(u.y, a.z, a.w);
  } else if (fmt & LN_BF16) {
    const uint2 u = *(const uint2*)((const bf16_t*)xv + o);
    a = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
  } else a = *(const float4*)((const float*)xv + o);
  return a;
}
// ... and their bf16 image
__device__ __forceinline__ void store_bf4(bf16_t* img, size_t o, const float4 r) { *(uint2*)(img + o) = make_uint2(pack_bf2(r.x, r.y), pack_bf2(r.z, r.w)); }
// Rows [M, Mpad16) of a bf16 image are zero: they are reduction padding of the fast GEMMs.  The calling wave zeroes rows
// first, first + step, ... below Mpad16.
__device__ __forceinline__ void zero_pad_rows(bf16_t* img, int H, int first, int Mpad16, int step, int lane) {
  for (int row = first; row < Mpad16; row += step)
    for (int c = lane * 4; c < H; c += 256) *(uint2*)(img + (size_t)row * H + c) = make_uint2(0u, 0u);
}

// ---- float4 row arithmetic
__device__ __forceinline__ float sum4(const float4 v) { return v.x + v.y + v.z + v.w; }
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 mul4(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 scale4(const float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ void acc4(float4& t, const float4 a) { t.x += a.x; t.y += a.y; t.z += a.z; t.w += a.w; }
// t += a * b (component after component: the order the statements had when they were written out in place)
__device__ __forceinline__ void fmacc4(float4& t, const float4 a, const float4 b) { t.x += a.x * b.x; t.y += a.y * b.y; t.z += a.z * b.z; t.w += a.w * b.w; }
__device__ __forceinline__ void fmacc4(float4& t, const float4 a, float s) { t.x += a.x * s; t.y += a.y * s; t.z += a.z * s; t.w += a.w * s; }
__device__ __forceinline__ float sqdev4(const float4 v, float m) {
  const float e0 = v.x - m, e1 = v.y - m, e2 = v.z - m, e3 = v.w - m;
  return e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
}
__device__ __forceinline__ float4 norm4(const float4 v, float m, float r) {
  return make_float4((v.x - m) * r, (v.y - m) * r, (v.z - m) * r, (v.w - m) * r);
}
__device__ __forceinline__ float4 affine4(const float4 n, const float4 g, const float4 b) {
  return make_float4(n.x * g.x + b.x, n.y * g.y + b.y, n.z * g.z + b.z, n.w * g.w + b.w);
}
// LayerNorm backward of one row given u = dy * gamma, the normalised input n, their row means cu / eu and rstd r
__device__ __forceinline__ float4 ln_dx4(const float4 u, const float4 n, float cu, float eu, float r) {
  return make_float4(r * (u.x - cu - n.x * eu), r * (u.y - cu - n.y * eu), r * (u.z - cu - n.z * eu), r * (u.w - cu - n.w * eu));
}
// dropout keep factors of columns c .. c+3 (c % 4 == 0) of a row: the 4-wide mask stream of common.h (one hash pair per 4
// elements instead of two hashes per element -- the LayerNorm-backward kernel spent 15 % of its time hashing)
__device__ __forceinline__ float4 keep4(RngKey k, int row, int c, float p, float inv_keep) {
  float f[4];
  drop_scale4(k, hamt_mix32((uint32_t)row ^ k.k0), (uint32_t)(c >> 2), p, inv_keep, f);
  return make_float4(f[0], f[1], f[2], f[3]);
}

// columns c .. c+3 of ang W^T + b, W = nn.Linear's [H, 4]: one float4 per output column
__device__ __forceinline__ float4 angle_proj4(const float* __restrict__ W, const float* __restrict__ b, int c, const float4 x) {
  const float4* w = (const float4*)(W + (size_t)c * LN_ANGLE_K);
  const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  const float4 bb = *(const float4*)(b + c);
  float4 a;
  a.x = bb.x + x.x * w0.x + x.y * w0.y + x.z * w0.z + x.w * w0.w;
  a.y = bb.y + x.x * w1.x + x.y * w1.y + x.z * w1.z + x.w * w1.w;
  a.z = bb.z + x.x * w2.x + x.y * w2.y + x.z * w2.z + x.w * w2.w;
  a.w = bb.w + x.x * w3.x + x.y * w3.y + x.z * w3.z + x.w * w3.w;
  return a;
}

// ---- column sums over rows
// Block stage: the NWV waves' contributions t to ONE vector go through LDS, waves summed in a fixed order, to row `vec` of
// ws[][H] (vec = block * vectors + v).  Every wave of the block calls it; the LDS buffer is free again on return.
template <int NV, int NWV>
__device__ __forceinline__ void block_partial(const float4 (&t)[NV], float* __restrict__ ws, size_t vec, int H) {
  __shared__ float4 red[NWV][NV * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) red[w][i * 64 + lane] = t[i];
  __syncthreads();
  for (int e = threadIdx.x; e < NV * 64; e += 64 * NWV) {
    const int c = e * 4;
    if (c < H) {
      float4 s = red[0][e];
#pragma unroll
      for (int k = 1; k < NWV; ++k) acc4(s, red[k][e]);
      *(float4*)(ws + vec * H + c) = s;
    }
  }
  __syncthreads();
}

// Grid stage, for a 256-thread block = 16 float4 column lanes x 16 phases: `col4` is this lane's float4 of partial 0, partial b
// lies b * stride floats behind it.  Phase p sums partials p, p + 16, ... (4 independent loads per trip), the 16 phase sums
// meet in LDS, and phase 0 -- the threads for which this returns true -- gets the total in `t`.  (Every phase sum starts from
// +0, so none is -0, and the total does not depend on whether phase 0's sum is added to zero or taken as the start.)
__device__ __forceinline__ bool reduce_partials(const float* __restrict__ col4, size_t stride, int nb, float4& t) {
  const int l16 = threadIdx.x & 15, ph = threadIdx.x >> 4;
  t = zero4();
  for (int b0 = ph; b0 < nb; b0 += 64) {
    float4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + 16 * u;
      q[u] = b < nb ? *(const float4*)(col4 + (size_t)b * stride) : zero4();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc4(t, q[u]);
  }
  __shared__ float4 red[16][16];
  red[ph][l16] = t;
  __syncthreads();
  if (ph != 0) return false;
#pragma unroll
  for (int i = 1; i < 16; ++i) acc4(t, red[i][l16]);
  return true;
}

// ---- host side
// LAUNCH(NV) for the NV = ceil(H / 256) of a row of H elements
#define LN_ROW_DISPATCH(H, LAUNCH) \
  switch (((H) + 255) / 256) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }

// the embedders' rows: whole 64-column groups (their reductions read float4 columns in blocks of 64)
static inline int ln_row_check_h(int H, const char* who) {
  HAMT_CHECK_ARG(H % 64 == 0 && H >= 64 && H <= 1024, "%s: H=%d unsupported (need H%%64==0, H<=1024)", who, H);
  return HAMT_OK;
}
// A angle features in rows of ld floats; ld_align = 4 where the row is read as one float4
static inline int ln_row_check_angle(int A, int ld, int ld_align, const char* who) {
  HAMT_CHECK_ARG(A == LN_ANGLE_K && ld >= LN_ANGLE_K && ld % ld_align == 0, "%s: angle features %d (ld %d): only 4 is built", who, A, ld);
  return HAMT_OK;
}
