// attn_cls: ONE query per (image, head) against that image's Sk keys -- the cls row of a ViT's last block in a forward-only pass
// (vision_transformer.py:154-178 with only x[:, 0] read afterwards, :346).  hamt_attn_small_fwd would spend a whole MFMA row
// tile on that one query; here the work is two streaming passes over K and V (memory bound: 2 * Sk * 64 elements per wave).
//
// One wave per (image, head).  Lane l = (grp, sub) = (l / 8, l % 8): `sub` owns the 8 columns [8 sub, 8 sub + 8) of the head, `grp`
// one of the 8 keys a wave instruction covers, so every K / V load is 8 rows x 128 (bf16) or 256 (fp32) contiguous bytes, 16 bytes
// per lane.  Order of the arithmetic (tests/_attn_cls_ref.py restates it in numpy):
//   score_j = scale * butterfly_{1,2,4}( fma chain over the lane's 8 columns, left to right )
//   m = max_j score_j;  p_j = expf(score_j - m);  l = butterfly_{32..1}( lane's p_j, j = lane, lane + 64, ... added in order )
//   o_c = butterfly_{8,16,32}( fma chain over the keys j = grp, grp + 8, ... of p_j * v_jc ) / l
// Scores and probabilities pass through 1 KB of LDS; no atomics, no scratch.
#include "common.h"

namespace {

constexpr int CLS_MAX_SK = 256;

struct ClsArgs {
  const void *q, *k, *v;
  void* o;
  int heads, Sk, ldq, ldk, ldv, ldo;
  float scale;
};

__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int i = 0; i < 4; ++i) { f[i] = a[i]; f[4 + i] = b[i]; }
}
__device__ __forceinline__ void load8(const bf16_t* p, float (&f)[8]) {
  const s16x8 a = *reinterpret_cast<const s16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) f[i] = bf2f((bf16_t)a[i]);
}
__device__ __forceinline__ void store8(float* p, const float (&f)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{f[4], f[5], f[6], f[7]};
}

template <typename TI>
__global__ __launch_bounds__(HAMT_WAVE) void attn_cls_fwd_kernel(ClsArgs a) {
  __shared__ float s_p[CLS_MAX_SK];
  const int lane = threadIdx.x, sub = lane & 7, grp = lane >> 3;
  const int b = blockIdx.x / a.heads, h = blockIdx.x - b * a.heads, Sk = a.Sk;
  const int col = h * 64 + sub * 8;
  const TI* kb = static_cast<const TI*>(a.k) + (size_t)b * Sk * a.ldk + col;
  const TI* vb = static_cast<const TI*>(a.v) + (size_t)b * Sk * a.ldv + col;
  float q[8];
  load8(static_cast<const TI*>(a.q) + (size_t)b * a.ldq + col, q);
  // ---- scores.  A key index behind the last one re-reads the last row (in bounds) and its result is dropped.
#pragma unroll 4
  for (int j0 = 0; j0 < Sk; j0 += 8) {
    const int j = j0 + grp;
    float kk[8];
    load8(kb + (size_t)min(j, Sk - 1) * a.ldk, kk);
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc = __builtin_fmaf(q[i], kk[i], acc);
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if (sub == 0 && j < Sk) s_p[j] = acc * a.scale;
  }
  __syncthreads();
  // ---- softmax in fp32 over the <= 4 keys of each lane
  float sv[CLS_MAX_SK / HAMT_WAVE], m = -INFINITY;
#pragma unroll
  for (int t = 0; t < CLS_MAX_SK / HAMT_WAVE; ++t) {
    const int j = lane + t * HAMT_WAVE;
    sv[t] = j < Sk ? s_p[j] : -INFINITY;
    m = fmaxf(m, sv[t]);
  }
  m = wave_max(m);
  float l = 0.0f;
#pragma unroll
  for (int t = 0; t < CLS_MAX_SK / HAMT_WAVE; ++t) {
    const int j = lane + t * HAMT_WAVE;
    if (j < Sk) {
      const float p = expf(sv[t] - m);
      l += p;
      s_p[j] = p;
    }
  }
  l = wave_sum(l);
  __syncthreads();
  // ---- P V
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int j0 = 0; j0 < Sk; j0 += 8) {
    const int j = j0 + grp;
    float vv[8];
    load8(vb + (size_t)min(j, Sk - 1) * a.ldv, vv);
    if (j < Sk) {
      const float p = s_p[j];
#pragma unroll
      for (int i = 0; i < 8; ++i) o[i] = __builtin_fmaf(p, vv[i], o[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    o[i] += __shfl_xor(o[i], 8, 64);
    o[i] += __shfl_xor(o[i], 16, 64);
    o[i] += __shfl_xor(o[i], 32, 64);
    o[i] = o[i] / l;
  }
  if (grp == 0) store8(static_cast<float*>(a.o) + (size_t)b * a.ldo + col, o);
}

}  // namespace

extern "C" int hamt_attn_cls_fwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, void* o, void* stream) {
  const char* who = "hamt_attn_cls_fwd";
  HAMT_CHECK_ARG(d, "%s: null desc", who);
  HAMT_CHECK_ARG(d->d_head == 64, "%s: d_head=%d unsupported (64 only)", who, d->d_head);
  HAMT_CHECK_ARG(d->B >= 0 && d->heads > 0 && d->Sk > 0, "%s: bad sizes", who);
  HAMT_CHECK_ARG(d->Sq == 1, "%s: one query per (image, head): Sq=%d", who, d->Sq);
  HAMT_CHECK_ARG(d->p_drop == 0.f, "%s: no dropout on this path (p_drop=%g)", who, (double)d->p_drop);
  HAMT_CHECK_ARG((d->dtype_qkv == HAMT_F32 || d->dtype_qkv == HAMT_BF16) && d->dtype_o == HAMT_F32,
                 "%s: q / k / v are fp32 or bf16, o is fp32", who);
  if (d->Sk > CLS_MAX_SK) {
    hamt_set_error("%s: Sk=%d is beyond the %d keys one wave keeps", who, d->Sk, CLS_MAX_SK);
    return HAMT_ERR_UNSUPPORTED;
  }
  const int es = d->dtype_qkv == HAMT_BF16 ? 2 : 4, eo = 4, W = d->heads * 64;
  HAMT_CHECK_ARG(d->ldq >= W && d->ldk >= W && d->ldv >= W && d->ldo >= W, "%s: a row stride is shorter than heads * 64", who);
  HAMT_CHECK_ARG((d->ldq * es) % 16 == 0 && (d->ldk * es) % 16 == 0 && (d->ldv * es) % 16 == 0 && (d->ldo * eo) % 16 == 0,
                 "%s: rows must be 16-byte aligned", who);
  HAMT_CHECK_ARG((long long)d->B * d->heads <= 0x7fffffffLL, "%s: B * heads exceeds the grid", who);
  if (d->B == 0) return HAMT_OK;
  HAMT_CHECK_ARG(q && k && v && o, "%s: null pointer", who);
  HAMT_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) % 16 == 0, "%s: q / k / v / o must be 16-byte aligned", who);
  const ClsArgs a{q, k, v, o, d->heads, d->Sk, d->ldq, d->ldk, d->ldv, d->ldo, d->scale};
  const dim3 grid((unsigned)(d->B * d->heads)), block(HAMT_WAVE);
  hipStream_t s = as_stream(stream);
  if (d->dtype_qkv == HAMT_BF16) hipLaunchKernelGGL((attn_cls_fwd_kernel<bf16_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((attn_cls_fwd_kernel<float>), grid, block, 0, s, a);
  HAMT_CHECK_LAUNCH(who);
  return HAMT_OK;
}
