// REVERIE's object embedding on gfx950 (finetune reverie/vlnbert_navref.py:31-42), per object row:
//     y = dropout( LN_out( LN_img(x1) + LN_ang(ang W_ang^T + b_ang) + LN_pos(pos W_pos^T + b_pos) + nav + tt ) )
// where x1 = obj W_img^T + b_img is the dense layer's output (bf16 or fp32) and tt / nav are the token-type row 1 and the STOP
// navigation-type row 2, the same two rows for every object.  ONE launch behind the dense layer: the K = 4 and K = 5 projections
// are FMAs that never exist in memory, the four LayerNorms keep fp32 statistics in registers, the dropout mask is hamt_ln_fwd's
// p_post stream (regenerated in backward, nothing stored).  Backward is one launch + a small reduction: per row the branch
// activations are recomputed, dropout and the output LayerNorm are undone to de = d(LN_out input), then the three branch
// LayerNorm backwards give dx1 (fp32, or the padded bf16 image img_linear's weight gradient reads) and the projections' inputs'
// gradients; the 17 column sums (every gamma / beta, both projections' weights and biases, colsum(de) for the two constant rows)
// leave as per-block partials that the second kernel sums in a fixed order into the gradient destinations.
//
// One 64-lane wave per row; the row layout, its arithmetic, the K = 4 projection and the column-sum reduction are ln_row.h's (this
// file multiplies its row sums by 1 / H where norm.hip and vis_embed.hip divide by H).  All three branch LayerNorms may see a
// constant row (REVERIE pads a viewpoint without objects with one all-zero row, and the fresh obj_embeddings have zero biases):
// the variance is then 0 and rstd = eps^-1/2 = 1e6, the normalised row 0 -- the output is beta, as in the reference, and no
// value is non-finite.
#include "ln_row.h"

namespace {

constexpr int OE_A = LN_ANGLE_K;   // angle features
constexpr int OE_P = 5;            // position box features
// per-block partial vectors: dgamma_out, dbeta_out, colsum(de), dgamma_img / ang / pos, db_ang, dW_ang[:, 0..3], db_pos, dW_pos[:, 0..4]
constexpr int OE_V = 7 + 1 + OE_A + 1 + OE_P - 1;
static_assert(OE_V == 17, "partial vector count");
constexpr int OE_NWV = 8;          // waves (rows) per backward block
constexpr uint32_t OE_POST_SALT = 0x5bd1e995u;   // hamt_ln_fwd's p_post stream (norm.hip)

// columns c .. c+3 of pos W^T + b, W [H, 5]: the 20 weights of 4 consecutive columns are 5 aligned float4s (c % 4 == 0)
__device__ __forceinline__ float4 oe_pos(const float* __restrict__ W, const float* __restrict__ b, int c, const float (&x)[OE_P]) {
  const float4* w = (const float4*)(W + (size_t)c * OE_P);
  const float4 q0 = w[0], q1 = w[1], q2 = w[2], q3 = w[3], q4 = w[4];
  const float4 bb = *(const float4*)(b + c);
  float4 a;
  a.x = bb.x + x[0] * q0.x + x[1] * q0.y + x[2] * q0.z + x[3] * q0.w + x[4] * q1.x;
  a.y = bb.y + x[0] * q1.y + x[1] * q1.z + x[2] * q1.w + x[3] * q2.x + x[4] * q2.y;
  a.z = bb.z + x[0] * q2.z + x[1] * q2.w + x[2] * q3.x + x[3] * q3.y + x[4] * q3.z;
  a.w = bb.w + x[0] * q3.w + x[1] * q4.x + x[2] * q4.y + x[3] * q4.z + x[4] * q4.w;
  return a;
}

__device__ __forceinline__ void oe_row_inputs(const hamt_obj_embed_desc& d, int row, const float* __restrict__ ang,
                                              const float* __restrict__ pos, float (&av)[OE_A], float (&pv)[OE_P]) {
  const float* ar = ang + (size_t)row * d.ld_ang;
  const float* pr = pos + (size_t)row * d.ld_pos;      // 20-byte rows: element loads, no vector alignment assumed
#pragma unroll
  for (int k = 0; k < OE_A; ++k) av[k] = ar[k];
#pragma unroll
  for (int k = 0; k < OE_P; ++k) pv[k] = pr[k];
}

// e = LN_img(v) + LN_ang(a) + LN_pos(q) + nav + tt   (the reference's order of the additions)
__device__ __forceinline__ float4 oe_sum_branches(const float4 n1, const float4 n2, const float4 n3, const hamt_obj_embed_params& p, int c) {
  const float4 g1 = *(const float4*)(p.gamma_img + c), b1 = *(const float4*)(p.beta_img + c);
  const float4 g2 = *(const float4*)(p.gamma_ang + c), b2 = *(const float4*)(p.beta_ang + c);
  const float4 g3 = *(const float4*)(p.gamma_pos + c), b3 = *(const float4*)(p.beta_pos + c);
  const float4 tn = *(const float4*)(p.nav + c), tt = *(const float4*)(p.tt + c);
  float4 e = affine4(n1, g1, b1);
  acc4(e, affine4(n2, g2, b2));
  acc4(e, affine4(n3, g3, b3));
  acc4(e, tn);
  acc4(e, tt);
  return e;
}

template <int NV>
__global__ __launch_bounds__(256) void obj_embed_fwd_kernel(hamt_obj_embed_desc d, hamt_obj_embed_params p, const void* __restrict__ x1,
                                                            const float* __restrict__ ang, const float* __restrict__ pos,
                                                            float* __restrict__ y, float* __restrict__ stats, const uint64_t* __restrict__ rng) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  const int H = d.H;
  if (row >= d.M) return;
  float av[OE_A], pv[OE_P];
  oe_row_inputs(d, row, ang, pos, av, pv);
  const int xfmt = d.x_bf16 ? LN_BF16 : LN_F32;
  float4 v[NV], a[NV], q[NV];
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      v[i] = load_row4(x1, (size_t)row * H + c, xfmt);
      a[i] = angle_proj4(p.w_ang, p.b_ang, c, make_float4(av[0], av[1], av[2], av[3]));
      q[i] = oe_pos(p.w_pos, p.b_pos, c, pv);
      s1 += sum4(v[i]); s2 += sum4(a[i]); s3 += sum4(q[i]);
    } else { v[i] = zero4(); a[i] = v[i]; q[i] = v[i]; }
  }
  wave_sum3(s1, s2, s3);
  const float inv_h = 1.0f / (float)H;
  const float m1 = s1 * inv_h, m2 = s2 * inv_h, m3 = s3 * inv_h;
  float t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((i * 64 + lane) * 4 < H) { t1 += sqdev4(v[i], m1); t2 += sqdev4(a[i], m2); t3 += sqdev4(q[i], m3); }
  wave_sum3(t1, t2, t3);
  const float r1 = rsqrtf(t1 * inv_h + d.eps_img), r2 = rsqrtf(t2 * inv_h + d.eps_ang), r3 = rsqrtf(t3 * inv_h + d.eps_pos);
  float s4 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      v[i] = oe_sum_branches(norm4(v[i], m1, r1), norm4(a[i], m2, r2), norm4(q[i], m3, r3), p, c);
      s4 += sum4(v[i]);
    }
  }
  s4 = wave_sum(s4);
  const float m4 = s4 * inv_h;
  float t4 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((i * 64 + lane) * 4 < H) t4 += sqdev4(v[i], m4);
  t4 = wave_sum(t4);
  const float r4 = rsqrtf(t4 * inv_h + d.eps_out);
  const RngKey kd = rng_key(rng, d.call_id ^ OE_POST_SALT);
  const float ik = d.p_drop > 0.f ? 1.0f / (1.0f - d.p_drop) : 1.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      float4 r = affine4(norm4(v[i], m4, r4), *(const float4*)(p.gamma_out + c), *(const float4*)(p.beta_out + c));
      if (d.p_drop > 0.f) r = mul4(r, keep4(kd, row, c, d.p_drop, ik));
      *(float4*)(y + (size_t)row * H + c) = r;
    }
  }
  if (lane == 0) {
    const size_t M = d.M;
    stats[row] = m1; stats[M + row] = r1; stats[2 * M + row] = m2; stats[3 * M + row] = r2;
    stats[4 * M + row] = m3; stats[5 * M + row] = r3; stats[6 * M + row] = m4; stats[7 * M + row] = r4;
  }
}

// one row per wave, OE_NWV rows per block; the block's 17 column-sum contributions go to ws[block][17][H]
template <int NV>
__global__ __launch_bounds__(64 * OE_NWV) void obj_embed_bwd_kernel(hamt_obj_embed_desc d, hamt_obj_embed_params p, const float* __restrict__ dy,
                                                                    const void* __restrict__ x1, const float* __restrict__ ang,
                                                                    const float* __restrict__ pos, const float* __restrict__ stats,
                                                                    float* __restrict__ dx, bf16_t* __restrict__ dx16, float* __restrict__ ws,
                                                                    const uint64_t* __restrict__ rng) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int H = d.H;
  const size_t M = d.M;
  if (dx16 && blockIdx.x == 0) zero_pad_rows(dx16, H, d.M + w, d.Mpad16, OE_NWV, lane);
  const int row = blockIdx.x * OE_NWV + w;
  const bool live = row < d.M;      // (no early return: every wave takes part in the block reduction below)
  float av[OE_A] = {0.f, 0.f, 0.f, 0.f}, pv[OE_P] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const float4 z4 = zero4();
  float4 dyo[NV], no[NV], de[NV], n1[NV], n2[NV], n3[NV], d2[NV], d3[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { dyo[i] = z4; no[i] = z4; de[i] = z4; n1[i] = z4; n2[i] = z4; n3[i] = z4; d2[i] = z4; d3[i] = z4; }
  if (live) {
    oe_row_inputs(d, row, ang, pos, av, pv);
    const float m1 = stats[row], r1 = stats[M + row], m2 = stats[2 * M + row], r2 = stats[3 * M + row];
    const float m3 = stats[4 * M + row], r3 = stats[5 * M + row], m4 = stats[6 * M + row], r4 = stats[7 * M + row];
    const RngKey kd = rng_key(rng, d.call_id ^ OE_POST_SALT);
    const float ik = d.p_drop > 0.f ? 1.0f / (1.0f - d.p_drop) : 1.0f;
      const float inv_h = 1.0f / (float)H;
    const int xfmt = d.x_bf16 ? LN_BF16 : LN_F32;
    float su = 0.f, tu = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        n1[i] = norm4(load_row4(x1, o, xfmt), m1, r1);
        n2[i] = norm4(angle_proj4(p.w_ang, p.b_ang, c, make_float4(av[0], av[1], av[2], av[3])), m2, r2);
        n3[i] = norm4(oe_pos(p.w_pos, p.b_pos, c, pv), m3, r3);
        no[i] = norm4(oe_sum_branches(n1[i], n2[i], n3[i], p, c), m4, r4);
        float4 g = *(const float4*)(dy + o);
        if (d.p_drop > 0.f) g = mul4(g, keep4(kd, row, c, d.p_drop, ik));
        dyo[i] = g;
        const float4 u = mul4(g, *(const float4*)(p.gamma_out + c));
        su += sum4(u); tu += dot4(u, no[i]);
      }
    }
    su = wave_sum(su); tu = wave_sum(tu);
    float s1 = 0.f, t1 = 0.f, s2 = 0.f, t2 = 0.f, s3 = 0.f, t3 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        de[i] = ln_dx4(mul4(dyo[i], *(const float4*)(p.gamma_out + c)), no[i], su * inv_h, tu * inv_h, r4);
        const float4 u1 = mul4(de[i], *(const float4*)(p.gamma_img + c));
        const float4 u2 = mul4(de[i], *(const float4*)(p.gamma_ang + c));
        const float4 u3 = mul4(de[i], *(const float4*)(p.gamma_pos + c));
        s1 += sum4(u1); t1 += dot4(u1, n1[i]);
        s2 += sum4(u2); t2 += dot4(u2, n2[i]);
        s3 += sum4(u3); t3 += dot4(u3, n3[i]);
      }
    }
    wave_sum3(s1, s2, s3);
    wave_sum3(t1, t2, t3);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        const float4 r = ln_dx4(mul4(de[i], *(const float4*)(p.gamma_img + c)), n1[i], s1 * inv_h, t1 * inv_h, r1);
        if (dx) *(float4*)(dx + o) = r;
        if (dx16) store_bf4(dx16, o, r);
        d2[i] = ln_dx4(mul4(de[i], *(const float4*)(p.gamma_ang + c)), n2[i], s2 * inv_h, t2 * inv_h, r2);
        d3[i] = ln_dx4(mul4(de[i], *(const float4*)(p.gamma_pos + c)), n3[i], s3 * inv_h, t3 * inv_h, r3);
      }
    }
  }
  // block sums of the 17 contributions, one vector at a time through LDS (a dead wave contributes zeros), waves in a fixed order
#pragma unroll
  for (int v = 0; v < OE_V; ++v) {
    float4 t[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (v == 0) t[i] = mul4(dyo[i], no[i]);
      else if (v == 1) t[i] = dyo[i];
      else if (v == 2) t[i] = de[i];
      else if (v == 3) t[i] = mul4(de[i], n1[i]);
      else if (v == 4) t[i] = mul4(de[i], n2[i]);
      else if (v == 5) t[i] = mul4(de[i], n3[i]);
      else if (v == 6) t[i] = d2[i];
      else if (v < 7 + OE_A) t[i] = scale4(d2[i], av[v - 7]);
      else if (v == 7 + OE_A) t[i] = d3[i];
      else t[i] = scale4(d3[i], pv[v - 8 - OE_A]);
    }
    block_partial<NV, OE_NWV>(t, ws, (size_t)blockIdx.x * OE_V + v, H);
  }
}

// ws[nb][17][H] -> the gradients (ADDED to what is there).  block = 64 columns (16 float4 lanes) x 16 partial-row phases.
__global__ __launch_bounds__(256) void obj_embed_reduce_kernel(int nb, int H, const float* __restrict__ ws, hamt_obj_embed_grads g) {
  const int per = H / 64;                          // blocks per vector
  const int v = blockIdx.x / per, col = (blockIdx.x % per) * 64 + (threadIdx.x & 15) * 4;
  float4 t;
  if (!reduce_partials(ws + (size_t)v * H + col, (size_t)OE_V * H, nb, t)) return;
  const float e[4] = {t.x, t.y, t.z, t.w};
  float* dst[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  int stride = 1, off = 0;
  switch (v) {
    case 0: dst[0] = g.dgamma_out; break;
    case 1: dst[0] = g.dbeta_out; break;
    case 2: dst[0] = g.dbeta_img; dst[1] = g.dbeta_ang; dst[2] = g.dbeta_pos; dst[3] = g.dtt; dst[4] = g.dnav; break;
    case 3: dst[0] = g.dgamma_img; break;
    case 4: dst[0] = g.dgamma_ang; break;
    case 5: dst[0] = g.dgamma_pos; break;
    case 6: dst[0] = g.db_ang; break;
    case 7 + OE_A: dst[0] = g.db_pos; break;
    default:
      if (v < 7 + OE_A) { dst[0] = g.dw_ang; stride = OE_A; off = v - 7; }
      else { dst[0] = g.dw_pos; stride = OE_P; off = v - 8 - OE_A; }
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if (!dst[j]) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[j][(size_t)(col + k) * stride + off] += e[k];
  }
}

int oe_blocks(int M) { return (M + OE_NWV - 1) / OE_NWV; }

bool oe_aligned(const void* ptr) { return ((uintptr_t)ptr & 15u) == 0; }

int oe_check(const hamt_obj_embed_desc* d, const hamt_obj_embed_params* p, const char* who) {
  HAMT_CHECK_ARG(d && p, "%s: null pointer", who);
  if (int rc = ln_row_check_h(d->H, who)) return rc;
  if (int rc = ln_row_check_angle(d->A, d->ld_ang, 1, who)) return rc;      // (rows are read element by element)
  HAMT_CHECK_ARG(d->P == OE_P && d->ld_pos >= OE_P, "%s: position features %d (ld %d): only 5 is built", who, d->P, d->ld_pos);
  HAMT_CHECK_ARG(d->M >= 0 && d->p_drop >= 0.f && d->p_drop < 1.f, "%s: bad M=%d or dropout p=%g", who, d->M, (double)d->p_drop);
  const void* ps[14] = {p->w_ang, p->b_ang, p->w_pos, p->b_pos, p->gamma_img, p->beta_img, p->gamma_ang, p->beta_ang, p->gamma_pos,
                        p->beta_pos, p->tt, p->nav, p->gamma_out, p->beta_out};
  for (int i = 0; i < 14; ++i) HAMT_CHECK_ARG(ps[i] && oe_aligned(ps[i]), "%s: parameter %d null or not 16-byte aligned", who, i);
  return HAMT_OK;
}

}  // namespace

size_t hamt_obj_embed_ws_bytes(int M, int H) {     // (hamt_workspace_bytes: HAMT_WS_OBJ_EMBED_BWD)
  return (size_t)oe_blocks(M < 1 ? 1 : M) * OE_V * H * 4;
}

extern "C" int hamt_obj_embed_fwd(const hamt_obj_embed_desc* d, const hamt_obj_embed_params* p, const void* x1, const float* ang,
                                  const float* pos, float* y, float* stats, const uint64_t* rng, void* stream) {
  const int rc = oe_check(d, p, "hamt_obj_embed_fwd");
  if (rc != HAMT_OK) return rc;
  HAMT_CHECK_ARG(x1 && ang && pos && y && stats, "hamt_obj_embed_fwd: null pointer");
  HAMT_CHECK_ARG(oe_aligned(x1) && oe_aligned(y), "hamt_obj_embed_fwd: x1 / y not 16-byte aligned");
  if (d->M == 0) return HAMT_OK;
  dim3 grid((d->M + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((obj_embed_fwd_kernel<NV>), grid, block, 0, s, *d, *p, x1, ang, pos, y, stats, rng)
  LN_ROW_DISPATCH(d->H, LAUNCH)
#undef LAUNCH
  HAMT_CHECK_LAUNCH("hamt_obj_embed_fwd");
  return HAMT_OK;
}

extern "C" int hamt_obj_embed_bwd(const hamt_obj_embed_desc* d, const hamt_obj_embed_params* p, const hamt_obj_embed_grads* g, const float* dy,
                                  const void* x1, const float* ang, const float* pos, const float* stats, float* dx, void* dx16, float* ws,
                                  const uint64_t* rng, void* stream) {
  const int rc = oe_check(d, p, "hamt_obj_embed_bwd");
  if (rc != HAMT_OK) return rc;
  HAMT_CHECK_ARG(g && dy && x1 && ang && pos && stats && ws, "hamt_obj_embed_bwd: null pointer");
  HAMT_CHECK_ARG(dx || dx16, "hamt_obj_embed_bwd: neither dx nor dx16");
  HAMT_CHECK_ARG(!dx16 || d->Mpad16 >= d->M, "hamt_obj_embed_bwd: Mpad16 %d < M %d", d->Mpad16, d->M);
  if (d->M == 0) return HAMT_OK;
  const int nb = oe_blocks(d->M);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((obj_embed_bwd_kernel<NV>), dim3(nb), dim3(64 * OE_NWV), 0, s, *d, *p, dy, x1, ang, pos, stats, dx, (bf16_t*)dx16, ws, rng)
  LN_ROW_DISPATCH(d->H, LAUNCH)
#undef LAUNCH
  HAMT_CHECK_LAUNCH("hamt_obj_embed_bwd");
  hipLaunchKernelGGL(obj_embed_reduce_kernel, dim3(OE_V * (d->H / 64)), dim3(256), 0, s, nb, d->H, ws, *g);
  HAMT_CHECK_LAUNCH("hamt_obj_embed_bwd (reduce)");
  return HAMT_OK;
}
