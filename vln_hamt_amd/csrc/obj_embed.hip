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
// One 64-lane wave per row, H <= 1024 kept in registers as float4s.  All three branch LayerNorms may see a constant row (REVERIE
// pads a viewpoint without objects with one all-zero row, and the fresh obj_embeddings have zero biases): the variance is then 0
// and rstd = eps^-1/2 = 1e6, the normalised row 0 -- the output is beta, as in the reference, and no value is non-finite.
#include "common.h"

namespace {

constexpr int OE_A = 4;            // angle features
constexpr int OE_P = 5;            // position box features
// per-block partial vectors: dgamma_out, dbeta_out, colsum(de), dgamma_img / ang / pos, db_ang, dW_ang[:, 0..3], db_pos, dW_pos[:, 0..4]
constexpr int OE_V = 7 + 1 + OE_A + 1 + OE_P - 1;
static_assert(OE_V == 17, "partial vector count");
constexpr int OE_NWV = 8;          // waves (rows) per backward block
constexpr uint32_t OE_POST_SALT = 0x5bd1e995u;   // hamt_ln_fwd's p_post stream (norm.hip)

__device__ __forceinline__ float4 oe_load_x(const void* xv, size_t o, int bf16) {
  if (bf16) {
    const uint2 u = *(const uint2*)((const bf16_t*)xv + o);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
  }
  return *(const float4*)((const float*)xv + o);
}

// columns c .. c+3 of ang W^T + b, W [H, 4]: one float4 per output column
__device__ __forceinline__ float4 oe_ang(const float* __restrict__ W, const float* __restrict__ b, int c, const float (&x)[OE_A]) {
  const float4* w = (const float4*)(W + (size_t)c * OE_A);
  const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  const float4 bb = *(const float4*)(b + c);
  float4 a;
  a.x = bb.x + x[0] * w0.x + x[1] * w0.y + x[2] * w0.z + x[3] * w0.w;
  a.y = bb.y + x[0] * w1.x + x[1] * w1.y + x[2] * w1.z + x[3] * w1.w;
  a.z = bb.z + x[0] * w2.x + x[1] * w2.y + x[2] * w2.z + x[3] * w2.w;
  a.w = bb.w + x[0] * w3.x + x[1] * w3.y + x[2] * w3.z + x[3] * w3.w;
  return a;
}

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

__device__ __forceinline__ float oe_sum4(const float4 v) { return v.x + v.y + v.z + v.w; }
__device__ __forceinline__ float oe_dot4(const float4 a, const float4 b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }
__device__ __forceinline__ float4 oe_norm(const float4 v, float m, float r) {
  return make_float4((v.x - m) * r, (v.y - m) * r, (v.z - m) * r, (v.w - m) * r);
}
__device__ __forceinline__ float oe_sqdev(const float4 v, float m) {
  const float e0 = v.x - m, e1 = v.y - m, e2 = v.z - m, e3 = v.w - m;
  return e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
}

__device__ __forceinline__ void wave_sum3(float& a, float& b, float& c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64); }
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
  float4 e;
  e.x = (((n1.x * g1.x + b1.x) + (n2.x * g2.x + b2.x)) + (n3.x * g3.x + b3.x) + tn.x) + tt.x;
  e.y = (((n1.y * g1.y + b1.y) + (n2.y * g2.y + b2.y)) + (n3.y * g3.y + b3.y) + tn.y) + tt.y;
  e.z = (((n1.z * g1.z + b1.z) + (n2.z * g2.z + b2.z)) + (n3.z * g3.z + b3.z) + tn.z) + tt.z;
  e.w = (((n1.w * g1.w + b1.w) + (n2.w * g2.w + b2.w)) + (n3.w * g3.w + b3.w) + tn.w) + tt.w;
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
  float4 v[NV], a[NV], q[NV];
  float s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      v[i] = oe_load_x(x1, (size_t)row * H + c, d.x_bf16);
      a[i] = oe_ang(p.w_ang, p.b_ang, c, av);
      q[i] = oe_pos(p.w_pos, p.b_pos, c, pv);
      s1 += oe_sum4(v[i]); s2 += oe_sum4(a[i]); s3 += oe_sum4(q[i]);
    } else { v[i] = make_float4(0.f, 0.f, 0.f, 0.f); a[i] = v[i]; q[i] = v[i]; }
  }
  wave_sum3(s1, s2, s3);
  const float inv_h = 1.0f / (float)H;
  const float m1 = s1 * inv_h, m2 = s2 * inv_h, m3 = s3 * inv_h;
  float t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((i * 64 + lane) * 4 < H) { t1 += oe_sqdev(v[i], m1); t2 += oe_sqdev(a[i], m2); t3 += oe_sqdev(q[i], m3); }
  wave_sum3(t1, t2, t3);
  const float r1 = rsqrtf(t1 * inv_h + d.eps_img), r2 = rsqrtf(t2 * inv_h + d.eps_ang), r3 = rsqrtf(t3 * inv_h + d.eps_pos);
  float s4 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      v[i] = oe_sum_branches(oe_norm(v[i], m1, r1), oe_norm(a[i], m2, r2), oe_norm(q[i], m3, r3), p, c);
      s4 += oe_sum4(v[i]);
    }
  }
  s4 = wave_sum(s4);
  const float m4 = s4 * inv_h;
  float t4 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((i * 64 + lane) * 4 < H) t4 += oe_sqdev(v[i], m4);
  t4 = wave_sum(t4);
  const float r4 = rsqrtf(t4 * inv_h + d.eps_out);
  const RngKey kd = rng_key(rng, d.call_id ^ OE_POST_SALT);
  const float ik = d.p_drop > 0.f ? 1.0f / (1.0f - d.p_drop) : 1.0f;
  const uint32_t rowh = hamt_mix32((uint32_t)row ^ kd.k0);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const float4 g = *(const float4*)(p.gamma_out + c), b = *(const float4*)(p.beta_out + c);
      float4 r;
      r.x = (v[i].x - m4) * r4 * g.x + b.x; r.y = (v[i].y - m4) * r4 * g.y + b.y;
      r.z = (v[i].z - m4) * r4 * g.z + b.z; r.w = (v[i].w - m4) * r4 * g.w + b.w;
      if (d.p_drop > 0.f) {
        float f_[4]; drop_scale4(kd, rowh, (uint32_t)(c >> 2), d.p_drop, ik, f_);
        r.x *= f_[0]; r.y *= f_[1]; r.z *= f_[2]; r.w *= f_[3];
      }
      *(float4*)(y + (size_t)row * H + c) = r;
    }
  }
  if (lane == 0) {
    const size_t M = d.M;
    stats[row] = m1; stats[M + row] = r1; stats[2 * M + row] = m2; stats[3 * M + row] = r2;
    stats[4 * M + row] = m3; stats[5 * M + row] = r3; stats[6 * M + row] = m4; stats[7 * M + row] = r4;
  }
}

__device__ __forceinline__ float4 oe_mul(const float4 a, const float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float4 oe_scale(const float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
// LayerNorm backward of one row given u = dy * gamma, the normalised input n, their wave means cu / eu and rstd r
__device__ __forceinline__ float4 oe_ln_dx(const float4 u, const float4 n, float cu, float eu, float r) {
  return make_float4(r * (u.x - cu - n.x * eu), r * (u.y - cu - n.y * eu), r * (u.z - cu - n.z * eu), r * (u.w - cu - n.w * eu));
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
  if (dx16 && blockIdx.x == 0)      // zero the reduction-padding rows [M, Mpad16) of the bf16 gradient image
    for (int r = d.M + w; r < d.Mpad16; r += OE_NWV)
      for (int c = lane * 4; c < H; c += 256) *(uint2*)(dx16 + (size_t)r * H + c) = make_uint2(0u, 0u);
  const int row = blockIdx.x * OE_NWV + w;
  const bool live = row < d.M;      // (no early return: every wave takes part in the block reduction below)
  float av[OE_A] = {0.f, 0.f, 0.f, 0.f}, pv[OE_P] = {0.f, 0.f, 0.f, 0.f, 0.f};
  const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 dyo[NV], no[NV], de[NV], n1[NV], n2[NV], n3[NV], d2[NV], d3[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { dyo[i] = z4; no[i] = z4; de[i] = z4; n1[i] = z4; n2[i] = z4; n3[i] = z4; d2[i] = z4; d3[i] = z4; }
  if (live) {
    oe_row_inputs(d, row, ang, pos, av, pv);
    const float m1 = stats[row], r1 = stats[M + row], m2 = stats[2 * M + row], r2 = stats[3 * M + row];
    const float m3 = stats[4 * M + row], r3 = stats[5 * M + row], m4 = stats[6 * M + row], r4 = stats[7 * M + row];
    const RngKey kd = rng_key(rng, d.call_id ^ OE_POST_SALT);
    const float ik = d.p_drop > 0.f ? 1.0f / (1.0f - d.p_drop) : 1.0f;
    const uint32_t rowh = hamt_mix32((uint32_t)row ^ kd.k0);
    const float inv_h = 1.0f / (float)H;
    float su = 0.f, tu = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        n1[i] = oe_norm(oe_load_x(x1, o, d.x_bf16), m1, r1);
        n2[i] = oe_norm(oe_ang(p.w_ang, p.b_ang, c, av), m2, r2);
        n3[i] = oe_norm(oe_pos(p.w_pos, p.b_pos, c, pv), m3, r3);
        no[i] = oe_norm(oe_sum_branches(n1[i], n2[i], n3[i], p, c), m4, r4);
        float4 g = *(const float4*)(dy + o);
        if (d.p_drop > 0.f) {
          float f_[4]; drop_scale4(kd, rowh, (uint32_t)(c >> 2), d.p_drop, ik, f_);
          g.x *= f_[0]; g.y *= f_[1]; g.z *= f_[2]; g.w *= f_[3];
        }
        dyo[i] = g;
        const float4 u = oe_mul(g, *(const float4*)(p.gamma_out + c));
        su += oe_sum4(u); tu += oe_dot4(u, no[i]);
      }
    }
    su = wave_sum(su); tu = wave_sum(tu);
    float s1 = 0.f, t1 = 0.f, s2 = 0.f, t2 = 0.f, s3 = 0.f, t3 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        de[i] = oe_ln_dx(oe_mul(dyo[i], *(const float4*)(p.gamma_out + c)), no[i], su * inv_h, tu * inv_h, r4);
        const float4 u1 = oe_mul(de[i], *(const float4*)(p.gamma_img + c));
        const float4 u2 = oe_mul(de[i], *(const float4*)(p.gamma_ang + c));
        const float4 u3 = oe_mul(de[i], *(const float4*)(p.gamma_pos + c));
        s1 += oe_sum4(u1); t1 += oe_dot4(u1, n1[i]);
        s2 += oe_sum4(u2); t2 += oe_dot4(u2, n2[i]);
        s3 += oe_sum4(u3); t3 += oe_dot4(u3, n3[i]);
      }
    }
    wave_sum3(s1, s2, s3);
    wave_sum3(t1, t2, t3);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        const float4 r = oe_ln_dx(oe_mul(de[i], *(const float4*)(p.gamma_img + c)), n1[i], s1 * inv_h, t1 * inv_h, r1);
        if (dx) *(float4*)(dx + o) = r;
        if (dx16) *(uint2*)(dx16 + o) = make_uint2(pack_bf2(r.x, r.y), pack_bf2(r.z, r.w));
        d2[i] = oe_ln_dx(oe_mul(de[i], *(const float4*)(p.gamma_ang + c)), n2[i], s2 * inv_h, t2 * inv_h, r2);
        d3[i] = oe_ln_dx(oe_mul(de[i], *(const float4*)(p.gamma_pos + c)), n3[i], s3 * inv_h, t3 * inv_h, r3);
      }
    }
  }
  // block sums of the 17 contributions, one vector at a time through LDS (a dead wave contributes zeros), waves in a fixed order
  __shared__ float4 red[OE_NWV][NV * 64];
#pragma unroll
  for (int v = 0; v < OE_V; ++v) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      float4 t;
      if (v == 0) t = oe_mul(dyo[i], no[i]);
      else if (v == 1) t = dyo[i];
      else if (v == 2) t = de[i];
      else if (v == 3) t = oe_mul(de[i], n1[i]);
      else if (v == 4) t = oe_mul(de[i], n2[i]);
      else if (v == 5) t = oe_mul(de[i], n3[i]);
      else if (v == 6) t = d2[i];
      else if (v < 7 + OE_A) t = oe_scale(d2[i], av[v - 7]);
      else if (v == 7 + OE_A) t = d3[i];
      else t = oe_scale(d3[i], pv[v - 8 - OE_A]);
      red[w][i * 64 + lane] = t;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < NV * 64; e += 64 * OE_NWV) {
      const int c = e * 4;
      if (c < H) {
        float4 t = red[0][e];
#pragma unroll
        for (int k = 1; k < OE_NWV; ++k) { const float4 r = red[k][e]; t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w; }
        *(float4*)(ws + ((size_t)blockIdx.x * OE_V + v) * H + c) = t;
      }
    }
    __syncthreads();
  }
}

// ws[nb][17][H] -> the gradients (ADDED to what is there).  block = 64 columns (16 float4 lanes) x 16 partial-row phases.
__global__ __launch_bounds__(256) void obj_embed_reduce_kernel(int nb, int H, const float* __restrict__ ws, hamt_obj_embed_grads g) {
  const int l16 = threadIdx.x & 15, ph = threadIdx.x >> 4;
  const int per = H / 64;                          // blocks per vector
  const int v = blockIdx.x / per, col = (blockIdx.x % per) * 64 + l16 * 4;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b0 = ph; b0 < nb; b0 += 64) {           // 4 independent loads per trip
    float4 q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int b = b0 + 16 * u;
      q[u] = b < nb ? *(const float4*)(ws + ((size_t)b * OE_V + v) * H + col) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { t.x += q[u].x; t.y += q[u].y; t.z += q[u].z; t.w += q[u].w; }
  }
  __shared__ float4 red[16][16];
  red[ph][l16] = t;
  __syncthreads();
  if (ph != 0) return;
  t = red[0][l16];
#pragma unroll
  for (int i = 1; i < 16; ++i) { const float4 r = red[i][l16]; t.x += r.x; t.y += r.y; t.z += r.z; t.w += r.w; }
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
  HAMT_CHECK_ARG(d->H % 64 == 0 && d->H >= 64 && d->H <= 1024, "%s: H=%d unsupported (need H%%64==0, H<=1024)", who, d->H);
  HAMT_CHECK_ARG(d->A == OE_A && d->ld_ang >= OE_A, "%s: angle features %d (ld %d): only 4 is built", who, d->A, d->ld_ang);
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
  const int nv = (d->H + 255) / 256;
  dim3 grid((d->M + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((obj_embed_fwd_kernel<NV>), grid, block, 0, s, *d, *p, x1, ang, pos, y, stats, rng)
  switch (nv) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
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
  const int nv = (d->H + 255) / 256;
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((obj_embed_bwd_kernel<NV>), dim3(nb), dim3(64 * OE_NWV), 0, s, *d, *p, dy, x1, ang, pos, stats, dx, (bf16_t*)dx16, ws, rng)
  switch (nv) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; default: LAUNCH(4); }
#undef LAUNCH
  HAMT_CHECK_LAUNCH("hamt_obj_embed_bwd");
  hipLaunchKernelGGL(obj_embed_reduce_kernel, dim3(OE_V * (d->H / 64)), dim3(256), 0, s, nb, d->H, ws, *g);
  HAMT_CHECK_LAUNCH("hamt_obj_embed_bwd (reduce)");
  return HAMT_OK;
}
