// The two-stream visual embedding of gfx950:   e = LN_img(x1) + LN_ang(ang W_ang^T + b_ang)
// where x1 = img W_img^T + b_img is the dense layer's output (bf16 in bf16 mode, what a linear returns under autocast; fp32 in
// fp32 mode).  ONE launch instead of four (the K = 4 angle projection, two LayerNorms, the sum): the angle projection is 4 FMAs
// per element and never exists in memory, the two normalised streams are added in registers, the bf16 image of the sum the
// panorama encoder's first GEMM reads is written alongside.  Backward is one launch + a small reduction: dx1 (the dense layer's
// output gradient, as the padded bf16 image its weight-gradient GEMM reads, or fp32), the angle projection recomputed, and the
// column sums that are the gradients of both LayerNorms' parameters and of the angle projection -- per-block partials, summed
// into the parameters' gradient slots by the second kernel.
//
// Replaces ImageEmbeddings.forward's / HistoryEmbeddings.forward's
//     img_layer_norm(img_linear(img)) + ang_layer_norm(ang_linear(ang))            (vilmodel.py:498-500, 549-551, 557-558;
//                                                                                    finetune vilmodel_cmt.py:575-578, 585-586)
// One 64-lane wave per row, fp32 statistics: the row layout, its arithmetic, the K = 4 projection and the column-sum reduction are
// ln_row.h's; angle_feat_size is 4 everywhere in the reference (r2r_model_config.json / vlnbert_init.py) and the only size built.
#include "ln_row.h"

namespace {

constexpr int VE_A = LN_ANGLE_K;   // angle features
constexpr int VE_V = 4 + VE_A;     // partial vectors per block: dgamma_img, dbeta (both), dgamma_ang, db_ang, dW_ang[:, 0..3]

template <int NV>
__global__ __launch_bounds__(256) void vis_embed_fwd_kernel(hamt_vis_embed_desc d, const void* __restrict__ x1, const float* __restrict__ ang,
                                                            const float* __restrict__ W2, const float* __restrict__ b2,
                                                            const float* __restrict__ g1, const float* __restrict__ be1,
                                                            const float* __restrict__ g2, const float* __restrict__ be2,
                                                            float* __restrict__ y, bf16_t* __restrict__ y16, float* __restrict__ stats) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + w;
  const int H = d.H;
  if (row >= d.M) {
    if (y16) zero_pad_rows(y16, H, row, d.Mpad16, gridDim.x * 4, lane);
    return;
  }
  const int xfmt = d.x_bf16 ? LN_BF16 : LN_F32;
  const float4 av = *(const float4*)(ang + (size_t)row * d.ld_ang);
  float4 v[NV], a[NV];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      v[i] = load_row4(x1, (size_t)row * H + c, xfmt);
      a[i] = angle_proj4(W2, b2, c, av);
      s1 += sum4(v[i]);
      s2 += sum4(a[i]);
    } else { v[i] = zero4(); a[i] = v[i]; }
  }
  wave_sum2(s1, s2);
  const float m1 = s1 / (float)H, m2 = s2 / (float)H;
  float q1 = 0.f, q2 = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i)
    if ((i * 64 + lane) * 4 < H) { q1 += sqdev4(v[i], m1); q2 += sqdev4(a[i], m2); }
  wave_sum2(q1, q2);
  const float r1 = rsqrtf(q1 / (float)H + d.eps1), r2 = rsqrtf(q2 / (float)H + d.eps2);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < H) {
      const size_t o = (size_t)row * H + c;
      float4 r = affine4(norm4(v[i], m1, r1), *(const float4*)(g1 + c), *(const float4*)(be1 + c));
      acc4(r, affine4(norm4(a[i], m2, r2), *(const float4*)(g2 + c), *(const float4*)(be2 + c)));
      *(float4*)(y + o) = r;
      if (y16) store_bf4(y16, o, r);
    }
  }
  if (lane == 0) {
    stats[row] = m1; stats[(size_t)d.M + row] = r1; stats[2 * (size_t)d.M + row] = m2; stats[3 * (size_t)d.M + row] = r2;
  }
}

template <int NV, int NWV>
__global__ __launch_bounds__(64 * NWV) void vis_embed_bwd_kernel(hamt_vis_embed_desc d, const float* __restrict__ dy, const void* __restrict__ x1,
                                                                 const float* __restrict__ ang, const float* __restrict__ W2,
                                                                 const float* __restrict__ b2, const float* __restrict__ g1,
                                                                 const float* __restrict__ g2, const float* __restrict__ stats,
                                                                 float* __restrict__ dx, bf16_t* __restrict__ dx16, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int H = d.H;
  if (dx16 && blockIdx.x == 0) zero_pad_rows(dx16, H, d.M + w, d.Mpad16, NWV, lane);
  const int xfmt = d.x_bf16 ? LN_BF16 : LN_F32;
  float4 acc[VE_V][NV];
#pragma unroll
  for (int v = 0; v < VE_V; ++v)
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[v][i] = zero4();
  for (int row = blockIdx.x * NWV + w; row < d.M; row += gridDim.x * NWV) {
    const float m1 = stats[row], r1 = stats[(size_t)d.M + row], m2 = stats[2 * (size_t)d.M + row], r2 = stats[3 * (size_t)d.M + row];
    const float4 av = *(const float4*)(ang + (size_t)row * d.ld_ang);
    float4 ga[NV], gb[NV], h1[NV], h2[NV];
    float s1 = 0.f, s2 = 0.f, t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        const float4 g = *(const float4*)(dy + o);
        const float4 p = norm4(load_row4(x1, o, xfmt), m1, r1), q = norm4(angle_proj4(W2, b2, c, av), m2, r2);
        fmacc4(acc[0][i], g, p);
        acc4(acc[1][i], g);
        fmacc4(acc[2][i], g, q);
        const float4 u = mul4(g, *(const float4*)(g1 + c)), z = mul4(g, *(const float4*)(g2 + c));
        s1 += sum4(u);
        t1 += dot4(u, p);
        s2 += sum4(z);
        t2 += dot4(z, q);
        ga[i] = u; gb[i] = z; h1[i] = p; h2[i] = q;
      }
    }
    wave_sum2(s1, t1);
    wave_sum2(s2, t2);
    const float c1 = s1 / (float)H, e1 = t1 / (float)H, c2 = s2 / (float)H, e2 = t2 / (float)H;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < H) {
        const size_t o = (size_t)row * H + c;
        const float4 r = ln_dx4(ga[i], h1[i], c1, e1, r1), z = ln_dx4(gb[i], h2[i], c2, e2, r2);
        if (dx) *(float4*)(dx + o) = r;
        if (dx16) store_bf4(dx16, o, r);
        acc4(acc[3][i], z);
        fmacc4(acc[4][i], z, av.x);
        fmacc4(acc[5][i], z, av.y);
        fmacc4(acc[6][i], z, av.z);
        fmacc4(acc[7][i], z, av.w);
      }
    }
  }
#pragma unroll
  for (int v = 0; v < VE_V; ++v) block_partial<NV, NWV>(acc[v], ws, (size_t)blockIdx.x * VE_V + v, H);
}

struct VeOut { float* p[6]; };    // dgamma_img, dbeta_img, dgamma_ang, dbeta_ang, db_ang [H each], dW_ang [H][4]

// ws[nb][VE_V][H] -> the six gradients (ADDED to what is there).  block = 64 columns (16 float4 lanes) x 16 partial-row phases.
__global__ __launch_bounds__(256) void vis_embed_reduce_kernel(int nb, int H, const float* __restrict__ ws, VeOut out) {
  const int per = H / 64;                          // blocks per vector
  const int v = blockIdx.x / per, col = (blockIdx.x % per) * 64 + (threadIdx.x & 15) * 4;
  float4 t;
  if (reduce_partials(ws + (size_t)v * H + col, (size_t)VE_V * H, nb, t)) {
    const float e[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = col + k;
      if (v == 0) out.p[0][c] += e[k];
      else if (v == 1) { if (out.p[1]) out.p[1][c] += e[k]; if (out.p[3]) out.p[3][c] += e[k]; }
      else if (v == 2) out.p[2][c] += e[k];
      else if (v == 3) out.p[4][c] += e[k];
      else out.p[5][(size_t)c * VE_A + (v - 4)] += e[k];
    }
  }
}

void ve_geometry(int M, int* nb) {      // 8-wave blocks, >= 2 rows per wave, <= 256 partials
  int b = (M + 15) / 16;
  *nb = b < 1 ? 1 : (b > 256 ? 256 : b);
}

}  // namespace

size_t hamt_vis_embed_ws_bytes(int M, int H) {     // (hamt_workspace_bytes: HAMT_WS_VIS_EMBED_BWD)
  int nb;
  ve_geometry(M, &nb);
  return (size_t)nb * VE_V * H * 4;
}

extern "C" int hamt_vis_embed_fwd(const hamt_vis_embed_desc* d, const void* x1, const float* ang, const float* w_ang, const float* b_ang,
                                  const float* gamma_img, const float* beta_img, const float* gamma_ang, const float* beta_ang,
                                  float* y, void* y16, float* stats, void* stream) {
  HAMT_CHECK_ARG(d && x1 && ang && w_ang && b_ang && gamma_img && beta_img && gamma_ang && beta_ang && y && stats, "hamt_vis_embed_fwd: null pointer");
  if (int rc = ln_row_check_h(d->H, "hamt_vis_embed_fwd")) return rc;
  if (int rc = ln_row_check_angle(d->A, d->ld_ang, 4, "hamt_vis_embed_fwd")) return rc;
  if (d->M == 0) return HAMT_OK;
  const int rows = (y16 && d->Mpad16 > d->M) ? d->Mpad16 : d->M;
  dim3 grid((rows + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((vis_embed_fwd_kernel<NV>), grid, block, 0, s, *d, x1, ang, w_ang, b_ang, gamma_img, beta_img, gamma_ang, beta_ang, y, (bf16_t*)y16, stats)
  LN_ROW_DISPATCH(d->H, LAUNCH)
#undef LAUNCH
  HAMT_CHECK_LAUNCH("hamt_vis_embed_fwd");
  return HAMT_OK;
}

extern "C" int hamt_vis_embed_bwd(const hamt_vis_embed_desc* d, const float* dy, const void* x1, const float* ang, const float* w_ang,
                                  const float* b_ang, const float* gamma_img, const float* gamma_ang, const float* stats, float* dx, void* dx16,
                                  float* dgamma_img, float* dbeta_img, float* dgamma_ang, float* dbeta_ang, float* db_ang, float* dw_ang,
                                  float* ws, void* stream) {
  HAMT_CHECK_ARG(d && dy && x1 && ang && w_ang && b_ang && gamma_img && gamma_ang && stats && ws, "hamt_vis_embed_bwd: null pointer");
  HAMT_CHECK_ARG(dgamma_img && dgamma_ang && db_ang && dw_ang && (dbeta_img || dbeta_ang), "hamt_vis_embed_bwd: null gradient pointer");
  HAMT_CHECK_ARG(dx || dx16, "hamt_vis_embed_bwd: neither dx nor dx16");
  if (int rc = ln_row_check_h(d->H, "hamt_vis_embed_bwd")) return rc;
  if (int rc = ln_row_check_angle(d->A, d->ld_ang, 4, "hamt_vis_embed_bwd")) return rc;
  if (d->M == 0) return HAMT_OK;
  int nb;
  ve_geometry(d->M, &nb);
  hipStream_t s = (hipStream_t)stream;
#define LAUNCH(NV) hipLaunchKernelGGL((vis_embed_bwd_kernel<NV, 8>), dim3(nb), dim3(512), 0, s, *d, dy, x1, ang, w_ang, b_ang, gamma_img, gamma_ang, stats, dx, (bf16_t*)dx16, ws)
  LN_ROW_DISPATCH(d->H, LAUNCH)
#undef LAUNCH
  HAMT_CHECK_LAUNCH("hamt_vis_embed_bwd");
  VeOut o{{dgamma_img, dbeta_img, dgamma_ang, dbeta_ang, db_ang, dw_ang}};
  hipLaunchKernelGGL(vis_embed_reduce_kernel, dim3(VE_V * (d->H / 64)), dim3(256), 0, s, nb, d->H, ws, o);
  HAMT_CHECK_LAUNCH("hamt_vis_embed_bwd (reduce)");
  return HAMT_OK;
}
