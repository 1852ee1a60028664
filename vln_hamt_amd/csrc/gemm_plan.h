// Which kernel runs a hamt_gemm problem: the whole dispatch policy of gemm.hip / gemm_fast.hip / gemm_q4.hip as ONE pure host function
// (no HIP, no device code, no globals), so that it can be asked -- hamt_gemm_plan -- and tested without a GPU.  The launchers only
// instantiate and launch what the plan names; each family's compiled epilogues are the lists below, which the plan consults and the
// launch switches are generated from.
#pragma once
#include "../../include/hamt.h"
#include <stddef.h>
#include <stdio.h>

constexpr int PLAN_BN = 128, PLAN_BK = 64;    // tile columns / k-tile of the 32 .. 128-row tiles (gemm_frag.h: BN, BK)

// Epilogues (HAMT_EPI_* combinations) each kernel family is compiled for -- compiled per flag set: a dynamic one unrolled 64x overflowed
// the I-cache.  X(E) once per combination.
#define HAMT_EPIS_NARROW(X) X(0) X(HAMT_EPI_BIAS) X(HAMT_EPI_ACCUM)       /* gemm_q4_kernel; gemm_fast_kernel<32>: narrow-output epilogues only */
#define HAMT_EPIS_P8(X) HAMT_EPIS_NARROW(X) X(HAMT_EPI_BIAS | HAMT_EPI_GELU_GRAD) X(HAMT_EPI_MUL_AUX)
#define HAMT_EPIS_P8_FWD(X) /* gemm_p8_kernel<.., B_KM = false, NB = 4> only: forward-only epilogues (the pre-LN ViT blocks: residual add / dropout in the epilogue) */ \
  X(HAMT_EPI_BIAS | HAMT_EPI_ADD_AUX) X(HAMT_EPI_BIAS | HAMT_EPI_ADD_AUX | HAMT_EPI_DROPOUT) X(HAMT_EPI_BIAS | HAMT_EPI_GELU_GRAD | HAMT_EPI_DROPOUT) \
  X(HAMT_EPI_BIAS | HAMT_EPI_GELU) X(HAMT_EPI_BIAS | HAMT_EPI_GELU | HAMT_EPI_DROPOUT)
#define HAMT_EPIS_256(X) HAMT_EPIS_P8(X) /* gemm_fast256_kernel */ \
  X(HAMT_EPI_BIAS | HAMT_EPI_ADD_AUX) X(HAMT_EPI_BIAS | HAMT_EPI_ADD_AUX | HAMT_EPI_DROPOUT) X(HAMT_EPI_BIAS | HAMT_EPI_GELU_GRAD | HAMT_EPI_DROPOUT)
#define HAMT_EPIS_FAST(X) HAMT_EPIS_P8(X) HAMT_EPIS_P8_FWD(X) /* gemm_fast_kernel<64 | 128>; any other combination runs its run-time epilogue, EPI = -1 */ \
  X(HAMT_EPI_BIAS | HAMT_EPI_GELU | HAMT_EPI_SAVE_PRE) X(HAMT_EPI_BIAS | HAMT_EPI_RELU) X(HAMT_EPI_MUL_DGELU)
// (tile rows, K groups, ring depth) gemm_kg_kernel is compiled for; its epilogue is the run-time one
#define HAMT_KG_VARIANTS(X) X(32, 2, 3) X(32, 3, 2) X(32, 2, 4) X(64, 2, 3) X(64, 3, 2) X(128, 2, 2)

#define HAMT_EPI_IS(E) if (e == (E)) return true;
static inline bool gemm_epi_narrow(int e) { HAMT_EPIS_NARROW(HAMT_EPI_IS) return false; }
static inline bool gemm_epi_256(int e) { HAMT_EPIS_256(HAMT_EPI_IS) return false; }
static inline bool gemm_epi_fast(int e) { HAMT_EPIS_FAST(HAMT_EPI_IS) return false; }
static inline bool gemm_epi_p8(int e, bool b_kmajor, int nb) {
  HAMT_EPIS_P8(HAMT_EPI_IS)
  if (!b_kmajor && nb == 4) { HAMT_EPIS_P8_FWD(HAMT_EPI_IS) }
  return false;
}
#undef HAMT_EPI_IS

// The dispatch switches (tuning and tests; gemm.hip reads them from the environment once per process); 0 / -1 = not set.
struct GemmTuning {
  bool no_fast;   // HAMT_NO_FAST (set at all): the generic kernels of gemm.hip for everything
  int fast_bm;    // HAMT_FAST_BM = 32 / 64 / 128 / 256: the plain tile of that height, nothing else
  int ks;         // HAMT_KS: this many K slices wherever split-K can run
  int kg;         // HAMT_KG: 1 = never K groups, any other value = always, the variant 100 * tile rows + 10 * groups + ring depth
  int q4, p8;     // HAMT_Q4 / HAMT_P8 = 0 / 1: never / whenever the kernel can run the problem
  int p8_bn;      // HAMT_P8_BN = 192 / 256: the two-phase tile's columns
};

enum GemmFamily { GEMM_F32, GEMM_BF16 /* the generic kernels of gemm.hip */, GEMM_FAST, GEMM_FAST256, GEMM_P8, GEMM_KG, GEMM_Q4 };

struct GemmPlan {
  GemmFamily family;
  int tile_rows;              // GEMM_FAST: 32 / 64 / 128; GEMM_KG: 32 / 64 / 128
  int p8_nb;                  // GEMM_P8: column blocks of 64 (3 | 4)
  int kg_groups, kg_depth;    // GEMM_KG
  int epi;                    // the EPI template argument the kernel is compiled with (-1: run-time epilogue)
  bool a_kmajor, b_kmajor;
  int ksplit;                 // K slices over the grid (GEMM_FAST only; 1: no split)
};

// name of the plan's kernel as rocprofv3 prints it (hamt_last_kernel)
static inline int gemm_plan_name(const GemmPlan& p, char* buf, size_t n) {
  const char *a = p.a_kmajor ? "true" : "false", *b = p.b_kmajor ? "true" : "false";
  switch (p.family) {
    case GEMM_F32: return snprintf(buf, n, "gemm_f32_kernel<%s, %s>", a, b);
    case GEMM_BF16: return snprintf(buf, n, "gemm_bf16_kernel<%s, %s, ...>", a, b);
    case GEMM_FAST: return snprintf(buf, n, "gemm_fast_kernel<%d, %d, %s, %s>", p.tile_rows, p.epi, a, b);
    case GEMM_FAST256: return snprintf(buf, n, "gemm_fast256_kernel<%d, %s, %s>", p.epi, a, b);
    case GEMM_P8: return snprintf(buf, n, "gemm_p8_kernel<%d, %s, %s, %d>", p.epi, a, b, p.p8_nb);
    case GEMM_KG: return snprintf(buf, n, "gemm_kg_kernel<%d, %d, %d, %s>", p.tile_rows, p.kg_groups, p.kg_depth, b);
    case GEMM_Q4: return snprintf(buf, n, "gemm_q4_kernel<%d, %s>", p.epi, b);
  }
  return -1;
}

// Layouts: NT (forward), NN (dgrad: B = W stored [K][N]), TN (wgrad: A = dY stored [K][M], B = X stored [K][N]).
// K-contiguous operands need K % 64 == 0 (the caller pads with zeros); K-strided operands are clamped to row K-1,
// so for a ragged K the OTHER operand must hold zeros there (NN: zero-padded dY columns; TN: zero-padded dY rows).
// (16-byte aligned operand pointers: hamt_gemm_ws has checked them.)
static inline bool gemm_fast_eligible(const hamt_gemm_desc& d) {
  if (d.prec != HAMT_PREC_BF16 || d.dtype_a != HAMT_BF16 || d.dtype_b != HAMT_BF16) return false;
  if (d.a_kmajor && !d.b_kmajor) return false;
  if (d.K < 64 || d.M < 1 || d.N < 1) return false;
  if (d.K % 64 != 0) return false;     // (TN too: the caller pads the reduction rows of A with zeros)
  if (d.lda % 8 || d.ldb % 8) return false;
  {   // the DMA pieces address their operand with 32-bit byte offsets from its base
    const double a_bytes = 2.0 * (d.a_kmajor ? (double)d.K : (double)d.M) * d.lda, b_bytes = 2.0 * (d.b_kmajor ? (double)d.K : (double)d.N) * d.ldb;
    if (a_bytes >= 4294967296.0 || b_bytes >= 4294967296.0) return false;
  }
  if (d.a_kmajor && d.lda < 64) return false;
  if (d.b_kmajor && d.ldb < 128) return false;
  return true;
}

struct GemmKg { int rows, groups, depth; };   // rows = 0: no K groups

// K groups inside the workgroup (gemm_kg_kernel) instead of plain tiles / split-K: when the whole output is at most one round
// of workgroups of that kernel and the reduction is long enough to amortise the extra LDS pass.  Measured (tools/ksplit_sweep.py,
// B = 16 shapes, us): 1280x768x3072 29.4 -> 16.7, x2304 17.6 -> 14.5, 1968x768x3072 29.9 -> 22.2, x2304 22.9 -> 17.8; no gain once
// the plain tiles fill the chip (B = 64).
static inline GemmKg gemm_kg_variant(const hamt_gemm_desc& d, const GemmTuning& t) {
  if (d.a_kmajor || t.kg == 1) return {0, 0, 0};
  if (t.kg) {     // forced: digits [rows][groups][depth]; whatever is not one of the compiled variants lands on a neighbour
    const int bm = t.kg / 100, G = (t.kg / 10) % 10, D = t.kg % 10;
    if (bm == 32) return G == 2 && D == 3 ? GemmKg{32, 2, 3} : G == 3 ? GemmKg{32, 3, 2} : GemmKg{32, 2, 4};
    if (bm == 128) return {128, 2, 2};
    return G == 2 ? GemmKg{64, 2, 3} : GemmKg{64, 3, 2};
  }
  const int nk = d.K / PLAN_BK;
  if (nk < 12 || d.N > 1024) return {0, 0, 0};
  const long tn = (d.N + 127) / 128, t32 = (long)((d.M + 31) / 32) * tn, t64 = (long)((d.M + 63) / 64) * tn;
  // a VERY long reduction over a small output (the MLM decoder's dgrad: 768 x 768 x 30 528 at B = 64): 144 workgroups walking 477
  // k-tiles each took 157 us in the step (profiles/r04_*); split-K over the grid (10 slices of 128-row tiles, ~360 workgroups, the
  // partial tiles are 24 MB) is the better form there -- when the caller can take it (plain / accumulate epilogue, fp32 C)
  if (nk >= 192 && t64 <= 128 && !(d.epilogue & ~HAMT_EPI_ACCUM) && d.dtype_c == HAMT_F32 && d.ldc == d.N) return {0, 0, 0};
  if (t32 <= 256) return {32, 2, 4};
  if (t64 <= 256 && nk >= 24) return {64, 3, 2};
  // one 128-row tile per CU, two groups (B = 64 text / vision streams: 5120x768x3072 41.2 -> 35.3 us, 2752x768x2304 27.7 -> 24.2)
  const long t128 = (long)((d.M + 127) / 128) * tn;
  if (t128 <= 256 && nk >= 36) return {128, 2, 2};
  return {0, 0, 0};
}

// K slices over the grid given `ws_bytes` of workspace for the fp32 partial tiles (1 = no split)
static inline int gemm_ksplit(const hamt_gemm_desc& d, size_t ws_bytes, const GemmTuning& t) {
  if (d.epilogue & ~HAMT_EPI_ACCUM) return 1;
  if (d.dtype_c != HAMT_F32 || d.ldc != d.N) return 1;
  if (!t.fast_bm && !t.ks && gemm_kg_variant(d, t).rows) return 1;
  const long tiles = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
  const int nk = d.K / PLAN_BK;
  int s;
  if (t.ks) s = t.ks > nk ? nk : t.ks;
  else {
    if (tiles >= 192 || nk < 16) return 1;
    s = (int)(384 / tiles);
    if (s > nk / 8) s = nk / 8;
    if (s > 16) s = 16;
  }
  while (s > 1 && (size_t)s * d.M * d.N * 4 > ws_bytes) --s;
  return s < 2 ? 1 : s;
}

// The kernel hamt_gemm_ws runs `d` on with `ws_bytes` of workspace (0: none).  A family that has no kernel for the epilogue is passed over.
static inline GemmPlan gemm_plan(const hamt_gemm_desc& d, size_t ws_bytes, const GemmTuning& t) {
  GemmPlan p{GEMM_BF16, 0, 0, 0, 0, -1, d.a_kmajor != 0, d.b_kmajor != 0, 1};
  if (t.no_fast || !gemm_fast_eligible(d)) {
    if (d.prec == HAMT_PREC_F32) p.family = GEMM_F32;
    return p;
  }
  const int e = d.epilogue, nk = d.K / PLAN_BK;
  const int ks = p.ksplit = gemm_ksplit(d, ws_bytes, t);
  const long t128 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128), t64 = (long)((d.M + 63) / 64) * ((d.N + 127) / 128);
  const bool one_tile = ks == 1 && !t.fast_bm;      // the families below the plain tiles: never split, never under HAMT_FAST_BM
  // The 128-square tile with the four-deep ring (gemm_q4.hip): narrow outputs whose 128-square tiling is about one round of the chip.
  // The ring takes no fewer than 3 k-tiles (and no split, and K-strided B rows of >= 128: both hold here).
  if (one_tile && t.q4 != 0 && !d.a_kmajor && nk >= 3 && gemm_epi_narrow(e)) {
    // (measured, profiles/r05_q4_probe.txt: equal to the K-group / 64-row tiles on warm operands, 13 - 20 % ahead on cold ones -- the step's
    // case -- at 240 and at 132 tiles; behind them below ~100 tiles, behind the 256-row tiles beyond one round and on N = 1536)
    if (t.q4 == 1 || (d.N <= 1024 && d.K >= 192 && t128 >= 120 && t128 <= 256)) { p.family = GEMM_Q4; p.epi = e; return p; }
  }
  // 256-square two-phase kernel (one 8-wave workgroup per CU): by estimated time.  Measured on MI355X (tools/gemm_sweep.py,
  // tools/p8_probe.py): a p8 tile costs ~6 us + 1.55 us per k-tile whatever the grid, the 64/128-row tiles run the
  // step's shapes at ~620 TFLOP/s.
  if (one_tile && t.p8 != 0 && d.K >= 128 && !d.a_kmajor && (!d.b_kmajor || d.ldb >= 256)) {
    const long t256 = (long)((d.M + 255) / 256) * ((d.N + 255) / 256), t192 = (long)((d.M + 255) / 256) * ((d.N + 191) / 192);
    const double t_p8 = (double)((t256 + 255) / 256) * (6.0 + 1.55 * nk);
    // 256 x 192 tiles: 3/4 of the MFMA work and 7/8 of the operand bytes of a 256-square tile per k-tile -- but measured 0.92-0.94 of
    // its TIME at K = 768 .. 3072 (tools/gemm_bench.py with HAMT_P8_BN = 192 / 256: a tile's life is prologue, barriers and the
    // store tail as much as MFMA issue): worth it only where it does not add a round -- 5120 x 2304 x 768: 180 tiles -> 240, one
    // round either way, 27.6 -> 26.0 us; 11520 x 768 x 3072: 65.2 -> 59.8; 11520 x 768 x 2304 (NN, acc): 55.3 -> 50.9.  The FFN-1
    // epilogue (gelu + gelu', two stores per tile) measured 4 % SLOWER with the narrow tile at 720 tiles: kept on 256 columns there.
    const double t_p8n = (double)((t192 + 255) / 256) * (6.0 + 1.44 * nk);
    const bool n192 = t.p8_bn ? t.p8_bn == 192 : (t_p8n < 0.97 * t_p8 && !((e & HAMT_EPI_GELU_GRAD) && t192 > 512));
    const double t_small = 2.0 * d.M * d.N * d.K / 620e6;
    if (t.p8 == 1 || (n192 ? t_p8n : t_p8) < 0.95 * t_small) {
      const int nb = n192 && gemm_epi_p8(e, p.b_kmajor, 3) ? 3 : 4;
      if (gemm_epi_p8(e, p.b_kmajor, nb)) { p.family = GEMM_P8; p.p8_nb = nb; p.epi = e; return p; }
    }
  }
  if (one_tile) {
    const GemmKg kg = gemm_kg_variant(d, t);
    if (kg.rows) { p.family = GEMM_KG; p.tile_rows = kg.rows; p.kg_groups = kg.groups; p.kg_depth = kg.depth; return p; }
  }
  // 256-square tiles (8 waves, one workgroup per CU, operands re-used twice as often per DMA piece and LDS read): when the
  // reduction is long, the grid is 0.8 .. 1 tile per CU or at least 3 per CU, and the K-strided operand rows are wide enough.
  if (ks == 1 && !d.a_kmajor && !(d.b_kmajor && d.ldb < 256) && gemm_epi_256(e)) {
    const long t256 = (long)((d.M + 255) / 256) * ((d.N + 255) / 256);   // (measured: 5120x3072x768 35.7 us with 128-row tiles, 40 with 256)
    // (K >= 2048: one workgroup per CU exposes the tile's prologue and store tail: long reductions only)
    if (t.fast_bm ? t.fast_bm == 256 : (d.K >= 2048 && ((t256 >= 208 && t256 <= 256) || t256 >= 768))) { p.family = GEMM_FAST256; p.epi = e; return p; }
  }
  // Tile height.  The ring is 2 deep (64 / 48 KiB), so 2 workgroups of 128 rows or 3 of 64 rows share a CU and one's
  // prologue / epilogue / DMA issue overlaps another's MFMA loop (measured: 4096^3 894 TFLOP/s vs 692 with a 3-deep
  // ring at one workgroup per CU).  128-row tiles do ~1.4x the flops per LDS byte, 64-row tiles fill the chip when the
  // grid is small: pick the one with the lower (rounds of resident workgroups) x (time per tile) estimate.
  const long r128 = (t128 * ks + 511) / 512, r64 = (t64 * ks + 767) / 768;
  const bool bm64 = t.fast_bm ? t.fast_bm == 64 : (t128 * ks < 1024 && r64 * 25 < r128 * 36);   // tile-time ratio 1 : 1.44
  // 32-row tiles: for grids so small (the B = 16 shapes: 1280 x 768 outputs are 120 tiles of 64 rows) that 64-row tiles leave every
  // SIMD with at most one wave, which then issues its DMA pieces, reads its fragments and multiplies strictly in turn.  Not for TN,
  // and only for the narrow-output epilogues: 64 rows otherwise.
  const bool bm32 = !d.a_kmajor && (t.fast_bm ? t.fast_bm == 32 : (bm64 && ks == 1 && t64 <= 160 && d.K <= 1024));
  p.family = GEMM_FAST;
  p.tile_rows = bm32 ? (gemm_epi_narrow(e) ? 32 : 64) : bm64 ? 64 : 128;
  p.epi = gemm_epi_fast(e) ? e : -1;
  return p;
}
