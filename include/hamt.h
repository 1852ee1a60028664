/*
 * hamt.h -- C ABI of libhamt_hip.so: hand-written HIP (gfx950 / MI355X) kernels for the HAMT
 * history-aware multimodal transformer forward/backward.
 *
 * The reference (cshizhe/VLN-HAMT) is pure Python: its "interface" for this path is the torch.nn
 * class surface of pretrain_src/model/{vilmodel,pretrain_cmt}.py.  That surface is re-declared in
 * the vln-hamt_amd/model package; every forward there lowers to the entry points below through ctypes
 * (vln-hamt_amd/_lib.py).  Each entry point names the reference op group it replaces
 * (file:line relative to /root/reference; IDs A1..A24 are SURVEY.md section 8a).
 *
 * Conventions
 *  - plain C: raw device pointers, sizes, a hipStream_t passed as void*; no torch types.
 *  - return 0 on success, negative hamt_status otherwise; hamt_last_error() gives the text
 *    (thread-local).  No C++ exception crosses the boundary.
 *  - asynchronous on the given stream; no allocation, no synchronisation, no global mutable state:
 *    every scratch buffer is passed in by the caller (hipGraph-capture safe).
 *  - row-major tensors; "ld*" are leading dimensions in ELEMENTS; every row must start 16-byte
 *    aligned (ld * sizeof(elem) % 16 == 0).
 *  - dropout is counter based: mask(idx) = hash(rng[0] (seed), rng[1] (epoch), call_id, idx) with
 *    `rng` a DEVICE pointer to two uint64 (so a captured graph draws fresh masks every replay when
 *    the epoch word is bumped) and call_id a host value unique per call site; backward replays the
 *    mask from the same triple, nothing is stored.
 */
#ifndef HAMT_H
#define HAMT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HAMT_ABI_VERSION 2   /* 2 (round 6): hamt_gemm_ln_fwd / hamt_graph_split_* removed (round 5); hamt_embed_sum_bwd takes V and ws_bytes,
                              * hamt_scatter_add_rows_ordered takes T; hamt_wgrad_grouped_ex and the dtype HAMT_F16 added.  Entry points added since (the
                              * policy / nav / obs / eval families, hamt_attn_cls_fwd, hamt_image_resample, hamt_range_audit) change no existing signature and leave the number at 2. */

typedef enum { HAMT_OK = 0, HAMT_ERR_ARG = -1, HAMT_ERR_UNSUPPORTED = -2, HAMT_ERR_LAUNCH = -3 } hamt_status;
typedef enum { HAMT_F32 = 0, HAMT_BF16 = 1,
               /* one byte per element, `aux` of HAMT_EPI_GELU_GRAD (without HAMT_EPI_DROPOUT) / HAMT_EPI_MUL_AUX only: the saved gelu'(x),
                * whose range is [-0.129, 1.129], as code q in [0, 255] with value = 0.005 q - 0.13 (0 and 1 are exact: q = 26 / 226;
                * |error| <= 0.0025, the size of bf16's rounding of values near 1).  Halves the bytes of the image the FFN-1 epilogue
                * writes next to gelu(x) and the FFN-2 dgrad epilogue reads back (vilmodel.py:168-175 BertIntermediate backward). */
               HAMT_U8G = 2,
               /* IEEE half, for `C` of hamt_gemm (epilogue: none / HAMT_EPI_BIAS / HAMT_EPI_ACCUM) and for `x` / `z` of the LayerNorm family only: the output of a dense layer in front of a
                * LayerNorm (vilmodel.py:139-143, 181-185) kept in two bytes with 10 mantissa bits instead of bf16's 7 -- the rounding of
                * that interface is 8 x finer at the same HBM bytes (round 6: the bf16 head outputs at B = 64 drop from 1.03e-2 to
                * ~6.5e-3 of the fp32 reference).  The store clamps at +-65504 instead of writing inf.  With the random weights of the tests
                * and the benchmark the dense outputs are O(1 .. 100), far inside half's range; a trained checkpoint with outlier channels
                * need not be, and a clamped value is a silently wrong LayerNorm row -- hamt_range_audit counts the elements at the limit
                * per dense layer, and the Python side (audit.HalfRangeWatch) reports them and moves single layers to HAMT_F32 outputs */
               HAMT_F16 = 3 } hamt_dtype;
/* arithmetic of the contraction: bf16 MFMA operands with fp32 accumulate, or exact fp32 MFMA */
typedef enum { HAMT_PREC_BF16 = 0, HAMT_PREC_F32 = 1 } hamt_prec;

int hamt_version(void);
/* copies the calling thread's last error text into buf (NUL terminated); returns its length */
int hamt_last_error(char* buf, size_t n);
/* name (as rocprofv3 prints it, template arguments included) of the kernel the calling thread's most recent hamt_gemm /
 * hamt_gemm_ws call launched for its contraction -- lets a profiler attribute recorded calls to kernel-trace rows.  A bf16-path
 * attention backward (hamt_attn_small_bwd, hamt_attn_varlen_bwd, hamt_attn_varlen_cross_bwd) leaves its kernel here too, by family:
 * attn_s128_bwd_kernel, attn_wide_bwd_kernel, attn_wide_bwd_kernel<packed> (a packed call with a side above 128), attn16_bwd_kernel. */
int hamt_last_kernel(char* buf, size_t n);
/* Caller-provided scratch sizes (the library never allocates).  shape[] by op:
 *   HAMT_WS_GEMM_SPLITK  {M, N, K}  bytes hamt_gemm_ws can use for its deterministic split-K (0: it will not split)
 *   HAMT_WS_COLSUM       {M, N}     hamt_colsum `ws`
 *   HAMT_WS_SUMSQ        {}         hamt_sumsq `ws`
 *   HAMT_WS_LN_BWD       {M, H}     hamt_ln_bwd / hamt_ln_bwd_add `ws`
 *   HAMT_WS_WGRAD_TABLE  {M_0, M_1, ...}  (output rows of every problem) hamt_wgrad_grouped `table`
 *   HAMT_WS_LNRED_TABLE  {n}        hamt_ln_bwd_reduce_grouped `table`
 *   HAMT_WS_VIS_EMBED_BWD {M, H}    hamt_vis_embed_bwd `ws`
 *   HAMT_WS_EMBED_BWD     {R, H}    hamt_embed_sum_bwd `ws`
 *   HAMT_WS_OBJ_EMBED_BWD {M, H}    hamt_obj_embed_bwd `ws`
 *   HAMT_WS_IMAGE_PREP    {n}       hamt_image_prep `ws`
 * returns the size in bytes, or 0 for an unknown op / malformed shape */
enum { HAMT_WS_GEMM_SPLITK = 0, HAMT_WS_COLSUM = 1, HAMT_WS_SUMSQ = 2, HAMT_WS_LN_BWD = 3, HAMT_WS_WGRAD_TABLE = 4, HAMT_WS_LNRED_TABLE = 5, HAMT_WS_VIS_EMBED_BWD = 6,
       HAMT_WS_EMBED_BWD = 7 /* {R, H}: hamt_embed_sum_bwd `ws` = max(HAMT_WS_COLSUM {R, H}, 136 R bytes) */,
       HAMT_WS_OBJ_EMBED_BWD = 8, HAMT_WS_IMAGE_PREP = 9 /* {n}: hamt_image_prep `ws` */ };
size_t hamt_workspace_bytes(int op, const int* shape, int nshape);

/* ------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( A[M,K] * B[K,N] )            (all nn.Linear calls of A2-A5, A7, A10, A11,
 * A15-A20 forward; their dgrad dX = dY*W and wgrad dW = dY^T*X backward)
 *   a_kmajor = 0: A stored [M][K] (K contiguous)      1: A stored [K][M] (M contiguous)
 *   b_kmajor = 0: B stored [N][K] (nn.Linear weight)  1: B stored [K][N]
 *   forward  y = x W^T      : a_kmajor 0, b_kmajor 0      (vilmodel.py:97-99, 140, 169, 182 ...)
 *   dgrad    dx = dy W      : a_kmajor 0, b_kmajor 1
 *   wgrad    dW = dy^T x    : a_kmajor 1, b_kmajor 1
 * epilogue flags (applied in this order): v = alpha*acc; +bias[n]; store pre-activation to aux
 * (HAMT_EPI_SAVE_PRE); GELU(erf) or ReLU; multiply by gelu'(aux[m,n]) / relu'(aux[m,n])
 * (HAMT_EPI_MUL_DGELU / _DRELU: fused activation backward for dgrad); C += v (HAMT_EPI_ACCUM).
 * ---------------------------------------------------------------------------------------------- */
enum {
  HAMT_EPI_BIAS = 1, HAMT_EPI_GELU = 2, HAMT_EPI_RELU = 4, HAMT_EPI_ACCUM = 8,
  HAMT_EPI_MUL_DGELU = 16, HAMT_EPI_MUL_DRELU = 32, HAMT_EPI_SAVE_PRE = 64,
  /* bf16 training path: forward stores gelu(v) to C and gelu'(v) to aux in ONE erf/exp evaluation (A&S 7.1.26 erf,
   * |err| <= 1.5e-7, far below bf16 resolution); backward just multiplies by aux. */
  HAMT_EPI_GELU_GRAD = 128, HAMT_EPI_MUL_AUX = 256,
  /* C = epi(...) + aux  (residual add of the pre-LN ViT blocks, vision_transformer.py:196-197; aux fp32 or bf16 [M][ldaux]) */
  HAMT_EPI_ADD_AUX = 512,
  /* v = dropout(v) after the activation and before ADD_AUX (the proj_drop / Mlp.drop of the ViT blocks, vision_transformer.py:
   * 148-150, 176-177): keep factor of element (m, n) = drop_mask(rng, call_id, m, n >> 2)[n & 3], the same mask
   * hamt_cast_pad_bf16_dropout applies in backward.  With GELU_GRAD the stored gelu' is masked too (so backward's
   * MUL_AUX needs no second mask).  bf16 fast path only (bf16 operands, K % 64 == 0); anything else is an error. */
  HAMT_EPI_DROPOUT = 1024
};
typedef struct {
  int M, N, K;
  int lda, ldb, ldc, ldaux;
  int a_kmajor, b_kmajor;
  int dtype_a, dtype_b, dtype_c, dtype_aux; /* hamt_dtype */
  int prec;                                 /* hamt_prec  */
  int epilogue;                             /* HAMT_EPI_* */
  float alpha;
  int ka_rows, kb_rows; /* K-strided operands only: number of valid reduction rows actually stored in A / B when K was
                           rounded up for the other operand (0 = K).  Rows beyond are never dereferenced. */
  float p_drop;         /* HAMT_EPI_DROPOUT only */
  uint32_t call_id;
  const uint64_t* rng;  /* DEVICE pointer: {seed, epoch} */
} hamt_gemm_desc;
int hamt_gemm(const hamt_gemm_desc* d, const void* A, const void* B, void* C, const float* bias,
              void* aux, void* stream);
/* Same, with a caller-provided fp32 workspace that enables deterministic split-K for small outputs with a long
 * reduction (weight gradients: dW[768,768] = dY^T X over K = B*L rows).  hamt_gemm_ksplit() tells how many K
 * slices S the kernel would use for `d`; pass ws_bytes >= S*M*N*4 (less => fewer slices; NULL => no split).
 * A problem splits only with the plain or the HAMT_EPI_ACCUM epilogue into a dense fp32 C (ldc == N).  Slice s stores
 * alpha * (its part of the reduction) as an [M][N] fp32 tile at ws + s*M*N -- alpha is applied there, once per slice --
 * and a second kernel adds the S tiles in a fixed order (+ C under HAMT_EPI_ACCUM): slice order 0, 1, 2, ... when
 * M*N % 4 == 0 and ws and C are 16-byte aligned, otherwise four interleaved runs (s = 0, 4, ..; 1, 5, ..; ..) summed as
 * (r0 + r1) + (r2 + r3).  Deterministic; after the call the first S*M*N floats of ws hold those tiles, and nothing
 * behind them is written.
 * (hamt_workspace_bytes(HAMT_WS_GEMM_SPLITK) describes the NT problem {M, N, K} (both operands K-contiguous) only: it
 * answers 0 for weight-gradient (a_kmajor) shapes that do split.  Size the workspace from hamt_gemm_ksplit, as ops.gemm does.) */
int hamt_gemm_ksplit(const hamt_gemm_desc* d);
int hamt_gemm_ws(const hamt_gemm_desc* d, const void* A, const void* B, void* C, const float* bias,
                 void* aux, void* ws, size_t ws_bytes, void* stream);
/* K slices (>= 1) that hamt_gemm_ws would use for `d` with ws_bytes of workspace, and in `name` (n bytes) the kernel it would
 * launch, as hamt_last_kernel reports it; launches nothing, touches no device state.  Negative: bad argument. */
int hamt_gemm_plan(const hamt_gemm_desc* d, size_t ws_bytes, char* name, size_t n);

/* operand preparation for the bf16 fast path (both GEMM operands bf16, K-contiguous, K % 64 == 0):
 *   cast_pad_bf16:   y[Rpad][Cpad] (bf16) = x[R][C] (fp32), rows >= R and columns >= C zero filled
 *   cast_transpose:  y[C][Rpad] (bf16) = x[R][C]^T (fp32 or bf16 source), rows >= R zero filled
 * (dgrad uses the transposed weight, wgrad the transposed activations / gradients.) */
int hamt_cast_pad_bf16(int R, int C, int Rpad, int Cpad, const float* x, int ldx, void* y, int ldy, void* stream);
int hamt_cast_transpose(int R, int C, const void* x, int ldx, int dtype_x, void* y, int ldy, int Rpad, void* stream);
/* y[Rpad][C] (bf16) = x[R][C] (fp32) * keep(m, n) with the mask of a HAMT_EPI_DROPOUT GEMM of the same (rng, call_id):
 * the gradient of the dropped branch, ready as dgrad / wgrad operand.  C % 8 == 0; rows >= R zero filled. */
int hamt_cast_pad_bf16_dropout(int R, int C, int Rpad, const float* x, int ldx, void* y, int ldy, float p, uint32_t call_id,
                               const uint64_t* rng, void* stream);

/* dW[n][k] (+)= sum_m dy[m][n] * x[m][k] for K <= 8 (weight gradient of the 4-wide angle-feature linears, vilmodel.py:498,
 * 550, 558): exact fp32, K weighted column sums.  ws: >= 64*N*K floats */
int hamt_smallk_wgrad(int M, int N, int K, const float* dy, int lddy, const float* x, int ldx, float* dW,
                      int accumulate, float* ws, void* stream);

/* Grouped weight gradients: n independent problems in as few launches as the kernarg table allows,
 *     dW_p[M_p][N_p] (+)= dY_p^T X_p      and, when db != NULL,      db_p[M_p] (+)= column sums of dY_p,
 * with dY_p bf16 [K_p][ldy] (its M_p columns = the layer's output features) and X_p bf16 [K_p][ldx] (the layer's input
 * image), both exactly as the forward / dgrad GEMMs left them (K_p = rows padded to a multiple of 64; the padding rows are
 * zero, or of any content when K_valid names the valid rows).
 * Problems are packed into one launch per tile class (256-square tiles when the operand rows allow, else 128 / 64 rows).
 * This is what torch.autograd does one nn.Linear at a time in the reference (vilmodel.py: every nn.Linear backward);
 * weight gradients are not on the backward critical path, so the host queues them and hands the whole list over once per
 * backward pass: 768x768 outputs that alone fill 36 CUs become one chip-filling grid without split-K.
 * `probs` is a HOST array.  Requirements per problem: K % 64 == 0, ldy % 8 == 0 && ldy >= 64, ldx % 8 == 0 && ldx >= 128,
 * dy / x 16-byte aligned.  Deterministic (fixed summation order per output element). */
typedef struct {
  const void* dy;
  const void* x;
  float* dw;
  float* db; /* may be NULL */
  int M, N, K, ldy, ldx, ldw;
  int accum_dw, accum_db; /* 0: store, 1: += */
  float* ss; /* may be NULL.  ceil(M / 64) * ceil(N / 128) floats, ZERO on entry: every output tile stores the sum of squares of the
              * values it wrote (after accumulation) into the slot of its origin [row / 64][column / 128] -- a tile of any size
              * owns exactly one of these slots, the others stay zero -- so that sum(ss) = ||dW||^2 without reading dW back
              * (the global-norm clip of the step: hamt_sumsq_partials + hamt_sumsq_table over the remaining parameters).
              * Only meaningful for a dW written ONCE in the call sequence (a second, accumulating problem on the same dW
              * must use the same tiling to overwrite the same slots: pass NULL for both and reduce that parameter from memory) */
  int K_valid; /* 0 or K: every reduction row counts.  Else rows [K_valid, K) of dy and x are PADDING of any content
                * (uninitialised memory included): they are neither read (the loads re-read row K_valid - 1) nor multiplied */
  float wire_scale; /* 0: dW is stored as fp32 (the default).  != 0: `dw` points to a BF16 array of the same shape / ldw and the
                     * tile stores bf16(wire_scale * dW) -- the value a data-parallel gradient exchange puts on the wire (the stock DDP
                     * bf16_compress_hook's: divide by the world size, round to bf16), written straight from the accumulators instead
                     * of an fp32 store followed by a pack pass over the arena.  Store only (accum_dw must be 0), `ss` is ignored. */
  /* Optional SECOND pair of operands reduced into the same dW / db in the same launch: dW (+)= dy^T x + dy2^T x2 (a parameter used
   * twice in a pass -- the cross-attention weights LXRTXLayer shares between its two directions, vilmodel.py:401-412 -- as ONE problem
   * instead of a second, accumulating launch behind the first).  dy2 == NULL: none.  Same requirements as dy / x (K2 % 64 == 0, ...);
   * K_valid must be 0 or K (no ragged tail between the two reductions), K2_valid as K_valid; wire_scale must be 0. */
  const void* dy2;
  const void* x2;
  int K2, ldy2, ldx2, K2_valid;
} hamt_wgrad_desc;
/* `table`: caller-provided DEVICE scratch (16-byte aligned) that holds the launch table: HAMT_WGRAD_TABLE_ENTRY bytes per
 * entry, at most sum over the problems of ceil(M_p / 64) entries (large problems are cut into bands of tile rows); it is filled by small kernels from kernarg data, so `probs` need not outlive the call and the whole sequence can
 * be captured in a hipGraph.  The table must stay untouched until the launches have run.  Every requirement, the table's size
 * included, is checked on the host before the first launch: a refused call has written nothing (tests/test_gpu_wgrad.py). */
#define HAMT_WGRAD_TABLE_ENTRY 112
int hamt_wgrad_grouped(int n, const hamt_wgrad_desc* probs, void* table, size_t table_bytes, void* stream);
/* The same in two phases, for callers that replay a FIXED set of problems (a captured training step): phase 1 writes the launch table
 * (once: its content is a function of `probs` only), phase 2 launches the grouped kernels from a table a phase-1 call with the same
 * `probs` has written, phase 3 = both = hamt_wgrad_grouped.  A replayed phase-2 launch has no one-workgroup table-write kernel in front
 * of it: on a second stream such a kernel waited ~275 us behind the first stream's chip-filling tiles before it was dispatched. */
int hamt_wgrad_grouped_ex(int n, const hamt_wgrad_desc* probs, void* table, size_t table_bytes, int phase, void* stream);

/* column sums  out[n] (+)= sum_m x[m,n]   (bias gradients of every nn.Linear).  ws: >= 64*N floats */
int hamt_colsum(int M, int N, const void* x, int ldx, int dtype_x, float* out, int accumulate,
                float* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * attn_small: multi-head softmax attention for short sequences (A2 core vilmodel.py:101-126,
 * A7 core vilmodel.py:327-348): S = Q K^T * scale + mask[b, key]; P = softmax(S); P = dropout(P);
 * O = P V, heads split/merged by pointer arithmetic (head h = columns [h*64, h*64+64)).
 * Q rows (b*Sq + i) at q + row*ldq, K/V rows (b*Sk + j); mask is the reference's additive
 * (1-m)*-10000 row, fp32 [B, Sk] (may be NULL).  d_head must be 64.  lse[B,heads,Sq] (fp32) is
 * saved for backward.  Backward recomputes P (flash style) and needs delta = rowsum(dO*O)
 * computed by hamt_attn_small_bwd itself into `delta` ([B,heads,Sq] fp32 scratch).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int B, heads, Sq, Sk, d_head;
  int ldq, ldk, ldv, ldo;
  int dtype_qkv, dtype_o; /* hamt_dtype */
  float scale, p_drop;
  uint32_t call_id;
  int prec; /* hamt_prec: HAMT_PREC_BF16 = bf16 MFMA products with fp32 softmax; HAMT_PREC_F32 = exact fp32 MFMA */
} hamt_attn_desc;
int hamt_attn_small_fwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v,
                        const float* add_mask, void* o, float* lse, const uint64_t* rng, void* stream);
/* dq/dk/dv have the layout (ld, dtype) of q/k/v; do has the layout of o */
int hamt_attn_small_bwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v,
                        const float* add_mask, const void* o, const void* d_o, const float* lse,
                        float* delta, void* dq, void* dk, void* dv, const uint64_t* rng, void* stream);

/* attn_cls (csrc/attn_cls.hip): the same attention for ONE query per (image, head) -- the cls row of a ViT's last block in a forward-only
 * pass that reads nothing but x[:, 0] afterwards (vision_transformer.py:346).  d->B images, d->Sq must be 1, d->Sk <= 256 keys per image
 * (more: HAMT_ERR_UNSUPPORTED, nothing is launched), d_head 64, p_drop 0, no mask.  q row b at q + b*ldq, K / V rows (b*Sk + j), o row b at
 * o + b*ldo ([B, heads*64]); q / k / v share dtype_qkv (fp32 or bf16), o has dtype_o; every base pointer and row 16-byte aligned.
 * o = softmax(q k^T * scale) v with scores, softmax and the P V sums in fp32, whatever d->prec says.  One wave per (image, head), two
 * streaming passes over K and V; no atomics, no scratch, no lse (there is no backward). */
int hamt_attn_cls_fwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, void* o, void* stream);

/* Packed ("varlen") self-attention, bf16 path: the B sequences lie back to back, sample b owns rows [cu_seqlens[b], cu_seqlens[b + 1])
 * of q / k / v / o / d_o / dq / dk / dv (row strides as in the descriptor), at most d->Sq = d->Sk <= 256 tokens each, every key real (no
 * mask); lse is [B, heads, d->Sq].  = hamt_attn_small_* on the real tokens of a padded batch (vilmodel.py:96-129) without computing
 * the padded rows; a sequence of length 0 is skipped. */
int hamt_attn_varlen_fwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, const int* cu_seqlens,
                         void* o, float* lse, const uint64_t* rng, void* stream);
int hamt_attn_varlen_bwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, const int* cu_seqlens,
                         const void* o, const void* d_o, const float* lse, void* dq, void* dk, void* dv,
                         const uint64_t* rng, void* stream);
/* Cross attention with ONE side packed (BertXAttention, vilmodel.py:351-360, in the x-layers of a ragged batch: the instruction tokens
 * lie back to back, the visual stream keeps its fixed stride).  Exactly one of cu_q / cu_k is given.
 *   cu_q: query sequence b = rows [cu_q[b], cu_q[b + 1]) of q / o / d_o / dq (<= d->Sq rows), its keys = rows [b * Sk, (b + 1) * Sk)
 *         of k / v under add_mask [B, Sk] (may be NULL).  Query sequences b >= n_pairs -- the filler sequences that round a packed
 *         row count up to its bucket -- have no keys: o = 0, dq = 0, nothing added to dk / dv.
 *   cu_k: queries at the fixed stride d->Sq, sample b's keys = rows [cu_k[b], cu_k[b + 1]) of k / v / dk / dv (<= d->Sk, all real:
 *         add_mask is ignored); n_pairs = d->B.  Key rows no sample owns are not written: zero dk / dv behind the last real row.
 * `pair` (optional device array [B]; NULL = "b pairs with b, fillers behind n_pairs"): the key side of query sequence b -- the key sample
 * (cu_q form: rows [pair[b] * Sk, ...) and row pair[b] of add_mask) or the entry of cu_k (cu_k form); negative = a filler.  Every key
 * side must be named by at most one query sequence (dk / dv are stored, not accumulated).  For packed copies of a batch whose fillers lie
 * between the copies (forward_itm's replicated text, vilmodel.py:672-676).
 * lse is [B, heads, d->Sq] in both forms.  d->Sq, d->Sk <= 256 (more: HAMT_ERR_ARG, nothing is launched). */
int hamt_attn_varlen_cross_fwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, const int* cu_q,
                               const int* cu_k, int n_pairs, const int* pair, const float* add_mask, void* o, float* lse,
                               const uint64_t* rng, void* stream);
int hamt_attn_varlen_cross_bwd(const hamt_attn_desc* d, const void* q, const void* k, const void* v, const int* cu_q,
                               const int* cu_k, int n_pairs, const int* pair, const float* add_mask, const void* o, const void* d_o,
                               const float* lse, void* dq, void* dk, void* dv, const uint64_t* rng, void* stream);

/* ------------------------------------------------------------------------------------------------
 * vis_embed: the two-stream visual embedding   e = LN_img(x1) + LN_ang(ang W_ang^T + b_ang)
 *   ImageEmbeddings / HistoryEmbeddings (A10, A11): img_layer_norm(img_linear(img)) + ang_layer_norm(ang_linear(ang))
 *   (vilmodel.py:498-500, 549-551, 557-558; finetune vilmodel_cmt.py:575-578, 585-586); x1 [M, H] = img_linear's output
 *   (bf16 or fp32), ang [M, 4] fp32 with row stride ld_ang, w_ang [H, 4] / b_ang [H] = ang_linear's parameters.
 * fwd: y [M, H] fp32, y16 (optional) its bf16 image [Mpad16, H] (rows [M, Mpad16) zero), stats [4][M] = mean / rstd of the image
 *   stream, mean / rstd of the angle stream (for backward).
 * bwd: dy [M, H] -> dx = d(x1) as fp32 [M, H] and / or dx16 = its bf16 image [Mpad16, H] (the operand of img_linear's weight
 *   gradient; rows [M, Mpad16) zero); the gradients of both LayerNorms' gamma / beta, of b_ang and of w_ang are ADDED to the
 *   six output vectors (dbeta_img or dbeta_ang may be NULL).  ws: HAMT_WS_VIS_EMBED_BWD {M, H} bytes of scratch.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int M, H;
  int A;      /* angle features: 4 (the only size the reference uses and the only one built) */
  int ld_ang; /* row stride of ang, in floats (a multiple of 4) */
  float eps1, eps2;
  int x_bf16; /* x1 is bf16 (else fp32) */
  int Mpad16; /* rows of the optional bf16 images y16 / dx16 (0: none beyond M) */
} hamt_vis_embed_desc;
int hamt_vis_embed_fwd(const hamt_vis_embed_desc* d, const void* x1, const float* ang, const float* w_ang, const float* b_ang,
                       const float* gamma_img, const float* beta_img, const float* gamma_ang, const float* beta_ang,
                       float* y, void* y16, float* stats, void* stream);
int hamt_vis_embed_bwd(const hamt_vis_embed_desc* d, const float* dy, const void* x1, const float* ang, const float* w_ang,
                       const float* b_ang, const float* gamma_img, const float* gamma_ang, const float* stats, float* dx, void* dx16,
                       float* dgamma_img, float* dbeta_img, float* dgamma_ang, float* dbeta_ang, float* db_ang, float* dw_ang,
                       float* ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * obj_embed: REVERIE's object embedding (finetune reverie/vlnbert_navref.py:31-42), per object row
 *     y = dropout( LN_out( LN_img(x1) + LN_ang(ang W_ang^T + b_ang) + LN_pos(pos W_pos^T + b_pos) + nav + tt ) )
 *   x1 [M, H] = img_linear's output (bf16 or fp32); ang [M, 4] / pos [M, 5] fp32 with row strides ld_ang / ld_pos (any; read
 *   element by element); w_ang [H, 4], w_pos [H, 5] (nn.Linear layout); tt / nav = ONE row each (token_type_embeddings row 1,
 *   nav_type_embedding row 2), added to every object.  Every parameter pointer 16-byte aligned.  Dropout (p_drop) after the
 *   output LayerNorm uses the counter-based mask of hamt_ln_fwd's p_post under (rng, call_id); nothing is stored.
 * fwd: y [M, H] fp32; stats [8][M] = mean / rstd of the image, angle, position and output LayerNorms (for backward).
 * bwd: dy [M, H] -> dx = d(x1) as fp32 [M, H] and / or dx16 = its bf16 image [Mpad16, H] (rows [M, Mpad16) zero); the branch
 *   activations are recomputed from x1 / ang / pos.  Every parameter gradient is ADDED to its destination in `g` (a NULL
 *   destination is skipped); dtt and dnav (the two constant rows) both receive the column sum of d(LN_out input).  Per-block
 *   partials in ws (HAMT_WS_OBJ_EMBED_BWD {M, H} bytes) are summed in a fixed order: bit-reproducible, no atomics.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int M, H;
  int A;      /* angle features: 4 (the only size built) */
  int ld_ang; /* row stride of ang, in floats */
  int P;      /* position features: 5 (the only size built) */
  int ld_pos; /* row stride of pos, in floats */
  float eps_img, eps_ang, eps_pos, eps_out;
  float p_drop;
  uint32_t call_id;
  int x_bf16; /* x1 is bf16 (else fp32) */
  int Mpad16; /* rows of the optional bf16 image dx16 (0: none beyond M) */
} hamt_obj_embed_desc;
typedef struct {
  const float *w_ang, *b_ang, *w_pos, *b_pos;
  const float *gamma_img, *beta_img, *gamma_ang, *beta_ang, *gamma_pos, *beta_pos;
  const float *tt, *nav, *gamma_out, *beta_out;
} hamt_obj_embed_params;
typedef struct {
  float *dw_ang, *db_ang, *dw_pos, *db_pos;
  float *dgamma_img, *dbeta_img, *dgamma_ang, *dbeta_ang, *dgamma_pos, *dbeta_pos;
  float *dtt, *dnav, *dgamma_out, *dbeta_out;
} hamt_obj_embed_grads;
int hamt_obj_embed_fwd(const hamt_obj_embed_desc* d, const hamt_obj_embed_params* p, const void* x1, const float* ang, const float* pos,
                       float* y, float* stats, const uint64_t* rng, void* stream);
int hamt_obj_embed_bwd(const hamt_obj_embed_desc* d, const hamt_obj_embed_params* p, const hamt_obj_embed_grads* g, const float* dy,
                       const void* x1, const float* ang, const float* pos, const float* stats, float* dx, void* dx16, float* ws,
                       const uint64_t* rng, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ln: y = dropout_post( LayerNorm( dropout_pre(x) + residual ) )      fp32 statistics
 *   BertSelfOutput / BertOutput (A3/A5, vilmodel.py:139-143, 181-185): p_pre = p, residual, p_post = 0
 *   BertEmbeddings / Image / History embeddings (A1, A10, A11):        p_pre = 0, p_post = p
 *   prediction heads (pretrain_cmt.py:13-71): LN followed by Dropout:  p_post = p
 * z (the pre-LN sum) is written for backward (may alias x).  y16 (bf16 copy of y) optional.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int M, H;
  float eps, p_pre, p_post;
  uint32_t call_id;
  int Mpad16; /* rows of the optional bf16 images (y16 / dx16); rows [M, Mpad16) are written as zeros (0: no padding) */
  int io16;   /* HAMT_LN_X_BF16: `x` is bf16 (the dense layer in front wrote bf16, as a linear does under autocast);
               * HAMT_LN_Z_BF16: the saved pre-LN sum `z` is stored / read as bf16 (backward re-normalises it with the exact
               * fp32 mean / rstd).  HAMT_LN_X_F16 / HAMT_LN_Z_F16: the same two as IEEE half (HAMT_F16: same bytes, a rounding 8 x finer).
               * 0: both fp32.  At most one flag per tensor. */
} hamt_ln_desc;
#define HAMT_LN_X_BF16 1
#define HAMT_LN_Z_BF16 2
#define HAMT_LN_X_F16 4
#define HAMT_LN_Z_F16 8
int hamt_ln_fwd(const hamt_ln_desc* d, const void* x, const float* residual, const float* gamma,
                const float* beta, void* z, float* y, void* y16, float* mean, float* rstd,
                const uint64_t* rng, void* stream);
/* dz = d(pre-LN sum) (also the residual gradient); dx = dropout_pre-masked dz (may be NULL); dx16 (optional) = the same
 * as bf16 [Mpad16, H] -- the operand of the dgrad/wgrad GEMMs of the dense layer that produced x; dxsum (optional) +=
 * column sums of dx = that layer's bias gradient; dgamma/dbeta/dxsum are STORED (overwritten).  ws: HAMT_WS_LN_BWD {M, H} bytes
 * (3 H floats per block of the kernel, at most 256 blocks). */
int hamt_ln_bwd(const hamt_ln_desc* d, const float* dy, const void* z, const float* mean,
                const float* rstd, const float* gamma, float* dz, float* dx, void* dx16, float* dgamma,
                float* dbeta, float* dxsum, float* ws, const uint64_t* rng, void* stream);
/* pre-LN blocks (x + f(LN(x)), vision_transformer.py:196-197): dz = LayerNorm-backward(dy) + add, where `add` is the
 * gradient that reaches x through the residual path -- one pass instead of a LayerNorm backward and an add. */
int hamt_ln_bwd_add(const hamt_ln_desc* d, const float* dy, const void* z, const float* mean, const float* rstd,
                    const float* gamma, const float* add, float* dz, float* dgamma, float* dbeta, float* ws,
                    void* stream);
/* The second half of hamt_ln_bwd / hamt_ln_bwd_add on its own: sums the per-block partials a call with
 * dgamma == dbeta == dxsum == NULL left in `ws` (same M, H) into dgamma / dbeta / dxsum (stored; any may be NULL).  The
 * parameter gradients are not on the backward critical path, so the host runs this on an auxiliary stream. */
int hamt_ln_bwd_reduce(int M, int H, const float* ws, float* dgamma, float* dbeta, float* dxsum, void* stream);
/* The same for n calls at once (the end-of-backward form: one launch instead of one per LayerNorm; H % 64 == 0, pointers
 * 16-byte aligned).  `descs` is a HOST array; `table`: DEVICE scratch of >= n * HAMT_LNRED_TABLE_ENTRY bytes, filled by
 * small kernels from kernarg data (capturable; `descs` need not outlive the call). */
typedef struct {
  const float* ws;
  float* dgamma; /* each may be NULL */
  float* dbeta;
  float* dxsum;
  int M, H;
  int atomic; /* bit 0 / 1 / 2: dgamma / dbeta / dxsum is atomically ADDED to instead of stored (several LayerNorm calls sharing
               * one parameter's zero-initialised gradient slot: no separate accumulation pass) */
} hamt_ln_reduce_desc;
#define HAMT_LNRED_TABLE_ENTRY 48
int hamt_ln_bwd_reduce_grouped(int n, const hamt_ln_reduce_desc* descs, void* table, size_t table_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * gather/scatter family (embedding lookups A1/A10/A11, boolean-mask compaction A15/A19
 * pretrain_cmt.py:161-165, SPREL anchor gather A18 pretrain_cmt.py:211-214, cat/slice A9/A12)
 *   gather_rows:  out[r, col0:col0+W] = (base ? base[r, col0:col0+W] : 0) + src[idx[r], :W]   idx int64, r < R
 *   scatter_add:  dst[idx[r], :W] += src[r, col0:col0+W]   (atomic; duplicate indices allowed)
 * idx == NULL means identity (row copy between strided buffers); out may alias base.
 * ---------------------------------------------------------------------------------------------- */
int hamt_gather_rows(int R, int W, const float* src, int ld_src, const int64_t* idx, const float* base,
                     int ld_base, float* out, int ld_out, int col0, void* stream);
int hamt_scatter_add_rows(int R, int W, const float* src, int ld_src, int col0, const int64_t* idx,
                          float* dst, int ld_dst, void* stream);
/* scatter_add in a FIXED summation order (colliding rows are added in row order by one writer per table row: bit-reproducible, unlike the
 * atomic form); idx must be given; T = rows of the table (< 2^31): source rows whose index is outside [0, T) are skipped.  ws: 34 R ints of device
 * scratch.  Beyond 262 144 source rows (the ranking is quadratic) it falls back to the atomic kernel and says so on stderr, once. */
int hamt_scatter_add_rows_ordered(int R, int W, const float* src, int ld_src, int col0, const int64_t* idx,
                                  float* dst, int ld_dst, int T, int* ws, void* stream);
/* the same for a CONTIGUOUS table dst[T][W] of T <= 8 rows (idx must be given): fixed-order sums instead of atomics -- the table's
 * gradient is then bit-reproducible.  ws: 64 * T * W floats. */
int hamt_scatter_add_rows_small(int R, int W, const float* src, int ld_src, int col0, const int64_t* idx, int T, float* dst,
                                float* ws, void* stream);

/* BertEmbeddings sum (A1, vilmodel.py:62-66): z[b*L+l] = word[ids[b,l]] + pos[l] + type0 */
int hamt_embed_sum_fwd(int B, int L, int H, const int64_t* ids, const float* word, const float* pos,
                       const float* type_row, float* z, void* stream);
/* backward: dword[ids] += dz, dpos[l] += sum_b dz, dtype_row += sum dz (any of the three may be NULL);
 * V = rows of the word table (ids outside [0, V) are skipped).  ws / ws_bytes: device scratch and ITS SIZE; needed when dtype_row is given
 * (>= HAMT_WS_COLSUM {B * L, H}, checked).  With ws_bytes >= HAMT_WS_EMBED_BWD {B * L, H} the word rows are summed in a fixed order
 * (hamt_scatter_add_rows_ordered); with less (or beyond 262 144 rows) by atomic adds -- never written past ws_bytes */
int hamt_embed_sum_bwd(int B, int L, int H, int V, const int64_t* ids, const float* dz, float* dword,
                       float* dpos, float* dtype_row, float* ws, size_t ws_bytes, void* stream);

/* broadcast row ops over x[B, S, H]:
 *   mean over the middle axis  (A11 vilmodel.py:563-564):  y[b,:] = mean_s x[b,s,:]
 *   mul_bcast (A16 pretrain_cmt.py:176, A13 :722):  y[b,s,:] = a[b,s,:] * c[b,:]
 */
int hamt_mean_mid_fwd(int B, int S, int H, const float* x, float* y, void* stream);
int hamt_mean_mid_bwd(int B, int S, int H, const float* dy, float* dx, void* stream);
int hamt_mul_bcast_fwd(int B, int S, int H, const float* a, const float* c, int ldc_rows, float* y, void* stream);
int hamt_mul_bcast_bwd(int B, int S, int H, const float* a, const float* c, int ldc_rows, const float* dy,
                       float* da, float* dc, void* stream);
/* sums x[B,S,H] over b and/or s; `out` is ADDED to in both modes, never overwritten (zero it first for the plain sum):
 * mode 0: out[H] += sum_{b,s} (ws: >= 64*H floats); 1: out[s,H] += sum_b */
int hamt_sum_rows(int B, int S, int H, const float* x, int mode, float* out, float* ws, void* stream);

/* elementwise: out = a + b (+ c) ; dropout forward/backward (feature dropout, model_HAMT.py:32-52) */
/* image [N][C][H][W] fp32 -> patch rows y[N*(H/P)*(W/P) .. Rpad)[C*P*P] (fp32 or bf16; rows beyond the patches zero): column
 * order = the flattened conv weight [D][C][P][P], so PatchEmbed's conv (vision_transformer.py:216-221) becomes one GEMM */
int hamt_patchify(int N, int C, int H, int W, int P, const float* x, void* y, int ldy, int dtype_y, int Rpad, void* stream);
/* Panorama view transform of the image-input pipeline (pretrain_src/data/image_data.py:70-80, 225-237: timm's create_transform,
 * one PIL call chain per view on the host): for every OUTPUT slot i, crop box (left, top, width, height) of source view `src`
 * (uint8 [H][W][3] as stored) -> PIL's BICUBIC resize of the crop to 224 x 224 -> horizontal flip -> colour jitter ->
 * x / 255 -> (x - 0.5) / 0.5, PIL's / torch's result bit for bit (integer resampling taps, float32 blends rounded to uint8 after
 * every op; see csrc/image_prep.hip).  `order`: the three jitter ops from first to last in bits [1:0], [3:2], [5:4], each one of
 * HAMT_JIT_* (HAMT_JIT_SKIP: nothing), contrast at most once.  A slot with `zero` != 0
 * or src < 0 is written as 0.0 (padded history steps, the killed observation: image_tasks.py:61-69, 181-183).
 * Output: HAMT_IMAGE_NCHW fp32 y[n][3][224][224], or HAMT_IMAGE_PATCHES: the rows hamt_patchify(n, 3, 224, 224, 16, ...) makes of
 * that tensor (ldy, dtype_y fp32 / bf16, Rpad; rows beyond n * 196 zero) -- the fp32 image is then never written.
 * views_host / views_dev: the SAME table of n records in host memory (argument checks; read during the call only) and in device
 * memory (read by the kernels).  lut: DEVICE, 256 floats, lut[u] = the normalised value of byte u (made by the caller with the
 * framework's own arithmetic).  ws: HAMT_WS_IMAGE_PREP {n} bytes of device scratch, 16-byte aligned; its previous content is
 * irrelevant.  Two launches whatever n is (one when every slot is zero).  A crop box outside the view, an empty box, a misaligned
 * output, a short Rpad or ws: HAMT_ERR_ARG; a box side above 784 pixels: HAMT_ERR_UNSUPPORTED; nothing is launched then. */
enum { HAMT_JIT_BRIGHTNESS = 0, HAMT_JIT_CONTRAST = 1, HAMT_JIT_SATURATION = 2, HAMT_JIT_SKIP = 3 };
enum { HAMT_IMAGE_NCHW = 0, HAMT_IMAGE_PATCHES = 1 };
typedef struct {
  int32_t src;                       /* source view index in [0, n_src), < 0: none */
  int32_t left, top, width, height;  /* crop box in pixels */
  int32_t flip;
  int32_t zero;
  int32_t order;                     /* HAMT_JIT_* x 3 */
  float brightness, contrast, saturation;
  int32_t reserved;
} hamt_image_view;                   /* 48 bytes */
typedef struct {
  int n, n_src, H, W;                /* output slots, source views, view size */
  int layout;                        /* HAMT_IMAGE_* */
  int ldy, dtype_y, Rpad;            /* HAMT_IMAGE_PATCHES only */
} hamt_image_prep_desc;
int hamt_image_prep(const hamt_image_prep_desc* d, const hamt_image_view* views_host, const hamt_image_view* views_dev,
                    const uint8_t* src, const float* lut, void* y, void* ws, size_t ws_bytes, void* stream);
/* PIL's antialiased 8-bit resample of whole views at a real scale factor (Resample.c; the reference's build_image_lmdb.py:78 resizes
 * every 480 x 640 render to 248 x 330 with ANTIALIAS = LANCZOS, timm's Resize(248) in precompute_img_features_vit.py:51-52 does it
 * bicubically): src uint8 [n][H][W][3] -> Image.resize((OW, OH), filter) of every view, of which only the window of w x h pixels at
 * (x0, y0) is computed and written: dst uint8 [n][h][w][3].  Bit for bit PIL's result: two passes, horizontal first, the filter
 * support scaled by the reduction factor, 22-bit fixed-point taps, a uint8 intermediate; an axis whose size does not change is
 * not resampled.
 * hamt_image_resample_taps is a HOST function (no device, no stream): PIL's precompute_coeffs + normalize_coeffs_8bpc for the
 * output coordinates [first, first + count) of an axis resized in -> out, computed in double with the host's libm.  xmin[count],
 * xcnt[count]: first input coordinate and number of taps; k[count][ksize]: the taps, zero beyond xcnt.  Returns the number of
 * taps per coordinate the geometry needs (`ksize` must be at least that); with all three arrays NULL it only returns that number.
 * hamt_image_resample takes one table per axis, for the WINDOW's columns (count = w, first = x0) and rows (count = h, first = y0),
 * each laid out as int32 xmin[count] | xcnt[count] | k[count][kx or ky], once in host memory (argument checks and LDS sizing; read
 * during the call only) and once in device memory (read by the kernel).  The table of an axis whose size does not change is not
 * read and may be NULL.  One launch; no scratch.  An unknown filter, an empty window or one outside (OH, OW), a table whose bounds
 * leave the view, null pointers, or a geometry whose tables and one output row's input rows exceed the 160 KiB of LDS:
 * HAMT_ERR_ARG, and nothing is launched. */
enum { HAMT_RESAMPLE_BICUBIC = 0 /* a = -0.5, support 2 */, HAMT_RESAMPLE_LANCZOS = 1 /* support 3; PIL's former ANTIALIAS */ };
typedef struct {
  int n, H, W;                       /* views and their size */
  int OH, OW;                        /* size of the whole resized view */
  int x0, y0, w, h;                  /* the window of it that is written */
  int filter;                        /* HAMT_RESAMPLE_* */
  int kx, ky;                        /* taps per entry of the column / row table */
} hamt_image_resample_desc;
int hamt_image_resample_taps(int in, int out, int filter, int first, int count, int32_t* xmin, int32_t* xcnt, int32_t* k, int ksize);
int hamt_image_resample(const hamt_image_resample_desc* d, const int32_t* xtab_host, const int32_t* ytab_host, const int32_t* xtab_dev,
                        const int32_t* ytab_dev, const uint8_t* src, uint8_t* dst, void* stream);
int hamt_add3(size_t n, const float* a, const float* b, const float* c, float* out, void* stream);
int hamt_dropout(size_t n, const float* x, float* y, float p, uint32_t call_id, const uint64_t* rng, void* stream);
int hamt_cast_f32_bf16(size_t n, const float* x, void* y, void* stream);
/* Device-side batch collation (replaces the host loops of pretrain_src/data/common.py:5-29 `pad_tensors` /
 * `gen_seq_masks` and torch's pad_sequence as the six *_collate functions of data/r2r_tasks.py use them).  The host packs
 * the ragged per-sample rows back to back (no padding) into one pinned buffer and copies it once; on the device
 *   dst[b][t][:] = t < len_b ? src[prefix[b] + t][:] : pad_byte repeated      (rows of row_bytes bytes, any dtype)
 *   mask[b][t]   = t < len_b + add,   lens_out[b] = len_b + add               (bool bytes / int64; lens_out may be NULL)
 * with prefix[0..B] (int32, DEVICE) the exclusive prefix sum of the sample lengths in rows.  Bit exact by construction. */
int hamt_unpack_padded(const void* src, const int32_t* prefix, int B, int maxlen, int row_bytes, int pad_byte, void* dst, void* stream);
int hamt_seq_masks(const int32_t* prefix, int add, int B, int maxlen, uint8_t* mask, int64_t* lens_out, void* stream);
/* Gradient wire format of the data-parallel exchange (the stock DDP bf16_compress_hook's arithmetic: divide by the world
 * size, round to bf16, all-reduce(SUM) in bf16, widen): y[i] = bf16(x[i] * scale) and x[i] = fp32(y[i]).  x (fp32) and y
 * (bf16) must sit at the same element offset modulo 4 of 16-byte aligned bases (a mirrored staging arena). */
int hamt_wire_pack_bf16(size_t n, const float* x, void* y, float scale, void* stream);
int hamt_wire_unpack_bf16(size_t n, const void* y, float* x, void* stream);
/* x[i] = value where flag[i] == 0  (A16 in-place masked_fill_(nav_types == 0, -inf), pretrain_cmt.py:177;
 * its backward zeroes the gradient at the same positions) */
int hamt_fill_where_zero(size_t n, const int64_t* flag, float* x, float value, void* stream);
/* out[i] = (1 - mask[i]) * -10000: the additive attention mask of a bool (1 byte / element) keep-mask (vilmodel.py:597-599) */
int hamt_extend_mask(size_t n, const void* mask_u8, float* out, void* stream);
/* test aid: fill the LDS of every CU with `pattern` (a kernel that reads LDS it has not written then shows it) */
int hamt_debug_fill_lds(uint32_t pattern, void* stream);
/* measurement aid (bench.py `roofline`): with on != 0 every grouped weight-gradient KERNEL launched eagerly by
 * hamt_wgrad_grouped is bracketed by HIP events on its launch stream; hamt_debug_wgrad_times waits for them and returns
 * their number, writing up to `cap` durations (us), tile heights (256 = a 256-square tile) and flops (2 M N K over the
 * launch's table, K = the k-tiles actually multiplied).  Not for captures. */
int hamt_debug_wgrad_timing(int on);
int hamt_debug_wgrad_times(float* us, int* tile_rows, double* flops, int cap);
/* Which kernel each of those launches was: two_phase[i] = 1 for wgrad_grouped_p8_kernel (the two-phase 256-square tile), 0 for
 * wgrad_grouped_kernel (64 / 128 rows, and the one-phase 256-square tile behind HAMT_WGRAD_P8=0).  Returns their number. */
int hamt_debug_wgrad_variants(int* two_phase, int cap);
/* dx = dy * act'(h): mode 1 erf-GELU (vilmodel.py:23-29), mode 2 ReLU (h may be the ReLU output) */
int hamt_act_bwd(size_t n, const float* dy, const float* h, int mode, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * losses, reduction='none' as in the reference
 *   ce:  loss[r] = logsumexp(x[r,:C]) - x[r,label[r]]     (A15/A16/A20; -inf logits allowed)
 *        backward  dx[r,c] = g[r] * (softmax(x[r])[c] - [c == label[r]])
 *        a label outside [0, C) marks an ignored row (F.cross_entropy's ignore_index): loss 0, dx = 0
 *   mse: loss = (x - t)^2 elementwise (A17/A18); backward dx = 2 g (x - t)
 *   kl:  loss[r] = sum_c t*(log t - log_softmax(x)[c]) with 0*log0 = 0 (A19, pretrain_cmt.py:239-240)
 *        backward dx[r,c] = g[r] * (softmax(x)[c] * sum_c t - t[c])
 * ---------------------------------------------------------------------------------------------- */
int hamt_ce_fwd(int R, int C, const float* x, int ldx, const int64_t* label, float* loss, float* lse, void* stream);
int hamt_ce_bwd(int R, int C, const float* x, int ldx, const int64_t* label, const float* lse,
                const float* g, float* dx, int lddx, void* stream);
int hamt_mse_fwd(size_t n, const float* x, const float* t, float* loss, void* stream);
int hamt_mse_bwd(size_t n, const float* x, const float* t, const float* g, float* dx, void* stream);
int hamt_kl_fwd(int R, int C, const float* x, int ldx, const float* t, int ldt, float* loss, float* lse, void* stream);
int hamt_kl_bwd(int R, int C, const float* x, int ldx, const float* t, int ldt, const float* lse,
                const float* g, float* dx, int lddx, void* stream);
/* The loss / accuracy side of the proxy-task validation pass (pretrain_src/main_r2r.py:344-511), accumulated on the device.  Each call
 * ADDS into caller-owned accumulators -- sums fp64 [4], counts int64 [4] -- and reads nothing from the host; R == 0 is a no-op.  The
 * row terms are fp32 exactly as hamt_ce_fwd / hamt_kl_fwd / hamt_mse_fwd compute them; one workgroup folds them in fp64 in a fixed
 * order (no floating-point atomics), so the totals are bit-identical from run to run.  ws: 2 R floats of scratch, fully rewritten.
 *   hamt_eval_ce        sums[0] += sum of logsumexp(x[r]) - x[r, label[r]], counts[0] += rows whose arg-max (the LOWEST index among
 *                       the maxima, scores.max(-1)[1]) equals the label, counts[1] += rows, over the rows with label >= 0 (a negative
 *                       label: the row is ignored altogether; a label >= C: NaN).  A row with a NaN logit adds NaN and is not correct.
 *   hamt_eval_kl        sums[0] += sum_r sum_c t (log t - log_softmax(x)) with 0 log 0 = 0, counts[0] += rows where argmax x[r] ==
 *                       argmax t[r] (lowest index on ties), counts[1] += R
 *   hamt_eval_mse_cols  sums[c] += sum_r (x[r,c] - t[r,c])^2 for c < C <= 4; one launch */
int hamt_eval_ce(int R, int C, const float* x, int ldx, const int64_t* label, float* ws, double* sums, int64_t* counts, void* stream);
int hamt_eval_kl(int R, int C, const float* x, int ldx, const float* t, int ldt, float* ws, double* sums, int64_t* counts,
                 void* stream);
int hamt_eval_mse_cols(int R, int C, const float* x, int ldx, const float* t, int ldt, double* sums, void* stream);
/* A2C rollout loss of the finetune agent (finetune_src/r2r/agent_cmt.py:476-518), all [T, B] steps x episodes at once
 * (row-major [T][B] fp32 arrays): ret[t,b] = discounted return R_t = gamma R_{t+1} + reward_t seeded with last_value[b]
 * (NULL = 0: the caller passes the critic's value of the last state for episodes that have not ended, 0 for the others);
 * out[b] = {sum_t -logp (R - V) mask, sum_t 1/2 (R - V)^2 mask, sum_t -ent_w ent mask} (ent may be NULL).  bwd: gradients
 * of g[0] * sum(out) w.r.t. logp, value (critic term only: the advantage in the policy term is detached, :493) and ent. */
int hamt_a2c_fwd(int T, int B, const float* reward, const float* mask, const float* value, const float* logp, const float* ent,
                 const float* last_value, float gamma, float ent_w, float* ret, float* out, void* stream);
int hamt_a2c_bwd(int T, int B, const float* ret, const float* mask, const float* value, float ent_w, const float* g,
                 float* dlogp, float* dvalue, float* dent, void* stream);
/* The decision and loss side of ONE rollout step of the finetune agents (finetune_src/r2r/agent_cmt.py:336-401; the R2R-back, CVDN
 * and REVERIE agents repeat it verbatim), all B episodes in one launch, one wave per row of logit [B, V <= 256] (fp32, row stride
 * ld_logit, -inf entries allowed).  Per row b, written at the caller's row-t addresses of its [T, B] arrays (what hamt_a2c_fwd reads):
 *   ml      cross-entropy of the UNMASKED row against target[b] (:339), 0 where target == ignoreid or target is NULL
 *   action  a_t: forced_action[b] if given; else target (teacher), the lowest index among the maxima of the back-track-masked row
 *           (argmax, :356), or the inverse CDF of the masked softmax at uniform[b] (sample; uniform NULL: a 24-bit draw hashed
 *           from rng = {seed, epoch} (DEVICE, as every dropout kernel reads it), call_id and b)
 *   logp    teacher 0; argmax log_softmax(masked row)[a_t] (:358-359); sample the same clamped to [log eps, log(1 - eps)],
 *           eps = FLT_EPSILON, as torch.distributions.Categorical(probs).log_prob does (:361-366)
 *   ent     -sum p log p of the masked row, 0 log 0 = 0; written in sample mode only (:364)
 *   mask    !ended_in (:418-420);   env_action  -1 if a_t == cand_len - 1 (STOP), a_t == ignoreid or ended_in, else a_t (:372-375)
 *   prev_angle [B, A] = ob_ang[b, env_action, :] (ob_ang [B, V, A] contiguous), zeros where env_action == -1 or ob_ang is NULL (:382-385)
 *   ended   (in/out, uint8) |= env_action == -1 (:447);   hist_len (in/out, may be NULL) += !ended_in (:399-401)
 *   lse [B, 2]  log-sum-exp of the unmasked and of the masked row: all the backward needs next to the inputs
 * bt_mask [B, V] uint8 (non-zero = masked, :350), target, ob_ang, forced_action, uniform, prev_angle, hist_len may be NULL.
 * A row whose every slot is masked cannot occur on the path (the STOP slot is never a visited viewpoint); it, and an action outside
 * [0, V), give env_action -1, logp 0, ent 0 and zero gradients, never NaN or an out-of-bounds read.
 * bwd: dlogit[b, v] = g_ml[b] (softmax(logit)[v] - [v == target]) + g_logp[b] ([v == a_t] - p[v]) + g_ent[b] (-p[v] (log p[v] + H[b])),
 * p the masked softmax; the last two terms are 0 at masked positions, the first for ignored rows, the second where the clamp was
 * active.  g_ml / g_logp / g_ent may be NULL (= 0); row b of each is read at element b * gs_* (1 = contiguous, 0 = one value for
 * every row: the expanded gradient of a plain sum arrives like that, and needs no copy). */
#define HAMT_POLICY_TEACHER 0
#define HAMT_POLICY_ARGMAX 1
#define HAMT_POLICY_SAMPLE 2
int hamt_policy_step_fwd(int B, int V, int A, int mode, int64_t ignoreid, const float* logit, int ld_logit,
                         const int64_t* target, const uint8_t* bt_mask, const int32_t* cand_len, uint8_t* ended,
                         const float* ob_ang, const int64_t* forced_action, const float* uniform, const uint64_t* rng,
                         uint32_t call_id, float* ml, int64_t* action, float* logp, float* ent, float* mask,
                         int32_t* env_action, float* prev_angle, int32_t* hist_len, float* lse, void* stream);
int hamt_policy_step_bwd(int B, int V, int mode, int64_t ignoreid, const float* logit, int ld_logit, const int64_t* target,
                         const uint8_t* bt_mask, const int64_t* action, const float* lse, const float* g_ml,
                         const float* g_logp, const float* g_ent, int gs_ml, int gs_logp, int gs_ent, float* dlogit, int ld_dlogit,
                         void* stream);
/* REVERIE's rollout step (finetune_src/reverie/agent.py:253-307), one launch, one wave per row.  What differs from hamt_policy_step:
 *   the row    V + 1 <= 256 columns: act_logit [B, V] (V = ob_img_max_len; fp32, row stride ld_act, -inf at everything that is not a
 *              navigable candidate) and column V, STOP, made from obj_logit [B, O] (0 < O <= 256, row stride ld_obj, -inf at padding):
 *              HAMT_STOP_LOGIT_INDEX (float) of the row's arg-max, as the reference writes it (:253-254 keeps torch.max's indices) -- no
 *              gradient reaches obj_logit through the action row; HAMT_STOP_LOGIT_VALUE the maximum itself, whose gradient goes to the
 *              arg-max element.  Ties: the lowest index.
 *   ml         cross-entropy of the back-track-MASKED row (:269 precedes :274) against target[b]; a target that is not ignoreid and is
 *              >= cand_len[b] - 1 (cand_len = navigable candidates + 1) means STOP and is read as V, so the reference's V and
 *              hamt_nav_observe's cand_len - 1 both drive it.  bt_mask [B, V] uint8: column V is never masked.
 *   ref        cross-entropy of obj_logit[b, :O] against ref_target[b] (:275; ignoreid = 0); ref_target NULL and obj_id int32 [B, O] +
 *              goal_obj int32 [B] given: the first k < obj_len[b] with obj_id[b, k] == goal_obj[b] where the target is STOP and the
 *              episode had not ended, else ignored (_teacher_action, :150-160).  Both NULL: ref = 0.
 *   action     as hamt_policy_step over the V + 1 columns; teacher: the target with STOP read as V.
 *   env_action -1 iff a_t >= V, a_t == ignoreid or ended_in (:306); no cand_len - 1 rule.  prev_angle from ob_ang [B, V, A].
 *   pred_obj   int32 [B], written ONLY where (a_t >= V or last_step) and !ended_in (:299-304): -1 if obj_len[b] == 0 (obj_len is the
 *              true count; the reference pads an empty list to one slot for the model, the prediction stays None), else the lowest
 *              arg-max of obj_logit[b, :obj_len[b]].  pred_obj_id the same through obj_id (needs obj_id).  Either may be NULL.
 *   lse [B, 3] log-sum-exp of the masked action row and of the object row, and column V's value; saved int32 [B, 3]: the object
 *              arg-max and the effective ref / action targets.  With the inputs they are all the backward reads.
 * mask, ended, hist_len, logp, ent, forced_action, uniform, rng, call_id: as hamt_policy_step_fwd.  A row without a finite column
 * (VALUE with an object row of -inf) gives env_action -1, logp 0, ent 0 and zero gradients.
 * bwd: dact [B, V] and dobj [B, O] of sum_b g_ml ml + g_ref ref + g_logp logp + g_ent ent (each g NULL = 0, read at b * gs_*, 0 or 1);
 * column V's gradient is added to dobj[b, arg-max] (VALUE) or dropped (INDEX); masked and -inf positions get exactly 0. */
#define HAMT_STOP_LOGIT_INDEX 0
#define HAMT_STOP_LOGIT_VALUE 1
int hamt_policy_ref_step_fwd(int B, int V, int O, int A, int mode, int stop_logit, int last_step, int64_t ignoreid,
                             const float* act_logit, int ld_act, const float* obj_logit, int ld_obj, const int32_t* obj_len,
                             const int32_t* cand_len, const int64_t* target, const int64_t* ref_target, const int32_t* obj_id,
                             const int32_t* goal_obj, const uint8_t* bt_mask, uint8_t* ended, const float* ob_ang,
                             const int64_t* forced_action, const float* uniform, const uint64_t* rng, uint32_t call_id,
                             float* ml, float* ref, int64_t* action, float* logp, float* ent, float* mask, int32_t* env_action,
                             float* prev_angle, int32_t* hist_len, int32_t* pred_obj, int32_t* pred_obj_id, float* lse,
                             int32_t* saved, void* stream);
int hamt_policy_ref_step_bwd(int B, int V, int O, int mode, int stop_logit, const float* act_logit, int ld_act,
                             const float* obj_logit, int ld_obj, const uint8_t* bt_mask, const int64_t* action, const float* lse,
                             const int32_t* saved, const float* g_ml, const float* g_ref, const float* g_logp, const float* g_ent,
                             int gs_ml, int gs_ref, int gs_logp, int gs_ent, float* dact, int ld_dact, float* dobj, int ld_dobj,
                             void* stream);
/* The navigation-graph side of a rollout step and the evaluation metrics (csrc/nav.hip).  The graphs of all scans lie in one arena:
 * scan s has scan_n[s] nodes and owns the elements [scan_off[s], scan_off[s] + n * n) of `dist` (fp64, all-pairs shortest distances,
 * dist[x * n + y]) and `nxt` (int32, the next hop from x toward y; nxt[x, x] = x).  Node ids are local to their scan.  Episode b:
 * ep_scan[b], cur[b] (the node stood on), goal[b] = gt[b][gt_len - 1], gt int32 [B, g_max], path int32 [B, path_cap] (every node
 * stood on, the start first) with path_len, dtw_row fp64 [B, g_max + 1] (the last row of cal_dtw's matrix for path against gt),
 * last_dist / last_ndtw fp32 [B] (agent_cmt.py:284-289, :444-445), anomalies int32 [2].  One wave per episode.
 * g_max above HAMT_NAV_MAX_GT or a path_cap / p_max above HAMT_NAV_MAX_PATH: HAMT_ERR_UNSUPPORTED, nothing launched.
 *
 * hamt_nav_observe (before the policy step of step t): target[b] = what agent_cmt.py::_teacher_action returns -- ignoreid if
 * ended[b]; else the first slot c < cand_len[b] - 1 with cand_node[b, c] == the teacher's viewpoint; else slot cand_len[b] - 1 (STOP)
 * if that viewpoint is cur[b]; where the reference's assert fails (no teacher viewpoint, or one that is neither): ignoreid and
 * anomalies[0] += 1.  The teacher's viewpoint (env.py::_teacher_path_action): PATH_STEP gt[t + 1] if t < gt_len - 1 else cur;
 * PATH_INDEX the successor of cur's first occurrence in gt (cur if it is the last element, none if absent); SHORTEST nxt[cur, goal].
 * bt_mask[b, c] = 1 where c < cand_len[b] - 1 and cand_node[b, c] is in path[b][:path_len] (:342-349).  cand_node int32 [B, V], -1 =
 * padding.  target or bt_mask may be NULL (not computed).
 *
 * hamt_nav_advance (after it): env_action[b] >= 0 moves episode b to cand_node[b, env_action[b]] and appends it to path; the DTW row
 * advances by that node alone.  dist = (float)dist[cur, goal], ndtw = (float)exp(-dtw_row[gt_len] / (3 gt_len)); reward_row[b] is
 * agent_cmt.py:418-441 in fp32 with mask_row[b] = 1 - ended before the step (0: reward 0); a move that leaves the fp32 distance
 * unchanged (the reference raises NameError) gets ndtw - last_ndtw and anomalies[1] += 1.  last_dist / last_ndtw take dist / ndtw for
 * every episode.
 *
 * hamt_nav_eval: out fp64 [N, HAMT_NAV_EVAL_COLS] = env.py::_eval_item of trajectory i (path [N, p_max], gt [N, g_max], local nodes
 * of scan[i]) in the column order nav_error, oracle_error, trajectory_steps, trajectory_lengths, success, spl, oracle_success, DTW,
 * nDTW, SDTW, CLS.  A length outside [1, p_max] / [1, g_max] or a node outside its scan: a row of NaN. */
#define HAMT_NAV_PATH_STEP 0
#define HAMT_NAV_PATH_INDEX 1
#define HAMT_NAV_SHORTEST 2
#define HAMT_NAV_MAX_GT 512
#define HAMT_NAV_MAX_PATH 4096
#define HAMT_NAV_EVAL_COLS 11
int hamt_nav_observe(int B, int V, int mode, int t, int64_t ignoreid, int g_max, int path_cap, const int32_t* nxt,
                     const int64_t* scan_off, const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node,
                     const int32_t* cand_len, const uint8_t* ended, const int32_t* cur, const int32_t* goal, const int32_t* gt,
                     const int32_t* gt_len, const int32_t* path, const int32_t* path_len, int32_t* anomalies, int64_t* target,
                     uint8_t* bt_mask, void* stream);
int hamt_nav_advance(int B, int V, int g_max, int path_cap, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                     const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action, const float* mask_row,
                     int32_t* cur, const int32_t* goal, const int32_t* gt, const int32_t* gt_len, int32_t* path, int32_t* path_len,
                     double* dtw_row, float* last_dist, float* last_ndtw, int32_t* anomalies, float* reward_row, void* stream);
int hamt_nav_eval(int N, int p_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                  const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* gt, const int32_t* gt_len,
                  double* out, void* stream);
/* The same for the reference's other three agents (csrc/nav.hip, the same arena, the same clamping and NaN rows).
 *
 * Goal sets (CVDN's end_panos, REVERIE's viewpoints an object is visible from): goals int32 [B, e_max] with goal_len [B]; the distance
 * of a node is the minimum over the set, taken in fp64.  e_max above HAMT_NAV_MAX_GOALS: HAMT_ERR_UNSUPPORTED, nothing launched.
 * hamt_nav_advance_goals (after the policy step): the move as hamt_nav_advance (new node, appended to path);
 * dist = (float)min_e dist[cur, goals[e]], 0 for an empty set (cvdn/env.py:85-86); reward_row[b] is cvdn/agent.py:174-203 =
 * reverie/agent.py:337-366: 0 where mask_row[b] == 0 (ended before the step); a stop (env_action < 0) 2 if dist == 0 else -2; a move
 * +1, -1 or 0 by the sign of -(dist - last_dist) (an unchanged distance is no anomaly here).  last_dist takes dist for every episode.
 * There is no DTW row and no last_ndtw.
 * hamt_nav_eval_goals: out fp64 [N, HAMT_NAV_GOALS_EVAL_COLS] in the column order trajectory_steps, trajectory_lengths, success,
 * oracle_success, spl, gp, spl_ratio.  gt_lengths = the sum of dist along gt (reverie/env.py::_eval_item) or, with gt and gt_len NULL,
 * min_e dist[path[0], goals[e]] (cvdn/env.py::_eval_item); success = path[-1] in goals, oracle_success = any node of path in goals;
 * spl_ratio = gt_lengths / max(trajectory_lengths, gt_lengths, 0.01), spl = success * spl_ratio (REVERIE's rgspl = rgs * spl_ratio is
 * formed by the caller); gp = gt_lengths - min_e dist[path[-1], goals[e]].  A length outside [1, p_max] / [1, e_max] / [1, g_max] or a
 * node outside its scan: a row of NaN.  Only lengths are taken along gt, so g_max may reach HAMT_NAV_MAX_PATH.
 *
 * Return trips (R2R-Back: to the mid-stop, then on to the path's end): midstop int32 [B] (the ground truth's), first_ended uint8 [B]
 * (the first STOP has been made), midstop_at int32 [B] (where, -1 = not yet), and the recorder's `ended` uint8 [B].
 * hamt_nav_advance_back runs after the policy step, which has set ended |= stop: the move, the DTW row and ndtw as hamt_nav_advance;
 * d0 = (float)dist[cur, midstop], d1 = (float)dist[cur, goal], dist = first_ended (before the step) ? d1 : d0; reward_row[b] is the
 * block of hamt_nav_advance (agent_r2rback.py:241-265) on this dist, an unchanged fp32 distance on a move counted in anomalies[1].  An
 * episode with mask_row[b] != 0 that stops with first_ended clear: midstop_at = cur, first_ended = 1, last_dist = d1, and
 * ended = (end_on_miss && !(dist < 3)) -- the reference ends a missed mid-stop only under RL training (:252), otherwise the episode
 * goes on (:275).  Every other episode: last_dist = dist, `ended` as the policy step left it; one with mask_row[b] == 0 gets
 * first_ended = 1 (:276).  last_ndtw takes ndtw for every episode.
 * hamt_nav_eval_back: out fp64 [N, HAMT_NAV_BACK_EVAL_COLS] = env.py::R2RBackBatch._eval_item in the column order nav_error,
 * trajectory_steps, trajectory_lengths, success, spl, DTW, nDTW, SDTW, CLS; midstop[i] = -1 for None; success = midstop >= 0 and
 * dist[midstop, gt_midstop] <= 3 and dist[path[-1], gt[-1]] <= 3.  NaN rows as hamt_nav_eval, also for a midstop outside [-1, n) or
 * a gt_midstop outside [0, n). */
#define HAMT_NAV_MAX_GOALS 256
#define HAMT_NAV_GOALS_EVAL_COLS 7
#define HAMT_NAV_BACK_EVAL_COLS 9
int hamt_nav_advance_goals(int B, int V, int e_max, int path_cap, const double* dist, const int64_t* scan_off,
                           const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action,
                           const float* mask_row, int32_t* cur, const int32_t* goals, const int32_t* goal_len, int32_t* path,
                           int32_t* path_len, float* last_dist, float* reward_row, void* stream);
int hamt_nav_advance_back(int B, int V, int g_max, int path_cap, int end_on_miss, const double* dist, const int64_t* scan_off,
                          const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cand_node, const int32_t* env_action,
                          const float* mask_row, int32_t* cur, const int32_t* goal, const int32_t* midstop, const int32_t* gt,
                          const int32_t* gt_len, int32_t* path, int32_t* path_len, double* dtw_row, float* last_dist,
                          float* last_ndtw, uint8_t* first_ended, int32_t* midstop_at, uint8_t* ended, int32_t* anomalies,
                          float* reward_row, void* stream);
int hamt_nav_eval_goals(int N, int p_max, int e_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                        const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* goals,
                        const int32_t* goal_len, const int32_t* gt, const int32_t* gt_len, double* out, void* stream);
int hamt_nav_eval_back(int N, int p_max, int g_max, const double* dist, const int64_t* scan_off, const int32_t* scan_n,
                       const int32_t* scan, const int32_t* path, const int32_t* path_len, const int32_t* gt, const int32_t* gt_len,
                       const int32_t* midstop, const int32_t* gt_midstop, double* out, void* stream);
/* The observations of a rollout step, gathered from a viewpoint store (csrc/obs.hip).  The store holds every viewpoint of every scan in
 * the arena order of the navigation graphs, row = vp_base[scan] + local node (vp_base int64 = the prefix sum of scan_n), NV rows:
 * feat fp32 [NV, 36, F]; ang36 fp32 [36, 36, A] (base view, view); cand_cnt int32 [NV]; cand_point int32 [NV, C] (each candidate's view
 * index), cand_node int32 [NV, C] (its local node, -1 = padding), cand_ang fp32 [NV, C, 12, A] (its angle feature for each of the 12 base
 * headings).  C above HAMT_OBS_MAX_CAND: HAMT_ERR_UNSUPPORTED, nothing launched.  Episode b: ep_scan[b], cur[b], view[b] in [0, 36).
 *
 * hamt_obs_gather: with row = vp_base[ep_scan[b]] + cur[b] and n = min(cand_cnt[row], C, W - 1), slot c < n of episode b is candidate c
 * (image feat[row, cand_point[c]], angle cand_ang[row, c, view % 12], nav type 1), slot n is STOP (zeros, nav type 2); HAMT_OBS_PANO
 * (agent_cmt.py::_cand_pano_feature_variable) goes on with the views no candidate points to, ascending (image feat[row, v], angle
 * ang36[view, v], nav type 0); HAMT_OBS_CAND (::_candidate_variable) ends there.  The slots from ob_len[b] to W are zeros, nav type 0.
 * ob_img fp32 [B, W, F], ob_ang fp32 [B, W, A], ob_nav int64 [B, W], ob_mask uint8 [B, W] (1 = slot < ob_len), ob_len, cand_len (= n + 1)
 * int32 [B], cand_node_out / cand_point_out int32 [B, W] (the candidates' nodes / views, -1 elsewhere).  hist_img [B, F] = feat[row, view],
 * hist_pano_img [B, 36, F] = feat[row], hist_pano_ang [B, 36, A] = ang36[view] (::_history_variable): each may be NULL.  Every element of
 * every output is written by every call; ended episodes are gathered like the others.  A cur outside its scan or a view outside
 * [0, 36): nothing is read from the store, the episode is STOP alone (zeros everywhere, nav type 2 and mask 1 in slot 0, ob_len =
 * cand_len = 1, zero history rows), anomalies[0] += 1.  Rows are copied 16 bytes per lane when F % 4 == 0 and feat, ob_img, hist_img
 * and hist_pano_img are 16-byte aligned, element by element otherwise; no arithmetic touches a value.
 *
 * hamt_obs_turn: view[b] = cand_point_out[b, env_action[b]] where 0 <= env_action[b] < W and that slot holds a candidate; unchanged
 * otherwise.  view_log_row int32 [B] (may be NULL) receives the resulting views.  It reads what hamt_obs_gather wrote, not the store. */
#define HAMT_OBS_PANO 0
#define HAMT_OBS_CAND 1
#define HAMT_OBS_MAX_CAND 64
int hamt_obs_gather(int B, int W, int F, int A, int C, int layout, const float* feat, const float* ang36, const int32_t* cand_cnt,
                    const int32_t* cand_point, const int32_t* cand_node, const float* cand_ang, const int64_t* vp_base,
                    const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cur, const int32_t* view, float* ob_img,
                    float* ob_ang, int64_t* ob_nav, uint8_t* ob_mask, int32_t* ob_len, int32_t* cand_len, int32_t* cand_node_out,
                    int32_t* cand_point_out, float* hist_img, float* hist_pano_img, float* hist_pano_ang, int32_t* anomalies,
                    void* stream);
int hamt_obs_turn(int B, int W, const int32_t* cand_point_out, const int32_t* env_action, int32_t* view, int32_t* view_log_row,
                  void* stream);
/* REVERIE's candidate objects of a rollout step, gathered from an object store over the SAME arena rows (csrc/obs.hip; what
 * finetune_src/reverie/env.py::_get_obs :181-215 and reverie/agent.py::_object_variable :125-139 build on the host).  The store is CSR:
 * obj_off int64 [NV + 1] (row r owns the objects [obj_off[r], obj_off[r + 1]), already cut to the environment's max_objects; a viewpoint
 * without objects owns none), obj_feat fp32 [NObj, Fo], obj_view int32 [NObj] (the view each object was seen in), obj_pos fp32 [NObj, 5]
 * (reverie/data_utils.py::get_obj_local_pos), obj_id int32 [NObj] (>= 0).  ang36, vp_base, scan_n (S scans): the viewpoint store's.
 *
 * hamt_obj_gather: with row = vp_base[ep_scan[b]] + cur[b] and n = min(obj_off[row + 1] - obj_off[row], Ow), slot k < n of episode b is
 * object obj_off[row] + k: obj_feats fp32 [B, Ow, Fo] = its obj_feat row, obj_angles fp32 [B, Ow, A] = ang36[view[b], obj_view] (view NOT
 * reduced mod 12; obj_view clamped to [0, 36)), obj_poses fp32 [B, Ow, 5] = its obj_pos row, obj_ids int32 [B, Ow] = its id.  The slots
 * from n to Ow are zeros, id -1.  obj_masks uint8 [B, Ow] = 1 for k < max(n, 1): a viewpoint without objects shows the model ONE live,
 * all-zero slot (agent.py:126); obj_lens int32 [B] = n, the TRUE count hamt_policy_ref_step_fwd's obj_len wants.  Every element of every
 * output is written by every call; ended episodes are gathered like the others.  An ep_scan outside [0, S), a cur outside its scan, a
 * view outside [0, 36), or a row whose offsets leave [0, NObj] or descend: nothing is read from the object tables, the episode gets one
 * live zero slot, obj_lens = 0, ids -1, anomalies[0] += 1.  Ow above HAMT_OBJ_MAX_WIDTH (hamt_policy_ref_step's limit on O):
 * HAMT_ERR_UNSUPPORTED, nothing launched.  Rows are copied 16 bytes per lane when Fo % 4 == 0 and obj_feat and obj_feats are 16-byte
 * aligned, element by element otherwise; offsets into obj_feat are 64-bit; no arithmetic touches a value. */
#define HAMT_OBJ_MAX_WIDTH 256
int hamt_obj_gather(int B, int Ow, int Fo, int A, int S, int64_t NV, int64_t NObj, const int64_t* obj_off, const float* obj_feat,
                    const int32_t* obj_view, const float* obj_pos, const int32_t* obj_id, const float* ang36, const int64_t* vp_base,
                    const int32_t* scan_n, const int32_t* ep_scan, const int32_t* cur, const int32_t* view, float* obj_feats,
                    float* obj_angles, float* obj_poses, uint8_t* obj_masks, int32_t* obj_lens, int32_t* obj_ids, int32_t* anomalies,
                    void* stream);
/* The batch a PRETRAINING step consumes, gathered from resident tables in one launch (csrc/pretrain_gather.hip; what
 * pretrain_src/data/r2r_data.py::MultiStepNavData.get_input, the task datasets' corruption and the *_collate padding of r2r_tasks.py build
 * on the host).  Viewpoint tables, NV rows: feat fp32 [NV, 36, F]; prob fp32 [NV, 36, P] (soft labels, may be NULL); ang36 fp32
 * [36, 36, A]; cand_cnt int32 [NV]; cand_view int32 [NV, C] (each candidate's view); cand_ang fp32 [NV, C, 12, A] (its angle feature per
 * base heading).  Step tables, NS rows, the trajectories back to back: step_idx int32 [NS, 4] = (viewpoint row, view looked at, action
 * label in the 36-view layout, action label in the candidates-first layout); step_val fp32 [NS, A + 5] = (the A-wide action angle
 * feature the step leaves in the history, action angles [2] in the 36-view layout, action angles [2] in the candidates-first layout,
 * progress).  sp_table fp32 [36, 36, 2] (may be NULL without sp_targets).  records int32 [B, HAMT_PRETRAIN_RECORD]: (first step row of
 * the trajectory, history length t, flag bits HAMT_PRETRAIN_KILL_*, MRC mask: bit s zeroes history step s, SPREL anchor, then words the
 * kernel does not read).
 *
 * History step s < t of sample b is step row base + s: hist_img [B, Hmax, F] = feat[row, view], hist_ang [B, Hmax, A] = the step's angle
 * feature, hist_pano_img [B, Hmax, 36, F] = feat[row], hist_pano_ang [B, Hmax, 36, A] = ang36[view], hist_prob [B, Hmax, P] =
 * prob[row, view], hist_mrc uint8 [B, Hmax] = the mask bit; a masked step's hist_img and hist_pano_img rows are zeros.  hist_masks uint8
 * [B, Hmax + 1] = 1 for the first t + 1 slots (the cls slot), hist_lens int64 [B] = t + 1.  The observation is step row base + t, W = Omax
 * slots: HAMT_PRETRAIN_VIEWS36 = the 36 views in their own order (nav type 1 where a candidate points) and STOP (zeros, nav type 2);
 * HAMT_PRETRAIN_CANDS_FIRST = hamt_obs_gather's HAMT_OBS_PANO order.  ob_img [B, W, F], ob_ang [B, W, A], ob_nav int64 [B, W], ob_masks
 * uint8 [B, W], ob_lens int64 [B]; HAMT_PRETRAIN_KILL_V zeroes the sample's ob_img, HAMT_PRETRAIN_KILL_A its ob_ang.  act_view int64 [B],
 * act_ang fp32 [B, 2], progress fp32 [B]: the observed step's labels for `layout`; anchor int64 [B] and sp_targets fp32 [B, 36, 2] =
 * sp_table[anchor].  NULL outputs are skipped: the hist_* rows with Hmax = 0, the panorama pair, hist_prob / hist_mrc, the five
 * observation outputs (together; the labels need them), each label; hist_masks and hist_lens are always written.  Every element of every
 * output given is written by every call.  Nothing a record points to is trusted: a base or history length outside [0, NS] / [0, Hmax], an
 * anchor outside [0, 36) (with sp_targets), or a reached step row whose viewpoint row is outside [0, NV) or whose view is outside [0, 36)
 * is found BEFORE any table load; that sample is zeros everywhere (hist_masks 1 in the cls slot only, hist_lens 1, ob_masks and ob_lens 0,
 * labels 0) and anomalies[0] += 1.  Hmax above HAMT_PRETRAIN_MAX_HIST, C above HAMT_PRETRAIN_MAX_CAND or Omax above 37 + HAMT_PRETRAIN_MAX_CAND:
 * HAMT_ERR_UNSUPPORTED, nothing launched.  Rows are copied 16 bytes per lane where F (P) % 4 == 0 and the bases are 16-byte aligned, element by element otherwise;
 * offsets into feat and prob are 64-bit; no arithmetic touches a value. */
#define HAMT_PRETRAIN_VIEWS36 0
#define HAMT_PRETRAIN_CANDS_FIRST 1
#define HAMT_PRETRAIN_KILL_V 1
#define HAMT_PRETRAIN_KILL_A 2
#define HAMT_PRETRAIN_RECORD 8
#define HAMT_PRETRAIN_MAX_HIST 32
#define HAMT_PRETRAIN_MAX_CAND 64
int hamt_pretrain_gather(int B, int Hmax, int Omax, int F, int A, int P, int C, int layout, int64_t NV, int64_t NS, const float* feat,
                         const float* prob, const float* ang36, const int32_t* cand_cnt, const int32_t* cand_view, const float* cand_ang,
                         const int32_t* step_idx, const float* step_val, const float* sp_table, const int32_t* records, float* hist_img,
                         float* hist_ang, float* hist_pano_img, float* hist_pano_ang, float* hist_prob, uint8_t* hist_mrc,
                         uint8_t* hist_masks, int64_t* hist_lens, float* ob_img, float* ob_ang, int64_t* ob_nav, uint8_t* ob_masks,
                         int64_t* ob_lens, int64_t* act_view, float* act_ang, float* progress, int64_t* anchor, float* sp_targets,
                         int32_t* anomalies, void* stream);

/* ------------------------------------------------------------------------------------------------
 * optimiser side (A24): global L2 norm over a flat gradient arena, then the reference's HF AdamW
 * (optim/adamw.py:53-112): m,v update; p -= step_size * m / (sqrt(v) + eps); THEN p -= lr*wd*p.
 * hyper is a DEVICE array: [0]=lr, [1]=step_size (bias corrected lr), [2]=max_grad_norm (<=0: no clip).
 * gnorm_sq is a device scalar holding sum(g^2) (from hamt_sumsq); the clip coefficient
 * min(1, max_norm/(sqrt(gnorm_sq)+1e-6)) (torch clip_grad_norm_, main_r2r.py:271) is applied to g on
 * the fly.  p16 (optional) receives the bf16 shadow of the updated parameters; g is zeroed when
 * zero_grad != 0 (optimizer.zero_grad(), main_r2r.py:280).
 * ---------------------------------------------------------------------------------------------- */
int hamt_sumsq(size_t n, const float* g, float* out, int accumulate, float* ws, void* stream);
int hamt_adamw_flat(size_t n, float* p, float* g, float* m, float* v, void* p16, const float* hyper,
                    const float* gnorm_sq, float beta1, float beta2, float eps, float weight_decay,
                    int zero_grad, void* stream);
/* Whole-arena form: parameter i owns elements [ends[i-1], ends[i]) (offsets multiples of 8, n = ends[nparams-1]);
 * hyp[4*i..4*i+3] = {lr, step_size, weight_decay, active}; parameters with active == 0 are skipped entirely (the
 * reference's `if p.grad is None: continue`).  ends / hyp are DEVICE arrays refreshed by the host each step, so
 * the launch itself is static (hipGraph-capturable). */
int hamt_adamw_table(size_t n, float* p, float* g, float* m, float* v, void* p16, const int* ends,
                     const float* hyp, int nparams, const float* gnorm_sq, float max_norm, float beta1,
                     float beta2, float eps, int zero_grad, void* stream);
/* the same over the arena elements [first, first + n) only (p, g, m, v, p16 point at element `first`; `ends` / `hyp` still
 * describe the whole arena): a rank of a sharded optimizer updates just the segments it owns (parallel.ShardedGradSync), the
 * overlapped update one chunk per launch (optim.AdamW.launch_step_overlapped).  `first` and `n` are multiples of 4 (one 16-byte
 * access never straddles two parameters: offsets are multiples of 8) and need be nothing more: a range may start and end INSIDE
 * parameters, at any multiple of 4.  Nothing outside [first, first + n) is read or written, and an element's result does not
 * depend on the range it is updated in: disjoint ranges that cover the arena give, in any order, bit for bit what one
 * hamt_adamw_table launch gives (tests/test_gpu_adamw.py::test_adamw_table_range_union_is_the_whole). */
int hamt_adamw_table_range(size_t first, size_t n, float* p, float* g, float* m, float* v, void* p16,
                           const int* ends, const float* hyp, int nparams, const float* gnorm_sq,
                           float max_norm, float beta1, float beta2, float eps, int zero_grad, void* stream);
/* active == 2 in hyp: update like 1 but leave the gradient slot as it is (zero_grad then only applies to the active == 1
 * parameters): for slots whose producer overwrites them (the grouped weight-gradient launch stores, it does not accumulate).
 * hamt_sumsq_table: sum(g^2) over the ACTIVE parameters of the arena elements [first, first + n) (g points at element `first`;
 * same `ends` / `hyp` tables): the global-norm reduction that goes with it -- slots of inactive parameters are not read,
 * whatever they hold (torch clip_grad_norm_ over the parameters that have a gradient, main_r2r.py:271-273).  ws: 1024 floats.
 * accumulate: bit 0 = add to *out; bit 1 (HAMT_SUMSQ_SPARSE) = most of the range is inactive / skipped: the active elements are
 * spread evenly over the blocks (for a mostly active range the plain element ranges are faster). */
#define HAMT_SUMSQ_SPARSE 2
int hamt_sumsq_table(size_t first, size_t n, const float* g, const int* ends, const float* hyp, int nparams,
                     float* out, int accumulate, float* ws, void* stream);
/* active == 3: like 2, and hamt_sumsq_table skips the parameter as well -- its sum of squares comes from the weight-gradient
 * tiles (hamt_wgrad_desc.ss).  hamt_sumsq_partials: out (+)= sum of the n floats of `partials` (fixed order). */
int hamt_sumsq_partials(size_t n, const float* partials, float* out, int accumulate, void* stream);
/* g[0 .. n) = float(y16[0 .. n)) and out (+)= sum of g^2 over the ACTIVE parameters (table as hamt_sumsq_table; `first` = arena offset
 * of element 0): the widening of a reduce-scattered bf16 gradient chunk and its share of the global norm in one pass. */
int hamt_wire_unpack_sumsq(size_t first, size_t n, const void* y16, float* g, const int* ends, const float* hyp, int nparams,
                           float* out, int accumulate, float* ws, void* stream);
/* Ralamb / RangerLars (pretrain_src/optim/ralamb.py, lookahead.py): three launches over the arenas (moments + per-item partial sums of
 * squares, per-parameter trust ratio, update + Lookahead sync + bf16 shadow).  Deterministic: no float atomics, fixed summation order.
 * items (DEVICE, int32, 2 * nitems + nparams + 2 entries): [0, nitems] float4 start offset of every item (entry nitems = end of the
 *   last one), [nitems + 1, 2 * nitems] the parameter of every item, [2 * nitems + 1, 2 * nitems + nparams + 1] the first item of
 *   every parameter (last entry = nitems).  Items lie in arena order inside one parameter each, at most 1024 float4 long.
 * hyp: the hamt_adamw_table table, {lr, s*lr (RAdam step size times lr), weight_decay, active}; only columns 1 and 3 are read.
 * rl (DEVICE, nparams x 4 floats): {N_sma >= 5 (1 / 0), Lookahead action (0 none, 1 create the slow weights, 2 interpolate), alpha,
 *   -weight_decay*lr}.  partials: 2 floats per item (scratch).  stats (DEVICE, nparams x 4 floats): {weight_norm, adam_norm,
 *   trust_ratio, 0} of every active parameter after the call (inactive rows are left as they are).
 * Parameters with active == 0 are not touched at all (p, g, m, v, slow, p16, stats).  slow may be NULL (no Lookahead: every action
 * is then ignored); p16 may be NULL.  g is zeroed where active == 1 and zero_grad != 0. */
int hamt_ralamb_table(float* p, float* g, float* m, float* v, void* p16, float* slow, const int* items, int nitems,
                      const float* hyp, const float* rl, int nparams, float* partials, float* stats, const float* gnorm_sq,
                      float max_norm, float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps,
                      int zero_grad, void* stream);
/* The three passes of hamt_ralamb_table as calls of their own, passes 1 and 3 over the items [item_first, item_first + item_count)
 * only (p, g, m, v, p16, slow, partials point at the START of their arenas: the item table holds arena offsets; `items`, `hyp`, `rl`
 * still describe the whole arena): a rank of a sharded optimizer runs them over the items it owns (parallel.ShardedItemSync) and
 * hamt_ralamb_trust over all parameters, once the ranks have summed their partial slots.
 *   hamt_ralamb_moments_items: m, v (and g where it is zeroed) of the range's items and the partial slots of exactly those items.
 *   hamt_ralamb_trust: stats of every active parameter from all nitems partial slots, in the fixed order of hamt_ralamb_table.
 *   hamt_ralamb_apply_items: p, slow and p16 of the range's items, with the trust ratios in `stats`.
 * Nothing outside the range's items' elements and partial slots is read or written (the tables apart), and an item's result does not
 * depend on the range it is run in: disjoint item ranges that cover [0, nitems), in any order, with hamt_ralamb_trust between the last
 * moments call and the first apply call, give bit for bit what one hamt_ralamb_table launch gives with the same item table
 * (tests/test_gpu_ralamb_items.py::test_union_of_item_ranges_is_the_whole).  A range that does not lie inside [0, nitems], a NULL arena
 * or table and a misaligned one are HAMT_ERR_ARG and nothing is launched; item_count == 0 is HAMT_OK and launches nothing.  The item
 * table may cut a parameter into more items than 1024-float4 chunking needs (optim.rangerlars.item_table `cuts`): no item straddles a
 * boundary between two owners. */
int hamt_ralamb_moments_items(float* p, float* g, float* m, float* v, const int* items, int nitems, int item_first, int item_count,
                              const float* hyp, const float* rl, int nparams, float* partials, const float* gnorm_sq, float max_norm,
                              float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float eps, int zero_grad,
                              void* stream);
int hamt_ralamb_trust(const int* items, int nitems, const float* hyp, int nparams, const float* partials, float* stats, void* stream);
int hamt_ralamb_apply_items(float* p, const float* m, const float* v, void* p16, float* slow, const int* items, int nitems,
                            int item_first, int item_count, const float* hyp, const float* rl, int nparams, const float* stats,
                            float eps, void* stream);
/* torch.optim's AdamW / Adam / RMSprop (momentum 0, not centered) / SGD (momentum 0): the finetune agents' optimisers
 * (finetune_src/r2r/agent_cmt.py:62-77), one launch over the whole arena with hamt_adamw_table's `ends` table, flags, clip and sweep.
 * Per element, gg = g * min(1, max_norm / (sqrt(*gnorm_sq) + 1e-6)) (1 when gnorm_sq is NULL or max_norm <= 0), t the parameter's own step:
 *   ADAMW    p *= 1 - lr*wd;  m = b1 m + (1-b1) gg;  v = b2 v + (1-b2) gg^2;  p -= (lr / (1-b1^t)) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
 *   ADAM     gg += wd*p;  then ADAMW's moments and update, without the multiplicative decay
 *   RMSPROP  gg += wd*p;  v = alpha v + (1-alpha) gg^2 (alpha is passed as beta2);  p -= lr * gg / (sqrt(v) + eps);  m is not touched
 *   SGD      gg += wd*p;  p -= lr * gg;  m and v are not touched
 * hyp (DEVICE, nparams x 4 floats): {lr, lr / (1-b1^t), weight_decay, active} -- hamt_adamw_table's layout and flags, the table
 *   hamt_sumsq_table reads.  aux (DEVICE, nparams x 4 floats): {1 / sqrt(1-b2^t), 1 - lr*wd, 0, 0}.  The host forms every entry in
 *   float64 and rounds once.  An arena its rule does not touch may be NULL; a NULL arena the rule needs, an unknown rule, NULL
 *   ends / hyp / aux and n % 4 != 0 are HAMT_ERR_ARG and nothing is launched.  p16 may be NULL. */
typedef enum { HAMT_OPT_ADAMW = 0, HAMT_OPT_ADAM = 1, HAMT_OPT_RMSPROP = 2, HAMT_OPT_SGD = 3 } hamt_opt_rule;
int hamt_optim_table(int rule, size_t n, float* p, float* g, float* m, float* v, void* p16, const int* ends, const float* hyp,
                     const float* aux, int nparams, const float* gnorm_sq, float max_norm, float beta1, float beta2, float eps,
                     int zero_grad, void* stream);
/* g *= min(1, max_norm / (sqrt(*gnorm_sq) + 1e-6))  -- standalone clip for torch-optimiser users */
int hamt_clip_scale(size_t n, float* g, const float* gnorm_sq, float max_norm, void* stream);

/* rng[1] += 1 on the stream (new dropout epoch; call once per optimisation step) */
int hamt_rng_advance(uint64_t* rng, void* stream);

/* Range watch on a dense output (csrc/audit.hip): one pass over x [M, N] (row stride ld elements, ld >= N; dtype HAMT_F16, HAMT_BF16 or
 * HAMT_F32) folded into rec, four int64 values in DEVICE memory that the call ADDS to / maximises -- nothing is read back, a caller
 * copies the record out when it wants to look:
 *   rec[0] += elements at half's limit, |x| == 65504 (bits 0x7BFF under the sign); HAMT_F16 only, the other dtypes add 0.  The half store
 *             clamps at +-65504, so every overflow arrives as exactly this value.  A result that legitimately rounds to 65504 is counted
 *             too: the count bounds the clamps from above, and 0 proves there were none.
 *   rec[1] += non-finite elements (exponent field all ones)
 *   rec[2]  = max(rec[2], float32 bit pattern of the largest finite |x|), widened exactly from half / bf16 (non-negative float
 *             patterns order like integers; a record starts at 0)
 *   rec[3] += 1 (calls; M == 0 still counts, and reads nothing)
 * Only the M x N elements named are read: 16 bytes per lane where x and ld * elementsize are 16-byte aligned (a contiguous x counts as
 * one long row), element by element otherwise and for the N % (16 / elementsize) end of a row.  One launch, grid-stride over at most
 * 1024 workgroups; integer atomics only (at most one per field per workgroup, none for a zero contribution), so the record does not
 * depend on scheduling; no scratch.  Null pointers, another dtype, M < 0, N <= 0 or ld < N: HAMT_ERR_ARG, nothing is launched. */
int hamt_range_audit(const void* x, int dtype, int M, int N, int64_t ld, int64_t* rec, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* HAMT_H */
