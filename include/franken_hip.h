/* franken_hip.h — C ABI of libfranken_hip.so: the MI355X (gfx950) hot path of the
 * brainformer / GPT-2 decoder training step.
 *
 * The reference (ALVI-Labs/frankenstein) is pure Python on PyTorch: it has no FFI / plugin
 * interface, so each entry point below replaces a *PyTorch op call site* of the reference
 * (file:line given per function, relative to the reference root).  Conventions:
 *   - plain pointers + sizes only (device pointers unless stated), no torch types;
 *   - the library never allocates or frees device memory: outputs and scratch are caller
 *     allocated, scratch size comes from the matching *_workspace_bytes() query;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*; NULL = default stream)
 *     and returns immediately; no host synchronisation inside (graph-capturable);
 *   - return 0 on success, a negative FK_E* code otherwise; fk_last_error() returns a
 *     thread-local message.  Nothing throws across the boundary.
 *   - dtype: FK_F32 (exact-fp32 MFMA parity mode) or FK_BF16 (bf16 operands, fp32 accumulate).
 */
#ifndef FRANKEN_HIP_H
#define FRANKEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FK_VERSION 302

#define FK_OK 0
#define FK_EINVAL (-1)       /* bad shape / dtype / alignment / null pointer */
#define FK_ELAUNCH (-2)      /* hipGetLastError() after launch */
#define FK_EUNSUPPORTED (-3)

enum { FK_F32 = 0, FK_BF16 = 1 };
enum { FK_MASK_NONE = 0, FK_MASK_CAUSAL = 1, FK_MASK_BLOCK_CAUSAL = 2, FK_MASK_PREFIX = 3, FK_MASK_KEYPAD = 4, FK_MASK_DENSE = 5 };
/* fk_attn_* flags.  FK_ATTN_Q_PRESCALED: Q already holds scale * log2(e) * q (written so by fk_gemm_nt_rope's pre-scaled query
 * table), bf16 with D = 64 only: the kernels then work in the exp2 domain with the row constants (running reference maximum,
 * -LSE, -delta) as the initial MFMA accumulators, i.e. without any per-score multiply / subtract.  dQ, dK, dV are the same
 * quantities as without the flag (gradients w.r.t. the UNSCALED q, k, v).                                                  */
enum { FK_ATTN_Q_PRESCALED = 1 };
enum { FK_NORM_LAYER = 0, FK_NORM_RMS = 1 };
enum { FK_ACT_SWIGLU = 0, FK_ACT_GELU = 1 };
enum { FK_GEMV_GELU = 1 };   /* fk_gemv_nt flags */

int fk_version(void);
const char* fk_last_error(void);

/* ---- GEMM (nn.Linear: models/brainformer.py:119-124,141-145,149,171,285,342,501; models/gpt2_model.py:35,37,56,75,82-90,133,205)
 * fk_gemm_nt: C[M,N] = A[M,K] * B[N,K]^T (+ bias[N]) (+ residual[m % res_rows, n]); row-major, ld* in elements.
 *   A,B,bias,residual have `dtype`; C has `out_dtype` (= dtype, or FK_F32).  res_rows = 0 means one residual
 *   row per output row; res_rows = R broadcasts an [R, N] table over rows (the space embedding of
 *   models/brainformer.py:343).  K, lda, ldb multiples of 16 bytes.  Every leading dimension covers its row
 *   (lda, ldb >= K, ldc >= N, ldr >= N; the same for the H13 / G / dH13 buffers of the fused calls below): a
 *   shorter one is refused, whichever kernel the shape would have taken.                                     */
int fk_gemm_nt(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N,
               int64_t K, const void* bias, const void* residual, int64_t ldr, int64_t res_rows, int dtype,
               int out_dtype, void* stream);
/* fk_gemv_nt: the same product for the single-token decode step, 1 <= M <= 16 rows (models/gpt2_model.py:35,37,56,75,82-90,133 at one
 *   new token per sample), as a stream of the weight matrix instead of MFMA tiles, with the step's neighbours folded in:
 *     C[m, n] = act( sum_k LN(A[m, :])[k] * W[n, k] + bias[n] ) + residual[m, n].
 *   W is row-major [N, K] (ldw; the layout of the weight shadows, rows past N are never read); A, W, bias [N], residual [M, N] (ldr)
 *   have `dtype`, C has `out_dtype` (= dtype, or FK_F32).  bias / residual: NULL = absent.  ln_gamma != NULL: LayerNorm over K in
 *   front of the product (F.layer_norm, models/gpt2_model.py:27): gamma / beta fp32 [K], beta may be NULL, statistics and the
 *   normalised row kept in fp32.  flags & FK_GEMV_GELU: act = exact-erf GELU (the function of fk_gelu_fwd), else identity.
 *   Envelope: 1 <= M <= 16 (anything larger is refused, not forwarded), any N >= 1 (no multiple required), K a multiple of 16 bytes
 *   (8 bf16 / 4 fp32), every leading dimension covers its row, A and W rows 16-byte aligned, sizes within int32.
 *   fp32 accumulation; deterministic (no split over workgroups, no atomics, no workspace), and batch invariant: row m of the result
 *   does not depend on M, so a sample decodes to the same bits alone or in a batch.                                              */
int fk_gemv_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
               const void* bias, const void* residual, int64_t ldr, const float* ln_gamma, const float* ln_beta, float ln_eps,
               int flags, int dtype, int out_dtype, void* stream);
/* fk_gemm_nt_rope: fk_gemm_nt (+ bias) with apply_rope (models/brainformer.py:70-91) fused into the epilogue: the first
 * rot_cols output columns (q and k of a packed q|k|v projection, heads of width D) of row m are rotated by
 * table[m / T][pos_off + m % T][(n % D) / 2] = (cos, sin)  (table_bs = 0: one cache shared by all samples).
 * The first q_cols columns (the queries; 0 = none) take their pairs from table + q_table_off floats instead: a second copy
 * of the cache multiplied by softmax_scale * log2(e), which hands Q to fk_attn_* in the FK_ATTN_Q_PRESCALED form with a
 * single rounding (models/brainformer.py:153-168: the 1/sqrt(dh) of SDPA folded into the rotation).                      */
int fk_gemm_nt_rope(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N,
                    int64_t K, const void* bias, const float* table, int64_t table_bs, int64_t T, int64_t pos_off, int64_t D,
                    int64_t rot_cols, int64_t q_cols, int64_t q_table_off, int dtype, void* stream);
/* SwiGLU MLP fused into the projection epilogues (models/brainformer.py:124 and its autograd).  Hidden units use the
 * INTERLEAVED layout: for every 4 hidden units, 4 columns of h1 = w1 x followed by 4 columns of h3 = w3 x (W13 rows are
 * packed the same way, see fk_cast_pack_rows).
 *   fk_gemm_nt_swiglu : H13[M,2H] = A[M,K] * W13[2H,K]^T   and   G[M,H] = silu(h1) * h3        (one pass, G never re-read)
 *   fk_gemm_nt_dswiglu: dg = dY[M,K] * W2T[H,K]^T (never stored);  dH13[M,2H] = d(silu(h1) h3)/d(h1,h3) * dg         */
int fk_gemm_nt_swiglu(const void* A, int64_t lda, const void* W13, int64_t ldb, void* H13, int64_t ldh, void* G,
                      int64_t ldg, int64_t M, int64_t H, int64_t K, int dtype, void* stream);
int fk_gemm_nt_dswiglu(const void* dY, int64_t lda, const void* W2T, int64_t ldb, const void* H13, int64_t ldh, void* dH13,
                       int64_t lddh, int64_t M, int64_t H, int64_t K, int dtype, void* stream);
/* fk_mlp_bwd_fused (ABI 302): the two calls above that make up the data-gradient chain of the SwiGLU MLP's backward
 *   (autograd of models/brainformer.py:119-124) as ONE launch:   dg = dY W2T^T (never stored),   dH13 = SwiGLU'(H13) * dg (written once, for
 *   the weight gradients),   dX[M,D] = dH13 W13T^T with dH13 taken from registers instead of being read back.  bf16, D = 384, H % 32 == 0;
 *   W2T [H, D] and W13T [D, 2H] are the transposed shadows the two separate calls take.  Results are bit-identical to
 *   fk_gemm_nt_dswiglu followed by fk_gemm_nt (same products, operand slots and summation order).                        */
int fk_mlp_bwd_fused(const void* dY, int64_t lddy, const void* W2T, int64_t ldw2t, const void* H13, int64_t ldh, const void* W13T,
                     int64_t ldw13t, void* dH13, int64_t lddh, void* dX, int64_t lddx, int64_t M, int64_t H, int64_t D, int dtype,
                     void* stream);
/* fk_gemm_nt_route: which kernel fk_gemm_nt and its fused forms run for a problem (host only, nothing is launched): one of the
 *   FK_NT_* values below for bf16 operands, FK_NT_ROUTE_F32 for fp32 operands (always the register-staged kernel).  vec_epi: N, ldc
 *   (and ldr) are multiples of 8 and C (and the residual) 16-byte aligned; mode: 0 plain / bias / residual / RoPE, 1 fk_gemm_nt_swiglu
 *   (N = 2H), 2 fk_gemm_nt_dswiglu (N = H); has_rope: fk_gemm_nt_rope.  The token-on-the-lane kernels that fk_gemm_nt_rope and
 *   fk_gemm_nt_swiglu put in front at K = 384 from 45 825 rows on are not part of the answer (fk_gemm_nt_rope_route /
 *   fk_gemm_nt_swiglu_route below answer for a whole call of those two).  Follows the FK_NT_* environment knobs
 *   exactly as the launch does.                                                                                                    */
enum { FK_NT_RING2 = 0, FK_NT_RING192 = 1, FK_NT_RING128 = 2, FK_NT_BIG = 3, FK_NT_GLDS4 = 4, FK_NT_GLDS = 5, FK_NT_STAGED = 6, FK_NT_LANE = 7 };
#define FK_NT_ROUTE_F32 (-2)
int fk_gemm_nt_route(int64_t M, int64_t N, int64_t K, int dtype, int vec_epi, int mode, int has_rope);
/* fk_gemm_nt_rope_route / fk_gemm_nt_swiglu_route: the whole answer for a call of fk_gemm_nt_rope / fk_gemm_nt_swiglu (host only, nothing
 *   is launched): FK_NT_LANE where the entry point hands the call to a token-on-the-lane kernel (bf16, K = 384, 256-token workgroups that
 *   fill at least 70 % of their rounds of 256, i.e. 45 825 .. 65 536 rows, 91 649 .. 131 072, ...; H % 32 == 0, or N % 64 == 0 with D = 64,
 *   rot_cols % 64 == 0, q_cols % 64 == 0 and no bias; leading dimensions multiples of 8 that cover their rows; pos_off >= 0), else what
 *   fk_gemm_nt_route answers for the tiled form of the call.  align_ok: every pointer of the call (A, the weight, the outputs, the
 *   rotation table) is non-null and 16-byte aligned.  The entry points decide with the same functions.                              */
int fk_gemm_nt_rope_route(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int has_bias, int64_t T, int64_t pos_off,
                          int64_t D, int64_t rot_cols, int64_t q_cols, int align_ok, int dtype);
int fk_gemm_nt_swiglu_route(int64_t M, int64_t H, int64_t K, int64_t lda, int64_t ldb, int64_t ldh, int64_t ldg, int align_ok, int dtype);
/* fk_mlp_bwd_fused_route: which of its two kernels fk_mlp_bwd_fused runs (host only): FK_MLP_BWD_ASM, the generated-stream kernel, for
 *   whole 128-token tiles whose dH13 rows are addressable with 32-bit byte offsets (M % 128 == 0 and M * lddh * 2 < 2^32), else
 *   FK_MLP_BWD_HIPCC, the kernel hipcc schedules.                                                                                   */
enum { FK_MLP_BWD_HIPCC = 0, FK_MLP_BWD_ASM = 1 };
int fk_mlp_bwd_fused_route(int64_t M, int64_t lddh);
/* fk_gemm_tn: C[N1,N2] (fp32) (+)= sum_m A[m,N1] * B[m,N2]  — the weight gradient dW = dY^T X of a Linear
 *   (autograd of the call sites above).  Split over m with deterministic slab reduction.                     */
size_t fk_gemm_tn_workspace_bytes(int64_t M, int64_t N1, int64_t N2, int dtype);
int fk_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N1,
               int64_t N2, int accumulate, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* fk_gemm_tn_swiglu: the gradient of a SwiGLU-interleaved W13 ([2H, N2]: groups of 4 up rows, 4 gate rows), ADDED to the two plain
 *   gradients: d_up[(r / 8) * 4 + r % 4] += row r for r % 8 < 4, d_gate likewise for r % 8 >= 4 (both [H, N2] fp32, leading dimension
 *   ldc).  The slab reduction writes both (slabs summed in order, then + destination: the bits of fk_gemm_tn into a temporary followed
 *   by fk_add2d).  Needs a split plan (fk_gemm_tn_route(M, 2H, N2): nsplit > 1) and 16-byte aligned destinations with N2 % 4 == 0,
 *   ldc % 4 == 0; workspace as for fk_gemm_tn(M, 2H, N2).                                                                          */
int fk_gemm_tn_swiglu(const void* A, int64_t lda, const void* B, int64_t ldb, float* d_up, float* d_gate, int64_t ldc, int64_t M,
                      int64_t H, int64_t N2, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* fk_gemm_tn_route: what fk_gemm_tn does with a shape (host only): returns 0 for the 128 x 128 kernel, 128 or 192 for the large-tile
 *   kernel (its B columns per tile); *nsplit = the number of row splits (slabs summed in order when > 1), *rows_per_split = the rows
 *   of a split: split s covers rows [s * rows_per_split, min(M, (s + 1) * rows_per_split)), which may be empty.  Either may be NULL. */
int fk_gemm_tn_route(int64_t M, int64_t N1, int64_t N2, int dtype, int* nsplit, int64_t* rows_per_split);
/* fk_colsum: out[c] (+)= sum_r X[r,c]  (bias / space-embedding gradients).                                   */
size_t fk_colsum_workspace_bytes(int64_t rows, int64_t cols);
int fk_colsum(const void* X, int64_t ld, float* out, int64_t rows, int64_t cols, int accumulate, int dtype,
              void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused attention (F.scaled_dot_product_attention: models/brainformer.py:168,215; models/gpt2_model.py:64)
 * Q,K,V,O are [B, N, H, D] views: element (b,n,h,d) at base + b*bs + n*rs + h*D + d.  LSE [B,H,Nq] fp32.
 * mask: NONE | CAUSAL (k + k_off <= q + q_off) | BLOCK_CAUSAL ((k + k_off)/mask_c <= (q + q_off)/mask_c), the
 * analytic form of build_advanced_causal_mask (models/brainformer.py:93-111) incl. the [-t_q:, -t_k:] slice (:160-162).
 * PREFIX (per-sample masks of sorted token subsets, MAE's get_sub_att_matrix models/brainformer.py:392-413):
 * visible(q,k) = k < limits[b,q] <=> q >= qfirst[b,k], int32 tables from fk_prefix_mask.
 * KEYPAD (padding mask of models/simple_mae:228-236,349-352): visible(q,k) = limits[b,q] != 0 && qfirst[b,k] != 0, i.e. the two
 * int32 tables are the query / key validity flags (FK_ATTN_Q_PRESCALED kernels: the tiles in front of a sample's first zero key flag
 * take the mask-free path, same bits).  DENSE (any boolean mask: models/brainformer.py:160-168 passes whatever it is given):
 * `limits` points to uint8 [Bm, Hm, Nq, Nk] (non-zero = attend), mask_c = its batch stride and q_off its head stride in elements (0: one
 * mask for every sample / every head), k_off = 0, qfirst unused; every tile takes the per-element path of the generic kernels
 * (FK_ATTN_Q_PRESCALED is refused).
 * Fully masked rows give 0.  D in {8,16,32,64} (+128 for bf16).  Backward: dO shares O's strides, dQ/dK/dV share Q/K/V's strides; delta_ws
 * is fp32 scratch of 2 * B * H * roundup(Nq, 64) floats (the row statistics the dQ kernel hands to the dK/dV kernel).  rope_table != NULL
 * (self-attention only) additionally applies the inverse RoPE (rotation by -angle at position rope_off + index) to dQ and dK as they are
 * stored = apply_rope's backward.
 * *_dropout: the same with dropout on the attention probabilities (F.scaled_dot_product_attention(dropout_p=...) in training mode,
 * models/gpt2_model.py:64): softmax over all visible keys, then entries dropped with probability drop_p and the kept ones scaled by
 * 1 / (1 - drop_p).  No mask is stored: forward and backward regenerate it from (drop_seed[0..1] in DEVICE memory, drop_site, b, h, q, k)
 * — see fk_dropout.  drop_p == 0: identical to the plain entry points.  Generic kernels only (FK_ATTN_Q_PRESCALED is refused).            */
int fk_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int64_t B, int64_t H, int64_t Nq,
                int64_t Nk, int64_t D, int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs,
                int64_t v_rs, int64_t o_bs, int64_t o_rs, int mask_kind, int64_t mask_c, int64_t q_off, int64_t k_off,
                const int32_t* limits, const int32_t* qfirst, float scale, int flags, int dtype, void* stream);
int fk_attn_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                void* dQ, void* dK, void* dV, float* delta_ws, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t D,
                int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, int64_t o_bs,
                int64_t o_rs, int mask_kind, int64_t mask_c, int64_t q_off, int64_t k_off, const int32_t* limits,
                const int32_t* qfirst, float scale, const float* rope_table, int64_t rope_bs, int64_t rope_off, int flags,
                int dtype, void* stream);

int fk_attn_fwd_dropout(const void* Q, const void* K, const void* V, void* O, float* LSE, int64_t B, int64_t H, int64_t Nq,
                        int64_t Nk, int64_t D, int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs,
                        int64_t v_rs, int64_t o_bs, int64_t o_rs, int mask_kind, int64_t mask_c, int64_t q_off, int64_t k_off,
                        const int32_t* limits, const int32_t* qfirst, float scale, int flags, float drop_p, const uint32_t* drop_seed,
                        uint32_t drop_site, int dtype, void* stream);
int fk_attn_bwd_dropout(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                        void* dQ, void* dK, void* dV, float* delta_ws, int64_t B, int64_t H, int64_t Nq, int64_t Nk, int64_t D,
                        int64_t q_bs, int64_t q_rs, int64_t k_bs, int64_t k_rs, int64_t v_bs, int64_t v_rs, int64_t o_bs,
                        int64_t o_rs, int mask_kind, int64_t mask_c, int64_t q_off, int64_t k_off, const int32_t* limits,
                        const int32_t* qfirst, float scale, const float* rope_table, int64_t rope_bs, int64_t rope_off, int flags,
                        float drop_p, const uint32_t* drop_seed, uint32_t drop_site, int dtype, void* stream);
/* fk_attn_route: which kernels fk_attn_fwd / fk_attn_bwd (and their *_dropout forms) run for a problem (host only, nothing is launched;
 *   the launchers ask the same function).  Takes everything the decision reads: Nq, Nk, D, dtype, the mask (kind, mask_c, q_off, k_off as
 *   in the calls above; for FK_MASK_DENSE mask_c / q_off are the table strides), flags, has_dropout (drop_p != 0) and has_rope (a
 *   rope_table is given to the backward).  Writes the forward, dQ and dK/dV kernels (any of the three pointers may be NULL):
 *   GENERIC = the kernels for every dtype / head_dim / mask; FEWQ = the waves split the keys (Nq <= 32, Nk >= 1024, no mask, no dropout;
 *   the dQ form also needs no RoPE table); PS = the FK_ATTN_Q_PRESCALED tile loops; ASM = the generated instruction streams (every tile
 *   fully visible and aligned); DKDVW_ASM = the stream with 64 keys per wave.  Returns FK_OK, or FK_EINVAL for a problem the entry
 *   points refuse.                                                                                                                    */
enum { FK_ATTN_FWD_GENERIC = 0, FK_ATTN_FWD_FEWQ = 1, FK_ATTN_FWD_PS = 2, FK_ATTN_FWD_ASM = 3 };
enum { FK_ATTN_DQ_GENERIC = 0, FK_ATTN_DQ_FEWQ = 1, FK_ATTN_DQ_PS = 2, FK_ATTN_DQ_ASM = 3 };
enum { FK_ATTN_DKDV_GENERIC = 0, FK_ATTN_DKDV_PS = 1, FK_ATTN_DKDV_ASM = 2, FK_ATTN_DKDVW_ASM = 3 };
int fk_attn_route(int64_t Nq, int64_t Nk, int64_t D, int dtype, int mask_kind, int64_t mask_c, int64_t q_off, int64_t k_off, int flags,
                  int has_dropout, int has_rope, int* fwd, int* dq, int* dkdv);

/* ---- dropout (nn.Dropout in training mode: models/gpt2_model.py:40,75 resid_dropout, :85,91 MLP, :129 embeddings).
 *      y[i] = (res ? res[i] : 0) + (keep(i) ? x[i] / (1 - p) : 0), n contiguous elements (multiple of 16 bytes), y may alias x.  The backward
 *      is the same call on dy without res.  keep(i) is a counter-based decision, nothing is stored:
 *        bits = mix32(mix32(mix32(hi ^ seed[0]) + seed[1] * 0x85EBCA6B + site) ^ (lo * 0x9E3779B9)),  keep <=> bits >= p * 2^32,
 *      (step and site go THROUGH a mixer round, so the masks of two sites or steps are not shifted copies of one another),
 *      mix32 = lowbias32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16), (hi, lo) = the two words of i (for
 *      attention probabilities: hi = (b * H + h) * Nq + q, lo = k).  seed[0] = the run's seed, seed[1] = a step counter the caller advances
 *      once per forward — both read from DEVICE memory so that a captured graph draws a new mask on every replay; `site` numbers the
 *      dropout applications within one forward.  The stream is the library's own (torch's CPU and CUDA dropout streams differ too).     */
int fk_dropout(const void* x, const void* res, void* y, int64_t n, float p, const uint32_t* seed, uint32_t site, int dtype, void* stream);

/* ---- normalisation (nn.LayerNorm: models/brainformer.py:237,239,252,254,287,500; F.layer_norm models/gpt2_model.py:27;
 *      RMSNorm models/brainformer.py:221-232).  x,y [rows, dim] contiguous; gamma/beta fp32 (beta may be NULL);
 *      mean/rstd fp32 [rows] saved for backward (mean unused for RMS).                                        */
int fk_norm_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                int64_t rows, int64_t dim, float eps, int kind, int dtype, void* stream);
/* dx = (dres ? dres : 0) + norm_bwd(dy); dgamma/dbeta (fp32, +=  when accumulate) via workspace partials;
 *      mean may be NULL for FK_NORM_RMS only (a NULL mean with FK_NORM_LAYER is refused).                      */
size_t fk_norm_bwd_workspace_bytes(int64_t rows, int64_t dim);
int fk_norm_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                const void* dres, void* dx, float* dgamma, float* dbeta, int64_t rows, int64_t dim, int kind,
                int accumulate, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- RoPE (apply_rope, models/brainformer.py:70-91): in place on the first n_rot_heads*D columns of each row of
 *      x [B, T, ld]; interleaved pairs rotated by table[(pos_off + t)] ([.., D/2, 2] fp32 = (cos, sin), i.e.
 *      torch.view_as_real of the reference's complex cache); table_bs = 0 for a shared 2-D cache, else the per-sample
 *      stride of a 3-D cache.  conj != 0 rotates by -angle (the backward).                                     */
int fk_rope(void* x, int64_t B, int64_t T, int64_t ld, int64_t nheads, int64_t D, const float* table, int64_t table_bs,
            int64_t pos_off, int conj, int dtype, void* stream);

/* ---- patch tokeniser (Rearrange 'b (t p1) c -> b (t c) p1', models/brainformer.py:282,338): x fp32 [B,T,C] ->
 *      tok [B*(T/P)*C, ldp] in `dtype`, columns >= P zero-filled (ldp >= P, multiple of 16 bytes).              */
int fk_patchify(const float* x, void* tok, int64_t B, int64_t T, int64_t C, int64_t P, int64_t ldp, int dtype,
                void* stream);

/* ---- gated / pointwise MLP activations.  SwiGLU (models/brainformer.py:124): h13 [rows, 2*H] = [w1 x | w3 x],
 *      g = silu(h1) * h3.  GELU exact erf (models/gpt2_model.py:83,89).                                        */
int fk_swiglu_fwd(const void* h13, void* g, int64_t rows, int64_t H, int dtype, void* stream);
int fk_swiglu_bwd(const void* h13, const void* dg, void* dh13, int64_t rows, int64_t H, int dtype, void* stream);
int fk_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);
int fk_gelu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, void* stream);

/* ---- dtype / layout plumbing for weight shadows: dst[r*ldd + c] = src[r*lds + c] (or transposed: dst[c*ldd + r]).*/
int fk_cast_pack(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int transpose,
                 int dtype, void* stream);
/* same with a row map: source row j lands in destination row (j / rblk) * rstride + j % rblk + roff (rblk = 0: identity). */
int fk_cast_pack_rows(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int transpose,
                      int64_t rblk, int64_t rstride, int64_t roff, int dtype, void* stream);
/* many fk_cast_pack_rows jobs in ONE launch: the per-step refresh of every weight shadow after the optimizer update
 * (replaces ~150 tiny launches).  `jobs` is a DEVICE array; job j owns the chunks [chunk_begin, next job's chunk_begin):
 * ceil(rows*cols / 1024) chunks of 1024 consecutive elements for a plain job, ceil(rows/32) * ceil(cols/32) tiles of 32 x 32 source
 * elements for a transposed one; total_chunks = end of the last job.                                                  */
typedef struct fk_pack_job {
  const float* src; void* dst; int64_t lds, ldd;
  int32_t rows, cols, transpose, rblk, rstride, roff;
  int64_t chunk_begin;
} fk_pack_job;
int fk_cast_pack_multi(const fk_pack_job* jobs, int64_t njobs, int64_t total_chunks, int dtype, void* stream);
int fk_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);
/* y = a + b (same dtype) */
int fk_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);

/* fk_attn_combine: split-key attention.  A few queries against a long context (the perceiver's 32 learnable queries x 6144 tokens,
 * models/brainformer.py:204-215) fill the chip only when the KEYS are split over workgroups: the caller runs fk_attn_fwd / fk_attn_bwd on
 * views with the S key ranges folded into the batch dimension (queries replicated) and combines the partial results here.
 * parts [B, S, T, H, D]; lse_parts [B, S, H, T] or NULL.  With lse_parts (forward): out[b] = sum_s softmax_s(lse_parts)[s] * parts[b, s] and
 * lse_out [B, H, T] = log sum_s exp(lse_parts) (nullable).  Without (query gradient, already normalised by the global LSE): out = sum_s parts. */
int fk_attn_combine(const void* parts, const float* lse_parts, void* out, float* lse_out, int64_t B, int64_t S, int64_t T, int64_t H,
                    int64_t D, int dtype, void* stream);

/* ---- single-token decode step with the position on the DEVICE (`pos`: int32[1]), so one captured hipGraph serves every new token
 * of GPT.generate (models/gpt2_model.py:328-353; the reference re-forwards the whole sequence per token).
 * fk_gpt_embed_step: out[b,:] = wte[idx[b],:] + wpe[*pos,:].   fk_kv_append: kv[b, *pos, :] = qkv[b, d:3d] (kv [B, tmax, 2d]).
 * fk_attn_decode: o[b,h,:] = softmax_j(q[b,h,:] . k[b,j,h,:] * scale) v[b,j,h,:] over j = 0..*pos; k at kv + b*kv_bs + j*kv_rs + h*D,
 * v = k + H*D; strides in elements.                                                                                    */
int fk_gpt_embed_step(const int64_t* idx, const float* wte, const float* wpe, const int32_t* pos, void* out, int64_t B, int64_t dim,
                      int64_t vocab, int dtype, void* stream);
int fk_kv_append(const void* qkv, void* kv, const int32_t* pos, int64_t B, int64_t d, int64_t tmax, int dtype, void* stream);
int fk_attn_decode(const void* q, int64_t q_bs, const void* kv, int64_t kv_bs, int64_t kv_rs, void* out, int64_t o_bs, const int32_t* pos,
                   int64_t B, int64_t H, int64_t D, float scale, int dtype, void* stream);
/* fk_sample_topk: the sampling tail of GPT.generate (models/gpt2_model.py:340-351) as one launch: logits[b,:] / temperature, top-k
 * crop (values below the k-th largest -> -inf; top_k <= 0: none), softmax, ONE multinomial draw per row by inverse CDF with a
 * Philox4x32-10 uniform keyed by (*seed; *step, b).  Writes the token to cur[b] and, if out != NULL and *step < out_cols, to out[b*out_ld + *step] (out is [B, out_cols] with row
 * stride out_ld: a reused state or one graph replay too many cannot write past it; out != NULL needs 0 < out_cols <= out_ld); the last
 * block to finish sets *step += 1 and, if pos_inc != NULL, *pos_inc += 1 (so a captured decode graph advances by itself).  logits fp32,
 * `ticket` a zero-initialised uint32 scratch word owned by the caller.  top_k = 1 is the deterministic argmax (first maximum).
 * The draw is a pure function of (logits, temperature, top_k, *seed, *step, b), and tests/sample_ref.py restates it:
 *   x_i = logits_i * (1.0f / temperature), both operations in fp32; the crop keeps x_i >= the k-th largest x, ties kept (top_k >= V: none);
 *   e_i = exp(x_i - max kept x); the CDF runs in INDEX order and the token is the first index whose cumulative mass exceeds u * total;
 *   u = (c0 >> 8) / 2^24 in [0, 1), c0 = word 0 of Philox4x32-10 with the key (seed lo, seed hi) and the counter
 *   (step lo, step hi, b, 0x5A3C), lo / hi the 32-bit halves of *seed and *step;
 *   an entry without mass (-inf, or a logit that underflows) is never emitted, not even where rounding leaves u * total >= the sum.
 * The sums are fp32 (per-thread chunks of ceil(V / 1024) consecutive indices, then a scan), so a u * total within 2^-17 of the total
 * mass of a boundary between two tokens may fall on either side of it.                                                              */
int fk_sample_topk(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, const uint64_t* seed,
                   int64_t* step, int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket,
                   void* stream);

/* ---- beam search on the key/value caches (models/gpt2_model.py:355-454).  The W beams share one set of caches [W, Tmax, 2d]: slot b
 * holds the rows beam position b wrote, and the int32 ancestry table anc[b*anc_ld + j] names the slot that holds beam b's row j, so
 * reordering the beams rewrites the table and never copies a cache.
 * fk_attn_decode_beam: fk_attn_decode with one query per beam (q + b*q_bs + h*D) whose key row j < *pos is at
 *   kv + slot*kv_bs + j*kv_rs + h*D with slot = anc[b*anc_ld + j] clamped into [0, W) (value at + H*D); the row j == *pos is in slot b,
 *   where fk_kv_append has just written it.  D in {16, 32, 64, 128}; kv 16-byte aligned, kv_bs and kv_rs multiples of 16 bytes.
 * fk_beam_topk: per row r < R of fp32 logits (row stride ld >= V): x = logits / temperature, lp = x - logsumexp(x); the k largest lp in
 *   descending order to top_lp[r*k ..] and their ids to top_id[r*k ..]; equal values by ascending id, and of the values tied with the
 *   k-th the lowest ids are kept.  Deterministic.  1 <= k <= min(64, V), V < 2^31, temperature > 0.
 * fk_beam_select: one step of the stochastic beam search, one block.  Beam i reads row i*row_stride of top_lp / top_id (row_stride = 0:
 *   every beam reads row 0, the first step) and draws W of its k entries without replacement with probability ~ exp(top_lp) by the
 *   Gumbel-top-W rule: key = top_lp[i][j] - logf(-logf(u)), u = ((c0 >> 8) + 0.5) / 2^24 in fp32, c0 = word 0 of Philox4x32-10 keyed by
 *   *seed on the counter (step_lo, step_hi, i, 0xBEA30000 | j); the W largest keys win, larger key = earlier draw rank (ties: lower j).
 *   Of the W*W candidates (score = scores[i] + top_lp[i][j]) the W best survive, ordered by score descending, then parent, then draw
 *   rank.  Writes scores[W], cur[W] (the tokens), parent_log[*step*W ..] / tok_log[*step*W ..] while *step < log_rows, and the ancestry:
 *   for every column j <= *pos (j < anc_ld): anc[b][j] = old[parent[b]][j] with old[x][*pos] = x (*pos < 0: no column).  Then
 *   *step += 1 and, if pos_inc != NULL (it may be pos), *pos_inc += 1.  1 <= W <= 16, W <= k <= 64.                                */
int fk_attn_decode_beam(const void* q, int64_t q_bs, const void* kv, int64_t kv_bs, int64_t kv_rs, const int32_t* anc, int64_t anc_ld, void* out,
                        int64_t o_bs, const int32_t* pos, int64_t W, int64_t H, int64_t D, float scale, int dtype, void* stream);
int fk_beam_topk(const float* logits, int64_t ld, int64_t R, int64_t V, float temperature, int64_t k, float* top_lp, int64_t* top_id, void* stream);
int fk_beam_select(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t W, int64_t k, float* scores, const uint64_t* seed,
                   int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log, int64_t* tok_log, int64_t log_rows,
                   int32_t* anc, int64_t anc_ld, void* stream);

/* ---- the same step for a batch of S sentences with W beams each.  Row r = g*W + b is beam b of sentence g; the caches are [S*W, tmax, 2d]
 * and never reordered; the table is int32 [S*W, tmax] of LOCAL slots in [0, W): row j < *pos of row r lives in cache slot
 * g*W + anc[r*anc_ld + j], its row *pos in slot r.  One *pos and one *step serve all sentences (prompts of equal length).
 * fk_attn_decode_beam_grouped: fk_attn_decode_beam on grid (H, S*W) with slot = g*W + clamp(anc[r][j], 0, W-1), so a corrupt table stays
 *   inside its own sentence; *pos >= min(tmax, anc_ld) counts as the last row.  append != 0 folds fk_kv_append into the launch: qkv is the
 *   [q | k | v] row (3*H*D elements, 16-byte aligned, q_bs a multiple of 16 bytes), block (h, r) writes head h's D keys and D values of
 *   qkv[r] to kv[r, *pos] and uses them as key *pos; append == 0 reads row *pos from the cache.  S >= 1, S*W < 65536, tmax > 0.
 * fk_beam_select_grouped: fk_beam_select with one block per sentence g: beam i of sentence g reads row g*group_stride + i*row_stride of
 *   top_lp / top_id (row_stride = 0: the sentence's one row, the first step; group_stride >= (W-1)*row_stride + k), scores / cur at g*W,
 *   the logs are [log_rows, S, W], the table rows g*W .. g*W+W-1 (local entries, so the update is fk_beam_select's), the Philox key is
 *   seed[g] on the unchanged counter (step_lo, step_hi, i, 0xBEA30000 | j): sentence g draws what a one-sentence call with seed[g] draws.
 *   Every block reads *step and *pos on entry; the last one to finish sets *step += 1, *pos_inc += 1 and *ticket = 0 (`ticket`: a
 *   zero-initialised uint32 word owned by the caller).  Per sentence 1 <= W <= 16, W <= k <= 64.                                     */
int fk_attn_decode_beam_grouped(const void* qkv, int64_t q_bs, void* kv, int64_t kv_bs, int64_t kv_rs, int64_t tmax, const int32_t* anc, int64_t anc_ld,
                                void* out, int64_t o_bs, const int32_t* pos, int64_t S, int64_t W, int64_t H, int64_t D, float scale, int append, int dtype,
                                void* stream);
int fk_beam_select_grouped(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride, int64_t S, int64_t W, int64_t k,
                           float* scores, const uint64_t* seed, int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log,
                           int64_t* tok_log, int64_t log_rows, int32_t* anc, int64_t anc_ld, uint32_t* ticket, void* stream);

/* ---- end-of-text aware decoding.  `eos` is one token id (eos < 0: none; fin / done are then read as 0: nothing is finished and no id
 * below 0 is ever emitted).  Per row r: fin[r] int32 0/1 (the hypothesis has emitted eos),
 * len[r] int32 = its generated tokens so far, eos counted once.  inv_lenpow: fp32 [n_lenpow], entry L = 1 / L^alpha rounded from float64,
 * entry 0 = 1; the kernels only multiply by it, so norm = (score + lp) * inv_lenpow[L] is one fp32 add and one fp32 multiply, and a table
 * of ones (alpha = 0) ranks by the raw score bit for bit.  A length outside the table uses clamp(L, 0, n_lenpow-1).
 * fk_beam_select_eos: fk_beam_select_grouped (S >= 1 blocks, same Philox counters and keys, same draws) with these rules per sentence:
 *   a live beam i proposes its W drawn entries, raw = scores[i] + top_lp[i][pick], L = len[i] + 1; a finished beam proposes ONE candidate,
 *   r = 0: token eos, raw = scores[i], L = len[i].  The W best candidates survive, by norm = raw * inv_lenpow[L] descending, then by
 *   candidate number i*W + r.  Survivor b from (i, r): parent i, scores[b] = raw (the raw sums stay), len[b] = L,
 *   fin[b] = fin[i] || token == eos; cur, logs, table, *step and *pos_inc as in fk_beam_select_grouped (a finished beam keeps feeding eos
 *   and keeps appending its row).  Every block adds its unfinished survivors to *live_acc (atomic); the last block to finish stores the
 *   sum to live[0] and clears *live_acc, beside *step += 1.  With no eos among the tokens and a table of ones every output equals
 *   fk_beam_select_grouped's; a sentence whose beams are all finished is only sorted, and is a fixed point from the next step on.
 *   live_acc: a zero-initialised uint32 word owned by the caller, like ticket.
 * fk_beam_backtrack: the walk through the logs [log_rows, S, W] on the device, one block per sentence, one thread per final beam.
 *   n = min(*step, log_rows); beam b's tokens are tok_log[t][x_t], x_{n-1} = b, x_{t-1} = clamp(parent_log[t][x_t], 0, W-1).  The beams of
 *   a sentence are ranked by scores * inv_lenpow[len] descending, then beam number; rank 0 is the best.  Writes out_ids[(g*W + rank)*out_ld
 *   + t0 + t] for t < n, `pad` into the columns t0+n .. out_cols-1 (columns < t0, the prompt, are the caller's), out_scores[g*W + rank]
 *   (raw) and out_len[g*W + rank].  0 <= t0 <= out_cols <= out_ld; nothing is written at or beyond column out_cols.  A search without
 *   eos passes fin = 0, len = n and a table of ones.
 * fk_sample_topk_eos: fk_sample_topk with a per-row done[b] / len[b]: a done row draws nothing and writes eos to cur[b] / out[b][*step],
 *   every other row draws exactly what fk_sample_topk draws (Philox keyed by *step and b), len[b] += 1, and a row that draws eos becomes
 *   done.  live[0] = rows not done after the step, by the same live_acc / ticket hand-off.                                              */
int fk_beam_select_eos(const float* top_lp, const int64_t* top_id, int64_t row_stride, int64_t group_stride, int64_t S, int64_t W, int64_t k,
                       float* scores, const uint64_t* seed, int64_t* step, const int32_t* pos, int32_t* pos_inc, int64_t* cur, int32_t* parent_log,
                       int64_t* tok_log, int64_t log_rows, int32_t* anc, int64_t anc_ld, uint32_t* ticket, int64_t eos, int32_t* fin, int32_t* len,
                       const float* inv_lenpow, int64_t n_lenpow, uint32_t* live_acc, int32_t* live, void* stream);
int fk_beam_backtrack(const int32_t* parent_log, const int64_t* tok_log, int64_t log_rows, int64_t S, int64_t W, const int64_t* step, const float* scores,
                      const int32_t* len, const float* inv_lenpow, int64_t n_lenpow, int64_t* out_ids, int64_t out_ld, int64_t out_cols, int64_t t0,
                      int64_t pad, float* out_scores, int32_t* out_len, void* stream);
int fk_sample_topk_eos(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, const uint64_t* seed, int64_t* step,
                       int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket, int64_t eos, int32_t* done,
                       int32_t* len, uint32_t* live_acc, int32_t* live, void* stream);

/* ---- nucleus (top-p) sampling in the same one launch.
 * fk_sample_topp: fk_sample_topk_eos's arguments with `float top_p` behind top_k.  The rule, with x_i = logits_i / temperature:
 *   1. The top-k crop comes first and is unchanged: K is the set of i with x_i >= the k-th largest value, ties kept.  K is everything when
 *      top_k is off.
 *   2. e_i = exp(x_i - max_K x) and total = sum over K of e_i.
 *   3. For i in K, mass_gt(i) = sum { e_j : j in K, x_j > x_i } (strictly larger).
 *   4. Token i stays iff mass_gt(i) < top_p * total.
 *   5. The draw is the existing one: inverse CDF in index order over the tokens that stay, with the Philox uniform keyed by
 *      (*seed; *step, row).
 *   So the most likely token always stays; equal logits stay or go together, the same tie rule as the top-k crop; with no tie at the
 *   boundary this is exactly the usual "sorted cumulative probability" rule; top_p applies to the distribution renormalised after the
 *   top-k crop; and a token whose exact |mass_gt / total - top_p| is below 1e-4 may fall on either side, because the kernel uses its own
 *   exponential and its own summation (it sums floor(e_i * 2^32) as 64-bit integers, so the kept set does not depend on the order of
 *   its atomics: the same inputs give the same tokens).  The Philox counter layout is fk_sample_topk's: top_p = 1 draws the tokens
 *   fk_sample_topk (fk_sample_topk_eos) draws with the same seed and step.
 *   done == NULL selects the plain mode (fk_sample_topk's outputs): len, live_acc and live must then be NULL too and eos is ignored.  All
 *   four given selects the end-of-text mode with the rules of fk_sample_topk_eos.  A mixture is refused.  0 < top_p <= 1; NaN is refused. */
int fk_sample_topp(const float* logits, int64_t ld, int64_t B, int64_t V, float temperature, int64_t top_k, float top_p, const uint64_t* seed,
                   int64_t* step, int32_t* pos_inc, int64_t* cur, int64_t* out, int64_t out_ld, int64_t out_cols, uint32_t* ticket, int64_t eos,
                   int32_t* done, int32_t* len, uint32_t* live_acc, int32_t* live, void* stream);

/* ---- rules that depend on the tokens already emitted: repetition penalty, n-gram ban, minimum length.
 * fk_logit_rules rewrites fp32 logits [R, V] (row stride ld >= V; nothing at or behind column V is touched) in place, in front of
 *   fk_sample_topk / _eos / fk_sample_topp or fk_beam_topk, and keeps the token history of every row on the device.  One block per row.
 *   Per row: z = the row's logits, h[0 .. L) = its history (the prompt ids, then the tokens generated so far), g = *step = the number of
 *   generated tokens, L = t0 + g, e = eos (eos < 0: none), p = penalty, inv_p = 1 / p computed in float64 and rounded once to fp32.
 *   The rules run in this order, before any temperature:
 *   1. Repetition.  For every distinct token v in h with 0 <= v < V and v != e:  z[v] = z[v] > 0 ? z[v] * inv_p : z[v] * p, exactly one fp32
 *      multiply; a token that occurs several times is penalised once.  penalty == 1 leaves every logit as it is.
 *   2. n-gram ban, n = ngram >= 1 and L >= n: for every j in [0, L - n] with h[j .. j+n-2] == h[L-n+1 .. L-1] (ids compared as they are),
 *      z[h[j+n-1]] = -inf unless that token is e or outside [0, V).  n = 1 bans every token of h; L < n bans nothing.
 *   3. Minimum length: while g < min_new and 0 <= e < V, z[e] = -inf.
 *   4. A token that 2 or 3 bans is -inf whatever 1 made of it.
 *   History ids outside [0, V) are never used as an index; NaN logits stay NaN unless banned.  e is exempt from 1 and 2 on purpose (a
 *   prompt that is the end-of-text marker itself must not push every sentence away from ending).
 *   The history is int32, row stride hist_ld >= t0 + steps, t0 + steps <= 4096; the caller fills columns [0, t0) of every row of `hist`
 *   with the prompt before step 0 and the kernel appends: at *step > 0 column L - 1 gets cur[r], the token the previous sampling / select
 *   launch wrote (-1 if it lies outside [0, V)), before the rules are applied.
 *   Plain mode (hist2 == NULL and parent_log == NULL): rows never move, row r of `hist` is row r's history.
 *   Beam mode (both given): the rows are S sentences x W beams, r = g*W + b, which fk_beam_select* reorders every step, so two buffers
 *   [S*W, hist_ld] swap by the parity of *step: new = (*step odd ? hist2 : hist), old = the other, and at *step > 0
 *   new[r][:L-1] = old[g*W + clamp(parent_log[(*step-1)*R + r], 0, W-1)][:L-1], new[r][L-1] = cur[r]; no block reads what another block of
 *   the launch writes.  broadcast != 0 is the first step, R = S logits rows: row g uses the history in row g*W of the buffer of the step's
 *   parity and appends nothing (so every row of `hist` holds its sentence's prompt).  parent_log: the int32 [log_rows, S*W] log of the select.
 *   *step < 0, t0 + *step > min(hist_ld, 4096) or (beam mode) *step > log_rows: the launch writes nothing at all, neither history nor logits.
 *   Refused: a null logits / step / cur / hist, hist2 without parent_log or the reverse, R or V out of range, ld < V, a penalty that is
 *   not finite or <= 0, ngram or min_new < 0, hist_ld < t0 + steps, t0 + steps > 4096, W outside 1 .. 16 in beam mode, R not a multiple of W
 *   there (without broadcast), broadcast in plain mode.                                                                             */
int fk_logit_rules(float* logits, int64_t ld, int64_t R, int64_t V, float penalty, int64_t ngram, int64_t min_new, int64_t eos, const int64_t* step,
                   const int64_t* cur, int32_t* hist, int32_t* hist2, int64_t hist_ld, int64_t t0, int64_t steps, const int32_t* parent_log,
                   int64_t log_rows, int64_t W, int broadcast, void* stream);

/* ---- VQ-VAE tokenizer convolutions (models/vq_brain.py), channels-last [B, T, C], causal left padding dil*(K-1):
 * fk_im2col1d: cols[b, t, k, :] = x[b, t*stride + k*dil - pad, :] (zeros outside), Tout = (T-1)/stride + 1, so that
 *   CausalConv1d (:22-28) = fk_gemm_nt(cols, W') with W'[o, k*Cin + c] = W[o, c, k], and CausalConvTranspose1d(kernel 2s,
 *   stride s, :31-45) = the same with K = 2 taps and s*Cout phase-major output columns viewed as [B, s*T, Cout].
 * fk_col2im1d: adjoint of fk_im2col1d (dx from dcols; gather form, deterministic).   fk_elu_*: nn.ELU().
 * fk_argmax_rows: idx[r] = argmax_c x[r, c] (first on ties): nearest code of the cosine-similarity VQ lookup.          */
int fk_im2col1d(const void* x, void* cols, int64_t B, int64_t T, int64_t Cin, int64_t K, int64_t stride, int64_t dil, int dtype, void* stream);
int fk_col2im1d(const void* dcols, void* dx, int64_t B, int64_t T, int64_t Cin, int64_t K, int64_t stride, int64_t dil, int dtype, void* stream);
int fk_elu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);
int fk_elu_bwd(const void* x, const void* dy, void* dx, int64_t n, int dtype, void* stream);
int fk_argmax_rows(const void* x, int64_t ld, int64_t* idx, int64_t rows, int64_t cols, int dtype, void* stream);

/* ---- input pipeline on device (utils/data_utils.py:115-155 process_signal, :243-267 pad_truncate_brain_list).
 * Trials are packed row-wise: trial i = rows off[i] .. off[i+1]-1 of x [total_rows, C] fp32; block[i] in [0, nblocks) is its
 * recording block.  fk_block_stats: mean / population std per (block, channel) over every row of the block's trials
 * (fp64 accumulation, deterministic; std == 0 -> 1 like :145).  fk_zscore_smooth_pad: out[i, t, :] =
 * gaussian_filter1d((x_i - mean) / std, sigma, axis 0, mode 'reflect', radius 4)[t] for t < min(len_i, Tmax), zeros after
 * (the filter sees the whole trial, truncation to Tmax comes last, as in the reference).                          */
size_t fk_block_stats_workspace_bytes(int64_t ntrials, int64_t C);
int fk_block_stats(const float* x, const int64_t* off, const int32_t* block, int64_t ntrials, int64_t C, int64_t nblocks,
                   float* mean, float* stdv, void* workspace, size_t workspace_bytes, void* stream);
int fk_zscore_smooth_pad(const float* x, const int64_t* off, const int32_t* block, const float* mean, const float* stdv,
                         float* out, int64_t ntrials, int64_t C, int64_t Tmax, double sigma, void* stream);

/* ---- MAE gather / scatter (models/brainformer.py:429-457,468,472): rows of W elements.
 * gather : dst[b, i, :] = src[b, idx[b,i] (% idx_mod), :]     (src_bs = 0 broadcasts one table: embedding / pos-emb lookup)
 * scatter: dst[b, idx[b,i], :] = src[b, i, :]                 dtypes converted on the fly; batch strides in elements.
 * fk_scatter_add_rows: table[idx[r] (% idx_mod), :] += src[r, :] (fp32 atomics; gradient of a broadcast gather).
 * fk_prefix_mask: limits[b,i] = #{j : kid[b,j]/block <= qid[b,i]/block}, qfirst[b,j] = min{i : qid[b,i]/block >= kid[b,j]/block}
 * for ascending per-sample token ids = the analytic form of the gathered block-causal sub-mask.                        */
int fk_gather_rows(const void* src, int64_t src_bs, int src_dtype, const int64_t* idx, int64_t idx_mod, void* dst, int64_t dst_bs,
                   int dst_dtype, int64_t B, int64_t n, int64_t W, int scatter, void* stream);
int fk_scatter_add_rows(const void* src, int src_dtype, const int64_t* idx, int64_t idx_mod, float* table, int64_t rows, int64_t W,
                        void* stream);
int fk_prefix_mask(const int64_t* q_ids, const int64_t* k_ids, int64_t block, int32_t* limits, int32_t* qfirst, int64_t B,
                   int64_t nq, int64_t nk, void* stream);
/* 2-D strided copy (same dtype): dst[r*ldd + c] = src[r*lds + c]. */
int fk_copy2d(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int dtype, void* stream);

/* dst[r, c] += src[r, c] (fp32, strided): accumulates a weight-gradient slab into the flat gradient arena. */
int fk_add2d(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t rows, int64_t cols, void* stream);

/* ---- GPT input embedding (models/gpt2_model.py:183-196): out[b, t, :] = (t < t_ctx ? prefix[b, t, :]
 *      : wte[idx[b, t - t_ctx], :]) + wpe[t, :];  wte/wpe are the fp32 master tables, prefix/out have `dtype`.
 *      Backward of the wte gather: dwte[idx[b, j], :] += dout[b, t_ctx + j, :] (fp32 atomics; dwte is the same
 *      buffer the tied lm_head gradient accumulates into, models/gpt2_model.py:138).                          */
int fk_gpt_embed_fwd(const int64_t* idx, const void* prefix, const float* wte, const float* wpe, void* out, int64_t B,
                     int64_t t_ctx, int64_t t_words, int64_t dim, int64_t vocab, int dtype, void* stream);
int fk_gpt_embed_bwd_wte(const int64_t* idx, const void* dout, float* dwte, int64_t B, int64_t t_ctx, int64_t t_words,
                         int64_t dim, int64_t vocab, int dtype, void* stream);

/* ---- losses.  L1 (F.l1_loss, models/brainformer.py:557) / MSE (F.mse_loss, :473), mean reduction: loss2 fp32[2] = {loss, weight sum};
 *      row_weight (nullable, one weight per row of row_len elements) gives the masked mean of models/simple_mae:393-395;
 *      bwd: dpred = grad_out[0] * d(loss)/d(pred) with grad_out a DEVICE scalar (no host sync).
 *      CE (F.cross_entropy ignore_index mean, models/gpt2_model.py:210; train_brainformer.ipynb cell 3):
 *      logits [rows, V] (ld), targets int64 [rows]; loss2 = {mean nll over valid rows, #valid}; row_lse [rows].  */
size_t fk_loss_workspace_bytes(int64_t n);
int fk_l1_loss_fwd(const void* pred, const void* target, float* loss2, int64_t n, int squared, const float* row_weight,
                   int64_t row_len, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int fk_l1_loss_bwd(const void* pred, const void* target, const float* grad_out, void* dpred, int64_t n, int squared,
                   const float* row_weight, int64_t row_len, const float* loss2, int dtype, void* stream);
size_t fk_ce_workspace_bytes(int64_t rows);
int fk_ce_loss_fwd(const void* logits, int64_t ld, const int64_t* targets, float* loss2, float* row_lse, int64_t rows,
                   int64_t V, int64_t ignore_index, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int fk_ce_loss_bwd(const void* logits, int64_t ld, const int64_t* targets, const float* row_lse, const float* loss2,
                   const float* grad_out, void* dlogits, int64_t ldd, int64_t rows, int64_t V, int64_t ignore_index,
                   int dtype, void* stream);
/* The same loss with the vocabulary processed in CHUNKS, for a head whose [rows, V] logits are never materialised (lm_head + CE of
 * models/gpt2_model.py:205-210 at V = 50257): the caller runs the head GEMM chunk by chunk (fp32 output) and folds every chunk into
 * per-row running statistics; the backward recomputes each chunk and gets its d-logits in the compute dtype (GEMM operand).
 *   fk_ce_chunk_fwd   : merge chunk [rows, cw] (first vocabulary index col0) into row_m / row_s (running max / sum exp) and pick the
 *                       target logit into row_t when the target falls into the chunk; first != 0 initialises the statistics.
 *   fk_ce_chunk_finish: row_lse = row_m + log(row_s); loss2 = {mean nll over valid rows, #valid}  (workspace: fk_ce_workspace_bytes(rows)).
 *   fk_ce_chunk_bwd   : dlogits[rows, cw] = (exp(logit - lse) - onehot) * grad_out / #valid on valid rows and columns < cw_valid, else 0. */
int fk_ce_chunk_fwd(const float* logits, int64_t ld, const int64_t* targets, int64_t col0, float* row_m, float* row_s, float* row_t,
                    int64_t rows, int64_t cw, int first, void* stream);
int fk_ce_chunk_finish(const float* row_m, const float* row_s, const float* row_t, const int64_t* targets, float* row_lse, float* loss2,
                       int64_t rows, int64_t V, int64_t ignore_index, void* workspace, size_t workspace_bytes, void* stream);
int fk_ce_chunk_bwd(const float* logits, int64_t ld, const int64_t* targets, int64_t col0, const float* row_lse, const float* loss2,
                    const float* grad_out, void* dlogits, int64_t ldd, int64_t rows, int64_t cw, int64_t cw_valid, int64_t V,
                    int64_t ignore_index, int dtype, void* stream);

/* ---- vocabulary head + cross entropy as one product each way (csrc/head_ce.hip): lm_head + F.cross_entropy of models/gpt2_model.py:205-210
 *      and the `to_words` head of the notebook CE BrainFormer (notebooks_trainer/train_brainformer.ipynb cell 3) when only the loss is
 *      needed (utils/train_utils.py:138-139).  No [rows, V] tensor in either direction.
 *   fk_head_ce_fwd : row_m / row_s / row_t (running maximum, sum of exponentials, target logit; the inputs of fk_ce_chunk_finish) of
 *                    logits = H W^T (+ bias) straight from the MFMA accumulators.  H [rows, K] (ldh), W [wrows >= V, K] (ldw; rows past V
 *                    may be loaded with a tile but enter no result, whatever they hold), bias [>= V] or NULL in the compute dtype,
 *                    targets int64 [rows]; a target outside [0, V) leaves row_t = 0.  workspace: fk_head_ce_workspace_bytes.
 *   fk_head_ce_bwd : dlT [vpad, rows_pad] (row stride lddl) = TRANSPOSED d-logits, (exp(logit - row_lse) - onehot) * grad_out[0] /
 *                    max(loss2[1], 1) on rows whose target is in [0, V) and != ignore_index and vocabulary entries < V, zero elsewhere
 *                    (the padding feeds GEMMs).  When no row is valid the forward gives loss2 = {NaN, 0} (the mean over nothing, as
 *                    F.cross_entropy); the backward then writes zeros everywhere, dbpart included — the divisor is 1, not the count,
 *                    so that no Inf / NaN reaches the gradient products.
 *                    dH = fk_gemm_tn(dlT, W), dW = fk_gemm_nt(dlT, H^T).  dbpart (nullable): [2 * ceil(rows / 128), vpad] partial column
 *                    sums of the d-logits (bias gradient = their column sum).  rows <= rows_pad <= ceil(rows/128)*128, rows_pad % 4 == 0,
 *                    V <= vpad <= ceil(V/128)*128.
 *   fk_transpose2d : dst[c, r] = src[r, c] (H^T for the product above). */
size_t fk_head_ce_workspace_bytes(int64_t rows, int64_t V);
int fk_head_ce_fwd(const void* H, int64_t ldh, const void* W, int64_t ldw, int64_t wrows, const void* bias, const int64_t* targets,
                   float* row_m, float* row_s, float* row_t, int64_t rows, int64_t V, int64_t K, int dtype, void* workspace,
                   size_t workspace_bytes, void* stream);
int fk_head_ce_bwd(const void* H, int64_t ldh, const void* W, int64_t ldw, int64_t wrows, const void* bias, const int64_t* targets,
                   const float* row_lse, const float* loss2, const float* grad_out, void* dlT, int64_t lddl, int64_t rows_pad,
                   int64_t vpad, float* dbpart, int64_t rows, int64_t V, int64_t K, int64_t ignore_index, int dtype, void* stream);
int fk_transpose2d(const void* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int dtype, void* stream);

/* ---- CTC (csrc/ctc.hip): F.ctc_loss(log_softmax(logits, -1).transpose(0, 1), targets, input_lengths, target_lengths, blank, reduction,
 *      zero_infinity) with the log-softmax folded in, its gradient, and the greedy collapse.  The reference has no CTC: the yardstick is
 *      torch's float64 CPU loss (tests/ctc_ref.py).
 *   logits [B, T, C] fp32 / bf16 (batch stride ldb, row stride ldt >= C, unit column stride); all recursion arithmetic is fp32.
 *   targets int64 [B, Lmax] (row stride ldtgt).  target_lengths int64 [B] or NULL: the number of leading entries that differ from
 *   pad_value (the -100 label padding), counted on the device.  input_lengths int64 [B] or NULL: every sample has T frames.
 *   blank: any class in [0, C).  reduction: FK_CTC_NONE / SUM / MEAN (torch's mean: nll_b / max(L_b, 1) averaged over all B).
 *   Extended states l' = (blank, l_1, blank, ..., l_L, blank), S = 2 L + 1.  fk_ctc_route: FK_CTC_WAVE (2 Lmax + 1 <= 64: one wave, the
 *   state vector in registers), FK_CTC_LDS (2 Lmax + 1 <= 511: one workgroup, the state vector in LDS), FK_EINVAL beyond; no launch.
 *   fk_ctc_loss_fwd: row_lse [B T]; nll [B] (+inf for a sample without alignment, T_b < L_b + adjacent repeats; 0 under zero_infinity);
 *     loss2 = {reduced loss (the sum for FK_CTC_NONE), B}.  want_lattice != 0 runs the beta recursion beside the alpha recursion and
 *     leaves what fk_ctc_loss_bwd reads in the workspace: alpha and beta, fp32 [B, T, S_pad] with S_pad = 2 Lmax + 1 rounded up to a
 *     multiple of 64, log-domain, both including the frame's own log-probability (alpha_t(s) + beta_t(s) - lp_t(l'_s) sums to -nll at
 *     every t < T_b; states s >= 2 L_b + 1 hold -inf; frames t >= T_b are not written), the clamped lengths and classes, and per label
 *     the chain of its states.  workspace: fk_ctc_workspace_bytes(B, T, Lmax) with the lattice, fk_ctc_workspace_bytes(B, 0, Lmax) without.
 *   fk_ctc_loss_bwd: dlogits[b,t,c] = g_b (exp(logit - lse) - exp(logsumexp_{s: l'_s = c}(alpha_t(s) + beta_t(s)) + nll_b - (logit - lse)))
 *     with g_b from the DEVICE-resident grad_out (a scalar for SUM / MEAN, [B] for NONE; the reduction's factor is applied here).  Rows
 *     t >= T_b are exactly 0; every row of a sample without alignment is 0 under zero_infinity (NaN without, as torch's).  The states of
 *     one class are summed in a fixed order, no atomics: nll, loss2 and dlogits are the same bits every run.  Takes the workspace of
 *     the forward (same B, T, Lmax).
 *   Clamped on the device, so that every access stays inside the buffers: input_length into [0, T], target_length into [0, Lmax], a
 *     label into [0, C) and off the blank (label == blank becomes blank - 1, or 1 when blank is 0); the loss of a clamped label is
 *     meaningless but defined.
 *   fk_ctc_collapse: greedy decoding of the per-frame argmax int64 [B, T] (fk_argmax_rows): repeated frames merged, blanks dropped,
 *     order kept ("a _ a" -> "a a", "a a _" -> "a"); ids int64 [B, T] padded with `pad`, lengths int64 [B].                          */
#define FK_CTC_WAVE 0
#define FK_CTC_LDS 1
#define FK_CTC_NONE 0
#define FK_CTC_SUM 1
#define FK_CTC_MEAN 2
int fk_ctc_route(int64_t Lmax);
size_t fk_ctc_workspace_bytes(int64_t B, int64_t T, int64_t Lmax);
int fk_ctc_loss_fwd(const void* logits, int64_t ldb, int64_t ldt, const int64_t* targets, int64_t ldtgt, const int64_t* input_lengths,
                    const int64_t* target_lengths, int64_t pad_value, float* nll, float* loss2, float* row_lse, int64_t B, int64_t T,
                    int64_t C, int64_t Lmax, int64_t blank, int reduction, int zero_infinity, int want_lattice, int dtype, void* workspace,
                    size_t workspace_bytes, void* stream);
int fk_ctc_loss_bwd(const void* logits, int64_t ldb, int64_t ldt, const float* row_lse, const float* grad_out, void* dlogits, int64_t lddb,
                    int64_t lddt, int64_t B, int64_t T, int64_t C, int64_t Lmax, int64_t blank, int reduction, int zero_infinity, int dtype,
                    const void* workspace, size_t workspace_bytes, void* stream);
int fk_ctc_collapse(const int64_t* argmax, int64_t lda, const int64_t* input_lengths, int64_t* ids, int64_t ldi, int64_t* lengths, int64_t B,
                    int64_t T, int64_t blank, int64_t pad, void* stream);

/* ---- CTC forced alignment (csrc/ctc.hip): the most probable ALIGNMENT of logits [B, T, C] to a given transcript, with label spans and
 *      per-label log-probabilities.  Semantics of this build (tests/ctc_align_ref.py restates them in float64); all arithmetic is fp32.
 *   logits, targets, input_lengths, target_lengths, pad_value, blank: as fk_ctc_loss_fwd, lengths and labels clamped on the device in the
 *   same way.  Per sample: lp_t = log_softmax(logits[b, t, :]) (row_lse as in the loss), l' = (blank, l_1, blank, ..., l_L, blank),
 *   S = 2 L_b + 1.  v_0(0) = lp_0(blank), v_0(1) = lp_0(l_1), every other state -inf; for t >= 1
 *     v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s is odd and l'_s != l'_{s-2}) + lp_t(l'_s)
 *   with a back-pointer to the move that won; on an exact tie the smaller move wins (stay before s-1 before s-2).  The end state is the
 *   better of v_{T_b-1}(S-1) and v_{T_b-1}(S-2), S-1 on an exact tie; score[b] is that value, the log-probability of the single best
 *   alignment (score <= -nll of fk_ctc_loss_fwd), and the path is the back-pointer walk from the end state.
 *   Results (nothing else is written; the padding of a row stride keeps what it held):
 *     score fp32 [B];
 *     path int64 [B, T] (row stride ld_path >= T): the class emitted at frame t; `pad` for t >= T_b;
 *     index int64 [B, T] (ld_index >= T): which label of the target frame t emits, 0 .. L_b - 1; -1 on a blank frame and for t >= T_b;
 *     start, end int64 [B, Lmax] (ld_lab >= Lmax): label i holds the frames [start, end), end > start; -1 / -1 for i >= L_b;
 *     label_lp fp32 [B, Lmax] (ld_lab): the sum of lp_t(l_i) over the label's frames in ascending frame order, one fp32 add a frame; 0 for
 *       i >= L_b.  exp(label_lp / (end - start)) is the label's confidence (geometric mean of its frame posteriors).
 *   index, start, end, label_lp may each be NULL (not written); score and path may not.
 *   A sample without alignment (T_b < L_b + adjacent repeats, T_b = 0 < L_b, or every alignment at -inf): score -inf, path all `pad`, index
 *   all -1, every start = end = -1, label_lp = 0; never NaN.  T_b = 0 = L_b: score 0 and the same empty rows.  L_b = 0: an all-blank path.
 *   Envelope: fk_ctc_loss_fwd's (Lmax <= 255, C >= 2, blank in [0, C), ldt >= C, fp32 / bf16), T < 2^31 - 256; FK_EINVAL beyond, no launch.
 *   workspace: fk_ctc_align_workspace_bytes(B, T, Lmax) (0 outside the envelope): row_lse [B T] and the back-pointers, two bits per
 *   (t, s), uint32 [B, ceil(T / 16), S_pad].  Two launches (the first is fk_ctc_loss_fwd's row_lse), no atomics, the same bits every
 *   run, nothing waits for the host.                                                                                                  */
size_t fk_ctc_align_workspace_bytes(int64_t B, int64_t T, int64_t Lmax);
int fk_ctc_align(const void* logits, int64_t ldb, int64_t ldt, const int64_t* targets, int64_t ldtgt, const int64_t* input_lengths,
                 const int64_t* target_lengths, int64_t pad_value, int64_t B, int64_t T, int64_t C, int64_t Lmax, int64_t blank, int64_t pad,
                 float* score, int64_t* path, int64_t ld_path, int64_t* index, int64_t ld_index, int64_t* start, int64_t* end,
                 float* label_lp, int64_t ld_lab, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC prefix beam search (csrc/ctc.hip): the most probable LABELLINGS of logits [B, T, C] (fp32 / bf16, strides as above), n-best
 *      with scores.  Semantics of this build (tests/ctc_beam_ref.py restates them in float64); all arithmetic is fp32.
 *   A beam is at most W distinct prefixes (tuples of non-blank labels), each with pb / pnb, the log-mass of the alignments of the frames
 *   so far that end in blank / in its last label; total = logaddexp(pb, pnb); it starts as {(): (0, -inf)}.  Per frame t < T_b, with
 *   lp = log_softmax(logits[b, t, :]): the candidates are the min(K, C - 1) non-blank classes with the largest RAW logit (exact
 *   compares, equal logits by ascending class id: fk_beam_topk's rule).  Every prefix p of the beam, last label e, sends
 *     to p:         pb'  += total + lp[blank];   pnb' += pnb + lp[e]  (p non-empty; whether or not e is a candidate)
 *     to p + (c,):  pnb' += (c == e ? pb : total) + lp[c]   for every c that is a candidate OR for which p + (c,) is in the beam
 *   (pruning limits which NEW prefixes are proposed, never the flow of probability between resident prefixes).  The W entries with the
 *   largest total survive, an entry with total -inf never; exact ties: a resident prefix before a new one, then the lower slot /
 *   parent slot (slots are in the order of the last selection), then the better candidate.  The same bits every run; no atomics.
 *   Result: the final beam by total descending, the first nbest: ids int64 [B, nbest, T] (strides ld_ids_b, ld_ids_h >= T) padded with
 *   `pad`, lengths int64 [B, nbest], scores fp32 [B, nbest] = total.  A slot without hypothesis: length 0, score -inf, a row of pad.
 *   A score never exceeds the labelling's true log-probability (-nll of fk_ctc_loss_fwd) and equals it when nothing was pruned.
 *   Envelope: 1 <= W <= 32, 1 <= K <= 32, 1 <= nbest <= W, C >= 2, blank in [0, C), ldt >= C, T W < 2^31 - 1; FK_EINVAL beyond, no
 *   launch.  input_lengths int64 [B] (clamped into [0, T] on the device) or NULL: T frames each.  workspace:
 *   fk_ctc_beam_workspace_bytes(B, T, W, K) (0 outside the envelope): per row row_lse, lp[blank] and the K candidates, per sample a trie
 *   of at most T W + 1 prefixes {parent, label, first child, next sibling}.  Two launches, nothing waits for the host.                */
size_t fk_ctc_beam_workspace_bytes(int64_t B, int64_t T, int64_t W, int64_t K);
int fk_ctc_beam_search(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                       int64_t W, int64_t K, int64_t nbest, int64_t pad, int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths,
                       float* scores, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC prefix beam search with n-gram shallow fusion (csrc/ctc.hip): fk_ctc_beam_search with a backoff n-gram language model inside
 *      the selection.  Semantics of this build (tests/ctc_lm_ref.py restates them in float64); all arithmetic is fp32.
 *   The LM factor of a prefix depends on the prefix alone, so the acoustic recursion (pb, pnb, total, the flow between resident prefixes,
 *   the candidate rule) is EXACTLY fk_ctc_beam_search's.  Only the selection key changes:
 *     key(p) = total(p) + lmw(p);   lmw(()) = 0;   lmw(p + (c,)) = lmw(p) + (lm_weight * ln P_lm(c | p) + length_bonus)
 *   (the product, then the bonus, then the sum, each rounded).  A slot also carries lm(p) = the unweighted sum of ln P_lm and the LM state
 *   of p.  A new prefix gets its term by one look-up (state of its parent slot, its label); a resident prefix keeps its own; a prefix that
 *   returns to the beam gets the same bits (the same sum from the same parent value).  The W entries with the largest key survive, an
 *   entry whose total is -inf never; exact ties as in fk_ctc_beam_search.  The blank is never looked up.  use_eos != 0: the final beam is
 *   put in order once more by key + lm_weight * ln P_lm(</s> | state), equal keys in the order of the last selection, and lm includes
 *   that term.  Result, best first, the first nbest: ids and lengths as fk_ctc_beam_search, am fp32 [B, nbest] = total (the pure CTC mass:
 *   fk_ctc_beam_search's scores), lm fp32 [B, nbest] (unweighted), total fp32 [B, nbest] = the final key.  A slot without hypothesis:
 *   length 0, am = lm = total = -inf, a row of pad.  With lm_weight = 0, length_bonus = 0 and use_eos = 0 ids, lengths and am are
 *   fk_ctc_beam_search's bits.
 *   The model (frankenstein_amd/utils/ngram.py compiles and validates it): an LM token id is a class id, the end of sentence is id C.  A
 *   state is a context that occurs in the model, state 0 the empty context, lm_start_state the state of (<s>,).
 *     lm_table    int32 [lm_cap][4], 16-byte aligned: open addressing, {state, token, bits of the fp32 ln p, next state}, state -1 =
 *                 empty; lm_cap a power of two (>= 2 x entries); the home of (state, token) is fk_ngram_hash(state, token) & (lm_cap - 1)
 *                 with h = state * 0x9E3779B1 ^ token * 0x85EBCA6B; h ^= h >> 15; h *= 0x2C1B3C6D; h ^= h >> 12 (uint32), linear probing;
 *                 lm_max_probe = the largest number of entries a successful look-up reads
 *     lm_bow      fp32 [lm_states] ln of the backoff weight; lm_backoff int32 [lm_states] the state of the context without its first
 *                 symbol (strictly shorter)
 *     lm_uni_lp   fp32 [C + 1], lm_uni_next int32 [C + 1]: state 0, dense
 *   Look-up of (s, c), acc = 0, at most lm_order rounds: s == 0 -> (acc + uni_lp[c], uni_next[c]); else read at most lm_max_probe entries
 *   from the home of (s, c): a hit -> (acc + ln p, next); an empty entry or the last probe -> acc += bow[s], s = backoff[s]; behind the
 *   last round the unigram.  The device cannot check the tables: every loop is bounded by lm_order * lm_max_probe, every state read from a
 *   table is clamped into [0, lm_states), a token into [0, C], a table index by lm_cap - 1.  A malformed table gives wrong scores, never
 *   an unbounded loop or an access outside the tables.
 *   Envelope and workspace of fk_ctc_beam_search (fk_ctc_beam_workspace_bytes; the LM state lives in LDS), and 1 <= lm_order <= 8, lm_cap a
 *   power of two, 1 <= lm_max_probe <= lm_cap, 0 <= lm_start_state < lm_states, finite weights, no null table: FK_EINVAL beyond, no launch.
 *   Two launches (the first is fk_ctc_beam_search's), no atomics, the same bits every run, nothing waits for the host.                  */
uint32_t fk_ngram_hash(uint32_t state, uint32_t token);
int fk_ctc_beam_search_lm(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                          int64_t W, int64_t K, int64_t nbest, int64_t pad, const int32_t* lm_table, int64_t lm_cap, int64_t lm_max_probe,
                          const float* lm_bow, const int32_t* lm_backoff, int64_t lm_states, const float* lm_uni_lp, const int32_t* lm_uni_next,
                          int64_t lm_start_state, int64_t lm_order, float lm_weight, float length_bonus, int use_eos, int64_t* ids,
                          int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths, float* am, float* lm, float* total, int dtype, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- Lexicon-constrained CTC prefix beam search (csrc/ctc.hip): words out of a phoneme / letter head.  Semantics of this build
 *      (tests/ctc_lex_ref.py restates them in float64); all arithmetic is fp32.
 *   The head has a word separator class sep != blank, both in [0, C).  A lexicon maps pronunciations (non-empty tuples of classes, none
 *   blank or sep) to word ids in [0, V); several words may share a pronunciation (homophones, at most 8 a node), a word may have several.
 *   It is compiled to a trie, node 0 the root = the state at a word start; a node where a pronunciation ends is terminal (the root never).
 *   The acoustic recursion (pb, pnb, total, the candidate rule, the flow between resident prefixes) is EXACTLY fk_ctc_beam_search's, over
 *   labellings of the head's classes, sep included.  A slot also carries its trie node, its word count, lmw, lm (as fk_ctc_beam_search_lm)
 *   and the state of the word LM.  Only which NEW prefixes are proposed and the key change:
 *     p (node n) + (c,), c != sep:  proposed only if the trie has the child (n, c); it takes that child; lmw, lm, word state carry over
 *     p (node n) + (sep,):          proposed only if n is terminal.  w* = argmax over the words of n of ln P_lm(w | word state), exact ties
 *                                   to the first word of the node's list (ascending word id);  lmw' = lmw + (lm_weight * ln P(w*) +
 *                                   word_bonus) (the product, then the bonus, then the sum, each rounded);  lm' = lm + ln P(w*);  the word
 *                                   state advances by w*, the node becomes the root, the word count goes up by one
 *     key = total + lmw; an entry with total -inf is never kept; exact ties, and the bits of a prefix that returns, as in
 *     fk_ctc_beam_search_lm.  A rejected candidate has no key and costs no beam slot.  Neither blank nor sep is ever looked up in the LM.
 *   After the last frame a hypothesis at the root is complete; one at a terminal node is closed as if by a sep without acoustic term (its
 *   word, LM term, bonus and state advance) and is complete; one at any other node is incomplete: no closing term, its unfinished word is
 *   not emitted.  use_eos != 0: complete hypotheses add lm_weight * ln P_lm(</s> | state) (and lm that term).  Final order: complete
 *   before incomplete, then the final key descending, then the order of the last selection.
 *   Result, best first, the first nbest: words int64 [B, nbest, (T + 1) / 2] (strides ld_words_b, ld_words_h) padded with `pad`,
 *   word_lengths int64 [B, nbest], ids / lengths the labelling as fk_ctc_beam_search, am (the CTC mass) / lm (unweighted) / total (the
 *   final key) fp32 [B, nbest], complete uint8 [B, nbest].  A slot without hypothesis: lengths 0, scores -inf, rows of pad, complete 0.
 *   T_b = 0 gives the empty, complete hypothesis.
 *   Tables (frankenstein_amd/utils/lexicon.py compiles and validates them):
 *     trie_table  int32 [trie_cap][4], 16-byte aligned: open addressing, {node, class, child, 0}, node -1 = empty; trie_cap a power of two
 *                 (>= 2 x entries); the home of (node, class) is fk_ngram_hash(node, class) & (trie_cap - 1), linear probing;
 *                 trie_max_probe = the largest number of entries a successful look-up reads.  One probe sequence a look-up, no backoff.
 *     node_words  int32 [n_nodes][2], 8-byte aligned: {first, count} into word_list int32 [n_list]; count 0: not terminal
 *     lm_*        the word model as in fk_ctc_beam_search_lm, over V word ids, the end of sentence is id V.  Without a model pass a
 *                 unigram table of zeros (order 1, one state): every ln P is 0, w* the lowest id, only word_bonus acts.
 *   The device cannot check the tables: the trie loop is bounded by trie_max_probe, the word-LM look-ups by lm_order * lm_max_probe; a
 *   child read from the trie is clamped into [0, n_nodes), a count into [0, 8], a list index into [0, n_list), a word into [0, V), LM
 *   states and tokens as in fk_ctc_beam_search_lm, and every table index is masked.  A malformed table gives wrong words, never an
 *   unbounded loop or an access outside a table.
 *   Envelope of fk_ctc_beam_search; workspace fk_ctc_beam_lex_workspace_bytes(B, T, W, K) (0 outside the envelope: fk_ctc_beam_search's and
 *   one int32 per trie node, the word a sep node closed).  FK_EINVAL, no launch: sep outside [0, C) or equal to blank, a null table, a hash
 *   table that is not 16-byte aligned, a capacity that is no power of two, max_probe outside 1 .. cap, n_nodes < 1, n_list < 1, V < 1,
 *   weights that are not finite, a short workspace, words strides below (T + 1) / 2.
 *   Two launches (the first is fk_ctc_beam_search's), no atomics, the same bits every run, nothing waits for the host.
 *   Not built: LM look-ahead into the trie, an unknown-word path, forking on homophones (the choice is greedy per labelling).            */
size_t fk_ctc_beam_lex_workspace_bytes(int64_t B, int64_t T, int64_t W, int64_t K);
int fk_ctc_beam_search_lex(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t B, int64_t T, int64_t C, int64_t blank,
                           int64_t sep, int64_t W, int64_t K, int64_t nbest, int64_t pad, const int32_t* trie_table, int64_t trie_cap,
                           int64_t trie_max_probe, const int32_t* node_words, int64_t n_nodes, const int32_t* word_list, int64_t n_list, int64_t V,
                           const int32_t* lm_table, int64_t lm_cap, int64_t lm_max_probe, const float* lm_bow, const int32_t* lm_backoff,
                           int64_t lm_states, const float* lm_uni_lp, const int32_t* lm_uni_next, int64_t lm_start_state, int64_t lm_order,
                           float lm_weight, float word_bonus, int use_eos, int64_t* words, int64_t ld_words_b, int64_t ld_words_h,
                           int64_t* word_lengths, int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, int64_t* lengths, float* am, float* lm,
                           float* total, uint8_t* complete, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC prefix scores inside the GPT beam search (csrc/ctc.hip): one-pass joint CTC / attention decoding.  Every candidate c of every
 *      beam h of fk_beam_topk is rescored in front of fk_beam_select*:
 *          top_lp[r][j] <- (1 - weight) * top_lp[r][j] + weight * delta(h_r, c),   delta = psi(h c) - psi(h),
 *      psi = the CTC PREFIX log-probability (all labellings that start with the hypothesis) under logits [S, T, C] of the frame-synchronous
 *      head, sentence g = r / W.  Float64 restatement: tests/ctc_prefix_ref.py.
 *   y[t][c] = logits[g][t][c] - row_lse[g][t] for t < T_g = clamp(input_lengths[g], 0, T) (NULL: T).  lae = log(e^a + e^b), -inf for two -inf.
 *   A hypothesis (the generated tokens, behind the P prompt labels fk_ctc_prefix_init was given) carries r_n[t] / r_b[t] (the alignments of
 *   frames 0..t to it that end in a label / in the blank), psi and its last label.  Empty: r_n = -inf, r_b[t] = y[0][blank] + .. + y[t][blank]
 *   summed in frame order, psi = 0, last = -1.
 *   Extension by c (0 <= c < C, c != blank):  n[0] = y[0][c] if the hypothesis is empty, else -inf;  b[0] = -inf;  psi' = n[0];  for t >= 1:
 *       phi = (c == last) ? r_b[t-1] : lae(r_n[t-1], r_b[t-1]);   n[t] = lae(n[t-1], phi) + y[t][c];   b[t] = lae(n[t-1], b[t-1]) + y[t][blank];
 *       psi' = lae(psi', phi + y[t][c])                    (the kernels sum the T terms of psi' as one logsumexp)
 *   and the new hypothesis has r_n = n, r_b = b, psi = psi', last = c.  A label outside [0, C) or equal to the blank gives the impossible
 *   hypothesis (everything -inf, last = -2).
 *   delta = psi' - psi;  for c == eos (eos >= 0; tested first, eos need not be a class): delta = lae(r_n[T_g-1], r_b[T_g-1]) - psi, the
 *   probability of the whole labelling.  delta = FK_CTC_PREFIX_FLOOR when psi' or psi is -inf, c is the blank or outside [0, C), or T_g = 0:
 *   finite, so nothing behind it meets an inf or a NaN.  The joint value is two fp32 multiplies and one add, (1 - weight) one fp32 subtract.
 *   State: two buffers fp32 [S*W, 2, T] (r_n, then r_b; frames >= T_g hold -inf), psi fp32 [2][S*W], last int32 [2][S*W], the halves and the
 *   buffers swapped by the parity of *step exactly like hist / hist2 of fk_logit_rules: at *step > 0 (and broadcast == 0) row r first becomes
 *   extend(old[g*W + clamp(parent_log[(*step-1)*S*W + r], 0, W-1)], tok_log[(*step-1)*S*W + r]) in the buffer of *step's parity, then its k
 *   candidates are scored; no block reads what another block of the launch writes.  broadcast != 0 is the first step: top_lp / top_id are
 *   [S, k], row g uses the state of row g*W and nothing advances.  A row with fin[r] != 0 (fin may be NULL) is left untouched, state and
 *   top_lp; *step < 0 or > log_rows: the launch writes nothing.  Every element of a state row is written before it is read, so the buffers
 *   need no initialisation.
 * fk_ctc_prefix_init: row_lse [S, T] (fk_ctc_loss_fwd's launch), then per sentence the empty hypothesis extended by prompt[g][0 .. P) (int64,
 *   row stride prompt_ld; P = 0: none) into rows g*W .. g*W+W-1 of state0 and of the first halves of psi / last.  Two launches.
 * fk_ctc_prefix_score: one launch, one wave per row, the k candidates on the lanes; no atomics, the same bits every run, no host read.
 * Envelope: fp32 / bf16 logits, ldt >= C, ldb >= ldt, 1 <= T <= 1024, 1 <= k <= 64, 1 <= W <= 16, C >= 2, 0 <= blank < C, 0 <= P <= 64,
 *   0 <= weight <= 1, eos >= 0 only with fin: FK_EINVAL beyond, no launch.                                                            */
#define FK_CTC_PREFIX_FLOOR (-1e10f)
int fk_ctc_prefix_init(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, int64_t S, int64_t T, int64_t C, int64_t blank,
                       int64_t W, const int64_t* prompt, int64_t prompt_ld, int64_t P, float* row_lse, float* state0, float* psi, int32_t* last,
                       int dtype, void* stream);
int fk_ctc_prefix_score(const void* logits, int64_t ldb, int64_t ldt, const int64_t* input_lengths, const float* row_lse, int64_t S, int64_t T,
                        int64_t C, int64_t blank, int64_t W, int64_t k, float* top_lp, const int64_t* top_id, int broadcast, float weight,
                        int64_t eos, const int32_t* fin, const int64_t* step, const int32_t* parent_log, const int64_t* tok_log, int64_t log_rows,
                        float* state0, float* state1, float* psi, int32_t* last, int dtype, void* stream);

/* ---- n-best rescoring with a language model (csrc/rescore.hip): the hypotheses of one sentence (fk_ctc_beam_search's n-best list) share
 *      token prefixes, so every DISTINCT prefix is scored once: the list becomes a trie, the trie one packed GPT forward under an ancestor
 *      mask, the head goes through fk_head_ce_fwd (no [rows, V] logits), and the sums, the combination with the acoustic score and the
 *      ranking stay on the device.  The packing is exact: a node sees the causal context of its own flat sequence.  Semantics of this
 *      build (tests/rescore_ref.py restates them in float64).  One workgroup per sentence b < B unless noted; no atomics on global memory.
 *   Inputs: ids int64 [B, n, T] (strides ld_ids_b, ld_ids_h >= T; entries at or beyond a hypothesis' length are never read), lengths int64
 *   [B, n] (clamped into [0, T] on the device), am fp32 [B, n] or NULL (every slot present with am = 0).
 *   A hypothesis is UNSCORED when its am is not finite (the beam search's empty slot: length 0, score -inf), when a token inside its length
 *   lies outside [0, V), or when it does not fit the node capacity (below).  Length 0 with a finite am is the empty hypothesis and is scored.
 *   fk_nbest_trie: node 0 is the start token bos at depth 0 (parent -1).  Hypotheses are walked in order h = 0 .. n-1, tokens in order: a
 *     node is created the first time a (parent, token) pair is seen and gets the next free number, so parent[i] < i and depth[i] =
 *     depth[parent[i]] + 1.  leaf[h] = the node of h's last token, 0 for the empty hypothesis, -1 for an unscored one; equal hypotheses share
 *     a leaf; n_nodes[b] counts the root.  Overflow: a hypothesis whose new nodes do not ALL fit into node_cap - n_nodes becomes unscored and
 *     creates no node; later hypotheses are still tried.  tok / depth / parent int32 [B, node_cap]; dead nodes i >= n_nodes[b] hold bos, 0, -1.
 *     head_src / head_tgt int64 [B, node_cap - 1 + n] (both NULL: not written; a sizing pass reads only n_nodes), the rows of the vocabulary
 *     head for a packed forward with N = node_cap node rows behind P prefix rows: row i - 1 (1 <= i < N) is node i, hidden row P + parent[i],
 *     target tok[i] (a dead node: row P, target -100); row N - 1 + h is hypothesis h, hidden row P + leaf[h], target eos (row P and -100
 *     when eos is -1 or h is unscored).
 *   fk_nbest_trie_mask: every byte of the visibility table uint8 [B, P + N, P + N] (fk_attn_fwd's FK_MASK_DENSE, batch stride (P + N)^2):
 *     prefix row q sees prefix rows k <= q; a live node sees every prefix row and its ancestors-or-self; a dead node sees only itself.
 *     parent int32 [B, N].  One workgroup per row.
 *   fk_gpt_embed_pos: out[b, t] = prefix[b, t] + wpe[t] (t < P), out[b, P + i] = wte[tok[b, i]] + wpe[P + depth[b, i]]; tok / depth int32
 *     [B, N]; wte / wpe the fp32 master tables, prefix / out in `dtype` (fk_gpt_embed_fwd with a position per row; inference only).  A token
 *     is clamped into [0, vocab), a position below wpe_rows.
 *   fk_nbest_rescore: row_m / row_s / row_t fp32 [B, N - 1 + n] = fk_head_ce_fwd on the rows above; lp = row_t - (row_m + log(row_s)).
 *     cum[0] = 0, cum[i] = cum[parent[i]] + lp[i - 1] (one fp32 add per node, evaluated level by level: the adds of the sequential rule);
 *     lm[h] = cum[leaf[h]] (+ lp[N - 1 + h] with has_eos); total[h] = am_weight am[h] + lm_weight lm[h] + length_bonus len[h] in fp32;
 *     unscored (leaf < 0): lm = total = -inf.  Rank: scored hypotheses by total descending, exact ties by ascending original index, the
 *     unscored ones behind them in original order.  lm fp32 [B, n] in INPUT order; in the new order: ids_out int64 [B, n, T] (padded with
 *     `pad` behind the length), lengths_out int64 (clamped), am_out, lm_out, total_out fp32 [B, n], order int64 [B, n] (the original index
 *     of each place), n_scored int64 [B].  The same bits every run.  A NaN total leaves the order among the scored ones unspecified.
 *   Envelope (FK_EINVAL beyond, no launch): 1 <= n <= FK_NBEST_MAX_HYPS, 1 <= T <= FK_NBEST_MAX_T, 1 <= node_cap <= FK_NBEST_MAX_NODES
 *   (= 1 + 32 * 1024, the worst case of the largest list), N >= 1 and P + N <= FK_NBEST_MAX_ROWS for the mask and N <= FK_NBEST_MAX_ROWS
 *   for the scores, 0 <= bos < V, eos = -1 or in [0, V).  Nothing waits for the host.                                                   */
#define FK_NBEST_MAX_HYPS 32
#define FK_NBEST_MAX_T 1024
#define FK_NBEST_MAX_NODES 32769
#define FK_NBEST_MAX_ROWS 4096
int fk_nbest_trie(const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* am, int64_t B, int64_t n, int64_t T,
                  int64_t V, int64_t bos, int64_t eos, int64_t node_cap, int64_t P, int32_t* tok, int32_t* depth, int32_t* parent, int32_t* leaf,
                  int32_t* n_nodes, int64_t* head_src, int64_t* head_tgt, void* stream);
int fk_nbest_trie_mask(const int32_t* parent, const int32_t* n_nodes, uint8_t* mask, int64_t B, int64_t P, int64_t N, void* stream);
int fk_gpt_embed_pos(const int32_t* tok, const int32_t* depth, const void* prefix, const float* wte, const float* wpe, void* out, int64_t B, int64_t P,
                     int64_t N, int64_t dim, int64_t vocab, int64_t wpe_rows, int dtype, void* stream);
int fk_nbest_rescore(const float* row_m, const float* row_s, const float* row_t, const int32_t* depth, const int32_t* parent, const int32_t* leaf,
                     const int32_t* n_nodes, const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* am, int64_t B,
                     int64_t n, int64_t T, int64_t N, int has_eos, float am_weight, float lm_weight, float length_bonus, int64_t pad, float* lm,
                     int64_t* ids_out, int64_t* lengths_out, float* am_out, float* lm_out, float* total_out, int64_t* order, int64_t* n_scored,
                     void* stream);

/* ---- edit distance (csrc/editdist.hip): unit-cost Levenshtein distance on int64 ids compared by exact equality (no vocabulary; two
 *      different int64 ids stay different), and what an error rate, a minimum-Bayes-risk (MBR) selection from an n-best list and a
 *      minimum-word-error-rate (MWER) loss need over it.  Distances are int32, everything else fp32; no atomics, no workspace, the same bits
 *      every run, nothing waits for the host.  tests/edit_ref.py restates all of it in Python ints / float64.
 *   fk_edit_distance: B groups x n pairs.  a int64 [B, n_a, La] (strides ld_a_b, ld_a_h >= La) with n_a == n (pair h is a[g, h] against
 *     b[g, h]) or n_a == 1 (the group's one sequence, the reference, meets all n); alen int64 [B, n_a] or NULL; b int64 [B, n, Lb] with its
 *     own strides, blen int64 [B, n] or NULL.  A length is clamped into [0, L] on the device; with a NULL length a sequence ends at its first
 *     `pad_value` or at L (the -100 convention of fk_ctc_loss_fwd).  Entries at or behind the length are never used (behind a NULL length's
 *     first pad_value: never beyond the row).  dist int32 [B, n]; alen_out int32 [B, n_a] or NULL: the lengths of a as measured, so a rate
 *     needs no second pass.
 *   fk_edit_distance_route(La, Lb): the kernel a pair of row widths takes (host-side query, no launch).  One wave per pair sweeps
 *     anti-diagonals; the sequence of the narrower array sits on the lanes: FK_EDIT_LANE one row per lane (min(La, Lb) <= 64),
 *     FK_EDIT_ROWS4 four rows per lane (<= 256), FK_EDIT_ROWS16 sixteen (<= 1024); FK_EINVAL outside 1 .. FK_NBEST_MAX_T.
 *   fk_nbest_pairwise_distance: ids int64 [B, n, T], lengths int64 [B, n] (clamped), scores fp32 [B, n] or NULL (all valid) -> dist int32
 *     [B, n, n]: pairs i < j are computed once and mirrored, the diagonal is 0, and the row and the column (diagonal included) of a
 *     hypothesis whose score is not finite (the beam search's empty slot: length 0, score -inf) hold -1.
 *   fk_mbr_rank: over the valid j (finite score) of a sentence m = max_j scale s_j, w_j = exp(scale s_j - m), Z = sum_j w_j added in
 *     ascending j, p_j = w_j / Z, risk_i = sum_j p_j dist[i][j] (each product rounded, added in ascending j over the valid j).  The valid
 *     hypotheses are ranked by risk ascending, exact ties by the smaller input index (the better-scored hypothesis); the invalid ones follow
 *     in input order with risk +inf.  risk fp32 [B, n] in INPUT order; in the new order ids_out int64 [B, n, T] (padded with `pad` behind
 *     the length), lengths_out int64 (clamped), scores_out, risk_out fp32 [B, n], order int64 [B, n] (the input index of each place), n_valid
 *     int64 [B].  A NaN risk leaves the order among the valid ones unspecified.  One wave per sentence.
 *   fk_mwer_combine: nll fp32 [B, n], errors int32 [B, n]; hypothesis i of a sentence is valid when nll is finite, its score (scores fp32
 *     [B, n] or NULL) is finite and its length (lengths int64 [B, n] or NULL) is at most max_len.  Over the valid i: p = softmax(-nll), e_mean
 *     = the plain mean of the errors, loss[b] = sum_i p_i (e_i - e_mean), coef[b, i] = d loss[b] / d nll[b, i] = -p_i (e_i - sum_k p_k e_k);
 *     coef = 0 for an invalid i, loss = 0 for a sentence without a valid hypothesis.  loss fp32 [B], coef fp32 [B, n], count fp32 [1] = the
 *     sentences that have a valid hypothesis, valid uint8 [B, n] or NULL.  One launch.
 *   fk_mwer_reduce_rows: rows [B n, row_elems] in `dtype` (the gradient of logits expanded n times), valid uint8 [B, n] -> out [B, row_elems]
 *     in `dtype`: out[b] = (accumulate != 0 ? out[b] : 0) + the sum of rows[b n + i] over the valid i, added in ascending i in fp32.  A row
 *     that is not valid is never read (the CTC backward of an infeasible labelling is NaN).
 *   Envelope (FK_EINVAL beyond, no launch): 1 <= n <= FK_NBEST_MAX_HYPS, 1 <= La, Lb, T <= FK_NBEST_MAX_T, strides at least the row, a
 *   finite scale, no NULL required pointer.                                                                                              */
#define FK_EDIT_LANE 0
#define FK_EDIT_ROWS4 1
#define FK_EDIT_ROWS16 2
int fk_edit_distance_route(int64_t La, int64_t Lb);
int fk_edit_distance(const int64_t* a, int64_t ld_a_b, int64_t ld_a_h, const int64_t* alen, int64_t n_a, int64_t La, const int64_t* b, int64_t ld_b_b,
                     int64_t ld_b_h, const int64_t* blen, int64_t Lb, int64_t B, int64_t n, int64_t pad_value, int32_t* dist, int32_t* alen_out,
                     void* stream);
int fk_nbest_pairwise_distance(const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths, const float* scores, int64_t B, int64_t n,
                               int64_t T, int32_t* dist, void* stream);
int fk_mbr_rank(const int32_t* dist, const float* scores, float scale, const int64_t* ids, int64_t ld_ids_b, int64_t ld_ids_h, const int64_t* lengths,
                int64_t B, int64_t n, int64_t T, int64_t pad, float* risk, int64_t* ids_out, int64_t* lengths_out, float* scores_out, float* risk_out,
                int64_t* order, int64_t* n_valid, void* stream);
int fk_mwer_combine(const float* nll, const int32_t* errors, const float* scores, const int64_t* lengths, int64_t max_len, int64_t B, int64_t n,
                    float* loss, float* coef, float* count, uint8_t* valid, void* stream);
int fk_mwer_reduce_rows(const void* rows, const uint8_t* valid, void* out, int64_t B, int64_t n, int64_t row_elems, int accumulate, int dtype,
                        void* stream);

/* ---- optimizer: torch.optim.AdamW step fused with clip_grad_value_ (utils/train_utils.py:117-119,142-143) over a
 *      flat fp32 arena: g' = clamp(g * grad_scale, -clip, clip) (clip <= 0: no clamp); p *= 1 - lr*wd;
 *      m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).
 *      step is 1-based.  zero_grad != 0 also clears g (optimizer.zero_grad of the next step, :134).              */
int fk_adamw_step(float* p, float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, int64_t step, double clip, double grad_scale, int zero_grad, void* stream);

/* ---- the same update for several parameter groups, skipped parameters and torch.nn.utils.clip_grad_norm_, in ONE launch over the arena.
 *      segs: DEVICE array of nseg records sorted by begin, disjoint, begin / end multiples of 4 elements (the arena pads every tensor
 *      to 4); elements of [0, n) that lie in no segment are neither read nor written.  slot indexes `groups`, a HOST array of nslots
 *      (1..FK_ADAMW_MAX_SLOTS) hyper-parameter sets -- one per distinct (parameter group, bias-correction step) -- that is turned into
 *      floats exactly as fk_adamw_step does and travels by value with the launch; the per-element arithmetic is fk_adamw_step's, so
 *      one segment [0, n) with one slot gives its bits.  clip, grad_scale, zero_grad: as in fk_adamw_step.
 *   fk_grad_sumsq : partials[b] = block b's share of sum g^2 over the segments (the slots are ignored), b < npartials
 *                   (1..FK_GRAD_SUMSQ_MAX_BLOCKS blocks).  Fixed grid and summation order, no atomics: the same bits on every run.
 *   max_norm > 0  : every block of fk_adamw_step_groups adds the npartials partials in one fixed order, total = grad_scale * sqrt(sum),
 *                   coef = min(1, max_norm / (total + 1e-6)), and the gradient is g * grad_scale * coef; norm_out[0] = total (device
 *                   float).  max_norm == 0: no norm clip, partials / norm_out may be NULL.                                          */
#define FK_ADAMW_MAX_SLOTS 16
#define FK_GRAD_SUMSQ_MAX_BLOCKS 1024
typedef struct fk_adamw_seg { int64_t begin, end; int32_t slot, reserved; } fk_adamw_seg;
typedef struct fk_adamw_group { double lr, beta1, beta2, eps, weight_decay; int64_t step; } fk_adamw_group;
int fk_grad_sumsq(const float* g, int64_t n, const fk_adamw_seg* segs, int64_t nseg, float* partials, int npartials, void* stream);
int fk_adamw_step_groups(float* p, float* g, float* m, float* v, int64_t n, const fk_adamw_seg* segs, int64_t nseg,
                         const fk_adamw_group* groups, int nslots, double clip, double grad_scale, int zero_grad, double max_norm,
                         const float* partials, int npartials, float* norm_out, void* stream);

/* ---- vector quantiser of the VQ-VAE tokenizer (frankenstein_amd/models/vq_brain.py VectorQuantize: cosine-similarity codebook, build-defined
 *      semantics).  R data rows, K codes, D code dimension; codes / embed / embed_avg / sums fp32 [K, D], cluster_size / counts fp32 [K].
 * fk_vq_route: FK_VQ_FUSED when fk_vq_assign takes the problem (dtype FK_F32 / FK_BF16, D % 4 == 0, 4 <= D <= 128, 1 <= K < 2^31),
 *   else FK_VQ_CHAIN: the caller keeps the chain fk_norm_fwd, fk_gemm_nt, fk_argmax_rows, fk_gather_rows.  Host only, nothing is launched.
 * fk_vq_assign: one launch.  xn_r = x_r / max(|x_r|, 1e-12);  idx[r] = argmax_j <xn_r, codes_j>, the lowest index on an exact tie (a row
 *   of NaNs gives 0, as fk_argmax_rows); the similarity is exact fp32 (v_mfma_f32_32x32x2_f32) for either dtype of x, the codes are
 *   always the fp32 buffer.  x [R, D] in `dtype`, row stride ldx (elements, a multiple of 4).  Optional outputs (NULL = not written):
 *     q [R, D] in `dtype`, contiguous: codes[idx[r]] rounded to `dtype`;
 *     counts[j * counts_stride] += #rows with idx == j,  sums[j * ld_sums + d] += sum of xn_r[d] over those rows (fp32 atomics: the
 *       caller clears them; one packed [K, D + 1] tensor serves both);
 *     commit[0] = commit_scale * sum_r,d (x - q)^2 with q as rounded above: commit_partials holds ceil(R / 32) floats, one per workgroup,
 *       every one written; the last workgroup to finish adds them in index order (the same bits on every run).  ticket: a device word
 *       that is 0 before the launch and 0 again after it; launches that share it must be ordered on one stream.
 * fk_vq_bwd: dx[i] = dq[i] + d_commit[0] * c_scale * (x[i] - q[i]) over n contiguous elements of `dtype`: the straight-through gradient
 *   plus the commitment gradient (c_scale = 2 * commitment_weight / (R * D)).  dq == NULL counts as 0, d_commit == NULL as 0.
 * fk_vq_codebook_update: over the K codes; the EMA mode is two launches (the cluster sizes and their sum n by one workgroup into
 *   n_ws[0], one float of device scratch; then the codes), the k-means mode one.
 *   FK_VQ_EMA   : cs = decay * cs + (1 - decay) * counts;  avg = decay * avg + (1 - decay) * sums;  n = sum cs;
 *                 smoothed = (cs + eps) / (n + K * eps) * n;  embed = normalize(avg / smoothed);  codes with cs < dead are re-seeded:
 *                 embed = normalize(seed), avg = embed * dead, cs = dead.  seed fp32 [K, D]: rows of the batch (any positive length).
 *   FK_VQ_KMEANS: embed_j = normalize(sums_j / counts_j) where counts_j > 0, unchanged elsewhere; embed_avg, cluster_size, seed and n_ws
 *                 are not touched and may be NULL.
 *   normalize(v) = v / max(|v|, 1e-12).                                                                                              */
enum { FK_VQ_CHAIN = 0, FK_VQ_FUSED = 1 };
enum { FK_VQ_EMA = 0, FK_VQ_KMEANS = 1 };
int fk_vq_route(int64_t D, int64_t K, int dtype);
int fk_vq_assign(const void* x, int64_t ldx, const float* codes, int64_t* idx, void* q, float* counts, int64_t counts_stride, float* sums,
                 int64_t ld_sums, float* commit_partials, float* commit, float commit_scale, uint32_t* ticket, int64_t R, int64_t K,
                 int64_t D, int dtype, void* stream);
int fk_vq_bwd(const void* x, const void* q, const void* dq, const float* d_commit, float c_scale, void* dx, int64_t n, int dtype,
              void* stream);
int fk_vq_codebook_update(float* embed, float* embed_avg, float* cluster_size, const float* counts, int64_t counts_stride,
                          const float* sums, int64_t ld_sums, const float* seed, float* n_ws, int64_t K, int64_t D, float decay, float eps,
                          float dead, int mode, void* stream);

/* ---- per-session input adapter (build-defined: the reference hands date_info to every forward and never reads it; float64
 *      restatement in tests/day_adapter_ref.py).  With C = n_electrodes and d = day[b], the session ("day") of sample b:
 *          y[b, t, :] = x[b, t, :] + x[b, t, :] @ delta[d] + bias[d]          0 <= d < n_days
 *          y[b, t, :] = x[b, t, :]                                            any other d (-1 = unknown session), or day == NULL
 *      delta [n_days, C, C] and bias [n_days, C] are fp32 masters (zeros = the identity; weight decay pulls towards it); no
 *      nonlinearity; x fp32 [B, T, C] is data and gets no gradient.  Products and sums are fp32 in both compute modes (exact
 *      fp32-input MFMA; x + bias is added to the finished sum); the only rounding to `dtype` is the store.  day: int64 [B] ON THE DEVICE,
 *      never read by the host; an out-of-range value selects the pass-through, it is never used as an index.
 * fk_day_adapter_fwd writes y straight in fk_patchify's layout and contract: tok[b, (t / P) * C + c, p] in `dtype`, row stride
 *   ldp >= P, columns P..ldp-1 zero; with delta == 0 and bias == 0 the values are those of fk_patchify.  The adapted [B, T, C]
 *   signal never exists in memory.  P = 1, ldp = 1, dtype = FK_F32 is the natural [B, T, C] layout.
 * fk_day_adapter_bwd: d_tok fp32 in the same layout (row stride ldp), dy[b, tp * P + p, c'] = d_tok[b, tp * C + c', p]:
 *          d_delta[d, c, c'] = sum_{b: day[b] = d} sum_t x[b, t, c] * dy[b, t, c']
 *          d_bias[d, c']     = sum_{b: day[b] = d} sum_t dy[b, t, c']
 *   ALL n_days slices are overwritten; a day absent from the batch (and every day when day == NULL) gets exact zeros.  No atomics,
 *   no host read of day; the summation order is fixed by (B, T, C, P) and the contents of day: the same bits on every run.
 *   Scratch is the caller's workspace (fk_day_adapter_bwd_workspace_bytes; not needed when day == NULL); graph-capturable.
 * Envelope (anything else is refused with FK_EINVAL, on the host, before any launch): 1 <= C <= 512 (any C: tails are padded in
 *   LDS), T % P == 0, ldp >= P, n_days >= 1 (<= 65535 for the backward), sizes within int32, pointers aligned to their element. */
int fk_day_adapter_fwd(const float* x, const int64_t* day, const float* delta, const float* bias, void* tok, int64_t B, int64_t T,
                       int64_t C, int64_t P, int64_t ldp, int64_t n_days, int dtype, void* stream);
size_t fk_day_adapter_bwd_workspace_bytes(int64_t B, int64_t T, int64_t C, int64_t P, int64_t n_days);
int fk_day_adapter_bwd(const float* x, const int64_t* day, const float* d_tok, int64_t ldp, float* d_delta, float* d_bias,
                       void* workspace, size_t workspace_bytes, int64_t B, int64_t T, int64_t C, int64_t P, int64_t n_days,
                       void* stream);

/* ---- training-time signal augmentation inside the patch tokeniser (build-defined: the reference has none; float64 restatement in
 *      tests/augment_ref.py).  One launch with fk_patchify's reads and writes; no noise or mask tensor exists.
 * Random numbers: Philox4x32-10 with key (words[0], words[1]), `words` = int32 [2] ON THE DEVICE holding [seed, step] (the caller
 *   advances the step word on the device, inside a captured graph too), counter (i0, i1, b, 0xA0610000 | kind) -> words w0..w3.
 *   A pair of standard normals from a word pair (wa, wb):  u1 = ((wa >> 9) + 0.5) / 2^23  (24 bits: exact in fp32, never 0 or 1;
 *   ((wa >> 8) + 0.5) / 2^24 would need 25 and round to 1.0 at the top),  u2 = (wb >> 8) / 2^24,  r = sqrt(-2 ln u1),
 *   (r cos 2 pi u2, r sin 2 pi u2)  (logf, sqrtf, sincospif(2 u2)).  (w0, w1) gives normals 0 and 1 of a block, (w2, w3) normals 2, 3.
 *     kind 1 white      (i0, i1) = (t, c >> 2)   normal c & 3 is n_w(b, t, c); t is the OUTPUT frame
 *     kind 2 offset     (c >> 2, 0)              normal c & 3 is n_o(b, c), constant over time
 *     kind 3 electrode  (c >> 2, 0)              channel c of sample b is dropped iff w[c & 3] < thresh,
 *                                                thresh = min(floor(chan_drop_p * 2^32), 2^32 - 1) (host, double)
 *     kind 4 span m     (m, 0), m < n_time_masks len = ((w0 >> 8) * (time_mask_len + 1)) >> 24, start = ((w1 >> 8) * (T - len + 1)) >> 24
 *                                                (64-bit products); output frames start <= t < start + len are masked; spans may overlap
 *     kind 5 shift      (0, 0)                   s_b = (((w0 >> 8) * (2 time_shift + 1)) >> 24) - time_shift, in [-time_shift, time_shift]
 * Output element (b, t, c):
 *   1. ts = t - s_b; outside [0, T): +0.  Otherwise src = x[b, ts, c].
 *   2. keep_padding and noise on (white_sd > 0 or offset_sd > 0), and every channel of frame x[b, ts, :] exactly zero: +0 (the
 *      pipeline pads with zeros and SimpleMAE recognises padding as all-zero frames: noise must not turn padding into data).
 *   3. v = src + white_sd * n_w(b, t, c) + offset_sd * n_o(b, c) in fp32; a term whose sd is 0 is skipped, not multiplied by zero.
 *   4. channel dropped, or t inside a span: +0.  Masks come last: a masked element is exactly zero, the z-scored mean.
 *   5. one rounding to `dtype`; tok[b, (t / P) * C + c, p] for p < P, zeros for P <= p < ldp (fk_patchify's layout).
 *   With every knob zero the result has fk_patchify's bits.  P = 1, ldp = 1, FK_F32 is the augmented [B, T, C] signal itself.
 * Refused with FK_EINVAL on the host, before any launch: a null pointer, T % P != 0, ldp < P, a P * (C + 1) fp32 slab above 64 KiB,
 *   a negative or non-finite sd, chan_drop_p outside [0, 1), n_time_masks outside [0, 8], time_mask_len outside [0, T], time_shift
 *   outside [0, T), a dtype other than FK_F32 / FK_BF16, sizes beyond int32, misaligned pointers.  cfg is read on the host. */
typedef struct fk_augment_cfg {
  float white_sd, offset_sd, chan_drop_p;
  int32_t time_shift, n_time_masks, time_mask_len, keep_padding, reserved;
} fk_augment_cfg;
int fk_augment_patchify(const float* x, void* tok, int64_t B, int64_t T, int64_t C, int64_t P, int64_t ldp, const fk_augment_cfg* cfg,
                        const uint32_t* words, int dtype, void* stream);

/* ---- low-rank adapters (LoRA) on a frozen Linear (build-defined: the reference fine-tunes every parameter; float64 restatement in
 *      tests/lora_ref.py).  For W [N, K] (frozen), A [r, K], B [N, r] and s = alpha / r:
 *          y = x W^T + b + s (x A^T) B^T
 *      The base product stays with fk_gemm_nt; these entry points are the products with one extent equal to r.
 * fk_lora_fwd: one launch.  x [M, K] (row stride ldx), A [r, K] and B [N, r] contiguous, all in `dtype` (the compute-dtype shadows):
 *          u[m, j]   = round_to_dtype( sum_k x[m, k] A[j, k] )                       fp32 accumulation, ONE rounding
 *          out[m, n] = round_to_dtype( (res ? res[m, n] : 0) + scale * colscale(n) * sum_j u[m, j] B[n, j] )     fp32 accumulation
 *          colscale(n) = q_scale for n < q_cols, 1 elsewhere  (the query columns a projection epilogue pre-scales)
 *   u_out [M, r] (contiguous; may be NULL) receives u: it is the MFMA operand of the second product and the tensor the backward
 *   reads.  res (row stride ldr) may be NULL, a separate tensor, or `out` itself (every element is read by the lane that writes it).
 *   The data gradient is the same call on the transposed shadows B^T [r, N] and A^T [K, r]:
 *          fk_lora_fwd(dy, ldy, Bt, At, M, K, N, r, s, 0, 1, dh, ldh, du, dh, ldh, ...)   ->   du = dy B (unscaled),  dh += s du A.
 * fk_lora_wgrad: dy [M, N], u [M, r], du [M, r], x [M, K] contiguous in `dtype`; dA [r, K], dB [N, r] fp32:
 *          dB[n, j] (+)= scale * sum_m dy[m, n] u[m, j]        dA[j, k] (+)= scale * sum_m du[m, j] x[m, k]
 *   with du the UNSCALED dy B of the call above (scale * du^T x = (scale du)^T x).  accumulate != 0 adds to dA / dB, 0 overwrites.
 *   Rows are split in slices of 64 whose partials (workspace: fk_lora_wgrad_workspace_bytes, 0 for M <= 64) are added in slice
 *   order inside this entry point: no atomics, the same bits on every run.
 * fk_lora_merge: W, A, B fp32 masters (contiguous), out [N, K] (row stride ldo) in out_dtype:
 *          out[n, k] = fma(scale, c_r, W[n, k]),   c_0 = 0,  c_{j+1} = fma(B[n, j], A[j, k], c_j)      all fp32
 *   stored as fp32, or as bf16 rounded from that same fp32 value: a merged bf16 shadow has the bits of casting the merged master.
 * fk_lora_route (host): the forward's kernel variant, or -1 outside the envelope: FK_F32 / FK_BF16, 4 <= r <= 64 with r % 4 == 0,
 *   N and K multiples of 8 (4 for fp32), M >= 1, every extent and leading dimension below 2^31.  Outside it, a leading dimension
 *   shorter than its row, ldx not a multiple of 16 bytes, a null or misaligned pointer or a short workspace: FK_EINVAL on the host,
 *   before any launch.  No scratch memory, no host synchronisation, graph-capturable. */
enum { FK_LORA_R32 = 0, FK_LORA_R64 = 1 };
int fk_lora_route(int64_t M, int64_t N, int64_t K, int64_t r, int dtype);
int fk_lora_fwd(const void* x, int64_t ldx, const void* A, const void* B, int64_t M, int64_t N, int64_t K, int64_t r, float scale,
                int64_t q_cols, float q_scale, const void* res, int64_t ldr, void* u_out, void* out, int64_t ldo, int dtype,
                void* stream);
size_t fk_lora_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t r);
int fk_lora_wgrad(const void* dy, const void* u, const void* du, const void* x, int64_t M, int64_t N, int64_t K, int64_t r, float scale,
                  float* dA, float* dB, int accumulate, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int fk_lora_merge(const float* W, const float* A, const float* B, int64_t N, int64_t K, int64_t r, float scale, void* out, int64_t ldo,
                  int out_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FRANKEN_HIP_H */
