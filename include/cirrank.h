/*
 * cirrank.h - C ABI of libcirrank.so, the MI355X (gfx950) kernel library behind the stage-II
 * candidate re-ranking forward path of Cuberick-Orion/Candidate-Reranking-CIR.
 *
 * The reference has no native code and no FFI: its "operators" are PyTorch-eager op sequences
 * inside three Python files.  Each entry point below replaces one such sequence; the citation
 * names the reference lines whose arithmetic it computes (paths relative to the reference's src/).
 * The Python host (candidate_reranking_cir_amd/) binds these with ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()) - except cir_wgrad_grouped's descriptor array -; the caller owns all buffers; the
 *     library allocates nothing, never synchronises the device, and keeps no state besides the
 *     kernel-selection overrides of cir_set_tuning (default: none) and the cached CU count;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     work is enqueued on it and nowhere else;
 *   - leading dimensions / strides are in ELEMENTS of the tensor they describe - except the "split8" operand rows of ABI v14
 *     (cir_split8, cir_gemm_split8, cir_layernorm_split8, cir_attention_split8), which are BYTE rows of three segments and take their
 *     leading dimensions / strides in BYTES where the argument name says so;
 *   - dtype codes: CIR_BF16 / CIR_F16 for 16-bit activations and weights (fp32 accumulate
 *     everywhere), CIR_F32 for fp32 tensors - and, since ABI v11, as the OPERAND type of cir_gemm_bias_act, cir_attention
 *     and cir_patchify: the "exact" precision mode, every tensor fp32 like the reference's (validate_stage2.py:140-141:
 *     model.float()), products on the f32-input MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32: IEEE fmaf chains, 157.3 TFLOP/s
 *     peak = 1/16 of the 16-bit rate); the RESIDUAL STREAM (every x + sublayer(x) and the
 *     LayerNorm outputs that feed one) is either fp32 or fp16 ("stream dtype": CIR_F32 / CIR_F16),
 *     independently of the operand type - sums are formed in fp32 and rounded on the store (a GEMM with an fp16
 *     residual rounds its result to the stream type before the residual joins it: two roundings there);
 *   - return 0 on success, a negative CIR_E* code for an argument error detected before launch,
 *     or a positive hipError_t from the launch.  Nothing throws or aborts across the ABI.
 *   - functions are re-entrant and may be called from any host thread.
 */
#ifndef CIRRANK_H
#define CIRRANK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CIR_ABI_VERSION 15

enum { CIR_BF16 = 0, CIR_F16 = 1, CIR_F32 = 2 };
enum { CIR_ACT_NONE = 0, CIR_ACT_GELU = 1, CIR_ACT_RELU = 2 };
enum {
    CIR_OK = 0,
    CIR_EINVAL = -1,   /* null pointer / non-positive extent */
    CIR_ESHAPE = -2,   /* extent not supported by the kernels (see each function) */
    CIR_EALIGN = -3,   /* pointer or leading dimension not 16-byte aligned */
    CIR_EDTYPE = -4    /* dtype code not supported here */
};

int cir_version(void);
const char* cir_strerror(int code);

/*
 * Kernel-selection overrides for tests and A/B measurements (the library reads NO environment
 * variables).  Every knob defaults to 0 = automatic choice; a process that never calls this
 * function always gets the automatic choice.  Returns CIR_EINVAL for an unknown knob or a
 * value outside the knob's range.  Not part of any reference interface.
 *   CIR_TUNE_GEMM_TILE        0 auto | 128 | 256 : force the 128x128 or the persistent 256x256 GEMM
 *                             kernel where the shape allows it (cir_gemm_bias_act)
 *   CIR_TUNE_GEMM_GROUP_W     0 auto | 1..64    : n-panels per raster group of the 256x256 kernel
 *   CIR_TUNE_ATTN_SHARED_MAX  0 auto (608) | -1 never | 32..608 : largest padded key count for which
 *                             cir_attention stages a head's K/V once per workgroup in LDS; -2: as 0, and cir_attention_split8
 *                             runs on the f32-input MFMA (attn_f32_kernel) instead of its three-term fp16 form
 */
enum { CIR_TUNE_GEMM_TILE = 0, CIR_TUNE_GEMM_GROUP_W = 1, CIR_TUNE_ATTN_SHARED_MAX = 2 };
int cir_set_tuning(int knob, int value);

/*
 * C[b] = act(A[b] * W[b]^T + bias[b]) (+ residual[b]),   b = 0..batch-1
 *   A (M,K) 16-bit row-major (lda), W (N,K) 16-bit row-major "torch Linear" layout (ldw),
 *   bias fp32 (N) or NULL, residual (M,N) (ldr) or NULL (added after the activation),
 *   C (M,N) (ldc): out_dtype = in_dtype (operand copy), CIR_F32 or CIR_F16 (residual stream; also from
 *   bf16 operands).  res_dtype: CIR_F32 (with a C in the operand type or fp32) or CIR_F16 (only with an fp16 C; an fp16 C
 *   from bf16 operands takes ONLY an fp16 residual - CIR_EDTYPE otherwise).  C may alias residual.
 *   Requirements: K % 64 == 0, N % 16 == 0, 16-byte aligned rows.
 *   in_dtype CIR_F32 (ABI v11, "exact" mode): A, W, residual and C all fp32 (out_dtype and res_dtype must be CIR_F32), K % 32 == 0,
 *   one fmaf chain per output starting at the bias (K ascending within each group of 16, see csrc/gemm.hip), GELU evaluated as
 *   written in the reference: 0.5 x (1 + erf(x / sqrt 2)) with erff.
 *   Rounding: one rounding of the fp32 result to the type of C - except an fp16 residual-stream C WITH a residual, which
 *   rounds A*W^T + bias to fp16 first, adds the residual in fp32 and rounds again.  Both tile sizes (128 x 128, persistent
 *   256 x 256; picked from M*N*batch) start their accumulators at the bias, walk K in the same order and share the epilogue
 *   arithmetic: the result does not depend on the tile choice, i.e. not on the batch size, in any output type (ABI v8).
 * Replaces every nn.Linear on the path: vit.py:35-41,72,84; med.py:158-168,250-251,319-333;
 * nlvr_encoder.py:150-168,250-264,383-396; blip_stage2.py:50-54 (first layer); the erf GELU is
 * ACT2FN['gelu'] (nlvr_encoder.py:376-379) / nn.GELU (vit.py:26).
 */
int cir_gemm_bias_act(const void* A, int64_t lda, int64_t strideA,
                      const void* W, int64_t ldw, int64_t strideW,
                      const float* bias, int64_t strideBias,
                      const void* residual, int res_dtype, int64_t ldr, int64_t strideR,
                      void* C, int64_t ldc, int64_t strideC,
                      int64_t M, int N, int K, int batch,
                      int act, int in_dtype, int out_dtype, void* stream);

/*
 * C = act(LayerNorm(X; gamma, beta, eps) * W^T + b) WITHOUT a LayerNorm pass (ABI v12): the GEMM reads the raw fp16 residual-stream
 * rows X (M, K) (ldx; K = the whole normalised row) and the caller hands over the affine folded into the weight:
 *     Wg (N, K) = W diag(gamma) rounded to fp16 (ldw),   colsum[n] = sum_k Wg[n,k] (fp32, of the ROUNDED values),
 *     bias[n] = b[n] + sum_k W[n,k] beta[k] (fp32)
 * so that  C[m,n] = act( rstd_m * (sum_k X[m,k] Wg[n,k] - mean_m * colsum[n]) + bias[n] ),  C (M, N) fp16 (ldc).
 * mean_m / rstd_m (biased variance E[x^2] - mean^2 in fp32, eps added before the root) are formed inside the kernel from the same
 * fragments it multiplies (csrc/gemm256.hip, LNF): no normalised copy of X is written or read.  act CIR_ACT_NONE | CIR_ACT_GELU;
 * dtype CIR_F16 only (CIR_EDTYPE otherwise: the rows are the fp16 stream).  K % 128 == 0, N % 16 == 0, N >= 64, 16-byte aligned rows.
 * The result does not depend on M (always the 256 x 256 kernel; a row's statistics are summed in one fixed order).
 * Replaces norm1 + attn.qkv and norm2 + mlp.fc1 of every ViT block: vit.py:107-109 with :72 / :36-37.
 */
int cir_gemm_ln_bias_act(const void* X, int64_t ldx, const void* Wg, int64_t ldw, const float* colsum, const float* bias,
                         void* C, int64_t ldc, int64_t M, int N, int K, float eps, int act, int dtype, void* stream);

/*
 * y = act(x),  hi = fp16(y),  lo = fp16(y - hi)   (ABI v13):  x (rows, cols) fp32 with leading dimension ldx; hi, lo (rows, cols) fp16
 *   with leading dimension ldo; hi2 (optional, same layout) receives a second copy of hi.
 *   act CIR_ACT_NONE | CIR_ACT_GELU (0.5 y (1 + erf(y / sqrt 2)), erff) | CIR_ACT_RELU.  cols % 8 == 0, ldx % 4 == 0, ldo % 8 == 0, 16-byte aligned.
 *   The operand split of the "text32" precision mode: with hi = buf, lo = buf + cols, hi2 = buf + 2 cols, ldo = 3 cols a row of buf is
 *   [hi | lo | hi]; against weight rows [W_hi | W_hi | W_lo] ONE cir_gemm_bias_act of depth 3 cols on fp16 operands forms
 *   A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T in one fp32 accumulator: ~20 significant bits of a fp32 Linear at 3/16 of the f32-input MFMA's
 *   cost.  The MFMA keeps fp16 subnormals, so lo is stored unscaled.  No reference counterpart (the reference's fp32 Linear is what the
 *   three products approximate).
 */
int cir_split16(const float* x, int64_t ldx, void* hi, void* lo, void* hi2, int64_t ldo, int64_t rows, int cols, int act, void* stream);

/*
 * "split8" operand rows (ABI v14, round 6): y = act(x) as three byte segments per row,
 *     [ hi: cols x fp16 = fp16(y) | lo8: cols x e4m3 = e4m3((y - hi) 2^12) | hi8: cols x e4m3 = e4m3(hi) ]      = 4 cols bytes,
 *   both e4m3 terms clamped to +-448 first (OCP e4m3 has no infinity; the conversion does not saturate).  x (rows, cols) fp32 with leading
 *   dimension ldx (elements); out rows ldo_bytes apart.  act as cir_split16, GELU by an erf good to 1.5e-7.  cols % 16 == 0, 16-byte aligned.
 *   The A operand of cir_gemm_split8.  No reference counterpart (see there).
 */
int cir_split8(const float* x, int64_t ldx, void* out, int64_t ldo_bytes, int64_t rows, int cols, int act, void* stream);

/*
 * cir_attention on fp32 tensors (the CIR_F32 form: fp32 products, fp32 softmax) with the context written as split8 rows (ABI v14):
 *   out row (b1, b0, query) = [H*64 x fp16 | H*64 x e4m3 lo | H*64 x e4m3 hi] at out + b1 o_s1_bytes + b0 o_s0_bytes + query o_rs_bytes.
 *   Replaces BertSelfAttention.forward's core (nlvr_encoder.py:140-222, med.py:158-240) + the operand split in front of the attention
 *   output projection (nlvr_encoder.py:230-236) in the "text32" precision mode.  Strides of q / k / v in elements (% 4), of out in bytes (% 16).
 */
int cir_attention_split8(const float* q, int64_t q_s1, int64_t q_s0, int64_t q_rs, const float* k, int64_t k_s1, int64_t k_s0, int64_t k_rs,
                         const float* v, int64_t v_s1, int64_t v_s0, int64_t v_rs, const float* mask, int64_t m_s1, int64_t m_s0,
                         void* out, int64_t o_s1_bytes, int64_t o_s0_bytes, int64_t o_rs_bytes, int B1, int B0, int H, int Lq, int Lk,
                         float scale, void* stream);

/*
 * cir_layernorm on fp32 stream rows with the operand copy written as split8 rows (ABI v14): y_stream (fp32, may be NULL) as cir_layernorm
 *   writes it (bit for bit), y_split (batch, rows) rows of 4 cols bytes [fp16 | e4m3 lo | e4m3 hi] ld_split_bytes / stride_split_bytes apart.
 *   x / residual / y_stream strides per batch item in elements; gamma / beta (cols) or per batch item (strideG).  cols % 16 == 0, cols <= 1024.
 *   Replaces LayerNorm + the operand split in front of the text side's qkv and fc1 Linears (nlvr_encoder.py:262-264 / 469-476 -> :105-107 / 399).
 */
int cir_layernorm_split8(const float* x, int64_t strideX, const float* residual, int64_t strideR, const float* gamma, const float* beta,
                         int64_t strideG, float* y_stream, int64_t strideY, void* y_split, int64_t ld_split_bytes, int64_t stride_split_bytes,
                         int64_t rows, int cols, int batch, float eps, void* stream);

/*
 * C[b] = act(A[b] W[b]^T + bias[b]) (+ residual[b]) for a fp32 Linear whose operands travel as split8 rows (ABI v14; replaces the
 *   torch.nn.Linear calls of the text side - nlvr_encoder.py:105-107 / 230-236 / 399 / 411, med.py the same - in the "text32" precision
 *   mode, where the reference computes in fp32: validate_stage2.py:140-141):
 *     A (batch, M, K) rows [A_hi fp16 | e4m3(A_lo 2^12) | e4m3(A_hi)]           (cir_split8 / cir_layernorm_split8 / cir_attention_split8 /
 *                                                                                 this function with out_split = 1)
 *     W (batch, N, K) rows [W_hi fp16 | e4m3(W_hi 2^w_exp_hi) | e4m3(W_lo 2^w_exp_lo)],  W_hi = fp16(W), W_lo = W - W_hi
 *   ONE launch forms  A_hi W_hi^T  on the fp16 MFMA  +  A_lo W_hi^T + A_hi W_lo^T  on the block-scaled fp8 MFMA
 *   (v_mfma_scale_f32_16x16x128_f8f6f4, E8M0 scales 2^-12, 2^-w_exp_hi, 2^-w_exp_lo: twice the fp16 rate) in one fp32 accumulator that
 *   starts at the bias: the corrections are 2^-11 of the result and keep 4 significant bits per factor -> ~2^-16 of the result, against
 *   2^-11 for one fp16 product; cost 2 K / 64 K-tiles (three fp16 products: 3 K / 64; the f32-input MFMA: 16 K / 64).
 *   lda / ldw / strides in BYTES (rows are 4 K bytes long), K % 256 == 0, N % 16 == 0, 16-byte aligned.
 *   out_split 0: C (batch, M, N) fp32, ldc / strideC in elements, residual fp32 or NULL (only with CIR_ACT_NONE);
 *   out_split 1: C = split8 rows of act(.) (the next GEMM's operand: fc1 -> fc2), ldc / strideC in BYTES (>= 4 N), N % 64 == 0, no residual.
 *   The 128 x 128 and the persistent 256 x 256 kernel are chosen as in cir_gemm_bias_act and give the same bits.
 */
int cir_gemm_split8(const void* A, int64_t lda_bytes, int64_t strideA_bytes, const void* W, int64_t ldw_bytes, int64_t strideW_bytes,
                    const float* bias, int64_t strideBias, const float* residual, int64_t ldr, int64_t strideR,
                    void* C, int64_t ldc, int64_t strideC, int64_t M, int N, int K, int batch, int act, int out_split,
                    int w_exp_hi, int w_exp_lo, void* stream);

/*
 * y[b] = LayerNorm(x[b] (+ residual[b]); gamma[b], beta[b], eps) over the last dimension.
 *   x, residual (rows, cols) in x_dtype (CIR_F32 or CIR_F16: the residual stream); gamma/beta fp32 (cols);
 *   outputs: y_stream in y_stream_dtype (CIR_F32 / CIR_F16: the copy that feeds the next residual) and/or
 *   y16 (16-bit operand copy in dtype16); either may be NULL.  fp32 statistics.  cols % 4 == 0, cols <= 1024.
 *   Strides select the per-batch slice (stride 0 = shared).  Replaces nn.LayerNorm at vit.py:107-110,192
 *   (eps 1e-6) and med.py:253 / nlvr_encoder.py:252-264,395 (eps 1e-12), including the twin LayerNormA/B.
 */
int cir_layernorm(const void* x, int x_dtype, int64_t strideX, const void* residual, int64_t strideR,
                  const float* gamma, const float* beta, int64_t strideG,
                  void* y_stream, int y_stream_dtype, void* y16, int64_t strideY,
                  int64_t rows, int cols, int batch, float eps, int dtype16, void* stream);

/*
 * out = softmax(q k^T * scale + mask) v per (batch item, head), head_dim fixed at 64.
 *   Batch items are indexed (b1, b0), b1 < B1, b0 < B0; element (b1,b0,row,h,d) of q lives at
 *   q + b1*q_s1 + b0*q_s0 + row*q_rs + h*64 + d (same scheme for k, v, out); mask is an additive
 *   fp32 key mask (Lk) per item at mask + b1*m_s1 + b0*m_s0, or NULL.  kv_index (B1 int64, or NULL):
 *   item b1 reads its K/V from row kv_index[b1] of k / v instead of row b1 - the candidates of a
 *   query are then attended straight out of a per-image K/V bank (the cross-query reuse of
 *   SURVEY section 8(f)-1) with no gather copy.  16-bit in/out, fp32 softmax - or, dtype CIR_F32 (ABI v11), fp32 q / k / v / out
 *   with fp32 operands in both products (csrc/attention_f32.hip).  Replaces BertSelfAttention.forward (nlvr_encoder.py:140-222, med.py:158-240: the
 *   transpose_for_scores / matmul / scale / mask / softmax / matmul / merge-heads sequence) and
 *   Attention.forward's core (vit.py:73-83).
 */
int cir_attention(const void* q, int64_t q_s1, int64_t q_s0, int64_t q_rs,
                  const void* k, int64_t k_s1, int64_t k_s0, int64_t k_rs,
                  const void* v, int64_t v_s1, int64_t v_s0, int64_t v_rs,
                  const float* mask, int64_t m_s1, int64_t m_s0, const int64_t* kv_index,
                  void* out, int64_t o_s1, int64_t o_s0, int64_t o_rs,
                  int B1, int B0, int H, int Lq, int Lk, float scale, int dtype, void* stream);

/*
 * Cross-attention of ONE query row per (branch, head) over the tokens of each candidate, K / V projections folded out of
 * the token side (last fusion layer, where only the two CLS rows are used: nlvr_encoder.py:906-908 with :321-344):
 *   out[t][r][:] = sum_j softmax_j(qp[t][r] . x[t][j] * scale) x[t][j]     r < 32 rows, j < Lk keys, width D
 * x (T, Lk, D) 16-bit tokens (item stride x_s1, rows contiguous; with x_index (T int64, or NULL) item t reads the tokens of
 * row x_index[t] of an index-feature bank instead - the cross-query reuse of SURVEY section 8(f)-1), qp (T, 32, D) =
 * W_k^T q per row (rows beyond 2H: any finite values), out (T, 32, D).  The caller forms qp with a 64 x D GEMM per (branch, head) and applies W_v (+ b_v) to
 * `out` with a D x 64 GEMM (cir_gemm_bias_act, batched); the key bias is constant over j and drops out of the softmax.
 * D in {128, 256, .., 768}; no key mask.  Replaces, for that layer, the 4 D x D K|V projection of every candidate token
 * plus BertSelfAttention.forward's cross branch (nlvr_encoder.py:150-168, 183-217).
 */
int cir_cls_cross_attention(const void* x, int64_t x_s1, const int64_t* x_index, const void* qp, void* out, int T, int Lk, int D,
                            float scale, int dtype, void* stream);

/*
 * Cross-attention of ALL caption tokens of both branches over a candidate's image tokens with the key and value projections folded out of
 * the token side (ABI v11, round 5; csrc/xattn_fold.hip) - the two-branch BertLayer's crossattention.self{0,1} (nlvr_encoder.py:150-168,
 * 183-217, called :321-344) without ever forming K = X W_k^T or V = X W_v^T:
 *   out[t][tok][b][h 64 + d] = sum_f W_v[b][h 64 + d][f] (sum_j softmax_j((q[b][t L + tok][h] W_k[b][h]) . x[t][j] * scale) x[t][j][f]) + b_v[b][h 64 + d]
 * (the key bias is constant over j and drops out of the softmax; the rows of the softmax sum to 1, so the value bias adds as it is).
 * q (2, T L, D) 16-bit: the cross-attention QUERY projection incl. its bias (branch stride q_sb, row stride q_rs); x (T, N, D) 16-bit tokens
 * (item stride x_s1, rows contiguous); wkt / wvp (2, D, D each, branch stride w_sb): key.weight / value.weight re-ordered per MFMA fragment, one
 * contiguous KiB (64 lanes x 8 values; lane = 16 g + i) per wave-load -
 *   wkt[b] block ((u 2 + t) 12 + h) 2 + s : lane (g, i) holds key.weight[64 h + 32 s + 8 g + j][32 u + 8 (i >> 2) + 4 t + (i & 3)],  j < 8
 *   wvp[b] block (u 4 + e) 12 + h         : lane (g, i) holds value.weight[64 h + 16 e + i][32 u + (j < 4 ? 4 g + j : 16 + 4 g + j - 4)]
 * (u < D / 32 feature units, t < 2, s < 2, e < 4, h < 12; candidate_reranking_cir_amd/ops.py: fold_pack_key / fold_pack_value);
 * bv (2, D) fp32 value bias; out (T, L, 2, D)-shaped through strides.
 * D = 768, H = 12, L <= 32, N <= 608 (N <= 224: 48 query rows per wave, csrc/xattn_fold.hip; 225 .. 608 - the 384-px geometry's 577 tokens -: 16 rows per
 * wave, csrc/xattn_fold_units.hip) (CIR_ESHAPE otherwise: use cir_gemm_bias_act + cir_attention).  key_mask (ABI v14; NULL = none): additive fp32
 * mask (T, N), rows mask_stride apart, shared by both branches - the (1 - attention_mask) * finfo.min of padded candidate token sets
 * (nlvr_encoder.py:863-868): logits = scores * scale + mask; masks below -2e38 are clamped there (all-masked rows stay uniform).  16-bit operands, fp32
 * accumulation and softmax; Q' = q W_k and C' = P X are rounded to the operand type where the projected path rounds K and V.
 * 614 MFLOP per (candidate, both branches) instead of 969 at 197 keys (3.0 instead of 5.7 GFLOP at 577), and no (T N, 4 D) K|V tensor.
 */
int cir_cross_attention_folded(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp, int64_t w_sb,
                               const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st, int64_t o_sr, int64_t o_sb,
                               int T, int L, int N, int D, int H, float scale, int dtype, void* stream);

/*
 * cir_cross_attention_folded for captions of up to 64 tokens (csrc/xattn_fold_units.hip; additive within ABI v15): the same operator
 * (nlvr_encoder.py:150-168, 183-217), the same operands, packed weights, key mask and strides, for the captions the reference does not cut at 32
 * tokens (blip_stage2.py:113: padding='longest', no max_length; FashionIQ joins two captions per query).  D = 768, H = 12, L <= 64, N <= 224
 * (CIR_ESHAPE otherwise: use cir_gemm_bias_act + cir_attention).  A wave owns one head and up to three 16-token blocks of it; the cost grows in
 * 16-token steps (12 ceil(L / 16) blocks per candidate and branch).  A row's result does not depend on T, on the candidate's place in the batch or
 * on L: every block assignment accumulates in one order.
 */
int cir_cross_attention_folded_long(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp, int64_t w_sb,
                                    const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st, int64_t o_sr, int64_t o_sb,
                                    int T, int L, int N, int D, int H, float scale, int dtype, void* stream);

/*
 * cir_cross_attention_folded for captions of at most 16 tokens (csrc/xattn_fold_units.hip; additive within ABI v15): the same operator
 * (nlvr_encoder.py:150-168, 183-217), the same operands, packed weights, key mask and strides, for the short modification sentences the reference
 * never pads (blip_stage2.py:113: batch 1, padding='longest').  D = 768, H = 12, L <= 16, N <= 608 (CIR_ESHAPE otherwise: use
 * cir_cross_attention_folded).  One wave per head and one 16-token block: 12 blocks per candidate and branch where cir_cross_attention_folded
 * runs 24 (N <= 224: its 32 stacked rows per head group; 225 .. 608: a second wave per head on zero queries).  A row's bits are those of
 * cir_cross_attention_folded at 225 .. 608 keys and of cir_cross_attention_folded_long at <= 224 keys (same body, same accumulation order).
 */
int cir_cross_attention_folded_short(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp, int64_t w_sb,
                                     const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st, int64_t o_sr, int64_t o_sb,
                                     int T, int L, int N, int D, int H, float scale, int dtype, void* stream);

/*
 * cir_cross_attention_folded_long at the reference's 384-px geometry (csrc/xattn_fold_units.hip; additive within ABI v15): the same operator
 * (nlvr_encoder.py:150-168, 183-217), the same operands, packed weights, key mask and strides, for captions of more than 32 tokens
 * (blip_stage2.py:113: padding='longest', no max_length) against the 577 image tokens of 384 px (validate_stage2.py:327).  D = 768, H = 12,
 * 33 <= L <= 64, 225 <= N <= 608 (CIR_ESHAPE otherwise: cir_cross_attention_folded_long below 225 keys, cir_cross_attention_folded up to 32
 * tokens, cir_gemm_bias_act + cir_attention beyond).  Four waves per head: two 32-token halves x two KEY halves (16-key blocks 0-19 and 20-39 of a
 * 640-key capacity); one instantiation for every L, so a row's result does not depend on T, on the candidate's place in the batch, on L or
 * on the wave that held it.  Summation order of a row: 32-feature units in order; key blocks in order within a half; half 0 + half 1 (row
 * sums and contexts alike; both halves form the probabilities against the row's common maximum).  The key sum has two parts: rows are not
 * bit-identical to cir_cross_attention_folded's.
 */
int cir_cross_attention_folded_long_wide(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp, int64_t w_sb,
                                         const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st, int64_t o_sr, int64_t o_sb,
                                         int T, int L, int N, int D, int H, float scale, int dtype, void* stream);

/*
 * BertEmbeddings.forward (nlvr_encoder.py:68-91, med.py:87-110):
 *   y[r] = LayerNorm(word[ids[r]] + pos[r % L]) for r < rows; fp32 tables, outputs as cir_layernorm
 *   (y_stream in CIR_F32 / CIR_F16, y16 in dtype16).
 */
int cir_embed_layernorm(const int64_t* ids, const float* word, const float* pos,
                        const float* gamma, const float* beta, void* y_stream, int y_stream_dtype, void* y16,
                        int64_t rows, int L, int cols, int vocab, float eps, int dtype16, void* stream);

/*
 * timm PatchEmbed's im2col (vit.py:182; Conv2d k=p s=p == GEMM over flattened patches):
 *   patches[(b*gh+py)*gw+px][c*p*p + ky*p + kx] = image[b][c][py*p+ky][px*p+kx]
 *   image fp32 or 16-bit (img_dtype), patches 16-bit (dtype16) - or fp32 from an fp32 image (dtype16 = CIR_F32, ABI v11).
 */
int cir_patchify(const void* image, int img_dtype, void* patches, int dtype16,
                 int B, int C, int H, int Wd, int patch, void* stream);

/*
 * The reference's image transform (data_utils.py:23-101: TargetPad | SquarePad -> Resize(dim, BICUBIC) -> CenterCrop(dim) -> ToTensor ->
 * Normalize) from decoded uint8 RGB images of any sizes, one launch per batch (csrc/preprocess.hip; additive within ABI v15).  Bit for bit
 * PIL's 8-bit resize: two separable integer passes (horizontal first) over a uint8 intermediate,
 *     pixel = clip8(((1 << 21) + sum_j kk[j] * p[xmin + j]) >> 22),   int32 throughout, arithmetic shift
 * with the 22-bit fixed-point coefficients of libImaging's precompute_coeffs handed in as tables (the host forms them in float64:
 * candidate_reranking_cir_amd/preprocess.py: resample_taps).  The zero pad is never materialised: a coordinate of the padded image outside
 * the source reads 0.  Only the dim x dim pixels that survive the centre crop are computed.
 *   src        B images packed in one uint8 buffer of src_bytes bytes, each (h, w, 3) HWC RGB, each starting 16-byte aligned
 *   desc       B descriptors of 16 int32: {offset / 16, h, w, hp, vp, padded w, padded h, crop left, crop top, horizontal tap table
 *              (offset into taps, row stride), vertical tap table (offset, row stride), resized w, resized h, 0}
 *   taps       taps_len int32.  A tap table has one row per SURVIVING output coordinate (dim rows): {xmin, count, kk[0 .. count)} in
 *              coordinates of the padded image, rows `row stride` (>= 2 + the largest count) int32 apart.  A pass PIL skips (extent
 *              unchanged) is the table {x, 1, 1 << 22}, which reproduces the pixel exactly.
 *   table      768 values in the output type: table[c * 256 + u] = ((u / 255) - mean_c) / std_c as torch forms it in fp32 (ToTensor +
 *              Normalize, data_utils.py:82-83 / 99-100), converted to the output type by the host; unused (may be NULL) for CIR_PRE_RAW
 *   out        layout CIR_PRE_CHW: (B, 3, dim, dim) in dtype;  CIR_PRE_PATCHES: cir_patchify's operand rows (B (dim / 16)^2, 3 * 16 * 16),
 *              column order (c, ky, kx), in dtype (dim % 16 == 0, CIR_ESHAPE otherwise);  CIR_PRE_RAW: (B, dim, dim, 3) uint8, the resized
 *              and cropped image itself (dtype ignored)
 * dtype CIR_F32 / CIR_F16 / CIR_BF16.  Every source read is checked against the image's extent and the buffer's size, every tap-table row
 * against taps_len, every tap count against its row stride: no content of desc / taps can cause an access outside the buffers (a
 * descriptor that does not fit its buffer yields the image of an all-zero source).  Coefficients are multiplied as signed 24-bit values
 * (PIL's stay below 1.3 * 2^22 in magnitude).  dim <= 4096; src, desc, taps, table, out 16-byte aligned.
 */
enum { CIR_PRE_CHW = 0, CIR_PRE_PATCHES = 1, CIR_PRE_RAW = 2 };
int cir_preprocess_images(const uint8_t* src, int64_t src_bytes, const int32_t* desc, const int32_t* taps, int64_t taps_len, const void* table,
                          void* out, int B, int dim, int layout, int dtype, void* stream);

/*
 * Token assembly (vit.py:184-187): x[b][0] = cls + pos[0]; x[b][1+i] = proj[b*P+i] + pos[1+i].
 *   proj (B*P, D) (patch-embed GEMM output incl. bias) and x in stream_dtype (CIR_F32 / CIR_F16),
 *   cls (D), pos (P+1, D) fp32 parameters.  D % 8 == 0.
 */
int cir_vit_assemble(const void* proj, const float* cls, const float* pos, void* x, int stream_dtype,
                     int B, int P, int D, void* stream);

/*
 * y (M, N) fp32 = x (M, K) 16-bit * W (N, K) 16-bit ^T + bias, for tiny N (<= 8): the last
 * Linear of cls_head (blip_stage2.py:53, 134-136).  K % 8 == 0.
 */
int cir_small_linear(const void* x, int64_t ldx, const void* W, const float* bias, float* y,
                     int64_t M, int N, int K, int dtype, void* stream);

/*
 * dst[i] = convert(src[index[i]]) for rows of `row_elems` elements (index NULL = identity).
 * Replaces the per-query candidate gather torch.stack(itemgetter(*names)(name_to_feat))
 * (validate_stage2.py:115, 251, 266), the `.expand(K, ...)` of z_t / ids to the K candidates
 * (blip_stage2.py:118-121) and dtype conversion at the boundary.  row_elems % 8 == 0; every pair of
 * {f32, bf16, f16} (a conversion rounds once, from the fp32 value).  Indices are clamped to [0, src_rows).
 */
int cir_gather_rows(const void* src, int src_dtype, const int64_t* index, void* dst, int dst_dtype,
                    int64_t n_rows, int64_t row_elems, int64_t src_rows, void* stream);

/*
 * Per-row descending argsort (validate_stage2.py:53,174,188: torch.argsort(..., descending=True)):
 *   idx[q][j] = index of the j-th largest logit of row q, ties broken by lower index.  K <= 8192
 *   (also ranks a whole index for stage I: validate.py:58, 203 sort ascending distances = descending -distance).
 * The kernel is cir_topk_select's segment sort (csrc/rank.hip) on one segment with k = n.
 */
int cir_topk_desc(const float* logits, int64_t* idx, int Q, int K, void* stream);

/*
 * Stage-I retrieval over an index of ANY size (csrc/rank.hip; three entry points, additive within ABI v15 like cir_cross_attention_folded_long):
 * what stage II reads of a full ranking - the first k columns of every row (validate.py:57-64: sorted_index_names[:, :k]) and the place of the
 * target and of the CIRR group members (validate.py:202-226) - without sorting the row.  The order is cir_topk_desc's, exactly: a before b
 * <=> a.val > b.val, or equal values and a.idx < b.idx; a NaN reads as -inf; an excluded column does not exist (CIRR drops the reference
 * image from every row, validate.py:207-210).  The order is strict and total, so results are unique and equal cir_topk_desc's wherever both run.
 *
 * cir_topk_select (validate.py:57-64, 202-226): values fp32 (Q, n), rows ld >= n elements apart, never written; exclude int64 (Q) or NULL: one
 *   column per row to drop, -1 = none; idx int64 (Q, k) receives the first k columns of the order; val fp32 (Q, k) or NULL receives their keys as
 *   sorted (a NaN appears as -inf).  1 <= k <= 2048, k <= n - 1, n < 2^31 (CIR_ESHAPE otherwise).  One workgroup per (row, segment of 8192
 *   columns) sorts its segment in LDS and keeps its first k pairs; groups of floor(8192 / k) such lists are sorted again until one is left.  Grids
 *   are one-dimensional over (row, segment): Q * ceil(n / 8192) < 2^31 (CIR_ESHAPE beyond).  No atomics; no workgroup waits for another.
 *   workspace: a caller-owned device buffer of at least cir_topk_select_workspace(Q, n, k) bytes, 8-byte aligned (CIR_EINVAL when NULL or
 *   smaller); its contents are scratch.
 * cir_topk_select_workspace (validate.py:57-64, 202-226): pure host function; the bytes cir_topk_select needs for these extents, or a negative
 *   CIR_E* code for extents it refuses.
 * cir_rank_of (validate.py:57-64, 202-226): cols int64 (Q, m), m <= 8 (CIR_ESHAPE beyond); rank int64 (Q, m) receives the number of non-excluded
 *   columns that come before cols[q][t] in the order above - its position in the ranking, which is what `labels` marks (validate.py:60-64, 213-226);
 *   -1 for a column outside [0, n) or equal to the row's excluded one.  One pass over the row per workgroup, integer counts, fixed-order reduction.
 */
int64_t cir_topk_select_workspace(int Q, int n, int k);
int cir_topk_select(const float* values, int64_t ld, const int64_t* exclude, int64_t* idx, float* val, int Q, int n, int k,
                    void* workspace, int64_t workspace_bytes, void* stream);
int cir_rank_of(const float* values, int64_t ld, const int64_t* cols, const int64_t* exclude, int64_t* rank, int Q, int n, int m, void* stream);

/*
 * Rank refinement (csrc/rank.hip; four entry points, additive within ABI v15 like cir_topk_select; 66 entry points in all): a fast precision mode's logits decide the
 * order of a row wherever two values are far enough apart; only the rest is scored again by the exact mode.  Consumers of a logits matrix only
 * ever sort its rows (validate_stage2.py:53, 174, 188), so the matrix with the undecided entries overwritten sorts as the exact mode's.
 * The rule, for a row s and a margin >= 0, width = 2 * margin (exact in fp32): sort the row in cir_topk_desc's order (value descending, ties to
 * the lower column, a NaN as -inf); neighbours a, b of the sorted row are linked iff the fp32 difference a - b <= width (a difference that is
 * not a number links nothing); an entry is undecided iff it is linked to a neighbour.  If |fast - exact| <= margin on every entry of the row,
 * the stable descending argsort of the refined row equals that of the exact row at every position.
 *
 * cir_rank_undecided (validate_stage2.py:53, 174, 188): values fp32 (Q, K), rows ld >= K elements apart, never written; active uint8 (Q) or
 *   NULL: a row whose byte is 0 yields nothing (a skipped query holds one fill value everywhere); margin finite and >= 0 (CIR_EINVAL otherwise).
 *   pos int64 (capacity Q * K) receives the flat positions q * K + k of all undecided entries in ascending order, count int64 (1) their number;
 *   pos beyond count is not written.  1 <= K <= 8192 (one row per workgroup in LDS, like cir_topk_desc; CIR_ESHAPE beyond).  Three launches: a
 *   sort and flag pass per row, one workgroup that adds up the rows' counts, a compaction pass per row.  No atomics; no workgroup waits for
 *   another; every count is an integer: the same input gives the same pos and count bit for bit.
 *   workspace: a caller-owned device buffer of at least cir_rank_undecided_workspace(Q, K) bytes, 8-byte aligned (CIR_EINVAL when NULL,
 *   misaligned or smaller); its contents are scratch.
 * cir_rank_undecided_workspace (validate_stage2.py:53, 174, 188): pure host function; the bytes cir_rank_undecided needs for these extents, or a
 *   negative CIR_E* code for extents it refuses.
 * cir_rank_refine_apply (validate_stage2.py:53, 174, 188): values[q * ld + k] <- referee[i] for pos[i] = q * K + k, i < n (n = 0: nothing is
 *   written but stats).  stats: 16 bytes on the device, 8-byte aligned: fp32 max_i |old - referee| at byte 0 (a difference that is not a number
 *   does not enter the maximum), int64 at byte 8 the number of i that fail |old - referee| <= margin - the run-time check of the bound on
 *   exactly the entries it matters for.  A position outside [0, Q * K) is not written and counts as failing.  One workgroup, fixed-order reduction.
 * cir_rank_undecided_cuts (validate.py:60-64, 218-226; cirr_test_submission_stage2.py: the first 50 names): cir_rank_undecided for consumers that
 *   read only the first places of a row in order and the SETS before a few recall cut-offs.  A cluster is a maximal run [a, b] of linked places
 *   of the sorted row; with first >= 0 and up to 8 strictly ascending cuts >= 1 (a HOST array of n_cuts int32, copied into the kernel arguments;
 *   may be NULL when n_cuts = 0), a cluster is selected iff b > a and (a < first, or a < c <= b for some cut c); an entry is undecided iff its
 *   cluster is selected.  first >= K selects every cluster (cir_rank_undecided's rule); a cut >= K selects nothing; first = 0 without cuts selects
 *   nothing.  If |fast - exact| <= margin on every entry of the row, places 0 .. min(first, K) - 1 of the stable descending argsort of the refined
 *   row hold the exact row's columns, and for every cut c < K the set of columns in places 0 .. c - 1 is the exact row's.
 *   first < 0, n_cuts outside 0 .. 8, a cut < 1 or cuts not strictly ascending: CIR_EINVAL, before any launch.  values, ld, active, margin, pos,
 *   count, K <= 8192, the workspace (cir_rank_undecided_workspace) and the three launches are cir_rank_undecided's; the flag pass adds integer
 *   max / min reductions over the workgroup for the clusters that straddle a boundary.  Same input, same pos and count, bit for bit.
 */
int64_t cir_rank_undecided_workspace(int Q, int K);
int cir_rank_undecided(const float* values, int64_t ld, const unsigned char* active, float margin, int64_t* pos, int64_t* count, int Q, int K,
                       void* workspace, int64_t workspace_bytes, void* stream);
int cir_rank_refine_apply(float* values, int64_t ld, const int64_t* pos, const float* referee, int64_t n, float margin, void* stats, int Q, int K,
                          void* stream);
int cir_rank_undecided_cuts(const float* values, int64_t ld, const unsigned char* active, float margin, int first, const int* cuts, int n_cuts,
                            int64_t* pos, int64_t* count, int Q, int K, void* workspace, int64_t workspace_bytes, void* stream);

/*
 * fp32 y (M,N) = x (M,K) W(N,K)^T + bias (mode 0), 1 - x W^T (mode 1) or x W^T - 1 (mode 2, the exact
 * negative of mode 1, so that cir_topk_desc ranks by ascending distance): stage I's 256-d heads
 * vision_proj / text_proj (blip_stage1.py:42-43, 58, 83) and its distance matrix
 * `1 - predicted_features @ index_features.T` (validate.py:57, 202).  x rows at stride ldx.
 * M <= 65535 * 64 rows per call (CIR_ESHAPE beyond: one grid dimension of 64-row blocks).
 */
int cir_linear_f32(const float* x, int64_t ldx, const float* W, const float* bias, float* y,
                   int64_t M, int N, int K, int mode, void* stream);

/* y = x / max(||x||_2, 1e-12) row-wise, fp32 (F.normalize at blip_stage1.py:58, 83). */
int cir_l2_normalize(const float* x, float* y, int64_t rows, int cols, void* stream);


/* ------------------------------------------------------------------------------------------------------------------------
 * Training-mode operators: what BLIP_NLVR.img_txt_fusion in train() mode and its backward need
 * besides the operators above (blip_stage2.py:65-99 driven by stage2_train.py:202-216; dropout nlvr_encoder.py:86-90, 207,
 * 250-264, 397).  The dense layers' forward and dgrad run on cir_gemm_bias_act (dgrad over a transposed weight copy, cir_transpose16),
 * the weight gradients on cir_bmm.
 * Dropout is counter-based: element i of a launch is kept iff hash(seed, i) >= p, scaled by 1 / (1 - p) (stand-alone operators: splitmix64 of
 * (seed, flat index); fused operators: the pair hash described at cir_residual_layernorm_train); the backward
 * operators regenerate the same mask from the same (seed, p) - no mask tensor exists.  None of these is on the inference path.
 */
/* dst[b][c][r] = src[b][r][c], 16-bit elements (dtype CIR_BF16 / CIR_F16 names the payload only). */
int cir_transpose16(const void* src, void* dst, int rows, int cols, int64_t ld_src, int64_t ld_dst, int batch, int64_t s_src, int64_t s_dst,
                    int dtype, void* stream);
/* `count` transposes in one launch (ABI v10): matrix i - rows_i x cols_i, contiguous - at element offset off_i of src is written transposed at
 * the same offset of dst.  table (DEVICE memory, 4 int64 per matrix): {off_i, rows_i, cols_i, index of its first 32 x 32 tile}; total_tiles =
 * the sum of the tile counts.  The trainer transposes every trained weight of its flat 16-bit parameter buffer with it, once per step. */
int cir_transpose16_multi(const void* src, void* dst, const int64_t* table, int count, int64_t total_tiles, int dtype, void* stream);
/* C[z] = alpha * op(A[z]) * op(B[z]) (+ C[z] if accumulate): op(A) (M,K) from A stored (M,K) [trans_a 0] or (K,M) [1]; op(B) (K,N)
 * from B stored (K,N) [trans_b 0] or (N,K) [1].  Any extents, fp32 accumulate.  Two batch levels: z = z1 * nb2 + z2 with a stride per
 * level and operand (element units; 0 broadcasts), nb1 * nb2 <= 65535.  in_dtype CIR_BF16 / CIR_F16: MFMA kernel (64 x 64 tiles,
 * edges predicated, 16-byte loads when base / ld / strides allow, 2-byte loads otherwise), out_dtype = in_dtype or CIR_F32;
 * in_dtype CIR_F32: plain kernel, fp32 out.  Used for the un-fused attention of the training pass (Q K^T, P V and their four
 * adjoints per (candidate or triplet, head)) and, with trans_a = 1 and a batch over row chunks, for the weight gradients.
 * accumulate: 0 C = ..., 1 C += ... (read-modify-write: batch items must own their C), 2 (ABI v10; MFMA kernel, fp32 C) atomic C += ... -
 * batch items may share one C (stride 0): the row chunks of a weight gradient sum straight into dW, in no fixed order. */
int cir_bmm(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int trans_a, int trans_b,
            int nb1, int nb2, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1, int64_t sC2, float alpha, int accumulate,
            int in_dtype, int out_dtype, void* stream);
/* Weight gradient of a dense layer (ABI v10; train_wgrad.hip): dw (N, K) fp32 (row stride ldw) += dy^T x, dy (rows, N) and x (rows, K) 16-bit
 * row-major (strides ldy, ldx; multiples of 8) read AS STORED - LDS-DMA staging, transposing LDS reads, 128 x 128 output tiles, the rows split
 * over `splits` workgroups per tile (0: chosen from the shape) that add their partial tiles into dw atomically (no fixed summation order).
 * N % 128 == 0 and K % 128 == 0 (CIR_ESHAPE otherwise: use cir_bmm with trans_a); any row count (a tail below 64 rows runs on cir_bmm's kernel).
 * Adjoint of nn.Linear's weight (nlvr_encoder.py:150-168, 250-264, 383-409 under stage2_train.py:216's backward). */
int cir_wgrad(const void* dy, int64_t ldy, const void* x, int64_t ldx, float* dw, int64_t ldw, int64_t rows, int N, int K, int splits, int in_dtype,
              void* stream);
/* Up to 16 weight gradients in ONE launch: dw_i += dy_i^T x_i.  The 13 weight gradients of one two-branch BertLayer together have ~940 output
 * tiles - enough to fill the chip with every tile's row sum formed by one workgroup (plain adds, no atomics; a 768 x 768 weight alone has 36
 * tiles and needs an 8 .. 16-way row split whose atomic traffic costs as much as the product).  Units are balanced by splitting the longer row
 * counts (the FFN's stacked 2R rows) to the shortest one's length - and, when the group fills the chip, halved once more (two workgroups' atomic
 * adds per tile: measured faster than the tail of a 2.4-round launch).  Same shape rules as cir_wgrad; splits 0 = automatic.
 * `problems` is a HOST array (the one exception to "every pointer is a device pointer": it is read during the call, its members dy / x / dw are
 * device pointers); count <= 16 (CIR_ESHAPE beyond: call again). */
typedef struct { const void* dy; int64_t ldy; const void* x; int64_t ldx; float* dw; int64_t ldw; int64_t rows; int N, K, splits; } cir_wgrad_desc;
int cir_wgrad_grouped(const cir_wgrad_desc* problems, int count, int in_dtype, void* stream);
/* P = softmax(S * scale + mask) per row (S fp32 (rows, cols); mask fp32 (cols) shared by each group of rows_per_mask rows, or
 * NULL), Pd = dropout(P, p_drop, seed); both 16-bit (dtype).  nlvr_encoder.py:183-207. */
int cir_softmax_dropout(const float* S, int64_t ld_s, const float* mask, int64_t rows_per_mask, int64_t ld_mask, void* P, void* Pd, int64_t ld_p,
                        int64_t rows, int cols, float scale, float p_drop, uint64_t seed, int dtype, void* stream);
/* dS = scale * P * (dP - sum_cols(dP * P)), dP = dropout-backward(dPd) with the forward's (p_drop, seed); dPd fp32, dS 16-bit. */
int cir_softmax_dropout_bwd(const void* P, int64_t ld_p, const float* dPd, int64_t ld_d, void* dS, int64_t ld_ds, int64_t rows, int cols,
                            float scale, float p_drop, uint64_t seed, int dtype, void* stream);
/* FUSED attention of the training pass (round 4): out = dropout(softmax(q k^T * scale + mask)) v per (group, head), head dimension 64, with
 * the log2-domain log-sum-exp of every row written to lse (G, H, Lq) - and its recomputing backward: dq / dk / dv (grad_dtype: CIR_F32, or the operand type - ABI v10 - so that the
 * projection's dgrad / wgrad products read them as they are) from q, k, v,
 * out, d_out and lse; the probabilities are recomputed tile by tile and the dropout mask regenerated from its counter (the pair hash of the
 * fused kernels, see below: row = (g * H + h) * Lq + query, col = key), so no score / probability tensor exists in memory.  Tensors are head views: element
 * (g, h, row, d) at base + g * x_sg + h * x_sh + row * x_sr + d; out and d_out share one layout; mask fp32 (G, Lk) additive or NULL;
 * dsum_scratch fp32 (G * H * Lq) receives rowsum(d_out * out) - with out taken from its optional fp32 twin out32 (written by the
 * forward, same layout): it then equals sum_j Pd_ij dPd_ij term for term and the row sums of dS vanish.  Mask values are clamped at -2e38; a
 * group whose EVERY key is at that clamp (finfo.min on all keys) has uniform rows and lse = -2e38 * log2(e) exactly, and the backward
 * recognises it by that lse (its gradients are those of the uniform rows).  A row whose keys are all masked by huge values ABOVE the clamp
 * (say -1e35 everywhere) is not supported: its lse absorbs log2 of the row sum and the backward cannot rebuild P.  Replaces, for BertSelfAttention.forward in train() mode
 * (nlvr_encoder.py:140-222, dropout :207) and its adjoint, the cir_bmm / cir_softmax_dropout[_bwd] chain. */
int cir_attention_train_fwd(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                            const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, void* out, int64_t o_sg, int64_t o_sh,
                            int64_t o_sr, float* out32, float* lse, int G, int H, int Lq, int Lk, float scale, float p_drop, uint64_t seed,
                            int dtype, void* stream);
int cir_attention_train_bwd(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                            const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* out, const void* d_out,
                            int64_t o_sg, int64_t o_sh, int64_t o_sr, const float* out32, const float* lse,
                            float* dsum_scratch, void* dq, int64_t dq_sg,
                            int64_t dq_sh, int64_t dq_sr, void* dk, int64_t dk_sg, int64_t dk_sh, int64_t dk_sr, void* dv, int64_t dv_sg,
                            int64_t dv_sh, int64_t dv_sr, int grad_dtype, int G, int H, int Lq, int Lk, float scale, float p_drop, uint64_t seed,
                            int dtype, void* stream);
/* Attention MAPS of the fused training attention (csrc/attn_maps.hip; two entry points, additive within ABI v15: 72 in all): what
 * nlvr_encoder.py:199-203 keeps when save_attention is set - attention_probs after the softmax and BEFORE the dropout (save_attention_map)
 * and the gradient its register_hook receives (save_attn_gradients) - rebuilt tile by tile from q, k and the forward's log2-domain lse
 * (cir_attention_train_fwd; p_drop = 0 there or not: the maps are the pre-dropout quantities) and written out as fp32:
 *   probs  (G, H, Lq, ldk) = exp2(q k^T * scale * log2e + mask * log2e - lse)       (the kSatLse rule of cir_attention_train_bwd applies)
 *   dprobs (G, H, Lq, ldk) = dmul * d_o v^T                                          (dmul: e.g. the inverse of a loss scale, a power of two)
 * Tensors are head views as in cir_attention_train_bwd (element (g, h, row, d) at base + g * x_sg + h * x_sh + row * x_sr + d, strides
 * multiples of 8, 16-byte aligned bases); mask fp32 (G, Lk) additive or NULL; lse fp32 (G, H, Lq).  v, d_o and dprobs are all NULL
 * (probabilities only - the same bits as the full call's probs) or all non-NULL.  Row pitch ldk: ldk % 4 == 0, ldk >= Lk; columns
 * [Lk, ldk) of every row are written with 0 and nothing outside the G * H * Lq * ldk elements is touched.  head_dim must be 64.
 * CIR_ESHAPE: a bad ldk, head_dim != 64, an inconsistent NULL pattern.  16-bit operands (CIR_BF16 / CIR_F16).  Plain vector stores. */
int cir_attention_maps(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                       const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* d_o, int64_t o_sg,
                       int64_t o_sh, int64_t o_sr, const float* lse, float* probs, float* dprobs, int64_t ldk, int G, int H, int Lq, int Lk,
                       int head_dim, float scale, float dmul, int dtype, void* stream);
/* Grad-CAM of the same maps without materialising them (nlvr_encoder.py:199-203 are the two factors):
 *   cam (G, Lq, ldk) = (1 / H) sum_h probs[g, h] * max(dprobs[g, h], 0)
 * one wave per (group, query tile, key tile) sums the heads in the order 0 .. H-1 in fp32 registers: no atomics, the result repeats bit for
 * bit.  Same inputs (v and d_o required), checks and pad rule (columns [Lk, ldk) = 0) as cir_attention_maps. */
int cir_attention_gradcam(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                          const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* d_o, int64_t o_sg,
                          int64_t o_sh, int64_t o_sr, const float* lse, float* cam, int64_t ldk, int G, int H, int Lq, int Lk, int head_dim,
                          float scale, float dmul, int dtype, void* stream);
/* LayerNorm backward from the saved fp32 input x of the forward: dx (written), dgamma / dbeta (fp32, ACCUMULATED atomically). */
int cir_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int64_t rows, int cols,
                      float eps, void* stream);
/* FUSED row passes of the training step (ABI v10; train_fused.hip).  BertSelfOutput / BertOutput in train() mode
 * (nlvr_encoder.py:248-264, 399-409: dense -> dropout -> + residual -> LayerNorm, incl. the averaged two-branch merge :257-260):
 *   pre = dropout(alpha * (t0 + t1), p_drop, seed) + residual;  y = LayerNorm(pre; gamma, beta, eps)
 * t0 / t1 (t1 may be NULL) / residual fp32 (rows, cols) contiguous; pre (fp32, kept for the backward), y32 (fp32 or NULL) and y16 (16-bit in
 * dtype16, or NULL) are written.  cols % 4 == 0, cols <= 1024.
 * Dropout of the FUSED kernels (this one, its adjoint, cir_attention_train_*; ABI v10): element (row, col) is dropped iff its 16 random bits
 * are below round(p * 65536); the bits of the column pair (2j, 2j + 1) are the low / high half of
 *   hash32((uint32)seed + (uint32)(seed >> 32) * 0x85EBCA6B + (uint32)row * 0x9E3779B9 + (uint32)(row >> 32) * 0xC2B2AE35  ^  j),
 * hash32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 - two 32-bit multiplies per pair instead of the three
 * 64-bit ones per element of the stand-alone kernels' splitmix64 (which made the hash ~10x the MFMA time of an attention tile). */
int cir_residual_layernorm_train(const float* t0, const float* t1, const float* residual, const float* gamma, const float* beta, float* pre,
                                 float* y32, void* y16, int64_t rows, int cols, float eps, float alpha, float p_drop, uint64_t seed, int dtype16,
                                 void* stream);
/* Its adjoint: dx = d pre from dy and the saved pre (x) as cir_layernorm_bwd (dx may be NULL when only the dense branch is wanted), dgamma / dbeta
 * ACCUMULATED; and, when dt16 is given, the gradient of the dense branch  dt = alpha * dropout'(dx + t_add)  (t_add fp32 or NULL: a second
 * LayerNorm's d pre over the SAME dense output, as behind the two-branch merge) written as the 16-bit operand (dtype16) of that layer's dgrad /
 * wgrad products, with its column sums ACCUMULATED into dbias and dbias2 (either may be NULL): the dense layer's bias gradient. */
int cir_layernorm_bwd_fused(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, const float* t_add,
                            void* dt16, float* dbias, float* dbias2, int64_t rows, int cols, float eps, float alpha, float p_drop, uint64_t seed,
                            int dtype16, void* stream);
/* 16-bit rows (rows, cols), row strides lda / ldz / ldo (multiples of 8), cols % 8 == 0.  mode 0: sums[c] += sum_r a[r][c] (bias gradient of a
 * dense layer whose output gradient is 16-bit: behind the attention adjoints);  mode 1: out = a * gelu'(z) (erf form) and, when sums is given,
 * sums[c] += sum_r out[r][c] - BertIntermediate's adjoint (nlvr_encoder.py:383-396) with the bias gradient in the same pass. */
int cir_rows16_colsum(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, float* sums, int64_t rows, int cols, int mode,
                      int dtype, void* stream);
/* The backward of a gradient-CHECKPOINTED ViT block (vit.py:36-37: Mlp.forward's fc1 -> act; vit.py:103-105: attn / mlp of block i wrapped in
 * checkpoint_wrapper when use_grad_checkpointing and i >= depth - ckpt_layer): gelu(z) was released with the forward and fc2's weight gradient
 * wants it back.  One pass over a (= d gelu(z)) and z writes BOTH  out = a * gelu'(z)  (bit-identical to cir_rows16_colsum mode 1, and so are
 * the sums)  and  out_f = gelu(z)  (bit-identical to cir_eltwise mode 0 on the same z), and, when sums is given, sums[c] += sum_r out[r][c].
 * 16-bit rows (rows, cols), cols % 8 == 0 (CIR_ESHAPE); row strides lda / ldz / ldo / ldf multiples of 8 elements and all four pointers
 * 16-byte aligned (CIR_EALIGN); dtype CIR_BF16 / CIR_F16; a, z, out, out_f required (CIR_EINVAL), sums may be NULL. */
int cir_rows16_gelu_pair(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, void* out_f, int64_t ldf, float* sums,
                         int64_t rows, int cols, int dtype, void* stream);
/* out[r] = a[r] + scale[r / rows_per_group] * b[r] over rows of `cols` fp32 values (a may be NULL: out = scale * b); out fp32 or 16-bit
 * (out_dtype).  DropPath - timm's per-sample stochastic depth around both branches of a ViT block (vit.py:98-109; blip_stage2.py:37 builds the
 * stage-II image encoder with drop_path_rate 0.1) - in the ViT fine-tuning pass: the forward adds the sample-scaled branch to the stream, the
 * backward writes the sample-scaled stream gradient as the 16-bit operand of the branch's adjoint products.  cols % 4 == 0. */
int cir_rows_scale_add(const float* a, const float* b, const float* scale, void* out, int64_t rows, int cols, int64_t rows_per_group, int out_dtype,
                       void* stream);
/* mode 0: out = gelu(z) (erf form, ACT2FN['gelu']); 1: out = dy * gelu'(z); 2: relu(z); 3: dy * (z > 0); 4: dropout(z, p_drop, seed);
 * 5: z + dy; 6: p_drop * z (scale).  z in z_dtype (CIR_F32 / CIR_BF16 / CIR_F16), dy fp32, out in out_dtype. */
int cir_eltwise(const void* z, int z_dtype, const float* dy, void* out, int out_dtype, int64_t n, int mode, float p_drop, uint64_t seed, void* stream);
/* out[c] += sum_r x[r][c] (bias gradients; fp32, atomics).  rows <= 65535 * 32 per call (CIR_ESHAPE beyond). */
int cir_colsum(const float* x, int64_t ld, float* out, int64_t rows, int cols, void* stream);
/* BertEmbeddings backward (nlvr_encoder.py:49-91): dword[ids[r]] += dy[r], dpos[r % L] += dy[r] (fp32, atomics). */
int cir_embed_bwd(const int64_t* ids, const float* dy, float* dword, float* dpos, int64_t rows, int L, int cols, void* stream);
/* Fixed-order forms (deterministic training mode; train_det.hip and the `_ordered` launches of train.hip / train_fused.hip).  The operators
 * above that add across workgroups with fp32 atomics (cir_layernorm_bwd, cir_layernorm_bwd_fused, cir_rows16_colsum, cir_colsum,
 * cir_embed_bwd) have a twin here that computes the same sums in an order fixed by the shapes alone: same inputs, same device, same build ->
 * the same bits, call after call.  Every destination is still ACCUMULATED (old + sum).  The workspaces are the caller's (`partials`: fp32,
 * `partial_elems` elements; contents undefined before and after), nothing is allocated or synchronised, a workspace that is too small is
 * refused with CIR_ESHAPE before any launch.  No workgroup waits for another: partial sums are stored with plain stores and added by a later
 * launch on the same stream.
 *
 * cir_colsum_ordered: out[c] += sum_r x[r][c], ld >= cols.  The order: the rows are cut into blocks of 256.  Inside a block, row lane l
 * (0 .. 7) adds rows l, l + 8, l + 16, ... in ascending order into one fp32 accumulator that starts at 0, and the eight lanes are combined as
 * ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  With one block (rows <= 256) that value is added to out[c].  With B > 1 blocks the B block
 * sums are stored to partials (needs B * cols elements), summed over the blocks by the same rule (lane l adds block sums l, l + 8, ...; all
 * B of them form ONE block here, whatever B), and the result is added to out[c].  rows <= 65535 * 256.
 * "The finishing sum" below is this operator applied to one row of partial sums per workgroup: workgroup sums in ascending workgroup order
 * per lane, eight lanes, the fixed tree, then added to the destination. */
int cir_colsum_ordered(const float* x, int64_t ld, float* out, int64_t rows, int cols, float* partials, int64_t partial_elems, void* stream);
/* cir_layernorm_bwd with dgamma / dbeta in a fixed order: workgroup b (rows 32 b .. 32 b + 31) sums its rows as cir_layernorm_bwd does (wave w
 * takes rows 32 b + 4 i + w for i = 0 .. 7 in that order; the four waves are added 0 + 1 + 2 + 3 left to right) and stores the 2 * cols sums
 * to row b of partials; then the finishing sum over the ceil(rows / 32) workgroups.  partial_elems >= ceil(rows / 32) * 2 * cols.  dx is
 * bit-identical to cir_layernorm_bwd's. */
int cir_layernorm_bwd_ordered(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int64_t rows, int cols,
                              float eps, float* partials, int64_t partial_elems, void* stream);
/* cir_layernorm_bwd_fused likewise: workgroup b (32 rows, wave w rows 32 b + 4 i + w in order, waves combined (0 + 1) + (2 + 3)) stores
 * dgamma | dbeta | bias-gradient sums (the third only when dt16 and dbias are given) to row b of partials, then the finishing sum; dbias2
 * receives the same bias sums as dbias.  partial_elems >= ceil(rows / 32) * (3 or 2) * cols.  dx / dt16 are bit-identical to the plain form's. */
int cir_layernorm_bwd_fused_ordered(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, const float* t_add,
                                    void* dt16, float* dbias, float* dbias2, int64_t rows, int cols, float eps, float alpha, float p_drop,
                                    uint64_t seed, int dtype16, float* partials, int64_t partial_elems, void* stream);
/* cir_rows16_colsum (both modes) likewise; sums is required.  Workgroup b covers rows 64 b .. 64 b + 63: row lane l (0 .. 7) adds rows
 * 64 b + 8 i + l for i = 0 .. 7 in order, the lanes are added 0 + 1 + ... + 7 left to right, the sums go to row b of partials, then the
 * finishing sum.  partial_elems >= ceil(rows / 64) * cols.  `out` (mode 1) is bit-identical to the plain form's. */
int cir_rows16_colsum_ordered(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, float* sums, int64_t rows, int cols,
                              int mode, int dtype, float* partials, int64_t partial_elems, void* stream);
/* cir_rows16_gelu_pair (vit.py:36-37, 103-105) with the sums in the fixed order of cir_rows16_colsum_ordered (the same workgroups, the same
 * partials, the same finishing sum: the same bits as its mode 1).  partials is required, partial_elems >= ceil(rows / 64) * cols when sums
 * is given; with sums NULL no sum is formed.  out / out_f are bit-identical to the plain form's. */
int cir_rows16_gelu_pair_ordered(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, void* out_f, int64_t ldf, float* sums,
                                 int64_t rows, int cols, int dtype, float* partials, int64_t partial_elems, void* stream);
/* cir_embed_bwd in a fixed order; ids outside [0, table_rows) are skipped.
 * dword: the rows are cut into chunks of 512.  Inside a chunk the rows of one id are added in ascending row order, starting from the first
 * of them.  With one chunk that sum is added to dword[id].  Otherwise the chunk sums of an id are added in ascending chunk order, starting
 * from the first chunk that holds the id, and the total is added to dword[id] (one plain read-modify-write per element: each id has one
 * owner).  A heavy id - the padding id fills half of a stage-I batch - is so summed by many workgroups of at most 512 rows each.
 * dpos[l] += the ordered column sum (cir_colsum_ordered's order) of dy read as (ceil(rows / L), L * cols) - the rows r = l, l + L, l + 2 L, ...
 * of dy; a short last sequence simply ends the lists of the positions it lacks.
 * index: int32 workspace, index_elems >= ceil(rows / 512) * table_rows (first row of each id per chunk, by integer atomic min);
 * partial_elems >= max(rows * cols if rows > 512, S * L * cols if S > 1) with S = ceil(ceil(rows / L) / 256). */
int cir_embed_bwd_ordered(const int64_t* ids, const float* dy, float* dword, float* dpos, int64_t rows, int L, int cols, int64_t table_rows,
                          float* partials, int64_t partial_elems, int32_t* index, int64_t index_elems, void* stream);
/* The weight gradients need no twin: cir_wgrad / cir_wgrad_grouped with splits = 1 give every 128 x 128 tile of dw to ONE workgroup, which
 * adds its sum over all 64-row steps with a plain read-modify-write; the tail (rows % 64) then runs as ONE cir_bmm batch item (accumulate 2,
 * nb1 = nb2 = 1) after it on the same stream: every element of dw has exactly one adder there too, so the atomic add is old + value.  cir_bmm
 * with accumulate 1 and one batch item per C is a single read-modify-write per element as well. */
/* torch.optim.AdamW step in place on fp32 parameter / moments (stage2_train.py:120-126 builds that optimizer). */
int cir_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int step, void* stream);
/* The same step with GradScaler.step's found_inf decision (stage2_train.py:215-218: `scaler.step(optimizer)` skips the update when the
 * unscaled gradients hold an inf / NaN) taken ON THE DEVICE - no host read between backward and the update (ABI 15).  `state` = 8 x 32 bit
 * of device memory, zero-initialised by the caller once: [0] found_inf of the step in flight (the caller clears it before the first check of
 * a step), [1] applied steps t, [2] skipped steps, [3] / [4] fp32 bias corrections 1 - beta^t of the step in flight.
 *   cir_grads_check     g[i] *= scale (scale != 1: GradScaler.unscale_) and state[0] |= any non-finite g[i]; one pass over g.
 *   cir_adamw_begin     after every check of the step: flag set -> state[2] += 1; else state[1] += 1 and the corrections for the new t.
 *   cir_adamw_step_dev  cir_adamw_step's update with t / corrections from `state`; a no-op while state[0] is set.  `p16` (optional):
 *                       the 16-bit operand copy of the updated parameters (dtype16 = CIR_F16 / CIR_BF16), written in the same pass. */
int cir_grads_check(float* g, int64_t n, float scale, int32_t* state, void* stream);
int cir_adamw_begin(int32_t* state, float beta1, float beta2, void* stream);
int cir_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       const int32_t* state, void* p16, int dtype16, void* stream);
/* Parameter groups and clip_grad_norm_ on the same device state (additive within ABI 15).  The reference builds ONE group
 * (stage2_train.py:138) and steps it under the scaler (:215-218); its schedules write every group's lr (utils.py:216-241).  A trained ViT
 * beside the text encoders wants a lower rate for visual_encoder.*, no decay on biases / LayerNorm / pos_embed / cls_token, and a bound on
 * the gradient norm - all decided where the gradients are, without a host read.  state[5] = fp32 clip coefficient, state[6] = fp32
 * pre-clip norm of the step in flight; state[7] stays free.
 *   cir_grads_sumsq            one read-only pass over g (n >= 1 fp32, 16-byte aligned): state[0] |= any non-finite element (cir_grads_check's
 *                              test; state[1..7] untouched) and partials[b] = the float64 sum of squares workgroup b read.  Fixed order, no
 *                              float atomics: the partials repeat bit for bit.  The grid is a function of n alone.
 *   cir_grads_sumsq_workspace  pure host function: the number of doubles cir_grads_sumsq(n) writes (CIR_EINVAL for n < 1).
 *   cir_adamw_begin_clip       cir_adamw_begin + the clip, after the norm passes of EVERY work item of the step wrote their partials side by
 *                              side: total_norm = fp32(sqrt(sum of the n_partials doubles, in index order with a fixed tree)),
 *                              coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 (torch.nn.utils.clip_grad_norm_), state[5] = coef,
 *                              state[6] = total_norm.  Flag set: state[2] += 1, state[1] / [3] / [4] stay, state[6] = the norm as summed
 *                              (inf / NaN possible), state[5] = 0.  max_norm finite and > 0 (CIR_EINVAL).
 *   cir_adamw_step_groups      cir_adamw_step_dev with (lr, weight_decay, eps) per float4: `groups` holds up to CIR_ADAMW_MAX_GROUPS triples
 *                              and travels BY VALUE as a kernel argument (a schedule that rewrites lr uploads nothing).  seg_end / seg_group:
 *                              DEVICE arrays of nseg ascending segment END offsets in elements - every end a multiple of 8, the last = n -
 *                              and one group id per segment (the trainers' slabs pad each parameter to 8 elements: no float4 straddles
 *                              two parameters; the padding belongs to the segment before it).  Both NULL with nseg = 1: every element
 *                              takes group `group` - the per-tensor form, the only one whose n may be no multiple of 4.  clip != 0:
 *                              g is multiplied by state[5] in registers (one fp32 rounding); g itself is never written.  nseg = 1 without
 *                              clip has the bits of cir_adamw_step_dev.  The table lives on the device, so this entry point CANNOT check
 *                              it: a C caller gets no refusal for a bad table.  The kernel never reads outside the nseg entries and takes
 *                              every id modulo 8; an id in ngroups..7 then selects a triple of `groups` the caller did not fill - with a
 *                              zero-initialised struct lr = 0, weight_decay = 0, eps = 0: m and v are updated, p keeps its value (0 / 0 =
 *                              NaN where v' is 0) - and ends that do not ascend or are no multiples of 8 give elements another segment's
 *                              scalars.  Check the table where it is built, as train_ops.SegmentTable does on the host.
 *                              CIR_EINVAL: nseg < 1, ngroups outside 1..8, `group` outside 0..ngroups-1, one of the two arrays NULL, a
 *                              table with n % 4 != 0; CIR_EALIGN: p, g, m, v not 16-byte, p16 / seg_end not 8-byte, seg_group not 4-byte
 *                              aligned; CIR_EDTYPE: p16 with a dtype16 other than CIR_F16 / CIR_BF16. */
#define CIR_ADAMW_MAX_GROUPS 8
typedef struct cir_adamw_groups {
    float lr[CIR_ADAMW_MAX_GROUPS], weight_decay[CIR_ADAMW_MAX_GROUPS], eps[CIR_ADAMW_MAX_GROUPS];
} cir_adamw_groups;
int cir_grads_sumsq(const float* g, int64_t n, int32_t* state, double* partials, void* stream);
int64_t cir_grads_sumsq_workspace(int64_t n);
int cir_adamw_begin_clip(int32_t* state, float beta1, float beta2, const double* partials, int64_t n_partials, float max_norm, void* stream);
int cir_adamw_step_groups(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, const int32_t* state,
                          const int64_t* seg_end, const int32_t* seg_group, int nseg, int group, const cir_adamw_groups* groups, int ngroups,
                          int clip, void* p16, int dtype16, void* stream);
/* Contrastive head of the stage-I training step (blip_stage1.py:83-91; driven by stage1_train.py:170-172):
 *   p_hat = F.normalize(p) = p / max(||p||, 1e-12),   logits = p_hat target^T / temp
 * p (B, E) fp32 = text_proj of the CLS rows; target (Bt, E) fp32, used as given (the reference's pooled target features are already
 * normalised); temp = DEVICE pointer to the fp32 scalar parameter (no host read).  Outputs p_hat (B, E), inv_norm (B) = 1 / max(||p||, 1e-12),
 * logits (B, Bt), all contiguous fp32.
 * cir_contrastive_bwd, from dlogits (B, Bt):  dp_hat = dlogits target / temp,  dp = (dp_hat - p_hat (p_hat . dp_hat)) inv_norm  (written to dp),
 * dtemp = -sum dlogits * logits / temp = -sum_i (p_hat_i . dp_hat_i) / temp  WRITTEN (not added) to *dtemp; row_scratch: fp32 (B) work space.
 * Optionally (x, W, dx, dW, db all given, or all NULL) text_proj's adjoint in the same call: x (B, D) rows at stride ldx (the CLS rows of the
 * fp32 stream), W (E, D) the text_proj weight; dx (B, D) at stride lddx = dp W, dW (E, D) = dp^T x, db (E) = column sums of dp - all WRITTEN.
 * Every reduction runs in a fixed order without atomics: the outputs repeat bit for bit.  dtype: CIR_F32 only (CIR_EDTYPE otherwise).
 * E % 4 == 0, E <= 1024, B <= 65535, B * Bt < 2^31 (CIR_ESHAPE); D % 4 == 0 and ldx, lddx >= D, multiples of 4; 16-byte aligned matrices,
 * 4-byte aligned scalars / vectors (temp, inv_norm, row_scratch, dtemp). */
int cir_contrastive_fwd(const float* p, const float* target, const float* temp, float* p_hat, float* inv_norm, float* logits, int B, int Bt, int E,
                        int dtype, void* stream);
int cir_contrastive_bwd(const float* dlogits, const float* target, const float* temp, const float* p_hat, const float* inv_norm, float* dp,
                        float* row_scratch, float* dtemp, const float* x, int64_t ldx, const float* W, float* dx, int64_t lddx, float* dW, float* db,
                        int D, int B, int Bt, int E, int dtype, void* stream);
/* Image side of the stage-I training step with a trained image encoder (stage1_train.py --blip-img-tune: :144-190 / :383-425; additive
 * within ABI 15).  Same conventions as the pair above: fp32 only (CIR_EDTYPE otherwise), fixed-order reductions, no atomics - every output
 * repeats bit for bit.
 *   cir_contrastive_bwd_target (blip_stage1.py:91, the adjoint w.r.t. target_features - the transposed product cir_contrastive_bwd does not
 *     form):  dtarget[j][:] = (1 / temp) sum_i dlogits[i][j] p_hat[i][:],  dlogits (B, Bt), p_hat (B, E), dtarget (Bt, E) WRITTEN, temp a
 *     DEVICE pointer.  E % 4 == 0, E <= 1024, B, Bt <= 65535, B * Bt < 2^31.
 *   cir_pooled_head_fwd (blip_stage1.py:57: F.normalize(vision_proj(image_embeds[:, 0, :]))):  t = x W^T + b,  t_hat = t / max(||t||, 1e-12).
 *     x = Bt rows of D at stride ldx - the CLS rows of a (Bt, N, D) token tensor read in place with ldx = N * D -, W (E, D), b (E); writes
 *     t_hat (Bt, E) and inv_norm (Bt) = 1 / max(||t||, 1e-12).  t_hat has the bits of cir_l2_normalize(cir_linear_f32(x, W, b)): the same
 *     FMA chains in the same order.
 *   cir_pooled_head_bwd, from dt_hat (Bt, E):  dt = inv_norm (dt_hat - t_hat (t_hat . dt_hat)) (a row the epsilon clamped: dt = dt_hat /
 *     1e-12, as F.normalize differentiates) WRITTEN to dt (Bt, E, work space and result);  dW (E, D) += dt^T x and db (E) += column sums of
 *     dt - both ADDED to what is there (the mini-batches of one step each contribute; rows in order, one adder per element);  dx = dt W
 *     WRITTEN into Bt rows of D at stride lddx - the CLS rows of a (Bt, N, D) token-gradient tensor; the other rows are NOT touched: the
 *     caller zeroes them.  dx may be NULL (frozen image encoder: vision_proj's gradients only).
 * E % 4 == 0, E <= 1024, D % 4 == 0, D <= 2048, Bt <= 65535, ldx / lddx >= D and multiples of 4; 16-byte aligned matrices and rows, 4-byte
 * aligned vectors (b, db, inv_norm). */
int cir_contrastive_bwd_target(const float* dlogits, const float* p_hat, const float* temp, float* dtarget, int B, int Bt, int E, int dtype,
                               void* stream);
int cir_pooled_head_fwd(const float* x, int64_t ldx, const float* W, const float* bias, float* t_hat, float* inv_norm, int Bt, int E, int D,
                        int dtype, void* stream);
int cir_pooled_head_bwd(const float* dt_hat, const float* t_hat, const float* inv_norm, const float* x, int64_t ldx, const float* W, float* dt,
                        float* dx, int64_t lddx, float* dW, float* db, int Bt, int E, int D, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CIRRANK_H */
