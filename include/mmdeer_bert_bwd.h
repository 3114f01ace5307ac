/* mmdeer -- C ABI of the BERT trunk's BACKWARD operators (csrc/bert_bwd.hip): the gradients of the three operators of
 * include/mmdeer_bert.h that a fine-tuned BertModel layer needs beyond mmdeer_gemm -- masked multi-head self-attention, residual
 * add + LayerNorm and the erf GELU.  The Linear layers' gradients are mmdeer_gemm calls (dX = dY W with trans_w, dW = dY^T X with
 * trans_a and trans_w, bias_grad).  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding),
 * exported by the same library and covered by the same MMDEER_ABI_VERSION.  The conventions are mmdeer_bert.h's: every call
 * enqueues on `stream`, never synchronises and allocates nothing; a refused call writes nothing, returns -1 and leaves its reason
 * in mmdeer_last_error(), and every refusal is decided on the host before any HIP runtime call; "act" = fp32 when act_f32 != 0,
 * else bf16.  A call without rows (B = 0 or M = 0) writes nothing and returns 0 once its shape has passed the checks; its pointers
 * are not looked at.  No atomics: every sum has one owner and a fixed order, so two runs of a call on the same operands store the
 * same bits.  Rows are batch-major: row b * L + t is token t of sample b. */
#ifndef MMDEER_BERT_BWD_H_
#define MMDEER_BERT_BWD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the most workgroups whose partial column sums mmdeer_bert_add_ln_bwd leaves in its scratch */
#define MMDEER_BERT_LN_BWD_PARTS 1024

/* ---- mmdeer_bert_attn_bwd: the backward of mmdeer_bert_attn_fwd, two launches, heads = H / 64.
 *   qkv    act [B * L][ld_qkv]: the forward's input, columns [Q | K | V]
 *   mask   fp32 [B * L]: the forward's
 *   dctx   act [B * L][ld_dctx]: the gradient of ctx
 *   dqkv   act, row stride ld_dqkv, columns [dQ | dK | dV]: columns [0, 3 H) of rows [0, B * L) are written, nothing else
 *   workspace  fp32, the CALLER's: the row statistics [2][B][heads][L] (log-sum-exp, then delta); mmdeer_bert_attn_bwd_workspace
 *              gives its size in BYTES, workspace_bytes is what the caller has
 * Per sample and head, over the VALID keys j:  P = softmax(Q K^T / 8),  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - delta),
 * dQ = dS K / 8,  dK = dS^T Q / 8.  The semantics are the forward's: a masked key is excluded exactly, so its dK and dV rows are
 * exact zeros; a masked QUERY row attends, receives its dQ and contributes to dK and dV; a sample without a valid key gets exact
 * zeros in all of dqkv (the forward's one deviation, mirrored).
 * delta_i = sum_j P_ij dP_ij is summed from the call's own P and dP, not from the forward's stored output (which the call does not
 * take): with a single valid key P = 1 and delta = dP to the bit, so dQ and dK are the exact zeros of exact arithmetic.
 * Every output element has one owner.  Launch 1, one workgroup per (sample, head, 64 query rows), walks the keys twice: first the
 * running maximum, sum and delta, which go to the workspace as log-sum-exp and delta (the statistics are recomputed from qkv here;
 * mmdeer_bert_attn_fwd keeps nothing), then dQ.  Launch 2, one workgroup per (sample, head, 64 keys), walks the queries for dK
 * and dV.  bf16: all four products of each launch on mfma_f32_32x32x16_bf16 with fp32 accumulation; scores, P and dS are fp32
 * in registers and rounded to bf16 only as MFMA operands.  The dQ kernel holds K, V and K^T in LDS tiles of 128 keys (53,888 bytes,
 * 180 VGPRs); the dK / dV kernel holds Q, dO and their transposes in tiles of 64 queries (36,352 bytes, 172 VGPRs); neither spills.
 * fp32: plain-FMA kernels, one thread per query row and one per key (parity, not speed).  Rows past L of a last tile are
 * zero-filled in LDS and never stored; nothing is read beyond B * L rows.
 * Refuses: a NULL args pointer; H % 64 != 0, H < 64 or H > MMDEER_BERT_MAX_HIDDEN (1024); B < 0; L < 1 with B > 0, L < 0;
 * L > MMDEER_BERT_MAX_TOKENS (512); ld_qkv < 3 H, ld_dqkv < 3 H or ld_dctx < H, or one of the three not a multiple of 8;
 * B * L * ld >= 2^31 for any of the three; with B > 0: a NULL qkv, mask, dctx, dqkv or workspace; workspace_bytes below
 * mmdeer_bert_attn_bwd_workspace(B, L, H); qkv, dctx, dqkv or workspace not 16-byte aligned; mask not 4-byte aligned. */
typedef struct mmdeer_bert_attn_bwd_args {
  const void* qkv;
  const float* mask;
  const void* dctx;
  void* dqkv;
  float* workspace;
  long long workspace_bytes;
  int32_t B, L, H, ld_qkv, ld_dctx, ld_dqkv, act_f32;
  void* stream;
} mmdeer_bert_attn_bwd_args;
int mmdeer_bert_attn_bwd(const mmdeer_bert_attn_bwd_args* a);
/* bytes of workspace for a call of that shape (0 without rows); -1 for a shape the call refuses */
long long mmdeer_bert_attn_bwd_workspace(int32_t B, int32_t L, int32_t H);

/* ---- mmdeer_bert_add_ln_bwd: the backward of out = LayerNorm(y + x; gamma, beta, eps) from the forward's INPUTS.
 *   y, x   act [M] rows of N, row strides ld_y, ld_x; x may be NULL.  s = y + x, its mean and rstd are recomputed in fp32 exactly as
 *          the forward computes them (one wave per row, the row in registers), and xhat = (s - mean) rstd from them -- never from
 *          `out`, which loses xhat where gamma = 0.
 *   g      act [M][ld_g]: the gradient of out
 *   g2     act [M][ld_g2] or NULL: a second gradient of the same tensor (the one that arrives by the residual branch); G = g + g2 in
 *          fp32 before anything else
 *   gamma  fp32 [N]
 *   ds     act, row stride ld_ds: the gradient of s, which is the gradient of y and of x alike:
 *          ds = rstd (G gamma - mean_n(G gamma) - xhat mean_n(G gamma xhat)).  Columns [0, N) of rows [0, M) are written, nothing
 *          else.  ds may alias g or g2 (same rows, same leading dimension).
 *   dgamma, dbeta  fp32 [N], written: dgamma = sum_m G xhat, dbeta = sum_m G.  Both NULL: no sums are formed and scratch is not
 *          looked at.  Each of at most MMDEER_BERT_LN_BWD_PARTS workgroups sums its rows in row order and leaves one partial pair in
 *          `scratch`; a second launch folds the partials in a fixed order.
 *   scratch  fp32, the caller's, mmdeer_bert_add_ln_bwd_scratch(M, N) ELEMENTS, scratch_elems is what the caller has
 * Refuses: a NULL args pointer; N % 4 != 0, N < 4 or N > MMDEER_BERT_MAX_HIDDEN; M < 0; a leading dimension (ld_x only with x,
 * ld_g2 only with g2) below N or not a multiple of 4; eps < 0 or not finite; M * ld >= 2^31 for any operand; exactly one of dgamma
 * and dbeta NULL; with M > 0: a NULL y, g, gamma or ds; with the sums: a NULL scratch or scratch_elems below the sizing entry's;
 * gamma, dgamma, dbeta or scratch not 16-byte aligned; y, x, g, g2 or ds not aligned to 4 act elements. */
typedef struct mmdeer_bert_add_ln_bwd_args {
  const void* y;
  const void* x;
  const void* g;
  const void* g2;
  const float* gamma;
  void* ds;
  float* dgamma; float* dbeta;
  float* scratch;
  long long scratch_elems;
  float eps;
  int32_t M, N, ld_y, ld_x, ld_g, ld_g2, ld_ds, act_f32;
  void* stream;
} mmdeer_bert_add_ln_bwd_args;
int mmdeer_bert_add_ln_bwd(const mmdeer_bert_add_ln_bwd_args* a);
/* fp32 elements of scratch for the column sums of a call of that shape (0 for M = 0); -1 for a shape the call refuses */
long long mmdeer_bert_add_ln_bwd_scratch(int32_t M, int32_t N);

/* ---- mmdeer_bert_gelu_bwd: dx = g (Phi(x) + x phi(x)) with Phi(x) = (1 + erf(x / sqrt 2)) / 2 and phi(x) = exp(-x^2 / 2) / sqrt(2 pi):
 * the derivative of the erf form, from the PRE-activation x, computed in fp32 on 4-element chunks.
 *   x    act [M] rows of N, row stride ld_x: the forward's input
 *   g    act [M][ld_g]: the gradient of gelu(x)
 *   dx   act, row stride ld_dx: columns [0, N) of rows [0, M) are written, nothing else.  In place over g (dx == g, ld_dx == ld_g) is allowed.
 * Refuses: a NULL args pointer; N % 4 != 0 or N < 4; M < 0; a leading dimension below N or not a multiple of 4; M * ld >= 2^31 for
 * any of the three; with M > 0: a NULL x, g or dx; x, g or dx not aligned to 4 act elements. */
typedef struct mmdeer_bert_gelu_bwd_args {
  const void* x;
  const void* g;
  void* dx;
  int32_t M, N, ld_x, ld_g, ld_dx, act_f32;
  void* stream;
} mmdeer_bert_gelu_bwd_args;
int mmdeer_bert_gelu_bwd(const mmdeer_bert_gelu_bwd_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_BERT_BWD_H_ */
