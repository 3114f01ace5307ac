/* mmdeer -- C ABI of the BERT trunk's forward operators (csrc/bert.hip): what a BertModel layer needs beyond mmdeer_gemm -- the
 * embedding sum with its LayerNorm, masked multi-head self-attention over the tokens of a sample, residual add + LayerNorm with the
 * eps as an argument, and the erf GELU.  The Linear layers of the trunk run on mmdeer_gemm (mmdeer.h) as it is.  A companion of
 * mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding), exported by the same library and covered by the same
 * MMDEER_ABI_VERSION.  The conventions are mmdeer.h's: every call enqueues on `stream`, never synchronises and allocates nothing; a
 * refused call writes nothing, returns -1 and leaves its reason in mmdeer_last_error(), and every refusal is decided on the host
 * before any HIP runtime call; "act" = fp32 when act_f32 != 0, else bf16.  A call without rows (B = 0 or M = 0) writes nothing and
 * returns 0 once its shape has passed the checks; its pointers are not looked at.  No atomics: two runs of a call on the same
 * operands store the same bits.  Rows are batch-major: row b * L + t is token t of sample b. */
#ifndef MMDEER_BERT_H_
#define MMDEER_BERT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDEER_BERT_HEAD_DIM 64
#define MMDEER_BERT_MAX_HIDDEN 1024
#define MMDEER_BERT_MAX_TOKENS 512

/* ---- mmdeer_bert_embed_fwd: BertEmbeddings without dropout, one launch.
 *   x[b * L + t][0, H) = LayerNorm(word[clamp(ids[b * L + t])] + pos[t] + type[tt]; gamma, beta, eps)   (biased variance, fp32 statistics)
 *   tt = type_ids == NULL ? 0 : clamp(type_ids[b * L + t]).  Ids are CLAMPED to [0, V) and type ids to [0, T) for memory safety, as
 *   mmdeer_token_embed_fwd clamps its ids (torch raises on such an id; checking here would cost a device sync).
 *   ids       int64 [B * L]
 *   type_ids  int64 [B * L] or NULL
 *   word      fp32 [V][H];  pos fp32 [P][H];  type fp32 [T][H];  gamma, beta fp32 [H]
 *   x         act, row stride ld_x elements: columns [0, H) of rows [0, B * L) are written, nothing else
 * Refuses: a NULL args pointer; H % 64 != 0, H < 64 or H > MMDEER_BERT_MAX_HIDDEN; B < 0, L < 0, V < 1, P < 1, T < 1; L > P
 * (max_position_embeddings); ld_x < H or ld_x % 4 != 0; eps < 0 or not finite; B * L * ld_x >= 2^31; with B * L > 0: a NULL ids,
 * word, pos, type, gamma, beta or x; ids / type_ids not 8-byte aligned; a table, gamma or beta not 16-byte aligned; x not aligned
 * to 4 act elements. */
typedef struct mmdeer_bert_embed_args {
  const long long* ids;
  const long long* type_ids;
  const float* word; const float* pos; const float* type;
  const float* gamma; const float* beta;
  void* x;
  float eps;
  int32_t B, L, H, V, P, T, ld_x, act_f32;
  void* stream;
} mmdeer_bert_embed_args;
int mmdeer_bert_embed_fwd(const mmdeer_bert_embed_args* a);

/* ---- mmdeer_bert_attn_fwd: masked multi-head self-attention of BertSelfAttention (no dropout), one launch, heads = H / 64.
 *   qkv   act [B * L][ld_qkv]: columns [Q | K | V], each H wide, head h at columns [64 h, 64 h + 64) of its block
 *   mask  fp32 [B * L]: key b * L + t is valid iff mask != 0 (an arbitrary binary pattern, not necessarily a prefix)
 *   ctx   act, row stride ld_ctx: ctx[b * L + i][64 h + d] = sum_j softmax_j(Q_i . K_j / 8) V_j[d] over the VALID keys j of sample b.
 *         Columns [0, H) of rows [0, B * L) are written, nothing else.
 * Masked keys are excluded exactly (their probability is 0, not exp(finfo.min)): for a sample with at least one valid key this is
 * what the additive finfo.min mask of the reference computes.  Every query row, masked or not, attends to the valid keys of its
 * sample and is written.  THE ONE DEVIATION: a sample without a valid key gets ZEROS in all its ctx rows (the reference gives a
 * rounding-dependent uniform average of V there); nothing downstream of the trunk reads such a sample un-multiplied by its mask.
 * bf16: mfma_f32_32x32x16_bf16 for Q K^T and P V with fp32 accumulation, the softmax (running maximum and sum over key tiles) in
 * fp32, P rounded to bf16 for the second product.  fp32: a plain-FMA kernel with the same running softmax (parity, not speed).
 * One workgroup per (sample, head, 64 query rows); rows past L of the last query or key tile are predicated, never read.
 * Refuses: a NULL args pointer; H % 64 != 0, H < 64 or H > MMDEER_BERT_MAX_HIDDEN; B < 0; L < 1 with B > 0, L < 0;
 * L > MMDEER_BERT_MAX_TOKENS; ld_qkv < 3 H or ld_qkv % 8 != 0; ld_ctx < H or ld_ctx % 4 != 0; B * L * ld_qkv >= 2^31; with B > 0: a
 * NULL qkv, mask or ctx; qkv not 16-byte aligned; mask not 4-byte aligned; ctx not aligned to 4 act elements. */
typedef struct mmdeer_bert_attn_args {
  const void* qkv;
  const float* mask;
  void* ctx;
  int32_t B, L, H, ld_qkv, ld_ctx, act_f32;
  void* stream;
} mmdeer_bert_attn_args;
int mmdeer_bert_attn_fwd(const mmdeer_bert_attn_args* a);

/* ---- mmdeer_bert_add_ln_fwd: BertSelfOutput / BertOutput behind their Linear: out = LayerNorm(y + x; gamma, beta, eps), row by row
 * (biased variance; the sum, the statistics and the normalisation in fp32; two passes over the row in registers).
 *   y, x  act [M] rows of N, row strides ld_y, ld_x;  x may be NULL (plain LayerNorm of y)
 *   out   act, row stride ld_out: columns [0, N) of rows [0, M) are written, nothing else.  out may alias y or x (same rows).
 * Refuses: a NULL args pointer; N % 4 != 0, N < 4 or N > MMDEER_BERT_MAX_HIDDEN; M < 0; a leading dimension below N or not a
 * multiple of 4; eps < 0 or not finite; M * ld >= 2^31 for any of the three; with M > 0: a NULL y, gamma, beta or out; gamma or
 * beta not 16-byte aligned; y, x or out not aligned to 4 act elements. */
typedef struct mmdeer_bert_add_ln_args {
  const void* y;
  const void* x;
  const float* gamma; const float* beta;
  void* out;
  float eps;
  int32_t M, N, ld_y, ld_x, ld_out, act_f32;
  void* stream;
} mmdeer_bert_add_ln_args;
int mmdeer_bert_add_ln_fwd(const mmdeer_bert_add_ln_args* a);

/* ---- mmdeer_bert_gelu_fwd: out = 0.5 x (1 + erf(x / sqrt 2)), the exact erf form (hidden_act = "gelu"), computed in fp32.
 *   x    act [M] rows of N, row stride ld_x
 *   out  act, row stride ld_out: columns [0, N) of rows [0, M) are written, nothing else.  In place (out == x, ld_out == ld_x) is allowed.
 * Refuses: a NULL args pointer; N % 4 != 0 or N < 4; M < 0; a leading dimension below N or not a multiple of 4; M * ld >= 2^31 for
 * either; with M > 0: a NULL x or out; x or out not aligned to 4 act elements. */
typedef struct mmdeer_bert_gelu_args {
  const void* x;
  void* out;
  int32_t M, N, ld_x, ld_out, act_f32;
  void* stream;
} mmdeer_bert_gelu_args;
int mmdeer_bert_gelu_fwd(const mmdeer_bert_gelu_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_BERT_H_ */
