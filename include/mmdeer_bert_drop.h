/* mmdeer -- C ABI of the BERT trunk's DROPOUT operators (csrc/bert_drop.hip): the five operators of include/mmdeer_bert.h and
 * include/mmdeer_bert_bwd.h that carry a dropout site of transformers.BertModel in train() -- the embedding LayerNorm, the attention
 * probabilities and the residual add + LayerNorm behind BertSelfOutput's and BertOutput's dense -- each with that dropout inside the
 * same launch.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding), exported by the same
 * library and covered by the same MMDEER_ABI_VERSION.  Each args struct is its plain counterpart's plus
 *   site       the dropout site id, >= 0
 *   dropout_p  the probability of dropping an element, finite and in [0, 1)
 *   seed, offset  the user seed and the step counter of the library's counter-hash dropout (mmdeer.h: mmdeer_dropout_mask)
 * and conventions and refusals are the counterpart's; in addition each call refuses a dropout_p that is not finite or lies outside
 * [0, 1), and a negative site.  dropout_p == 0 runs the plain entry's kernel and stores its bits.
 *
 * THE MASK, stated once.  Element (row, col) of a site is kept iff mmdeer_dropout_mask keeps it:
 *   mix32((row * 0x9E3779B1) ^ (col * 0x85EBCA77) ^ key(seed, offset, site)) < floor((1 - p) 2^32),   m = keep * float(1 / (1 - p))
 * with no column shift.  Masks are regenerated wherever they are needed and never stored.
 *   hidden sites (embed, drop_add_ln)   row = b * L + t (the row of the operand), col = n in [0, N)
 *   attention site                      row = (b * heads + h) * L + i (the query), col = j (the key)
 * The caller chooses the site ids; mmdeer/bert.py uses MMDEER_BERT_DROP_SITE_EMBED for the embeddings and
 * MMDEER_BERT_DROP_SITE_LAYER0 + 4 * layer + {0: attention, 1: self-output, 2: output}, a block above every other site id of the
 * package (all below 200).
 *
 * THE DEVICE COUNTER.  include/mmdeer_graph.h declares a twin mmdeer_<entry>_dev(args, offset_dev) of each entry, which adds a
 * device-resident counter to `offset` when the kernel runs (HIP-graph replays).  The entries here are its NULL-counter case: the same
 * kernels, in which every wave forms key(seed, offset, site) once, in scalar registers, before its first element. */
#ifndef MMDEER_BERT_DROP_H_
#define MMDEER_BERT_DROP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDEER_BERT_DROP_SITE_EMBED 256
#define MMDEER_BERT_DROP_SITE_LAYER0 260

/* ---- mmdeer_bert_embed_drop_fwd: mmdeer_bert_embed_fwd with BertEmbeddings' dropout behind the LayerNorm, one launch:
 *   x[b * L + t][n] = m[b * L + t][n] * LayerNorm(word + type + pos)[n], the product in fp32 before the one rounding to act. */
typedef struct mmdeer_bert_embed_drop_args {
  const long long* ids;
  const long long* type_ids;
  const float* word; const float* pos; const float* type;
  const float* gamma; const float* beta;
  void* x;
  float eps;
  int32_t B, L, H, V, P, T, ld_x, act_f32;
  int32_t site;
  float dropout_p;
  uint64_t seed, offset;
  void* stream;
} mmdeer_bert_embed_drop_args;
int mmdeer_bert_embed_drop_fwd(const mmdeer_bert_embed_drop_args* a);

/* ---- mmdeer_bert_attn_drop_fwd: mmdeer_bert_attn_fwd with the dropout of BertSelfAttention on the probabilities, one launch:
 *   P = softmax(Q K^T / 8) over the valid keys as in the plain entry, ctx = (P o m) V.
 * The softmax sum runs over the UNDROPPED probabilities (bf16: over the rounded ones, as in the plain kernel); only the operand of the
 * second product is masked, with keep alone, and 1 / (1 - p) is applied in fp32 to the accumulator together with 1 / l.  A block
 * of 32 keys without a valid one is skipped as before.  A query all of whose valid keys are dropped stores exact zeros.  bf16: a
 * lane holds 16 keys of one query, so the keep decision is one mix32 per held element from a per-lane row key. */
typedef struct mmdeer_bert_attn_drop_args {
  const void* qkv;
  const float* mask;
  void* ctx;
  int32_t B, L, H, ld_qkv, ld_ctx, act_f32;
  int32_t site;
  float dropout_p;
  uint64_t seed, offset;
  void* stream;
} mmdeer_bert_attn_drop_args;
int mmdeer_bert_attn_drop_fwd(const mmdeer_bert_attn_drop_args* a);

/* ---- mmdeer_bert_drop_add_ln_fwd: out = LayerNorm(drop(y) + x; gamma, beta, eps): mmdeer_bert_add_ln_fwd with the hidden dropout
 * on the dense output y.  s = y m + x is formed in fp32 from the stored y; out may alias y or x (same rows), as in the plain entry. */
typedef struct mmdeer_bert_drop_add_ln_args {
  const void* y;
  const void* x;
  const float* gamma; const float* beta;
  void* out;
  float eps;
  int32_t M, N, ld_y, ld_x, ld_out, act_f32;
  int32_t site;
  float dropout_p;
  uint64_t seed, offset;
  void* stream;
} mmdeer_bert_drop_add_ln_args;
int mmdeer_bert_drop_add_ln_fwd(const mmdeer_bert_drop_add_ln_args* a);

/* ---- mmdeer_bert_attn_drop_bwd: the backward of mmdeer_bert_attn_drop_fwd; mmdeer_bert_attn_bwd's two launches, ownership, masked-key,
 * masked-query and dead-sample semantics, no atomics.  Per sample and head, over the valid keys, with k = keep and c = 1 / (1 - p):
 *   dV = c (P o k)^T dO,  dPd = dO V^T,  delta_i = c sum_j P_ij k_ij dPd_ij,  dS = P o (m o dPd - delta),  dQ = dS K / 8,  dK = dS^T Q / 8
 * c is factored out of every product: the kernels sum delta' = sum_j P_ij k_ij dPd_ij from their own P and dPd as the plain kernels
 * sum delta (the workspace holds the log-sum-exp and delta'), form P o (k o dPd - delta') and apply c in fp32 to the accumulators of
 * dQ, dK and dV.  With a single valid key P = 1 and delta' = k dPd to the bit, so dQ and dK are exact zeros whether the key is kept
 * or dropped.  Both launches regenerate k from (row, col).  The workspace is mmdeer_bert_attn_bwd's in size and alignment;
 * mmdeer_bert_attn_drop_bwd_workspace gives the bytes. */
typedef struct mmdeer_bert_attn_drop_bwd_args {
  const void* qkv;
  const float* mask;
  const void* dctx;
  void* dqkv;
  float* workspace;
  long long workspace_bytes;
  int32_t B, L, H, ld_qkv, ld_dctx, ld_dqkv, act_f32;
  int32_t site;
  float dropout_p;
  uint64_t seed, offset;
  void* stream;
} mmdeer_bert_attn_drop_bwd_args;
int mmdeer_bert_attn_drop_bwd(const mmdeer_bert_attn_drop_bwd_args* a);
/* bytes of workspace for a call of that shape (0 without rows); -1 for a shape the call refuses */
long long mmdeer_bert_attn_drop_bwd_workspace(int32_t B, int32_t L, int32_t H);

/* ---- mmdeer_bert_drop_add_ln_bwd: the backward of mmdeer_bert_drop_add_ln_fwd from the forward's INPUTS: mmdeer_bert_add_ln_bwd with
 * s recomputed as drop(y) + x, and TWO gradients:
 *   ds   act, row stride ld_ds: the gradient of s, which is the gradient of x (it goes on by the residual branch); may alias g or g2
 *   dy   act, row stride ld_dy: dy = ds o m from the fp32 ds, the gradient of the dense output y, which the two GEMMs behind it read;
 *        an exact zero where the element was dropped.  Columns [0, N) of rows [0, M) are written, nothing else.
 * dgamma, dbeta, scratch and the two-launch fold are the plain entry's.  Beyond its refusals: a NULL dy with M > 0, ld_dy below N or
 * not a multiple of 4, M * ld_dy >= 2^31, dy not aligned to 4 act elements. */
typedef struct mmdeer_bert_drop_add_ln_bwd_args {
  const void* y;
  const void* x;
  const void* g;
  const void* g2;
  const float* gamma;
  void* ds;
  void* dy;
  float* dgamma; float* dbeta;
  float* scratch;
  long long scratch_elems;
  float eps;
  int32_t M, N, ld_y, ld_x, ld_g, ld_g2, ld_ds, ld_dy, act_f32;
  int32_t site;
  float dropout_p;
  uint64_t seed, offset;
  void* stream;
} mmdeer_bert_drop_add_ln_bwd_args;
int mmdeer_bert_drop_add_ln_bwd(const mmdeer_bert_drop_add_ln_bwd_args* a);
/* fp32 elements of scratch for the column sums of a call of that shape (0 for M = 0); -1 for a shape the call refuses */
long long mmdeer_bert_drop_add_ln_bwd_scratch(int32_t M, int32_t N);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_BERT_DROP_H_ */
