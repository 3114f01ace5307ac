/* mmdeer -- C ABI of the temporal audio encoder's operators WITH PER-SAMPLE LENGTHS (csrc/lstm_seq.hip): the recurrence of one
 * bidirectional LSTM layer and the attention pool over time on a batch padded to T steps, in which sample b has lengths[b] = n_b valid
 * steps.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding), exported by the same library and
 * covered by the same MMDEER_ABI_VERSION.  Each args struct is its plain counterpart's (mmdeer_lstm_seq_args, mmdeer_temporal_pool_args)
 * plus, as its last field,
 *   lengths   const int32_t* in DEVICE memory, [B], 4-byte aligned.  The kernels clamp each value to [0, T] when they run; the host
 *             never dereferences the pointer, checks no value and does not synchronise, so a captured graph replays with whatever the
 *             buffer holds at that replay.
 * Conventions and refusals are the counterparts' (checked on the host before any HIP call, reason in mmdeer_last_error()), and one
 * more: lengths NULL or not 4-byte aligned (with T > 0 and B > 0).
 *
 * SEMANTICS.  Sample b is processed as that sample alone at its own length: torch's pack_padded_sequence(enforce_sorted=False) ->
 * nn.LSTM -> pad_packed_sequence(total_length=T) per layer, and a pool whose scores are -inf at t >= n_b.
 *   mmdeer_lstm_seq_len_fwd   both directions start sample b from zero state at its own first valid step (t = 0; t = n_b - 1 for the
 *       reverse direction).  h rows t >= n_b are stored as exact zeros, by the kernel, whatever xg holds there: xg is not read at
 *       t >= n_b (NaN and Inf included).  The tape rows of t >= n_b are NOT written; the backward does not read them.
 *   mmdeer_lstm_seq_len_bwd   dgates rows t >= n_b are stored as exact zeros; dh_out and the tape are not read there.  The reverse
 *       direction's cell state before step n_b - 1 is 0.  The caller's dW_hh GEMMs over the row-shifted views of h rely on the stored
 *       zero rows of h (the reverse direction's step n_b - 1 reads row n_b).
 *   mmdeer_temporal_pool_len_fwd   softmax over t < n_b; weights at t >= n_b are exact zeros; attended sums the valid steps.
 *       n_b = 0: a zero attended row and zero weights (no division).  h and z are not read at t >= n_b.
 *   mmdeer_temporal_pool_len_bwd   dh and dz rows t >= n_b are stored as exact zeros; dw2 is the deterministic two-launch fold of the
 *       plain entry; db2 an exact zero.
 * A workgroup of the recurrence steps only to the largest length among its rows and stores the zero rows beyond it in a plain loop.
 * With every length equal to T each entry stores the plain entry's bits. */
#ifndef MMDEER_SEQLEN_H_
#define MMDEER_SEQLEN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmdeer_lstm_seq_len_args {
  const void* xg; int32_t ld_xg;
  const void* w_hh;
  const void* w_hh_t;
  void* h; int32_t ld_h;
  float* tape_gates; float* tape_c;
  const void* dh_out; int32_t ld_dh;
  void* dgates; int32_t ld_dg;
  int32_t T, B, hidden, ndir, act_f32;
  void* stream;
  const int32_t* lengths;
} mmdeer_lstm_seq_len_args;
int mmdeer_lstm_seq_len_fwd(const mmdeer_lstm_seq_len_args* a);
int mmdeer_lstm_seq_len_bwd(const mmdeer_lstm_seq_len_args* a);

typedef struct mmdeer_temporal_pool_len_args {
  const void* h; int32_t ld_h;
  const void* z; int32_t ld_z;
  const float* w2; const float* b2;
  void* attended; int32_t ld_att;
  float* weights;
  const void* dout; int32_t ld_dout;
  void* dh; int32_t ld_dh;
  void* dz; int32_t ld_dz;
  float* dw2; float* db2; float* scratch;
  int32_t T, B, hidden, act_f32;
  void* stream;
  const int32_t* lengths;
} mmdeer_temporal_pool_len_args;
int mmdeer_temporal_pool_len_fwd(const mmdeer_temporal_pool_len_args* a);
int mmdeer_temporal_pool_len_bwd(const mmdeer_temporal_pool_len_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_SEQLEN_H_ */
