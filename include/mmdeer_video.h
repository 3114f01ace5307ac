/* mmdeer -- C ABI of the temporal video encoder's operators (csrc/conv_time.hip, csrc/bn_time.hip on csrc/bn_rows.h): a companion of mmdeer.h,
 * in the same grammar (mmdeer/_header.py derives the ctypes binding of both), exported by the same library and covered by the same
 * MMDEER_ABI_VERSION.  The conventions are mmdeer.h's: every call enqueues on `stream` and never synchronises; a refused call
 * writes nothing, returns -1 and leaves its reason in mmdeer_last_error(), and every refusal is decided on the host before any
 * HIP runtime call; "act" = fp32 when act_f32 != 0, else bf16.
 *
 * Layout.  The encoder's activations are matrices of 512 channels whose rows are time-major: row t * B + b.  One time step is
 * then a shift of B rows for every row at once.  An activation that feeds a convolution lives in a PADDED buffer of
 * (T + 2) * B rows: the first and the last B rows are zero (the caller zeroes them), the T * B rows in between are the interior.
 * The time padding of the convolution is therefore in the buffer, not in the kernel. */
#ifndef MMDEER_VIDEO_H_
#define MMDEER_VIDEO_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- nn.Conv1d(512, 512, kernel_size = 3, padding = 1) over time as ONE implicit GEMM launch per pass.
 * C and N must both be 512; anything else is refused.  B = 0 or T = 0 writes nothing and returns 0.
 *
 * mmdeer_conv3_time_pack: the weight's device images from the fp32 parameter weight [N][C][3]:
 *   image       [3][N][C] act: image[j][n][c]       = weight[n][c][j]       (read by the forward)
 *   image_rev_t [3][C][N] act: image_rev_t[j][c][n] = weight[n][c][2 - j]   (read by the input gradient; NULL: not written)
 *
 * mmdeer_conv3_time: y[r][n] = bias[n] + sum_{j < 3} sum_{c < C} x[r + j * B][c] * w[j][n][c] for r < T * B.
 *   x    act [(T + 2) * B][ld_x >= C], a padded buffer; tap j of output row r reads padded row r + j * B unconditionally, and no
 *        row outside the (T + 2) * B rows of x is read into a stored output
 *   w    act [3][N][C] dense: `image` for the forward.  The input gradient is the same call on the padded dY with `image_rev_t`,
 *        without bias and with N and C swapped (both 512: only the image differs)
 *   bias fp32 [N] or NULL
 *   y    act [T * B][ld_y >= N]: written, nothing else is
 *   tile -1 = by tile count, 0 = 64 x 64, 2 = 128 x 128 output tiles (mmdeer_gemm's numbering)
 * x, w, y and bias must be 16-byte aligned and ld_x, ld_y multiples of 16 bytes.  (T + 2) * B must stay below 2^31 / 512.
 * The weight gradients are three ordinary weight-gradient problems on row-shifted views, dW[:, :, j] = dY^T x[j * B : j * B + T * B]
 * (mmdeer_gemm_batch; the bias gradient comes from the same launch). */
typedef struct mmdeer_conv3_time_args {
  const void* x; int32_t ld_x;
  const void* w;
  const float* bias;
  void* y; int32_t ld_y;
  int32_t T, B, C, N, act_f32, tile;
  void* stream;
} mmdeer_conv3_time_args;
int mmdeer_conv3_time_pack(const float* weight, int N, int C, void* image, void* image_rev_t, int act_f32, void* stream);
int mmdeer_conv3_time(const mmdeer_conv3_time_args* a);

/* ---- nn.BatchNorm1d(512) over the R rows of an act matrix [R][ld >= 512] (C must be 512; R = 0 writes nothing and returns 0).
 * Pointers to act rows must be 16-byte aligned with leading dimensions multiples of 16 bytes; fp32 vectors 16-byte aligned.
 *
 * mmdeer_bn_time_stats: per-channel mean[C] and rstd[C] = 1 / sqrt(biased variance + eps), fp32, of x as stored.  Row blocks
 *   accumulate (count, mean, M2) by Welford's update and are merged by Chan's formula in a fixed order: deterministic, no
 *   floating-point atomics, and no cancellation for a channel with a large offset.  When running_mean is non-NULL the same call
 *   updates running_mean, running_var (both required then; momentum, the variance unbiased by R / (R - 1)) and, when non-NULL,
 *   adds 1 to the int64 num_batches_tracked -- all on the device, so a captured graph keeps updating them.  Needs `scratch`.
 * mmdeer_bn_time_apply: out = drop(relu((x - mean) * rstd * gamma + beta)).  relu != 0 applies the ReLU; drop_site >= 0 with
 *   dropout_p > 0 applies the library's counter-hash dropout of that site at (row, channel) (mmdeer_dropout_mask gives the same
 *   mask; offset_dev is honoured).  `out` act [R][ld_out] may be the interior of a padded buffer.
 * mmdeer_bn_time_bwd: g = dout * (out > 0) * mask_scale (out NULL: g = dout), dbeta = sum_r g, dgamma = sum_r g * xhat by a
 *   deterministic two-stage fold (needs `scratch`); dx = gamma * rstd * (g - dbeta / R - xhat * dgamma / R).
 * running != 0 (evaluation mode) in _apply and _bwd: `mean` and `rstd` point at running_mean and running_VAR; rstd is formed as
 *   1 / sqrt(var + eps) per use and the statistics are constants of the backward: dx = gamma * rstd * g.
 * scratch: fp32, at least MMDEER_BN_TIME_SCRATCH elements. */
#define MMDEER_BN_TIME_SCRATCH (1024 * 1024)
typedef struct mmdeer_bn_time_args {
  const void* x; int32_t ld_x;
  float* mean; float* rstd;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float momentum, eps;
  const float* gamma; const float* beta;
  void* out; int32_t ld_out;
  int32_t relu, drop_site;
  float dropout_p;
  uint64_t seed, offset;
  const uint64_t* offset_dev;
  const void* dout; int32_t ld_dout;
  void* dx; int32_t ld_dx;
  float* dgamma; float* dbeta;
  float mask_scale;
  int32_t running;
  float* scratch;
  int32_t R, C, act_f32;
  void* stream;
} mmdeer_bn_time_args;
int mmdeer_bn_time_stats(const mmdeer_bn_time_args* a);
int mmdeer_bn_time_apply(const mmdeer_bn_time_args* a);
int mmdeer_bn_time_bwd(const mmdeer_bn_time_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_VIDEO_H_ */
