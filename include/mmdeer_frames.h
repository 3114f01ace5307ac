/* mmdeer -- C ABI of the frame video encoder's operators (csrc/conv2d.hip, csrc/bn2d.hip on csrc/bn_rows.h): the forward of the Conv2d
 * backbone that turns frames into per-frame features.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives the ctypes binding),
 * exported by the same library and covered by the same MMDEER_ABI_VERSION.  The conventions are mmdeer.h's: every call enqueues on
 * `stream`, never synchronises and allocates nothing; a refused call writes nothing, returns -1 and leaves its reason in
 * mmdeer_last_error(), and every refusal is decided on the host before any HIP runtime call; "act" = fp32 when act_f32 != 0,
 * else bf16.  N = 0 (no frames) writes nothing and returns 0.
 *
 * Layout.  Activations are channels-last: one row of C channels per (n, h, w).  The output of a convolution is the dense matrix
 * [N * OH * OW][Cout].  An activation that FEEDS a convolution of kernel size k (padding p = k / 2, stride 2) lives in a padded
 * buffer [N][Hp = H + 2 p][Wp = W + 2 p][Cp] whose border pixels are zero; the kernel that produces the buffer writes all of it,
 * border included.  Tap row kh of output position (n, oh, ow) is then the KWe * Cp contiguous elements that start at padded pixel
 * (n, 2 oh + kh, 2 ow): the spatial padding is in the buffer, not in the kernel, and the convolution is an implicit GEMM with one
 * K loop per tap row.
 *   k = 3: Cp = Cin (a multiple of the 16-byte chunk: 4 fp32 / 8 bf16 elements), KWe = 3.
 *   k = 7: Cin must be 3 and a pixel is ONE 16-byte chunk, Cp = 4 (fp32) or 8 (bf16), channels 3 .. Cp - 1 zero; KWe = 8, so a
 *          tap row is 128 bytes, a whole K-tile in both dtypes.  The eighth pixel meets zero weights, but it is read: it is the
 *          next pixel of the buffer (border or data: finite), and behind the last pixel of the last frame the buffer carries one
 *          more zero pixel, the slack.  The buffer has N * Hp * Wp + 1 pixels.
 * Every buffer of a call (N * Hp * Wp * Cp, N * OH * OW * Cout) must have fewer than 2^31 elements. */
#ifndef MMDEER_FRAMES_H_
#define MMDEER_FRAMES_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mmdeer_frames_pack: frames fp32 NCHW [N][3][H][W] -> `out`, the padded buffer of the 7 x 7 convolution (p = 3, Cp as above),
 *   act [N * (H + 6) * (W + 6) + 1][Cp]: interior pixels hold (r, g, b, 0 ...), the border and the slack pixel are zero.
 * mmdeer_conv2d_pack: weight fp32 [Cout][Cin][k][k] -> image act [k][Cout][KWe * Cp]:
 *   image[kh][co][kw * Cp + c] = weight[co][c][kh][kw] for kw < k and c < Cin, else 0.
 *   k must be 3 (Cin a multiple of the 16-byte chunk) or 7 (Cin = 3); Cout a multiple of 64.
 * frames / weight must be 4-byte aligned (fp32), out / image 16-byte aligned. */
int mmdeer_frames_pack(const float* frames, int N, int H, int W, void* out, int act_f32, void* stream);
int mmdeer_conv2d_pack(const float* weight, int Cout, int Cin, int k, void* image, int act_f32, void* stream);

/* ---- mmdeer_conv2d_s2: nn.Conv2d(Cin, Cout, k, stride = 2, padding = k / 2) as ONE implicit-GEMM launch.
 *   y[(n * OH + oh) * OW + ow][co] = bias[co] + sum_{kh < k} sum_{e < KWe * Cp} x[((n * Hp + 2 oh + kh) * Wp + 2 ow) * Cp + e] * w[kh][co][e]
 *   with OH = (H + 2 p - k) / 2 + 1 and OW likewise (H, W >= 1 give OH, OW >= 1).
 *   x    act, the padded buffer of an H x W input described above; no element outside it is read into a stored output
 *   w    act [k][Cout][KWe * Cp], mmdeer_conv2d_pack's image
 *   bias fp32 [Cout] or NULL
 *   y    act [N * OH * OW][Cout] dense: written, nothing else is
 *   k    3 or 7 with Cin as for mmdeer_conv2d_pack; Cout a multiple of 64
 *   tile -1 = by tile count, 0 = 64 x 64, 2 = 128 x 128 output tiles (mmdeer_gemm's numbering)
 * x, w, y and bias must be 16-byte aligned. */
typedef struct mmdeer_conv2d_args {
  const void* x;
  const void* w;
  const float* bias;
  void* y;
  int32_t N, H, W, Cin, Cout, k, act_f32, tile;
  void* stream;
} mmdeer_conv2d_args;
int mmdeer_conv2d_s2(const mmdeer_conv2d_args* a);

/* ---- nn.BatchNorm2d(C) + ReLU on the dense act matrix x [M = N * H * W][C] of a convolution's output, C in {64, 128, 256, 512}.
 *
 * mmdeer_bn2d_stats: per-channel mean[C] and rstd[C] = 1 / sqrt(biased variance + eps), fp32, over the M rows of x as stored.
 *   The method is mmdeer_bn_time_stats': Welford row blocks merged by Chan's formula in a fixed order -- deterministic, no
 *   floating-point atomics, no cancellation for a channel with a large offset.  When running_mean is non-NULL the same call updates
 *   running_mean and running_var (both required then; momentum, the variance unbiased by M / (M - 1)) and, when non-NULL, adds 1
 *   to the int64 num_batches_tracked, all on the device.  Needs `scratch`.
 * mmdeer_bn2d_apply: v = relu((x - mean) * rstd * gamma + beta) goes to `out` in one of three forms (dest):
 *   MMDEER_BN2D_PAD   act [N][H + 2][W + 2][C]: v in the interior, an exactly zero border -- the padded buffer of a 3 x 3 convolution
 *   MMDEER_BN2D_POOL  the same buffer of nn.MaxPool2d(3, stride 2, padding 1) of v: act [N][PH + 2][PW + 2][C], PH = (H - 1) / 2 + 1,
 *                     PW likewise
 *   MMDEER_BN2D_AVG   fp32 [N][C]: the mean of v over the H * W positions of each frame (nn.AdaptiveAvgPool2d(1))
 *   running != 0 (evaluation mode): `mean` and `rstd` point at running_mean and running_VAR; rstd is formed per use.
 * x and out must be 16-byte aligned, the fp32 vectors too.  scratch: fp32, at least MMDEER_BN2D_SCRATCH elements. */
#define MMDEER_BN2D_SCRATCH (1024 * 1024)
#define MMDEER_BN2D_PAD 0
#define MMDEER_BN2D_POOL 1
#define MMDEER_BN2D_AVG 2
typedef struct mmdeer_bn2d_args {
  const void* x;
  float* mean; float* rstd;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float momentum, eps;
  const float* gamma; const float* beta;
  void* out;
  int32_t dest, running;
  float* scratch;
  int32_t N, H, W, C, act_f32;
  void* stream;
} mmdeer_bn2d_args;
int mmdeer_bn2d_stats(const mmdeer_bn2d_args* a);
int mmdeer_bn2d_apply(const mmdeer_bn2d_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_FRAMES_H_ */
