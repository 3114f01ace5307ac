/* mmdeer -- C ABI of the frame video encoder's BACKWARD operators (csrc/bn2d_bwd.hip on csrc/bn_rows.h, csrc/conv2d_bwd.hip): the
 * gradients of the Conv2d backbone whose forward is include/mmdeer_frames.h.  A companion of mmdeer.h in the same grammar (mmdeer/_header.py derives
 * the ctypes binding), exported by the same library and covered by the same MMDEER_ABI_VERSION.  The conventions are mmdeer.h's:
 * every call enqueues on `stream`, never synchronises and allocates nothing; a refused call writes nothing, returns -1 and leaves its
 * reason in mmdeer_last_error(), and every refusal is decided on the host before any HIP runtime call; "act" = fp32 when
 * act_f32 != 0, else bf16.  N = 0 (no frames) writes nothing and returns 0.  Every buffer of a call must have fewer than 2^31
 * elements, and every pointer must be 16-byte aligned.  No floating-point atomics: every reduction has a fixed order, so two runs
 * of a call on the same operands store the same bits.
 *
 * The layouts are mmdeer_frames.h's: channels-last rows, the dense output [N * OH * OW][Cout] of a convolution, the padded buffer
 * [N][Hp][Wp][Cp] (+ slack) that feeds one.  One backward layer is mmdeer_bn2d_bwd (the gradient at the convolution's output from
 * the gradient at the layer's output), mmdeer_conv2d_wgrad (weight and bias gradient) and, where the layer's input has a gradient,
 * mmdeer_conv2d_dgrad (the gradient of the interior of its padded input buffer, which is the DENSE or POOL source of the layer
 * before). */
#ifndef MMDEER_FRAMES_BWD_H_
#define MMDEER_FRAMES_BWD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mmdeer_bn2d_bwd: the backward of mmdeer_bn2d_stats + mmdeer_bn2d_apply on y [M = N * H * W][C], C in {64, 128, 256, 512}.
 *   With xhat = (y - mean) * rstd and v = relu(xhat * gamma + beta) -- the forward's own expression, so the ReLU mask and the
 *   pool's arg-max are the forward's bit for bit -- and u the gradient that reaches v through the forward's destination:
 *     g = u * (v > 0),  dbeta[c] = sum_m g,  dgamma[c] = sum_m g * xhat  (per-block partials, then a fold, both in a fixed order)
 *     running == 0:  dy = gamma * rstd * (g - dbeta / M - xhat * dgamma / M)
 *     running != 0:  dy = gamma * rstd * g; `mean` and `rstd` point at running_mean and running_VAR, as in mmdeer_bn2d_apply
 *   `dout` holds u in one of three source forms (src), the mirrors of the forward's three destinations:
 *     MMDEER_BN2D_SRC_DENSE  act [M][C]: the gradient of the interior of the next convolution's padded buffer (mmdeer_conv2d_dgrad's dx)
 *     MMDEER_BN2D_SRC_POOL   act [N * PH * PW][C], PH = (H - 1) / 2 + 1, PW likewise: the gradient of the interior of the pooled
 *                            buffer.  Position (h, w) receives the sum over the at most four 3 x 3 stride-2 windows that contain
 *                            it and whose maximum it is; ties go to the FIRST maximum in (kh, kw) row-major order among the
 *                            in-image positions (torch's rule).  A gather: a first launch writes one index byte per pooled
 *                            element into `pool_idx` (N * PH * PW * C bytes, required for this source), and every position then
 *                            reads at most four of them.
 *     MMDEER_BN2D_SRC_AVG    fp32 [N][C], the gradient of the frame means: every position of frame n receives dout[n][c] / (H * W)
 *   y        act [M][C], the convolution's output as stored
 *   dy       act [M][C] dense: written whole, nothing else is (a caller may keep further rows behind it)
 *   dgamma, dbeta  fp32 [C], written
 *   scratch  fp32, at least MMDEER_BN2D_BWD_SCRATCH elements */
#define MMDEER_BN2D_BWD_SCRATCH (1024 * 1024)
#define MMDEER_BN2D_SRC_DENSE 0
#define MMDEER_BN2D_SRC_POOL 1
#define MMDEER_BN2D_SRC_AVG 2
typedef struct mmdeer_bn2d_bwd_args {
  const void* y;
  const float* mean; const float* rstd;
  const float* gamma; const float* beta;
  const void* dout;
  void* dy;
  float* dgamma; float* dbeta;
  float* scratch;
  void* pool_idx;
  float eps;
  int32_t src, running;
  int32_t N, H, W, C, act_f32;
  void* stream;
} mmdeer_bn2d_bwd_args;
int mmdeer_bn2d_bwd(const mmdeer_bn2d_bwd_args* a);

/* ---- mmdeer_conv2d_wgrad: the weight (and bias) gradient of mmdeer_conv2d_s2, one MFMA launch and a fold launch.
 *   dw[co][c][kh][kw] = sum_{m < M} dy[m][co] * x[origin(m) + (kh * Wp + kw) * Cp + c],  M = N * OH * OW,
 *   dbias[co] = sum_m dy[m][co], with origin(m) = ((n * Hp + 2 oh) * Wp + 2 ow) * Cp the forward's origin of output row m: an implicit
 *   GEMM per tap row kh whose reduction rows are gathered out of the padded buffer; no im2col buffer exists.  The reduction is cut
 *   into `slices` ranges of whole K-tiles (32 rows in fp32, 64 in bf16), one workgroup per (output tile, slice); each writes its
 *   fp32 partial to `scratch`, and the fold launch adds the slices in index order and writes the parameter's layout, dropping the
 *   image's padding lanes (kw >= k, c >= Cin).
 *   x       act, the forward's padded input buffer (k, Cin, Cp, KWe and the slack as for mmdeer_conv2d_s2)
 *   dy      act [M][Cout]
 *   dw      fp32 [Cout][Cin][k][k], written (not accumulated)
 *   dbias   fp32 [Cout], written, or NULL
 *   slices  -1 = chosen from the tile count (enough workgroups for 256 CUs), else 1 .. MMDEER_CONV2D_WGRAD_MAX_SLICES as given
 *   scratch fp32, scratch_elems >= mmdeer_conv2d_wgrad_scratch(a) elements
 * mmdeer_conv2d_wgrad_scratch: the scratch elements the call needs (pointers are not looked at), or -1 for a refused shape. */
#define MMDEER_CONV2D_WGRAD_MAX_SLICES 256
typedef struct mmdeer_conv2d_wgrad_args {
  const void* x;
  const void* dy;
  float* dw;
  float* dbias;
  float* scratch;
  long long scratch_elems;
  int32_t N, H, W, Cin, Cout, k, act_f32, slices;
  void* stream;
} mmdeer_conv2d_wgrad_args;
long long mmdeer_conv2d_wgrad_scratch(const mmdeer_conv2d_wgrad_args* a);
int mmdeer_conv2d_wgrad(const mmdeer_conv2d_wgrad_args* a);

/* ---- mmdeer_conv2d_pack_t: weight fp32 [Cout][Cin][3][3] -> image act [3][3][Cin][Cout]: image[kh][kw][c][co] = weight[co][c][kh][kw].
 * mmdeer_conv2d_dgrad: the input gradient of a 3 x 3 mmdeer_conv2d_s2 (k = 7, the first layer, has none: refused).
 *   dx[(n * H + h) * W + w][c] = sum_{kh, kw} sum_co dy[(n * OH + (h + 1 - kh) / 2) * OW + (w + 1 - kw) / 2][co] * wt[kh][kw][c][co]
 *   over the taps with (h + 1 - kh) and (w + 1 - kw) even and the quotients inside [0, OH) x [0, OW).  Only these products are
 *   formed: the positions fall into four parity classes of (h, w) with 4 / 2 / 2 / 1 taps, each class an implicit GEMM with
 *   K = Cout per tap on the forward's gathered tile body, all four in one launch (the class is a tile coordinate).
 *   dy   act [M + 1][Cout], M = N * OH * OW: row M must be ZERO -- a tap whose quotient falls outside the image reads it
 *   wt   act [3][3][Cin][Cout], mmdeer_conv2d_pack_t's image
 *   dx   act [N * H * W][Cin] dense, written whole: the gradient of the interior of the padded input buffer
 *   Cin a multiple of the 16-byte chunk (4 fp32 / 8 bf16 elements), Cout a multiple of 64 */
int mmdeer_conv2d_pack_t(const float* weight, int Cout, int Cin, int k, void* image, int act_f32, void* stream);
typedef struct mmdeer_conv2d_dgrad_args {
  const void* dy;
  const void* wt;
  void* dx;
  int32_t N, H, W, Cin, Cout, k, act_f32;
  void* stream;
} mmdeer_conv2d_dgrad_args;
int mmdeer_conv2d_dgrad(const mmdeer_conv2d_dgrad_args* a);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_FRAMES_BWD_H_ */
