// The backward of nn.BatchNorm2d(C) + ReLU (+ MaxPool2d(3, 2, 1) / AdaptiveAvgPool2d(1)) of the frame video encoder's backbone on the
// dense channels-last output y [M = N * H * W][C] of a convolution (include/mmdeer_frames_bwd.h), C in {64, 128, 256, 512}.
//
// Launches.  POOL source only: one index byte per pooled element (the first maximum of its window in (kh, kw) row-major order among
// the in-image positions).  Then, for every source, bn_rows.h's backward -- partial sums, fold, dy -- with this file's gradient
// functor.  g is formed twice, by one function: the upstream gradient is gathered, never scattered, so there is no atomic and no
// ordering to fix.  The ReLU mask and the pool's arg-max come from Norm, the expression the forward stored its output from.
#include "bn_rows.h"

namespace mmdeer {
namespace {

// the backward's gradient functor (bn_rows.h): g = u * (v > 0) and xhat of this thread's four channels of row r
template <bool F32, int SRC>
struct Grad {
  using Args = mmdeer_bn2d_bwd_args;
  Norm norm;
  void* dy;
  int C, cq, H, W, PH, PW;
  float inv_hw;
  const void* y;
  const void* dout;
  const unsigned char* idx;

  __device__ __forceinline__ void init(const mmdeer_bn2d_bwd_args& a, int cq_) {
    norm.load(a, cq_);
    C = a.C; cq = cq_; H = a.H; W = a.W;
    PH = (H - 1) / 2 + 1; PW = (W - 1) / 2 + 1;
    inv_hw = 1.f / (float)(H * W);
    y = a.y; dout = a.dout; dy = a.dy; idx = reinterpret_cast<const unsigned char*>(a.pool_idx);
  }
  __device__ __forceinline__ f32x4 scale() const { return norm.gamma * norm.rstd; }
  __device__ __forceinline__ void store(int r, const f32x4& d) const { st4<F32>(dy, (long long)r * C + 4 * cq, d); }
  // the pooled element (n, ph, pw) gives its gradient to window position `at` (= 3 i + j) only
  __device__ __forceinline__ void take(f32x4& u, long long q, unsigned at) const {
    const unsigned w = *reinterpret_cast<const unsigned*>(idx + q * C + 4 * cq);
    const f32x4 d = ld4<F32>(dout, q * C + 4 * cq);
    if ((w & 0xFFu) == at) u.x += d.x;
    if (((w >> 8) & 0xFFu) == at) u.y += d.y;
    if (((w >> 16) & 0xFFu) == at) u.z += d.z;
    if ((w >> 24) == at) u.w += d.w;
  }
  __device__ __forceinline__ f32x4 operator()(int r, f32x4& xh) const {
    const f32x4 x = ld4<F32>(y, (long long)r * C + 4 * cq);
    xh = norm.xhat(x);
    const f32x4 v = norm(x);
    f32x4 u{0.f, 0.f, 0.f, 0.f};
    if constexpr (SRC == MMDEER_BN2D_SRC_DENSE) {
      u = ld4<F32>(dout, (long long)r * C + 4 * cq);
    } else if constexpr (SRC == MMDEER_BN2D_SRC_AVG) {
      const int n = r / (H * W);
      u = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(dout) + (long long)n * C + 4 * cq) * inv_hw;
    } else {
      const int n = r / (H * W), rem = r - n * (H * W), h = rem / W, w = rem - h * W;
      // the windows ph with 2 ph - 1 <= h <= 2 ph + 1: one for an even h (window row 1), two for an odd one (rows 2 and 0)
      const int ph0 = h >> 1, i0 = (h & 1) ? 2 : 1, pw0 = w >> 1, j0 = (w & 1) ? 2 : 1;
      const bool ph1 = (h & 1) && ph0 + 1 < PH, pw1 = (w & 1) && pw0 + 1 < PW;
      const long long q00 = ((long long)n * PH + ph0) * PW + pw0;
      take(u, q00, 3 * i0 + j0);
      if (pw1) take(u, q00 + 1, 3 * i0);
      if (ph1) {
        take(u, q00 + PW, j0);
        if (pw1) take(u, q00 + PW + 1, 0);
      }
    }
    return f32x4{v.x > 0.f ? u.x : 0.f, v.y > 0.f ? u.y : 0.f, v.z > 0.f ? u.z : 0.f, v.w > 0.f ? u.w : 0.f};
  }
};

// one thread-quad per pooled element: the window position (3 i + j) of its first maximum, one byte per channel
template <bool F32>
__global__ __launch_bounds__(256) void bn2d_pool_index_kernel(mmdeer_bn2d_bwd_args a, int PH, int PW, long long Q, int ppb) {
  const Lane l = lane_of(a.C);
  Norm norm;
  norm.load(a, l.cq);
  const int C = a.C, H = a.H, W = a.W;
  unsigned char* idx = reinterpret_cast<unsigned char*>(a.pool_idx);
  const long long q0 = (long long)blockIdx.x * ppb, q1 = min(q0 + ppb, Q);
  for (long long q = q0 + l.par; q < q1; q += l.PAR) {
    const int pw = (int)(q % PW), ph = (int)((q / PW) % PH);
    const long long n = q / ((long long)PW * PH);
    f32x4 best{-1.f, -1.f, -1.f, -1.f};   // every value is >= 0: the first in-image position is always taken
    unsigned at0 = 0, at1 = 0, at2 = 0, at3 = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      int h;
      if (!pool_tap(i, ph, H, h)) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        int w;
        if (!pool_tap(j, pw, W, w)) continue;
        const f32x4 t = norm(ld4<F32>(a.y, ((n * H + h) * W + w) * C + 4 * l.cq));
        const unsigned at = 3 * i + j;
        if (t.x > best.x) { best.x = t.x; at0 = at; }
        if (t.y > best.y) { best.y = t.y; at1 = at; }
        if (t.z > best.z) { best.z = t.z; at2 = at; }
        if (t.w > best.w) { best.w = t.w; at3 = at; }
      }
    }
    *reinterpret_cast<unsigned*>(idx + q * C + 4 * l.cq) = at0 | (at1 << 8) | (at2 << 16) | (at3 << 24);
  }
}

template <bool F32>
int launch_bn2d_bwd_src(const mmdeer_bn2d_bwd_args& a, int M) {
  if (a.src == MMDEER_BN2D_SRC_DENSE) return bn_launch_bwd<Grad<F32, MMDEER_BN2D_SRC_DENSE>, 1>(a, M);
  if (a.src == MMDEER_BN2D_SRC_AVG) return bn_launch_bwd<Grad<F32, MMDEER_BN2D_SRC_AVG>, 1>(a, M);
  const int PH = (a.H - 1) / 2 + 1, PW = (a.W - 1) / 2 + 1;
  const long long Q = (long long)a.N * PH * PW;
  const PixelPlan p = bn_pixel_plan(Q);
  hipLaunchKernelGGL((bn2d_pool_index_kernel<F32>), dim3(p.nblk), dim3(256), 0, (hipStream_t)a.stream, a, PH, PW, Q, p.ppb);
  return bn_launch_bwd<Grad<F32, MMDEER_BN2D_SRC_POOL>, 1>(a, M);
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn2d_bwd(const mmdeer_bn2d_bwd_args* a) {
  TRY(bn_check_nhwc(a, "bn2d_bwd", "y"));
  MMDEER_CHECK(a->src == MMDEER_BN2D_SRC_DENSE || a->src == MMDEER_BN2D_SRC_POOL || a->src == MMDEER_BN2D_SRC_AVG,
               "bn2d_bwd: src must be 0, 1 or 2 (got %d)", a->src);
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->y && a->dout && a->dy, "bn2d_bwd: NULL pointer (y, dout, dy)");
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->beta && a->dgamma && a->dbeta && a->scratch,
               "bn2d_bwd: NULL pointer (mean, rstd, gamma, beta, dgamma, dbeta, scratch)");
  MMDEER_CHECK(a->src != MMDEER_BN2D_SRC_POOL || a->pool_idx, "bn2d_bwd: NULL pointer (pool_idx is required for the POOL source)");
  MMDEER_CHECK(al16(a->y) && al16(a->dout) && al16(a->dy) && al16(a->mean) && al16(a->rstd) && al16(a->gamma) && al16(a->beta) &&
                   al16(a->dgamma) && al16(a->dbeta) && al16(a->scratch) && al16(a->pool_idx),
               "bn2d_bwd: misaligned pointer (every pointer needs 16 bytes)");
  const int M = a->N * a->H * a->W;
  return a->act_f32 ? launch_bn2d_bwd_src<true>(*a, M) : launch_bn2d_bwd_src<false>(*a, M);
}

}  // extern "C"
