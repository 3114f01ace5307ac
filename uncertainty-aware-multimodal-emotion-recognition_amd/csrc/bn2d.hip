// nn.BatchNorm2d(C) + ReLU of the frame video encoder's backbone (reference src/models/encoders.py:418-440) on the dense channels-last
// output x [M = N * H * W][C] of a convolution, C in {64, 128, 256, 512}, forward only; the statistics are per channel over all M rows.
//
// The lane mapping, the statistics (Welford row blocks merged by Chan's formula in a fixed order) and the normalisation itself are
// bn_rows.h's; this file holds the apply kernels.
//
// Apply: v = relu((x - mean) * rstd * gamma + beta) goes to one of three destinations (include/mmdeer_frames.h).  The two padded
// ones run one thread-quad per pixel of the OUTPUT buffer, border pixels included, so the buffer's zero border needs no launch
// of its own.  The max pool starts its running maximum at 0 instead of padding with -inf: after the ReLU every value is >= 0, and
// every 3 x 3 window holds at least one real element (its centre (2 ph, 2 pw) is inside the image), so the two agree.
#include "bn_rows.h"

namespace mmdeer {
namespace {

// PAD and POOL: OH x OW is the interior of the output buffer (H x W, or the pooled size); Q = N (OH + 2) (OW + 2) output pixels
template <bool F32, bool POOL>
__global__ __launch_bounds__(256) void bn2d_apply_padded_kernel(mmdeer_bn2d_args a, int OH, int OW, long long Q, int ppb) {
  const Lane l = lane_of(a.C);
  Norm norm;
  norm.load(a, l.cq);
  const int C = a.C, H = a.H, W = a.W, OWp = OW + 2, OHp = OH + 2;
  auto row = [&](long long r) __attribute__((always_inline)) { return ld4<F32>(a.x, r * C + 4 * l.cq); };
  const long long q0 = (long long)blockIdx.x * ppb, q1 = min(q0 + ppb, Q);
  for (long long q = q0 + l.par; q < q1; q += l.PAR) {
    const int wp = (int)(q % OWp), hp = (int)((q / OWp) % OHp);
    const long long n = q / ((long long)OWp * OHp);
    f32x4 v{0.f, 0.f, 0.f, 0.f};
    if (hp >= 1 && hp <= OH && wp >= 1 && wp <= OW) {
      const int oh = hp - 1, ow = wp - 1;
      if constexpr (!POOL) {
        v = norm(row((n * H + oh) * W + ow));
      } else {   // the running maximum starts at 0: see the head of this file
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          int h;
          if (!pool_tap(i, oh, H, h)) continue;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            int w;
            if (!pool_tap(j, ow, W, w)) continue;
            const f32x4 t = norm(row((n * H + h) * W + w));
            v = f32x4{fmaxf(v.x, t.x), fmaxf(v.y, t.y), fmaxf(v.z, t.z), fmaxf(v.w, t.w)};
          }
        }
      }
    }
    st4<F32>(a.out, q * C + 4 * l.cq, v);
  }
}

// the two as kernels of one parameter, MMDEER_LAUNCH_ACT's form
template <bool F32>
constexpr auto bn2d_apply_pad_kernel = bn2d_apply_padded_kernel<F32, false>;
template <bool F32>
constexpr auto bn2d_apply_pool_kernel = bn2d_apply_padded_kernel<F32, true>;

// AVG: one workgroup per frame; each thread's rows by a compensated sum, the PAR partial sums of a channel in index order out of LDS
template <bool F32>
__global__ __launch_bounds__(256) void bn2d_apply_avg_kernel(mmdeer_bn2d_args a) {
  __shared__ f32x4 ss[256];
  const Lane l = lane_of(a.C);
  Norm norm;
  norm.load(a, l.cq);
  const int C = a.C, CQ = C >> 2, HW = a.H * a.W;
  const long long base = (long long)blockIdx.x * HW;
  // compensated (Kahan) sum: bf16 activations take few distinct values, and adding equal terms to a growing fp32 sum rounds the same way
  // every time -- the plain sum drifted by 4e-5 of the result over 16500 terms
  f32x4 s{0.f, 0.f, 0.f, 0.f}, comp{0.f, 0.f, 0.f, 0.f};
  for (int r = l.par; r < HW; r += l.PAR) {
    const f32x4 v = norm(ld4<F32>(a.x, (base + r) * C + 4 * l.cq)) - comp, t = s + v;
    comp = (t - s) - v;
    s = t;
  }
  ss[threadIdx.x] = s;
  __syncthreads();
  if (l.par != 0) return;
  for (int q = 1; q < l.PAR; ++q) s += ss[q * CQ + l.cq];
  *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.out) + (long long)blockIdx.x * C + 4 * l.cq) = s * (1.f / (float)HW);
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn2d_stats(const mmdeer_bn2d_args* a) {
  TRY(bn_check_nhwc(a, "bn2d_stats", "x"));
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->x && al16(a->x), "bn2d_stats: x must be non-NULL and 16-byte aligned");
  return bn_launch_stats(a, "bn2d_stats", a->x, a->C, a->N * a->H * a->W);
}

int mmdeer_bn2d_apply(const mmdeer_bn2d_args* a) {
  TRY(bn_check_nhwc(a, "bn2d_apply", "x"));
  MMDEER_CHECK(a->dest == MMDEER_BN2D_PAD || a->dest == MMDEER_BN2D_POOL || a->dest == MMDEER_BN2D_AVG, "bn2d_apply: dest must be 0, 1 or 2 (got %d)", a->dest);
  const bool pool = a->dest == MMDEER_BN2D_POOL;
  const int OH = pool ? (a->H - 1) / 2 + 1 : a->H, OW = pool ? (a->W - 1) / 2 + 1 : a->W;
  const long long Q = (long long)a->N * (OH + 2) * (OW + 2);
  MMDEER_CHECK(a->dest == MMDEER_BN2D_AVG || Q * a->C < LIMIT, "bn2d_apply: out has 2^31 elements or more");
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->x && a->out && al16(a->x) && al16(a->out), "bn2d_apply: x and out must be non-NULL and 16-byte aligned");
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->beta && al16(a->mean) && al16(a->rstd) && al16(a->gamma) && al16(a->beta),
               "bn2d_apply: mean, rstd, gamma, beta must be non-NULL and 16-byte aligned");
  hipStream_t s = (hipStream_t)a->stream;
  if (a->dest == MMDEER_BN2D_AVG) {
    MMDEER_LAUNCH_ACT(bn2d_apply_avg_kernel, a->act_f32, dim3(a->N), dim3(256), s, *a);
    return 0;
  }
  const PixelPlan p = bn_pixel_plan(Q);
  if (pool) MMDEER_LAUNCH_ACT(bn2d_apply_pool_kernel, a->act_f32, dim3(p.nblk), dim3(256), s, *a, OH, OW, Q, p.ppb);
  else MMDEER_LAUNCH_ACT(bn2d_apply_pad_kernel, a->act_f32, dim3(p.nblk), dim3(256), s, *a, OH, OW, Q, p.ppb);
  return 0;
}

}  // extern "C"
