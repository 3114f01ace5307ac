// nn.BatchNorm2d(C) + ReLU of the frame video encoder's backbone (reference src/models/encoders.py:418-440) on the dense channels-last
// output x [M = N * H * W][C] of a convolution, C in {64, 128, 256, 512}, forward only; the statistics are per channel over all M rows.
//
// Lane mapping (all kernels): thread t owns the four consecutive channels 4 * (t % (C / 4)) .. + 3 (one 16-byte fp32 / 8-byte bf16
// access per row) of every PAR-th row of its workgroup's share, PAR = 256 / (C / 4) = 2 .. 16 rows in flight per workgroup.
//
// Statistics: bn_time.hip's method (bn_fold.h holds the shared code).  Each thread runs Welford's update over its rows, the PAR
// partials of a workgroup are merged by Chan's formula through LDS in index order, and the per-block (mean, M2) -- the count
// follows from the block index -- go to scratch; a second launch merges the blocks per channel, writes mean and rstd and updates
// the running buffers.  Fixed order, no atomics: deterministic, and no cancellation for a channel with a large offset.
//
// Apply: v = relu((x - mean) * rstd * gamma + beta) goes to one of three destinations (include/mmdeer_frames.h).  The two padded
// ones run one thread-quad per pixel of the OUTPUT buffer, border pixels included, so the buffer's zero border needs no launch
// of its own.  The max pool starts its running maximum at 0 instead of padding with -inf: after the ReLU every value is >= 0, and
// every 3 x 3 window holds at least one real element (its centre (2 ph, 2 pw) is inside the image), so the two agree.
#include "../../include/mmdeer_frames.h"
#include "bn2d_norm.h"   // Lane, Norm (shared with bn2d_bwd.hip); bn_fold.h

namespace mmdeer {
namespace {

static_assert(BN_MAXBLK * 2 * 512 == MMDEER_BN2D_SCRATCH, "scratch holds two per-channel partials per row block");

template <bool F32>
__global__ __launch_bounds__(256) void bn2d_stats_partial_kernel(mmdeer_bn2d_args a, int M, int rpb) {
  __shared__ f32x4 sm[256], sM2[256];
  __shared__ float sn[16];
  const Lane l = lane_of(a.C);
  const int CQ = a.C >> 2, r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  f32x4 mean{0.f, 0.f, 0.f, 0.f}, M2{0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  auto update = [&](const f32x4& x) __attribute__((always_inline)) {
    n += 1.f;
    const float inv = 1.f / n;
    const f32x4 d = x - mean;
    mean += d * inv;
    M2 += d * (x - mean);
  };
  auto row = [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.C + 4 * l.cq); };
  int r = r0 + l.par;
  for (; r + 3 * l.PAR < r1; r += 4 * l.PAR) {
    const f32x4 x0 = row(r), x1 = row(r + l.PAR), x2 = row(r + 2 * l.PAR), x3 = row(r + 3 * l.PAR);
    update(x0); update(x1); update(x2); update(x3);
  }
  for (; r < r1; r += l.PAR) update(row(r));
  sm[threadIdx.x] = mean; sM2[threadIdx.x] = M2;
  if (l.cq == 0) sn[l.par] = n;
  __syncthreads();
  if (l.par != 0) return;
  for (int q = 1; q < l.PAR; ++q) {
    chan_merge(n, mean, M2, sn[q], sm[q * CQ + l.cq], sM2[q * CQ + l.cq]);
    n += sn[q];
  }
  float* part = a.scratch + (long long)blockIdx.x * 2 * a.C;
  *reinterpret_cast<f32x4*>(part + 4 * l.cq) = mean;
  *reinterpret_cast<f32x4*>(part + a.C + 4 * l.cq) = M2;
}

__global__ __launch_bounds__(256) void bn2d_stats_final_kernel(mmdeer_bn2d_args a, int M, int rpb, int nblk) {
  bn_fold_stats(a, M, a.C, rpb, nblk);
}

// PAD and POOL: OH x OW is the interior of the output buffer (H x W, or the pooled size); Q = N (OH + 2) (OW + 2) output pixels
template <bool F32, bool POOL>
__global__ __launch_bounds__(256) void bn2d_apply_pad_kernel(mmdeer_bn2d_args a, int OH, int OW, long long Q, int ppb) {
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
          const int h = 2 * oh - 1 + i;
          if (h < 0 || h >= H) continue;
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const int w = 2 * ow - 1 + j;
            if (w < 0 || w >= W) continue;
            const f32x4 t = norm(row((n * H + h) * W + w));
            v = f32x4{fmaxf(v.x, t.x), fmaxf(v.y, t.y), fmaxf(v.z, t.z), fmaxf(v.w, t.w)};
          }
        }
      }
    }
    st4<F32>(a.out, q * C + 4 * l.cq, v);
  }
}

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

constexpr long long LIMIT = 1ll << 31;   // elements of one buffer

int check_bn2d(const mmdeer_bn2d_args* a, const char* op) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->C == 64 || a->C == 128 || a->C == 256 || a->C == 512, "%s: unsupported C=%d (64, 128, 256 or 512)", op, a->C);
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "%s: bad shape N=%d H=%d W=%d", op, a->N, a->H, a->W);
  MMDEER_CHECK((long long)a->N * a->H * a->W * a->C < LIMIT, "%s: x has 2^31 elements or more", op);
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn2d_stats(const mmdeer_bn2d_args* a) {
  TRY(check_bn2d(a, "bn2d_stats"));
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->x && al16(a->x), "bn2d_stats: x must be non-NULL and 16-byte aligned");
  MMDEER_CHECK(a->mean && a->rstd && a->scratch && al16(a->scratch), "bn2d_stats: NULL pointer (mean, rstd, scratch) or misaligned scratch");
  MMDEER_CHECK(!a->running_mean == !a->running_var, "bn2d_stats: running_mean and running_var go together");
  MMDEER_CHECK(a->running_mean || !a->num_batches_tracked, "bn2d_stats: num_batches_tracked needs the running buffers");
  const int M = a->N * a->H * a->W, rpb = bn_rows_per_block(M), nblk = bn_blocks(M);
  hipStream_t s = (hipStream_t)a->stream;
  MMDEER_LAUNCH_ACT(bn2d_stats_partial_kernel, a->act_f32, dim3(nblk), dim3(256), s, *a, M, rpb);
  hipLaunchKernelGGL(bn2d_stats_final_kernel, dim3(a->C / BN_FOLD_CH), dim3(256), 0, s, *a, M, rpb, nblk);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_bn2d_apply(const mmdeer_bn2d_args* a) {
  TRY(check_bn2d(a, "bn2d_apply"));
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
  // pixels per workgroup: at least 32, and at most BN_MAXBLK workgroups
  long long ppb = (Q + BN_MAXBLK - 1) / BN_MAXBLK;
  if (ppb < 32) ppb = 32;
  const dim3 grid((unsigned)((Q + ppb - 1) / ppb));
  if (pool) {
    if (a->act_f32) hipLaunchKernelGGL((bn2d_apply_pad_kernel<true, true>), grid, dim3(256), 0, s, *a, OH, OW, Q, (int)ppb);
    else hipLaunchKernelGGL((bn2d_apply_pad_kernel<false, true>), grid, dim3(256), 0, s, *a, OH, OW, Q, (int)ppb);
  } else {
    if (a->act_f32) hipLaunchKernelGGL((bn2d_apply_pad_kernel<true, false>), grid, dim3(256), 0, s, *a, OH, OW, Q, (int)ppb);
    else hipLaunchKernelGGL((bn2d_apply_pad_kernel<false, false>), grid, dim3(256), 0, s, *a, OH, OW, Q, (int)ppb);
  }
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
