// BatchNorm over the rows of a channels-last activation matrix x [M][ld >= C], C in {64, 128, 256, 512}: everything that is not specific
// to one operator.  bn_time.hip (BatchNorm1d on [R][512], the temporal CNN) and bn2d.hip / bn2d_bwd.hip (BatchNorm2d on the dense
// output [N * H * W][C] of a convolution, the frame backbone) are this code with their own apply kernels and gradient functors.
//
// Lane mapping (all kernels): a workgroup of 256 threads owns a block of consecutive rows; thread t owns the four consecutive channels
// 4 * (t % (C / 4)) .. + 3 (one 16-byte fp32 / 8-byte bf16 access per row) of every PAR-th row of the block, PAR = 256 / (C / 4) =
// 2 .. 16 rows in flight per workgroup.  At C = 512 a wave reads 1 KiB (fp32) of one row per instruction.  The row block is 32 rows,
// or longer so that at most BN_MAXBLK workgroups run: their per-channel partials fit the fixed scratch.
// Row loop (bn_rows): a thread's rows in index order.  With BATCH = 4 the loads of four rows are issued before the first is used --
// the stores of `out` / `dx` may alias the loads as far as the compiler knows, so it would not hoist them itself.
// Folds of the per-block partials: a workgroup owns BN_FOLD_CH channels, its 256 threads are BN_FOLD_SEG segments of consecutive blocks
// x BN_FOLD_CH channels; each thread folds its segment in index order, then the threads of segment 0 fold the segment results in
// index order out of LDS.  The order is a function of M alone: deterministic.  (One thread per channel over all blocks took 68 us at
// 256 blocks: a chain of dependent 300 ns steps on two workgroups.)
//
// Statistics: each thread runs Welford's update over its rows (one reciprocal per row, shared by its four channels), the PAR partials
// of a workgroup are merged by Chan's formula through LDS in index order, and the per-block (mean, M2) -- the count follows from
// the block index -- go to scratch.  A second launch merges the blocks per channel, again by Chan's formula, writes mean and
// rstd and updates the running buffers.  Fixed order, no atomics: deterministic.  A plain (sum x, sum x^2) loses
// every digit of the variance of a channel whose mean is large against its spread; this form does not.
// Backward: the same block structure for the partial sums of g and g * xhat, a fold launch, then dx = k (g - mb - xhat mg).  What g
// is belongs to the operator: a gradient functor (below) forms it, once in each of the two row passes.
#pragma once
#include "../../include/mmdeer_frames_bwd.h"
#include "../../include/mmdeer_frames.h"
#include "../../include/mmdeer_video.h"
#include "elem.h"

namespace mmdeer {
namespace {

constexpr int BN_MAXBLK = 1024;    // row blocks at most; scratch = BN_MAXBLK * 2 * C floats
constexpr int BN_FOLD_CH = 8, BN_FOLD_SEG = 32;   // fold kernels: channels per workgroup, block segments per channel
constexpr long long LIMIT = 1ll << 31;   // elements of one buffer
static_assert(BN_MAXBLK * 2 * 512 == MMDEER_BN_TIME_SCRATCH && MMDEER_BN2D_SCRATCH == MMDEER_BN_TIME_SCRATCH &&
                  MMDEER_BN2D_BWD_SCRATCH == MMDEER_BN_TIME_SCRATCH, "scratch holds two per-channel partials per row block");

// rows per block: at least 32, even, and at most BN_MAXBLK blocks
struct RowPlan {
  int rpb, nblk;
};
inline RowPlan bn_row_plan(int M) {
  int rpb = (M + BN_MAXBLK - 1) / BN_MAXBLK;
  if (rpb < 32) rpb = 32;
  rpb = (rpb + 1) & ~1;
  return RowPlan{rpb, (M + rpb - 1) / rpb};
}
// pixels per block of the kernels that run one thread-quad per output pixel: at least 32, and at most BN_MAXBLK blocks
struct PixelPlan {
  int ppb;
  unsigned nblk;
};
inline PixelPlan bn_pixel_plan(long long Q) {
  long long ppb = (Q + BN_MAXBLK - 1) / BN_MAXBLK;
  if (ppb < 32) ppb = 32;
  return PixelPlan{(int)ppb, (unsigned)((Q + ppb - 1) / ppb)};
}

// the checks of an operator on [N * H * W][C]; `what` names its input in the message
template <typename A>
int bn_check_nhwc(const A* a, const char* op, const char* what) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->C == 64 || a->C == 128 || a->C == 256 || a->C == 512, "%s: unsupported C=%d (64, 128, 256 or 512)", op, a->C);
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "%s: bad shape N=%d H=%d W=%d", op, a->N, a->H, a->W);
  MMDEER_CHECK((long long)a->N * a->H * a->W * a->C < LIMIT, "%s: %s has 2^31 elements or more", op, what);
  return 0;
}

struct Lane {
  int cq, par, PAR;
};
__device__ __forceinline__ Lane lane_of(int C) {
  const int CQ = C >> 2;   // a power of two
  return Lane{(int)threadIdx.x & (CQ - 1), (int)threadIdx.x / CQ, 256 / CQ};
}

__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
  return f32x4{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)};
}

// mean and rstd of this thread's four channels
struct Stats {
  f32x4 mean, rstd;
  // A: an argument struct with mean, rstd, running, eps
  template <typename A>
  __device__ __forceinline__ void load(const A& a, int cq) {
    mean = *reinterpret_cast<const f32x4*>(a.mean + 4 * cq);
    rstd = *reinterpret_cast<const f32x4*>(a.rstd + 4 * cq);
    if (a.running) {   // `rstd` holds the running variance
      rstd = f32x4{1.f / sqrtf(rstd.x + a.eps), 1.f / sqrtf(rstd.y + a.eps), 1.f / sqrtf(rstd.z + a.eps), 1.f / sqrtf(rstd.w + a.eps)};
    }
  }
  __device__ __forceinline__ f32x4 xhat(const f32x4& x) const { return (x - mean) * rstd; }
};

// the normalisation of this thread's four channels.  The backward forms the ReLU mask and the pool's arg-max from the same expression
// as the forward stored its output from, so the two agree bit for bit.
struct Norm : Stats {
  f32x4 gamma, beta;
  // A: Stats' fields, gamma, beta
  template <typename A>
  __device__ __forceinline__ void load(const A& a, int cq) {
    Stats::load(a, cq);
    gamma = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cq);
    beta = *reinterpret_cast<const f32x4*>(a.beta + 4 * cq);
  }
  // a constant channel gives beta exactly: (x - mean) is an exact zero
  __device__ __forceinline__ f32x4 affine(const f32x4& x) const { return fma4((x - mean) * rstd, gamma, beta); }
  __device__ __forceinline__ f32x4 operator()(const f32x4& x) const { return relu4(affine(x)); }
};

// a thread's rows r, r + PAR, ... < r1 in index order: use(row, load(row)), the loads of BATCH rows issued before the first use
template <int BATCH, typename Load, typename Use>
__device__ __forceinline__ void bn_rows(int r, int r1, int PAR, Load load, Use use) {
  if constexpr (BATCH > 1) {
    for (; r + (BATCH - 1) * PAR < r1; r += BATCH * PAR) {
      decltype(load(r)) v[BATCH];
#pragma unroll
      for (int i = 0; i < BATCH; ++i) v[i] = load(r + i * PAR);
#pragma unroll
      for (int i = 0; i < BATCH; ++i) use(r + i * PAR, v[i]);
    }
  }
  for (; r < r1; r += PAR) use(r, load(r));
}

// The 3 x 3 stride-2 window (padding 1) of a pooled element, one axis at a time: tap k < 3 of pooled coordinate p sits at image
// coordinate x = 2 p - 1 + k; -> whether that is inside [0, L).  The walk over a window's in-image positions in (kh, kw) row-major
// order is a loop over kh around a loop over kw, each skipping the taps outside; the position's number is 3 kh + kw, and the centre
// (kh = kw = 1) is always inside.  The two loops stand in the kernel: handed to a helper as a callback, or flattened to one loop
// over nine taps, they compile to other address arithmetic and the max-pool forward of layer 1 takes 0.8 to 2.5 % longer.
__device__ __forceinline__ bool pool_tap(int k, int p, int L, int& x) {
  x = 2 * p - 1 + k;
  return x >= 0 && x < L;
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// Chan's merge of (na, ma, M2a) with (nb, mb, M2b); nb may be 0
__device__ __forceinline__ void chan_merge(float na, f32x4& ma, f32x4& M2a, float nb, const f32x4& mb, const f32x4& M2b) {
  const float n = na + nb;
  if (nb == 0.f) return;
  const float fb = nb / n, fab = na * fb;
  const f32x4 d = mb - ma;
  ma += d * fb;
  M2a += M2b + d * d * fab;
}

// per-block partials: scratch[block][0][C] = mean, scratch[block][1][C] = M2 of the block's rows
template <bool F32>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const void* x, int ld, int C, int M, int rpb, float* scratch) {
  __shared__ f32x4 sm[256], sM2[256];
  __shared__ float sn[16];
  const Lane l = lane_of(C);
  const int CQ = C >> 2, r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  f32x4 mean{0.f, 0.f, 0.f, 0.f}, M2{0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  bn_rows<4>(r0 + l.par, r1, l.PAR, [&](int r) __attribute__((always_inline)) { return ld4<F32>(x, (long long)r * ld + 4 * l.cq); },
             [&](int, const f32x4& v) __attribute__((always_inline)) {
               n += 1.f;
               const float inv = 1.f / n;
               const f32x4 d = v - mean;
               mean += d * inv;
               M2 += d * (v - mean);
             });
  sm[threadIdx.x] = mean; sM2[threadIdx.x] = M2;
  if (l.cq == 0) sn[l.par] = n;
  __syncthreads();
  if (l.par != 0) return;
  for (int q = 1; q < l.PAR; ++q) {
    chan_merge(n, mean, M2, sn[q], sm[q * CQ + l.cq], sM2[q * CQ + l.cq]);
    n += sn[q];
  }
  float* part = scratch + (long long)blockIdx.x * 2 * C;
  *reinterpret_cast<f32x4*>(part + 4 * l.cq) = mean;
  *reinterpret_cast<f32x4*>(part + C + 4 * l.cq) = M2;
}

// The channels of an operator's rows -- a constant where the operator has one width only: the fold's loads are a chain of dependent
// steps, and with C = 512 known their addresses cost no 64-bit multiply (the launch is 7 % longer at R = 32768 without).
template <typename A>
__device__ __forceinline__ int bn_channels(const A& a) { return a.C; }
__device__ __forceinline__ int bn_channels(const mmdeer_bn_time_args&) { return 512; }

// the fold of the blocks' (count, mean, M2) per channel (the head of this file), mean / rstd and the running-buffer update.
// A: an argument struct with C, scratch, mean, rstd, eps, running_mean, running_var, momentum, num_batches_tracked
template <typename A>
__global__ __launch_bounds__(256) void bn_stats_final_kernel(A a, int M, int rpb, int nblk) {
  __shared__ float sn[BN_FOLD_SEG][BN_FOLD_CH], sm[BN_FOLD_SEG][BN_FOLD_CH], sM2[BN_FOLD_SEG][BN_FOLD_CH];
  const int C = bn_channels(a);
  const int cl = threadIdx.x % BN_FOLD_CH, seg = threadIdx.x / BN_FOLD_CH, c = blockIdx.x * BN_FOLD_CH + cl;
  const int per = (nblk + BN_FOLD_SEG - 1) / BN_FOLD_SEG, b0 = seg * per, b1 = min(b0 + per, nblk);
  float n = 0.f, mean = 0.f, M2 = 0.f;
  auto merge = [&](float nb, float mb, float M2b) __attribute__((always_inline)) {
    if (nb == 0.f) return;
    const float nn = n + nb, fb = nb / nn, d = mb - mean;
    mean += d * fb;
    M2 += M2b + d * d * (n * fb);
    n = nn;
  };
#pragma unroll 4
  for (int b = b0; b < b1; ++b)
    merge((float)min(rpb, M - b * rpb), a.scratch[(long long)b * 2 * C + c], a.scratch[(long long)b * 2 * C + C + c]);
  sn[seg][cl] = n; sm[seg][cl] = mean; sM2[seg][cl] = M2;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < BN_FOLD_SEG; ++s) merge(sn[s][cl], sm[s][cl], sM2[s][cl]);
  const float var = M2 / (float)M;
  a.mean[c] = mean;
  a.rstd[c] = 1.f / sqrtf(var + a.eps);
  if (a.running_mean) {
    const float unbiased = M > 1 ? M2 / (float)(M - 1) : var;
    a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
    a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * unbiased;
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
  }
}

// the statistics of x [M > 0][ld >= a->C] as two launches.  A: bn_stats_final_kernel's, with act_f32 and stream
template <typename A>
int bn_launch_stats(const A* a, const char* op, const void* x, int ld, int M) {
  MMDEER_CHECK(a->mean && a->rstd && a->scratch && al16(a->scratch), "%s: NULL pointer (mean, rstd, scratch) or misaligned scratch", op);
  MMDEER_CHECK(!a->running_mean == !a->running_var, "%s: running_mean and running_var go together", op);
  MMDEER_CHECK(a->running_mean || !a->num_batches_tracked, "%s: num_batches_tracked needs the running buffers", op);
  const RowPlan p = bn_row_plan(M);
  hipStream_t s = (hipStream_t)a->stream;
  MMDEER_LAUNCH_ACT(bn_stats_partial_kernel, a->act_f32, dim3(p.nblk), dim3(256), s, x, ld, a->C, M, p.rpb, a->scratch);
  hipLaunchKernelGGL(bn_stats_final_kernel<A>, dim3(a->C / BN_FOLD_CH), dim3(256), 0, s, *a, M, p.rpb, p.nblk);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ backward
// A gradient functor G is the operator's side of the backward, for this thread's four channels:
//   typename G::Args            the operator's argument struct (with C, running, scratch, dgamma, dbeta)
//   void init(a, cq)            load what every row needs
//   f32x4 operator()(r, xhat)   g of row r, and the row's xhat into `xhat`
//   f32x4 scale()               gamma * rstd
//   void store(r, dx)           the input gradient of row r
// BATCH: bn_rows' -- rows whose loads are issued together.

// per-block partial sums: scratch[block][0][C] = sum g, scratch[block][1][C] = sum g * xhat
template <typename G, int BATCH>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(typename G::Args a, int M, int rpb) {
  __shared__ f32x4 sg[256], sx[256];
  const Lane l = lane_of(a.C);
  G grad;
  grad.init(a, l.cq);
  const int CQ = a.C >> 2, r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  f32x4 s{0.f, 0.f, 0.f, 0.f}, sxh{0.f, 0.f, 0.f, 0.f};
  struct GX { f32x4 g, xh; };
  bn_rows<BATCH>(r0 + l.par, r1, l.PAR, [&](int r) __attribute__((always_inline)) { GX v; v.g = grad(r, v.xh); return v; },
                 [&](int, const GX& v) __attribute__((always_inline)) {
                   s += v.g;
                   sxh = fma4(v.g, v.xh, sxh);
                 });
  sg[threadIdx.x] = s; sx[threadIdx.x] = sxh;
  __syncthreads();
  if (l.par != 0) return;
  for (int q = 1; q < l.PAR; ++q) {
    s += sg[q * CQ + l.cq];
    sxh += sx[q * CQ + l.cq];
  }
  float* part = a.scratch + (long long)blockIdx.x * 2 * a.C;
  *reinterpret_cast<f32x4*>(part + 4 * l.cq) = s;
  *reinterpret_cast<f32x4*>(part + a.C + 4 * l.cq) = sxh;
}

// dbeta / dgamma: the fold of the blocks' partial sums (the head of this file)
__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(const float* scratch, float* dbeta, float* dgamma, int C, int nblk) {
  __shared__ float sb[BN_FOLD_SEG][BN_FOLD_CH], sg[BN_FOLD_SEG][BN_FOLD_CH];
  const int cl = threadIdx.x % BN_FOLD_CH, seg = threadIdx.x / BN_FOLD_CH, c = blockIdx.x * BN_FOLD_CH + cl;
  const int per = (nblk + BN_FOLD_SEG - 1) / BN_FOLD_SEG, b0 = seg * per, b1 = min(b0 + per, nblk);
  float db = 0.f, dg = 0.f;
#pragma unroll 4
  for (int b = b0; b < b1; ++b) {
    db += scratch[(long long)b * 2 * C + c];
    dg += scratch[(long long)b * 2 * C + C + c];
  }
  sb[seg][cl] = db; sg[seg][cl] = dg;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < BN_FOLD_SEG; ++s) { db += sb[s][cl]; dg += sg[s][cl]; }
  dbeta[c] = db;
  dgamma[c] = dg;
}

template <typename G, int BATCH>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(typename G::Args a, int M, int rpb) {
  const Lane l = lane_of(a.C);
  G grad;
  grad.init(a, l.cq);
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  const float inv_m = 1.f / (float)M;
  const f32x4 scale = grad.scale();
  f32x4 mb{0.f, 0.f, 0.f, 0.f}, mg{0.f, 0.f, 0.f, 0.f};
  if (!a.running) {
    mb = *reinterpret_cast<const f32x4*>(a.dbeta + 4 * l.cq) * inv_m;
    mg = *reinterpret_cast<const f32x4*>(a.dgamma + 4 * l.cq) * inv_m;
  }
  struct GX { f32x4 g, xh; };
  bn_rows<BATCH>(r0 + l.par, r1, l.PAR, [&](int r) __attribute__((always_inline)) { GX v; v.g = grad(r, v.xh); return v; },
                 [&](int r, const GX& v) __attribute__((always_inline)) { grad.store(r, scale * (v.g - mb - v.xh * mg)); });
}

// the three launches of the backward over M > 0 rows
template <typename G, int BATCH>
int bn_launch_bwd(const typename G::Args& a, int M) {
  const RowPlan p = bn_row_plan(M);
  hipStream_t s = (hipStream_t)a.stream;
  hipLaunchKernelGGL((bn_bwd_partial_kernel<G, BATCH>), dim3(p.nblk), dim3(256), 0, s, a, M, p.rpb);
  hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3(a.C / BN_FOLD_CH), dim3(256), 0, s, a.scratch, a.dbeta, a.dgamma, a.C, p.nblk);
  hipLaunchKernelGGL((bn_bwd_dx_kernel<G, BATCH>), dim3(p.nblk), dim3(256), 0, s, a, M, p.rpb);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace mmdeer
