// Device code shared by the batch normalisations over rows (bn_time.hip: BatchNorm1d on [R][512]; bn2d.hip: BatchNorm2d on the dense
// channels-last output [M][C] of a convolution): Chan's merge of Welford partials, the row-block split, and the second launch of the
// statistics -- the fold of the blocks' (count, mean, M2) per channel in a fixed order, mean / rstd and the running-buffer update.
#pragma once
#include "elem.h"

namespace mmdeer {
namespace {

constexpr int BN_MAXBLK = 1024;    // row blocks at most; scratch = BN_MAXBLK * 2 * C floats
constexpr int BN_FOLD_CH = 8, BN_FOLD_SEG = 32;   // fold kernels: channels per workgroup, block segments per channel

// rows per block: at least 32, even, and at most BN_MAXBLK blocks
inline int bn_rows_per_block(int R) {
  int rpb = (R + BN_MAXBLK - 1) / BN_MAXBLK;
  if (rpb < 32) rpb = 32;
  return (rpb + 1) & ~1;
}
inline int bn_blocks(int R) { const int rpb = bn_rows_per_block(R); return (R + rpb - 1) / rpb; }

// Chan's merge of (na, ma, M2a) with (nb, mb, M2b); nb may be 0
__device__ __forceinline__ void chan_merge(float na, f32x4& ma, f32x4& M2a, float nb, const f32x4& mb, const f32x4& M2b) {
  const float n = na + nb;
  if (nb == 0.f) return;
  const float fb = nb / n, fab = na * fb;
  const f32x4 d = mb - ma;
  ma += d * fb;
  M2a += M2b + d * d * fab;
}

__device__ __forceinline__ f32x4 fma4(f32x4 a, f32x4 b, f32x4 c) {
  return f32x4{fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w)};
}

// Fold of the blocks' (count, mean, M2) over R rows of C channels, by a workgroup of 256 threads that owns BN_FOLD_CH channels: its
// threads are BN_FOLD_SEG segments of consecutive blocks x BN_FOLD_CH channels; each thread folds its segment in index order, then
// the threads of segment 0 fold the segment results in index order out of LDS.  The order is a function of R alone.
// A: an argument struct with scratch, mean, rstd, eps, running_mean, running_var, momentum, num_batches_tracked.
template <typename A>
__device__ __forceinline__ void bn_fold_stats(const A& a, int R, int C, int rpb, int nblk) {
  __shared__ float sn[BN_FOLD_SEG][BN_FOLD_CH], sm[BN_FOLD_SEG][BN_FOLD_CH], sM2[BN_FOLD_SEG][BN_FOLD_CH];
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
    merge((float)min(rpb, R - b * rpb), a.scratch[(long long)b * 2 * C + c], a.scratch[(long long)b * 2 * C + C + c]);
  sn[seg][cl] = n; sm[seg][cl] = mean; sM2[seg][cl] = M2;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < BN_FOLD_SEG; ++s) merge(sn[s][cl], sm[s][cl], sM2[s][cl]);
  const float var = M2 / (float)R;
  a.mean[c] = mean;
  a.rstd[c] = 1.f / sqrtf(var + a.eps);
  if (a.running_mean) {
    const float unbiased = R > 1 ? M2 / (float)(R - 1) : var;
    a.running_mean[c] = (1.f - a.momentum) * a.running_mean[c] + a.momentum * mean;
    a.running_var[c] = (1.f - a.momentum) * a.running_var[c] + a.momentum * unbiased;
    if (c == 0 && a.num_batches_tracked) *a.num_batches_tracked += 1;
  }
}

}  // namespace
}  // namespace mmdeer
