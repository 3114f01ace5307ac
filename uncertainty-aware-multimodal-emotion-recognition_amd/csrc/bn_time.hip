// nn.BatchNorm1d(512) over the rows of an [R][512] activation matrix, for the temporal video encoder (reference
// src/models/encoders.py:450-459): the statistics are per channel over all R = T * B rows -- the library's only normalisation
// across rows.
//
// Lane mapping (all kernels): a workgroup owns a block of consecutive rows; thread t owns the four consecutive channels
// 4 * (t & 127) .. + 3 (one 16-byte fp32 / 8-byte bf16 access per row) of every second row of the block, rows of parity t >> 7.
// A wave therefore reads 1 KiB (fp32) of one row per instruction, and a thread issues the loads of four of its rows before it uses the
// first (the row loops are written out in batches of four: the stores of `out` / `dx` may alias the loads as far as the compiler
// knows, so it would not hoist them itself).  The row block length is 32 rows, or longer so that at most BN_MAXBLK workgroups run:
// their per-channel partials fit the fixed scratch.
// Folds of the per-block partials: a workgroup owns 8 channels, its 256 threads are 32 segments of consecutive blocks x 8 channels;
// each thread folds its segment in index order, then the threads of segment 0 fold the 32 segment results in index order out of
// LDS.  The order is a function of (R) alone: deterministic.  (One thread per channel over all blocks took 68 us at 256 blocks: a
// chain of dependent 300 ns steps on two workgroups.)
//
// Statistics: each thread runs Welford's update over its rows (one reciprocal per row, shared by its four channels), the two
// row parities of a workgroup are merged by Chan's formula through LDS, and the per-block (mean, M2) -- the count follows from
// the block index -- go to scratch.  A second launch merges the blocks per channel, again by Chan's formula, writes mean and
// rstd and updates the running buffers.  Fixed order, no atomics: deterministic.  A plain (sum x, sum x^2) loses
// every digit of the variance of a channel whose mean is large against its spread; this form does not.
// Backward: the same block structure for the partial sums of g and g * xhat, a fold launch, then dx.
#include "../../include/mmdeer_video.h"
#include "bn_fold.h"

namespace mmdeer {
namespace {

constexpr int BN_C = 512;          // channels
static_assert(BN_MAXBLK * 2 * BN_C == MMDEER_BN_TIME_SCRATCH, "scratch holds two per-channel partials per row block");

template <bool F32>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(mmdeer_bn_time_args a, int rpb) {
  __shared__ f32x4 sm[128], sM2[128];
  __shared__ float sn;
  const int tid = threadIdx.x, cq = tid & 127, par = tid >> 7;
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, a.R);
  f32x4 mean{0.f, 0.f, 0.f, 0.f}, M2{0.f, 0.f, 0.f, 0.f};
  float n = 0.f;
  auto update = [&](const f32x4& x) __attribute__((always_inline)) {
    n += 1.f;
    const float inv = 1.f / n;
    const f32x4 d = x - mean;
    mean += d * inv;
    M2 += d * (x - mean);
  };
  auto row = [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.ld_x + 4 * cq); };
  int r = r0 + par;
  for (; r + 6 < r1; r += 8) {
    const f32x4 x0 = row(r), x1 = row(r + 2), x2 = row(r + 4), x3 = row(r + 6);
    update(x0); update(x1); update(x2); update(x3);
  }
  for (; r < r1; r += 2) update(row(r));
  if (par == 1) { sm[cq] = mean; sM2[cq] = M2; if (cq == 0) sn = n; }
  __syncthreads();
  if (par == 0) {
    chan_merge(n, mean, M2, sn, sm[cq], sM2[cq]);
    float* part = a.scratch + (long long)blockIdx.x * 2 * BN_C;
    *reinterpret_cast<f32x4*>(part + 4 * cq) = mean;
    *reinterpret_cast<f32x4*>(part + BN_C + 4 * cq) = M2;
  }
}

// fold of the blocks' (count, mean, M2): see the head of this file and bn_fold.h
__global__ __launch_bounds__(256) void bn_stats_final_kernel(mmdeer_bn_time_args a, int rpb, int nblk) {
  bn_fold_stats(a, a.R, BN_C, rpb, nblk);
}

// mean and rstd of this thread's four channels (running != 0: `rstd` holds the running variance)
__device__ __forceinline__ void bn_load_stats(const mmdeer_bn_time_args& a, int cq, f32x4& mean, f32x4& rstd) {
  mean = *reinterpret_cast<const f32x4*>(a.mean + 4 * cq);
  rstd = *reinterpret_cast<const f32x4*>(a.rstd + 4 * cq);
  if (a.running) {
    rstd = f32x4{1.f / sqrtf(rstd.x + a.eps), 1.f / sqrtf(rstd.y + a.eps), 1.f / sqrtf(rstd.z + a.eps), 1.f / sqrtf(rstd.w + a.eps)};
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void bn_apply_kernel(mmdeer_bn_time_args a, DropCtx dc, int rpb) {
  const int tid = threadIdx.x, cq = tid & 127, par = tid >> 7;
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, a.R);
  f32x4 mean, rstd;
  bn_load_stats(a, cq, mean, rstd);
  const f32x4 gamma = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cq), beta = *reinterpret_cast<const f32x4*>(a.beta + 4 * cq);
  const bool drop = a.drop_site >= 0 && a.dropout_p > 0.f;
  const unsigned dkey = drop ? drop_key(dc, a.drop_site) : 0u;
  auto row = [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.ld_x + 4 * cq); };
  auto emit = [&](int r, const f32x4& x) __attribute__((always_inline)) {
    f32x4 v = fma4((x - mean) * rstd, gamma, beta);   // a constant channel gives beta exactly: (x - mean) is an exact zero
    if (a.relu) v = relu4(v);
    if (drop) v = drop4(v, ((unsigned)r * 0x9E3779B1u) ^ dkey, (unsigned)(4 * cq), 0, dc);
    st4<F32>(a.out, (long long)r * a.ld_out + 4 * cq, v);
  };
  int r = r0 + par;
  for (; r + 6 < r1; r += 8) {
    const f32x4 x0 = row(r), x1 = row(r + 2), x2 = row(r + 4), x3 = row(r + 6);
    emit(r, x0); emit(r + 2, x1); emit(r + 4, x2); emit(r + 6, x3);
  }
  for (; r < r1; r += 2) emit(r, row(r));
}

// g = dout * (out > 0) * mask_scale of this thread's four channels in row r
template <bool F32>
__device__ __forceinline__ f32x4 bn_grad_in(const mmdeer_bn_time_args& a, int r, int cq) {
  f32x4 g = ld4<F32>(a.dout, (long long)r * a.ld_dout + 4 * cq);
  if (a.out) {
    const f32x4 o = ld4<F32>(a.out, (long long)r * a.ld_out + 4 * cq);
    const float ms = a.mask_scale;
    g = f32x4{o.x > 0.f ? g.x * ms : 0.f, o.y > 0.f ? g.y * ms : 0.f, o.z > 0.f ? g.z * ms : 0.f, o.w > 0.f ? g.w * ms : 0.f};
  }
  return g;
}

template <bool F32>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(mmdeer_bn_time_args a, int rpb) {
  __shared__ f32x4 s0[128], s1[128];
  const int tid = threadIdx.x, cq = tid & 127, par = tid >> 7;
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, a.R);
  f32x4 mean, rstd;
  bn_load_stats(a, cq, mean, rstd);
  f32x4 sg{0.f, 0.f, 0.f, 0.f}, sgx{0.f, 0.f, 0.f, 0.f};
  auto row = [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.ld_x + 4 * cq); };
  auto add = [&](const f32x4& g, const f32x4& x) __attribute__((always_inline)) {
    sg += g;
    sgx = fma4(g, (x - mean) * rstd, sgx);
  };
  int r = r0 + par;
  for (; r + 6 < r1; r += 8) {
    const f32x4 g0 = bn_grad_in<F32>(a, r, cq), g1 = bn_grad_in<F32>(a, r + 2, cq), g2 = bn_grad_in<F32>(a, r + 4, cq), g3 = bn_grad_in<F32>(a, r + 6, cq);
    const f32x4 x0 = row(r), x1 = row(r + 2), x2 = row(r + 4), x3 = row(r + 6);
    add(g0, x0); add(g1, x1); add(g2, x2); add(g3, x3);
  }
  for (; r < r1; r += 2) add(bn_grad_in<F32>(a, r, cq), row(r));
  if (par == 1) { s0[cq] = sg; s1[cq] = sgx; }
  __syncthreads();
  if (par == 0) {
    float* part = a.scratch + (long long)blockIdx.x * 2 * BN_C;
    *reinterpret_cast<f32x4*>(part + 4 * cq) = sg + s0[cq];
    *reinterpret_cast<f32x4*>(part + BN_C + 4 * cq) = sgx + s1[cq];
  }
}

// dbeta / dgamma: fold of the blocks' partial sums (see the head of this file)
__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(mmdeer_bn_time_args a, int nblk) {
  __shared__ float s0[BN_FOLD_SEG][BN_FOLD_CH], s1[BN_FOLD_SEG][BN_FOLD_CH];
  const int cl = threadIdx.x % BN_FOLD_CH, seg = threadIdx.x / BN_FOLD_CH, c = blockIdx.x * BN_FOLD_CH + cl;
  const int per = (nblk + BN_FOLD_SEG - 1) / BN_FOLD_SEG, b0 = seg * per, b1 = min(b0 + per, nblk);
  float sg = 0.f, sgx = 0.f;
#pragma unroll 4
  for (int b = b0; b < b1; ++b) {
    sg += a.scratch[(long long)b * 2 * BN_C + c];
    sgx += a.scratch[(long long)b * 2 * BN_C + BN_C + c];
  }
  s0[seg][cl] = sg; s1[seg][cl] = sgx;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < BN_FOLD_SEG; ++s) { sg += s0[s][cl]; sgx += s1[s][cl]; }
  a.dbeta[c] = sg;
  a.dgamma[c] = sgx;
}

template <bool F32>
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(mmdeer_bn_time_args a, int rpb) {
  const int tid = threadIdx.x, cq = tid & 127, par = tid >> 7;
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, a.R);
  f32x4 mean, rstd;
  bn_load_stats(a, cq, mean, rstd);
  const f32x4 k = *reinterpret_cast<const f32x4*>(a.gamma + 4 * cq) * rstd;
  f32x4 mb{0.f, 0.f, 0.f, 0.f}, mg{0.f, 0.f, 0.f, 0.f};
  if (!a.running) {
    const float invR = 1.f / (float)a.R;
    mb = *reinterpret_cast<const f32x4*>(a.dbeta + 4 * cq) * invR;
    mg = *reinterpret_cast<const f32x4*>(a.dgamma + 4 * cq) * invR;
  }
  auto row = [&](int r) __attribute__((always_inline)) { return ld4<F32>(a.x, (long long)r * a.ld_x + 4 * cq); };
  auto emit = [&](int r, const f32x4& g, const f32x4& x) __attribute__((always_inline)) {
    st4<F32>(a.dx, (long long)r * a.ld_dx + 4 * cq, k * (g - mb - (x - mean) * rstd * mg));
  };
  int r = r0 + par;
  for (; r + 6 < r1; r += 8) {
    const f32x4 g0 = bn_grad_in<F32>(a, r, cq), g1 = bn_grad_in<F32>(a, r + 2, cq), g2 = bn_grad_in<F32>(a, r + 4, cq), g3 = bn_grad_in<F32>(a, r + 6, cq);
    const f32x4 x0 = row(r), x1 = row(r + 2), x2 = row(r + 4), x3 = row(r + 6);
    emit(r, g0, x0); emit(r + 2, g1, x1); emit(r + 4, g2, x2); emit(r + 6, g3, x3);
  }
  for (; r < r1; r += 2) emit(r, bn_grad_in<F32>(a, r, cq), row(r));
}

int check_bn(const mmdeer_bn_time_args* a, const char* op) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->C == BN_C, "%s: C must be %d (got %d)", op, BN_C, a->C);
  MMDEER_CHECK(a->R >= 0, "%s: bad row count R=%d", op, a->R);
  return 0;
}
bool act_ok(const mmdeer_bn_time_args* a, const void* p, int ld) {
  return p && al16(p) && ld >= BN_C && ld % (a->act_f32 ? 4 : 8) == 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn_time_stats(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_stats"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x), "bn_time_stats: x must be non-NULL, 16-byte aligned, ld_x >= %d and a multiple of 16 bytes", BN_C);
  MMDEER_CHECK(a->mean && a->rstd && a->scratch && al16(a->scratch), "bn_time_stats: NULL pointer (mean, rstd, scratch) or misaligned scratch");
  MMDEER_CHECK(!a->running_mean == !a->running_var, "bn_time_stats: running_mean and running_var go together");
  MMDEER_CHECK(a->running_mean || !a->num_batches_tracked, "bn_time_stats: num_batches_tracked needs the running buffers");
  const int rpb = bn_rows_per_block(a->R), nblk = bn_blocks(a->R);
  hipStream_t s = (hipStream_t)a->stream;
  MMDEER_LAUNCH_ACT(bn_stats_partial_kernel, a->act_f32, dim3(nblk), dim3(256), s, *a, rpb);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(BN_C / BN_FOLD_CH), dim3(256), 0, s, *a, rpb, nblk);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_bn_time_apply(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_apply"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x) && act_ok(a, a->out, a->ld_out),
               "bn_time_apply: x and out must be non-NULL, 16-byte aligned, ld >= %d and a multiple of 16 bytes", BN_C);
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->beta && al16(a->mean) && al16(a->rstd) && al16(a->gamma) && al16(a->beta),
               "bn_time_apply: mean, rstd, gamma, beta must be non-NULL and 16-byte aligned");
  MMDEER_CHECK(a->dropout_p >= 0.f && a->dropout_p < 1.f, "bn_time_apply: dropout_p must be in [0, 1)");
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, a->offset_dev);
  const int rpb = bn_rows_per_block(a->R), nblk = bn_blocks(a->R);
  MMDEER_LAUNCH_ACT(bn_apply_kernel, a->act_f32, dim3(nblk), dim3(256), (hipStream_t)a->stream, *a, dc, rpb);
  return 0;
}

int mmdeer_bn_time_bwd(const mmdeer_bn_time_args* a) {
  TRY(check_bn(a, "bn_time_bwd"));
  if (a->R == 0) return 0;
  MMDEER_CHECK(act_ok(a, a->x, a->ld_x) && act_ok(a, a->dout, a->ld_dout) && act_ok(a, a->dx, a->ld_dx) &&
               (!a->out || act_ok(a, a->out, a->ld_out)),
               "bn_time_bwd: x, dout, dx (and out) must be non-NULL, 16-byte aligned, ld >= %d and a multiple of 16 bytes", BN_C);
  MMDEER_CHECK(a->mean && a->rstd && a->gamma && a->dgamma && a->dbeta && a->scratch && al16(a->mean) && al16(a->rstd) &&
               al16(a->gamma) && al16(a->dgamma) && al16(a->dbeta) && al16(a->scratch),
               "bn_time_bwd: mean, rstd, gamma, dgamma, dbeta, scratch must be non-NULL and 16-byte aligned");
  const int rpb = bn_rows_per_block(a->R), nblk = bn_blocks(a->R);
  hipStream_t s = (hipStream_t)a->stream;
  MMDEER_LAUNCH_ACT(bn_bwd_partial_kernel, a->act_f32, dim3(nblk), dim3(256), s, *a, rpb);
  hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3(BN_C / BN_FOLD_CH), dim3(256), 0, s, *a, nblk);
  MMDEER_HIP(hipGetLastError());
  MMDEER_LAUNCH_ACT(bn_bwd_dx_kernel, a->act_f32, dim3(nblk), dim3(256), s, *a, rpb);
  return 0;
}

}  // extern "C"
