// The backward of nn.BatchNorm2d(C) + ReLU (+ MaxPool2d(3, 2, 1) / AdaptiveAvgPool2d(1)) of the frame video encoder's backbone on the
// dense channels-last output y [M = N * H * W][C] of a convolution (include/mmdeer_frames_bwd.h), C in {64, 128, 256, 512}.
//
// Lane mapping: bn2d.hip's (bn2d_norm.h) -- thread t owns four consecutive channels of every PAR-th row of its workgroup's share.
// The ReLU mask and the pool's arg-max come from Norm, the expression the forward stored its output from.
//
// Launches.  POOL source only: one index byte per pooled element (the first maximum of its window in (kh, kw) row-major order among
// the in-image positions).  Then, for every source: per-block partial sums of g and g * xhat over the block's rows (each thread its
// rows in index order, the PAR partials of a workgroup in index order out of LDS) into scratch; the fold of the blocks per channel
// in a fixed order (bn_fold.h's split: segments of consecutive blocks, then the segments) into dbeta and dgamma; and dy.  g is
// formed twice, by one function: the upstream gradient is gathered, never scattered, so there is no atomic and no ordering to fix.
#include "../../include/mmdeer_frames_bwd.h"
#include "bn2d_norm.h"

namespace mmdeer {
namespace {

static_assert(BN_MAXBLK * 2 * 512 == MMDEER_BN2D_BWD_SCRATCH, "scratch holds two per-channel partials per row block");

// g = u * (v > 0) and xhat of this thread's four channels of row r
template <bool F32, int SRC>
struct Grad {
  Norm norm;
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
    y = a.y; dout = a.dout; idx = reinterpret_cast<const unsigned char*>(a.pool_idx);
  }
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
      const int h = 2 * ph - 1 + i;
      if (h < 0 || h >= H) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int w = 2 * pw - 1 + j;
        if (w < 0 || w >= W) continue;
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

// per-block partial sums: scratch[block][0][C] = sum g, scratch[block][1][C] = sum g * xhat
template <bool F32, int SRC>
__global__ __launch_bounds__(256) void bn2d_bwd_partial_kernel(mmdeer_bn2d_bwd_args a, int M, int rpb) {
  __shared__ f32x4 sg[256], sx[256];
  const Lane l = lane_of(a.C);
  Grad<F32, SRC> grad;
  grad.init(a, l.cq);
  const int CQ = a.C >> 2, r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  f32x4 s{0.f, 0.f, 0.f, 0.f}, sxh{0.f, 0.f, 0.f, 0.f};
  for (int r = r0 + l.par; r < r1; r += l.PAR) {
    f32x4 xh;
    const f32x4 g = grad(r, xh);
    s += g;
    sxh = fma4(g, xh, sxh);
  }
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

// the fold of the blocks' partials: a workgroup owns BN_FOLD_CH channels, its threads are BN_FOLD_SEG segments of consecutive blocks
__global__ __launch_bounds__(256) void bn2d_bwd_fold_kernel(mmdeer_bn2d_bwd_args a, int nblk) {
  __shared__ float sb[BN_FOLD_SEG][BN_FOLD_CH], sg[BN_FOLD_SEG][BN_FOLD_CH];
  const int C = a.C, cl = threadIdx.x % BN_FOLD_CH, seg = threadIdx.x / BN_FOLD_CH, c = blockIdx.x * BN_FOLD_CH + cl;
  const int per = (nblk + BN_FOLD_SEG - 1) / BN_FOLD_SEG, b0 = seg * per, b1 = min(b0 + per, nblk);
  float db = 0.f, dg = 0.f;
  for (int b = b0; b < b1; ++b) {
    db += a.scratch[(long long)b * 2 * C + c];
    dg += a.scratch[(long long)b * 2 * C + C + c];
  }
  sb[seg][cl] = db; sg[seg][cl] = dg;
  __syncthreads();
  if (seg != 0) return;
  for (int s = 1; s < BN_FOLD_SEG; ++s) { db += sb[s][cl]; dg += sg[s][cl]; }
  a.dbeta[c] = db;
  a.dgamma[c] = dg;
}

template <bool F32, int SRC>
__global__ __launch_bounds__(256) void bn2d_bwd_dy_kernel(mmdeer_bn2d_bwd_args a, int M, int rpb) {
  const Lane l = lane_of(a.C);
  Grad<F32, SRC> grad;
  grad.init(a, l.cq);
  const int r0 = blockIdx.x * rpb, r1 = min(r0 + rpb, M);
  const float inv_m = 1.f / (float)M;
  const f32x4 scale = grad.norm.gamma * grad.norm.rstd;
  f32x4 mb{0.f, 0.f, 0.f, 0.f}, mg{0.f, 0.f, 0.f, 0.f};
  if (!a.running) {
    mb = *reinterpret_cast<const f32x4*>(a.dbeta + 4 * l.cq) * inv_m;
    mg = *reinterpret_cast<const f32x4*>(a.dgamma + 4 * l.cq) * inv_m;
  }
  for (int r = r0 + l.par; r < r1; r += l.PAR) {
    f32x4 xh;
    const f32x4 g = grad(r, xh);
    st4<F32>(a.dy, (long long)r * a.C + 4 * l.cq, scale * (g - mb - xh * mg));
  }
}

constexpr long long LIMIT = 1ll << 31;   // elements of one buffer

template <bool F32, int SRC>
int launch_bn2d_bwd(const mmdeer_bn2d_bwd_args& a, int M, hipStream_t s) {
  const int rpb = bn_rows_per_block(M), nblk = bn_blocks(M);
  hipLaunchKernelGGL((bn2d_bwd_partial_kernel<F32, SRC>), dim3(nblk), dim3(256), 0, s, a, M, rpb);
  hipLaunchKernelGGL(bn2d_bwd_fold_kernel, dim3(a.C / BN_FOLD_CH), dim3(256), 0, s, a, nblk);
  hipLaunchKernelGGL((bn2d_bwd_dy_kernel<F32, SRC>), dim3(nblk), dim3(256), 0, s, a, M, rpb);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

template <bool F32>
int launch_bn2d_bwd_src(const mmdeer_bn2d_bwd_args& a, int M, hipStream_t s) {
  if (a.src == MMDEER_BN2D_SRC_DENSE) return launch_bn2d_bwd<F32, MMDEER_BN2D_SRC_DENSE>(a, M, s);
  if (a.src == MMDEER_BN2D_SRC_AVG) return launch_bn2d_bwd<F32, MMDEER_BN2D_SRC_AVG>(a, M, s);
  const int PH = (a.H - 1) / 2 + 1, PW = (a.W - 1) / 2 + 1;
  const long long Q = (long long)a.N * PH * PW;
  long long ppb = (Q + BN_MAXBLK - 1) / BN_MAXBLK;   // pooled elements per workgroup: at least 32, and at most BN_MAXBLK workgroups
  if (ppb < 32) ppb = 32;
  hipLaunchKernelGGL((bn2d_pool_index_kernel<F32>), dim3((unsigned)((Q + ppb - 1) / ppb)), dim3(256), 0, s, a, PH, PW, Q, (int)ppb);
  return launch_bn2d_bwd<F32, MMDEER_BN2D_SRC_POOL>(a, M, s);
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bn2d_bwd(const mmdeer_bn2d_bwd_args* a) {
  MMDEER_CHECK(a, "bn2d_bwd: NULL argument struct");
  MMDEER_CHECK(a->C == 64 || a->C == 128 || a->C == 256 || a->C == 512, "bn2d_bwd: unsupported C=%d (64, 128, 256 or 512)", a->C);
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "bn2d_bwd: bad shape N=%d H=%d W=%d", a->N, a->H, a->W);
  MMDEER_CHECK((long long)a->N * a->H * a->W * a->C < LIMIT, "bn2d_bwd: y has 2^31 elements or more");
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
  hipStream_t s = (hipStream_t)a->stream;
  return a->act_f32 ? launch_bn2d_bwd_src<true>(*a, M, s) : launch_bn2d_bwd_src<false>(*a, M, s);
}

}  // extern "C"
