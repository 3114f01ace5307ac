// The evidence tail as an operator of its own (reference deer.py:55, 86-98): the last Linear(K -> 4 O) of an evidence net, the
// NIG activations and the three uncertainties in ONE launch, for G nets side by side; and its backward.  nig.hip's kernels are
// the same thing hard-wired to 3 nets x 64 inputs x 1 output inside MultimodalDEER; these take any 1 <= G, O <= 8 and any K that
// is a multiple of 8 up to 512, and the backward takes upstream gradients for all seven outputs.
//
// Forward (grid: 64-sample blocks x G, 256 threads).  Four lanes per sample; lane q of a quad owns the 8-element chunks
// q, q + 4, ... of the sample's K-slice (16-byte loads; a quad reads 64 (bf16) / 128 (fp32) contiguous bytes per step).  The net's
// 4 O x K weights are staged once per workgroup in LDS in the activation dtype (at most 64 KB); the lanes of a wave read at most
// four different addresses of it per step (one per q), so the reads are broadcasts.  The quad's partial dot products are folded
// with two DPP steps and lane o & 3 of the quad writes output o: one 16-byte store of the raw evidence and the seven planes.
// The activations are nig_dev.h's (one rounding per operation), so mu, nu, alpha, beta are bit for bit nig_fwd's for equal evidence.
//
// Backward, three launches, no float atomics:
//   tail_bwd_dx   (same grid): d evidence per (sample, output) -> global (a->devid or the scratch) and LDS; dx = (devid . W) with
//                 the optional (x > 0) * mask_scale factor, W staged in LDS in panels of 256 columns.
//   tail_bwd_dw   (grid: 64-column slices of K x G x P batch parts): x and devid tiles through LDS, 8 fp32 accumulators per
//                 thread over the part's samples in index order -> one partial per part.
//   tail_bwd_fold: dw, db = the P partials added in index order.  Two runs give identical bits.
#include "../../include/mmdeer.h"
#include "elem.h"
#include "nig_dev.h"

namespace mmdeer {
namespace {

constexpr int TAIL_ROWS = 64;        // samples per workgroup (4 lanes each)
constexpr int TAIL_MAX_PARTS = 64;   // batch parts of the weight gradient
constexpr int TAIL_PANEL = 256;      // weight columns staged per pass of the backward

// rows [0, R) x columns [c0, c0 + cols) of the net's [R][K] weights -> LDS [R][cols], 16 bytes per thread and step
template <bool F32>
__device__ __forceinline__ void stage_w(const void* w, long long net_off, int R, int K, int c0, int cols, void* lds) {
  constexpr int EPC = F32 ? 4 : 8;
  const int per_row = cols / EPC, n = R * per_row;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int r = i / per_row, c = (i - r * per_row) * EPC;
    const long long src = net_off + (long long)r * K + c0 + c;
    if constexpr (F32)
      reinterpret_cast<f32x4*>(lds)[i] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(w) + src);
    else
      reinterpret_cast<u32x4*>(lds)[i] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(w) + src);
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void evidence_tail_fwd_kernel(mmdeer_evidence_tail_args a) {
#pragma clang fp contract(off)   // the uncertainties round once per operation, as the reference's tensor expressions do
  extern __shared__ __attribute__((aligned(16))) unsigned char tail_lds[];
  const int g = blockIdx.y, K = a.K, O = a.O, R = 4 * O, GO = a.G * O;
  stage_w<F32>(a.w, (long long)g * R * K, R, K, 0, K, tail_lds);
  __syncthreads();
  const int q = threadIdx.x & 3;
  const int b = blockIdx.x * TAIL_ROWS + (threadIdx.x >> 2);
  const bool live = b < a.B;
  const long long xrow = (long long)(live ? b : 0) * a.ld_x + (long long)g * K;
  const int nchunk = K >> 3;
  for (int o = 0; o < O; ++o) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = q; c < nchunk; c += 4) {
      float x[8];
      ld8<F32>(a.x, xrow + 8 * c, x);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float w[8];
        ld8<F32>(tail_lds, (long long)(4 * o + j) * K + 8 * c, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j] = fmaf(x[i], w[i], acc[j]);
      }
    }
    f32x4 ev;
    ev.x = quad_sum(acc[0]); ev.y = quad_sum(acc[1]); ev.z = quad_sum(acc[2]); ev.w = quad_sum(acc[3]);
    if (live && q == (o & 3)) {
      const f32x4 bias = *reinterpret_cast<const f32x4*>(a.b + (long long)g * R + 4 * o);
      ev += bias;
      const long long col = (long long)g * O + o, at = (long long)b * GO + col, plane = (long long)a.B * GO;
      *reinterpret_cast<f32x4*>(a.evid + 4 * at) = ev;
      const Nig n = nig_act(ev);
      const float am1 = n.alpha - 1.f;
      const float alea = n.beta / am1;
      const float epi = n.beta / (n.nu * am1);
      a.nig_out[at] = n.mu;
      a.nig_out[plane + at] = n.nu;
      a.nig_out[2 * plane + at] = n.alpha;
      a.nig_out[3 * plane + at] = n.beta;
      a.nig_out[4 * plane + at] = alea;
      a.nig_out[5 * plane + at] = epi;
      a.nig_out[6 * plane + at] = alea + epi;
    }
  }
}

// d evidence of one (sample, output) from the upstream gradients of the seven planes; a NULL plane contributes no term at all
__device__ __forceinline__ f32x4 tail_devid(const mmdeer_evidence_tail_args& a, const f32x4& ev, long long at) {
#pragma clang fp contract(off)
  const Nig n = nig_act(ev);
  const float am1 = n.alpha - 1.f;
  const float* const* go = a.g_out;
  const bool hasA = go[4] || go[6], hasE = go[5] || go[6];
  const float gA = (go[4] ? go[4][at] : 0.f) + (go[6] ? go[6][at] : 0.f);     // reaches beta / (alpha - 1)
  const float gE = (go[5] ? go[5][at] : 0.f) + (go[6] ? go[6][at] : 0.f);     // reaches beta / (nu (alpha - 1))
  float dnu = go[1] ? go[1][at] : 0.f, dal = go[2] ? go[2][at] : 0.f, dbe = go[3] ? go[3][at] : 0.f;
  if (hasA) {
    dal -= gA * n.beta / (am1 * am1);
    dbe += gA / am1;
  }
  if (hasE) {
    dnu -= gE * n.beta / (n.nu * n.nu * am1);
    dal -= gE * n.beta / (n.nu * (am1 * am1));
    dbe += gE / (n.nu * am1);
  }
  f32x4 d;
  d.x = go[0] ? go[0][at] : 0.f;
  d.y = softplus_grad(ev.y) * dnu;
  d.z = softplus_grad(ev.z) * dal;
  d.w = softplus_grad(ev.w) * dbe;
  return d;
}

template <bool F32>
__global__ __launch_bounds__(256) void evidence_tail_bwd_dx_kernel(mmdeer_evidence_tail_args a, float* devid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tail_lds[];
  const int g = blockIdx.y, K = a.K, O = a.O, R = 4 * O, GO = a.G * O;
  const int ldd = R + 1;                                      // odd row stride: the 16 samples of a wave hit 16 banks
  float* const de = reinterpret_cast<float*>(tail_lds);       // [TAIL_ROWS][R + 1]
  unsigned char* const wl = tail_lds + ((TAIL_ROWS * ldd * 4 + 15) & ~15);
  const int s = threadIdx.x >> 2, q = threadIdx.x & 3;
  const int b = blockIdx.x * TAIL_ROWS + s;
  const bool live = b < a.B;
  for (int o = q; o < O; o += 4) {
    f32x4 d{0.f, 0.f, 0.f, 0.f};
    if (live) {
      const long long at = (long long)b * GO + (long long)g * O + o;
      d = tail_devid(a, *reinterpret_cast<const f32x4*>(a.evid + 4 * at), at);
      *reinterpret_cast<f32x4*>(devid + 4 * at) = d;
    }
    de[s * ldd + 4 * o] = d.x; de[s * ldd + 4 * o + 1] = d.y; de[s * ldd + 4 * o + 2] = d.z; de[s * ldd + 4 * o + 3] = d.w;
  }
  if (!a.dx) return;                                          // uniform: every thread leaves together
  const float scale = a.mask_scale;
  for (int c0 = 0; c0 < K; c0 += TAIL_PANEL) {
    const int cols = K - c0 < TAIL_PANEL ? K - c0 : TAIL_PANEL;
    __syncthreads();                                          // de written / the previous panel read by everyone
    stage_w<F32>(a.w, (long long)g * R * K, R, K, c0, cols, wl);
    __syncthreads();
    if (!live) continue;
    for (int c = q; c < (cols >> 3); c += 4) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < R; ++r) {
        const float d = de[s * ldd + r];
        float w[8];
        ld8<F32>(wl, (long long)r * cols + 8 * c, w);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = fmaf(d, w[i], acc[i]);
      }
      const long long col = (long long)g * K + c0 + 8 * c;
      if (scale > 0.f) {
        float x[8];
        ld8<F32>(a.x, (long long)b * a.ld_x + col, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = x[i] > 0.f ? acc[i] * scale : 0.f;
      }
      st8<F32>(a.dx, (long long)b * a.ld_dx + col, acc);
    }
  }
}

// partial weight / bias gradients of batch part blockIdx.z: pw [P][G][R][K], pb [P][G][R]
template <bool F32>
__global__ __launch_bounds__(256) void evidence_tail_bwd_dw_kernel(mmdeer_evidence_tail_args a, const float* devid, float* pw, float* pb) {
  __shared__ float xs[TAIL_ROWS][64];
  __shared__ float ds[TAIL_ROWS][32];
  const int g = blockIdx.y, p = blockIdx.z, P = gridDim.z, K = a.K, O = a.O, R = 4 * O, GO = a.G * O;
  const int k0 = blockIdx.x * 64;
  const int s = threadIdx.x >> 2, q = threadIdx.x & 3;        // loader role: row s, 16 columns of x / 8 of devid
  const int kk = threadIdx.x & 63, rg = threadIdx.x >> 6;     // compute role: column kk, rows [8 rg, 8 rg + 8) (uniform per wave)
  const int nblk = (a.B + TAIL_ROWS - 1) / TAIL_ROWS;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float bacc = 0.f;
  for (int blk = p; blk < nblk; blk += P) {
    const int b = blk * TAIL_ROWS + s;
    const bool live = b < a.B;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = 16 * q + 8 * h;
      float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (live && k0 + c < K) ld8<F32>(a.x, (long long)b * a.ld_x + (long long)g * K + k0 + c, x);
#pragma unroll
      for (int i = 0; i < 8; ++i) xs[s][c + i] = x[i];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = 8 * q + 4 * h;
      f32x4 d{0.f, 0.f, 0.f, 0.f};
      if (live && r < R) d = *reinterpret_cast<const f32x4*>(devid + 4 * ((long long)b * GO + (long long)g * O) + r);
      ds[s][r] = d.x; ds[s][r + 1] = d.y; ds[s][r + 2] = d.z; ds[s][r + 3] = d.w;
    }
    __syncthreads();
    if (8 * rg < R) {
      for (int i = 0; i < TAIL_ROWS; ++i) {
        const float xv = xs[i][kk];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(ds[i][8 * rg + j], xv, acc[j]);
      }
    }
    if (blockIdx.x == 0 && threadIdx.x < R)
      for (int i = 0; i < TAIL_ROWS; ++i) bacc += ds[i][threadIdx.x];
    __syncthreads();
  }
  if (k0 + kk < K) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (8 * rg + j < R) pw[(((long long)p * a.G + g) * R + 8 * rg + j) * K + k0 + kk] = acc[j];
  }
  if (blockIdx.x == 0 && threadIdx.x < R) pb[((long long)p * a.G + g) * R + threadIdx.x] = bacc;
}

// dw, db = sum over the P batch parts in index order.  Eight loads in flight per thread (index clamped, value masked to +0) before
// their eight ordered additions: a plain loop waits for each load in turn (15.6 us for 780 sums of 64 parts).
__global__ __launch_bounds__(256) void evidence_tail_bwd_fold_kernel(const float* pw, const float* pb, int P, long long nw, long long nb,
                                                                     float* dw, float* db) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + nb) return;
  const float* const src = i < nw ? pw + i : pb + (i - nw);
  const long long stride = i < nw ? nw : nb;
  float sum = 0.f;
  for (int p0 = 0; p0 < P; p0 += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(p0 + u < P ? p0 + u : P - 1) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += p0 + u < P ? v[u] : 0.f;
  }
  if (i < nw) dw[i] = sum;
  else db[i - nw] = sum;
}

int tail_parts(int B) {
  const int nblk = (B + TAIL_ROWS - 1) / TAIL_ROWS;
  return nblk < 1 ? 1 : (nblk > TAIL_MAX_PARTS ? TAIL_MAX_PARTS : nblk);
}

int check_shape(const char* op, int B, int G, int K, int O) {
  MMDEER_CHECK(B >= 0, "%s: B must be >= 0 (got %d)", op, B);
  MMDEER_CHECK(G >= 1 && G <= 8, "%s: G must be in [1, 8] (got %d)", op, G);
  MMDEER_CHECK(O >= 1 && O <= 8, "%s: O must be in [1, 8] (got %d)", op, O);
  MMDEER_CHECK(K >= 8 && K <= 512 && K % 8 == 0, "%s: K must be a multiple of 8 in [8, 512] (got %d)", op, K);
  return 0;
}

int check_tail(const mmdeer_evidence_tail_args* a, bool bwd) {
  const char* op = bwd ? "evidence_tail_bwd" : "evidence_tail_fwd";
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  if (check_shape(op, a->B, a->G, a->K, a->O) != 0) return -1;
  const int el = a->act_f32 ? 4 : 8;              // elements per 16 bytes
  MMDEER_CHECK(a->ld_x >= a->G * a->K && a->ld_x % el == 0, "%s: ld_x must be >= G * K = %d and a multiple of %d (got %d)", op,
               a->G * a->K, el, a->ld_x);
  MMDEER_CHECK(a->x && a->w, "%s: NULL pointer (x, w)", op);
  MMDEER_CHECK(al16(a->x), "%s: x must be 16-byte aligned", op);
  MMDEER_CHECK(al16(a->w), "%s: w must be 16-byte aligned", op);
  MMDEER_CHECK(a->evid && al16(a->evid), "%s: evid must be a 16-byte aligned pointer", op);
  if (!bwd) {
    MMDEER_CHECK(a->b && al16(a->b), "%s: b must be a 16-byte aligned pointer", op);
    MMDEER_CHECK(a->nig_out, "%s: NULL pointer (nig_out)", op);
  } else {
    MMDEER_CHECK(a->dw && a->db, "%s: NULL pointer (dw, db)", op);
    MMDEER_CHECK(a->scratch && al16(a->scratch), "%s: scratch must be a 16-byte aligned pointer", op);
    MMDEER_CHECK(!a->devid || al16(a->devid), "%s: devid must be 16-byte aligned", op);
    if (a->dx) {
      MMDEER_CHECK(a->ld_dx >= a->G * a->K && a->ld_dx % el == 0, "%s: ld_dx must be >= G * K = %d and a multiple of %d (got %d)", op,
                   a->G * a->K, el, a->ld_dx);
      MMDEER_CHECK(al16(a->dx), "%s: dx must be 16-byte aligned", op);
    }
  }
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

long long mmdeer_evidence_tail_scratch(int B, int G, int K, int O) {
  if (check_shape("evidence_tail_scratch", B, G, K, O) != 0) return -1;
  const long long R = 4 * O, P = tail_parts(B);
  return (long long)B * G * R + P * G * R * K + P * G * R;      // devid | weight partials | bias partials (all multiples of 4)
}

int mmdeer_evidence_tail_fwd(const mmdeer_evidence_tail_args* a) {
  if (check_tail(a, false) != 0) return -1;
  if (a->B == 0) return 0;
  const dim3 grid((unsigned)((a->B + TAIL_ROWS - 1) / TAIL_ROWS), (unsigned)a->G);
  const size_t lds = (size_t)4 * a->O * a->K * (a->act_f32 ? 4 : 2);
  MMDEER_LAUNCH_ACT_LDS(evidence_tail_fwd_kernel, a->act_f32, grid, dim3(256), lds, (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_evidence_tail_bwd(const mmdeer_evidence_tail_args* a) {
  if (check_tail(a, true) != 0) return -1;
  const hipStream_t s = (hipStream_t)a->stream;
  const int R = 4 * a->O;
  const long long nw = (long long)a->G * R * a->K, nb = (long long)a->G * R;
  if (a->B == 0) {
    MMDEER_HIP(hipMemsetAsync(a->dw, 0, sizeof(float) * nw, s));
    MMDEER_HIP(hipMemsetAsync(a->db, 0, sizeof(float) * nb, s));
    return 0;
  }
  const int P = tail_parts(a->B);
  float* const devid = a->devid ? a->devid : a->scratch;
  float* const pw = a->scratch + (long long)a->B * nb;
  float* const pb = pw + (long long)P * nw;
  const dim3 grid((unsigned)((a->B + TAIL_ROWS - 1) / TAIL_ROWS), (unsigned)a->G);
  const int cols = a->K < TAIL_PANEL ? a->K : TAIL_PANEL;
  const size_t lds = (size_t)((TAIL_ROWS * (R + 1) * 4 + 15) & ~15) + (size_t)R * cols * (a->act_f32 ? 4 : 2);
  MMDEER_LAUNCH_ACT_LDS(evidence_tail_bwd_dx_kernel, a->act_f32, grid, dim3(256), lds, s, *a, devid);
  const dim3 gw((unsigned)((a->K + 63) / 64), (unsigned)a->G, (unsigned)P);
  MMDEER_LAUNCH_ACT(evidence_tail_bwd_dw_kernel, a->act_f32, gw, dim3(256), s, *a, (const float*)devid, pw, pb);
  hipLaunchKernelGGL(evidence_tail_bwd_fold_kernel, dim3((unsigned)((nw + nb + 255) / 256)), dim3(256), 0, s, (const float*)pw,
                     (const float*)pb, P, nw, nb, a->dw, a->db);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
