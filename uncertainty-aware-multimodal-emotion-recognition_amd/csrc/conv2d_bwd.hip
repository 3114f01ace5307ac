// The backward of the frame video encoder's stride-2 convolutions (include/mmdeer_frames_bwd.h): the weight gradient and the input
// gradient of conv2d.hip's forward, on the same buffers -- the padded channels-last input [N][Hp][Wp][Cp] and the dense rows
// [M = N OH OW][Cout] -- as implicit GEMMs on the register-staged tile body of gemm_kernel.inc.
//
// Weight gradient.  Per tap row kh:  dW_kh [Cout][KWe Cp] = dy^T [Cout][M] x X_kh [M][KWe Cp], where row m of X_kh is the KWe Cp
// contiguous elements at origin(m) + kh Wp Cp of the padded buffer: the transposed-transposed product of gemm_kernel.inc
// (TA = TB = true: both operands are stored [reduction][row]) whose B rows are gathered.  The loader is the transposed tile loader
// with one change: a thread's four reduction rows m .. m + 3 of B start at their own origins, which it forms from (n, oh, ow) of m
// once per K-tile and steps with carries.  As in that body the loads are straight-line, nothing is computed on a loaded register
// before the LDS store, and a reduction row beyond M reads a clamped address; only the one ragged K-tile at the end of the
// reduction masks its registers (both operands: a clamped read may hold anything).  The reduction is cut into slices of whole
// K-tiles, one workgroup per (tile, slice); every workgroup stores its fp32 partial tile to the caller's scratch, and a second
// launch adds the slices in index order and writes [Cout][Cin][k][k], dropping the image's padding lanes.  The bias gradient, the
// row sums of dy^T, comes out of the A fragments of the tiles at (kh = 0, first column tile), as in gemm_group_kernel.
//
// Input gradient (3 x 3).  dx at (h, w) sums dy at ((h + 1 - kh) / 2, (w + 1 - kw) / 2) over the taps of matching parity, so the
// positions fall into four parity classes with 4 / 2 / 2 / 1 taps.  A class is the forward's kernel with the roles turned round:
// one k_loop pass per tap into the same accumulators, A rows gathered out of dy (a tap outside the image reads the zero row behind
// dy), B the tap's [Cin][Cout] slice of the transposed image, and an epilogue that scatters the class's rows to their positions in
// dx.  The class is blockIdx.y; a class with fewer row tiles than the largest lets the surplus workgroups return.
#include "../../include/mmdeer_frames_bwd.h"
#include "conv2d_geom.h"
#include "elem.h"
#include "gemm_kernel.inc"

namespace mmdeer {
namespace {

constexpr int WG_BM = 64, WG_BN = 64;   // output tile of both kernels

struct WgradArgs {
  const void* dy;
  const void* x;
  float* slab;            // [slices][Cout][k * KC]
  float* slab_b;          // [slices][Cout]
  long long slab_stride;  // Cout * k * KC
  int M, Cout, KC, tiles_m, tiles_n, slices, nkt, nk_per, want_bias;
  ConvGeom cg;
};

template <typename CT>
__global__ __launch_bounds__(256, 3) void conv2d_wgrad_kernel(const WgradArgs a) {
  constexpr int BM = WG_BM, BN = WG_BN, KT = Elem<CT>::KT, EPC = Elem<CT>::EPC;
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int A_BYTES = BM * LDS_ROW, B_BYTES = BN * LDS_ROW, STAGE = A_BYTES + B_BYTES;
  constexpr int SPAD = BN + 4;
  constexpr int LDS_BYTES = cmax(2 * STAGE, BM * SPAD * 4);
  constexpr int QN = KT / 4, UNITS = QN * (BM / EPC);
  static_assert(BM == BN && UNITS <= 256, "one loader geometry for both operands");
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;
  const ConvGeom cg = a.cg;

  int bid = blockIdx.x;
  const int tnb = bid % a.tiles_n; bid /= a.tiles_n;
  const int kh = bid % cg.k; bid /= cg.k;
  const int tmb = bid % a.tiles_m, slice = bid / a.tiles_m;
  const int row0 = tmb * BM, col0 = tnb * BN;
  const int kt0 = slice * a.nk_per, kt1 = min(kt0 + a.nk_per, a.nkt);
  const int M = a.M, Cout = a.Cout, per = cg.OH * cg.OW;

  // the transposed loader's coordinates: four consecutive reduction rows 4 q .. 4 q + 3 of the K-tile x EPC consecutive tile rows
  // from c0.  Threads beyond UNITS, and B columns beyond KC, load the operand's first chunk and never store / are never stored.
  const int q = tid % QN, c0 = (tid / QN) * EPC;
  const bool a_ok = tid < UNITS, b_ok = tid < UNITS && col0 + c0 < a.KC;
  const CT* A = reinterpret_cast<const CT*>(a.dy);
  const CT* X = reinterpret_cast<const CT*>(a.x);
  const long long a_col = row0 + c0, x_off = (long long)kh * cg.Wp * cg.Cp + col0 + c0;

  RTile ra, rb;
  auto gload = [&](int kt) __attribute__((always_inline)) {
    const int m0 = kt * KT + 4 * q, mm = min(m0, M - 1);
    int n = mm / per;
    const int r = mm - n * per;
    int oh = r / cg.OW, ow = r - oh * cg.OW;
    auto one = [&](int j, u32x4& va, u32x4& vb) __attribute__((always_inline)) {
      const bool ok = m0 + j < M;
      const long long org = (((long long)n * cg.Hp + 2 * oh) * cg.Wp + 2 * ow) * cg.Cp;
      const CT* pa = (a_ok && ok) ? A + (long long)(m0 + j) * Cout + a_col : A;
      const CT* pb = (b_ok && ok) ? X + org + x_off : X;
      va = *reinterpret_cast<const u32x4*>(pa);
      vb = *reinterpret_cast<const u32x4*>(pb);
      if (++ow == cg.OW) {
        ow = 0;
        if (++oh == cg.OH) { oh = 0; ++n; }
      }
    };
    one(0, ra.r0, rb.r0); one(1, ra.r1, rb.r1); one(2, ra.r2, rb.r2); one(3, ra.r3, rb.r3);
  };
  // the ragged last K-tile of the reduction: rows m >= M count as zero in both operands
  auto ktail = [&](int kt) __attribute__((always_inline)) {
    ra = tile_ktail_mask<CT, true>(ra, kt * KT, M, tid);
    rb = tile_ktail_mask<CT, true>(rb, kt * KT, M, tid);
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
    tile_lstore<CT, BM, true>(lds + buf * STAGE, ra, tid);
    tile_lstore<CT, BN, true>(lds + buf * STAGE + A_BYTES, rb, tid);
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) bsum[i] = 0.f;
  const bool do_bsum = a.want_bias && kh == 0 && tnb == 0 && wn == 0;

  auto compute = [&](int cur) __attribute__((always_inline)) {
    const unsigned char* la = lds + cur * STAGE + (wm * WTM + li) * LDS_ROW + lg * 16;
    const unsigned char* lb = lds + cur * STAGE + A_BYTES + (wn * WTN + li) * LDS_ROW + lg * 16;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u32x4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const u32x4*>(la + i * 16 * LDS_ROW + s * 64);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = *reinterpret_cast<const u32x4*>(lb + j * 16 * LDS_ROW + s * 64);
      if (do_bsum) {
#pragma unroll
        for (int i = 0; i < TM; ++i) bsum[i] += chunk_sum<CT>(fa[i]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma_chunk<CT>(fa[i], fb[j], acc[i][j]);
    }
  };

  // the K loop of gemm_kernel.inc: the loads of tile t + 1 are issued before the MFMAs of tile t and stored to the other LDS
  // buffer behind them; one barrier per K-tile.  An empty slice (more slices than K-tiles) stores a zero tile.
  if (kt0 < kt1) {
    gload(kt0);
    if (kt0 * KT + KT > M) ktail(kt0);
    lstore(0);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
      const int cur = (kt - kt0) & 1;
      const bool more = kt + 1 < kt1;
      if (more) gload(kt + 1);
      compute(cur);
      if (more) {
        if ((kt + 1) * KT + KT > M) ktail(kt + 1);
        lstore(cur ^ 1);
      }
      __syncthreads();
    }
  }

  if (do_bsum) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lg == 0) a.slab_b[(long long)slice * Cout + row0 + wm * WTM + i * 16 + li] = v;
    }
  }

  // accumulators -> fp32 staging in LDS (the loop ended with a barrier: the operand tiles are dead) -> 16-byte stores to the slab
  float* S = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(wm * WTM + i * 16 + lg * 4 + r) * SPAD + wn * WTN + j * 16 + li] = acc[i][j][r];
  __syncthreads();
  const int cc = tid % (BN / 4), gc = col0 + cc * 4;
  if (gc >= a.KC) return;
  float* out = a.slab + (long long)slice * a.slab_stride + (long long)kh * a.KC + gc;
  const long long ld = (long long)cg.k * a.KC;
#pragma unroll 4
  for (int row = tid / (BN / 4); row < BM; row += 256 / (BN / 4))
    *reinterpret_cast<f32x4*>(out + (row0 + row) * ld) = *reinterpret_cast<const f32x4*>(S + row * SPAD + cc * 4);
}

// one thread per element of dw (then of dbias): the slices in index order
__global__ __launch_bounds__(256) void conv2d_wgrad_fold_kernel(const WgradArgs a, int Cin, float* dw, float* dbias) {
  const int k = a.cg.k;
  const long long total = (long long)a.Cout * Cin * k * k, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e < total) {
    const int kw = (int)(e % k), kh = (int)((e / k) % k), c = (int)((e / (k * k)) % Cin), co = (int)(e / ((long long)k * k * Cin));
    const float* src = a.slab + ((long long)co * k + kh) * a.KC + kw * a.cg.Cp + c;
    float s = 0.f;
    for (int sl = 0; sl < a.slices; ++sl) s += src[sl * a.slab_stride];
    dw[e] = s;
  } else if (dbias && e - total < a.Cout) {
    const float* src = a.slab_b + (e - total);
    float s = 0.f;
    for (int sl = 0; sl < a.slices; ++sl) s += src[(long long)sl * a.Cout];
    dbias[e - total] = s;
  }
}

struct DgradArgs {
  const void* dy;
  const void* wt;
  void* dx;
  int N, H, W, Cin, Cout, OH, OW, M, tiles_n;
};

template <typename CT>
__global__ __launch_bounds__(256, 3) void conv2d_dgrad_kernel(const DgradArgs a) {
  constexpr int BM = WG_BM, BN = WG_BN;
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int A_BYTES = BM * LDS_ROW, B_BYTES = BN * LDS_ROW, STAGE = A_BYTES + B_BYTES;
  constexpr int SPAD = BN + 4;
  constexpr int LDS_BYTES = cmax(2 * STAGE, BM * SPAD * 4);
  constexpr int MODE = sizeof(CT) == 4 ? SRC_F32 : SRC_BF16_V16;
  constexpr bool F32 = sizeof(CT) == 4;
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

  // the class (ph, pw) holds the positions h = 2 i + ph, w = 2 j + pw: Ha x Wa of them per frame, in the order (n, i, j)
  const int ph = blockIdx.y >> 1, pw = blockIdx.y & 1;
  const int Ha = (a.H + 1 - ph) >> 1, Wa = (a.W + 1 - pw) >> 1, per = Ha * Wa, Mc = a.N * per;
  const int tmb = blockIdx.x / a.tiles_n, tnb = blockIdx.x - tmb * a.tiles_n;
  const int row0 = tmb * BM, col0 = tnb * BN;
  if (row0 >= Mc) return;   // the whole workgroup: this class has fewer row tiles than the largest

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;

  // this thread's two A rows (tid >> 3) + 32 j; a row beyond Mc keeps (0, ph, pw) and is never read through its origin
  int rn[2], rh[2], rw[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = row0 + (tid >> 3) + 32 * j;
    rn[j] = 0; rh[j] = ph; rw[j] = pw;
    if (m < Mc) {
      const int n = m / per, r = m - n * per, i = r / Wa;
      rn[j] = n; rh[j] = 2 * i + ph; rw[j] = 2 * (r - i * Wa) + pw;
    }
  }
  const long long zero_row = (long long)a.M * a.Cout;
  auto origin = [&](int j, int kh, int kw) __attribute__((always_inline)) -> long long {
    const int oh = (rh[j] + 1 - kh) >> 1, ow = (rw[j] + 1 - kw) >> 1;   // both differences are even and >= 0
    return (oh < a.OH && ow < a.OW) ? (((long long)rn[j] * a.OH + oh) * a.OW + ow) * a.Cout : zero_row;
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) bsum[i] = 0.f;

  constexpr int KT = Elem<CT>::KT;
  KArgs ka;
  ka.stamps = nullptr;
  ka.A = a.dy; ka.B = a.wt;
  ka.a_off = 0; ka.lda = 0; ka.ldb = a.Cout;
  ka.a_rows = Mc - row0; ka.b_rows = a.Cin - col0;
  ka.K = a.Cout; ka.kt0 = 0; ka.kt1 = a.Cout / KT; ka.do_bsum = false;
  // an even position takes tap 1, an odd one taps 0 and 2
#pragma unroll 1
  for (int kh = ph ? 0 : 1; kh < 3; kh += 2) {
#pragma unroll 1
    for (int kw = pw ? 0 : 1; kw < 3; kw += 2) {   // each pass ends with a barrier: the LDS stages are free for the next one
      const RowGather rg{origin(0, kh, kw), origin(1, kh, kw), 0, 0};
      ka.b_off = ((long long)(kh * 3 + kw) * a.Cin + col0) * a.Cout;
      k_loop<CT, BM, BN, false, false, MODE, MODE, TM, TN, true>(ka, lds, acc, bsum, rg);
    }
  }

  // accumulators -> fp32 staging -> one thread per four channels scatters the class's rows to their positions in dx
  float* S = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(wm * WTM + i * 16 + lg * 4 + r) * SPAD + wn * WTN + j * 16 + li] = acc[i][j][r];
  __syncthreads();
  const int cc = tid % (BN / 4), gc = col0 + cc * 4;
  if (gc >= a.Cin) return;
  for (int row = tid / (BN / 4); row < BM; row += 256 / (BN / 4)) {
    const int m = row0 + row;
    if (m >= Mc) break;
    const int n = m / per, r = m - n * per, i = r / Wa, h = 2 * i + ph, w = 2 * (r - i * Wa) + pw;
    st4<F32>(a.dx, (((long long)n * a.H + h) * a.W + w) * a.Cin + gc, *reinterpret_cast<const f32x4*>(S + row * SPAD + cc * 4));
  }
}

// one thread per image element
template <bool F32>
__global__ __launch_bounds__(256) void conv2d_pack_t_kernel(const float* w, int Cout, int Cin, void* image) {
  const long long total = 9ll * Cin * Cout, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int co = (int)(e % Cout), c = (int)((e / Cout) % Cin), tap = (int)(e / ((long long)Cout * Cin));
  st1<F32>(image, e, w[((long long)co * Cin + c) * 9 + tap]);
}

constexpr long long LIMIT = 1ll << 31;   // elements of one buffer

// the checks of the shape and the plan of the weight gradient; the scratch query and the call share them
int wgrad_plan(const mmdeer_conv2d_wgrad_args* a, const char* op, WgradArgs& w, int& KWe, long long& need) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "%s: bad shape N=%d H=%d W=%d", op, a->N, a->H, a->W);
  MMDEER_CHECK(conv_geom(a->H, a->W, a->Cin, a->k, a->act_f32, w.cg, KWe),
               "%s: unsupported kernel size / Cin (k=%d Cin=%d): 7 with Cin = 3, or 3 with Cin a multiple of %d", op, a->k, a->Cin, a->act_f32 ? 4 : 8);
  MMDEER_CHECK(a->Cout > 0 && a->Cout % 64 == 0, "%s: unsupported Cout=%d (a multiple of 64)", op, a->Cout);
  MMDEER_CHECK(a->slices == -1 || (a->slices >= 1 && a->slices <= MMDEER_CONV2D_WGRAD_MAX_SLICES), "%s: slices must be -1 or 1 .. %d (got %d)", op,
               MMDEER_CONV2D_WGRAD_MAX_SLICES, a->slices);
  const long long M = (long long)a->N * w.cg.OH * w.cg.OW, in_elems = ((long long)a->N * w.cg.Hp * w.cg.Wp + (KWe - a->k)) * w.cg.Cp;
  MMDEER_CHECK(in_elems < LIMIT && M * a->Cout < LIMIT, "%s: a buffer has 2^31 elements or more (input %lld, dy %lld)", op, in_elems, M * a->Cout);
  const int KT = a->act_f32 ? 32 : 64;
  w.M = (int)M; w.Cout = a->Cout; w.KC = KWe * w.cg.Cp;
  w.tiles_m = a->Cout / WG_BM; w.tiles_n = ceil_div(w.KC, WG_BN);
  w.nkt = ceil_div(w.M, KT);
  const int tiles = w.tiles_m * w.tiles_n * a->k;
  int slices = a->slices;
  if (slices == -1) {   // two workgroups for each of 256 CUs, as far as the reduction has K-tiles for them
    slices = ceil_div(512, tiles);
    if (slices > w.nkt) slices = w.nkt;
    if (slices > MMDEER_CONV2D_WGRAD_MAX_SLICES) slices = MMDEER_CONV2D_WGRAD_MAX_SLICES;
    if (slices < 1) slices = 1;
  }
  w.slices = slices;
  w.nk_per = w.nkt ? ceil_div(w.nkt, slices) : 0;
  w.slab_stride = (long long)a->Cout * a->k * w.KC;
  need = (long long)slices * (w.slab_stride + a->Cout);
  MMDEER_CHECK(need < LIMIT, "%s: the scratch has 2^31 elements or more (%lld)", op, need);
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

long long mmdeer_conv2d_wgrad_scratch(const mmdeer_conv2d_wgrad_args* a) {
  WgradArgs w{};
  int KWe;
  long long need;
  if (wgrad_plan(a, "conv2d_wgrad_scratch", w, KWe, need) != 0) return -1;
  return need;
}

int mmdeer_conv2d_wgrad(const mmdeer_conv2d_wgrad_args* a) {
  WgradArgs w{};
  int KWe;
  long long need;
  TRY(wgrad_plan(a, "conv2d_wgrad", w, KWe, need));
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->x && a->dy && a->dw && a->scratch, "conv2d_wgrad: NULL pointer (x, dy, dw, scratch)");
  MMDEER_CHECK(al16(a->x) && al16(a->dy) && al16(a->dw) && al16(a->dbias) && al16(a->scratch),
               "conv2d_wgrad: misaligned pointer (x, dy, dw, dbias, scratch need 16 bytes)");
  MMDEER_CHECK(a->scratch_elems >= need, "conv2d_wgrad: scratch too short (%lld elements, %lld needed: mmdeer_conv2d_wgrad_scratch)", a->scratch_elems, need);
  w.dy = a->dy; w.x = a->x;
  w.slab = a->scratch; w.slab_b = a->scratch + (long long)w.slices * w.slab_stride;
  w.want_bias = a->dbias != nullptr;
  hipStream_t s = (hipStream_t)a->stream;
  const dim3 grid((unsigned)(w.tiles_m * w.tiles_n * a->k * w.slices));
  if (a->act_f32) hipLaunchKernelGGL(conv2d_wgrad_kernel<float>, grid, dim3(256), 0, s, w);
  else hipLaunchKernelGGL(conv2d_wgrad_kernel<bf16_t>, grid, dim3(256), 0, s, w);
  const long long total = (long long)a->Cout * a->Cin * a->k * a->k + a->Cout;
  hipLaunchKernelGGL(conv2d_wgrad_fold_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, a->Cin, a->dw, a->dbias);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_conv2d_pack_t(const float* weight, int Cout, int Cin, int k, void* image, int act_f32, void* stream) {
  MMDEER_CHECK(k == 3 && Cin > 0 && Cin % (act_f32 ? 4 : 8) == 0, "conv2d_pack_t: unsupported kernel size / Cin (k=%d Cin=%d): 3 with Cin a multiple of %d", k,
               Cin, act_f32 ? 4 : 8);
  MMDEER_CHECK(Cout > 0 && Cout % 64 == 0, "conv2d_pack_t: unsupported Cout=%d (a multiple of 64)", Cout);
  MMDEER_CHECK(weight && image, "conv2d_pack_t: NULL pointer (weight, image)");
  MMDEER_CHECK(al16(weight) && al16(image), "conv2d_pack_t: misaligned pointer (weight, image need 16 bytes)");
  const long long total = 9ll * Cin * Cout;
  MMDEER_CHECK(total < LIMIT, "conv2d_pack_t: the image has 2^31 elements or more");
  MMDEER_LAUNCH_ACT(conv2d_pack_t_kernel, act_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, weight, Cout, Cin, image);
  return 0;
}

int mmdeer_conv2d_dgrad(const mmdeer_conv2d_dgrad_args* a) {
  MMDEER_CHECK(a, "conv2d_dgrad: NULL argument struct");
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "conv2d_dgrad: bad shape N=%d H=%d W=%d", a->N, a->H, a->W);
  MMDEER_CHECK(a->k == 3 && a->Cin > 0 && a->Cin % (a->act_f32 ? 4 : 8) == 0,
               "conv2d_dgrad: unsupported kernel size / Cin (k=%d Cin=%d): 3 with Cin a multiple of %d; the 7 x 7 layer has no input gradient", a->k, a->Cin,
               a->act_f32 ? 4 : 8);
  MMDEER_CHECK(a->Cout > 0 && a->Cout % 64 == 0, "conv2d_dgrad: unsupported Cout=%d (a multiple of 64)", a->Cout);
  const int OH = (a->H - 1) / 2 + 1, OW = (a->W - 1) / 2 + 1;
  const long long M = (long long)a->N * OH * OW, dx_elems = (long long)a->N * a->H * a->W * a->Cin;
  MMDEER_CHECK((M + 1) * a->Cout < LIMIT && dx_elems < LIMIT, "conv2d_dgrad: a buffer has 2^31 elements or more (dy %lld, dx %lld)", (M + 1) * a->Cout, dx_elems);
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->dy && a->wt && a->dx, "conv2d_dgrad: NULL pointer (dy, wt, dx)");
  MMDEER_CHECK(al16(a->dy) && al16(a->wt) && al16(a->dx), "conv2d_dgrad: misaligned pointer (dy, wt, dx need 16 bytes)");
  DgradArgs d{};
  d.dy = a->dy; d.wt = a->wt; d.dx = a->dx;
  d.N = a->N; d.H = a->H; d.W = a->W; d.Cin = a->Cin; d.Cout = a->Cout; d.OH = OH; d.OW = OW; d.M = (int)M;
  d.tiles_n = ceil_div(a->Cin, WG_BN);
  // the even-even class is the largest: its row tiles bound every class's
  const int rows = a->N * ((a->H + 1) / 2) * ((a->W + 1) / 2);
  const dim3 grid((unsigned)(ceil_div(rows, WG_BM) * d.tiles_n), 4);
  hipStream_t s = (hipStream_t)a->stream;
  if (a->act_f32) hipLaunchKernelGGL(conv2d_dgrad_kernel<float>, grid, dim3(256), 0, s, d);
  else hipLaunchKernelGGL(conv2d_dgrad_kernel<bf16_t>, grid, dim3(256), 0, s, d);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
