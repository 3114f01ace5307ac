// Stride-2 convolutions of the frame video encoder's backbone (reference src/models/encoders.py:418-440): nn.Conv2d(3, 64, 7, 2, 3)
// and nn.Conv2d(C, 2 C, 3, 2, 1) on channels-last activations as ONE implicit-GEMM launch each, forward only.
//
// The input lives in a padded channels-last buffer [N][Hp][Wp][Cp] with a zero border (include/mmdeer_frames.h), so tap row kh of
// output row m = (n * OH + oh) * OW + ow is KWe * Cp contiguous elements at ((n * Hp + 2 oh + kh) * Wp + 2 ow) * Cp: per tap row an
// ordinary [M][K] x [Cout][K]^T product whose A rows are gathered.  The kernel is the register-staged tile body of
// gemm_kernel.inc, as conv_time.hip's: k passes of k_loop into the same accumulators -- pass kh with its A origin moved by one
// padded image row (Wp * Cp elements) and its own [Cout][K] slice of the weight image -- then one gemm_epilogue (bias, dense store).
// The one new piece is the row origin: k_loop's gathered form (RowGather) takes this thread's four origins, computed once per
// workgroup from (n, oh, ow), in place of row * lda, in the fast loader and in the generic one alike.
//
// What is read.  A stored row m < M reads, in pass kh, the elements [origin + kh Wp Cp, + K).  2 (OH - 1) + k <= Hp and
// 2 (OW - 1) + k <= Wp, so with K = k Cp (the 3 x 3 layers) that is inside the buffer.  The 7 x 7 layer reads KWe = 8 pixels per tap
// row so that a tap row is one whole K-tile: the eighth meets zero weights and is the next pixel of the buffer -- border or data,
// finite -- or, behind the last pixel of the last frame, the slack pixel the buffer carries for exactly this.  Rows >= M read the
// buffer's first row through a clamped pointer (gemm_kernel.inc), and are never stored.
//
// The descriptor is a one-problem GemmGroup (M = N OH OW, N = Cout, K = KWe Cp, batch 1, no split); its batch stride sB, unused by a
// batch of one, carries the tap stride of the image.
#include "../../include/mmdeer_frames.h"
#include "conv2d_geom.h"   // ConvGeom, conv_geom (shared with conv2d_bwd.hip)
#include "elem.h"
#include "gemm_kernel.inc"
#include "options.h"

namespace mmdeer {
namespace {

template <typename CT, int BM, int BN>
__global__ __launch_bounds__(256, (BM * BN <= 64 * 64) ? 3 : 2) void conv2d_s2_kernel(const GemmGroup g, const ConvGeom cg) {
  constexpr int KT = Elem<CT>::KT;
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int A_BYTES = BM * LDS_ROW, B_BYTES = BN * LDS_ROW, STAGE = A_BYTES + B_BYTES;
  constexpr int SPAD = BN + 4;
  constexpr int LDS_BYTES = cmax(2 * STAGE, BM * SPAD * 4);
  constexpr int MODE = sizeof(CT) == 4 ? SRC_F32 : SRC_BF16_V16;
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

  int bid = blockIdx.x;
  if (g.xcd_remap) bid = xcd_contiguous(bid, gridDim.x);
  TileAt at;
  const __attribute__((address_space(4))) GemmProblem& p = *locate_tile(g, bid, 0, at);
  const int row0 = at.tmb * BM, col0 = at.tnb * BN;

  // this thread's A rows: (tid >> 3) + 32 j of the tile; a row beyond M keeps origin 0 and is never read through it
  const int per = cg.OH * cg.OW;
  auto origin = [&](int j) __attribute__((always_inline)) -> long long {
    const int m = row0 + (threadIdx.x >> 3) + 32 * j;
    if (m >= p.M) return 0;
    const int n = m / per, r = m - n * per, oh = r / cg.OW, ow = r - oh * cg.OW;
    return (((long long)n * cg.Hp + 2 * oh) * cg.Wp + 2 * ow) * cg.Cp;
  };
  const RowGather rg{origin(0), origin(1), origin(2), origin(3)};

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) bsum[i] = 0.f;

  KArgs ka;
  ka.stamps = nullptr;
  ka.A = p.A; ka.B = p.B;
  ka.lda = 0; ka.ldb = p.ldb;
  ka.a_rows = p.M - row0; ka.b_rows = p.N - col0;
  ka.K = p.K; ka.kt0 = 0; ka.kt1 = (p.K + KT - 1) / KT; ka.do_bsum = false;
  const long long tap_a = (long long)cg.Wp * cg.Cp;
#pragma unroll 1
  for (int kh = 0; kh < cg.k; ++kh) {   // each pass ends with a barrier: the LDS stages are free for the next one
    ka.a_off = kh * tap_a;
    ka.b_off = (long long)col0 * p.ldb + kh * p.sB;
    k_loop<CT, BM, BN, false, false, MODE, MODE, TM, TN, true>(ka, lds, acc, bsum, rg);
  }
  gemm_epilogue<BM, BN>(g, p, lds, acc, 0, 0, row0, col0);
}

// one thread per padded pixel (and the slack pixel): a 16-byte store of (r, g, b, 0 ...) or of zeros
template <bool F32>
__global__ __launch_bounds__(256) void frames_pack_kernel(const float* f, int N, int H, int W, void* out) {
  const int Hp = H + 6, Wp = W + 6;
  const long long npix = (long long)N * Hp * Wp + 1, q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= npix) return;
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  const int wp = (int)(q % Wp), hp = (int)((q / Wp) % Hp);
  const long long n = q / ((long long)Wp * Hp);
  if (n < N && hp >= 3 && hp < H + 3 && wp >= 3 && wp < W + 3) {
    const long long plane = (long long)H * W, at = (n * 3 * H + (hp - 3)) * W + (wp - 3);
    v = f32x4{f[at], f[at + plane], f[at + 2 * plane], 0.f};
  }
  if constexpr (F32) st4<true>(out, q * 4, v);
  else st8<false>(out, q * 8, v, f32x4{0.f, 0.f, 0.f, 0.f});
}

// one thread per image element
template <bool F32>
__global__ __launch_bounds__(256) void conv2d_pack_kernel(const float* w, int Cout, int Cin, int k, int Cp, int KWe, void* image) {
  const int K = KWe * Cp;
  const long long total = (long long)k * Cout * K, e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int x = (int)(e % K), co = (int)((e / K) % Cout), kh = (int)(e / ((long long)K * Cout));
  const int kw = x / Cp, c = x - kw * Cp;
  st1<F32>(image, e, (kw < k && c < Cin) ? w[(((long long)co * Cin + c) * k + kh) * k + kw] : 0.f);
}

template <typename CT>
int launch_conv2d(const GemmGroup& g, const ConvGeom& cg, int BM, int total, hipStream_t s) {
  if (BM == 64) hipLaunchKernelGGL((conv2d_s2_kernel<CT, 64, 64>), dim3(total), dim3(256), 0, s, g, cg);
  else hipLaunchKernelGGL((conv2d_s2_kernel<CT, 128, 128>), dim3(total), dim3(256), 0, s, g, cg);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

constexpr long long LIMIT = 1ll << 31;   // elements of one buffer

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_frames_pack(const float* frames, int N, int H, int W, void* out, int act_f32, void* stream) {
  MMDEER_CHECK(N >= 0 && H >= 1 && W >= 1, "frames_pack: bad shape N=%d H=%d W=%d", N, H, W);
  const long long npix = (long long)N * (H + 6) * (W + 6) + 1;
  MMDEER_CHECK(npix * (act_f32 ? 4 : 8) < LIMIT, "frames_pack: the padded buffer of %lld pixels has 2^31 elements or more", npix);
  if (N == 0) return 0;
  MMDEER_CHECK(frames && out, "frames_pack: NULL pointer (frames, out)");
  MMDEER_CHECK(al4(frames) && al16(out), "frames_pack: misaligned pointer (frames needs 4 bytes, out 16)");
  MMDEER_LAUNCH_ACT(frames_pack_kernel, act_f32, dim3((unsigned)((npix + 255) / 256)), dim3(256), (hipStream_t)stream, frames, N, H, W, out);
  return 0;
}

int mmdeer_conv2d_pack(const float* weight, int Cout, int Cin, int k, void* image, int act_f32, void* stream) {
  ConvGeom cg;
  int KWe;
  MMDEER_CHECK(conv_geom(1, 1, Cin, k, act_f32, cg, KWe), "conv2d_pack: unsupported kernel size / Cin (k=%d Cin=%d): 7 with Cin = 3, or 3 with Cin a multiple of %d",
               k, Cin, act_f32 ? 4 : 8);
  MMDEER_CHECK(Cout > 0 && Cout % 64 == 0, "conv2d_pack: unsupported Cout=%d (a multiple of 64)", Cout);
  MMDEER_CHECK(weight && image, "conv2d_pack: NULL pointer (weight, image)");
  MMDEER_CHECK(al4(weight) && al16(image), "conv2d_pack: misaligned pointer (weight needs 4 bytes, image 16)");
  const long long total = (long long)k * Cout * KWe * cg.Cp;
  MMDEER_CHECK(total < LIMIT, "conv2d_pack: the image has 2^31 elements or more");
  MMDEER_LAUNCH_ACT(conv2d_pack_kernel, act_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), (hipStream_t)stream, weight, Cout, Cin, k,
                    cg.Cp, KWe, image);
  return 0;
}

int mmdeer_conv2d_s2(const mmdeer_conv2d_args* a) {
  MMDEER_CHECK(a, "conv2d_s2: NULL argument struct");
  ConvGeom cg;
  int KWe;
  MMDEER_CHECK(a->N >= 0 && a->H >= 1 && a->W >= 1, "conv2d_s2: bad shape N=%d H=%d W=%d", a->N, a->H, a->W);
  MMDEER_CHECK(conv_geom(a->H, a->W, a->Cin, a->k, a->act_f32, cg, KWe),
               "conv2d_s2: unsupported kernel size / Cin (k=%d Cin=%d): 7 with Cin = 3, or 3 with Cin a multiple of %d", a->k, a->Cin, a->act_f32 ? 4 : 8);
  MMDEER_CHECK(a->Cout > 0 && a->Cout % 64 == 0, "conv2d_s2: unsupported Cout=%d (a multiple of 64)", a->Cout);
  MMDEER_CHECK(a->tile == -1 || a->tile == TILE_64x64 || a->tile == TILE_128x128, "conv2d_s2: tile must be -1, 0 or 2 (got %d)", a->tile);
  const long long M = (long long)a->N * cg.OH * cg.OW, in_elems = ((long long)a->N * cg.Hp * cg.Wp + (KWe - a->k)) * cg.Cp;
  MMDEER_CHECK(in_elems < LIMIT && M * a->Cout < LIMIT, "conv2d_s2: a buffer has 2^31 elements or more (input %lld, output %lld)", in_elems,
               M * a->Cout);
  if (a->N == 0) return 0;
  MMDEER_CHECK(a->x && a->w && a->y, "conv2d_s2: NULL pointer (x, w, y)");
  MMDEER_CHECK(al16(a->x) && al16(a->w) && al16(a->y) && al16(a->bias), "conv2d_s2: misaligned pointer (x, w, y, bias need 16 bytes)");
  GemmGroup g{};
  g.nprob = 1;
  g.xcd_remap = opt(OPT_XCD);   // as the GEMM kernels: each XCD owns a contiguous range of tiles
  g.drop = make_drop(0.f, 0, 0);
  GemmProblem& p = g.p[0];
  gemm_problem_defaults(p);
  p.A = a->x; p.B = a->w; p.C = a->y; p.bias = a->bias;
  p.M = (int)M; p.N = a->Cout; p.K = KWe * cg.Cp;
  p.lda = p.K; p.ldb = p.K; p.ldc = a->Cout;
  p.sB = (long long)a->Cout * p.K;   // tap stride of the image (see the head of this file)
  p.a_f32 = p.b_f32 = p.c_f32 = a->act_f32 ? 1 : 0;
  p.a_mode = p.b_mode = a->act_f32 ? SRC_F32 : SRC_BF16_V16;
  // 128 x 128 tiles once they give every CU a workgroup and the layer has the columns for them
  const bool big = a->tile == TILE_128x128 || (a->tile == -1 && a->Cout >= 128 && gemm_tiles(p.M, p.N, 128, 128) >= 256);
  const int BM = big ? 128 : 64;
  p.tiles_m = ceil_div(p.M, BM); p.tiles_n = ceil_div(p.N, BM);
  const int total = p.tiles_m * p.tiles_n;
  g.tile_start[0] = 0;
  for (int j = 1; j <= GEMM_MAX_PROBLEMS; ++j) g.tile_start[j] = total;
  return a->act_f32 ? launch_conv2d<float>(g, cg, BM, total, (hipStream_t)a->stream) : launch_conv2d<bf16_t>(g, cg, BM, total, (hipStream_t)a->stream);
}

}  // extern "C"
