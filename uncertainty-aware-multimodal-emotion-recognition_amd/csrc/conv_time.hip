// Convolution over time for the temporal video encoder (reference src/models/encoders.py:450-459): nn.Conv1d(512, 512, 3,
// padding = 1) on time-major rows (row t * B + b) as ONE implicit GEMM launch per pass.
//
// The input lives in a padded buffer of (T + 2) * B rows whose first and last B rows are zero, so tap j of output row r is padded
// row r + j * B for every r < T * B: three ordinary [M][512] x [512][512]^T products on row-shifted views of one matrix, summed.
// The kernel is the register-staged tile body of gemm_kernel.inc: three k_loop passes into the same accumulators -- pass j with
// its A origin moved by j * B rows and its own [N][C] slice of the weight image -- then one gemm_epilogue (bias, store).  Against
// three accumulating mmdeer_gemm calls that saves two launches and two read-modify-write passes over the output.
//
// The operand loader reads rows beyond a_rows through a clamped pointer (gemm_kernel.inc: FastLoader) -- garbage, harmless only
// for output rows that are never stored.  Here a_rows = T * B - row0 in every pass, so a stored row r reads exactly the padded rows
// r, r + B, r + 2 B < (T + 2) * B and nothing else: the time padding is in the buffer, the loader needs no masking.
//
// The descriptor is a one-problem GemmGroup (M = T * B, N = K = 512, batch 1, no split); its batch strides sA / sB, unused by a
// batch of one, carry the tap strides: B * ld_x elements of A and N * C elements of the image.
#include "../../include/mmdeer_video.h"
#include "gemm_kernel.inc"
#include "options.h"

namespace mmdeer {
namespace {

constexpr int CONV_W = 512;   // channels in and out

template <typename CT, int BM, int BN>
__global__ __launch_bounds__(256, (BM * BN <= 64 * 64) ? 3 : 2) void conv3_time_kernel(const GemmGroup g) {
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
  ka.lda = p.lda; ka.ldb = p.ldb;
  ka.a_rows = p.M - row0; ka.b_rows = p.N - col0;
  ka.K = p.K; ka.kt0 = 0; ka.kt1 = p.K / KT; ka.do_bsum = false;
#pragma unroll 1
  for (int tap = 0; tap < 3; ++tap) {   // each pass ends with a barrier: the LDS stages are free for the next one
    ka.a_off = (long long)row0 * p.lda + tap * p.sA;
    ka.b_off = (long long)col0 * p.ldb + tap * p.sB;
    k_loop<CT, BM, BN, false, false, MODE, MODE>(ka, lds, acc, bsum);
  }
  gemm_epilogue<BM, BN>(g, p, lds, acc, 0, 0, row0, col0);
}

// weight fp32 [N][C][3] -> image [3][N][C] and image_rev_t [3][C][N]: a 32 x 32 (n, c) tile through LDS, so that the reads (96
// contiguous floats per n) and both images' writes (along c, along n) are coalesced
template <bool F32>
__global__ __launch_bounds__(256) void conv3_time_pack_kernel(const float* w, int N, int C, void* image, void* image_rev_t) {
  __shared__ float t[32][97];
  const int n0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tid = threadIdx.x;
  for (int e = tid; e < 32 * 96; e += 256) {
    const int n = e / 96, k = e - n * 96;
    t[n][k] = w[((long long)(n0 + n) * C + c0) * 3 + k];
  }
  __syncthreads();
  for (int e = tid; e < 3 * 32 * 32; e += 256) {
    const int j = e >> 10, a = (e >> 5) & 31, b = e & 31;
    st1<F32>(image, ((long long)j * N + n0 + a) * C + c0 + b, t[a][b * 3 + j]);
    if (image_rev_t) st1<F32>(image_rev_t, ((long long)j * C + c0 + a) * N + n0 + b, t[b][a * 3 + 2 - j]);
  }
}

template <typename CT>
int launch_conv(const GemmGroup& g, int BM, int total, hipStream_t s) {
  if (BM == 64) hipLaunchKernelGGL((conv3_time_kernel<CT, 64, 64>), dim3(total), dim3(256), 0, s, g);
  else hipLaunchKernelGGL((conv3_time_kernel<CT, 128, 128>), dim3(total), dim3(256), 0, s, g);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_conv3_time_pack(const float* weight, int N, int C, void* image, void* image_rev_t, int act_f32, void* stream) {
  MMDEER_CHECK(N == CONV_W && C == CONV_W, "conv3_time_pack: C and N must be %d (got C=%d N=%d)", CONV_W, C, N);
  MMDEER_CHECK(weight && image, "conv3_time_pack: NULL pointer (weight, image)");
  MMDEER_LAUNCH_ACT(conv3_time_pack_kernel, act_f32, dim3(C / 32, N / 32), dim3(256), (hipStream_t)stream, weight, N, C, image, image_rev_t);
  return 0;
}

int mmdeer_conv3_time(const mmdeer_conv3_time_args* a) {
  MMDEER_CHECK(a, "conv3_time: NULL argument struct");
  MMDEER_CHECK(a->C == CONV_W && a->N == CONV_W, "conv3_time: C and N must be %d (got C=%d N=%d)", CONV_W, a->C, a->N);
  MMDEER_CHECK(a->T >= 0 && a->B >= 0, "conv3_time: bad shape T=%d B=%d", a->T, a->B);
  MMDEER_CHECK(a->tile == -1 || a->tile == TILE_64x64 || a->tile == TILE_128x128, "conv3_time: tile must be -1, 0 or 2 (got %d)", a->tile);
  MMDEER_CHECK(((long long)a->T + 2) * a->B < (1ll << 31) / CONV_W, "conv3_time: (T + 2) * B = %lld rows is too many",
               ((long long)a->T + 2) * a->B);
  if (a->T == 0 || a->B == 0) return 0;
  const int el = a->act_f32 ? 4 : 8;
  MMDEER_CHECK(a->x && a->w && a->y, "conv3_time: NULL pointer (x, w, y)");
  MMDEER_CHECK(a->ld_x >= a->C && a->ld_y >= a->N, "conv3_time: leading dimensions too small (ld_x=%d ld_y=%d)", a->ld_x, a->ld_y);
  MMDEER_CHECK(al16(a->x) && al16(a->w) && al16(a->y) && al16(a->bias) && a->ld_x % el == 0 && a->ld_y % el == 0,
               "conv3_time: misaligned pointer or leading dimension (x, w, y, bias need 16 bytes)");
  GemmGroup g{};
  g.nprob = 1;
  g.xcd_remap = opt(OPT_XCD);   // as the GEMM kernels: each XCD owns a contiguous range of tiles
  g.drop = make_drop(0.f, 0, 0);
  GemmProblem& p = g.p[0];
  gemm_problem_defaults(p);
  p.A = a->x; p.B = a->w; p.C = a->y; p.bias = a->bias;
  p.M = a->T * a->B; p.N = a->N; p.K = a->C;
  p.lda = a->ld_x; p.ldb = a->C; p.ldc = a->ld_y;
  p.sA = (long long)a->B * a->ld_x;   // tap strides (see the head of this file)
  p.sB = (long long)a->N * a->C;
  p.a_f32 = p.b_f32 = p.c_f32 = a->act_f32 ? 1 : 0;
  p.a_mode = p.b_mode = a->act_f32 ? SRC_F32 : SRC_BF16_V16;
  // 128 x 128 tiles once they give every CU a workgroup; below that the small tile spreads the rows over more of the chip
  const bool big = a->tile == TILE_128x128 || (a->tile == -1 && gemm_tiles(p.M, p.N, 128, 128) >= 256);
  const int BM = big ? 128 : 64;
  p.tiles_m = ceil_div(p.M, BM); p.tiles_n = ceil_div(p.N, BM);
  const int total = p.tiles_m * p.tiles_n;
  g.tile_start[0] = 0;
  for (int j = 1; j <= GEMM_MAX_PROBLEMS; ++j) g.tile_start[j] = total;
  return a->act_f32 ? launch_conv<float>(g, BM, total, (hipStream_t)a->stream) : launch_conv<bf16_t>(g, BM, total, (hipStream_t)a->stream);
}

}  // extern "C"
