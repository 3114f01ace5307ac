// Grouped MFMA GEMM: C = epilogue(A * B^T) for a list of independent problems in ONE launch.
#pragma once
#include "common.h"

namespace mmdeer {

// One problem:  C[M,N] (+)= op(A)[M,K] * op(B)[N,K]^T, strided-batched over `batch`.
//   trans_a == 0 : A stored [M][K]  (K contiguous, leading dim lda)
//   trans_a == 1 : A stored [K][M]  (M contiguous, leading dim lda)   -- the loader transposes 4xEPC blocks in registers
//   trans_b      : same for B ([N][K] vs [K][N]).
// This one kernel therefore serves  Y = X W^T (0,0),  dX = dY W (0,1: W is [N_layer][K_layer]) and
// dW = dY^T X (1,1) without any transposed copy in HBM.  All problems of one launch share (trans_a, trans_b).
//
// split-K (splitk > 1, weight-gradient problems): slice s reduces K-tiles [s*ceil(nk/S), ...) and writes its
// partial tile (and partial bias gradient) with plain stores to  slab + s*slab_stride + (offset of the final
// destination inside the flat gradient buffer); launch_reduce_partials() folds the S slices, or the tile's last-arriving
// slice does inside the launch (GemmFold below).  The sums are never atomic: the result is deterministic either way.
struct GemmProblem {
  const void* A;
  const void* B;
  void* C;
  const float* bias;    // [N] added before activation, or null
  float* bias_grad;     // dW problems: [M] row sums of op(A) over K (== column sums of dY), or null
  const void* Y;        // epilogue mask source: C *= (Y > 0) * mask_scale, or null   (ReLU+dropout backward)
  float* slab_c;        // split-K: where slice 0 of C goes (same z-strides / ldc as C); null when splitk == 1
  float* slab_b;        // split-K: where slice 0 of bias_grad goes
  long long sA, sB, sC, sBias, sBiasGrad, sY;  // batch strides, in elements
  long long slab_stride;                      // elements between consecutive K-slices
  int M, N, K, batch;
  int lda, ldb, ldc, ldy;
  int tiles_m, tiles_n;   // filled by the launcher
  int splitk;             // >= 1
  float mask_scale;
  int drop_site;        // forward dropout site (after ReLU), -1 = none
  int drop_shift;       // dropout granularity: one decision per 2^shift columns
  int regen_site;       // multiply by the REGENERATED keep mask of this site (backward of a no-ReLU dropout), -1 = none
  unsigned char a_f32, b_f32, c_f32, y_f32;   // storage dtypes (1 = fp32, 0 = bf16)
  unsigned char trans_a, trans_b, relu, accumulate;
  unsigned char a_mode, b_mode;               // loader mode, filled by the launcher (SrcMode)
  unsigned char pad_[2];
};

static_assert(sizeof(GemmProblem) == 192, "warm_descriptor (gemm_tile.h) touches the descriptor's cache lines by byte offset");

enum SrcMode { SRC_F32 = 0, SRC_BF16_V16 = 1, SRC_BF16_V8 = 2 };

constexpr int GEMM_MAX_PROBLEMS = 16;   // all weight-gradient problems of a backward pass fit one launch

// In-launch fold of the weight-gradient DMA kernel (gemm_tt256.hip), all zero = off: the launch leaves nothing for
// launch_reduce_partials.  With `cnt`, the workgroups of a split-K tile count their arrivals in one word per tile and the last
// arriver adds the slices (rowops.h: the fold's order) and writes the final tile and bias gradient; the words are ZERO before the
// launch and zero again when it ends (the last arriver resets its word), so they need no launch of their own.  The segments are
// row partials complete before the launch (ReduceTable's field meanings, rowops.h): `nseg` of them are folded by extra workgroups
// behind the tiles, two 256-element blocks each.  `bump`: as ReduceTable's.
constexpr int GEMM_FOLD_SEGMENTS = 8;
constexpr int GEMM_FOLD_SLICES = 8;         // most K-slices a counted tile may have
struct GemmFold {
  unsigned* cnt;
  int cnt_n;                                // words at cnt: the launch is refused when it has more workgroups
  int nseg;
  unsigned long long* bump;
  const float* src[GEMM_FOLD_SEGMENTS];
  float* dst[GEMM_FOLD_SEGMENTS];
  long long stride[GEMM_FOLD_SEGMENTS];
  int nparts[GEMM_FOLD_SEGMENTS];
  int n[GEMM_FOLD_SEGMENTS];
  int bstart[GEMM_FOLD_SEGMENTS + 1];       // filled by the launcher
};

struct GemmGroup {
  unsigned long long* stamps;   // diagnostic builds (-DMMDEER_STAMPS) only: s_memtime samples of workgroup 0; else null
  int nprob;
  int xcd_remap;   // 1: renumber workgroups so that each XCD (blockIdx % 8) owns a contiguous range of tiles
  int tile_start[GEMM_MAX_PROBLEMS + 1];
  DropCtx drop;
  GemmProblem p[GEMM_MAX_PROBLEMS];
  GemmFold fold;   // (behind p: the preloaded-form kernels and locate_tile address what lies in front by offset)
};
static_assert(sizeof(GemmGroup) + 64 + 256 <= 4096, "the kernel-argument segment (leading scalars of the preloaded form, hidden arguments) stays under 4 KiB");

enum GemmTile { TILE_64x64 = 0, TILE_128x64 = 1, TILE_128x128 = 2, TILE_256x256 = 3, TILE_256x128 = 4 };   // 256x256: bf16 LDS-DMA kernels only; 256x128: bf16 weight gradients only

// compute_f32 = 1: fp32 operands in LDS, v_mfma_f32_16x16x4_f32 (exact fp32); 0: bf16 operands, v_mfma_f32_16x16x32_bf16.
// prepare_gemm_group: every argument check, the clamp of splitk and the source mode of every operand (a_mode / b_mode).
// launch_gemm_group: prepare, then one launch per distinct (a_mode, b_mode) pair of the group -- a pair that no kernel instantiates
// is refused for every problem before the first launch.  Enqueues on `stream`, never synchronises.  Returns 0 / -1 (message via
// mmdeer_last_error()).  describe_gemm_group walks the group the same way and writes one line per launch into out[cap] instead of
// launching ("<kernel> <BM>x<BN>[ <variant>] a=<mode> b=<mode> tiles=<total>", lines separated by '\n'); returns the launch count.
int prepare_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile);
int launch_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile, hipStream_t stream);
int describe_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile, char* out, int cap);

// Whether the whole group runs as ONE launch of kernel `k` (prepare and route on a copy: nothing is launched, nothing written).
bool gemm_group_single_launch(const GemmGroup& g, int compute_f32, GemmTile tile, int k);

// The kernel one launch runs: a pure function (gemm.hip: gemm_route) of a homogeneous sub-group (one (a_mode, b_mode) pair), the compute
// dtype, the requested tile and the options.  `variant`: waves per workgroup of the LDS-DMA NT kernel (4 / 8; the ring depth follows from
// tile and waves, gemm_glds.hip), KG of the weight-gradient DMA kernel (1 / 2), 0 for the others.
enum GemmKernel { GEMM_NT_REG = 0, GEMM_NX_REG, GEMM_TT_REG, GEMM_NT_GLDS, GEMM_NT256, GEMM_TT_DMA, GEMM_KERNEL_COUNT };
struct GemmRoute { GemmKernel kernel; int BM, BN, variant; };
GemmRoute gemm_route(const GemmGroup& sub, int compute_f32, GemmTile tile);

// One launcher per GemmKernel (gemm_nt / _nx / _tt / _glds / _nt256 / _tt256.hip), looked up by route.kernel in gemm.hip.  `total` =
// workgroups; the caller has filled tiles_m / tiles_n / tile_start for (r.BM, r.BN) and guarantees what the kernel's predicate
// (gemm.hip) states.
typedef int GemmLauncher(const GemmGroup& g, int total, const GemmRoute& r, int compute_f32, hipStream_t s);
GemmLauncher gemm_launch_nt_reg, gemm_launch_nx_reg, gemm_launch_tt_reg, gemm_launch_nt_glds, gemm_launch_nt256, gemm_launch_tt_dma;

// The bf16-compute (A mode, B mode) pairs the register-staged kernels instantiate, per transposition (fp32 compute: (F32, F32) only).
// gemm_modes_instantiated (gemm.hip) and the three dispatchers (GEMM_REG_LAUNCHER, gemm_kernel.inc) expand these lists.
#define GEMM_MODE_PAIRS_NT(X) X(SRC_BF16_V16, SRC_BF16_V16) X(SRC_F32, SRC_BF16_V16) X(SRC_F32, SRC_BF16_V8) X(SRC_BF16_V8, SRC_BF16_V8)
#define GEMM_MODE_PAIRS_NX(X) X(SRC_BF16_V16, SRC_BF16_V16) X(SRC_BF16_V16, SRC_BF16_V8)
#define GEMM_MODE_PAIRS_TT(X) X(SRC_BF16_V16, SRC_BF16_V16) X(SRC_BF16_V16, SRC_F32) X(SRC_BF16_V16, SRC_BF16_V8)

void gemm_problem_defaults(GemmProblem& p);

// gemm_ln.hip: C = epilogue(LayerNorm(Y) W^T + bias) in one launch (bf16, K = LayerNorm width in {256, 512}); `g` holds the
// one GEMM problem (A ignored); the normalised rows, mean and rstd (and an optional fp32 copy) are written for the backward.
int launch_gemm_ln(GemmGroup& g, const void* Y, const float* gamma, const float* beta, void* xln, float* out32, float* mean,
                   float* rstd, hipStream_t s);

// tile policy of the executors (gemm.hip): option "tile" when set, else by tile count and operand layout
GemmTile pick_tile(const GemmGroup& g);
// target number of K-tiles per split-K slice of a weight-gradient problem (gemm.hip)
int ksteps_target(int compute_f32);

// tiles of one M x N matrix at tile size BM x BN (gemm.hip: group_tiles sums them over a group)
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline long long gemm_tiles(int M, int N, int BM, int BN) { return (long long)ceil_div(M, BM) * ceil_div(N, BN); }
// K-tile count of a problem for the given compute dtype (64 bf16 / 32 fp32 elements of K per tile)
inline int gemm_ktiles(int K, int compute_f32) { const int kt = compute_f32 ? 32 : 64; return (K + kt - 1) / kt; }

}  // namespace mmdeer
