// Host side of the grouped GEMM: validation, loader-mode selection, partition of a group by (A mode, B mode), the choice of the
// kernel each sub-group runs (gemm_route) and the walk that launches -- or only describes -- a group.
#include "gemm.h"
#include "options.h"

#include <cstdio>

namespace mmdeer {

// target number of K-tiles per split-K slice of a weight-gradient problem (option "ksteps" overrides)
// in units of 64 batch rows.  Defaults: bf16 (256x256 LDS-DMA kernel) 16 = 1024 rows per slice -- the slab
// traffic, 4 B per parameter per slice written and read back, is what limits the slice count; fp32 8.
int ksteps_target(int f32) {
  const int v = opt(OPT_KSTEPS);
  if (v > 0) return v;
  if (!f32 && opt(OPT_DW_TILE) == 4) return 32;   // 256x128: two K-slices at 4096 rows
  return f32 ? 8 : 16;
}

namespace {
const int TILE_BM[5] = {64, 128, 128, 256, 256}, TILE_BN[5] = {64, 64, 128, 256, 128};

// workgroups of a group at tile size BM x BN, split-K slices not counted
long long group_tiles(const GemmGroup& g, int BM, int BN) {
  long long t = 0;
  for (int i = 0; i < g.nprob; ++i) t += gemm_tiles(g.p[i].M, g.p[i].N, BM, BN) * g.p[i].batch;
  return t;
}

template <typename Pred>
bool every_problem(const GemmGroup& g, Pred pred) {
  for (int i = 0; i < g.nprob; ++i)
    if (!pred(g.p[i])) return false;
  return true;
}

// ---- what each LDS-DMA kernel takes, per problem.  All three also need bf16 compute, option glds and both operands in whole
// 16-byte chunks (a_mode = b_mode = SRC_BF16_V16): gemm_route checks that once per sub-group.
// Weight-gradient DMA kernel (gemm_tt256.hip; trans_a = trans_b = 1).  Used twice: by prepare_gemm_group BEFORE the source modes
// exist -- when the whole group meets it, a transposed operand may end in a half-valid chunk and still be read as V16 -- and by
// gemm_route per sub-group.  The storage conditions (bf16, ld and batch stride % 8) are what V16 itself requires, so they only
// decide anything in prepare; the output conditions matter in both (a half-valid chunk read by the register-staged fallback
// would be dropped).  splitk is compared with <= 1 because prepare asks before it has normalised a 0 to 1.
bool dw_dma_takes(const GemmProblem& q) {
  return !q.a_f32 && !q.b_f32 && q.lda % 8 == 0 && q.ldb % 8 == 0 && q.sA % 8 == 0 && q.sB % 8 == 0 &&
         q.K % 32 == 0 && q.c_f32 && !q.bias && !q.relu && !q.Y && q.drop_site < 0 && q.regen_site < 0 &&
         (uintptr_t)q.C % 16 == 0 && q.sC % 4 == 0 && (q.splitk <= 1 || ((uintptr_t)q.slab_c % 16 == 0 && q.slab_stride % 4 == 0));
}
// ... and the tile requests that ask for it: 256x256 and 256x128 tiles exist only there, 128x128 under option dw_tile = 2
bool dw_dma_requested(const GemmGroup& g, int compute_f32, GemmTile tile_req) {
  return g.p[0].trans_a && g.p[0].trans_b && !compute_f32 && opt(OPT_GLDS) &&
         (tile_req == TILE_256x256 || tile_req == TILE_256x128 || (tile_req == TILE_128x128 && opt(OPT_DW_TILE) == 2));
}
// 256-row forward kernel (gemm_nt256.hip; no transposition, tile 256x256 requested): bias / ReLU / dropout epilogue, no mask, no split-K
bool nt256_takes(const GemmProblem& q) {
  return q.K % 32 == 0 && q.splitk == 1 && !q.bias_grad && !q.Y && (uintptr_t)q.C % 16 == 0 && q.sC % 8 == 0 && q.ldc % 8 == 0 &&
         (!q.bias || ((uintptr_t)q.bias % 16 == 0 && q.sBias % 4 == 0));
}
// LDS-DMA NT kernel (gemm_glds.hip; no transposition): whole 64-element K tiles, no split-K
bool nt_glds_takes(const GemmProblem& q) { return q.K % 64 == 0 && q.splitk == 1 && !q.bias_grad; }
}  // namespace

// smallest tile that still gives the chip >= ~2 workgroups per CU; otherwise the largest tile count wins
// (the Stack C and Stack B executors and mmdeer_gemm / mmdeer_gemm_batch share this policy)
GemmTile pick_tile(const GemmGroup& g) {
  const int ft = opt(OPT_TILE);
  if (ft >= 0 && ft <= 4) return (GemmTile)ft;
  // weight-gradient groups (both operands transposed): the strided loads and the packing LDS store cost the same per
  // K-tile whatever the tile size, so the largest tile wins; split-K supplies the parallelism
  if (g.p[0].trans_a) { const int t = opt(OPT_DW_TILE); return (GemmTile)(t < 2 ? 2 : t > 4 ? 4 : t); }   // 256x256 (falls back to 128x128 per sub-group where the kernel does not apply)
  // bf16: 128x64 and 64x64 run on the LDS-DMA kernel, 128x128 only on the register-staged one (measured on the
  // trimodal in_proj, 768 tiles of 128x128: 28.5 us against 17 us as 1536 tiles of 128x64)
  const bool f32 = g.p[0].a_f32 && g.p[0].b_f32;
  if (f32 && group_tiles(g, 128, 128) >= 512) return TILE_128x128;
  if (!f32) {   // big forward problems: 256x256 tiles when they fill most of the chip in one round (in_proj: 192)
    const long long t256 = group_tiles(g, 256, 256);
    const bool plain = every_problem(g, [](const GemmProblem& p) { return !p.Y && !p.trans_b; });
    if (plain && t256 >= 160 && t256 <= 256) return TILE_256x256;
  }
  // ~one 128x64 tile per CU: the 8-wave 128x64 kernel (gemm_route) moves 25 % fewer operand bytes than two 64x64
  // workgroups per CU, and the K loop of those is bound by the CU's vector-memory path
  const long long t128x64 = group_tiles(g, 128, 64);
  if (!f32 && !g.p[0].trans_a && !g.p[0].trans_b && t128x64 >= 200 && t128x64 <= 320) return TILE_128x64;
  if (t128x64 >= opt(OPT_T128)) return TILE_128x64;   // option "t128": smallest 128x64 tile count that selects that kernel
  return TILE_64x64;
}

// The kernel a homogeneous sub-group runs, and its tile.
GemmRoute gemm_route(const GemmGroup& sub, int compute_f32, GemmTile tile_req) {
  const GemmProblem& p0 = sub.p[0];
  // every LDS-DMA kernel: bf16 compute on operands read in whole 16-byte chunks
  const bool dma = !compute_f32 && p0.a_mode == SRC_BF16_V16 && p0.b_mode == SRC_BF16_V16 && opt(OPT_GLDS);
  const bool big = tile_req == TILE_256x256 || tile_req == TILE_256x128;   // tiles the register-staged kernels do not have
  if (p0.trans_a) {   // weight gradient.  256-row tiles exist only as the LDS-DMA kernel; anything else of such a group runs 128x128
    if (dma && dw_dma_requested(sub, compute_f32, tile_req) && every_problem(sub, dw_dma_takes)) {
      // 128x128: the K-split form (KG = 2) needs 64-row stages
      const bool k2 = tile_req == TILE_128x128 && opt(OPT_DW_KG) == 2 &&
                      every_problem(sub, [](const GemmProblem& q) { return q.K % 64 == 0; });
      return {GEMM_TT_DMA, TILE_BM[tile_req], TILE_BN[tile_req], k2 ? 2 : 1};
    }
    const GemmTile t = big ? TILE_128x128 : tile_req;
    return {GEMM_TT_REG, TILE_BM[t], TILE_BN[t], 0};
  }
  const GemmTile t = big ? TILE_128x64 : tile_req;
  if (p0.trans_b) return {GEMM_NX_REG, TILE_BM[t], TILE_BN[t], 0};
  if (dma && tile_req == TILE_256x256 && every_problem(sub, nt256_takes)) {
    // 256x192 tiles when they fill the chip in one round and 256x256 tiles do not
    const long long t192 = group_tiles(sub, 256, 192);
    const bool n192 = opt(OPT_NT192) && every_problem(sub, [](const GemmProblem& q) { return q.N % 192 == 0; }) && t192 <= 256 &&
                      t192 > group_tiles(sub, 256, 256);
    return {GEMM_NT256, 256, n192 ? 192 : 256, 0};
  }
  if (dma && every_problem(sub, nt_glds_takes)) {
    const long long t64 = group_tiles(sub, 128, 64), t128 = group_tiles(sub, 128, 128);
    // These launches are bound by the bytes a CU pulls through its vector-memory path (~40 B/clk of LDS-DMA): when 128x64
    // tiles need two workgroups per CU (in_proj dX: 512 tiles x 576 KB) and 128x128 tiles cover the problems with about one
    // 8-wave workgroup per CU (256 x 768 KB), the square tile moves a third fewer bytes per CU
    if (t == TILE_128x64 && opt(OPT_NT128) && every_problem(sub, [](const GemmProblem& q) { return q.N % 128 == 0; }) && t64 > 320 &&
        t128 >= 160 && t128 <= 320)
      return {GEMM_NT_GLDS, 128, 128, 8};
    if (t == TILE_64x64) return {GEMM_NT_GLDS, 64, 64, 4};
    // up to ~one workgroup per CU: the 8-wave form (96 KiB ring, one per CU); more tiles: 4 waves, 72 KiB ring, two per CU
    if (t == TILE_128x64) return {GEMM_NT_GLDS, 128, 64, (t64 <= 320 && opt(OPT_NT8)) ? 8 : 4};
    // (other 128x128 launches keep the register-staged kernel: its 74 KiB of LDS allow two workgroups per CU)
  }
  return {GEMM_NT_REG, TILE_BM[t], TILE_BN[t], 0};
}

// whether a kernel instantiates the (A mode, B mode) pair (gemm.h: GEMM_MODE_PAIRS_*)
bool gemm_modes_instantiated(int ta, int tb, int compute_f32, int am, int bm) {
  if (compute_f32) return am == SRC_F32 && bm == SRC_F32;
#define X(a, b) || (am == a && bm == b)
  if (!ta && !tb) return false GEMM_MODE_PAIRS_NT(X);
  if (!ta && tb) return false GEMM_MODE_PAIRS_NX(X);
  if (ta && tb) return false GEMM_MODE_PAIRS_TT(X);
#undef X
  return false;
}

bool gemm_group_single_launch(const GemmGroup& g, int compute_f32, GemmTile tile_req, int k) {
  GemmGroup c = g;
  if (prepare_gemm_group(c, compute_f32, tile_req) != 0) return false;   // (the launch itself will refuse it, with this message)
  for (int i = 1; i < c.nprob; ++i)
    if (c.p[i].a_mode != c.p[0].a_mode || c.p[i].b_mode != c.p[0].b_mode) return false;
  return gemm_route(c, compute_f32, tile_req).kernel == k;
}

void gemm_problem_defaults(GemmProblem& p) {
  p = GemmProblem{};
  p.batch = p.splitk = 1;
  p.drop_site = p.regen_site = -1;
  p.mask_scale = 1.f;
}

int prepare_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile_req) {
  MMDEER_CHECK(g.nprob >= 1 && g.nprob <= GEMM_MAX_PROBLEMS, "gemm: bad problem count %d", g.nprob);
  MMDEER_CHECK((int)tile_req >= 0 && (int)tile_req <= 4, "gemm: bad tile id %d", (int)tile_req);
  const int ta = g.p[0].trans_a ? 1 : 0, tb = g.p[0].trans_b ? 1 : 0;
  MMDEER_CHECK(!ta || tb, "gemm: (trans_a=1, trans_b=0) is not instantiated");
  // the whole group runs on the weight-gradient DMA kernel (it alone tolerates padded, half-valid row ends)
  const bool pad256 = dw_dma_requested(g, compute_f32, tile_req) && every_problem(g, dw_dma_takes);
  for (int i = 0; i < g.nprob; ++i) {
    GemmProblem& p = g.p[i];
    MMDEER_CHECK((p.trans_a ? 1 : 0) == ta && (p.trans_b ? 1 : 0) == tb, "gemm[%d]: all problems of a launch must share trans flags", i);
    MMDEER_CHECK(p.M >= 0 && p.N > 0 && p.K > 0 && p.batch >= 1, "gemm[%d]: bad shape M=%d N=%d K=%d", i, p.M, p.N, p.K);
    MMDEER_CHECK(p.A && p.B && p.C, "gemm[%d]: A / B / C must be non-NULL", i);
    MMDEER_CHECK(p.N % 4 == 0, "gemm[%d]: N=%d must be a multiple of 4", i, p.N);
    MMDEER_CHECK(p.trans_a || p.K % 4 == 0, "gemm[%d]: K=%d must be a multiple of 4 for a k-contiguous A", i, p.K);
    MMDEER_CHECK(p.trans_b || p.K % 4 == 0, "gemm[%d]: K=%d must be a multiple of 4 for a k-contiguous B", i, p.K);
    MMDEER_CHECK(!p.trans_a || p.M % 4 == 0, "gemm[%d]: M=%d must be a multiple of 4 for a transposed A", i, p.M);
    MMDEER_CHECK(p.lda % 4 == 0 && p.ldb % 4 == 0 && p.ldc % 4 == 0, "gemm[%d]: leading dims must be multiples of 4", i);
    MMDEER_CHECK(p.lda >= (p.trans_a ? p.M : p.K), "gemm[%d]: lda=%d is shorter than a row of A (%d)", i, p.lda, p.trans_a ? p.M : p.K);
    MMDEER_CHECK(p.ldb >= (p.trans_b ? p.N : p.K), "gemm[%d]: ldw=%d is shorter than a row of W (%d)", i, p.ldb, p.trans_b ? p.N : p.K);
    MMDEER_CHECK(p.ldc >= p.N, "gemm[%d]: ldc=%d is shorter than a row of C (N=%d)", i, p.ldc, p.N);
    MMDEER_CHECK(!p.Y || p.ldy >= p.N, "gemm[%d]: ldy=%d is shorter than a row of Y (N=%d)", i, p.ldy, p.N);
    MMDEER_CHECK(((uintptr_t)p.A % 16 == 0) && ((uintptr_t)p.B % 16 == 0) && ((uintptr_t)p.C % 8 == 0),
                 "gemm[%d]: A and B must be 16-byte aligned, C 8-byte aligned", i);
    MMDEER_CHECK(p.M == 0 || ((long long)p.lda * (p.trans_a ? p.K : p.M) >= 8 && (long long)p.ldb * (p.trans_b ? p.K : p.N) >= 8),
                 "gemm[%d]: operands must hold at least 8 elements", i);
    MMDEER_CHECK(!p.Y || p.ldy % 4 == 0, "gemm[%d]: ldy must be a multiple of 4", i);
    MMDEER_CHECK(!(p.accumulate && !p.c_f32), "gemm[%d]: accumulate needs an fp32 C", i);
    if (p.splitk < 1) p.splitk = 1;
    if (p.splitk > 1) {
      MMDEER_CHECK(p.slab_c && p.c_f32 && !p.bias && !p.relu && !p.Y && !p.accumulate && p.drop_site < 0 && p.regen_site < 0,
                   "gemm[%d]: split-K needs an fp32 slab and no epilogue", i);
      MMDEER_CHECK(!p.bias_grad || p.slab_b, "gemm[%d]: split-K with bias_grad needs slab_b", i);
      const int nk = gemm_ktiles(p.K, compute_f32);
      if (p.splitk > nk) p.splitk = nk;
    }
    if (compute_f32) {
      MMDEER_CHECK(p.a_f32 && p.b_f32, "gemm[%d]: fp32 compute needs fp32 operands", i);
      p.a_mode = p.b_mode = SRC_F32;
    } else {
      // 16-byte loads of a bf16 source need 16-byte aligned rows AND no half-valid chunk (extent multiple of 8).
      // Exception, weight-gradient DMA kernel only (pad256): a transposed operand may end in a half-valid chunk
      // when its rows are padded -- the extra columns are read from inside the row and only feed outputs that are
      // never stored (the padded audio block: 84 valid columns in 128-element rows).
      const bool av16 = p.lda % 8 == 0 && p.sA % 8 == 0 &&
                        (p.trans_a ? (p.M % 8 == 0 || (pad256 && p.batch == 1 && p.lda >= (p.M + 7) / 8 * 8)) : p.K % 8 == 0);
      const bool bv16 = p.ldb % 8 == 0 && p.sB % 8 == 0 &&
                        (p.trans_b ? (p.N % 8 == 0 || (pad256 && p.batch == 1 && p.ldb >= (p.N + 7) / 8 * 8)) : p.K % 8 == 0);
      p.a_mode = p.a_f32 ? SRC_F32 : (av16 ? SRC_BF16_V16 : SRC_BF16_V8);
      p.b_mode = p.b_f32 ? SRC_F32 : (bv16 ? SRC_BF16_V16 : SRC_BF16_V8);
    }
  }
  return 0;
}

namespace {
struct KernelEntry { const char* name; GemmLauncher* launch; };
const KernelEntry KERNELS[GEMM_KERNEL_COUNT] = {   // indexed by GemmKernel
    {"nt_reg", gemm_launch_nt_reg}, {"nx_reg", gemm_launch_nx_reg}, {"tt_reg", gemm_launch_tt_reg},
    {"nt_glds", gemm_launch_nt_glds}, {"nt256", gemm_launch_nt256}, {"tt_dma", gemm_launch_tt_dma}};

struct DryRun { char* out; int cap, len; };   // describe_gemm_group: the lines written so far (always NUL-terminated within cap)
void describe_launch(DryRun& d, const GemmRoute& r, const GemmGroup& sub, int total) {
  static const char* const mode[3] = {"f32", "v16", "v8"};   // SrcMode
  char var[8] = "";   // w<waves> / k<KG>
  if (r.variant) snprintf(var, sizeof var, " %c%d", r.kernel == GEMM_NT_GLDS ? 'w' : 'k', r.variant);
  if (d.len >= d.cap) return;
  const int n = snprintf(d.out + d.len, d.cap - d.len, "%s%s %dx%d%s a=%s b=%s tiles=%d", d.len ? "\n" : "", KERNELS[r.kernel].name,
                         r.BM, r.BN, var, mode[sub.p[0].a_mode], mode[sub.p[0].b_mode], total);
  d.len = d.len + n < d.cap ? d.len + n : d.cap;
}

// Runs (dry == null) or describes a group; returns the number of launches, -1 when refused.
int walk_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile_req, hipStream_t stream, DryRun* dry) {
  if (prepare_gemm_group(g, compute_f32, tile_req) != 0) return -1;
  g.xcd_remap = opt(OPT_XCD);
  const int ta = g.p[0].trans_a ? 1 : 0, tb = g.p[0].trans_b ? 1 : 0;
  // every problem's source-mode pair before the first launch of the group: a refused group writes nothing
  for (int i = 0; i < g.nprob; ++i)
    MMDEER_CHECK(gemm_modes_instantiated(ta, tb, compute_f32, g.p[i].a_mode, g.p[i].b_mode),
                 "gemm[%d]: source-mode pair (%d,%d) is not instantiated for trans=(%d,%d)", i, g.p[i].a_mode, g.p[i].b_mode, ta, tb);
  // One launch per distinct (A mode, B mode) pair: the kernels are specialised on the pair so that their K loop
  // has no data-dependent control flow.  Most groups are homogeneous (one launch).
  int launches = 0;
  bool done[GEMM_MAX_PROBLEMS] = {};
  for (int i = 0; i < g.nprob; ++i) {
    if (done[i]) continue;
    GemmGroup sub{};
    sub.stamps = g.stamps; sub.xcd_remap = g.xcd_remap; sub.drop = g.drop;
    for (int j = i; j < g.nprob; ++j) {
      if (done[j] || g.p[j].a_mode != g.p[i].a_mode || g.p[j].b_mode != g.p[i].b_mode) continue;
      done[j] = true;
      sub.p[sub.nprob++] = g.p[j];
    }
    const GemmRoute r = gemm_route(sub, compute_f32, tile_req);
    if (g.fold.cnt || g.fold.nseg || g.fold.bump) {
      // the caller asked gemm_group_single_launch first: a group that splits, or runs another kernel, has no in-launch fold
      MMDEER_CHECK(sub.nprob == g.nprob && r.kernel == GEMM_TT_DMA, "gemm: the in-launch fold needs the whole group in one tt_dma launch");
      sub.fold = g.fold;
    }
    int total = 0;
    for (int j = 0; j < sub.nprob; ++j) {
      GemmProblem& q = sub.p[j];
      q.tiles_m = ceil_div(q.M, r.BM); q.tiles_n = ceil_div(q.N, r.BN);
      sub.tile_start[j] = total;
      total += (int)gemm_tiles(q.M, q.N, r.BM, r.BN) * q.batch * q.splitk;
    }
    for (int j = sub.nprob; j <= GEMM_MAX_PROBLEMS; ++j) sub.tile_start[j] = total;
    if (total == 0) continue;  // empty batch: nothing to do
    if (sub.fold.cnt) MMDEER_CHECK(total <= sub.fold.cnt_n, "gemm: %d workgroups but %d tile counters", total, sub.fold.cnt_n);
    if (sub.fold.nseg) {
      GemmFold& f = sub.fold;
      MMDEER_CHECK(f.nseg > 0 && f.nseg <= GEMM_FOLD_SEGMENTS, "gemm: bad fold segment count %d", f.nseg);
      int blocks = 0;
      for (int j = 0; j < f.nseg; ++j) {
        MMDEER_CHECK(f.src[j] && f.dst[j] && f.n[j] % 4 == 0 && f.nparts[j] >= 1 && f.stride[j] % 4 == 0,
                     "gemm: fold segment %d: n and stride must be multiples of 4", j);
        f.bstart[j] = blocks;
        blocks += (f.n[j] + 255) / 256;
      }
      for (int j = f.nseg; j <= GEMM_FOLD_SEGMENTS; ++j) f.bstart[j] = blocks;
    }
    ++launches;
    if (dry) describe_launch(*dry, r, sub, total);
    else TRY(KERNELS[r.kernel].launch(sub, total, r, compute_f32, stream));
  }
  return launches;
}
}  // namespace

int launch_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile_req, hipStream_t stream) {
  return walk_gemm_group(g, compute_f32, tile_req, stream, nullptr) < 0 ? -1 : 0;
}

int describe_gemm_group(GemmGroup& g, int compute_f32, GemmTile tile_req, char* out, int cap) {
  DryRun d{out, out && cap > 0 ? cap : 0, 0};
  if (d.cap) out[0] = 0;
  return walk_gemm_group(g, compute_f32, tile_req, nullptr, &d);
}

}  // namespace mmdeer
