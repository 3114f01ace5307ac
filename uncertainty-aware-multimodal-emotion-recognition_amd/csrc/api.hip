// libmmdeer_hip.so -- C ABI (include/mmdeer.h): version and error plumbing, and the single operators as thin wrappers of the
// launchers (the options live in options.hip, the Stack C executor in stackc.hip, Stack B's in stackb.hip).  Host code only: every
// function enqueues on the caller's stream and returns; nothing here allocates device memory or synchronises.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mmdeer.h"
#include "../../include/mmdeer_routes.h"
#include "../../include/mmdeer_video.h"
#include "../../include/mmdeer_frames.h"
#include "../../include/mmdeer_frames_bwd.h"
#include "../../include/mmdeer_bert.h"
#include "../../include/mmdeer_bert_bwd.h"
#include "../../include/mmdeer_bert_drop.h"
#include "../../include/mmdeer_optim.h"
#include "../../include/mmdeer_graph.h"
#include "../../include/mmdeer_drop_dev.h"
#include "../../include/mmdeer_seqlen.h"
#include "attention.h"
#include "common.h"
#include "gemm.h"
#include "nig.h"
#include "optim.h"
#include "options.h"
#include "chain.h"
#include "rowops.h"

namespace mmdeer {

#ifdef MMDEER_STAMPS
void tf_set_stamps(unsigned long long* p);   // tri_fused.hip
#endif
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

LossCfg loss_cfg(const mmdeer_loss_cfg& c) {
  LossCfg cfg;
  cfg.reg_w = c.reg_weight; cfg.kl_w = c.kl_weight; cfg.ece_w = c.ece_weight; cfg.cross_w = c.cross_weight;
  for (int i = 0; i < 3; ++i) cfg.task_w[i] = c.task_weight[i];
  return cfg;
}

DropCtx make_drop(float p, uint64_t seed, uint64_t offset, const uint64_t* offset_dev) {
  DropCtx d;
  d.seed = seed;
  d.offset = offset;
  d.offset_dev = reinterpret_cast<const unsigned long long*>(offset_dev);
  double keep = 1.0 - (double)p;
  if (keep < 0) keep = 0;
  double t = keep * 4294967296.0;
  d.thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
  d.scale = keep > 0 ? (float)(1.0 / keep) : 0.f;
  return d;
}

}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

const char* mmdeer_version(void) { return "mmdeer-hip 0.1.0 (gfx950)"; }
int mmdeer_abi_version(void) { return MMDEER_ABI_VERSION; }
const char* mmdeer_last_error(void) { return g_err; }

#ifdef MMDEER_STAMPS
// diagnostic library only (not part of the ABI)
int mmdeer_debug_nig_stamps(unsigned long long* out16) { return mmdeer::debug_nig_stamps(out16); }
void mmdeer_debug_tf_stamps(void* p) { mmdeer::tf_set_stamps(reinterpret_cast<unsigned long long*>(p)); }
#endif

// ------------------------------------------------------------------ single operators
namespace {
// Whether a problem of mmdeer_gemm / mmdeer_gemm_batch may be split: the fold of its slab slices runs over C and bias_grad as dense
// runs of a multiple of 4 floats with 16-byte vector accesses.  The others (a C with ldc != N, an unaligned output) run their whole
// reduction in one workgroup per tile, at any K: whether a call is accepted, and what it writes, does not depend on the split policy.
bool batch_may_split(const mmdeer_gemm_args& q) {
  return q.ldc == q.N && (long long)q.M * q.N % 4 == 0 && ((uintptr_t)q.C % 16) == 0 &&
         (!q.bias_grad || (q.M % 4 == 0 && ((uintptr_t)q.bias_grad % 16) == 0));
}

// Everything mmdeer_gemm does before its first launch, shared with the dry run mmdeer_gemm_route: the argument mapping, the split
// decision, the tile and every check of the group launcher.  Touches no GPU and dereferences no operand pointer.
int gemm_front(const mmdeer_gemm_args* a, GemmGroup& g, GemmTile& t, int& f32) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  g = GemmGroup{};
  g.nprob = 1;
  GemmProblem& p = g.p[0];
  gemm_problem_defaults(p);
  p.A = a->A; p.B = a->W; p.C = a->C; p.bias = a->bias; p.bias_grad = a->bias_grad; p.Y = a->Y;
  p.M = a->M; p.N = a->N; p.K = a->K; p.lda = a->lda; p.ldb = a->ldw; p.ldc = a->ldc; p.ldy = a->ldy;
  p.a_f32 = a->a_f32; p.b_f32 = a->w_f32; p.c_f32 = a->c_f32; p.y_f32 = a->y_f32;
  p.trans_a = a->trans_a; p.trans_b = a->trans_w; p.relu = a->relu; p.accumulate = a->accumulate;
  p.drop_site = a->drop_site; p.drop_shift = a->drop_shift; p.regen_site = a->regen_site;
  p.mask_scale = a->mask_scale;
  MMDEER_CHECK(a->A && a->W && a->C, "gemm: A / W / C must be non-NULL");
  if (a->splitk > 1) {
    // the request is checked whether or not the problem is then split: acceptance does not depend on the layout of C
    MMDEER_CHECK(a->slab != nullptr && ((uintptr_t)a->slab % 16) == 0,
                 "gemm: split-K needs a 16-byte aligned slab of splitk * (M*N + M) floats");
    MMDEER_CHECK(a->c_f32 && !a->bias && !a->relu && !a->Y && !a->accumulate && a->drop_site < 0 && a->regen_site < 0,
                 "gemm: split-K needs an fp32 C and no epilogue");
    if (batch_may_split(*a)) {
      p.splitk = a->splitk;
      p.slab_stride = ((long long)a->M * a->N + a->M + 3) / 4 * 4;
      p.slab_c = a->slab;
      p.slab_b = a->slab + (long long)a->M * a->N;
    }
  }
  g.drop = make_drop(a->dropout_p, a->seed, a->offset, a->offset_dev);
  g.stamps = reinterpret_cast<unsigned long long*>(a->debug);
  t = (a->tile >= 0 && a->tile <= 4) ? (GemmTile)a->tile : pick_tile(g);
  f32 = a->compute_f32 ? 1 : 0;
  TRY(prepare_gemm_group(g, f32, t));   // every check before the first launch (prepare also clamps splitk to the K-tile count)
  return 0;
}
}  // namespace

int mmdeer_gemm(const mmdeer_gemm_args* a) {
  GemmGroup g;
  GemmTile t;
  int f32;
  TRY(gemm_front(a, g, t, f32));
  const GemmProblem& p = g.p[0];
  const int sk = p.splitk;
  TRY(launch_gemm_group(g, f32, t, (hipStream_t)a->stream));
  if (sk > 1) {   // fold the K-slices into C (and bias_grad); batch_may_split: dense C, M*N and M multiples of 4
    ReduceTable rt{};
    rt.nseg = 1;
    rt.src[0] = p.slab_c; rt.dst[0] = reinterpret_cast<float*>(p.C); rt.nparts[0] = sk;
    rt.n[0] = a->M * a->N; rt.stride[0] = p.slab_stride;
    if (p.bias_grad) {
      rt.nseg = 2;
      rt.src[1] = p.slab_b; rt.dst[1] = p.bias_grad; rt.nparts[1] = sk; rt.n[1] = a->M; rt.stride[1] = p.slab_stride;
    }
    TRY(launch_reduce_partials(rt, (hipStream_t)a->stream));
  }
  return 0;
}

int mmdeer_gemm_route(const mmdeer_gemm_args* a, char* out, int cap) {
  GemmGroup g;
  GemmTile t;
  int f32;
  TRY(gemm_front(a, g, t, f32));
  return describe_gemm_group(g, f32, t, out, cap);
}

namespace {
// weight-gradient batch: split policy of Exec::set_split (ksteps_target K-tiles per slice, capped)
// `boost` multiplies the slice count of every problem of a group whose tiles would leave most of the chip idle (Stack B: a
// group is 16 matrices of 256 x 256 = 16 tiles; at the default 4 slices that is 64 workgroups, each a chain of 32 K-steps)
constexpr int BATCH_SPLITK_MAX = 16;
int batch_splitk(int K, int f32, int boost) {
  const int nk = gemm_ktiles(K, f32);
  int sk;
  if (boost < 0) sk = (nk + (-boost) - 1) / (-boost);      // boost = -L: slices of at most L K-tiles (batch_boost's search below)
  else { const int kst = ksteps_target(f32); sk = ((nk + kst - 1) / kst) * boost; }
  if (sk > BATCH_SPLITK_MAX) sk = BATCH_SPLITK_MAX;
  if (sk > nk / 2) sk = nk / 2;          // at least two K-tiles per slice
  return sk < 1 ? 1 : sk;
}
// The split of one group of problems.  bf16 weight-gradient DMA kernel (128 x 128 tiles, the default): the slice length L (in 64-row
// K-tiles) that minimises a cost model of the group -- rounds of 256 workgroups x (the longest slice at 0.62 us per K-tile per workgroup +
// a fixed 4 us) + the fold of the slabs (two passes over 64 KiB per slice tile at ~3 TB/s, + 4 us if anything is folded) -- returned as
// -L.  (Round 4 before this: a fixed 16 K-tiles per slice, times a boost that counted 256 x 256 tiles: Stack B's first group of 16
// matrices ran as 592 workgroups in three rounds + a 17 us fold, 68 us, where 148 unsplit workgroups take one round of ~43 us.)
// Other kernels: slices of ksteps_target K-tiles, times `boost` when the group would leave most of the chip idle.
int batch_problem_splitk(const mmdeer_gemm_args& q, int f32, int boost) { return batch_may_split(q) ? batch_splitk(q.K, f32, boost) : 1; }

int batch_boost(const mmdeer_gemm_args* a, int n, int f32) {
  if (!f32 && opt(OPT_DW_TILE) == 2 && opt(OPT_KSTEPS) == 0) {
    int bestL = 16;
    double best = 1e30;
    for (int L = 8; L <= 256; L += (L < 32 ? 8 : L < 64 ? 16 : 32)) {
      long long wgs = 0, slab_tiles = 0;
      int longest = 0;
      for (int i = 0; i < n; ++i) {
        const long long tiles = gemm_tiles(a[i].M, a[i].N, 128, 128);
        const int nk = gemm_ktiles(a[i].K, f32), sk = batch_problem_splitk(a[i], f32, -L), len = (nk + sk - 1) / sk;
        wgs += tiles * sk;
        if (sk > 1) slab_tiles += tiles * sk;
        if (len > longest) longest = len;
      }
      const double cost = (double)((wgs + 255) / 256) * (longest * 0.62 + 4.0) + (slab_tiles ? slab_tiles * 0.044 + 4.0 : 0.0);
      if (cost < best - 1e-9) { best = cost; bestL = L; }
    }
    return -bestL;
  }
  // tiles of the kernel that will run (256 x 256 unless the 128 x 128 kernel was chosen by option with a fixed slice length)
  const int t = (!f32 && opt(OPT_DW_TILE) == 2) ? 128 : 256;
  long long wgs = 0;
  for (int i = 0; i < n; ++i)
    wgs += gemm_tiles(a[i].M, a[i].N, t, t) * batch_problem_splitk(a[i], f32, 1);
  int boost = 1;
  while (boost < 4 && wgs * boost * 2 <= 256) boost *= 2;
  return boost;
}
long long batch_slice_elems(const mmdeer_gemm_args& a) { return ((long long)a.M * a.N + a.M + 63) / 64 * 64; }

// Every check of mmdeer_gemm_batch (and of the group launcher it feeds), made before the first launch: a refused call writes nothing.
int check_gemm_batch(const mmdeer_gemm_args* a, int n) {
  for (int i = 0; i < n; ++i) {
    const mmdeer_gemm_args& q = a[i];
    MMDEER_CHECK(q.trans_a && q.trans_w && q.c_f32 && !q.bias && !q.relu && !q.Y && q.drop_site < 0 && q.regen_site < 0 && !q.accumulate,
                 "gemm_batch[%d]: weight-gradient problems only (both operands transposed, fp32 C, no epilogue)", i);
    MMDEER_CHECK((q.compute_f32 ? 1 : 0) == (a[0].compute_f32 ? 1 : 0), "gemm_batch[%d]: all problems must share the compute dtype", i);
    MMDEER_CHECK(!q.compute_f32 || (q.a_f32 && q.w_f32), "gemm_batch[%d]: fp32 compute needs fp32 operands", i);
    MMDEER_CHECK(q.A && q.W && q.C, "gemm_batch[%d]: A / W / C must be non-NULL", i);
    MMDEER_CHECK(q.M > 0 && q.N > 0 && q.K > 0 && q.M % 4 == 0 && q.N % 4 == 0,
                 "gemm_batch[%d]: M=%d N=%d K=%d: positive, M and N multiples of 4", i, q.M, q.N, q.K);
    MMDEER_CHECK(q.lda >= q.M && q.ldw >= q.N && q.ldc >= q.N && q.lda % 4 == 0 && q.ldw % 4 == 0 && q.ldc % 4 == 0,
                 "gemm_batch[%d]: lda >= M, ldw >= N, ldc >= N, all multiples of 4", i);
    MMDEER_CHECK((long long)q.lda * q.K >= 8 && (long long)q.ldw * q.K >= 8, "gemm_batch[%d]: operands must hold at least 8 elements", i);
    MMDEER_CHECK(((uintptr_t)q.A % 16) == 0 && ((uintptr_t)q.W % 16) == 0 && ((uintptr_t)q.C % 8) == 0,
                 "gemm_batch[%d]: A and W must be 16-byte aligned, C 8-byte aligned", i);
  }
  return 0;
}
}  // namespace

long long mmdeer_gemm_batch_slab_elems(const mmdeer_gemm_args* a, int n) {
  if (!a || n <= 0) return 0;
  long long tot = 0;
  for (int i0 = 0; i0 < n; i0 += GEMM_MAX_PROBLEMS) {
    const int cnt = (n - i0) < GEMM_MAX_PROBLEMS ? (n - i0) : GEMM_MAX_PROBLEMS, f32 = a[i0].compute_f32 ? 1 : 0;
    const int boost = batch_boost(a + i0, cnt, f32);
    for (int i = i0; i < i0 + cnt; ++i) {
      const int sk = batch_problem_splitk(a[i], f32, boost);
      if (sk > 1) tot += sk * batch_slice_elems(a[i]);
    }
  }
  return tot;
}

int mmdeer_gemm_batch(const mmdeer_gemm_args* a, int n, float* slab, long long slab_elems, void* stream) {
  MMDEER_CHECK(a != nullptr && n >= 0, "gemm_batch: bad arguments");
  TRY(check_gemm_batch(a, n));
  const long long need = mmdeer_gemm_batch_slab_elems(a, n);
  MMDEER_CHECK(need == 0 || (slab != nullptr && ((uintptr_t)slab % 16) == 0 && need <= slab_elems),
               "gemm_batch: slab too small or unaligned (%lld floats given, %lld needed, 16-byte aligned)", slab_elems, need);
  const int f32 = n > 0 && a[0].compute_f32 ? 1 : 0;
  // every group is built and checked (operand source modes included) before the first launch
  std::vector<GemmGroup> groups((n + GEMM_MAX_PROBLEMS - 1) / GEMM_MAX_PROBLEMS);
  std::vector<ReduceTable> folds(groups.size());
  std::vector<GemmTile> tiles(groups.size());
  long long used = 0;
  for (int i0 = 0, gi = 0; i0 < n; i0 += GEMM_MAX_PROBLEMS, ++gi) {
    GemmGroup& g = groups[gi];
    ReduceTable& rt = folds[gi];
    g = GemmGroup{};
    rt = ReduceTable{};
    static_assert(2 * GEMM_MAX_PROBLEMS <= REDUCE_MAX_SEGMENTS, "the fold of one group (C and bias_grad per problem) is one launch");
    const int boost = batch_boost(a + i0, (n - i0) < GEMM_MAX_PROBLEMS ? (n - i0) : GEMM_MAX_PROBLEMS, f32);
    for (int i = i0; i < n && i < i0 + GEMM_MAX_PROBLEMS; ++i) {
      const mmdeer_gemm_args& q = a[i];
      GemmProblem& p = g.p[g.nprob++];
      gemm_problem_defaults(p);
      p.A = q.A; p.B = q.W; p.C = q.C; p.bias_grad = q.bias_grad;
      p.M = q.M; p.N = q.N; p.K = q.K; p.lda = q.lda; p.ldb = q.ldw; p.ldc = q.ldc;
      p.a_f32 = q.a_f32; p.b_f32 = q.w_f32; p.c_f32 = 1; p.trans_a = 1; p.trans_b = 1;
      const int sk = batch_problem_splitk(q, f32, boost);
      if (sk > 1) {         // batch_may_split: C is dense (ldc == N) and M*N, M are multiples of 4 -- the fold counts are exact
        const long long per = batch_slice_elems(q);
        p.splitk = sk; p.slab_stride = per; p.slab_c = slab + used; p.slab_b = slab + used + (long long)q.M * q.N;
        used += sk * per;
        int k = rt.nseg;
        rt.src[k] = p.slab_c; rt.dst[k] = reinterpret_cast<float*>(p.C); rt.nparts[k] = sk; rt.n[k] = q.M * q.N; rt.stride[k] = per; ++k;
        if (p.bias_grad) { rt.src[k] = p.slab_b; rt.dst[k] = p.bias_grad; rt.nparts[k] = sk; rt.n[k] = q.M; rt.stride[k] = per; ++k; }
        rt.nseg = k;
      }
    }
    g.drop = make_drop(0.f, 0, 0);
    tiles[gi] = pick_tile(g);
    TRY(prepare_gemm_group(g, f32, tiles[gi]));
    // bf16 compute: the weight-gradient kernels read dY (A) in whole 16-byte chunks only (a padded M only where the whole group runs on
    // the LDS-DMA kernels); W may be fp32 (converted by the loader) or bf16
    for (int k = 0; k < g.nprob; ++k)
      MMDEER_CHECK(f32 || g.p[k].a_mode == SRC_BF16_V16,
                   "gemm_batch[%d]: bf16 compute needs a bf16 A (dY) with lda %% 8 == 0 and M %% 8 == 0", i0 + k);
  }
  hipStream_t s = (hipStream_t)stream;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    TRY(launch_gemm_group(groups[gi], f32, tiles[gi], s));
    if (folds[gi].nseg > 0) TRY(launch_reduce_partials(folds[gi], s));
  }
  return 0;
}

int mmdeer_reduce_batch(int n, const float* const* src, float* const* dst, const int32_t* nparts, const int32_t* count,
                        const long long* stride, void* stream) {
  MMDEER_CHECK(n >= 0 && (n == 0 || (src && dst && nparts && count && stride)), "reduce_batch: bad arguments");
  for (int i = 0; i < n; ++i)       // every segment before the first launch: a refused call writes nothing
    MMDEER_CHECK(src[i] && dst[i] && nparts[i] >= 1 && count[i] >= 0 && count[i] % 4 == 0 && stride[i] % 4 == 0 &&
                     ((uintptr_t)src[i] % 16) == 0 && ((uintptr_t)dst[i] % 16) == 0,
                 "reduce_batch[%d]: 16-byte aligned pointers, count and stride multiples of 4", i);
  for (int i0 = 0; i0 < n; i0 += REDUCE_MAX_SEGMENTS) {
    ReduceTable t{};
    for (int i = i0; i < n && i < i0 + REDUCE_MAX_SEGMENTS; ++i) {
      const int k = t.nseg++;
      t.src[k] = src[i]; t.dst[k] = dst[i]; t.nparts[k] = nparts[i]; t.n[k] = count[i]; t.stride[k] = stride[i];
    }
    TRY(launch_reduce_partials(t, (hipStream_t)stream));
  }
  return 0;
}

int mmdeer_pack_transposed_batch(int n, const float* const* src, const int32_t* rows, const int32_t* cols, void* dst,
                                 const long long* dst_off, const int32_t* ld_dst, const int32_t* dst_col, int dst_f32, void* stream) {
  MMDEER_CHECK(n >= 0 && (n == 0 || (src && rows && cols && dst && dst_off && ld_dst && dst_col)), "pack_transposed_batch: bad arguments");
  for (int i = 0; i < n; ++i)       // every matrix before the first launch: a refused call writes nothing
    MMDEER_CHECK(src[i] && rows[i] > 0 && cols[i] > 0 && dst_off[i] >= 0 && dst_col[i] >= 0 && ld_dst[i] >= 0 &&
                     (ld_dst[i] == 0 || (long long)dst_col[i] + rows[i] <= ld_dst[i]),
                 "pack_transposed_batch[%d]: bad matrix (rows %d, cols %d, dst_off %lld, ld_dst %d, dst_col %d)", i, rows[i], cols[i],
                 dst_off[i], ld_dst[i], dst_col[i]);
  for (int i0 = 0; i0 < n; i0 += PACKT_MAX) {
    PackTTable t{};
    for (int i = i0; i < n && i < i0 + PACKT_MAX; ++i) {
      const int k = t.nmat++;
      t.src[k] = src[i]; t.rows[k] = rows[i]; t.cols[k] = cols[i]; t.dst_off[k] = dst_off[i]; t.ld_dst[k] = ld_dst[i]; t.dst_col[k] = dst_col[i];
    }
    TRY(launch_pack_transposed(t, dst, dst_f32 ? 1 : 0, (hipStream_t)stream));
  }
  return 0;
}

int mmdeer_adamw_flat(const mmdeer_adamw_flat_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  MMDEER_CHECK(a->params && a->grads && a->exp_avg && a->exp_avg_sq && a->scratch, "adamw_flat: params / grads / moments / scratch must be non-NULL");
  MMDEER_CHECK(a->nseg >= 1 && a->nseg <= ADAM_MAX_SEGMENTS && a->seg_begin && a->seg_elems && a->seg_lr, "adamw_flat: 1..%d segments", ADAM_MAX_SEGMENTS);
  MMDEER_CHECK(a->step >= 1, "adamw_flat: step must be >= 1 (got %d)", a->step);
  MMDEER_CHECK(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps > 0.f, "adamw_flat: bad betas / eps");
  MMDEER_CHECK(a->flat_elems > 0 && a->flat_elems % 4 == 0, "adamw_flat: flat_elems must be a positive multiple of 4");
  AdamTable t{};
  t.nseg = a->nseg;
  for (int i = 0; i < a->nseg; ++i) {
    MMDEER_CHECK(a->seg_begin[i] >= 0 && a->seg_elems[i] >= 0 && a->seg_begin[i] + a->seg_elems[i] <= a->flat_elems && a->seg_elems[i] < (1ll << 31),
                 "adamw_flat: segment %d out of range", i);
    t.param[i] = a->params + a->seg_begin[i];
    t.off[i] = a->seg_begin[i];
    t.n[i] = (int)a->seg_elems[i];
    t.is_vec[i] = 0;
    t.lr[i] = a->seg_lr[i];
  }
  t.grads = a->grads; t.exp_avg = a->exp_avg; t.exp_avg_sq = a->exp_avg_sq;
  t.partials = a->scratch; t.norm_out = a->grad_norm; t.flat_elems = a->flat_elems;
  t.beta1 = a->beta1; t.beta2 = a->beta2; t.eps = a->eps; t.weight_decay = a->weight_decay;
  t.bias_corr1 = 1.f - powf(a->beta1, (float)a->step);
  t.bias_corr2 = 1.f - powf(a->beta2, (float)a->step);
  t.max_norm = a->max_grad_norm; t.grad_scale = a->grad_scale;
  // without a packed copy the kernel still needs a destination: the fp32 parameters themselves (a second store of p)
  if (a->packed) return launch_adamw_pack(t, a->packed, a->packed_f32 ? 1 : 0, nullptr, (hipStream_t)a->stream);
  return launch_adamw_pack(t, a->params, 1, nullptr, (hipStream_t)a->stream);
}

int mmdeer_layernorm_fwd(const void* y, void* out, float* out32, float* mean, float* rstd, const float* gamma,
                         const float* beta, int M, int N, int act_f32, void* stream) {
  return launch_ln_fwd(y, out, out32, mean, rstd, gamma, beta, M, N, act_f32, (hipStream_t)stream);
}
int mmdeer_layernorm_bwd_nparts(int M) { return ln_bwd_nparts(M); }
int mmdeer_layernorm_bwd(const void* dout, const void* y, const float* mean, const float* rstd, const float* gamma,
                         void* dz, float* dgamma, float* dbeta, float* partial, int M, int N, int act_f32,
                         float mask_scale, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  MMDEER_CHECK((dgamma != nullptr) == (dbeta != nullptr), "layernorm_bwd: pass both dgamma and dbeta, or neither");   // before the launch
  TRY(launch_ln_bwd(dout, y, mean, rstd, gamma, dz, partial, M, N, act_f32, mask_scale, s));
  if (!dgamma && !dbeta) return 0;      // the caller folds the partials (mmdeer_reduce_batch)
  ReduceTable t{};
  t.nseg = 2;
  t.src[0] = partial; t.dst[0] = dgamma; t.nparts[0] = ln_bwd_nparts(M); t.n[0] = N; t.stride[0] = 2 * N;
  t.src[1] = partial + N; t.dst[1] = dbeta; t.nparts[1] = ln_bwd_nparts(M); t.n[1] = N; t.stride[1] = 2 * N;
  return launch_reduce_partials(t, s);
}

// the device step counter of include/mmdeer_drop_dev.h: one 8-byte-aligned uint64_t that the host never dereferences
static int counter_ok(const char* op, const uint64_t* offset_dev) {
  MMDEER_CHECK(((uintptr_t)offset_dev & 7) == 0, "%s: offset_dev must be 8-byte aligned", op);
  return 0;
}

int mmdeer_trimodal_attn_fwd(const void* qkv, void* obar, float* probs, float* attn_w, float* av_w, int B,
                             int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream) {
  return mmdeer_trimodal_attn_fwd_dev(qkv, obar, probs, attn_w, av_w, B, act_f32, training, dropout_p, seed, offset, stream, nullptr);
}
int mmdeer_trimodal_attn_fwd_dev(const void* qkv, void* obar, float* probs, float* attn_w, float* av_w, int B,
                                 int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream,
                                 const uint64_t* offset_dev) {
  MMDEER_CHECK(B >= 0, "trimodal_attn_fwd: batch must be >= 0 (got %d)", B);
  MMDEER_CHECK(B == 0 || (qkv && obar && probs), "trimodal_attn_fwd: NULL pointer (qkv / obar / probs)");
  TRY(counter_ok("trimodal_attn_fwd", offset_dev));
  const int train = (training && dropout_p > 0.f) ? 1 : 0;      // the kernel draws (and reads the counter) only when train
  const DropCtx dc = make_drop(dropout_p, seed, offset, train ? offset_dev : nullptr);
  return launch_tri_attn_fwd(qkv, obar, probs, attn_w, av_w, B, act_f32, train, dc, (hipStream_t)stream);
}
int mmdeer_trimodal_attn_bwd(const void* qkv, const void* dobar, const float* probs, void* dqkv, int B,
                             int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream) {
  return mmdeer_trimodal_attn_bwd_dev(qkv, dobar, probs, dqkv, B, act_f32, training, dropout_p, seed, offset, stream, nullptr);
}
int mmdeer_trimodal_attn_bwd_dev(const void* qkv, const void* dobar, const float* probs, void* dqkv, int B,
                                 int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream,
                                 const uint64_t* offset_dev) {
  MMDEER_CHECK(B >= 0, "trimodal_attn_bwd: batch must be >= 0 (got %d)", B);
  MMDEER_CHECK(B == 0 || (qkv && dobar && probs && dqkv), "trimodal_attn_bwd: NULL pointer (qkv / dobar / probs / dqkv)");
  TRY(counter_ok("trimodal_attn_bwd", offset_dev));
  const int train = (training && dropout_p > 0.f) ? 1 : 0;
  const DropCtx dc = make_drop(dropout_p, seed, offset, train ? offset_dev : nullptr);
  return launch_tri_attn_bwd(qkv, dobar, probs, dqkv, B, act_f32, train, dc, (hipStream_t)stream);
}

int mmdeer_pack_qkv_headmajor(const float* in_proj_weight, void* whm_bf16, void* stream) {
  MMDEER_CHECK(in_proj_weight && whm_bf16, "pack_qkv_headmajor: NULL argument");
  MMDEER_CHECK(((uintptr_t)in_proj_weight % 16) == 0 && ((uintptr_t)whm_bf16 % 16) == 0, "pack_qkv_headmajor: buffers must be 16-byte aligned");
  return launch_pack_qkv_headmajor(in_proj_weight, whm_bf16, (hipStream_t)stream);
}
int mmdeer_trimodal_fused_fwd(const void* xtok, const void* whm_bf16, const float* in_proj_bias, void* obar, float* probs,
                              void* qkv_out, float* attn_w, float* av_w, int B, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* stream) {
  MMDEER_CHECK(B >= 0, "trimodal_fused_fwd: batch must be >= 0 (got %d)", B);
  MMDEER_CHECK(B == 0 || (xtok && whm_bf16 && in_proj_bias && obar && probs), "trimodal_fused_fwd: NULL argument");
  const DropCtx dc = make_drop(dropout_p, seed, offset);
  const int train = (training && dropout_p > 0.f) ? 1 : 0;
  TRY(launch_tri_fused_fwd(xtok, whm_bf16, in_proj_bias, obar, probs, qkv_out, B, train, dc, (hipStream_t)stream));
  return launch_tri_attn_weights(probs, attn_w, av_w, B, train, dc, (hipStream_t)stream);
}
int mmdeer_trimodal_fused_bwd(const void* xtok, const void* whm_bf16, const float* in_proj_bias, const void* dobar,
                              const float* probs, void* dqkv, int B, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* stream) {
  MMDEER_CHECK(B >= 0, "trimodal_fused_bwd: batch must be >= 0 (got %d)", B);
  MMDEER_CHECK(B == 0 || (xtok && whm_bf16 && in_proj_bias && dobar && probs && dqkv), "trimodal_fused_bwd: NULL argument");
  const DropCtx dc = make_drop(dropout_p, seed, offset);
  return launch_tri_fused_bwd(xtok, whm_bf16, in_proj_bias, dobar, probs, dqkv, B, (training && dropout_p > 0.f) ? 1 : 0, dc,
                              (hipStream_t)stream);
}


long long mmdeer_deer_loss_v1_scratch(long long n) { return n > 0 ? 4ll * deer_v1_nblocks(n) : 0; }
int mmdeer_deer_loss_v1(const float* mu, const float* nu, const float* alpha, const float* beta, const float* targets,
                        long long n, float evidence_weight, float kl_weight, float* loss_out, float* dmu, float* dnu,
                        float* dalpha, float* dbeta, float* scratch, void* stream) {
  MMDEER_CHECK(mu && nu && alpha && beta && targets && loss_out && scratch, "deer_loss_v1: NULL argument");
  MMDEER_CHECK(n > 0, "deer_loss_v1: n must be > 0 (got %lld)", n);
  const int ng = (dmu != nullptr) + (dnu != nullptr) + (dalpha != nullptr) + (dbeta != nullptr);
  MMDEER_CHECK(ng == 0 || ng == 4, "deer_loss_v1: pass all four gradient buffers or none");
  return launch_deer_loss_v1(mu, nu, alpha, beta, targets, n, evidence_weight, kl_weight, loss_out, dmu, dnu, dalpha, dbeta, scratch,
                             (hipStream_t)stream);
}
int mmdeer_uncertainty_reg_loss(const float* alpha, const float* beta, int B, int D, float diversity_weight,
                                float sparsity_weight, float* loss_out, float* dalpha, float* dbeta, void* stream) {
  MMDEER_CHECK(alpha && beta && loss_out, "uncertainty_reg_loss: NULL argument");
  MMDEER_CHECK((dalpha != nullptr) == (dbeta != nullptr), "uncertainty_reg_loss: pass both gradient buffers or none");
  return launch_unc_reg_loss(alpha, beta, B, D, diversity_weight, sparsity_weight, loss_out, dalpha, dbeta, (hipStream_t)stream);
}
int mmdeer_calibration_loss(const float* gamma, const float* alpha, const float* beta, const float* targets, long long n,
                            float* loss_out, int32_t* bin_counts, float* dgamma, float* dalpha, float* dbeta, void* stream) {
  MMDEER_CHECK(gamma && alpha && beta && targets && loss_out, "calibration_loss: NULL argument");
  MMDEER_CHECK(n > 0, "calibration_loss: n must be > 0 (got %lld)", n);
  const int ng = (dgamma != nullptr) + (dalpha != nullptr) + (dbeta != nullptr);
  MMDEER_CHECK(ng == 0 || ng == 3, "calibration_loss: pass all three gradient buffers or none");
  return launch_calibration_loss(gamma, alpha, beta, targets, n, loss_out, bin_counts, dgamma, dalpha, dbeta, nullptr, 15, (hipStream_t)stream);
}
int mmdeer_calibration_loss_bins(const float* gamma, const float* alpha, const float* beta, const float* targets, long long n,
                                 const float* edges, int n_bins, float* loss_out, int32_t* bin_counts, float* dgamma, float* dalpha,
                                 float* dbeta, void* stream) {
  MMDEER_CHECK(gamma && alpha && beta && targets && loss_out && edges, "calibration_loss_bins: NULL argument");
  MMDEER_CHECK(n > 0, "calibration_loss_bins: n must be > 0 (got %lld)", n);
  const int ng = (dgamma != nullptr) + (dalpha != nullptr) + (dbeta != nullptr);
  MMDEER_CHECK(ng == 0 || ng == 3, "calibration_loss_bins: pass all three gradient buffers or none");
  return launch_calibration_loss(gamma, alpha, beta, targets, n, loss_out, bin_counts, dgamma, dalpha, dbeta, edges, n_bins, (hipStream_t)stream);
}

long long mmdeer_nig_stats_elems(int B) { return (long long)nig_nblocks(B) * 3 * NIG_NSTAT; }
int mmdeer_nig_loss(const float* gamma, const float* nu, const float* alpha, const float* beta, const float* targets,
                    float* stats, float* dgamma, float* dnu, float* dalpha, float* dbeta, float* loss_out,
                    int32_t* bin_counts, int B, const mmdeer_loss_cfg* c, void* stream) {
  MMDEER_CHECK(gamma && nu && alpha && beta && targets && stats && c, "nig_loss: NULL argument");
  MMDEER_CHECK((dgamma && dnu && dalpha && dbeta) || (!dgamma && !dnu && !dalpha && !dbeta),
               "nig_loss: pass all four gradient outputs or none");
  const LossCfg cfg = loss_cfg(*c);
  hipStream_t s = (hipStream_t)stream;
  TRY(launch_nig_loss_stats(gamma, nu, alpha, beta, targets, stats, B, s));
  return launch_nig_loss_grad(gamma, nu, alpha, beta, targets, stats, dgamma, dnu, dalpha, dbeta, loss_out, bin_counts, B, cfg, s);
}

int mmdeer_dropout_mask(int site, int rows, int cols, float dropout_p, uint64_t seed, uint64_t offset,
                        unsigned char* out, void* stream) {
  return mmdeer_dropout_mask_dev(site, rows, cols, dropout_p, seed, offset, out, stream, nullptr);
}
int mmdeer_dropout_mask_dev(int site, int rows, int cols, float dropout_p, uint64_t seed, uint64_t offset,
                            unsigned char* out, void* stream, const uint64_t* offset_dev) {
  MMDEER_CHECK(out != nullptr, "dropout_mask: out is NULL");
  TRY(counter_ok("dropout_mask", offset_dev));
  const DropCtx dc = make_drop(dropout_p, seed, offset, dropout_p > 0.f ? offset_dev : nullptr);     // no dropout: no step to read
  return launch_dropout_mask(dc, site, rows, cols, out, (hipStream_t)stream);
}

}  // extern "C"
namespace {
// The argument mapping of mmdeer_chain, shared with the dry run mmdeer_chain_route; returns 1 for an empty batch (nothing to do).
int chain_front(const mmdeer_chain_args* a, ChainArgs& c) {
  MMDEER_CHECK(a && a->nseg >= 1 && a->nseg <= MMDEER_CHAIN_MAX_SEGS, "mmdeer_chain: 1..%d segments", MMDEER_CHAIN_MAX_SEGS);
  MMDEER_CHECK(a->rows >= 0, "mmdeer_chain: rows");
  if (a->rows == 0) return 1;
  MMDEER_CHECK(a->samples_per_workgroup == 0 || a->samples_per_workgroup == 16 || a->samples_per_workgroup == 32, "mmdeer_chain: samples_per_workgroup must be 0, 16 or 32");
  c = ChainArgs{};
  c.X = reinterpret_cast<const bf16_t*>(a->X); c.ldx = a->ldx; c.K0 = a->K0; c.B = a->rows; c.groups = 1; c.group_stride = 0;
  c.ts = a->samples_per_workgroup;
  c.drop = make_drop(a->dropout_p, a->seed, a->offset, a->offset_dev);
  c.nseg = a->nseg;
  c.stamps = reinterpret_cast<unsigned long long*>(a->debug);
  for (int i = 0; i < a->nseg; ++i) {
    const mmdeer_chain_seg& s = a->seg[i];
    ChainSeg& q = c.seg[i];
    chain_seg_defaults(q);
    q.W = reinterpret_cast<const bf16_t*>(s.W); q.bias = s.bias; q.N = s.N; q.K = s.K; q.ldw = s.K;
    q.kin_off = s.kin_off; q.nout_off = s.nout_off; q.relu = s.relu;
    q.drop_site = a->dropout_p > 0.f ? s.drop_site : -1; q.drop_shift = s.drop_shift; q.dcol_off = s.dcol_off;
    q.mask_y = reinterpret_cast<const bf16_t*>(s.mask_y); q.ld_mask = s.ld_mask; q.mask_col0 = s.mask_col0; q.mask_scale = s.mask_scale;
    q.res_add = s.res_add; q.res_dup = s.res_dup;
    q.end_layer = s.end_layer;
    if (s.end_layer) {
      q.nout = s.nout; q.stash = reinterpret_cast<bf16_t*>(s.stash); q.ld_stash = s.ld_stash;
      q.stash2 = reinterpret_cast<bf16_t*>(s.stash2); q.stash_split = s.stash_split;
      q.gamma = s.gamma; q.beta = s.beta; q.xln = reinterpret_cast<bf16_t*>(s.xln); q.mean = s.mean; q.rstd = s.rstd; q.residual = s.residual;
      q.lnb_gamma = s.lnb_gamma; q.lnb_y = reinterpret_cast<const bf16_t*>(s.lnb_y); q.lnb_mean = s.lnb_mean; q.lnb_rstd = s.lnb_rstd;
      q.lnb_dz = reinterpret_cast<bf16_t*>(s.lnb_dz); q.lnb_partial = s.lnb_partial; q.lnb_mask_scale = s.lnb_mask_scale;
    }
  }
  return 0;
}
}  // namespace
extern "C" {

// The layer-chain kernel as an operator (include/mmdeer.h: mmdeer_chain): every row of the input is a sample.
int mmdeer_chain(const mmdeer_chain_args* a) {
  ChainArgs c;
  const int rc = chain_front(a, c);
  if (rc != 0) return rc < 0 ? -1 : 0;
  return launch_chain(c, (hipStream_t)a->stream);
}

int mmdeer_chain_route(const mmdeer_chain_args* a, char* out, int cap) {
  if (out && cap > 0) out[0] = 0;
  ChainArgs c;
  const int rc = chain_front(a, c);
  if (rc != 0) return rc < 0 ? -1 : 0;
  ChainKernel k;
  TRY(launch_chain(c, nullptr, &k));
  if (out && cap > 0) snprintf(out, cap, "%s workgroups=%d", chain_kernel_name(k), chain_workgroups(c));
  return 1;
}

int mmdeer_chain_workgroups(int rows, int samples_per_workgroup) {
  ChainArgs c{};
  c.B = rows; c.ts = samples_per_workgroup;
  const int m = chain_samples_per_workgroup(c);
  return (rows + m - 1) / m;
}

int mmdeer_repack(const mmdeer_repack_job* jobs, int n, void* stream) {
  MMDEER_CHECK(n >= 0 && (n == 0 || jobs), "mmdeer_repack: jobs");
  // REPACK_MAX jobs per launch; every job is checked before the first launch, so that a refused call writes nothing
  std::vector<RepackTable> tabs((n + REPACK_MAX - 1) / REPACK_MAX);
  for (int j = 0; j < n; ++j) {
    const mmdeer_repack_job& s = jobs[j];
    RepackTable& t = tabs[j / REPACK_MAX];
    RepackJob& J = t.job[t.njobs++];
    J.src = reinterpret_cast<const bf16_t*>(s.src); J.dst = reinterpret_cast<bf16_t*>(s.dst);
    J.ld_src = s.ld_src; J.rows = s.rows; J.cols = s.cols; J.cols_valid = s.cols_valid; J.transpose = s.transpose;
    MMDEER_CHECK(s.layout == 0 || s.layout == 1, "mmdeer_repack: job %d layout", j);
    MMDEER_CHECK(s.cols_valid >= 0 && s.ld_src >= s.cols_valid, "mmdeer_repack: job %d: ld_src = %d is shorter than cols_valid = %d", j, s.ld_src, s.cols_valid);
    MMDEER_CHECK(s.layout == 1 || (s.dst_col >= 0 && s.ld_dst >= s.dst_col + (s.transpose ? s.rows : s.cols)),
                 "mmdeer_repack: job %d: a row-major image at column %d does not fit ld_dst = %d", j, s.dst_col, s.ld_dst);
    J.layout = s.layout; J.ld_dst = s.ld_dst; J.dst_col = s.dst_col;
  }
  for (size_t b = 0; b < tabs.size(); ++b) {
    if (check_repack(tabs[b]) < 0) {
      char msg[512];
      snprintf(msg, sizeof msg, "%s", mmdeer_last_error());
      MMDEER_CHECK(false, "mmdeer_repack: jobs %d..: %s", (int)b * REPACK_MAX, msg);
    }
  }
  for (RepackTable& t : tabs) TRY(launch_repack(t, (hipStream_t)stream));
  return 0;
}

long long mmdeer_sizeof(const char* n) {
  if (!n) return -1;
#define SZ(name) if (strcmp(n, #name) == 0) return (long long)sizeof(mmdeer_##name);
  SZ(gemm_args) SZ(chain_args) SZ(chain_seg) SZ(repack_job) SZ(forward_args) SZ(backward_args) SZ(adamw_args) SZ(adamw_flat_args)
  SZ(stackb_attn_train_args) SZ(stackb_attn_args) SZ(stackb_forward_args) SZ(stackb_weights) SZ(softmax_mix_args)
  SZ(lstm_seq_args) SZ(temporal_pool_args) SZ(evidence_tail_args) SZ(token_embed_args) SZ(token_pool_args) SZ(token_stats_args)
  SZ(conv3_time_args) SZ(bn_time_args)   // mmdeer_video.h
  SZ(conv2d_args) SZ(bn2d_args)          // mmdeer_frames.h
  SZ(bn2d_bwd_args) SZ(conv2d_wgrad_args) SZ(conv2d_dgrad_args)   // mmdeer_frames_bwd.h
  SZ(bert_embed_args) SZ(bert_attn_args) SZ(bert_add_ln_args) SZ(bert_gelu_args)   // mmdeer_bert.h
  SZ(bert_attn_bwd_args) SZ(bert_add_ln_bwd_args) SZ(bert_gelu_bwd_args)   // mmdeer_bert_bwd.h
  SZ(bert_embed_drop_args) SZ(bert_attn_drop_args) SZ(bert_drop_add_ln_args) SZ(bert_attn_drop_bwd_args) SZ(bert_drop_add_ln_bwd_args)   // mmdeer_bert_drop.h
  SZ(adamw_multi_tensor) SZ(adamw_multi_class) SZ(adamw_multi_args)   // mmdeer_optim.h
  SZ(adamw_multi_class_dev) SZ(adamw_multi_dev_args)   // mmdeer_graph.h
  SZ(lstm_seq_len_args) SZ(temporal_pool_len_args)   // mmdeer_seqlen.h
#undef SZ
  return -1;
}

int mmdeer_convert(const void* src, int src_f32, void* dst, int dst_f32, long long n, void* stream) {
  return launch_convert(src, src_f32, dst, dst_f32, n, (hipStream_t)stream);
}

}  // extern "C"
