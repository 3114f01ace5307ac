// Stack C: the host-side executor that strings the gfx950 kernels into the forward / backward / optimiser step of the fusion + DEER
// path (include/mmdeer.h: mmdeer_forward, mmdeer_backward, mmdeer_adamw_step, mmdeer_pack_weights, ...), with everything that knows
// its parameters: the parameter table, the workspace / weights layout and the table of derived weight images.  Host code only: every
// function enqueues on the caller's stream and returns; nothing here allocates device memory or synchronises.
#include <cstring>

#include "../../include/mmdeer.h"
#include "attention.h"
#include "common.h"
#include "gemm.h"
#include "nig.h"
#include "optim.h"
#include "options.h"
#include "chain.h"
#include "rowops.h"

namespace mmdeer {
namespace {

// ------------------------------------------------------------------ launch trace (mmdeer_trace_begin / _end, include/mmdeer.h)
// While a trace is open on the calling thread, mmdeer_forward / mmdeer_backward record the caller's next event behind every launch
// (or group of launches) and remember its label: the host turns consecutive events into per-launch durations of ITS run.
constexpr int TRACE_MAX = 32;
struct Trace { void** ev = nullptr; int max = 0, n = 0; const char* label[TRACE_MAX]; };
thread_local Trace g_trace;
int trace_mark(const char* label, hipStream_t s) {
  Trace& t = g_trace;
  if (!t.ev || t.n >= t.max || t.n >= TRACE_MAX) return 0;
  if (hipEventRecord((hipEvent_t)t.ev[t.n], s) != hipSuccess) { set_error("trace: hipEventRecord failed"); return -1; }
  t.label[t.n++] = label;
  return 0;
}
#define MARK(label) do { if (trace_mark(label, s) != 0) return -1; } while (0)

// ------------------------------------------------------------------ parameter table
struct ParamInfo { const char* name; int rows, cols; long long off; int is_matrix; };
#define X(idx, ident, rows, cols, off, ismat, name) {name, rows, cols, off, ismat},
constexpr ParamInfo kParams[] = {
#include "params.inc"
};
#undef X
enum ParamId {
#define X(idx, ident, rows, cols, off, ismat, name) ident = idx,
#include "params.inc"
#undef X
};
static_assert(MMDEER_NUM_PARAMS == MMDEER_NUM_PARAMS_ABI, "parameter table out of sync with the public header");

// short aliases
constexpr int P_AUD_W = MMDEER_P_AUDIO_VISUAL_AUDIO_PROJECTION_WEIGHT, P_AUD_B = MMDEER_P_AUDIO_VISUAL_AUDIO_PROJECTION_BIAS;
constexpr int P_VID_W = MMDEER_P_AUDIO_VISUAL_VIDEO_PROJECTION_WEIGHT, P_VID_B = MMDEER_P_AUDIO_VISUAL_VIDEO_PROJECTION_BIAS;
constexpr int P_AIN_W = MMDEER_P_AUDIO_VISUAL_CROSS_ATTENTION_IN_PROJ_WEIGHT, P_AIN_B = MMDEER_P_AUDIO_VISUAL_CROSS_ATTENTION_IN_PROJ_BIAS;
constexpr int P_AOUT_W = MMDEER_P_AUDIO_VISUAL_CROSS_ATTENTION_OUT_PROJ_WEIGHT, P_AOUT_B = MMDEER_P_AUDIO_VISUAL_CROSS_ATTENTION_OUT_PROJ_BIAS;
constexpr int P_AVF_W = MMDEER_P_AUDIO_VISUAL_FUSION_LAYERS_0_WEIGHT, P_AVF_B = MMDEER_P_AUDIO_VISUAL_FUSION_LAYERS_0_BIAS;
constexpr int P_AVF_G = MMDEER_P_AUDIO_VISUAL_FUSION_LAYERS_3_WEIGHT, P_AVF_BT = MMDEER_P_AUDIO_VISUAL_FUSION_LAYERS_3_BIAS;
constexpr int P_AVP_W = MMDEER_P_TRIMODAL_AUDIOVISUAL_PROJECTION_WEIGHT, P_AVP_B = MMDEER_P_TRIMODAL_AUDIOVISUAL_PROJECTION_BIAS;
constexpr int P_TXT_W = MMDEER_P_TRIMODAL_TEXT_PROJECTION_WEIGHT, P_TXT_B = MMDEER_P_TRIMODAL_TEXT_PROJECTION_BIAS;
constexpr int P_TIN_W = MMDEER_P_TRIMODAL_MODALITY_ATTENTION_IN_PROJ_WEIGHT, P_TIN_B = MMDEER_P_TRIMODAL_MODALITY_ATTENTION_IN_PROJ_BIAS;
constexpr int P_TOUT_W = MMDEER_P_TRIMODAL_MODALITY_ATTENTION_OUT_PROJ_WEIGHT, P_TOUT_B = MMDEER_P_TRIMODAL_MODALITY_ATTENTION_OUT_PROJ_BIAS;
constexpr int P_TFF_W = MMDEER_P_TRIMODAL_FINAL_0_WEIGHT, P_TFF_B = MMDEER_P_TRIMODAL_FINAL_0_BIAS;
constexpr int P_TFF_G = MMDEER_P_TRIMODAL_FINAL_3_WEIGHT, P_TFF_BT = MMDEER_P_TRIMODAL_FINAL_3_BIAS;
constexpr int P_OP_W = MMDEER_P_OUTP0_WEIGHT, P_OP_B = MMDEER_P_OUTP0_BIAS, P_OP_G = MMDEER_P_OUTP3_WEIGHT, P_OP_BT = MMDEER_P_OUTP3_BIAS;
constexpr int P_FP0_W = MMDEER_P_FP0_WEIGHT, P_FP0_B = MMDEER_P_FP0_BIAS, P_FP1_W = MMDEER_P_FP3_WEIGHT, P_FP1_B = MMDEER_P_FP3_BIAS;
constexpr int P_EV0_W = MMDEER_P_HEAD0_EV0_WEIGHT, P_EV0_B = MMDEER_P_HEAD0_EV0_BIAS;
constexpr int P_EV1_W = MMDEER_P_HEAD0_EV3_WEIGHT, P_EV1_B = MMDEER_P_HEAD0_EV3_BIAS;
constexpr int P_EV2_W = MMDEER_P_HEAD0_EV6_WEIGHT, P_EV2_B = MMDEER_P_HEAD0_EV6_BIAS;

constexpr int AUD = MMDEER_AUDIO_DIM, VID = MMDEER_VIDEO_DIM, TXT = MMDEER_TEXT_DIM, INTER = MMDEER_INTER_DIM;
constexpr int FUS = MMDEER_FUSION_DIM, HID = MMDEER_HIDDEN_DIM, EV1 = 128, EV2 = 64;
constexpr int SPLITK_MAX = 8;
constexpr int AUD_PAD = 128;   // the 84 audio features padded to a K-tile multiple for the LDS-DMA kernels

// ------------------------------------------------------------------ workspace / weights layout (layout.inc)
struct Layout {
  using ACT = char; using BF16 = char; using F32 = float;   // what a pointer to each element kind points to
#define X(buf, kind, name, elems, bf16_only) kind* name;
#include "layout.inc"
#undef X
  size_t wbytes;     // size of the weights buffer
  size_t bytes;      // size of the workspace
};

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

Layout make_layout(void* base, void* wbase, int B, int f32) {
  Layout L{};
  const size_t size_ACT = f32 ? 4 : 2, size_BF16 = 2, size_F32 = 4;
  const size_t Bz = (size_t)(B > 0 ? B : 1), nblk = (size_t)nig_nblocks(B);
  // LayerNorm-backward partial slabs: one per workgroup of ln_bwd_kernel, or of the layer chain that ran instead (more above 8192)
  const size_t np = (size_t)(ln_bwd_nparts(B) > chain_workgroups_max(B) ? ln_bwd_nparts(B) : chain_workgroups_max(B));
  const size_t nhead = nblk > (size_t)chain_workgroups_max(B) ? nblk : (size_t)chain_workgroups_max(B);   // nig_bwd_kernel's blocks, or the chain's workgroups
  char* const base_W = reinterpret_cast<char*>(wbase);
  char* const base_S = reinterpret_cast<char*>(base);
  size_t off_W = 0, off_S = 0;
#define X(buf, kind, name, elems, bf16_only)                                                      \
  L.name = reinterpret_cast<Layout::kind*>(base_##buf ? base_##buf + off_##buf : nullptr);        \
  off_##buf += align_up((bf16_only) && f32 ? 0 : (size_t)(elems) * size_##kind);
#include "layout.inc"
#undef X
  L.wbytes = off_W;
  L.bytes = off_S;
  return L;
}

// byte offset of the field `name` of buffer `buf` ('W' / 'S'), -1 for a name that buffer does not have
long long layout_offset(char buf, int batch, int f32, const char* name) {
  if (!name || batch < 0) return -1;
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);   // any non-null base: only differences are returned
  const Layout L = make_layout(base, base, batch, f32);
#define X(b, kind, field, elems, bf16_only) \
  if (buf == #b[0] && strcmp(name, #field) == 0) return reinterpret_cast<const char*>(L.field) - base;
#include "layout.inc"
#undef X
  return -1;
}

// ------------------------------------------------------------------ derived weight images
// Which bf16 images of which matrix the kernels read besides the packed row-major copy in L.wpack -- stated ONCE, here, per row range
// of a parameter; repack_images (from the packed bf16 copy), pack_transposed_weights (fp32 mode: only the W^T copies exist) and the
// image table of the fused optimiser step (mmdeer_adamw_step) each lower this table to their launch's descriptors.
enum : unsigned {
  IMG_FRAG = 1,    // L.wfpack: fragment-major image (chain.h) of the matrix S the forward chains stream
  IMG_FRAGT = 2,   // L.wtfpack: fragment-major image of S^T (the backward chains)
  IMG_WT = 4,      // L.wtpack: row-major W^T, which the dX GEMMs multiply by.  Absent where no dX is needed: the three input projections
                   // and the heads' last layers (not in the table at all: the NIG kernels read them from L.wpack)
  IMG_PAD = 8,     // L.wa_pad: the rows zero-padded to AUD_PAD columns, and L.wa_frag: the fragment-major image of that (whole matrix only)
  IMG_HM = 16,     // L.wqkv_hm: the rows in tri_fused.hip's head-major order (the whole [1536][512] in_proj only)
  IMG_CHAIN = IMG_FRAG | IMG_FRAGT | IMG_WT,   // a layer of the forward and backward chains
};
struct ImageRange {
  int pid, row0, rows;          // rows [row0, row0 + rows) of parameter pid; the ranges of a parameter cover all its rows
  unsigned img;                 // IMG_* set
  int s_pid, s_row0, s_rows;    // IMG_FRAG / IMG_FRAGT: S = s_rows rows from row s_row0 of parameter s_pid on (stacked parameters follow each
                                // other in the flat buffer), at the flat offset of its first element in L.wfpack / L.wtfpack
  int wt_pid, wt_ld;            // IMG_WT: the range is columns of the [cols][wt_ld] matrix at parameter wt_pid's flat offset in L.wtpack
  constexpr int cols() const { return kParams[pid].cols; }
  constexpr long long off() const { return kParams[pid].off + (long long)row0 * cols(); }              // flat offset of the range
  constexpr long long s_off() const { return kParams[s_pid].off + (long long)s_row0 * cols(); }        // ... of S
  constexpr int s_row() const { return (int)((off() - s_off()) / cols()); }                            // the range's first row in S
  constexpr int wt_col() const { return (int)((off() - kParams[wt_pid].off) / cols()); }               // its first column in W^T
};
constexpr ImageRange whole(int pid, unsigned img) {   // a matrix on its own
  return {pid, 0, kParams[pid].rows, img, pid, 0, kParams[pid].rows, pid, kParams[pid].rows};
}
constexpr ImageRange stacked(int pid, int first, int n, unsigned img) {   // one of n equal parameters from `first` on that the kernels read as ONE matrix
  return {pid, 0, kParams[pid].rows, img, first, 0, n * kParams[pid].rows, first, n * kParams[pid].rows};
}
constexpr ImageRange kImages[] = {
    whole(P_AUD_W, IMG_PAD),
    whole(P_VID_W, IMG_FRAG),
    // the AV in_proj [q; k; v]: the attention has one key per query, so only the value rows are ever multiplied by (the chains' matrix);
    // the query / key rows exist in the W^T copy alone
    {P_AIN_W, 0, 2 * INTER, IMG_WT, P_AIN_W, 0, 3 * INTER, P_AIN_W, 3 * INTER},
    {P_AIN_W, 2 * INTER, INTER, IMG_CHAIN, P_AIN_W, 2 * INTER, INTER, P_AIN_W, 3 * INTER},
    whole(P_AOUT_W, IMG_CHAIN), whole(P_AVF_W, IMG_CHAIN), whole(P_AVP_W, IMG_CHAIN),
    whole(P_TXT_W, IMG_FRAG),
    whole(P_TIN_W, IMG_HM | IMG_WT),   // tri_fused.hip + the in_proj dX GEMM
    whole(P_TOUT_W, IMG_CHAIN), whole(P_TFF_W, IMG_CHAIN), whole(P_OP_W, IMG_CHAIN), whole(P_FP0_W, IMG_CHAIN), whole(P_FP1_W, IMG_CHAIN),
    // the three first head layers: one stacked [384][256] matrix for the kernels, three parameters for the optimiser
    stacked(P_EV0_W, P_EV0_W, 3, IMG_CHAIN), stacked(P_EV0_W + 1, P_EV0_W, 3, IMG_CHAIN), stacked(P_EV0_W + 2, P_EV0_W, 3, IMG_CHAIN),
    whole(P_EV1_W, IMG_CHAIN), whole(P_EV1_W + 1, IMG_CHAIN), whole(P_EV1_W + 2, IMG_CHAIN),   // second head layers [64][128], each on its own
};
constexpr int kNumImages = sizeof(kImages) / sizeof(kImages[0]);
static_assert(kNumImages <= ADAM_MAX_IMAGED, "the fused optimiser step takes one AdamImaged per range");

// the forward head chain ends in the NIG head (option chain_nigf): the loss statistics in the workspace are wave partials then.
// Forward, backward and mmdeer_loss_stats of one step must agree on it: it depends on the options and the batch size only.
bool nig_tail_plan(int B, int f32) {
  return !f32 && opt(OPT_CHAIN) && opt(OPT_CHAIN_NIGF) && B >= opt(OPT_CHAIN_MIN) && B <= opt(OPT_CHAIN_MAX);
}

// Builder for the executor's GEMM problems.  `es` = bytes of one activation element.
struct Exec {
  int B, f32;
  int slice_div = 1; // > 1: weight-gradient K-slices this many times shorter (a launch with few problems: see mmdeer_backward phase 2)
  size_t es;
  bool drop_on;      // dropout active
  float mask_scale;  // 1/(1-p) when dropout is active, else 1
  DropCtx dc;
  const Layout* L;
  hipStream_t s;

  const char* W(int pid) const { return L->wpack + (size_t)kParams[pid].off * es; }
  const float* V(int pid) const { return L->vpack + kParams[pid].off; }

  // Y = X W^T + b: activations in, activations out
  GemmProblem fwd(const void* A, int a_f32, int lda, int pidW, int pidB, void* C, int ldc, int M, int relu, int site) const {
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = A; p.a_f32 = a_f32; p.lda = lda;
    p.B = W(pidW); p.b_f32 = f32; p.ldb = kParams[pidW].cols;
    p.C = C; p.c_f32 = f32; p.ldc = ldc;
    p.bias = V(pidB);
    p.M = M; p.N = kParams[pidW].rows; p.K = kParams[pidW].cols;
    p.relu = relu;
    p.drop_site = drop_on ? site : -1;
    return p;
  }
  // dX = dY W, optionally masked by (Yprev > 0) * mask_scale.  Runs as an NT GEMM against the packed W^T
  // ([K_layer][N_layer], reduction-contiguous), i.e. on the LDS-DMA kernel in bf16 mode.
  const char* WT(int pid) const { return L->wtpack + (size_t)kParams[pid].off * es; }
  // fragment-major images of W / W^T for the layer chains (bf16 mode; kImages above says which exist)
  const bf16_t* WF(int pid, size_t elem_off = 0) const { return reinterpret_cast<const bf16_t*>(L->wfpack) + kParams[pid].off + elem_off; }
  const bf16_t* WTF(int pid, size_t elem_off = 0) const { return reinterpret_cast<const bf16_t*>(L->wtfpack) + kParams[pid].off + elem_off; }
  GemmProblem dx(const void* dY, int ldy_in, int pidW, void* dX, int ldx, int M, const void* Ymask, int ldmask) const {
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = dY; p.a_f32 = f32; p.lda = ldy_in;
    p.B = WT(pidW); p.b_f32 = f32; p.ldb = kParams[pidW].rows;
    p.C = dX; p.c_f32 = f32; p.ldc = ldx;
    p.M = M; p.N = kParams[pidW].cols; p.K = kParams[pidW].rows;
    p.Y = Ymask; p.y_f32 = f32; p.ldy = ldmask; p.mask_scale = mask_scale;
    return p;
  }
  // dW = dY^T X (+ db = column sums of dY), written into the flat gradient buffer.  The reduction runs over the
  // batch (K = Mred rows): it is split into K-slices of ~ksteps_target() K-tiles whose partials go to the slab.
  GemmProblem dw(const void* dY, int ldy_in, const void* X, int x_f32, int ldx, int pidW, int pidB, float* grads, int Mred) const {
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = dY; p.a_f32 = f32; p.lda = ldy_in; p.trans_a = 1;
    p.B = X; p.b_f32 = x_f32; p.ldb = ldx; p.trans_b = 1;
    p.C = grads + kParams[pidW].off; p.c_f32 = 1; p.ldc = kParams[pidW].cols;
    p.bias_grad = grads + kParams[pidB].off;
    p.M = kParams[pidW].rows; p.N = kParams[pidW].cols; p.K = Mred;
    set_split(p, grads);
    return p;
  }
  // (re)derive the split-K fields from p.K and the final destinations p.C / p.bias_grad
  void set_split(GemmProblem& p, float* grads) const {
    const int nk = gemm_ktiles(p.K, f32);
    int kst = ksteps_target(f32);
    // 128x128 weight-gradient tiles (option dw_tile = 2, the default): K-slices of B rows -- the B-row problems run their whole
    // reduction in one workgroup (no slab, nothing to fold), the 2B-row ones (trimodal in_proj, the stacked AV calls) get two
    // slices as long as the others' one.  Measured against other slice lengths at B = 512 ... 16384.
    if (!f32 && opt(OPT_DW_TILE) == 2 && opt(OPT_KSTEPS) == 0) { kst = B / 64 / slice_div; kst = kst < 4 ? 4 : kst > 128 ? 128 : kst; }
    int sk = (nk + kst - 1) / kst;
    const int cap = opt(OPT_SPLITK_MAX) < SPLITK_MAX ? opt(OPT_SPLITK_MAX) : SPLITK_MAX;
    if (sk > cap) sk = cap;
    if (sk < 1) sk = 1;
    p.splitk = sk;
    p.slab_stride = MMDEER_FLAT_ELEMS;
    p.slab_c = L->slab + (reinterpret_cast<float*>(p.C) - grads);
    p.slab_b = p.bias_grad ? L->slab + (p.bias_grad - grads) : nullptr;
  }
  // segments that fold a split-K problem's slabs into its final destinations
  // The counts round up to 4 (the fold's f32x4 granule) without reading or writing past C / bias_grad: every problem of the
  // backward has M, N, ldc and batch strides multiples of 4 (the group launcher refuses a transposed A with M % 4, and any
  // N % 4) and Stack C's parameter table (params.inc) has no size or offset that is not, so the rounding is exact.
  static void add_slab_segments(ReduceTable& t, const GemmProblem& p) {
    if (p.splitk <= 1) return;
    const long long csz = (long long)(p.batch - 1) * p.sC + (long long)(p.M - 1) * p.ldc + p.N;   // extent of C incl. batches
    int k = t.nseg;
    t.src[k] = p.slab_c; t.dst[k] = reinterpret_cast<float*>(p.C); t.nparts[k] = p.splitk;
    t.n[k] = (int)((csz + 3) / 4 * 4); t.stride[k] = p.slab_stride; ++k;
    if (p.bias_grad) {
      const long long bsz = (long long)(p.batch - 1) * p.sBiasGrad + p.M;
      t.src[k] = p.slab_b; t.dst[k] = p.bias_grad; t.nparts[k] = p.splitk;
      t.n[k] = (int)((bsz + 3) / 4 * 4); t.stride[k] = p.slab_stride; ++k;
    }
    t.nseg = k;
  }
  int run(GemmGroup& g) const {
    g.drop = dc;
    return launch_gemm_group(g, f32, pick_tile(g), s);
  }
  int run1(const GemmProblem& p) const {
    GemmGroup g{};
    g.nprob = 1;
    g.p[0] = p;
    return run(g);
  }
};

int check_weights(const void* w, size_t w_bytes, int f32) {
  MMDEER_CHECK(w != nullptr, "weights buffer is NULL");
  MMDEER_CHECK(((uintptr_t)w % 256) == 0, "weights buffer must be 256-byte aligned");
  const size_t need = mmdeer_weights_bytes(f32);
  MMDEER_CHECK(w_bytes >= need, "weights buffer too small: %zu bytes given, %zu needed", w_bytes, need);
  return 0;
}
int check_common(int batch, const void* ws, size_t ws_bytes, const void* w, size_t w_bytes, int f32) {
  MMDEER_CHECK(batch >= 0, "batch must be >= 0 (got %d)", batch);
  MMDEER_CHECK(ws != nullptr, "workspace is NULL");
  MMDEER_CHECK(((uintptr_t)ws % 256) == 0, "workspace must be 256-byte aligned");
  const size_t need = mmdeer_workspace_bytes(batch, f32);
  MMDEER_CHECK(ws_bytes >= need, "workspace too small: %zu bytes given, %zu needed for batch %d", ws_bytes, need, batch);
  return check_weights(w, w_bytes, f32);
}

// ------------------------------------------------------------------ packing the parameters into L (the `weights` buffer)
// fp32 mode: the W^T copies (compute dtype) of the matrices whose dX the backward needs, from the fp32 parameters
int pack_transposed_weights(const void* const* params, const Layout& L, int f32, hipStream_t s) {
  PackTTable tt{};
  for (const ImageRange& r : kImages) {
    if (!(r.img & IMG_WT)) continue;
    const int k = tt.nmat++;
    tt.src[k] = reinterpret_cast<const float*>(params[r.pid]) + (long long)r.row0 * r.cols();
    tt.dst_off[k] = kParams[r.wt_pid].off;
    tt.rows[k] = r.rows; tt.cols[k] = r.cols();
    tt.ld_dst[k] = r.wt_ld; tt.dst_col[k] = r.wt_col();
  }
  return launch_pack_transposed(tt, L.wtpack, f32, s);
}

// bf16 mode: EVERY derived image of the packed weights in ONE launch (chain.h: launch_repack), all from L.wpack -- the bf16 copies
// the optimiser step or the parameter pack has just written.  Neighbouring ranges that are rows of the same image become one job
// (the stacked head layers; the two row ranges of the AV in_proj in its W^T copy).
int repack_images(const Layout& L, bool with_transposed, hipStream_t s) {
  RepackTable t{};
  const bf16_t* wp = reinterpret_cast<const bf16_t*>(L.wpack);
  // S = `rows` rows of `cols_valid` columns at flat offset src_off, zero-padded to `cols` columns
  auto job = [&](long long src_off, int rows, int cols_valid, int cols, int transpose, int layout, char* dst_base, long long dst_off,
                 int ld_dst = 0, int dst_col = 0) {
    RepackJob& J = t.job[t.njobs++];
    J.src = wp + src_off; J.ld_src = cols_valid; J.rows = rows; J.cols = cols; J.cols_valid = cols_valid;
    J.transpose = transpose; J.layout = layout;
    J.dst = reinterpret_cast<bf16_t*>(dst_base) + dst_off; J.ld_dst = ld_dst; J.dst_col = dst_col;
  };
  auto for_runs = [&](unsigned kind, auto emit) {
    for (int i = 0, j; i < kNumImages; i = j) {
      const ImageRange& a = kImages[i];
      j = i + 1;
      if (!(a.img & kind)) continue;
      int rows = a.rows;
      for (; j < kNumImages; rows += kImages[j++].rows) {
        const ImageRange& b = kImages[j];
        const bool same = kind == IMG_WT ? (b.wt_pid == a.wt_pid && b.wt_ld == a.wt_ld) : (b.s_pid == a.s_pid && b.s_row0 == a.s_row0 && b.s_rows == a.s_rows);
        if (!(b.img & kind) || !same || b.off() != a.off() + (long long)rows * a.cols()) break;
      }
      emit(a, rows);
    }
  };
  // the fragment-major image of S is row-tile major: rows [r, r + n) of S are the image of those rows alone, n K elements from r K on
  for_runs(IMG_FRAG, [&](const ImageRange& a, int rows) { job(a.off(), rows, a.cols(), a.cols(), 0, 1, L.wfpack, a.off()); });
  for (const ImageRange& r : kImages) {
    if (r.img & IMG_PAD) {      // [256][84] -> [256][128]
      job(r.off(), r.rows, r.cols(), AUD_PAD, 0, 0, L.wa_pad, 0, AUD_PAD, 0);
      job(r.off(), r.rows, r.cols(), AUD_PAD, 0, 1, L.wa_frag, 0);
    }
    if (r.img & IMG_HM) job(r.off(), r.rows, r.cols(), r.cols(), 0, 2, L.wqkv_hm, 0, r.cols(), 0);
  }
  if (with_transposed) {
    // W^T copies (what pack_transposed_weights writes in fp32 mode): [cols of W][rows of W]
    for_runs(IMG_WT, [&](const ImageRange& a, int rows) { job(a.off(), rows, a.cols(), a.cols(), 1, 0, L.wtpack, kParams[a.wt_pid].off, a.wt_ld, a.wt_col()); });
    // fragment-major images of S^T (N' = cols of S, K' = rows of S): the rows of S interleave there, so a job is all of S
    bool whole_s = true;
    for_runs(IMG_FRAGT, [&](const ImageRange& a, int rows) {
      whole_s = whole_s && rows == a.s_rows;
      job(a.off(), rows, a.cols(), a.cols(), 1, 1, L.wtfpack, a.s_off());
    });
    MMDEER_CHECK(whole_s, "image table: the ranges of a matrix with a fragment-major W^T image must be neighbours and cover it");
  }
  return launch_repack(t, s);
}

// fp32 parameters -> L.wpack / L.vpack and every derived image.  The W^T copies for the backward dX GEMMs always, not only when the
// caller trains: a caller skips the pack while the parameters are unchanged, so an inference call followed by a training call on
// the same parameters would find them missing (the backward pass then multiplied by whatever the buffer held)
int pack_params(const void* const* params, const Layout& L, int f32, hipStream_t s) {
  PackTable t{};
  t.nseg = MMDEER_NUM_PARAMS;
  for (int i = 0; i < MMDEER_NUM_PARAMS; ++i) {
    t.src[i] = reinterpret_cast<const float*>(params[i]);
    t.dst_off[i] = kParams[i].off;
    t.n[i] = kParams[i].rows * kParams[i].cols;
    t.is_vec[i] = kParams[i].is_matrix ? 0 : 1;
  }
  TRY(launch_pack_params(t, L.wpack, f32, L.vpack, s));
  if (f32) return pack_transposed_weights(params, L, f32, s);
  return repack_images(L, true, s);       // bf16: W^T, fragment-major, head-major and padded images in one launch
}
// `who`: the entry point's prefix of the message
int check_params(const void* const* params, const char* who) {
  for (int i = 0; i < MMDEER_NUM_PARAMS; ++i)
    MMDEER_CHECK(params[i] != nullptr && ((uintptr_t)params[i] % 16) == 0, "%s: params[%d] (%s) must be non-NULL and 16-byte aligned", who, i, kParams[i].name);
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_num_params(void) { return MMDEER_NUM_PARAMS; }
const char* mmdeer_param_name(int i) { return (i >= 0 && i < MMDEER_NUM_PARAMS) ? kParams[i].name : ""; }
int mmdeer_param_rows(int i) { return (i >= 0 && i < MMDEER_NUM_PARAMS) ? kParams[i].rows : -1; }
int mmdeer_param_cols(int i) { return (i >= 0 && i < MMDEER_NUM_PARAMS) ? kParams[i].cols : -1; }
long long mmdeer_param_offset(int i) { return (i >= 0 && i < MMDEER_NUM_PARAMS) ? kParams[i].off : -1; }
long long mmdeer_flat_elems(void) { return MMDEER_FLAT_ELEMS; }

size_t mmdeer_workspace_bytes(int batch, int compute_f32) { return make_layout(nullptr, nullptr, batch, compute_f32).bytes; }
size_t mmdeer_weights_bytes(int compute_f32) { return make_layout(nullptr, nullptr, 0, compute_f32).wbytes; }
long long mmdeer_workspace_offset(int batch, int compute_f32, const char* name) { return layout_offset('S', batch, compute_f32 ? 1 : 0, name); }
long long mmdeer_weights_offset(int compute_f32, const char* name) { return layout_offset('W', 0, compute_f32 ? 1 : 0, name); }

int mmdeer_trace_begin(void** events, int n_events) {
  MMDEER_CHECK(events != nullptr && n_events > 0, "trace_begin: no events");
  g_trace = Trace{};
  g_trace.ev = events; g_trace.max = n_events;
  return 0;
}
int mmdeer_trace_end(void) { const int n = g_trace.n; g_trace.ev = nullptr; return n; }
const char* mmdeer_trace_label(int i) { return (i >= 0 && i < g_trace.n && i < TRACE_MAX) ? g_trace.label[i] : ""; }

long long mmdeer_bucket_begin(int b) {
  switch (b) { case 0: return kParams[P_FP0_W].off; case 1: return kParams[P_AVP_W].off; case 2: return 0; default: return -1; }
}
long long mmdeer_bucket_end(int b) {
  switch (b) { case 0: return MMDEER_FLAT_ELEMS; case 1: return kParams[P_FP0_W].off; case 2: return kParams[P_AVP_W].off; default: return -1; }
}

int mmdeer_forward(const mmdeer_forward_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  const int B = a->batch, f32 = a->compute_f32 ? 1 : 0;
  TRY(check_common(B, a->workspace, a->workspace_bytes, a->weights, a->weights_bytes, f32));
  MMDEER_CHECK(!(f32 && a->inputs_bf16), "bf16 inputs need compute_f32 = 0");
  MMDEER_CHECK(a->dropout_p >= 0.f && a->dropout_p < 1.f, "dropout_p must be in [0,1) (got %f)", a->dropout_p);
  MMDEER_CHECK(!(a->bump_offset_dev && (f32 || B == 0)), "bump_offset_dev needs bf16 compute and a non-empty batch");
  hipStream_t s = (hipStream_t)a->stream;
  const Layout L = make_layout(a->workspace, a->weights, B, f32);
  if (a->repack) {
    MMDEER_CHECK(a->params != nullptr, "params is NULL");
    for (int i = 0; i < MMDEER_NUM_PARAMS; ++i) {
      MMDEER_CHECK(a->params[i] != nullptr, "params[%d] (%s) is NULL", i, kParams[i].name);
      MMDEER_CHECK(((uintptr_t)a->params[i] % 16) == 0, "params[%d] (%s) must be 16-byte aligned", i, kParams[i].name);
    }
    TRY(pack_params(a->params, L, f32, s));
  }
  if (B == 0) return 0;
  MMDEER_CHECK(a->audio && a->video && a->text, "audio / video / text must be non-NULL");
  MMDEER_CHECK(a->nig_out != nullptr, "nig_out is NULL");

  Exec X;
  X.B = B; X.f32 = f32; X.es = f32 ? 4 : 2; X.L = &L; X.s = s;
  X.drop_on = a->training && a->dropout_p > 0.f;
  // The device-side dropout step counter (HIP-graph replays) is advanced by the LAST kernel of the STEP (the fold at the end of
  // mmdeer_backward, which draws no mask): with bump_offset_dev every kernel of the forward and of the backward adds the pending 1
  // to the host-side offset -- the same effective offset everywhere, and no kernel has to exist just to bump the counter (round 3:
  // the pad launch in front of the first mask; the chains took that launch away).
  const bool bump = a->bump_offset_dev && a->offset_dev;
  X.dc = make_drop(a->dropout_p, a->seed, a->offset + (bump ? 1 : 0), a->offset_dev);
  X.mask_scale = X.drop_on ? X.dc.scale : 1.f;
  const int in_f32 = a->inputs_bf16 ? 0 : 1;
  const size_t es = X.es;
  const bool chains = !f32 && opt(OPT_CHAIN) && B >= opt(OPT_CHAIN_MIN) && B <= opt(OPT_CHAIN_MAX);
  // The input chain: with bf16 feature blocks and 16-sample chain workgroups (B <= 4096) the three input projections run as the
  // first two layers of the audio-visual chain below -- the workgroup reads its samples' text, video and raw 84-wide audio rows
  // itself (padding the audio rows in LDS and leaving the padded copy for the weight-gradient launch): no pad launch, no F1 launch.
  const bool in_chain = chains && opt(OPT_CHAIN_IN) && !in_f32 && chain_samples_per_workgroup(B) == 16;
  const bool nig_tail = nig_tail_plan(B, f32);

  // F0 (bf16 mode): 84-wide rows are not 16-byte aligned -- zero-pad the audio block to 128 columns so that it runs on the
  //     LDS-DMA kernels
  if (!f32 && !in_chain) {
    PadTable pt{};
    pt.src[0] = a->audio; pt.dst[0] = L.audio_pad; pt.src_f32[0] = in_f32; pt.rows[0] = B; pt.cols[0] = AUD; pt.ld_dst[0] = AUD_PAD;
    pt.nseg = 1;
    TRY(launch_pad_cols(pt, s));
    MARK("pad_cols (audio 84 -> 128)");
  }
  // F1: the three input projections (fusion.py:236-237, 322) in one launch
  if (!in_chain) {
    GemmGroup g{};
    g.nprob = 3;
    g.p[0] = X.fwd(a->video, in_f32, VID, P_VID_W, P_VID_B, L.avin, INTER, B, 0, -1);                       // rows [0,B)
    g.p[1] = X.fwd(a->audio, in_f32, AUD, P_AUD_W, P_AUD_B, L.avin + (size_t)B * INTER * es, INTER, B, 0, -1); // rows [B,2B)
    if (!f32) {
      g.p[1].A = L.audio_pad; g.p[1].a_f32 = 0; g.p[1].lda = AUD_PAD;
      g.p[1].B = L.wa_pad; g.p[1].ldb = AUD_PAD; g.p[1].K = AUD_PAD;
    }
    g.p[2] = X.fwd(a->text, in_f32, TXT, P_TXT_W, P_TXT_B, L.xtok + (size_t)FUS * es, 2 * FUS, B, 0, -1);     // token 1
    TRY(X.run(g));
    MARK("F1 input projections (3 problems)");
  }
  // bf16 mode: each LayerNorm runs inside the GEMM that consumes it (gemm_ln.hip: the workgroup of a 64-row tile owns whole
  // rows of its A operand, K = the LayerNorm width) -- three launches fewer in the forward; option "ln_fused" = 0 restores
  // the stand-alone LayerNorm kernel
  const bool lnf = !f32 && opt(OPT_LN_FUSED);
  auto ln_gemm = [&](const GemmProblem& q, const void* Y, int pidG, int pidBt, void* xln, float* out32, float* mean, float* rstd) -> int {
    GemmGroup g{};
    g.nprob = 1;
    g.p[0] = q;
    g.drop = X.dc;
    return launch_gemm_ln(g, Y, X.V(pidG), X.V(pidBt), xln, out32, mean, rstd, s);
  };
  // one workgroup per 16 samples (32 above B = 4096), each streaming all weights of its chain -- a fixed 25-45 us per chain
  // whatever the batch: worth it while the chip holds all workgroups at once and most CUs have one (measured per step: B = 4096
  // -5 to -15 us depending on the box, 3072 -4 us, 2048 0, 1024 +1 us, 64 +12 us; 16-sample workgroups in two rounds at 8192:
  // +9 us, 32-sample workgroups: see DESIGN.md)
  // F2-F6 are local to a sample (the AV "attention" has one key per query: softmax == 1, only the value and output projections
  // remain): in bf16 mode ONE launch walks them with the rows resident in LDS (chain.hip).  A workgroup holds the video and the
  // audio row of its 16 samples as two row groups; torch.cat of the two attention outputs is a re-view of the panel.
  if (chains) {
    ChainArgs c{};
    c.X = reinterpret_cast<const bf16_t*>(L.avin); c.ldx = INTER; c.K0 = INTER; c.B = B; c.groups = 2; c.group_stride = B;
    c.drop = X.dc;
    int k = 0;
    if (in_chain) {
      c.X = reinterpret_cast<const bf16_t*>(a->text); c.ldx = TXT; c.K0 = TXT; c.groups = 1;
      c.aux_video = reinterpret_cast<const bf16_t*>(a->video); c.aux_ldv = VID;
      c.aux_audio = reinterpret_cast<const bf16_t*>(a->audio); c.aux_lda = AUD;
      c.aux_audio_pad = reinterpret_cast<bf16_t*>(L.audio_pad);
      {   // F1c: text_projection -> token 1 of xtok (fusion.py:322, 325)
        ChainSeg q;
        chain_seg_defaults(q);
        q.W = X.WF(P_TXT_W); q.bias = X.V(P_TXT_B); q.N = FUS; q.K = TXT;
        q.end_layer = 1; q.nout = FUS; q.stash = reinterpret_cast<bf16_t*>(L.xtok) + FUS; q.ld_stash = 2 * FUS;
        c.seg[k++] = q;
      }
      {   // F1a: video_projection -> rows [0, B) of the stacked attention input (fusion.py:237)
        ChainSeg q;
        chain_seg_defaults(q);
        q.W = X.WF(P_VID_W); q.bias = X.V(P_VID_B); q.N = INTER; q.K = VID; q.in_aux = 1; q.kin_off = 0;
        c.seg[k++] = q;
      }
      {   // F1b: audio_projection on the padded rows -> rows [B, 2B) (fusion.py:236)
        ChainSeg q;
        chain_seg_defaults(q);
        q.W = reinterpret_cast<const bf16_t*>(L.wa_frag); q.bias = X.V(P_AUD_B); q.N = INTER; q.K = AUD_PAD; q.in_aux = 1; q.kin_off = VID;
        q.row_group = 1;
        q.end_layer = 1; q.nout = INTER; q.stash = reinterpret_cast<bf16_t*>(L.avin); q.ld_stash = INTER;
        c.seg[k++] = q;
      }
    }
    {   // F2: value projection (rows [2E, 3E) of the packed in_proj), attention-weight dropout = one decision per (row, head)
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WF(P_AIN_W, (size_t)2 * INTER * INTER); q.bias = X.V(P_AIN_B) + 2 * INTER;
      q.N = INTER; q.K = INTER; q.ldw = INTER;
      q.drop_site = X.drop_on ? SITE_AV_ATTN : -1; q.drop_shift = 5;
      q.end_layer = 1; q.nout = INTER; q.stash = reinterpret_cast<bf16_t*>(L.avv); q.ld_stash = INTER;
      c.seg[k++] = q;
    }
    {   // F3: out_proj of both calls; group z lands in columns [256 z, 256 z + 256) of cat (fusion.py:262)
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WF(P_AOUT_W); q.bias = X.V(P_AOUT_B); q.N = INTER; q.K = INTER; q.ldw = INTER;
      q.fold_groups = 1;
      q.end_layer = 1; q.nout = 2 * INTER; q.stash = reinterpret_cast<bf16_t*>(L.cat); q.ld_stash = 2 * INTER;
      c.seg[k++] = q;
    }
    {   // F4-F5: fusion_layers = Linear -> ReLU -> Dropout -> LayerNorm (fusion.py:263)
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WF(P_AVF_W); q.bias = X.V(P_AVF_B); q.N = INTER; q.K = 2 * INTER; q.ldw = 2 * INTER;
      q.relu = 1; q.drop_site = X.drop_on ? SITE_AV_FUSE : -1;
      q.end_layer = 1; q.nout = INTER; q.stash = reinterpret_cast<bf16_t*>(L.y_a2); q.ld_stash = INTER;
      q.gamma = X.V(P_AVF_G); q.beta = X.V(P_AVF_BT); q.xln = reinterpret_cast<bf16_t*>(L.av); q.out32 = a->audiovisual_features;
      q.mean = L.mean_a2; q.rstd = L.rstd_a2;
      c.seg[k++] = q;
    }
    {   // F6: audiovisual_projection -> token 0 (fusion.py:321, 325)
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WF(P_AVP_W); q.bias = X.V(P_AVP_B); q.N = FUS; q.K = INTER; q.ldw = INTER;
      q.end_layer = 1; q.nout = FUS; q.stash = reinterpret_cast<bf16_t*>(L.xtok); q.ld_stash = 2 * FUS;
      c.seg[k++] = q;
    }
    c.nseg = k;
    TRY(launch_chain(c, s));
    MARK(in_chain ? "chain F1-F6 (input projections + audio-visual fusion)" : "chain F2-F6 (audio-visual fusion)");
  } else {
    // F2: value projection of the shared AV cross-attention on [video_proj; audio_proj] (fusion.py:244-255;
    //     L = S = 1 so q/k are dead), attention-weight dropout = one decision per (row, head)
    {
      GemmProblem p = X.fwd(L.avin, f32, INTER, P_AIN_W, P_AIN_B, L.avv, INTER, 2 * B, 0, SITE_AV_ATTN);
      p.B = X.W(P_AIN_W) + (size_t)2 * INTER * INTER * es;   // rows [2E, 3E) of the packed [q;k;v] matrix
      p.bias = X.V(P_AIN_B) + 2 * INTER;
      p.N = INTER;
      p.drop_shift = 5;  // 32 columns = one head
      TRY(X.run1(p));
    }
    // F3: out_proj, batched over the two calls; batch z writes columns [256 z, 256 z + 256) of cat (fusion.py:262)
    {
      GemmProblem p = X.fwd(L.avv, f32, INTER, P_AOUT_W, P_AOUT_B, L.cat, 2 * INTER, B, 0, -1);
      p.batch = 2; p.sA = (long long)B * INTER; p.sC = INTER;
      TRY(X.run1(p));
    }
    // F4-F5: fusion_layers = Linear -> ReLU -> Dropout -> LayerNorm (fusion.py:263)
    TRY(X.run1(X.fwd(L.cat, f32, 2 * INTER, P_AVF_W, P_AVF_B, L.y_a2, INTER, B, 1, SITE_AV_FUSE)));
    // F5-F6: LayerNorm + audiovisual_projection -> token 0 (fusion.py:263, 321, 325)
    if (lnf) {
      TRY(ln_gemm(X.fwd(L.av, f32, INTER, P_AVP_W, P_AVP_B, L.xtok, 2 * FUS, B, 0, -1), L.y_a2, P_AVF_G, P_AVF_BT, L.av, a->audiovisual_features,
                  L.mean_a2, L.rstd_a2));
    } else {
      TRY(launch_ln_fwd(L.y_a2, L.av, a->audiovisual_features, L.mean_a2, L.rstd_a2, X.V(P_AVF_G), X.V(P_AVF_BT), B, INTER, f32, s));
      TRY(X.run1(X.fwd(L.av, f32, INTER, P_AVP_W, P_AVP_B, L.xtok, 2 * FUS, B, 0, -1)));
    }
  }
  if (!chains) MARK("F2-F6 separate launches");
  // F7: packed q|k|v in_proj of the 2-token self-attention (fusion.py:328)
  //     + F8: 2x2 softmax attention, token-pooled context.  bf16: ONE kernel, q|k|v stay in its accumulators
  if (a->prof_events[0]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->prof_events[0], s));
  if (!f32 && opt(OPT_FUSED_ATTN)) {
    void* qkv_out = (a->training && !opt(OPT_QKV_RECOMPUTE)) ? L.qkv : nullptr;
    TRY(launch_tri_fused_fwd(L.xtok, L.wqkv_hm, X.V(P_TIN_B), L.obar, L.probs, qkv_out, B, X.drop_on ? 1 : 0, X.dc, s));
    if (a->prof_events[1]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->prof_events[1], s));
    MARK("tri_fused_kernel<0> (in_proj + attention)");
    TRY(launch_tri_attn_weights(L.probs, a->trimodal_attention, a->av_attention, B, X.drop_on ? 1 : 0, X.dc, s));
    if (a->trimodal_attention || a->av_attention) MARK("attention weights");
  } else {
    TRY(X.run1(X.fwd(L.xtok, f32, FUS, P_TIN_W, P_TIN_B, L.qkv, 3 * FUS, 2 * B, 0, -1)));
    if (a->prof_events[1]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->prof_events[1], s));
    TRY(launch_tri_attn_fwd(L.qkv, L.obar, L.probs, a->trimodal_attention, a->av_attention, B, f32, X.drop_on ? 1 : 0, X.dc, s));
    MARK("in_proj GEMM + attention (unfused)");
  }
  // F9-F17 are local to a sample (Linear / ReLU / Dropout / LayerNorm): in bf16 mode ONE launch walks the chain with the rows
  // resident in LDS (chain.hip) and writes the same workspace buffers; option "chain" = 0 restores the separate launches
  if (chains) {
    ChainArgs c{};
    c.X = reinterpret_cast<const bf16_t*>(L.obar); c.ldx = FUS; c.K0 = FUS; c.B = B; c.groups = 1; c.group_stride = 0;
    c.drop = X.dc;
    auto lin = [&](int pidW, int pidB, int N, int K, int relu, int site, void* stash) {
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WF(pidW); q.bias = X.V(pidB); q.N = N; q.K = K; q.ldw = K;
      q.relu = relu; q.drop_site = X.drop_on ? site : -1;
      q.end_layer = 1; q.nout = N; q.stash = reinterpret_cast<bf16_t*>(stash); q.ld_stash = N;
      return q;
    };
    auto with_ln = [&](ChainSeg q, int pidG, int pidBt, void* xln, float* out32, float* mean, float* rstd) {
      q.gamma = X.V(pidG); q.beta = X.V(pidBt); q.xln = reinterpret_cast<bf16_t*>(xln); q.out32 = out32; q.mean = mean; q.rstd = rstd;
      return q;
    };
    int k = 0;
    c.seg[k++] = lin(P_TOUT_W, P_TOUT_B, FUS, FUS, 0, -1, L.pool);                                                    // F9
    c.seg[k++] = with_ln(lin(P_TFF_W, P_TFF_B, FUS, FUS, 1, SITE_TRI_FUSE, L.y_t3), P_TFF_G, P_TFF_BT, L.tri,        // F10-F11
                         a->trimodal_features, L.mean_t3, L.rstd_t3);
    c.seg[k++] = with_ln(lin(P_OP_W, P_OP_B, FUS, FUS, 1, SITE_OUT_PROJ, L.y_o1), P_OP_G, P_OP_BT, L.fused,           // F12-F13
                         a->fused_features, L.mean_o1, L.rstd_o1);
    c.seg[k++] = lin(P_FP0_W, P_FP0_B, HID, FUS, 1, SITE_FP0, L.h1);                                                   // F14
    c.seg[k++] = lin(P_FP1_W, P_FP1_B, HID, HID, 1, SITE_FP1, L.h2);                                                   // F15
    c.seg[k++] = lin(P_EV0_W, P_EV0_B, 3 * EV1, HID, 1, SITE_EV0, L.e1);                                               // F16
    for (int z = 0; z < 3; ++z) {                                                                                      // F17
      ChainSeg q = lin(P_EV1_W, P_EV1_B, EV2, EV1, 1, SITE_EV1, nullptr);
      q.W += (size_t)z * EV2 * EV1; q.bias += z * EV2;
      q.kin_off = z * EV1; q.nout_off = z * EV2; q.dcol_off = z * EV2;
      q.end_layer = z == 2; q.nout = 3 * EV2;
      if (z == 2) { q.stash = reinterpret_cast<bf16_t*>(L.e2); q.ld_stash = 3 * EV2; }
      c.seg[k++] = q;
    }
    c.nseg = k;
    if (nig_tail) {     // F18 as the chain's tail: last head layer, NIG activations, uncertainties, loss statistics (wave partials)
      ChainNigF& g = c.nigf;
      g.enabled = 1;
      g.w3 = reinterpret_cast<const bf16_t*>(X.W(P_EV2_W)); g.b3 = X.V(P_EV2_B); g.b3_stride = 64;
      g.evid = L.evid; g.nig_out = a->nig_out; g.targets = a->targets; g.wstats = L.stats;
    }
#ifdef MMDEER_STAMPS
    c.stamps = reinterpret_cast<unsigned long long*>(L.slab);   // diagnostic library: cycle samples of workgroup 0 (tools/chain_stamps.py)
#endif
    TRY(launch_chain(c, s));
    MARK(nig_tail ? "chain F9-F18 (trimodal fusion tail + head + NIG)" : "chain F9-F17 (trimodal fusion tail + head)");
  } else {
    // F9: out_proj on the pooled context (mean over tokens commutes with the linear map; fusion.py:335)
    TRY(X.run1(X.fwd(L.obar, f32, FUS, P_TOUT_W, P_TOUT_B, L.pool, FUS, B, 0, -1)));
    // F10-F11: final_fusion (fusion.py:338)
    TRY(X.run1(X.fwd(L.pool, f32, FUS, P_TFF_W, P_TFF_B, L.y_t3, FUS, B, 1, SITE_TRI_FUSE)));
    // F11-F12: LayerNorm of final_fusion + output_projection (fusion.py:338, 162); F13-F14: its LayerNorm + feature_processor.0
    if (lnf) {
      TRY(ln_gemm(X.fwd(L.tri, f32, FUS, P_OP_W, P_OP_B, L.y_o1, FUS, B, 1, SITE_OUT_PROJ), L.y_t3, P_TFF_G, P_TFF_BT, L.tri, a->trimodal_features,
                  L.mean_t3, L.rstd_t3));
      TRY(ln_gemm(X.fwd(L.fused, f32, FUS, P_FP0_W, P_FP0_B, L.h1, HID, B, 1, SITE_FP0), L.y_o1, P_OP_G, P_OP_BT, L.fused, a->fused_features,
                  L.mean_o1, L.rstd_o1));
    } else {
      TRY(launch_ln_fwd(L.y_t3, L.tri, a->trimodal_features, L.mean_t3, L.rstd_t3, X.V(P_TFF_G), X.V(P_TFF_BT), B, FUS, f32, s));
      TRY(X.run1(X.fwd(L.tri, f32, FUS, P_OP_W, P_OP_B, L.y_o1, FUS, B, 1, SITE_OUT_PROJ)));
      TRY(launch_ln_fwd(L.y_o1, L.fused, a->fused_features, L.mean_o1, L.rstd_o1, X.V(P_OP_G), X.V(P_OP_BT), B, FUS, f32, s));
    }
    {
      // F14-F15: feature_processor (deer.py:246)
      if (!lnf) TRY(X.run1(X.fwd(L.fused, f32, FUS, P_FP0_W, P_FP0_B, L.h1, HID, B, 1, SITE_FP0)));
      TRY(X.run1(X.fwd(L.h1, f32, HID, P_FP1_W, P_FP1_B, L.h2, HID, B, 1, SITE_FP1)));
      // F16: the three DEERLayer first layers stacked into one N = 384 GEMM (deer.py:49)
      {
        GemmProblem p = X.fwd(L.h2, f32, HID, P_EV0_W, P_EV0_B, L.e1, 3 * EV1, B, 1, SITE_EV0);
        p.N = 3 * EV1;
        TRY(X.run1(p));
      }
      // F17: second layers, strided-batched over the heads (deer.py:52)
      {
        GemmProblem p = X.fwd(L.e1, f32, 3 * EV1, P_EV1_W, P_EV1_B, L.e2, 3 * EV2, B, 1, SITE_EV1);
        p.batch = 3; p.sA = EV1; p.sB = (long long)EV2 * EV1; p.sC = EV2; p.sBias = EV2;
        TRY(X.run1(p));
      }
    }
  }
  if (!chains) MARK("F9-F17 separate launches");
  // F18: last layer (64 -> 4), NIG activations, uncertainties and -- with targets -- the loss statistics
  if (!nig_tail) {
    TRY(launch_nig_fwd(L.e2, X.W(P_EV2_W), X.V(P_EV2_B), 64, L.evid, a->nig_out, a->targets, L.stats, B, f32, s));
    MARK("nig_fwd (head's last layer + loss statistics)");
  }
  return 0;
}

int mmdeer_backward(const mmdeer_backward_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  const int B = a->batch, f32 = a->compute_f32 ? 1 : 0;
  TRY(check_common(B, a->workspace, a->workspace_bytes, a->weights, a->weights_bytes, f32));
  MMDEER_CHECK(B > 0, "backward needs a non-empty batch");
  MMDEER_CHECK(a->grads != nullptr, "grads is NULL");
  MMDEER_CHECK(a->audio && a->video && a->text, "audio / video / text must be non-NULL");
  hipStream_t s = (hipStream_t)a->stream;
  const Layout L = make_layout(a->workspace, a->weights, B, f32);
  Exec X;
  X.B = B; X.f32 = f32; X.es = f32 ? 4 : 2; X.L = &L; X.s = s;
  X.drop_on = a->training && a->dropout_p > 0.f;
  // bump_offset_dev: the matching forward ran with it -- the pending 1 is added here too, and the last launch of the pass (of phase
  // 2 in the two-call mode) advances the counter
  const bool bump = a->bump_offset_dev && a->offset_dev;
  X.dc = make_drop(a->dropout_p, a->seed, a->offset + (bump ? 1 : 0), a->offset_dev);
  X.mask_scale = X.drop_on ? X.dc.scale : 1.f;
  const int in_f32 = a->inputs_bf16 ? 0 : 1;
  const size_t es = X.es;
  float* G = a->grads;
  const int nwp = nig_tail_plan(B, f32) ? (B + 15) / 16 : 0;      // the forward left wave partials of the loss statistics
  const LossCfg cfg = loss_cfg(a->loss);
  const int nblk = nig_nblocks(B), npl = ln_bwd_nparts(B);

  // The q/k thirds of the AV in_proj never receive a gradient (L = S = 1): exact zeros in the reference.  They are
  // not touched here -- like the alignment gaps they keep the zeros of the caller's one-time initialisation of the
  // gradient buffer (two memset launches per step were ~9 us of GPU time for bytes that never change).

  // Backward = a chain of dX GEMMs (each M = batch rows, plenty of tiles) and ONE grouped launch of all
  // weight-gradient problems (few output tiles each, reduction over the batch, split over K into slabs) followed by
  // one deterministic slab reduction.
  auto reduce_head = [&](ReduceTable& t, int nparts) {
    int k = t.nseg;
    t.src[k] = L.part_w3; t.dst[k] = G + kParams[P_EV2_W].off; t.nparts[k] = nparts; t.n[k] = 768; t.stride[k] = 768; ++k;
    for (int d = 0; d < 3; ++d) {
      t.src[k] = L.part_b3 + d * 4; t.dst[k] = G + kParams[P_EV2_B + d].off; t.nparts[k] = nparts; t.n[k] = 4; t.stride[k] = 12; ++k;
    }
    t.nseg = k;
  };
  // `chained`: the partial slabs were written by a layer chain, one per workgroup of ITS grid (32-sample workgroups above B = 4096)
  auto reduce_ln = [&](ReduceTable& t, const float* part, int pidG, int N, bool chained) {
    int k = t.nseg;   // gamma and beta slices are adjacent in the flat buffer (N is a multiple of 64)
    t.src[k] = part; t.dst[k] = G + kParams[pidG].off; t.nparts[k] = chained ? chain_workgroups(B) : npl; t.n[k] = 2 * N; t.stride[k] = 2 * N; ++k;
    t.nseg = k;
  };
  // All weight-gradient problems are collected and run as ONE launch after the chain: a bucket on its own has
  // only 30-180 workgroups of 16-32 sequential K-steps, i.e. each of three launches took one workgroup's latency
  // (~35-40 us) on a mostly idle chip; together they fill it once.
  GemmGroup dwg{};
  ReduceTable rt{};
  auto add_dw = [&](const GemmProblem& q) { dwg.p[dwg.nprob++] = q; };
  const int phase = a->phase;
  MMDEER_CHECK(phase >= 0 && phase <= 2, "backward: phase must be 0, 1 or 2 (got %d)", phase);
  // backward chains (chain.hip): the head / trimodal run always when enabled; the audio-visual run only in the single-call mode
  // (in the two-call mode its first product, the token-0 dX, belongs to the first call)
  const int bmin = opt(OPT_CHAIN_MIN);
  const bool dchain = !f32 && opt(OPT_CHAIN) && opt(OPT_CHAIN_BWD) && B >= bmin && B <= opt(OPT_CHAIN_MAX) && phase == 0;
  // The end of the pass (or of phase 1): one launch of every weight-gradient problem collected + the fold of all partial slabs, then
  // the events of buckets [first_bucket, last_bucket], which are final now.  Per-bucket launches, also on a side stream beside the dX
  // chain, were measured slower: a bucket alone is 30-180 workgroups of 16-32 sequential K-steps on a mostly idle chip.
  auto finish = [&](int first_bucket, int last_bucket) -> int {
    if (dwg.nprob > 0) {
      TRY(X.run(dwg));
      MARK("weight gradients (all problems, one launch)");
      for (int i = 0; i < dwg.nprob; ++i) Exec::add_slab_segments(rt, dwg.p[i]);
    }
    if (bump && (phase == 0 || phase == 2)) rt.bump = reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(a->offset_dev));
    TRY(launch_reduce_partials(rt, s));
    MARK("reduce_partials (fold)");
    for (int b = first_bucket; b <= last_bucket; ++b)
      if (a->bucket_events[b]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->bucket_events[b], s));
    return 0;
  };

  if (phase != 2) {
  // ================= bucket 0: DEER head =================
  // B1: last head layer + NIG activations (+ loss gradient): a launch of its own, or (bf16 chain plan, loss mode, option chain_nig)
  // the prologue of the backward chain below -- the head kernel is 8 us of mostly fixed launch cost at B = 4096
  const bool bchain = !f32 && opt(OPT_CHAIN) && opt(OPT_CHAIN_BWD) && B >= bmin && B <= opt(OPT_CHAIN_MAX) && !a->g_fused;
  const bool nigfold = bchain && opt(OPT_CHAIN_NIG) && a->targets;
  if (!nigfold)
    TRY(launch_nig_bwd(L.e2, X.W(P_EV2_W), L.evid, a->targets, L.stats, a->targets ? a->global_stats : nullptr, a->g_mu, a->g_nu, a->g_alpha, a->g_beta, nullptr,
                       L.dz2, L.part_w3, L.part_b3, a->loss_out, a->bin_counts, B, f32, X.mask_scale, cfg, nwp, s));
  if (!nigfold) MARK("nig_bwd (head's last layer backward + loss gradient)");
  // B2-B10 are local to a sample like the forward's layers: in bf16 mode (chain_min <= B <= chain_max, no outside gradient on fused_features)
  // ONE launch of the layer-chain kernel walks the head's four dX products, both LayerNorm backwards and the three trimodal dX
  // products with the rows resident in LDS, and writes the same workspace buffers (the weight-gradient launch reads them)
  if (bchain) {
    ChainArgs c{};
    c.X = reinterpret_cast<const bf16_t*>(L.dz2); c.ldx = 3 * EV2; c.K0 = 3 * EV2; c.B = B; c.groups = 1; c.group_stride = 0;
    c.drop = X.dc;
    auto dxseg = [&](int pidW, int N, int K, void* stash, const void* ymask, int ldmask) {
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = X.WTF(pidW); q.N = N; q.K = K; q.ldw = K;
      q.end_layer = 1; q.nout = N; q.stash = reinterpret_cast<bf16_t*>(stash); q.ld_stash = N;
      q.mask_y = reinterpret_cast<const bf16_t*>(ymask); q.ld_mask = ldmask; q.mask_scale = X.mask_scale;
      return q;
    };
    auto with_lnb = [&](ChainSeg q, int pidG, const void* y, const float* mean, const float* rstd, void* dz, float* part) {
      q.lnb_gamma = X.V(pidG); q.lnb_y = reinterpret_cast<const bf16_t*>(y); q.lnb_mean = mean; q.lnb_rstd = rstd;
      q.lnb_dz = reinterpret_cast<bf16_t*>(dz); q.lnb_partial = part; q.lnb_mask_scale = X.mask_scale;
      return q;
    };
    int k = 0;
    for (int z = 0; z < 3; ++z) {     // evidence_net layer 3 (128 -> 64) per head: W^T [128][64], dX masked by e1
      ChainSeg q = dxseg(P_EV1_W, EV1, EV2, nullptr, L.e1, 3 * EV1);
      q.W += (size_t)z * EV2 * EV1;
      q.kin_off = z * EV2; q.nout_off = z * EV1; q.mask_col0 = z * EV1;
      q.end_layer = z == 2; q.nout = 3 * EV1;
      if (z == 2) { q.stash = reinterpret_cast<bf16_t*>(L.de1); q.ld_stash = 3 * EV1; }
      c.seg[k++] = q;
    }
    c.seg[k++] = dxseg(P_EV0_W, HID, 3 * EV1, L.dh2, L.h2, HID);          // evidence_net layer 0: W^T of the stacked heads [256][384]
    c.seg[k++] = dxseg(P_FP1_W, HID, HID, L.dh1, L.h1, HID);              // feature_processor
    c.seg[k++] = with_lnb(dxseg(P_FP0_W, FUS, HID, L.dfused, nullptr, 0), P_OP_G, L.y_o1, L.mean_o1, L.rstd_o1, L.dz_o1, L.part_ln_o1);
    c.seg[k++] = with_lnb(dxseg(P_OP_W, FUS, FUS, L.dtri, nullptr, 0), P_TFF_G, L.y_t3, L.mean_t3, L.rstd_t3, L.dz_t3, L.part_ln_t3);
    c.seg[k++] = dxseg(P_TFF_W, FUS, FUS, L.dpool, nullptr, 0);
    c.seg[k++] = dxseg(P_TOUT_W, FUS, FUS, L.dobar, nullptr, 0);         // attention out_proj (pooled context)
    c.nseg = k;
    if (nigfold) {
      ChainNig& g = c.nig;
      g.enabled = 1;
      g.e2 = reinterpret_cast<const bf16_t*>(L.e2); g.w3 = reinterpret_cast<const bf16_t*>(X.W(P_EV2_W)); g.evid = L.evid;
      g.targets = a->targets; g.stats = L.stats; g.gstats = a->global_stats; g.nblk = nblk; g.nwp = nwp;
      g.dz2 = reinterpret_cast<bf16_t*>(L.dz2); g.partial_w = L.part_w3; g.partial_b = L.part_b3;
      g.loss_out = a->loss_out; g.bin_counts = a->bin_counts; g.mask_scale = X.mask_scale; g.cfg = cfg;
    }
#ifdef MMDEER_STAMPS
    c.stamps = reinterpret_cast<unsigned long long*>(L.davin);   // diagnostic library: untouched until phase 2 (tools/chain_stamps.py bwd)
#endif
    TRY(launch_chain(c, s));
    MARK(nigfold ? "chain B1-B10 (head backward + loss gradient + head / trimodal dX)" : "chain B2-B10 (head / trimodal dX)");
  } else
  {
    // evidence_net layer 3 (128 -> 64), batched over heads: dX masked by e1
    {
      GemmProblem p = X.dx(L.dz2, 3 * EV2, P_EV1_W, L.de1, 3 * EV1, B, L.e1, 3 * EV1);
      p.batch = 3; p.sA = EV2; p.sB = (long long)EV2 * EV1; p.sC = EV1; p.sY = EV1;
      TRY(X.run1(p));
    }
    // evidence_net layer 0 (256 -> 3 x 128 stacked)
    {
      GemmProblem p = X.dx(L.de1, 3 * EV1, P_EV0_W, L.dh2, HID, B, L.h2, HID);
      p.K = 3 * EV1; p.ldb = 3 * EV1;   // W^T of the stacked heads: [256][384]
      TRY(X.run1(p));
    }
    // feature_processor
    TRY(X.run1(X.dx(L.dh2, HID, P_FP1_W, L.dh1, HID, B, L.h1, HID)));
    TRY(X.run1(X.dx(L.dh1, HID, P_FP0_W, L.dfused, FUS, B, nullptr, 0)));
  }
  // a gradient that reaches fused_features from outside the head (a caller's own consumer of that output)
  if (a->g_fused) TRY(launch_add_f32(L.dfused, f32, a->g_fused, (long long)B * FUS, s));
  {
    GemmProblem q = X.dw(L.dz2, 3 * EV2, L.e1, f32, 3 * EV1, P_EV1_W, P_EV1_B, G, B);
    q.batch = 3; q.sA = EV2; q.sB = EV1; q.sC = (long long)EV2 * EV1; q.sBiasGrad = EV2;
    add_dw(q);
    GemmProblem r = X.dw(L.de1, 3 * EV1, L.h2, f32, HID, P_EV0_W, P_EV0_B, G, B);
    r.M = 3 * EV1;
    add_dw(r);
    add_dw(X.dw(L.dh2, HID, L.h1, f32, HID, P_FP1_W, P_FP1_B, G, B));
    add_dw(X.dw(L.dh1, HID, L.fused, f32, FUS, P_FP0_W, P_FP0_B, G, B));
    reduce_head(rt, nigfold ? chain_workgroups(B) : nblk);
  }

  // ================= bucket 1: output_projection + trimodal fusion =================
  if (!bchain) {
    TRY(launch_ln_bwd(L.dfused, L.y_o1, L.mean_o1, L.rstd_o1, X.V(P_OP_G), L.dz_o1, L.part_ln_o1, B, FUS, f32, X.mask_scale, s));
    TRY(X.run1(X.dx(L.dz_o1, FUS, P_OP_W, L.dtri, FUS, B, nullptr, 0)));
    TRY(launch_ln_bwd(L.dtri, L.y_t3, L.mean_t3, L.rstd_t3, X.V(P_TFF_G), L.dz_t3, L.part_ln_t3, B, FUS, f32, X.mask_scale, s));
    TRY(X.run1(X.dx(L.dz_t3, FUS, P_TFF_W, L.dpool, FUS, B, nullptr, 0)));
    TRY(X.run1(X.dx(L.dpool, FUS, P_TOUT_W, L.dobar, FUS, B, nullptr, 0)));      // attention out_proj (pooled context)
  }
  if (!bchain) MARK("B2-B10 separate launches");
  if (!f32 && opt(OPT_FUSED_ATTN) && opt(OPT_QKV_RECOMPUTE)) {   // the forward kept q|k|v on chip: recompute the head tiles
    TRY(launch_tri_fused_bwd(L.xtok, L.wqkv_hm, X.V(P_TIN_B), L.dobar, L.probs, L.dqkv, B, X.drop_on ? 1 : 0, X.dc, s));
    MARK("tri_fused_kernel<1> (attention backward, recompute)");
  } else {
    TRY(launch_tri_attn_bwd(L.qkv, L.dobar, L.probs, L.dqkv, B, f32, X.drop_on ? 1 : 0, X.dc, s));
    MARK("attention backward (unfused)");
  }
  TRY(X.run1(X.dx(L.dqkv, 3 * FUS, P_TIN_W, L.dxtok, FUS, 2 * B, nullptr, 0)));  // in_proj
  MARK("in_proj dX GEMM");
  // (with the AV chain below, this product is its first segment)
  if (!dchain) TRY(X.run1(X.dx(L.dxtok, 2 * FUS, P_AVP_W, L.dav, INTER, B, nullptr, 0)));     // token 0 -> audiovisual features
  {
    add_dw(X.dw(L.dz_o1, FUS, L.tri, f32, FUS, P_OP_W, P_OP_B, G, B));
    add_dw(X.dw(L.dz_t3, FUS, L.pool, f32, FUS, P_TFF_W, P_TFF_B, G, B));
    add_dw(X.dw(L.dpool, FUS, L.obar, f32, FUS, P_TOUT_W, P_TOUT_B, G, B));
    add_dw(X.dw(L.dqkv, 3 * FUS, L.xtok, f32, FUS, P_TIN_W, P_TIN_B, G, 2 * B));
    add_dw(X.dw(L.dxtok, 2 * FUS, L.av, f32, INTER, P_AVP_W, P_AVP_B, G, B));                          // token 0
    add_dw(X.dw(L.dxtok + (size_t)FUS * es, 2 * FUS, a->text, in_f32, TXT, P_TXT_W, P_TXT_B, G, B));   // token 1
    reduce_ln(rt, L.part_ln_o1, P_OP_G, FUS, bchain);
    reduce_ln(rt, L.part_ln_t3, P_TFF_G, FUS, bchain);
  }
  if (phase == 1) return finish(0, 1);
  }   // phase != 2

  // Two-call mode, second call: only the five audio-visual weight gradients are left (~30 tiles of 128x128): whole-reduction
  // tiles would leave 7/8 of the chip idle for a full tile's latency, so their K is cut into eight slices (slabs + fold, as the
  // 256x256 plan did for everything).  Costs nothing in the single-call mode, where they ride along with the other ~200 tiles.
  if (phase == 2) X.slice_div = 8;
  // ================= bucket 2: audio-visual fusion =================
  // B13-B17 (token-0 dX, LayerNorm backward, the three AV dX products) are sample-local as well: one more launch of the chain
  // kernel.  The concatenation's backward is a re-view of the panel: columns [0,256) / [256,512) of d cat become the rows of the
  // audio->video / video->audio call.
  if (dchain) {
    ChainArgs c{};
    c.X = reinterpret_cast<const bf16_t*>(L.dxtok); c.ldx = 2 * FUS; c.K0 = FUS; c.B = B; c.groups = 1; c.group_stride = B;
    c.drop = X.dc;
    auto dxs = [&](const bf16_t* wt, int N, int K, int ldw, void* stash, int ld_stash, int nout) {
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = wt; q.N = N; q.K = K; q.ldw = ldw;
      q.end_layer = 1; q.nout = nout; q.stash = reinterpret_cast<bf16_t*>(stash); q.ld_stash = ld_stash;
      return q;
    };
    int k = 0;
    {   // token 0 -> audiovisual features, then the LayerNorm of fusion_layers backwards (mask of its Linear-ReLU-Dropout)
      ChainSeg q = dxs(X.WTF(P_AVP_W), INTER, FUS, FUS, L.dav, INTER, INTER);
      q.lnb_gamma = X.V(P_AVF_G); q.lnb_y = reinterpret_cast<const bf16_t*>(L.y_a2); q.lnb_mean = L.mean_a2; q.lnb_rstd = L.rstd_a2;
      q.lnb_dz = reinterpret_cast<bf16_t*>(L.dz_a2); q.lnb_partial = L.part_ln_a2; q.lnb_mask_scale = X.mask_scale;
      c.seg[k++] = q;
    }
    {   // fusion_layers dX: W^T [512][256]; the 512 columns = d cat, unfolded into the two calls' rows ([2B,256] stacked)
      ChainSeg q = dxs(X.WTF(P_AVF_W), 2 * INTER, INTER, INTER, L.dcats, INTER, INTER);
      q.fold_groups = 2;
      c.seg[k++] = q;
    }
    {   // AV out_proj; dX gets the regenerated attention-dropout factor of the forward value projection
      ChainSeg q = dxs(X.WTF(P_AOUT_W), INTER, INTER, INTER, L.davv, INTER, INTER);
      if (X.drop_on) { q.drop_site = SITE_AV_ATTN; q.drop_shift = 5; }
      c.seg[k++] = q;
    }
    // AV value projection (columns [2E, 3E) of W^T [256][768])
    c.seg[k++] = dxs(X.WTF(P_AIN_W, (size_t)2 * INTER * INTER), INTER, INTER, INTER, L.davin, INTER, INTER);
    c.nseg = k;
    TRY(launch_chain(c, s));
    MARK("chain B13-B17 (audio-visual dX)");
  } else {
    TRY(launch_ln_bwd(L.dav, L.y_a2, L.mean_a2, L.rstd_a2, X.V(P_AVF_G), L.dz_a2, L.part_ln_a2, B, INTER, f32, X.mask_scale, s));
    // fusion_layers dX, written "stacked" ([2B,256]: rows [0,B) = d audio_attended, rows [B,2B) = d video_attended)
    // by batching over the two column halves of the weight
    {
      GemmProblem p = X.dx(L.dz_a2, INTER, P_AVF_W, L.dcats, INTER, B, nullptr, 0);
      p.N = INTER; p.batch = 2; p.sB = (long long)INTER * INTER; p.sC = (long long)B * INTER;   // rows [256 z, 256 z + 256) of W^T [512][256]
      TRY(X.run1(p));
    }
    // AV out_proj; dX gets the regenerated attention-dropout factor of the forward value projection
    {
      GemmProblem p = X.dx(L.dcats, INTER, P_AOUT_W, L.davv, INTER, 2 * B, nullptr, 0);
      if (X.drop_on) { p.regen_site = SITE_AV_ATTN; p.drop_shift = 5; }
      TRY(X.run1(p));
    }
    // AV value projection (rows [2E,3E) of in_proj)
    {
      GemmProblem p = X.dx(L.davv, INTER, P_AIN_W, L.davin, INTER, 2 * B, nullptr, 0);
      p.B = X.WT(P_AIN_W) + (size_t)2 * INTER * es;   // columns [2E, 3E) of W^T [256][768]
      p.K = INTER;
      TRY(X.run1(p));
    }
  }
  {
    add_dw(X.dw(L.dz_a2, INTER, L.cat, f32, 2 * INTER, P_AVF_W, P_AVF_B, G, B));
    add_dw(X.dw(L.dcats, INTER, L.avv, f32, INTER, P_AOUT_W, P_AOUT_B, G, 2 * B));
    GemmProblem q = X.dw(L.davv, INTER, L.avin, f32, INTER, P_AIN_W, P_AIN_B, G, 2 * B);
    q.C = G + kParams[P_AIN_W].off + 2 * INTER * INTER;
    q.bias_grad = G + kParams[P_AIN_B].off + 2 * INTER;
    q.M = INTER;
    X.set_split(q, G);
    add_dw(q);
    add_dw(X.dw(L.davin, INTER, a->video, in_f32, VID, P_VID_W, P_VID_B, G, B));                                  // rows [0,B)
    if (f32) add_dw(X.dw(L.davin + (size_t)B * INTER * es, INTER, a->audio, in_f32, AUD, P_AUD_W, P_AUD_B, G, B));   // rows [B,2B)
    else add_dw(X.dw(L.davin + (size_t)B * INTER * es, INTER, L.audio_pad, 0, AUD_PAD, P_AUD_W, P_AUD_B, G, B));    // padded copy of F0
    reduce_ln(rt, L.part_ln_a2, P_AVF_G, INTER, dchain);
  }
  if (!dchain) MARK("B13-B17 separate launches");
  // ---- default: all weight gradients in one grouped split-K launch + one deterministic fold of every partial slab
  return finish(phase == 2 ? 2 : 0, 2);
}

// ------------------------------------------------------------------ optimiser step
int mmdeer_adamw_step(const mmdeer_adamw_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  const int f32 = a->compute_f32 ? 1 : 0;
  TRY(check_weights(a->weights, a->weights_bytes, f32));
  MMDEER_CHECK(a->params && a->grads && a->exp_avg && a->exp_avg_sq && a->lr, "adamw: params / grads / exp_avg / exp_avg_sq / lr must be non-NULL");
  MMDEER_CHECK(a->step >= 1, "adamw: step must be >= 1 (got %d)", a->step);
  MMDEER_CHECK(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps > 0.f, "adamw: bad betas / eps");
  const void* const* cparams = const_cast<const void* const*>(a->params);
  TRY(check_params(cparams, "adamw"));
  hipStream_t s = (hipStream_t)a->stream;
  const Layout L = make_layout(nullptr, a->weights, 0, f32);
  const bool images = !f32 && opt(OPT_ADAM_FUSED);   // bf16 mode: the update writes every derived weight image itself (optim.h: AdamImaged)
  AdamTable t{};    // the tensors of the element-wise update: all of them, or (images) those outside kImages -- the vectors, the 4 x 64 last head layers
  AdamImagedTable im{};
  im.base = reinterpret_cast<bf16_t*>(a->weights);
  const bool wt_on = a->pack_transposed != 0;
  auto rel = [&](const char* base, long long elem) { return (int)((reinterpret_cast<const bf16_t*>(base) - im.base) + elem); };
  bool imaged[MMDEER_NUM_PARAMS] = {};
  for (int i = 0; images && i < kNumImages; ++i) {
    const ImageRange& r = kImages[i];
    imaged[r.pid] = true;
    AdamImaged& M = im.m[im.n++];
    M.param = reinterpret_cast<float*>(a->params[r.pid]) + (long long)r.row0 * r.cols(); M.off = r.off();
    M.rows = r.rows; M.cols = r.cols(); M.cols_pad = (r.cols() + 63) / 64 * 64; M.lr = a->lr[r.pid];
    M.frag = M.fragT = M.wt = M.rowpad = M.hm = -1;
    if (r.img & IMG_FRAG) { M.frag = rel(L.wfpack, r.s_off()); M.frag_nkt = r.cols() / 64; M.frag_row0 = r.s_row(); }
    if ((r.img & IMG_FRAGT) && wt_on) { M.fragT = rel(L.wtfpack, r.s_off()); M.fragT_nkt = r.s_rows / 64; M.fragT_col0 = r.s_row(); }
    if ((r.img & IMG_WT) && wt_on) { M.wt = rel(L.wtpack, kParams[r.wt_pid].off); M.wt_ld = r.wt_ld; M.wt_col0 = r.wt_col(); }
    if (r.img & IMG_PAD) { M.rowpad = rel(L.wa_pad, 0); M.rowpad_ld = AUD_PAD; M.frag = rel(L.wa_frag, 0); M.frag_nkt = AUD_PAD / 64; M.frag_row0 = r.row0; }
    if (r.img & IMG_HM) { M.hm = rel(L.wqkv_hm, 0); M.hm_row0 = r.row0; }
  }
  for (int i = 0; i < MMDEER_NUM_PARAMS; ++i) {
    if (imaged[i]) continue;
    const int k = t.nseg++;
    t.param[k] = reinterpret_cast<float*>(a->params[i]);
    t.off[k] = kParams[i].off;
    t.n[k] = kParams[i].rows * kParams[i].cols;
    t.is_vec[k] = kParams[i].is_matrix ? 0 : 1;
    t.lr[k] = a->lr[i];
  }
  t.grads = a->grads; t.exp_avg = a->exp_avg; t.exp_avg_sq = a->exp_avg_sq;
  t.partials = L.wscratch;
  t.norm_out = a->grad_norm;
  t.flat_elems = MMDEER_FLAT_ELEMS;
  t.beta1 = a->beta1; t.beta2 = a->beta2; t.eps = a->eps; t.weight_decay = a->weight_decay;
  t.bias_corr1 = 1.f - powf(a->beta1, (float)a->step);
  t.bias_corr2 = 1.f - powf(a->beta2, (float)a->step);
  t.max_norm = a->max_grad_norm; t.grad_scale = a->grad_scale;
  if (images) return launch_adamw_pack_images(t, im, reinterpret_cast<bf16_t*>(L.wpack), L.vpack, s);
  TRY(launch_adamw_pack(t, L.wpack, f32, L.vpack, s));
  if (f32) { if (a->pack_transposed) TRY(pack_transposed_weights(cparams, L, f32, s)); }
  else TRY(repack_images(L, a->pack_transposed != 0, s));
  return 0;
}

int mmdeer_pack_weights(const void* const* params, void* weights, size_t weights_bytes, int compute_f32, void* stream) {
  const int f32 = compute_f32 ? 1 : 0;
  MMDEER_CHECK(params != nullptr, "pack_weights: params is NULL");
  TRY(check_weights(weights, weights_bytes, f32));
  TRY(check_params(params, "pack_weights"));
  return pack_params(params, make_layout(nullptr, weights, 0, f32), f32, (hipStream_t)stream);
}

int mmdeer_loss_stats(const void* workspace, size_t workspace_bytes, int batch, int compute_f32, float* out, void* stream) {
  static_assert(MMDEER_GLOBAL_STATS == NIG_GLOBAL_STATS, "public header out of sync with nig.h");
  MMDEER_CHECK(workspace && out, "loss_stats: NULL argument");
  MMDEER_CHECK(batch > 0, "loss_stats: batch must be > 0 (got %d)", batch);
  const Layout L = make_layout(const_cast<void*>(workspace), nullptr, batch, compute_f32 ? 1 : 0);
  MMDEER_CHECK(workspace_bytes >= L.bytes, "loss_stats: workspace of %zu bytes is smaller than the %zu of this batch", workspace_bytes, L.bytes);
  return launch_nig_stats_sum(L.stats, batch, out, nig_tail_plan(batch, compute_f32 ? 1 : 0) ? (batch + 15) / 16 : 0, (hipStream_t)stream);
}

}  // extern "C"
