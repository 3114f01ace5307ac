// Stack C: the host-side executor that strings the gfx950 kernels into the forward / backward / optimiser step of the fusion + DEER
// path (include/mmdeer.h: mmdeer_forward, mmdeer_backward, mmdeer_adamw_step, mmdeer_pack_weights, ...), with everything that knows
// its parameters: the parameter table, the workspace / weights layout and the table of derived weight images.  Host code only: every
// function enqueues on the caller's stream and returns; nothing here allocates device memory or synchronises.
#include <cstring>

#include "../../include/mmdeer.h"
#include "../../include/mmdeer_routes.h"
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

// ------------------------------------------------------------------ which chains run
// One answer for mmdeer_forward, mmdeer_backward and mmdeer_loss_stats: the three must agree on nig_tail (the loss statistics in the
// workspace are wave partials then), and it depends on the options and the batch size only.
struct Plan {
  // one workgroup per 16 samples (32 above B = 4096), each streaming all weights of its chain -- a fixed 25-45 us per chain
  // whatever the batch: worth it while the chip holds all workgroups at once and most CUs have one (measured per step: B = 4096
  // -5 to -15 us depending on the box, 3072 -4 us, 2048 0, 1024 +1 us, 64 +12 us; 16-sample workgroups in two rounds at 8192:
  // +9 us, 32-sample workgroups: see DESIGN.md)
  bool chains;     // forward: F2-F6 and F9-F17 as one launch each (chain.hip); option "chain" = 0 restores the separate launches
  // The input chain: with bf16 feature blocks and 16-sample chain workgroups (B <= 4096) the three input projections run as the
  // first two layers of the audio-visual chain -- the workgroup reads its samples' text, video and raw 84-wide audio rows
  // itself (padding the audio rows in LDS and leaving the padded copy for the weight-gradient launch): no pad launch, no F1 launch.
  bool in_chain;
  bool nig_tail;   // the forward head chain ends in the NIG head (option chain_nigf)
  int nwp;         // ... and leaves this many wave partials of the loss statistics, one per 16 samples (else 0)
  // backward chains: the head / trimodal run always when enabled (no outside gradient on fused_features); the audio-visual run only in
  // the single-call mode (in the two-call mode its first product, the token-0 dX, belongs to the first call)
  bool bchain, dchain;
  bool nigfold;    // the head's last layer backward + loss gradient as the prologue of bchain (loss mode, option chain_nig)
};
Plan make_plan(int B, int f32, int phase, bool g_fused, bool inputs_bf16, bool targets) {
  Plan p{};
  p.chains = !f32 && opt(OPT_CHAIN) && B >= opt(OPT_CHAIN_MIN) && B <= opt(OPT_CHAIN_MAX);
  p.in_chain = p.chains && opt(OPT_CHAIN_IN) && inputs_bf16 && chain_samples_per_workgroup(B) == 16;
  p.nig_tail = p.chains && opt(OPT_CHAIN_NIGF);
  p.nwp = p.nig_tail ? (B + 15) / 16 : 0;
  const bool bwd = p.chains && opt(OPT_CHAIN_BWD);
  p.bchain = bwd && !g_fused;
  p.dchain = bwd && phase == 0;
  p.nigfold = p.bchain && opt(OPT_CHAIN_NIG) && targets;
  return p;
}

// ------------------------------------------------------------------ the layers of Stack C
// Every Linear layer, with the LayerNorm behind it where it has one, is described ONCE (make_net); the forward and the backward derive
// each form a plan runs it in from that description (Exec below): forward GEMM problem, forward chain segment, dX GEMM problem, dX
// chain segment, dW GEMM problem.  What is irregular about a layer is a field here, not a patch at a use.
struct Rows { void* p; int ld; };   // rows of a workspace buffer or of a caller's feature block: first element, leading dimension
struct Layer {
  int pidW, pidB;
  int N, K, M;           // Y [M][N] = X [M][K] W^T + b as the kernels run it; M counts the rows of X and dY (B, or 2B: both AV calls / tokens)
  Rows in, out;          // X, Y (pre-LayerNorm)
  int in_f32;            // X's element type: the compute dtype, or that of the caller's feature blocks
  Rows dout, din;        // dY, dX; no din: an input projection
  int relu, site;        // ReLU; dropout site behind it, -1 = none
  Rows mask;             // dX is masked by (mask > 0) * mask_scale: the ReLU + dropout output that X is, where no LayerNorm lies between
  int shift = 0;         // dropout decisions per 2^shift columns (5 = one per head of the AV attention weights)
  int w_row0 = 0;        // the kernels multiply by rows [w_row0, w_row0 + N) of pidW only, columns of its [K][wt_ld] W^T copy ...
  int wt_ld;             // ... (AV value projection: the v third of in_proj [q; k; v] -- one key per query, so q / k are dead)
  int heads = 1;         // > 1: that many equal parameters from pidW / pidB on, on neighbouring N columns of Y / K columns of X: one batched
                         // problem with strides, one chain segment each (the heads' second layers)
  bool padded = false;   // bf16 audio projection: X = L.audio_pad, K = AUD_PAD, W = L.wa_pad / its fragment-major image L.wa_frag
  int row0 = 0;          // Y / dY are rows [row0, row0 + M) of out / dout: row group 1 of the chain's panel (audio under video in L.avin)
  int aux_col = -1;      // >= 0, input chain: X is these columns on of the chain's SECOND input panel [video | padded audio]
  bool open = false;     // the next layer's rows complete this one's output panel in the chain (video, then audio)
  bool cat_out = false;  // Y = torch.cat of the two AV calls: forward rows [z M/2, (z+1) M/2) of X land in columns [z N, (z+1) N) of out --
                         // batch = 2 / fold_groups = 1; the backward sees dout stacked again, M rows
  bool cat_in = false;   // ... and the layer that consumes it: dX is written stacked, the weight halves a batch of 2 / fold_groups = 2
  int regen = -1;        // dX is multiplied by the REGENERATED keep mask of this site (the no-ReLU dropout in front: the AV attention weights)
  int regen_shift = 0;
  // LayerNorm over Y (-1: none): normalised rows, optional fp32 copy for the caller, statistics; backward: dout holds its dz, the
  // gradient of the normalised rows is the consuming layer's din, gamma / beta partial slabs
  int pidG = -1, pidBt = -1;
  void* xln = nullptr; float* out32 = nullptr; float* mean = nullptr; float* rstd = nullptr; float* part = nullptr;
};
Layer linear(int pidW, int pidB, int N, int K, int M, Rows in, int in_f32, Rows out, Rows dout, Rows din, int relu = 0, int site = -1,
             Rows mask = {nullptr, 0}) {
  Layer l{pidW, pidB, N, K, M, in, out, in_f32, dout, din, relu, site, mask};
  l.wt_ld = N;
  return l;
}
void layer_norm(Layer& l, int pidG, int pidBt, void* xln, float* out32, float* mean, float* rstd, float* part) {
  l.pidG = pidG; l.pidBt = pidBt; l.xln = xln; l.out32 = out32; l.mean = mean; l.rstd = rstd; l.part = part;
}

struct Net { Layer vid, aud, txt, avv, aout, avf, avp, tin, tout, tff, op, fp0, fp1, ev0, ev1; };
// av32 / tri32 / fused32: the forward's optional fp32 copies of the three feature outputs
Net make_net(const Layout& L, int B, int f32, const void* audio, const void* video, const void* text, int in_f32, float* av32,
             float* tri32, float* fused32) {
  const size_t es = f32 ? 4 : 2;
  auto in = [](const void* p, int ld) { return Rows{const_cast<void*>(p), ld}; };
  const Rows none{nullptr, 0};
  Net n;
  // the input projections (fusion.py:236-237, 322): video / audio -> rows [0, B) / [B, 2B) of the stacked attention input, text -> token 1
  n.vid = linear(P_VID_W, P_VID_B, INTER, VID, B, in(video, VID), in_f32, {L.avin, INTER}, {L.davin, INTER}, none);
  n.vid.aux_col = 0; n.vid.open = true;
  // bf16 mode: 84-wide rows are not 16-byte aligned -- the audio block zero-padded to 128 columns runs on the LDS-DMA kernels
  n.aud = linear(P_AUD_W, P_AUD_B, INTER, f32 ? AUD : AUD_PAD, B, f32 ? in(audio, AUD) : Rows{L.audio_pad, AUD_PAD}, f32 ? in_f32 : 0,
                 {L.avin, INTER}, {L.davin, INTER}, none);
  n.aud.padded = !f32; n.aud.row0 = B; n.aud.aux_col = VID;
  // the two token slots of xtok / dxtok: token t of a sample at columns [t FUS, (t + 1) FUS) of its 2 FUS-wide row
  const Rows tok0{L.xtok, 2 * FUS}, tok1{L.xtok + (size_t)FUS * es, 2 * FUS}, dtok0{L.dxtok, 2 * FUS}, dtok1{L.dxtok + (size_t)FUS * es, 2 * FUS};
  n.txt = linear(P_TXT_W, P_TXT_B, FUS, TXT, B, in(text, TXT), in_f32, tok1, dtok1, none);
  // the shared AV cross-attention on [video_proj; audio_proj] (fusion.py:244-255; L = S = 1: softmax == 1, only the value and output
  // projections remain), attention-weight dropout = one decision per (row, head)
  n.avv = linear(P_AIN_W, P_AIN_B, INTER, INTER, 2 * B, {L.avin, INTER}, f32, {L.avv, INTER}, {L.davv, INTER}, {L.davin, INTER}, 0, SITE_AV_ATTN);
  n.avv.shift = 5; n.avv.w_row0 = 2 * INTER; n.avv.wt_ld = 3 * INTER;
  // out_proj of both calls; call z lands in columns [256 z, 256 z + 256) of cat (fusion.py:262)
  n.aout = linear(P_AOUT_W, P_AOUT_B, INTER, INTER, 2 * B, {L.avv, INTER}, f32, {L.cat, 2 * INTER}, {L.dcats, INTER}, {L.davv, INTER});
  n.aout.cat_out = true; n.aout.regen = SITE_AV_ATTN; n.aout.regen_shift = 5;
  // fusion_layers = Linear -> ReLU -> Dropout -> LayerNorm (fusion.py:263); its dX = d cat unfolded into the two calls' rows: [2B][256]
  // stacked, rows [0, B) = d audio_attended, rows [B, 2B) = d video_attended
  n.avf = linear(P_AVF_W, P_AVF_B, INTER, 2 * INTER, B, {L.cat, 2 * INTER}, f32, {L.y_a2, INTER}, {L.dz_a2, INTER}, {L.dcats, INTER}, 1, SITE_AV_FUSE);
  n.avf.cat_in = true;
  layer_norm(n.avf, P_AVF_G, P_AVF_BT, L.av, av32, L.mean_a2, L.rstd_a2, L.part_ln_a2);
  // audiovisual_projection -> token 0 (fusion.py:321, 325)
  n.avp = linear(P_AVP_W, P_AVP_B, FUS, INTER, B, {L.av, INTER}, f32, tok0, dtok0, {L.dav, INTER});
  // packed q|k|v in_proj of the 2-token self-attention (fusion.py:328): a GEMM of its own in the backward, and in the unfused forward
  n.tin = linear(P_TIN_W, P_TIN_B, 3 * FUS, FUS, 2 * B, {L.xtok, FUS}, f32, {L.qkv, 3 * FUS}, {L.dqkv, 3 * FUS}, {L.dxtok, FUS});
  // its out_proj on the pooled context (mean over tokens commutes with the linear map; fusion.py:335)
  n.tout = linear(P_TOUT_W, P_TOUT_B, FUS, FUS, B, {L.obar, FUS}, f32, {L.pool, FUS}, {L.dpool, FUS}, {L.dobar, FUS});
  // final_fusion (fusion.py:338) and output_projection (fusion.py:162): Linear -> ReLU -> Dropout -> LayerNorm
  n.tff = linear(P_TFF_W, P_TFF_B, FUS, FUS, B, {L.pool, FUS}, f32, {L.y_t3, FUS}, {L.dz_t3, FUS}, {L.dpool, FUS}, 1, SITE_TRI_FUSE);
  layer_norm(n.tff, P_TFF_G, P_TFF_BT, L.tri, tri32, L.mean_t3, L.rstd_t3, L.part_ln_t3);
  n.op = linear(P_OP_W, P_OP_B, FUS, FUS, B, {L.tri, FUS}, f32, {L.y_o1, FUS}, {L.dz_o1, FUS}, {L.dtri, FUS}, 1, SITE_OUT_PROJ);
  layer_norm(n.op, P_OP_G, P_OP_BT, L.fused, fused32, L.mean_o1, L.rstd_o1, L.part_ln_o1);
  // feature_processor (deer.py:246)
  n.fp0 = linear(P_FP0_W, P_FP0_B, HID, FUS, B, {L.fused, FUS}, f32, {L.h1, HID}, {L.dh1, HID}, {L.dfused, FUS}, 1, SITE_FP0);
  n.fp1 = linear(P_FP1_W, P_FP1_B, HID, HID, B, {L.h1, HID}, f32, {L.h2, HID}, {L.dh2, HID}, {L.dh1, HID}, 1, SITE_FP1, {L.h1, HID});
  // the three DEERLayer first layers (deer.py:49): neighbouring parameters read as ONE stacked [384][256] matrix (kImages)
  n.ev0 = linear(P_EV0_W, P_EV0_B, 3 * EV1, HID, B, {L.h2, HID}, f32, {L.e1, 3 * EV1}, {L.de1, 3 * EV1}, {L.dh2, HID}, 1, SITE_EV0, {L.h2, HID});
  // their second layers (deer.py:52), [64][128] each on its own third of e1
  n.ev1 = linear(P_EV1_W, P_EV1_B, EV2, EV1, B, {L.e1, 3 * EV1}, f32, {L.e2, 3 * EV2}, {L.dz2, 3 * EV2}, {L.de1, 3 * EV1}, 1, SITE_EV1, {L.e1, 3 * EV1});
  n.ev1.heads = 3;
  return n;
}

// Builder for the executor's GEMM problems and chain segments.  `es` = bytes of one activation element.
struct Exec {
  int B, f32;
  int slice_div = 1; // > 1: weight-gradient K-slices this many times shorter (a launch with few problems: see mmdeer_backward phase 2)
  size_t es;
  bool drop_on;      // dropout active
  bool bump;         // the step advances the device-side dropout counter (bump_offset_dev)
  float mask_scale;  // 1/(1-p) when dropout is active, else 1
  DropCtx dc;
  const Layout* L;
  hipStream_t s;

  const char* W(int pid) const { return L->wpack + (size_t)kParams[pid].off * es; }
  const float* V(int pid) const { return L->vpack + kParams[pid].off; }
  // the packed W^T ([K_layer][N_layer], reduction-contiguous) the dX GEMMs multiply by
  const char* WT(int pid) const { return L->wtpack + (size_t)kParams[pid].off * es; }
  // fragment-major images of W / W^T for the layer chains (bf16 mode; kImages above says which exist)
  const bf16_t* WF(int pid, size_t elem_off = 0) const { return reinterpret_cast<const bf16_t*>(L->wfpack) + kParams[pid].off + elem_off; }
  const bf16_t* WTF(int pid, size_t elem_off = 0) const { return reinterpret_cast<const bf16_t*>(L->wtfpack) + kParams[pid].off + elem_off; }
  // rows [row0, ...) of r
  char* at(const Rows& r, int row0) const { return reinterpret_cast<char*>(r.p) + (size_t)row0 * r.ld * es; }
  static bf16_t* bf(const void* p) { return reinterpret_cast<bf16_t*>(const_cast<void*>(p)); }

  // Y = X W^T + b: activations in, activations out
  GemmProblem fwd(const Layer& l) const {
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = l.in.p; p.a_f32 = l.in_f32; p.lda = l.in.ld;
    p.B = l.padded ? L->wa_pad : W(l.pidW) + (size_t)l.w_row0 * l.K * es; p.b_f32 = f32; p.ldb = l.K;
    p.C = at(l.out, l.row0); p.c_f32 = f32; p.ldc = l.out.ld;
    p.bias = V(l.pidB) + l.w_row0;
    p.M = l.M; p.N = l.N; p.K = l.K;
    p.relu = l.relu;
    p.drop_site = drop_on ? l.site : -1; p.drop_shift = l.shift;
    if (l.heads > 1) { p.batch = l.heads; p.sA = l.K; p.sB = (long long)l.N * l.K; p.sC = l.N; p.sBias = l.N; }
    if (l.cat_out) { p.M = l.M / 2; p.batch = 2; p.sA = (long long)p.M * l.in.ld; p.sC = l.N; }
    return p;
  }
  // ... as segment(s) of a forward chain, one per head; the layer's own LayerNorm runs at the layer end
  void fwd_seg(ChainArgs& c, const Layer& l) const {
    for (int z = 0; z < l.heads; ++z) {
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = l.padded ? bf(L->wa_frag) : WF(l.pidW, ((size_t)l.w_row0 + (size_t)z * l.N) * l.K);
      q.bias = V(l.pidB) + l.w_row0 + z * l.N;
      q.N = l.N; q.K = l.K; q.ldw = l.K;
      q.relu = l.relu; q.drop_site = drop_on ? l.site : -1; q.drop_shift = l.shift;
      q.kin_off = z * l.K; q.nout_off = z * l.N; q.dcol_off = z * l.N;
      if (l.aux_col >= 0) { q.in_aux = 1; q.kin_off = l.aux_col; }
      q.row_group = l.row0 ? 1 : 0;
      q.fold_groups = l.cat_out ? 1 : 0;
      if (z == l.heads - 1 && !l.open) {
        q.end_layer = 1; q.nout = (l.cat_out ? 2 : l.heads) * l.N; q.stash = bf(l.out.p); q.ld_stash = l.out.ld;
        if (l.pidG >= 0) { q.gamma = V(l.pidG); q.beta = V(l.pidBt); q.xln = bf(l.xln); q.out32 = l.out32; q.mean = l.mean; q.rstd = l.rstd; }
      }
      c.seg[c.nseg++] = q;
    }
  }
  // bf16 mode: a LayerNorm runs inside the GEMM that consumes it (gemm_ln.hip: the workgroup of a 64-row tile owns whole rows of its A
  // operand, K = the LayerNorm width) -- three launches fewer in the forward; option "ln_fused" = 0 restores the stand-alone kernel
  int fwd_ln(const Layer& l, const Layer& norm) const {
    GemmGroup g{};
    g.nprob = 1;
    g.p[0] = fwd(l);
    g.drop = dc;
    return launch_gemm_ln(g, norm.out.p, V(norm.pidG), V(norm.pidBt), norm.xln, norm.out32, norm.mean, norm.rstd, s);
  }
  int ln_fwd(const Layer& l) const {
    return launch_ln_fwd(l.out.p, l.xln, l.out32, l.mean, l.rstd, V(l.pidG), V(l.pidBt), l.M, l.N, f32, s);
  }
  // the LayerNorm of `l` backwards: the gradient of its normalised rows is the dX of the layer `next` that consumes them
  int ln_bwd(const Layer& l, const Layer& next) const {
    return launch_ln_bwd(next.din.p, l.out.p, l.mean, l.rstd, V(l.pidG), l.dout.p, l.part, l.M, l.N, f32, mask_scale, s);
  }
  // dX = dY W, optionally masked by (Yprev > 0) * mask_scale.  Runs as an NT GEMM against the packed W^T, i.e. on the LDS-DMA
  // kernel in bf16 mode.
  GemmProblem dx(const Layer& l) const {
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = l.dout.p; p.a_f32 = f32; p.lda = l.dout.ld;
    p.B = WT(l.pidW) + (size_t)l.w_row0 * es; p.b_f32 = f32; p.ldb = l.wt_ld;
    p.C = l.din.p; p.c_f32 = f32; p.ldc = l.din.ld;
    p.M = l.M; p.N = l.K; p.K = l.N;
    p.Y = l.mask.p; p.y_f32 = f32; p.ldy = l.mask.ld; p.mask_scale = mask_scale;
    if (drop_on && l.regen >= 0) { p.regen_site = l.regen; p.drop_shift = l.regen_shift; }
    if (l.heads > 1) { p.batch = l.heads; p.sA = l.N; p.sB = (long long)l.N * l.K; p.sC = l.K; p.sY = l.K; }
    if (l.cat_in) { p.N = l.K / 2; p.batch = 2; p.sB = (long long)p.N * l.N; p.sC = (long long)l.M * l.din.ld; }   // rows [z K/2, (z+1) K/2) of W^T
    return p;
  }
  // ... as segment(s) of a backward chain (the fragment-major W^T images).  `norm`: the LayerNorm whose normalised rows are this
  // layer's X runs backwards at the layer end, on the finished dX (mask of its Linear-ReLU-Dropout included)
  void dx_seg(ChainArgs& c, const Layer& l, const Layer* norm = nullptr) const {
    for (int z = 0; z < l.heads; ++z) {
      ChainSeg q;
      chain_seg_defaults(q);
      q.W = WTF(l.pidW, ((size_t)l.w_row0 + (size_t)z * l.N) * l.K);
      q.N = l.K; q.K = l.N; q.ldw = l.N;
      q.kin_off = z * l.N; q.nout_off = z * l.K;
      if (l.mask.p) { q.mask_y = bf(l.mask.p); q.ld_mask = l.mask.ld; q.mask_col0 = z * l.K; q.mask_scale = mask_scale; }
      if (drop_on && l.regen >= 0) { q.drop_site = l.regen; q.drop_shift = l.regen_shift; }
      q.fold_groups = l.cat_in ? 2 : 0;
      if (z == l.heads - 1) {
        q.end_layer = 1; q.nout = l.cat_in ? l.K / 2 : l.heads * l.K; q.stash = bf(l.din.p); q.ld_stash = l.din.ld;
        if (norm) {
          q.lnb_gamma = V(norm->pidG); q.lnb_y = bf(norm->out.p); q.lnb_mean = norm->mean; q.lnb_rstd = norm->rstd;
          q.lnb_dz = bf(norm->dout.p); q.lnb_partial = norm->part; q.lnb_mask_scale = mask_scale;
        }
      }
      c.seg[c.nseg++] = q;
    }
  }
  // dW = dY^T X (+ db = column sums of dY), written into the flat gradient buffer.  The reduction runs over the
  // batch (K = M rows): it is split into K-slices of ~ksteps_target() K-tiles whose partials go to the slab.
  GemmProblem dw(const Layer& l, float* grads) const {
    const int cols = kParams[l.pidW].cols;   // (the padded audio projection: 84 of X's 128 columns)
    GemmProblem p;
    gemm_problem_defaults(p);
    p.A = at(l.dout, l.row0); p.a_f32 = f32; p.lda = l.dout.ld; p.trans_a = 1;
    p.B = l.in.p; p.b_f32 = l.in_f32; p.ldb = l.in.ld; p.trans_b = 1;
    p.C = grads + kParams[l.pidW].off + (long long)l.w_row0 * cols; p.c_f32 = 1; p.ldc = cols;
    p.bias_grad = grads + kParams[l.pidB].off + l.w_row0;
    p.M = l.N; p.N = cols; p.K = l.M;
    if (l.heads > 1) { p.batch = l.heads; p.sA = l.N; p.sB = l.K; p.sC = (long long)l.N * l.K; p.sBiasGrad = l.N; }
    set_split(p, grads);
    return p;
  }
  // derive the split-K fields from p.K and the final destinations p.C / p.bias_grad
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
  // the gamma / beta partial slabs of l's LayerNorm backward -> the flat gradient (the two slices are adjacent there: N is a multiple
  // of 64).  `chained`: written by a layer chain, one per workgroup of ITS grid (32-sample workgroups above B = 4096)
  void add_ln_segment(ReduceTable& t, const Layer& l, float* grads, bool chained) const {
    const int k = t.nseg++;
    t.src[k] = l.part; t.dst[k] = grads + kParams[l.pidG].off; t.nparts[k] = chained ? chain_workgroups(B) : ln_bwd_nparts(B);
    t.n[k] = 2 * l.N; t.stride[k] = 2 * l.N;
  }
  // a chain over this batch whose workgroups read K0-wide input rows (two row groups: rows [0, B) and [group_stride, group_stride + B))
  ChainArgs chain(const Rows& x, int K0, int groups, long long group_stride) const {
    ChainArgs c{};
    c.X = bf(x.p); c.ldx = x.ld; c.K0 = K0; c.B = B; c.groups = groups; c.group_stride = group_stride;
    c.drop = dc;
    return c;
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
// `bump_offset_dev`: the device-side dropout step counter (HIP-graph replays) is advanced by the LAST kernel of the STEP (the fold at
// the end of mmdeer_backward -- of phase 2 in the two-call mode -- which draws no mask): with it every kernel of the forward and of
// the backward adds the pending 1 to the host-side offset -- the same effective offset everywhere, and no kernel has to exist just to
// bump the counter (round 3: the pad launch in front of the first mask; the chains took that launch away).
Exec make_exec(const Layout& L, int B, int f32, hipStream_t s, int training, float dropout_p, uint64_t seed, uint64_t offset,
               const uint64_t* offset_dev, int bump_offset_dev) {
  Exec X;
  X.B = B; X.f32 = f32; X.es = f32 ? 4 : 2; X.L = &L; X.s = s;
  X.drop_on = training && dropout_p > 0.f;
  X.bump = bump_offset_dev && offset_dev;
  X.dc = make_drop(dropout_p, seed, offset + (X.bump ? 1 : 0), offset_dev);
  X.mask_scale = X.drop_on ? X.dc.scale : 1.f;
  return X;
}


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

// The chain launches of one single-call training step (mmdeer_forward + mmdeer_backward(phase = 0), no outside gradient) and the
// kernel each would run: make_plan says which chains run, chain_route (chain.h) the kernel.
int mmdeer_step_chain_routes(int batch, int compute_f32, int inputs_bf16, int targets, char* out, int cap) {
  MMDEER_CHECK(batch >= 0, "step_chain_routes: batch");
  const int c = out && cap > 0 ? cap : 0;
  if (c) out[0] = 0;
  if (batch == 0) return 0;
  const Plan p = make_plan(batch, compute_f32 ? 1 : 0, 0, false, inputs_bf16 != 0, targets != 0);
  const int ms = chain_samples_per_workgroup(batch);
  int n = 0, len = 0;
  auto line = [&](const char* label) {
    ++n;
    if (len >= c) return;
    const int w = snprintf(out + len, c - len, "%s%s %s", len ? "\n" : "", label, chain_kernel_name(chain_route(ms)));
    len = len + w < c ? len + w : c;
  };
  if (p.chains) {
    line(p.in_chain ? "F1-F6" : "F2-F6");
    line(p.nig_tail ? "F9-F18" : "F9-F17");
  }
  if (p.bchain) line(p.nigfold ? "B1-B10" : "B2-B10");
  if (p.dchain) line("B13-B17");
  return n;
}

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

  const Exec X = make_exec(L, B, f32, s, a->training, a->dropout_p, a->seed, a->offset, a->offset_dev, a->bump_offset_dev);
  const int in_f32 = a->inputs_bf16 ? 0 : 1;
  const Plan plan = make_plan(B, f32, 0, false, !in_f32, false);
  const Net n = make_net(L, B, f32, a->audio, a->video, a->text, in_f32, a->audiovisual_features, a->trimodal_features, a->fused_features);

  // F0 (bf16 mode): 84-wide rows are not 16-byte aligned -- zero-pad the audio block to 128 columns so that it runs on the
  //     LDS-DMA kernels
  if (!f32 && !plan.in_chain) {
    PadTable pt{};
    pt.src[0] = a->audio; pt.dst[0] = L.audio_pad; pt.src_f32[0] = in_f32; pt.rows[0] = B; pt.cols[0] = AUD; pt.ld_dst[0] = AUD_PAD;
    pt.nseg = 1;
    TRY(launch_pad_cols(pt, s));
    MARK("pad_cols (audio 84 -> 128)");
  }
  // F1: the three input projections in one launch
  if (!plan.in_chain) {
    GemmGroup g{};
    g.nprob = 3;
    g.p[0] = X.fwd(n.vid);
    g.p[1] = X.fwd(n.aud);
    g.p[2] = X.fwd(n.txt);
    TRY(X.run(g));
    MARK("F1 input projections (3 problems)");
  }
  const bool lnf = !f32 && opt(OPT_LN_FUSED);   // LayerNorm inside the consuming GEMM (Exec::fwd_ln)
  // F2-F6 are local to a sample: in bf16 mode ONE launch walks them with the rows resident in LDS (chain.hip).  A workgroup holds the
  // video and the audio row of its 16 samples as two row groups; torch.cat of the two attention outputs is a re-view of the panel.
  if (plan.chains) {
    ChainArgs c = X.chain(n.avv.in, n.avv.K, 2, B);
    if (plan.in_chain) {    // F1c, F1a, F1b in front: the chain reads the text rows, and video / raw audio as its second input panel
      c = X.chain(n.txt.in, n.txt.K, 1, B);
      c.aux_video = Exec::bf(n.vid.in.p); c.aux_ldv = n.vid.in.ld;
      c.aux_audio = reinterpret_cast<const bf16_t*>(a->audio); c.aux_lda = AUD;
      c.aux_audio_pad = reinterpret_cast<bf16_t*>(L.audio_pad);
      X.fwd_seg(c, n.txt);
      X.fwd_seg(c, n.vid);
      X.fwd_seg(c, n.aud);
    }
    X.fwd_seg(c, n.avv);    // F2
    X.fwd_seg(c, n.aout);   // F3
    X.fwd_seg(c, n.avf);    // F4-F5
    X.fwd_seg(c, n.avp);    // F6
    TRY(launch_chain(c, s));
    MARK(plan.in_chain ? "chain F1-F6 (input projections + audio-visual fusion)" : "chain F2-F6 (audio-visual fusion)");
  } else {
    TRY(X.run1(X.fwd(n.avv)));    // F2
    TRY(X.run1(X.fwd(n.aout)));   // F3
    TRY(X.run1(X.fwd(n.avf)));    // F4
    // F5-F6: LayerNorm + audiovisual_projection
    if (lnf) {
      TRY(X.fwd_ln(n.avp, n.avf));
    } else {
      TRY(X.ln_fwd(n.avf));
      TRY(X.run1(X.fwd(n.avp)));
    }
  }
  if (!plan.chains) MARK("F2-F6 separate launches");
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
    TRY(X.run1(X.fwd(n.tin)));
    if (a->prof_events[1]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->prof_events[1], s));
    TRY(launch_tri_attn_fwd(L.qkv, L.obar, L.probs, a->trimodal_attention, a->av_attention, B, f32, X.drop_on ? 1 : 0, X.dc, s));
    MARK("in_proj GEMM + attention (unfused)");
  }
  // F9-F17 are local to a sample (Linear / ReLU / Dropout / LayerNorm): in bf16 mode ONE launch walks the chain with the rows
  // resident in LDS (chain.hip) and writes the same workspace buffers; option "chain" = 0 restores the separate launches
  if (plan.chains) {
    ChainArgs c = X.chain(n.tout.in, n.tout.K, 1, 0);
    X.fwd_seg(c, n.tout);   // F9
    X.fwd_seg(c, n.tff);    // F10-F11
    X.fwd_seg(c, n.op);     // F12-F13
    X.fwd_seg(c, n.fp0);    // F14
    X.fwd_seg(c, n.fp1);    // F15
    X.fwd_seg(c, n.ev0);    // F16
    X.fwd_seg(c, n.ev1);    // F17
    if (plan.nig_tail) {     // F18 as the chain's tail: last head layer, NIG activations, uncertainties, loss statistics (wave partials)
      ChainNigF& g = c.nigf;
      g.enabled = 1;
      g.w3 = reinterpret_cast<const bf16_t*>(X.W(P_EV2_W)); g.b3 = X.V(P_EV2_B); g.b3_stride = 64;
      g.evid = L.evid; g.nig_out = a->nig_out; g.targets = a->targets; g.wstats = L.stats;
    }
#ifdef MMDEER_STAMPS
    c.stamps = reinterpret_cast<unsigned long long*>(L.slab);   // diagnostic library: cycle samples of workgroup 0 (tools/chain_stamps.py)
#endif
    TRY(launch_chain(c, s));
    MARK(plan.nig_tail ? "chain F9-F18 (trimodal fusion tail + head + NIG)" : "chain F9-F17 (trimodal fusion tail + head)");
  } else {
    TRY(X.run1(X.fwd(n.tout)));   // F9
    TRY(X.run1(X.fwd(n.tff)));    // F10
    // F11-F12: LayerNorm of final_fusion + output_projection; F13-F14: its LayerNorm + feature_processor.0
    if (lnf) {
      TRY(X.fwd_ln(n.op, n.tff));
      TRY(X.fwd_ln(n.fp0, n.op));
    } else {
      TRY(X.ln_fwd(n.tff));
      TRY(X.run1(X.fwd(n.op)));
      TRY(X.ln_fwd(n.op));
      TRY(X.run1(X.fwd(n.fp0)));
    }
    TRY(X.run1(X.fwd(n.fp1)));    // F15
    TRY(X.run1(X.fwd(n.ev0)));    // F16: one N = 384 GEMM
    TRY(X.run1(X.fwd(n.ev1)));    // F17: strided-batched over the heads
  }
  if (!plan.chains) MARK("F9-F17 separate launches");
  // F18: last layer (64 -> 4), NIG activations, uncertainties and -- with targets -- the loss statistics
  if (!plan.nig_tail) {
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
  // (bump_offset_dev: the matching forward ran with it)
  Exec X = make_exec(L, B, f32, s, a->training, a->dropout_p, a->seed, a->offset, a->offset_dev, a->bump_offset_dev);
  const Net n = make_net(L, B, f32, a->audio, a->video, a->text, a->inputs_bf16 ? 0 : 1, nullptr, nullptr, nullptr);
  float* G = a->grads;
  const LossCfg cfg = loss_cfg(a->loss);
  const int nblk = nig_nblocks(B);

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
  // All weight-gradient problems are collected and run as ONE launch after the chain: a bucket on its own has
  // only 30-180 workgroups of 16-32 sequential K-steps, i.e. each of three launches took one workgroup's latency
  // (~35-40 us) on a mostly idle chip; together they fill it once.
  GemmGroup dwg{};
  ReduceTable rt{};
  auto add_dw = [&](const Layer& l) { dwg.p[dwg.nprob++] = X.dw(l, G); };
  const int phase = a->phase;
  MMDEER_CHECK(phase >= 0 && phase <= 2, "backward: phase must be 0, 1 or 2 (got %d)", phase);
  const Plan plan = make_plan(B, f32, phase, a->g_fused != nullptr, a->inputs_bf16 != 0, a->targets != nullptr);
  // The end of the pass (or of phase 1): one launch of every weight-gradient problem collected + the fold of all partial slabs, then
  // the events of buckets [first_bucket, last_bucket], which are final now.  Per-bucket launches, also on a side stream beside the dX
  // chain, were measured slower: a bucket alone is 30-180 workgroups of 16-32 sequential K-steps on a mostly idle chip.
  auto finish = [&](int first_bucket, int last_bucket) -> int {
    // the last launch of the pass (of phase 2 in the two-call mode) advances the dropout step counter
    unsigned long long* const bump = X.bump && (phase == 0 || phase == 2) ? reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(a->offset_dev)) : nullptr;
    // Option dw_fold: the weight-gradient launch folds for itself -- its last-arriving K-slice adds a tile's slices, workgroups behind
    // the tiles fold the row partials collected so far, it bumps the counter -- when the whole group is ONE launch of the DMA kernel
    // (asked on the host, before anything runs: a group that splits by source mode, or takes a register-staged kernel, keeps the fold
    // launch for everything).  The tile counters are words of the q/k thirds of the AV in_proj gradient, which nothing writes: zero by
    // the caller's one-time initialisation of `grads` (include/mmdeer.h), and zero again when the launch ends.
    dwg.drop = X.dc;
    const bool fold_in = opt(OPT_DW_FOLD) && dwg.nprob > 0 && rt.nseg <= GEMM_FOLD_SEGMENTS &&
                         gemm_group_single_launch(dwg, f32, pick_tile(dwg), GEMM_TT_DMA);
    if (fold_in) {
      GemmFold& f = dwg.fold;
      f.cnt = reinterpret_cast<unsigned*>(G + kParams[P_AIN_W].off);
      f.cnt_n = 2 * INTER * INTER;
      f.bump = bump;
      f.nseg = rt.nseg;
      for (int i = 0; i < rt.nseg; ++i) { f.src[i] = rt.src[i]; f.dst[i] = rt.dst[i]; f.stride[i] = rt.stride[i]; f.nparts[i] = rt.nparts[i]; f.n[i] = rt.n[i]; }
    }
    if (dwg.nprob > 0) {
      TRY(X.run(dwg));
      MARK("weight gradients (all problems, one launch)");
      for (int i = 0; i < dwg.nprob; ++i) Exec::add_slab_segments(rt, dwg.p[i]);
    }
    if (!fold_in) {
      rt.bump = bump;
      TRY(launch_reduce_partials(rt, s));
      MARK("reduce_partials (fold)");
    }
    for (int b = first_bucket; b <= last_bucket; ++b)
      if (a->bucket_events[b]) MMDEER_HIP(hipEventRecord((hipEvent_t)a->bucket_events[b], s));
    return 0;
  };

  if (phase != 2) {
  // ================= bucket 0: DEER head =================
  // B1: last head layer + NIG activations (+ loss gradient): a launch of its own, or (bf16 chain plan, loss mode, option chain_nig)
  // the prologue of the backward chain below -- the head kernel is 8 us of mostly fixed launch cost at B = 4096
  if (!plan.nigfold)
    TRY(launch_nig_bwd(L.e2, X.W(P_EV2_W), L.evid, a->targets, L.stats, a->targets ? a->global_stats : nullptr, a->g_mu, a->g_nu, a->g_alpha, a->g_beta, nullptr,
                       L.dz2, L.part_w3, L.part_b3, a->loss_out, a->bin_counts, B, f32, X.mask_scale, cfg, plan.nwp, s));
  if (!plan.nigfold) MARK("nig_bwd (head's last layer backward + loss gradient)");
  // B2-B10 are local to a sample like the forward's layers: in bf16 mode (chain_min <= B <= chain_max, no outside gradient on fused_features)
  // ONE launch of the layer-chain kernel walks the head's four dX products, both LayerNorm backwards and the three trimodal dX
  // products with the rows resident in LDS, and writes the same workspace buffers (the weight-gradient launch reads them)
  if (plan.bchain) {
    ChainArgs c = X.chain(n.ev1.dout, n.ev1.heads * n.ev1.N, 1, 0);
    X.dx_seg(c, n.ev1);
    X.dx_seg(c, n.ev0);
    X.dx_seg(c, n.fp1);
    X.dx_seg(c, n.fp0, &n.op);
    X.dx_seg(c, n.op, &n.tff);
    X.dx_seg(c, n.tff);
    X.dx_seg(c, n.tout);
    if (plan.nigfold) {
      ChainNig& g = c.nig;
      g.enabled = 1;
      g.e2 = reinterpret_cast<const bf16_t*>(L.e2); g.w3 = reinterpret_cast<const bf16_t*>(X.W(P_EV2_W)); g.evid = L.evid;
      g.targets = a->targets; g.stats = L.stats; g.gstats = a->global_stats; g.nblk = nblk; g.nwp = plan.nwp;
      g.dz2 = reinterpret_cast<bf16_t*>(L.dz2); g.partial_w = L.part_w3; g.partial_b = L.part_b3;
      g.loss_out = a->loss_out; g.bin_counts = a->bin_counts; g.mask_scale = X.mask_scale; g.cfg = cfg;
    }
#ifdef MMDEER_STAMPS
    c.stamps = reinterpret_cast<unsigned long long*>(L.davin);   // diagnostic library: untouched until phase 2 (tools/chain_stamps.py bwd)
#endif
    TRY(launch_chain(c, s));
    MARK(plan.nigfold ? "chain B1-B10 (head backward + loss gradient + head / trimodal dX)" : "chain B2-B10 (head / trimodal dX)");
  } else {
    TRY(X.run1(X.dx(n.ev1)));
    TRY(X.run1(X.dx(n.ev0)));
    TRY(X.run1(X.dx(n.fp1)));
    TRY(X.run1(X.dx(n.fp0)));
  }
  // a gradient that reaches fused_features from outside the head (a caller's own consumer of that output)
  if (a->g_fused) TRY(launch_add_f32(L.dfused, f32, a->g_fused, (long long)B * FUS, s));
  add_dw(n.ev1);
  add_dw(n.ev0);
  add_dw(n.fp1);
  add_dw(n.fp0);
  reduce_head(rt, plan.nigfold ? chain_workgroups(B) : nblk);

  // ================= bucket 1: output_projection + trimodal fusion =================
  if (!plan.bchain) {
    TRY(X.ln_bwd(n.op, n.fp0));
    TRY(X.run1(X.dx(n.op)));
    TRY(X.ln_bwd(n.tff, n.op));
    TRY(X.run1(X.dx(n.tff)));
    TRY(X.run1(X.dx(n.tout)));
  }
  if (!plan.bchain) MARK("B2-B10 separate launches");
  if (!f32 && opt(OPT_FUSED_ATTN) && opt(OPT_QKV_RECOMPUTE)) {   // the forward kept q|k|v on chip: recompute the head tiles
    TRY(launch_tri_fused_bwd(L.xtok, L.wqkv_hm, X.V(P_TIN_B), L.dobar, L.probs, L.dqkv, B, X.drop_on ? 1 : 0, X.dc, s));
    MARK("tri_fused_kernel<1> (attention backward, recompute)");
  } else {
    TRY(launch_tri_attn_bwd(L.qkv, L.dobar, L.probs, L.dqkv, B, f32, X.drop_on ? 1 : 0, X.dc, s));
    MARK("attention backward (unfused)");
  }
  TRY(X.run1(X.dx(n.tin)));
  MARK("in_proj dX GEMM");
  // token 0 -> audiovisual features (with the AV chain below, this product is its first segment)
  if (!plan.dchain) TRY(X.run1(X.dx(n.avp)));
  add_dw(n.op);
  add_dw(n.tff);
  add_dw(n.tout);
  add_dw(n.tin);
  add_dw(n.avp);
  add_dw(n.txt);
  X.add_ln_segment(rt, n.op, G, plan.bchain);
  X.add_ln_segment(rt, n.tff, G, plan.bchain);
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
  if (plan.dchain) {
    ChainArgs c = X.chain(n.avp.dout, n.avp.N, 1, B);
    X.dx_seg(c, n.avp, &n.avf);
    X.dx_seg(c, n.avf);
    X.dx_seg(c, n.aout);
    X.dx_seg(c, n.avv);
    TRY(launch_chain(c, s));
    MARK("chain B13-B17 (audio-visual dX)");
  } else {
    TRY(X.ln_bwd(n.avf, n.avp));
    TRY(X.run1(X.dx(n.avf)));
    TRY(X.run1(X.dx(n.aout)));
    TRY(X.run1(X.dx(n.avv)));
  }
  add_dw(n.avf);
  add_dw(n.aout);
  add_dw(n.avv);
  add_dw(n.vid);
  add_dw(n.aud);
  X.add_ln_segment(rt, n.avf, G, plan.dchain);
  if (!plan.dchain) MARK("B13-B17 separate launches");
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
  return launch_nig_stats_sum(L.stats, batch, out, make_plan(batch, compute_f32 ? 1 : 0, 0, false, false, false).nwp, (hipStream_t)stream);
}

}  // extern "C"
