/* mmdeer.h -- C ABI of libmmdeer_hip.so: the MI355X (gfx950) implementation of the
 * multimodal-fusion + DEER forward / loss / backward hot path.
 *
 * The reference has no FFI: its boundary is the Python nn.Module protocol
 * (SURVEY.md 8b).  Each entry point below replaces the torch-op sequence of the
 * cited reference function; the host-side mirror (mmdeer/model.py: MultimodalDEER,
 * compute_loss, DEERTrainer) binds these symbols with ctypes.
 *
 * Conventions
 *  - Plain pointers and sizes only; every buffer (inputs, outputs, parameters,
 *    workspace, gradients) is DEVICE memory owned by the caller.  The library
 *    allocates nothing, reads no environment variable and keeps no state between
 *    calls except the launch-plan option table below (mmdeer_set_option; the
 *    defaults are the shipped plan) and the communicators a caller creates
 *    (mmdeer_comm_init).
 *  - Every call only ENQUEUES work on `stream` (a hipStream_t passed as void*)
 *    and never synchronises the device: calls are graph-capturable.
 *  - Return value: 0 = ok, -1 = error; the message is in mmdeer_last_error()
 *    (thread-local).  No C++ exception crosses the ABI.
 *  - Matrices are row-major.  "act dtype" is fp32 when compute_f32 != 0, else bf16.
 */
#ifndef MMDEER_H_
#define MMDEER_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMDEER_ABI_VERSION 16

/* ---- fixed geometry of the path (reference fusion.py:47-50, deer.py:201-202, configs/config.yaml:13-20).
 * RESTRICTION: mmdeer_forward / mmdeer_backward / mmdeer_adamw_step (the Stack C entry points) are compiled for exactly this
 * geometry -- audio 84, video 256, text 768 -> intermediate 256 -> fusion 512 x 8 heads -> head 256 / 128 / 64 / 4 x 3
 * dimensions: the parameter table (MMDEER_NUM_PARAMS_ABI rows at fixed flat offsets), the workspace layout, the fused
 * projection + attention kernel (512-wide rows, head dimension 64, two tokens) and the NIG head kernels are sized by these
 * constants.  The reference's constructor takes other widths (fusion.py:47-50): for other audio / video / text widths (multiples
 * of 4; fusion 512, intermediate 256, 8 heads) the host mirror runs the fusion as a sequence of the single operators below
 * (mmdeer/generic_fusion.py: mmdeer_gemm, mmdeer_layernorm_*, mmdeer_trimodal_attn_*; pinned by tests/golden/fusion_geom.npz,
 * captured from the reference at 40 / 128 / 300); other fusion / head widths raise NotImplementedError.  The single operators
 * (mmdeer_gemm, mmdeer_layernorm_*, mmdeer_nig_loss, ...) and the Stack B entry points take any sizes that meet their
 * alignment rules (stackb.CompleteDEERModel runs other widths and depths: tests/test_gpu_stackb.py). */
#define MMDEER_AUDIO_DIM 84
#define MMDEER_VIDEO_DIM 256
#define MMDEER_TEXT_DIM 768
#define MMDEER_INTER_DIM 256
#define MMDEER_FUSION_DIM 512
#define MMDEER_NUM_HEADS 8
#define MMDEER_HIDDEN_DIM 256
#define MMDEER_NUM_DIMS 3        /* valence, arousal, dominance */
#define MMDEER_NUM_PARAMS_ABI 50 /* canonical parameter order: mmdeer_param_name(i) */
#define MMDEER_LOSS_OUT 20       /* per dim {total,nll,reg,kl,ece} x3, cross_dim, total, mean nll / reg / kl */

const char* mmdeer_version(void);
int mmdeer_abi_version(void);
const char* mmdeer_last_error(void);

/* canonical parameter table (order of `params` / layout of the flat gradient buffer) */
int mmdeer_num_params(void);
const char* mmdeer_param_name(int i);          /* reference state_dict key with fusion./head. prefix */
int mmdeer_param_rows(int i);
int mmdeer_param_cols(int i);                  /* 1 for vectors */
long long mmdeer_param_offset(int i);          /* element offset in the flat buffers */
long long mmdeer_flat_elems(void);             /* elements of the flat gradient buffer */

/* bytes of `workspace` needed for a batch of B samples (saved activations, backward scratch, split-K slabs) */
size_t mmdeer_workspace_bytes(int batch, int compute_f32);
/* bytes of `weights`: the packed copies of the parameters the kernels read (compute-dtype matrices, their W^T copies,
 * fp32 vectors, the padded audio weight, the head-major in_proj image).  ONE buffer per model and compute dtype, shared
 * by the workspaces of every batch size; written by mmdeer_forward(repack = 1), mmdeer_pack_weights and mmdeer_adamw_step. */
size_t mmdeer_weights_bytes(int compute_f32);

/* Launch-plan options (csrc/options.inc): integer switches that select between kernel plans with IDENTICAL results up to
 * rounding (A/B measurements, debugging); read at every call, so a process may change them between calls.
 *   fused_attn (1)     0: unfused in_proj GEMM + attention kernels also in bf16 mode
 *   qkv_recompute (1)  0: the fused forward stores q|k|v for the backward instead of recomputing the head tiles
 *   ln_fused (1)       0: the LayerNorms of the forward as stand-alone launches instead of inside the consuming GEMM (bf16)
 *   chain (1)          0: every sample-local layer as its own launch; 1 (bf16, chain_min <= B <= 8192): the runs F2-F6 and F9-F17
 *                      of the forward and, with chain_bwd (1), the head / trimodal and the audio-visual dX runs of the backward as
 *                      one launch each
 *   chain_min (512)    smallest batch that takes the chains
 *   chain_max (8192)   largest batch that takes the chains (beyond one round of 32-sample workgroups they lose)
 *   chain_nig (1)      0: the head's last-layer backward + loss gradient as a launch of their own also when the backward chain runs
 *   dw_tile (2)        weight-gradient launch: 2 = 128x128 tiles, K-slices of B rows (no split-K slabs for the B-row problems),
 *                      3 = 256x256 tiles + split-K slabs, 4 = 256x128 tiles; dw_kg (2): 1 = the 128x128 kernel on 32-row K stages
 *   chain_depth (4)    weight stages a wave of the 16-sample chain kernel keeps in flight (2, 4 or 8)
 *   chain_in (1)       0: the input projections as a pad launch + one 3-problem GEMM launch also where the first chain could run them
 *   chain_nigf (0)     1: the NIG head as the tail of the forward head chain (bit-identical, one launch fewer, measured slower)
 *   chain_ts (0)       16 / 32: force the samples per chain workgroup (0: 16 up to B = 4096, 32 above)
 *   dw_fold (1)        bf16 mode, all weight gradients in ONE launch of the DMA kernel: that launch adds its own K-slices (the tile's
 *                      last-arriving slice, in the fold's order), folds the row partials in workgroups behind its tiles and advances
 *                      the dropout counter -- bit-identical, one launch fewer; 0: the reduce_partials launch behind it
 *   adam_fused (1)     bf16 mode: mmdeer_adamw_step's update writes every derived weight image itself (0: element-wise update + repack launch)
 *   xcd, nt128, nt192, glds, nt8 (1), t128 (512), tile (-1), ksteps (0), splitk_max (8)   GEMM tile / split-K selection
 * mmdeer_set_option / mmdeer_get_option return -1 for an unknown name, mmdeer_set_option also for a value outside the option's
 * range (every option has one: booleans 0..1, dw_tile 2..4, dw_kg 1..2, tile -1..4, splitk_max 1..8, chain_depth 2..8, ...; the
 * message names it); mmdeer_option_name(i) enumerates (NULL past the end). */
int mmdeer_set_option(const char* name, int value);
int mmdeer_get_option(const char* name, int* value);
const char* mmdeer_option_name(int i);

/* Launch trace: between mmdeer_trace_begin(events, n) and mmdeer_trace_end() the calling thread's mmdeer_forward / mmdeer_backward
 * record the caller's events (hipEvent_t handles, in order) on the call's stream, one behind every launch or group of launches,
 * and remember a label for each: durations between consecutive events are the launches of THAT run (bench.py reports them in its
 * line).  mmdeer_trace_end returns the number of events recorded; mmdeer_trace_label(i) stays valid until the next trace_begin. */
int mmdeer_trace_begin(void** events, int n_events);
int mmdeer_trace_end(void);
const char* mmdeer_trace_label(int i);

/* Byte offset of a named buffer inside the workspace of (batch, compute_f32), -1 for an unknown name: lets a test read the
 * activations and activation-gradients a step left behind (tests/test_gpu_bf16_layers.py checks every kernel of the bench
 * configuration on its own stored inputs).  Names: every workspace field of csrc/layout.inc, the one list the layout is made of
 * (act dtype unless noted): audio_pad [B,128] bf16,
 * avin avv [2B,256], cat [B,512], y_a2 av [B,256], xtok [2B,512], qkv [2B,1536], obar pool y_t3 tri y_o1 fused [B,512],
 * h1 h2 [B,256], e1 [B,384], e2 [B,192], probs [B,8,4] f32, evid [B,3,4] f32, stats f32, mean_* rstd_* [B] f32, the gradients
 * dz2 de1 dh2 dh1 dfused dz_o1 dtri dz_t3 dpool dobar dqkv dxtok dav dz_a2 dcats davv davin of the same shapes, the fp32 partial
 * slabs part_ln_o1 part_ln_t3 part_ln_a2 part_w3 part_b3 and the split-K slab. */
long long mmdeer_workspace_offset(int batch, int compute_f32, const char* name);
/* The same for the packed-parameter buffer (`weights`): wpack / wtpack (compute-dtype matrices and their transposes at the
 * flat element offsets of mmdeer_param_offset), vpack (fp32 vectors, same offsets), wa_pad ([256][128] bf16 audio weight),
 * wqkv_hm (head-major in_proj image of the fused kernels), wscratch (the optimiser step's partials) and, empty with compute_f32,
 * wfpack / wtfpack (fragment-major images of W / W^T at the flat offsets) and wa_frag (that of wa_pad): every weights field of
 * csrc/layout.inc.  bench.py launches the roofline kernel on the step's operands. */
long long mmdeer_weights_offset(int compute_f32, const char* name);

typedef struct mmdeer_loss_cfg {
  float reg_weight;    /* losses.py:52  0.1  */
  float kl_weight;     /* losses.py:52  0.01 */
  float ece_weight;    /* losses.py:53  0.05 */
  float cross_weight;  /* losses.py:239 0.05 */
  float task_weight[3];/* losses.py:256-259 */
} mmdeer_loss_cfg;

/* Forward of HierarchicalMultimodalFusion (fusion.py:119-171, uncertainties=None) followed by
 * MultiDimensionalDEER (deer.py:233-266).  With `targets` the per-block statistics of
 * MultiTaskDEERLoss (losses.py:268-348) are accumulated in the same pass. */
typedef struct mmdeer_forward_args {
  int32_t batch;
  int32_t compute_f32;      /* 1: exact-fp32 MFMA path (parity config); 0: bf16 MFMA, fp32 accumulate */
  int32_t training;         /* 1: dropout active (counter-based hash keyed by seed/offset) */
  int32_t inputs_bf16;      /* 0: audio/video/text are fp32; 1: bf16 */
  int32_t repack;           /* 1: parameters changed since `weights` was last written */
  float dropout_p;
  uint64_t seed, offset;
  const uint64_t* offset_dev; /* optional device counter added to `offset` when the kernels run: lets a captured HIP
                               * graph draw fresh dropout masks on every replay (NULL: offset alone) */
  int32_t bump_offset_dev;  /* 1 (bf16 compute only; a training step = this call + mmdeer_backward with the same flag): every kernel
                             * of the step uses *offset_dev + 1 and the LAST launch of mmdeer_backward stores the incremented
                             * counter, so a replayed graph draws fresh masks without a counter kernel of its own */
  const void* audio;        /* [B, 84]  */
  const void* video;        /* [B, 256] */
  const void* text;         /* [B, 768] */
  const void* const* params;/* MMDEER_NUM_PARAMS_ABI fp32 device pointers, canonical order */
  void* workspace;
  size_t workspace_bytes;
  void* weights;            /* mmdeer_weights_bytes(compute_f32) bytes, 256-byte aligned */
  size_t weights_bytes;
  /* fp32 outputs; any may be NULL */
  float* nig_out;           /* [7][B][3]: mu, nu, alpha, beta, aleatoric, epistemic, uncertainty (deer.py:100-108) */
  float* fused_features;    /* [B, 512]  fusion.py:165 */
  float* audiovisual_features; /* [B, 256] */
  float* trimodal_features; /* [B, 512] */
  float* av_attention;      /* [B, 2]: audio_to_video, video_to_audio  (fusion.py:267-270) */
  float* trimodal_attention;/* [B, 2, 2]                               (fusion.py:342) */
  const float* targets;     /* [B, 3] or NULL */
  /* optional hipEvent_t pair recorded immediately before / after the trimodal in_proj GEMM launch
   * (M = 2B, K = 512, N = 1536 -- the roofline kernel of BASELINE.json); NULL = not recorded */
  void* prof_events[2];
  void* stream;
} mmdeer_forward_args;

int mmdeer_forward(const mmdeer_forward_args* a);

/* Backward through the whole path, using the activations `mmdeer_forward` left in `workspace`.
 *   loss mode  (targets != NULL): d MultiTaskDEERLoss / d parameters; loss_out / bin_counts are filled.
 *   chain mode (targets == NULL): g_mu/g_nu/g_alpha/g_beta [B,3] are upstream gradients (each may be NULL).
 * grads: flat fp32 buffer of mmdeer_flat_elems() elements, ZERO-INITIALISED ONCE by the caller: every slice that
 * receives a gradient is overwritten by each call; the 64-element alignment gaps and the q/k thirds of the AV
 * in_proj (which the reference also leaves at exactly zero: L = S = 1) are never written and keep those zeros.  The never-written
 * q/k words are also the weight-gradient launch's tile counters (option dw_fold) and are zero again when that launch ends. */
typedef struct mmdeer_backward_args {
  int32_t batch;
  int32_t compute_f32;
  int32_t training;
  int32_t inputs_bf16;
  float dropout_p;
  uint64_t seed, offset;    /* the values given to the matching mmdeer_forward */
  const uint64_t* offset_dev;
  const void* audio;
  const void* video;
  const void* text;
  void* workspace;
  size_t workspace_bytes;
  void* weights;            /* the buffer the matching mmdeer_forward read */
  size_t weights_bytes;
  const float* targets;
  const float* g_mu;
  const float* g_nu;
  const float* g_alpha;
  const float* g_beta;
  mmdeer_loss_cfg loss;
  float* grads;
  float* loss_out;          /* [MMDEER_LOSS_OUT] or NULL */
  int32_t* bin_counts;      /* [3][10] ECE bin populations or NULL */
  /* optional: hipEvent_t handles recorded when a gradient bucket of the flat buffer is final:
   * bucket 0 = head (params 28..49), 1 = output_projection + trimodal (12..27), 2 = audio-visual (0..11).
   * All weight gradients are produced by one grouped launch at the end of the pass (or of phase 1), so the events of
   * the buckets it covers are recorded together. */
  void* bucket_events[3];
  /* 0: the whole backward pass.  1 / 2: the pass in two calls -- 1 = head + output_projection + trimodal fusion
   * including their weight gradients (buckets 0 and 1 of the flat buffer are final when it returns), 2 = the
   * audio-visual remainder (bucket 2).  Lets a data-parallel caller start the all-reduce of buckets 0-1 (89 % of
   * the gradient) while part 2 runs.  Both calls take the same arguments; 1 must precede 2. */
  int32_t phase;
  int32_t bump_offset_dev;  /* as given to the matching mmdeer_forward (phase 1 and 2 both; the counter advances at the end of 2) */
  /* Exact-global loss for data parallelism (optional): MMDEER_GLOBAL_STATS floats = the loss statistics of
   * ALL ranks' batches (every rank calls mmdeer_loss_stats after its forward and the host sums the vectors across
   * ranks, e.g. mmdeer_allreduce with average = 0).  The ECE and cross-dimension terms are non-linear in these batch
   * statistics; with them the loss written to loss_out is that of the global batch on every rank and the gradients are
   * each rank's share of ITS gradient -- exchange them with a SUM, not a mean.  NULL: the statistics of this call's own
   * batch (DDP semantics, the default).  Used with `targets` only. */
  const float* global_stats;
  /* Optional upstream gradient wrt the fused_features output [B][512] fp32 (a consumer of that output other than the
   * DEER head): added to the head's own gradient before the output_projection backward.  Either mode. */
  const float* g_fused;
  void* stream;
} mmdeer_backward_args;

int mmdeer_backward(const mmdeer_backward_args* a);

/* Loss statistics of the batch whose forward (with targets) last ran on `workspace`: out[3][35] per-dimension sums
 * (5 loss sums + 10 ECE bins x {sum confidence, sum error, count}) followed by out[105] = batch.  All entries are plain
 * sums over samples, so adding the vectors of several ranks gives the statistics of the union of their batches. */
#define MMDEER_GLOBAL_STATS 106
int mmdeer_loss_stats(const void* workspace, size_t workspace_bytes, int batch, int compute_f32, float* out, void* stream);

/* bucket boundaries used by bucket_events: elements [mmdeer_bucket_begin(i), mmdeer_bucket_end(i)) of the flat buffer */
long long mmdeer_bucket_begin(int bucket);
long long mmdeer_bucket_end(int bucket);

/* ---- single operators (unit tests, and the building blocks of the two calls above) ---------------- */

/* C[M,N] = act(A[M,K] * W[N,K]^T + bias) with optional dropout; the `linear_act` part of SURVEY 8b.
 * a_f32 / w_f32 / c_f32: storage dtypes (1 fp32, 0 bf16).  trans_a / trans_w: operand stored [K][rows]. */
typedef struct mmdeer_gemm_args {
  const void* A; const void* W; void* C; const float* bias; float* bias_grad; const void* Y;
  int32_t M, N, K, lda, ldw, ldc, ldy;
  int32_t a_f32, w_f32, c_f32, y_f32, trans_a, trans_w, relu, accumulate;
  int32_t compute_f32, tile;            /* tile: 0 = 64x64, 1 = 128x64, 2 = 128x128, 3 = 256x256, 4 = 256x128 (bf16 dW), -1 = auto */
  int32_t drop_site, drop_shift, regen_site;
  float dropout_p, mask_scale;
  uint64_t seed, offset;
  const uint64_t* offset_dev; /* optional device counter added to `offset` when the kernel runs (HIP-graph replays draw fresh masks) */
  /* split-K (weight-gradient shapes: few output tiles, long reduction): splitk > 1 reduces K in slices whose fp32
   * partials go to `slab` (splitk * (M*N + M) floats, rounded up to a multiple of 4 per slice, 16-byte aligned) and are
   * then summed in a fixed order; needs an fp32 C and no epilogue.  A problem with ldc != N, a C not 16-byte aligned, or a
   * bias_grad with M % 4 != 0 or not 16-byte aligned is not split (one workgroup per tile runs its whole reduction). */
  int32_t splitk;
  float* slab;
  void* debug;   /* diagnostic builds (-DMMDEER_STAMPS) only: uint64 buffer for in-kernel cycle stamps; NULL otherwise */
  void* stream;
} mmdeer_gemm_args;
/* Writes C[r][0, N) for r < M (row stride ldc), bias_grad[0, M) when given, and, when the problem is split, the first
 * splitk * (M*N + M rounded up to 4) floats of `slab`; nothing else (M = 0 writes nothing).  Operand elements past K (past M /
 * N for a transposed operand) and rows past the operand are never read into a stored output.  Refuses (-1, writing nothing,
 * message in mmdeer_last_error()) unless: A, W, C non-NULL; N % 4 == 0; K % 4 == 0 for a k-contiguous operand; M % 4 == 0 for a
 * transposed A; lda, ldw, ldc (and ldy with Y) multiples of 4 with lda >= (trans_a ? M : K), ldw >= (trans_w ? N : K),
 * ldc >= N, ldy >= N; A and W 16-byte aligned, C 8-byte aligned; accumulate only with an fp32 C; splitk > 1 only with a slab, an
 * fp32 C and no epilogue (bias, relu, Y, accumulate, drop_site, regen_site); fp32 compute only with fp32 operands; not
 * (trans_a = 1, trans_w = 0).  Under bf16 compute an operand is read as fp32 (converted), as bf16 in 16-byte chunks (ld % 8 == 0
 * and extent % 8 == 0) or as bf16 in 8-byte chunks, and only these (A, W) pairs are instantiated -- (trans_a, trans_w) = (0, 0):
 * (16, 16), (f32, 16), (f32, 8), (8, 8); (0, 1): (16, 16), (16, 8); (1, 1): (16, 16), (16, f32), (16, 8).  Exception: a transposed
 * bf16 operand with extent % 8 != 0 and ld >= extent rounded up to 8 is read in 16-byte chunks when the call runs on the
 * weight-gradient DMA kernel (tile 3 or 4, or tile 2 under option dw_tile = 2; both operands bf16, K % 32 == 0, a 16-byte aligned
 * fp32 C, no epilogue but bias_grad / accumulate), so such an A is accepted there and refused elsewhere. */
int mmdeer_gemm(const mmdeer_gemm_args* a);
/* Dry run of mmdeer_gemm: everything it does before its first launch (argument checks, split decision, tile, operand source modes,
 * kernel route), touching no GPU and dereferencing no operand pointer.  Writes one line per launch the call would make into
 * out[cap] (NUL-terminated, lines separated by '\n'; truncated to fit), "<kernel> <BM>x<BN>[ <variant>] a=<mode> b=<mode> tiles=<workgroups>":
 * kernel nt_reg / nx_reg / tt_reg (register-staged), nt_glds (LDS-DMA, variant w4 / w8 = waves), nt256 (256-row forward), tt_dma
 * (weight-gradient LDS-DMA, variant k1 / k2 = K halves per stage); mode f32 / v16 / v8 as mmdeer_gemm's comment lists them.  Returns the
 * number of launches (M = 0: 0), or -1 with the message of mmdeer_last_error() exactly where mmdeer_gemm would refuse. */
int mmdeer_gemm_route(const mmdeer_gemm_args* a, char* out, int cap);

/* n weight-gradient problems (every one trans_a = trans_w = 1, fp32 C, no epilogue; the same compute dtype) as grouped
 * launches of up to 16 problems each + one deterministic fold of their split-K slabs per group -- the form in which
 * mmdeer_backward runs all its weight gradients in ONE launch, for operator sequences built outside the library (Stack B
 * training, mmdeer/stackb_train.py).  `splitk` / `slab` of the individual problems are ignored: the slices are carved out of
 * `slab` (slab_elems floats; mmdeer_gemm_batch_slab_elems gives the need) with the library's own split policy.
 * Writes C[r][0, N) (row stride ldc) and bias_grad[0, M) of every problem and the first mmdeer_gemm_batch_slab_elems floats of
 * `slab`, nothing else.  Refuses (-1, writing nothing) unless every problem has M, N multiples of 4, lda >= M, ldw >= N, ldc >= N
 * (multiples of 4), 16-byte aligned A / W, and the slab (16-byte aligned) holds the need.  A problem with ldc != N or an unaligned
 * C / bias_grad is not split (one workgroup per tile runs its whole reduction), so acceptance never depends on K. */
long long mmdeer_gemm_batch_slab_elems(const mmdeer_gemm_args* a, int n);
int mmdeer_gemm_batch(const mmdeer_gemm_args* a, int n, float* slab, long long slab_elems, void* stream);

/* n folds in ONE launch: dst[i][j] = sum over p < nparts[i] of src[i][p * stride[i] + j], j < count[i] (count and stride
 * multiples of 4, 16-byte aligned pointers; fixed order: deterministic).  nparts = 1 is a copy.  Operator sequences collect
 * the LayerNorm gamma / beta partials of mmdeer_layernorm_bwd(dgamma = NULL) and their gradient slices here instead of
 * paying one small launch each (up to 48 segments per launch; more are split over several).  Writes dst[i][0, count[i]) only;
 * refuses (-1, writing nothing) if any segment has nparts < 1, count or stride not a multiple of 4, or a pointer not 16-byte aligned. */
int mmdeer_reduce_batch(int n, const float* const* src, float* const* dst, const int32_t* nparts, const int32_t* count,
                        const long long* stride, void* stream);

/* n transposed compute-dtype copies in ONE launch: for matrix i (fp32, rows[i] x cols[i], row-major, dense) W^T[c][r] is
 * written to dst + dst_off[i] + c * ld_dst[i] + dst_col[i] + r (elements of the compute dtype; ld_dst 0 = rows[i]): dX = dY W
 * then runs as an NT GEMM on the LDS-DMA kernels.  Up to 32 matrices per launch (more are split).  Writes those rows * cols elements
 * only (bf16: round to nearest even, NaN stays NaN); refuses (-1, writing nothing) if any matrix has no source, rows or cols < 1, a
 * negative dst_off / dst_col / ld_dst, or ld_dst != 0 with dst_col + rows > ld_dst. */
int mmdeer_pack_transposed_batch(int n, const float* const* src, const int32_t* rows, const int32_t* cols, void* dst,
                                 const long long* dst_off, const int32_t* ld_dst, const int32_t* dst_col, int dst_f32, void* stream);

/* nn.LayerNorm(N), eps 1e-5 (fusion.py:102, 220, 305); out32 (fp32 copy of out) is optional.  Refuses (-1, before any launch) N <= 0,
 * N % 4 != 0, N > 1024, M < 0 and, when M > 0, a NULL y / out / mean / rstd / gamma / beta.  M = 0 writes nothing. */
int mmdeer_layernorm_fwd(const void* y, void* out, float* out32, float* mean, float* rstd, const float* gamma,
                         const float* beta, int M, int N, int act_f32, void* stream);
int mmdeer_layernorm_bwd_nparts(int M);   /* ceil(M / 16): one partial slab per 16 consecutive rows */
/* dz = (y > 0) * mask_scale * LayerNorm'(dout): the ReLU (+ dropout, mask_scale = 1 / (1 - p)) of the Linear-ReLU-Dropout-LayerNorm
 * blocks folded in; mask_scale <= 0: no mask (a LayerNorm behind a plain Linear, encoders.py:113-114).  partial: scratch of
 * mmdeer_layernorm_bwd_nparts(M) * 2 * N floats ([part][d gamma row | d beta row]); with dgamma = dbeta = NULL the fold of
 * the partials is left to the caller (mmdeer_reduce_batch: nparts = mmdeer_layernorm_bwd_nparts(M), stride = 2 N).
 * Refuses (-1, before any launch) N <= 0, N % 4 != 0, N > 1024, M < 0, a NULL partial, one of dgamma / dbeta without the other and,
 * when M > 0, a NULL dout / y / mean / rstd / gamma / dz.  M = 0 zeroes the one partial slab (and so dgamma, dbeta) and touches nothing else. */
int mmdeer_layernorm_bwd(const void* dout, const void* y, const float* mean, const float* rstd, const float* gamma,
                         void* dz, float* dgamma, float* dbeta, float* partial, int M, int N, int act_f32,
                         float mask_scale, void* stream);

/* 2-token, 8-head self-attention of TrimodalFusion (fusion.py:325-335) on a [2B,1536] q|k|v matrix; attn_w [B][2][2] and av_w [B][2]
 * are optional.  Both refuse (-1, before any launch) B < 0 and, when B > 0, a NULL qkv / obar / probs (backward: qkv / dobar / probs /
 * dqkv).  B = 0 writes nothing. */
int mmdeer_trimodal_attn_fwd(const void* qkv, void* obar, float* probs, float* attn_w, float* av_w, int B,
                             int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream);
int mmdeer_trimodal_attn_bwd(const void* qkv, const void* dobar, const float* probs, void* dqkv, int B,
                             int act_f32, int training, float dropout_p, uint64_t seed, uint64_t offset, void* stream);

/* The same attention with the packed in_proj FUSED in (bf16 compute; reference fusion.py:328-335, i.e. the
 * F.multi_head_attention_forward call behind nn.MultiheadAttention: in_proj -> scaled 2x2 scores -> softmax -> dropout -> P V,
 * followed by the mean over the two tokens that fusion.py:335 applies after out_proj and that commutes with it).
 *   mmdeer_pack_qkv_headmajor: in_proj_weight fp32 [1536][512] -> the head-major bf16 operand image (1536*512 bf16) the
 *                              fused kernels read; redo after every parameter update.
 *   mmdeer_trimodal_fused_fwd: xtok bf16 [2B][512] (row 2b + t) -> obar bf16 [B][512], probs fp32 [B][8][4]; q|k|v stay
 *                              on chip unless qkv_out (bf16 [2B][1536], optional) is given.  attn_w / av_w as above, optional.
 *   mmdeer_trimodal_fused_bwd: recomputes q|k|v per head tile and writes dqkv bf16 [2B][1536] from dobar bf16 [B][512]
 *                              and the saved probs.
 * Rounding points: the scores are products of q and k ROUNDED to bf16 (the values qkv_out holds), v enters P V and q, k, v enter the
 * backward unrounded.  The softmax over the two keys is stated with a clamp:
 *   probs[t][t] = 1 / (1 + 2^min((s[t][1-t] - s[t][t]) * log2(e) / 8, 115)),   probs[t][1-t] = 2^min(..) * probs[t][t],
 * so a key that loses by more than 115 ln 2 = 79.7 after the 1/8 keeps the probability 2^-115 (2.4e-35) where the true one is smaller,
 * and the winner's is 1.
 * Batch ceiling: both refuse (-1, before any launch) B > 2^21 - 1 = 2097151: obar and probs are addressed with 32-bit byte ranges and
 * offsets (B * 1024 bytes of obar must stay below 2^31).  Both also refuse B < 0 and, when B > 0, a NULL xtok / whm / bias / obar /
 * probs (backward: xtok / whm / bias / dobar / probs / dqkv).  B = 0 writes nothing. */
int mmdeer_pack_qkv_headmajor(const float* in_proj_weight, void* whm_bf16, void* stream);
int mmdeer_trimodal_fused_fwd(const void* xtok, const void* whm_bf16, const float* in_proj_bias, void* obar, float* probs,
                              void* qkv_out, float* attn_w, float* av_w, int B, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* stream);
int mmdeer_trimodal_fused_bwd(const void* xtok, const void* whm_bf16, const float* in_proj_bias, const void* dobar,
                              const float* probs, void* dqkv, int B, int training, float dropout_p, uint64_t seed,
                              uint64_t offset, void* stream);

/* MultiTaskDEERLoss on given NIG parameters [B,3] (losses.py:268-348); gradients optional (all four or none).
 * stats: scratch of mmdeer_nig_stats_elems(B) floats. */
long long mmdeer_nig_stats_elems(int B);
int mmdeer_nig_loss(const float* gamma, const float* nu, const float* alpha, const float* beta, const float* targets,
                    float* stats, float* dgamma, float* dnu, float* dalpha, float* dbeta, float* loss_out,
                    int32_t* bin_counts, int B, const mmdeer_loss_cfg* cfg, void* stream);

/* ---- the other loss classes of the path (a10, a13).  All tensors fp32, dense; gradient pointers are all
 * NULL (values only) or all set (gradient of the total, scaled for a mean over the n elements).
 *
 * deer.DEERLoss.forward (reference src/models/deer.py:125-195, loss variant 1) on n elements (mu, nu, alpha, beta and
 * targets of one shape): loss_out[5] = total, nll_loss, evidence_reg, kl_reg, mse with
 * total = mean(nll) + evidence_weight * mean(reg) + kl_weight * mean(clamp(kl, 0)); the clamp passes the gradient where
 * kl >= 0.  scratch: mmdeer_deer_loss_v1_scratch(n) floats (4 per block of 256 elements), written in full and no further.
 * Refused (-1, nothing written): a NULL tensor, n <= 0, one to three of the four gradient pointers. */
long long mmdeer_deer_loss_v1_scratch(long long n);
int mmdeer_deer_loss_v1(const float* mu, const float* nu, const float* alpha, const float* beta, const float* targets,
                        long long n, float evidence_weight, float kl_weight, float* loss_out, float* dmu, float* dnu,
                        float* dalpha, float* dbeta, float* scratch, void* stream);
/* losses.UncertaintyRegularizationLoss.forward with flat keys (src/utils/losses.py:363-416): alpha, beta [B][D], D <= 8;
 * loss_out[3] = reg_loss (= dw * diversity + sw * sparsity), diversity_loss, sparsity_loss.  The variance is the unbiased
 * one: B = 1 gives NaN in reg_loss, diversity_loss and every gradient element, as the reference does (sparsity_loss stays
 * finite).  Refused (-1, nothing written): B <= 0, D outside 1..8, one gradient pointer of the two. */
int mmdeer_uncertainty_reg_loss(const float* alpha, const float* beta, int B, int D, float diversity_weight,
                                float sparsity_weight, float* loss_out, float* dalpha, float* dbeta, void* stream);
/* losses.CalibrationLoss.forward, n_bins = 15, 'uniform' (src/utils/losses.py:431-497) on n flattened elements:
 * loss_out[1]; bin_counts[15] (optional) are the exact bin populations.  The bin edges are the embedded fp32 values of
 * torch.linspace(0, 1, 16): the same bits as mmdeer_calibration_loss_bins with that table.  Bin k is [edge k, edge k + 1),
 * the last bin is closed on the right; a confidence outside [0, 1] (alpha < 1) is in no bin and carries a zero gradient.
 * u = beta / (alpha - 1 + 1e-8) = inf in fp32 gives confidence 0 (bin 0) and, as in the fp32 reference program, NaN in
 * that sample's dalpha (0 * inf) and 0 in its dbeta.  The error clamp passes dgamma for 0 <= |y - gamma| / 2 <= 1. */
int mmdeer_calibration_loss(const float* gamma, const float* alpha, const float* beta, const float* targets, long long n,
                            float* loss_out, int32_t* bin_counts, float* dgamma, float* dalpha, float* dbeta, void* stream);
/* The same with any number of uniform bins (1 <= n_bins <= 32): `edges` is a HOST array of n_bins + 1 fp32 bin boundaries,
 * torch.linspace(0, 1, n_bins + 1) as fp32 evaluates it (the reference's rule, losses.py:459); bin_counts[n_bins].
 * Refused (-1, nothing written): n <= 0, n_bins outside 1..32, one or two of the three gradient pointers. */
int mmdeer_calibration_loss_bins(const float* gamma, const float* alpha, const float* beta, const float* targets, long long n,
                                 const float* edges, int n_bins, float* loss_out, int32_t* bin_counts, float* dgamma, float* dalpha,
                                 float* dbeta, void* stream);

/* keep-mask of one dropout site, for test harnesses: out[r*cols + c] in {0,1}.  Refuses (-1, before any launch) a NULL out and a
 * negative rows or cols; rows * cols = 0 writes nothing. */
int mmdeer_dropout_mask(int site, int rows, int cols, float dropout_p, uint64_t seed, uint64_t offset,
                        unsigned char* out, void* stream);

/* ---- optimiser step on the device (reference src/training/training.py:121-150, 219-224) ------------
 * clip_grad_norm_(max_grad_norm) + torch.optim.AdamW (decoupled weight decay, eps 1e-8 in the reference) on the flat
 * gradient buffer of mmdeer_backward.  Updates the fp32 master parameters in place and refreshes, in `weights`,
 * the packed copies mmdeer_forward / mmdeer_backward read -- so the next mmdeer_forward may pass repack = 0.
 * `lr` is a HOST array with one learning rate per live parameter (ABI order): the reference's three parameter
 * groups (0.5 lr for names containing "encoder", lr otherwise) reduce to that.  No host synchronisation.
 * The 64-element alignment gaps between the parameters in the flat buffers are NEITHER READ NOR WRITTEN, in every launch plan:
 * whatever `grads` holds there does not enter the norm, and the gaps of exp_avg / exp_avg_sq keep their values.
 * In `weights` the call writes what mmdeer_pack_weights would write for the updated parameters, byte for byte, and the
 * wscratch field (its sum-of-squares partials); bytes that belong to no image (vector positions of wpack, matrix positions of
 * vpack, W^T positions of matrices without a dX, the padding between fields) are left alone.  With pack_transposed = 0 the
 * two fields that hold W^T -- wtpack and wtfpack -- are left alone entirely and every other field is written as with 1. */
typedef struct {
  int32_t compute_f32;        /* dtype of the packed matrices, as in mmdeer_forward */
  int32_t pack_transposed;    /* 1: also refresh the W^T copies used by mmdeer_backward (fields wtpack, wtfpack); 0: leave both alone */
  int32_t step;               /* 1-based step count t (bias corrections 1 - beta^t) */
  float beta1, beta2, eps, weight_decay;
  float max_grad_norm;        /* > 0: gradients *= min(1, max_grad_norm / (||g||_2 + 1e-6)); <= 0: no clipping */
  float grad_scale;           /* gradients are multiplied by this first (dataset weight); 1 = none */
  const float* lr;            /* host array [mmdeer_num_params()] */
  void** params;              /* fp32 master parameters (device), canonical order, updated in place */
  const float* grads;         /* flat gradient buffer, mmdeer_flat_elems() floats; the gaps are not read */
  float* exp_avg;             /* flat first moments  (mmdeer_flat_elems() floats, zero before the first step) */
  float* exp_avg_sq;          /* flat second moments */
  float* grad_norm;           /* device scalar out (may be NULL): global gradient norm before clipping */
  void* weights;              /* mmdeer_weights_bytes(compute_f32) bytes */
  size_t weights_bytes;
  void* stream;
} mmdeer_adamw_args;
int mmdeer_adamw_step(const mmdeer_adamw_args* a);

/* The same update (clip_grad_norm_ + torch.optim.AdamW, training.py:121-150, 219-224) for ANY model whose parameters,
 * gradients and moments live in flat fp32 buffers with common offsets (Stack B: mmdeer/stackb.py): up to 56 learning-rate
 * segments [seg_begin[i], seg_begin[i] + seg_elems[i]) (offsets and lengths multiples of 4 elements), global norm over the
 * gradients of the segments (values outside every segment are neither read for the norm nor written).  `packed` (optional):
 * compute-dtype copy of the updated parameters at the same offsets (packed_f32 = 0: bf16), what the operator sequence's GEMMs
 * read.  Writes params, exp_avg, exp_avg_sq and packed inside the segments, scratch and grad_norm; refuses (-1, writing nothing)
 * more than 56 segments, a segment past flat_elems or not 4-element aligned. */
typedef struct mmdeer_adamw_flat_args {
  float* params; const float* grads; float* exp_avg; float* exp_avg_sq;
  void* packed; int32_t packed_f32;
  long long flat_elems;
  int32_t nseg; const long long* seg_begin; const long long* seg_elems; const float* seg_lr;
  float* scratch;            /* 256 floats */
  float* grad_norm;          /* optional device scalar: global norm before clipping */
  int32_t step;              /* 1-based */
  float beta1, beta2, eps, weight_decay, max_grad_norm, grad_scale;
  void* stream;
} mmdeer_adamw_flat_args;
int mmdeer_adamw_flat(const mmdeer_adamw_flat_args* a);

/* Refresh every packed copy of the parameters in `weights` (the compute-dtype matrices, their W^T copies, the padded
 * audio weight, the head-major in_proj image) without running a pass -- what mmdeer_forward does when repack = 1.  For a
 * caller that replays a captured graph (repack = 0 is frozen into it) after something other than mmdeer_adamw_step
 * changed the parameters. */
int mmdeer_pack_weights(const void* const* params, void* weights, size_t weights_bytes, int compute_f32, void* stream);

/* ---- side rows (a8, a9, a14) ----------------------------------------------------------------------
 * Their Linear(+ReLU) layers run on mmdeer_gemm and the LayerNorm on mmdeer_layernorm_fwd; the two entry points
 * below are the parts that are neither.
 *
 * deer.CrossModalAttention.forward core (reference src/models/deer.py:399-423), feature_dim 256, 8 heads:
 * q = query_proj(text), k_x / v_x = key_proj / value_proj(audio | video), each [B][256] with row stride ld;
 * scores (q.k)/sqrt(32) per head, softmax over the HEAD axis, head-collapsing weighted sum -> [B][32], times the
 * softmax of gate_logits [B][2] (the output of uncertainty_gate's last Linear).  Outputs fp32 [B][32]. */
int mmdeer_cross_modal_attn_fwd(const void* q, const void* k_audio, const void* v_audio, const void* k_video,
                                const void* v_video, int ld, const float* gate_logits, float* out_audio, float* out_video,
                                int B, int act_f32, void* stream);

/* backward of the above: g_audio / g_video fp32 [B][32] -> dq, dk_*, dv_* (act [B][256], row stride ld) and the gradient at the
 * two gate logits (fp32 [B][2]).  Recomputes the softmaxes from the saved projections. */
int mmdeer_cross_modal_attn_bwd(const void* q, const void* k_audio, const void* v_audio, const void* k_video, const void* v_video,
                                int ld, const float* gate_logits, const float* g_audio, const float* g_video, void* dq, void* dk_audio,
                                void* dv_audio, void* dk_video, void* dv_video, float* dgate_logits, int B, int act_f32, void* stream);

/* nn.LSTM cell at T = 1 with zero initial state (reference src/models/encoders.py:82-89, 380; torch gate order
 * i, f, g, o): gates [B][ndir*4*hidden] = W_ih x + b_ih + b_hh per direction ->
 * out[b][dir*hidden + j] = sigmoid(o) * tanh(sigmoid(i) * tanh(g)). */
int mmdeer_lstm_cell_t1(const void* gates, int ld_gates, void* out, int ld_out, int B, int hidden, int ndir, int act_f32,
                        void* stream);
/* d out -> d gates (act [B][ld_gates]; the forget-gate block is written as zeros: it multiplies c0 = 0) */
int mmdeer_lstm_cell_t1_bwd(const void* gates, int ld_gates, const void* dout, int ld_dout, void* dgates, int B, int hidden, int ndir,
                            int act_f32, void* stream);

/* ---- temporal audio encoder (reference src/models/encoders.py:376-389 at T > 1): one bidirectional nn.LSTM layer over all T
 * steps in ONE launch per pass (no workgroup waits on another; the launch count does not grow with T), and the attention pool
 * over time.  hidden (H) must be 256 and ndir 2; "act" = fp32 when act_f32 != 0, else bf16.  Every row index below is
 * t * B + b (time-major).  Pointers that the kernels read or write 16 bytes at a time (the images, the tape, and the rows of
 * xg / h / dh_out / dgates: pointer 16-byte aligned, leading dimension a multiple of 16 bytes) are refused when misaligned.
 * B = 0 or T = 0 writes nothing and returns 0.  A refused call (NULL pointer, H != 256, ndir != 2, leading dimension too
 * small, misalignment) writes nothing, returns -1 and leaves the reason in mmdeer_last_error(); all of that is checked on
 * the host before any HIP runtime call.
 *
 * mmdeer_lstm_seq_pack: the recurrent weights' device images, from the two directions' fp32 weight_hh [4H][H]:
 * image [2][4H][H] (row-major, act; read by the forward) and, unless image_t is NULL, image_t [2][H][4H] (the transpose, act;
 * read by the backward).
 *
 * mmdeer_lstm_seq_fwd: zero initial h and c, torch gate order i, f, g, o.
 *   xg      act [T*B][ld_xg >= 8H]: W_ih x_t + b_ih + b_hh, direction d in columns [4H d, 4H (d+1))
 *   h       act [T*B][ld_h >= 2H]: written, direction d in columns [H d, H (d+1)); the reverse direction reads x_{T-1} .. x_0 and
 *           its state after consuming x_t is stored at row t
 *   tape_gates fp32 [T*B][8H] dense: the activated gates sigmoid(i), sigmoid(f), tanh(g), sigmoid(o); tape_c fp32 [T*B][2H]
 *           dense: the cell state.  Both NULL (inference): no tape is written.
 * mmdeer_lstm_seq_bwd: backpropagation through time from dh_out act [T*B][ld_dh >= 2H] (the gradient at h), the tape and
 *   w_hh_t -> dgates act [T*B][ld_dg >= 8H], the gradient at xg.  The caller forms dW_hh = sum_t dgates_t^T h_{t-1} (forward
 *   direction; h_{t+1} for the reverse), dW_ih, the bias gradients and dx with mmdeer_gemm. */
typedef struct mmdeer_lstm_seq_args {
  const void* xg; int32_t ld_xg;
  const void* w_hh;          /* image of mmdeer_lstm_seq_pack */
  const void* w_hh_t;        /* image_t of mmdeer_lstm_seq_pack (backward) */
  void* h; int32_t ld_h;
  float* tape_gates; float* tape_c;
  const void* dh_out; int32_t ld_dh;
  void* dgates; int32_t ld_dg;
  int32_t T, B, hidden, ndir, act_f32;
  void* stream;
} mmdeer_lstm_seq_args;
int mmdeer_lstm_seq_pack(const float* w_hh_fwd, const float* w_hh_rev, int hidden, void* image, void* image_t, int act_f32, void* stream);
int mmdeer_lstm_seq_fwd(const mmdeer_lstm_seq_args* a);
int mmdeer_lstm_seq_bwd(const mmdeer_lstm_seq_args* a);

/* Attention pool over time: s_{b,t} = w2 . tanh(z_{b,t}) + b2[0], a_{b,t} = softmax over t (max-subtracted),
 * attended_b = sum_t a_{b,t} h_{b,t}.
 *   h act [T*B][ld_h >= 2H] (the LSTM output), z act [T*B][ld_z >= H] (W1 h + b1, from mmdeer_gemm), w2 fp32 [H], b2 fp32 [1]
 *   forward writes attended act [B][ld_att >= 2H] and weights fp32 [B][T]
 *   backward reads weights and dout act [B][ld_dout >= 2H] and writes dh act [T*B][ld_dh >= 2H] = a_t dout (the score path's
 *   share, dz W1, is the caller's GEMM), dz act [T*B][ld_dz >= H], dw2 fp32 [H] and db2 fp32 [1].  db2 is written as an exact
 *   zero: b2 shifts every score of a sample equally and the softmax does not see it.  scratch: fp32, at least
 *   MMDEER_TEMPORAL_POOL_SCRATCH elements (dw2's per-workgroup partials, folded in a fixed order: deterministic). */
#define MMDEER_TEMPORAL_POOL_SCRATCH (256 * 256)
typedef struct mmdeer_temporal_pool_args {
  const void* h; int32_t ld_h;
  const void* z; int32_t ld_z;
  const float* w2; const float* b2;
  void* attended; int32_t ld_att;
  float* weights;
  const void* dout; int32_t ld_dout;
  void* dh; int32_t ld_dh;
  void* dz; int32_t ld_dz;
  float* dw2; float* db2; float* scratch;
  int32_t T, B, hidden, act_f32;
  void* stream;
} mmdeer_temporal_pool_args;
int mmdeer_temporal_pool_fwd(const mmdeer_temporal_pool_args* a);
int mmdeer_temporal_pool_bwd(const mmdeer_temporal_pool_args* a);

/* ---- temporal text encoder (reference src/models/encoders.py:648-746; csrc/token_pool.hip).  Rows are batch-major: row
 * b * L + t.  The widths are fixed: E = 768 (`width`) and A = 384 (`att_width`); others are refused.  L is arbitrary.  Every
 * refusal (NULL or misaligned pointers, leading dimensions too small or misaligned, widths, negative B / L) is decided on the
 * host before any HIP call; B == 0 or L == 0 writes nothing and returns 0.  Activation rows ("act") need 16-byte alignment:
 * pointer % 16 == 0 and ld % (4 fp32 | 8 bf16) == 0.  mask is fp32 [B][L] and is taken as BINARY: m = 1 where it is nonzero.
 *
 * mmdeer_token_embed_fwd: the gather.  Either the tables (ids int64 [B][L], emb fp32 [V][768], pos fp32 [P][768], V < 2^24)
 *   or src fp32 [B*L][ld_src >= 768] (precomputed embeddings) with the tables NULL.
 *     tables: x = (emb[clamp(id, 0, V-1)] + pos[min(t, P-1)]) * m     and ids32 int32 [B*L] = the clamped ids
 *     src:    x = src * m
 *   x is act [B*L][ld_x >= 768].
 * mmdeer_token_embed_bwd: from dx act [B*L][ld_dx >= 768] and the mask, either d_src fp32 [B*L][ld_dsrc >= 768] = dx * m, or
 *   both table gradients in fp32, dense: d_pos [P][768] and d_emb [V][768] (all of it is written: rows that no valid token names,
 *   and row 0, the padding row, are exact zeros).  No floating-point atomics: d_pos sums over the samples in a fixed order, and
 *   d_emb groups the rows by id with mmdeer_sort_pairs (stable) and sums every run in row order, so two calls give the same
 *   bits.  B * L <= 2^20 (the sort's limit; more is refused).  ids32 is the forward's.  scratch: 16-byte aligned,
 *   mmdeer_token_embed_bwd_scratch(B * L) bytes. */
typedef struct mmdeer_token_embed_args {
  const int64_t* ids;
  const float* mask;
  const float* emb; const float* pos; int32_t V, P;
  const float* src; int32_t ld_src;
  void* x; int32_t ld_x;
  int32_t* ids32;
  const void* dx; int32_t ld_dx;
  float* d_src; int32_t ld_dsrc;
  float* d_emb; float* d_pos;
  void* scratch; long long scratch_bytes;
  int32_t B, L, width, act_f32;
  void* stream;
} mmdeer_token_embed_args;
long long mmdeer_token_embed_bwd_scratch(long long rows);
int mmdeer_token_embed_fwd(const mmdeer_token_embed_args* a);
int mmdeer_token_embed_bwd(const mmdeer_token_embed_args* a);

/* Masked attention pool over tokens (encoders.py:733-746).  x act [B*L][ld_x >= 768] is ALREADY masked (x_t = 0 where m_t = 0),
 * z act [B*L][ld_z >= 384] = W1 x + b1 (from mmdeer_gemm), w2 fp32 [384], b2 fp32 [1]:
 *     s_t = w2 . tanh(z_t) + b2      p = softmax(s) over ALL L positions (max-subtracted; padded positions take part)
 *     S = sum_t p_t m_t              a_t = p_t m_t / (S + 1e-10)            attended = sum_t a_t x_t
 *   forward writes attended act [B][ld_att >= 768], weights fp32 [B][L] (= a) and, when probs is not NULL, probs fp32 [B][L]
 *   (= p, which the backward reads).  A fully masked sample gives a = 0 and attended = 0 exactly.
 *   backward reads dout act [B][ld_dout >= 768], x, z, weights, probs and writes dx act [B*L][ld_dx >= 768] = a_t dout (the
 *   direct term only; the score path's share dz W1 is the caller's GEMM, and the caller multiplies the sum by m),
 *   dz act [B*L][ld_dz >= 384], dw2 fp32 [384] and db2 fp32 [1] = an exact zero (b2 shifts every score of a sample equally).
 *   With da_t = dout . x_t and c = sum_u a_u da_u:  ds_t = p_t (m_t (da_t - c) - c 1e-10) / (S + 1e-10).
 *   scratch: fp32, 16-byte aligned, at least MMDEER_TOKEN_POOL_SCRATCH elements (dw2's per-workgroup partials, folded in a
 *   fixed order: deterministic). */
#define MMDEER_TOKEN_POOL_SCRATCH (1024 * 384)
typedef struct mmdeer_token_pool_args {
  const void* x; int32_t ld_x;
  const void* z; int32_t ld_z;
  const float* mask;
  const float* w2; const float* b2;
  void* attended; int32_t ld_att;
  float* weights; float* probs;
  const void* dout; int32_t ld_dout;
  void* dx; int32_t ld_dx;
  void* dz; int32_t ld_dz;
  float* dw2; float* db2; float* scratch;
  int32_t B, L, width, att_width, act_f32;
  void* stream;
} mmdeer_token_pool_args;
int mmdeer_token_pool_fwd(const mmdeer_token_pool_args* a);
int mmdeer_token_pool_bwd(const mmdeer_token_pool_args* a);

/* Per-sample token statistics (encoders.py:648-699, "linguistic features") without the reference's host loop.
 * ids int32 [B][L], mask fp32 [B][L] -> out fp32 [B][ld_out >= 16].  With n valid tokens, u distinct valid ids, c_max the
 * largest multiplicity and id_max the largest valid id: out[b] = { n / max_length, u / max(n, 1), n / (id_max + 1), c_max,
 * #{999 <= id <= 1030} / max(n, 1), #{100 <= id <= 999} / max(n, 1), 0 x 10 } (columns 10 .. 15 pad K to a multiple of 4
 * for the GEMM that follows).  n = 0: all zeros.  L <= 2048 (a sample's ids are held in LDS; more is refused).  Negative valid
 * ids are undefined input (the reference's bincount raises on them). */
typedef struct mmdeer_token_stats_args {
  const int32_t* ids;
  const float* mask;
  float* out; int32_t ld_out;
  int32_t B, L, max_length;
  void* stream;
} mmdeer_token_stats_args;
int mmdeer_token_stats(const mmdeer_token_stats_args* a);

/* ---- the evidence tail as an operator of its own (reference src/models/deer.py:55, 86-98): the last Linear(K -> 4 O) of an
 * evidence net, the NIG activations and the three uncertainties in ONE launch for G nets side by side, and its backward.
 * "act" = fp32 when act_f32 != 0, else bf16.  Net g reads columns [g K, (g + 1) K) of x; output column g O + o.
 *   x        act [B][ld_x]: the activations below the last layer (after ReLU / dropout)
 *   w        act [G][4 O][K]: row 4 o + c of net g is the reference's weight row 4 o + c (c = 0..3: mu, nu^, alpha^, beta^)
 *   b        fp32 [G][4 O]
 *   evid     fp32 [B][G O][4]: the raw evidence x W^T + b, written by the forward and read by the backward
 *   nig_out  fp32 [7][B][G O]: mu = e0, nu = softplus(e1) + 1e-6, alpha = softplus(e2) + 1, beta = softplus(e3) + 1e-6,
 *            aleatoric = beta / (alpha - 1), epistemic = beta / (nu (alpha - 1)), total = aleatoric + epistemic; alpha - 1 is
 *            formed from the rounded fp32 alpha, so it is 0 and the uncertainties inf where e2 < about -17, as in torch
 *   g_out    backward: the upstream gradients of the seven planes, fp32 [B][G O] each.  A NULL plane is an output the loss does not
 *            use: its terms are dropped, not multiplied by zero, so a loss on mu, nu, alpha, beta alone has finite gradients
 *            where alpha - 1 = 0.  Where a given uncertainty plane meets alpha - 1 = 0 the result is inf / nan (no clamping).
 *   devid    fp32 [B][G O][4], optional: d evidence
 *   dx       act [B][ld_dx], optional: (devid . W) * ((x > 0) * mask_scale); mask_scale <= 0: no mask factor.  Must not alias x.
 *   dw, db   fp32 [G][4 O][K], [G][4 O]: overwritten.  Per-part partials folded in index order: no float atomics, two runs give
 *            identical bits.
 *   scratch  fp32, at least mmdeer_evidence_tail_scratch(B, G, K, O) elements, 16-byte aligned (backward only)
 * Accepted: 1 <= G <= 8, 1 <= O <= 8, K a multiple of 8 in [8, 512], ld_x and ld_dx >= G K and multiples of 8 (bf16) / 4 (fp32),
 * x, w, b, evid, devid, dx, scratch 16-byte aligned, B >= 0.  B = 0 launches nothing; the backward then zero-fills dw and db.
 * Anything else writes nothing, returns -1 and names the argument in mmdeer_last_error(); all of it is checked on the host
 * before any HIP runtime call.  mmdeer_evidence_tail_scratch returns -1 for a refused shape. */
typedef struct mmdeer_evidence_tail_args {
  const void* x; int32_t ld_x;
  const void* w;
  const float* b;
  float* evid;
  float* nig_out;
  const float* g_out[7];
  float* devid;
  void* dx; int32_t ld_dx;
  float* dw; float* db;
  float* scratch;
  float mask_scale;
  int32_t B, G, K, O, act_f32;
  void* stream;
} mmdeer_evidence_tail_args;
long long mmdeer_evidence_tail_scratch(int B, int G, int K, int O);
int mmdeer_evidence_tail_fwd(const mmdeer_evidence_tail_args* a);
int mmdeer_evidence_tail_bwd(const mmdeer_evidence_tail_args* a);

/* ---- streaming evaluation statistics (reference src/utils/metrics.py:59-125) ---------------------------
 * pred / target / unc: [B][3] fp32 (unc may be NULL).  acc: device double[3][8], zeroed by the caller before the first
 * batch; every call adds {n, sum p, sum t, sum p^2, sum t^2, sum pt, sum |p-t|, sum (p-t)^2} per emotion dimension over
 * the rows without NaN -- CCC, Pearson, MAE and RMSE follow from these 24 numbers, so validation copies 192 bytes to the
 * host instead of (N, 3) arrays.  sample_err / sample_unc (optional, [B]): per-sample mean |error| / mean uncertainty for
 * the quantile-binned calibration error (metrics.py:214-279), as fp32 programs (three additions from 0, one division by 3;
 * a NaN in the row gives NaN).  sample_err may be asked for without unc, sample_unc may not (-1).  B = 0 returns 0 and
 * touches nothing; two launches on the same inputs add the same bits. */
int mmdeer_eval_accumulate(const float* pred, const float* target, const float* unc, double* acc, float* sample_err,
                           float* sample_unc, int B, void* stream);

/* Quantile-binned calibration error of the reference (src/utils/metrics.py:214-279) without copying per-sample arrays to
 * the host.  err / unc: the per-sample device arrays mmdeer_eval_accumulate wrote (concatenated over the batches), n samples;
 * a sample counts when neither value is NaN and unc is finite.
 *   mmdeer_eval_quantile_select: for the nq = n_bins + 1 quantiles q_r = r / (nq - 1) of the valid uncertainties, the two
 *     order statistics np.quantile interpolates between -- vals[r][0..1] = sorted[floor(q_r (nv - 1))], the one after it --
 *     their weight frac[r] and *nvalid = nv.  (The host forms the edges: 2 nq floats, as numpy's 'linear' method does.)
 *   mmdeer_eval_ece_bins: bins[i] = {count, sum (1 - unc), sum (1 - err)} over edges[i] <= unc < edges[i + 1]; edges is a
 *     DEVICE array of n_bins + 1 doubles, n_bins <= 16.  ECE = sum_i count_i / nv * |sum1_i - sum2_i| / count_i.
 *     The comparison is in double: an uncertainty equal to an interior edge belongs to the upper bin, one equal to
 *     edges[n_bins] or below edges[0] to none.  Refused (-1, nothing written): n <= 0, n_bins outside 1..16. */
int mmdeer_eval_quantile_select(const float* err, const float* unc, long long n, int nq, float* vals, double* frac,
                                long long* nvalid, void* stream);
int mmdeer_eval_ece_bins(const float* err, const float* unc, long long n, const double* edges, int n_bins, double* bins,
                         void* stream);

/* ---- evaluator statistics (reference src/training/evaluation.py:135-355, 492-530, 578-682; csrc/evalstats.hip) ----------
 * pred / target / unc: [N][D] fp32 device arrays, 1 <= D <= 3, 1 <= N < 2^31.  Every reduction below has a fixed partition
 * and a fixed-order fold and uses no floating-point atomics: two calls on the same inputs give bit-identical outputs.
 *
 * mmdeer_bootstrap_moments: R <= 4096 bootstrap replicates.  Draw i < N of replicate r reads row
 *     j = ((splitmix64(key(seed, r) + i) >> 32) * N) >> 32,   key(seed, r) = splitmix64(seed + r * 0xD1B54A32D192ED03)
 *   (mmdeer/synth.py: bootstrap_indices restates it in numpy).  One index per (r, i) serves all D dimensions: the reference
 *   draws per dimension, but each interval is a marginal statistic, so its distribution is the same.
 *   mom[R][D][6] (fp64) = {n, sum p, sum t, sum p^2, sum t^2, sum pt} over the drawn rows where neither value is NaN;
 *   flags[R][D]: bit 0 the drawn valid p are all equal (min == max: pearsonr's exact test), bit 1 the same for t, bit 2
 *   both and the two constants are equal.  scratch: mmdeer_bootstrap_scratch(N, R) bytes, 16-byte aligned (a repacked
 *   32-byte row per sample and the per-workgroup partial sums).
 * mmdeer_bootstrap_ci: metric 0 = CCC (evaluation.py:656-682: 0.0 below two valid pairs or for a zero denominator, NaN
 *   for a constant sample), 1 = Pearson (NaN for a constant sample or when a NaN row was drawn).  NaN replicates are
 *   dropped, the rest sorted; ci[D][2] (fp64) = np.percentile (linear) at the levels q_lo, q_hi in [0, 1]; nkept[D] = the
 *   number of replicates kept ({0.0, 0.0} when none is). */
long long mmdeer_bootstrap_scratch(long long N, int R);
int mmdeer_bootstrap_moments(const float* pred, const float* target, long long N, int D, int R, unsigned long long seed,
                             double* mom, int* flags, void* scratch, long long scratch_bytes, void* stream);
int mmdeer_bootstrap_ci(const double* mom, const int* flags, long long N, int D, int R, int metric, double q_lo, double q_hi,
                        double* ci, int* nkept, void* stream);

/* Stable ascending sort of n <= 2^20 fp32 keys (keys[i * stride]) by the total order (key, index): order[n] (int32) is
 * exactly np.argsort(kind='stable') -- -0.0 == +0.0, NaN last.  A larger n is refused.  scratch:
 * mmdeer_sort_pairs_scratch(n) bytes, 8-byte aligned; after the call it holds the sorted (key image, index) pairs that
 * mmdeer_average_ranks reads: ranks[n] (fp64, original positions) = the tie-averaged 1-based ranks of
 * scipy.stats.rankdata (NaN keys rank as one run of ties at the end).
 * mmdeer_rank_moments: out[3] = {sum a'^2, sum b'^2, sum a'b'} of two rank arrays centred by (n + 1) / 2 (Spearman). */
long long mmdeer_sort_pairs_scratch(long long n);
int mmdeer_sort_pairs(const float* keys, long long stride, long long n, int* order, void* scratch, long long scratch_bytes,
                      void* stream);
int mmdeer_average_ranks(const void* sorted, long long n, double* ranks, void* stream);
int mmdeer_rank_moments(const double* ranks_a, const double* ranks_b, long long n, double* out, void* stream);

/* Bin tables of CalibrationAnalyzer.compute_ece (evaluation.py:492-530) per dimension.  Confidence 1 - u / (max u + 1e-8)
 * and the threshold np.median(|p - t|) are formed in float32 as numpy forms them; edges: DEVICE array of n_bins + 1
 * doubles (np.linspace(0, 1, n_bins + 1)), n_bins <= 32.  bins[D][2][n_bins][3] (fp64) = {count, sum confidence,
 * sum (|p - t| <= threshold)} under rule 0 ([lo, hi), last bin closed: the reference's weights) and rule 1 ((lo, hi],
 * first bin closed: sklearn's calibration_curve).  stats[D][4] = {max u, threshold, 1 if an uncertainty is not finite or
 * a confidence lies outside [0, 1] (the reference then returns 0.0), 1 if the threshold is NaN}.
 * scratch: mmdeer_calibration_bins_scratch(D) bytes. */
long long mmdeer_calibration_bins_scratch(int D);
int mmdeer_calibration_bins(const float* pred, const float* target, const float* unc, long long N, int D, const double* edges,
                            int n_bins, double* stats, double* bins, void* scratch, void* stream);

/* The table UncertaintyAnalyzer (evaluation.py:358-482) is computed from, per dimension d of u = unc[:, d] and
 * e = |pred - target|[:, d] (the float32 subtraction, as numpy forms it); 2 <= N <= 2^20 (the sort's limit).
 * table[D][MMDEER_UNC_TABLE] (fp64, device):
 *    0 N | 1 sum u | 2 sum e | 3 sum (u - mean u)^2 | 4 sum (e - mean e)^2 | 5 sum (u - mean u)(e - mean e) | 6 mean u
 *    7 population variance of u | 8 min u | 9 max u | 10 min e | 11 max e   (NaN with a NaN in the column, as np.min / np.max)
 *   12 flags: 1 = a NaN in u, 2 = a NaN in e | 13-15 zero
 *   16 + k, k < n_cuts <= 16: the sum of e over the n_keep[k] least uncertain samples -- the first n_keep[k] positions of the
 *        stable ascending order of u (ties in index order, NaN last: mmdeer_sort_pairs' order); 0 for n_keep[k] = 0, NaN
 *        with a NaN error in the prefix.  n_keep: HOST array, ascending, each in [0, N]; the sparsification curve's
 *        int(frac * N) is the caller's arithmetic, not recomputed here.
 *   32 + k, k < n_q <= 8: np.percentile(u, 100 * levels[k]), method 'linear', in fp64; NaN with a NaN in u.  levels: HOST
 *        array, each in [0, 1].
 * Unused entries are zero.  All D columns are sorted by the same launches (the launch count of one mmdeer_sort_pairs plus
 * four); sums are fp64 with a partition that depends on N alone and a fixed-order fold: two calls give bit-identical tables.
 * scratch: mmdeer_uncertainty_table_scratch(N, D) bytes (0 for an N or D out of range), 8-byte aligned. */
#define MMDEER_UNC_TABLE 40
long long mmdeer_uncertainty_table_scratch(long long N, int D);
int mmdeer_uncertainty_table(const float* pred, const float* target, const float* unc, long long N, int D, const long long* n_keep,
                             int n_cuts, const double* levels, int n_q, double* table, void* scratch, long long scratch_bytes,
                             void* stream);

/* ---- Stack B: complete_project.CompleteDEERModel, eval forward -----------------------------------------
 * Every Linear(+ReLU) of the model runs on mmdeer_gemm; with a single key the reference's MultiHeadAttention
 * (complete_project.py:120-184) is output_proj(value_proj(value)) exactly, i.e. two more GEMMs.  The four single
 * operators below are the remaining row-wise pieces; mmdeer_stackb_forward (further down) strings everything together.  Activations ("act") are fp32 when act_f32 != 0, else bf16; parameters and
 * the listed outputs are fp32.  encoder_dim 256 / fusion_dim 512 (ModelConfig defaults, complete_project.py:33-56).
 *
 * Alignment, for every row operator from here to mmdeer_outer_bwd (Stack B eval and training, the fusion row operators):
 * they read and write 4 elements at a time, so every act pointer -- and with it every row, the leading dimensions being
 * multiples of 4 -- starts on 4 elements (16 bytes in fp32, 8 bytes in bf16), and so do the fp32 buffers ev, out32,
 * weights4, unc4 and weights8 (16 bytes).  x1 / dx1 of the outer products (any ld1), logits, g4, the [B][3] outputs and
 * the parameter vectors carry no such rule.  A misaligned pointer is refused like any other bad argument: on the host,
 * -1, nothing written, the reason in mmdeer_last_error().
 *
 * out = x + LayerNorm(y) row by row (ResidualBlock, complete_project.py:60-73); x == NULL: plain LayerNorm (the
 * Linear-ReLU-LayerNorm stems, :84-88, 315-333).  N is 256 or 512; eps 1e-5, biased variance. */
int mmdeer_stackb_residual_ln(const void* y, int ld_y, const void* x, int ld_x, const float* gamma, const float* beta,
                              void* out, int ld_out, int M, int N, int act_f32, void* stream);

/* Tail of UncertaintyAwareAttention.forward (complete_project.py:262-304), one call per batch:
 *   u_m     = sigmoid(est_w3 . h2[3 b + m] + est_b3)                  uncertainty_estimator.estimator.5 + Sigmoid
 *   hidden  = relu(pre[b] + sum_m u_m * wn_w1_unc[:, m])              the 3 uncertainty columns of weight_network.0
 *   weights = softmax(wn_w2 hidden + wn_b2)                           weight_network.3 + Softmax(dim=1)
 *   final_m = weights_m * self_out[b, m] + (1 - u_m) * cross_out[b, m]
 * audio / video land in columns 0..255 / 256..511 of out_av (the av_fusion input), text in columns 0..255 of out_text. */
typedef struct mmdeer_stackb_attn_args {
  const void* h2;            /* act [3B][64]: estimator hidden layer 2 of the interleaved (b, modality) rows */
  const void* pre;           /* act [B][256]: weight_network.0 over the 768 self-attention columns + bias, no ReLU */
  const void* self_out;      /* act [B][768] */
  const void* cross_out;     /* act [B][768] */
  const float* est_w3;       /* [64] */
  const float* est_b3;       /* [1] */
  const float* wn_w1_unc;    /* &weight_network.0.weight[0][768]; rows ld_w1_unc apart (771 in the reference layout) */
  const float* wn_w2;        /* [3][256] */
  const float* wn_b2;        /* [3] */
  void* out_av;              /* act, row stride ld_av >= 512 */
  void* out_text;            /* act, row stride ld_text >= 256 */
  float* weights;            /* [B][3]  'attention_weights' */
  float* uncertainties;      /* [B][3]  'modality_uncertainties' */
  int32_t ld_w1_unc, ld_av, ld_text, B, act_f32;
  void* stream;
} mmdeer_stackb_attn_args;
int mmdeer_stackb_attn_mix(const mmdeer_stackb_attn_args* a);

/* HierarchicalFusionModule's gated combination (complete_project.py:360-364):
 * out = sigmoid(gate_logits) * tri + (1 - sigmoid(gate_logits)) * av, [B][N] act matrices with their own row strides;
 * out32 (optional): a dense fp32 [B][N] copy for the caller ('fused_features'). */
int mmdeer_stackb_gate_mix(const void* gate_logits, int ld_g, const void* tri, int ld_t, const void* av, int ld_av, void* out,
                           int ld_out, float* out32, int B, int N, int act_f32, void* stream);

/* DEERPredictionHead constraints + uncertainties (complete_project.py:395-418) and UncertaintyCalibrationLayer
 * (:421-459).  ev: fp32 [B][ld_ev], the raw (mu, nu, alpha, beta) outputs of head d at columns 4 d .. 4 d + 3.
 * out: eight fp32 [B][3] planes -- mu, nu, alpha, beta, aleatoric, epistemic, total, calibrated.
 * temperature [3]; calibration_network: w1 [32], b1 [32], w2 [16][32], b2 [16], w3 [16], b3 [1]. */
int mmdeer_stackb_head(const float* ev, int ld_ev, const float* temperature, const float* w1, const float* b1, const float* w2,
                       const float* b2, const float* w3, const float* b3, float* out, int B, void* stream);

/* ---- Stack B training (forward with dropout + backward).  The Linear / LayerNorm layers run on mmdeer_gemm (forward,
 * dX with the ReLU / dropout mask in the epilogue, dW + bias gradient) and mmdeer_layernorm_fwd / _bwd, sequenced by
 * the host (mmdeer/stackb.py); these are the remaining row operators.  Nothing here sums over the batch. */
typedef struct mmdeer_stackb_attn_train_args {
  /* forward operands: as mmdeer_stackb_attn_args */
  const void* h2; const void* pre; const void* self_out; const void* cross_out;
  const float* est_w3; const float* est_b3; const float* wn_w1_unc; const float* wn_w2; const float* wn_b2;
  void* out_av; void* out_text;
  /* saved by the forward, read by the backward */
  void* r;                  /* act [B][256]: weight_network hidden after ReLU and dropout */
  float* weights4;          /* fp32 [B][4]: softmax weights (audio, video, text, 0) */
  float* unc4;              /* fp32 [B][4]: modality uncertainties (audio, video, text, 0) */
  void* unc8;               /* optional, written by the BACKWARD: act [B][8] = (unc4, 0, 0, 0, 0) -- the uncertainties as a k-contiguous
                               operand of the weight-gradient GEMM of weight_network.0's uncertainty columns */
  /* backward: gradients in (d_av: rows of stride ld_av, audio | video; d_text: stride ld_text) and out */
  const void* d_av; const void* d_text;
  void* d_self; void* d_cross;    /* act [B][768] */
  void* d_pre;                    /* act [B][256] */
  void* d_logits8;                /* act [B][8]: columns 0..2, the rest written as zeros (8 columns = one 16-byte bf16 row,
                                     the narrowest k-contiguous operand mmdeer_gemm's vector loads take) */
  void* d_z8;                     /* act [3B][8]: column 0 = gradient at the estimator's pre-sigmoid output, the rest zeros */
  void* d_h2;                     /* act [3B][64] */
  int32_t ld_w1_unc, ld_av, ld_text, B, act_f32;
  int32_t ld_dcross;              /* row stride of d_cross read as [3B][256] rows (0: dense, 256) -- lets it be the right half of a [3B][512] matrix */
  int32_t training, drop_site;    /* weight_network.2 dropout: keep mask = hash(seed, offset, drop_site, row, col) */
  float dropout_p;
  uint64_t seed, offset;
  const uint64_t* offset_dev;     /* optional device counter added to `offset` (NULL: offset alone) */
  void* stream;
} mmdeer_stackb_attn_train_args;
int mmdeer_stackb_attn_mix_train_fwd(const mmdeer_stackb_attn_train_args* a);
int mmdeer_stackb_attn_mix_bwd(const mmdeer_stackb_attn_train_args* a);
/* d of mmdeer_stackb_gate_mix: dg (gate logits), dtri (already masked by tri > 0: tri is a Linear + ReLU output), dav */
int mmdeer_stackb_gate_mix_bwd(const void* dout, int ld_do, const void* gate_logits, int ld_g, const void* tri, int ld_t, const void* av,
                               int ld_av, void* dg, int ld_dg, void* dtri, int ld_dt, void* dav, int ld_dav, int B, int N, int act_f32,
                               void* stream);
/* g4: fp32 [4][B][3] gradients wrt (mu, nu, alpha, beta); dev: act [B][ld_dev], ld_dev >= 24 and a multiple of 8 (whole
 * 8-column blocks: the k-contiguous operand of the weight-gradient GEMM), dev[b][8 d + k] = gradient wrt head d's raw
 * output k (k < 4), columns 8 d + 4 .. 8 d + 7 written as zeros */
int mmdeer_stackb_head_bwd(const float* ev, int ld_ev, const float* g4, void* dev, int ld_dev, int B, int act_f32, void* stream);
/* out = (x + y) * (mask > 0 ? scale : 0) on [M][N] activation views (y, mask optional): gradient joins, residual sums,
 * ReLU / dropout masks that no GEMM epilogue can carry */
int mmdeer_add_masked(void* out, int ld_out, const void* x, int ld_x, const void* y, int ld_y, const void* mask, int ld_mask,
                      float scale, int M, int N, int act_f32, void* stream);

/* ---- alternative fusion modules of src/models/fusion.py:421-554 (AttentionFusion, BilinearFusion, AdaptiveFusionGating):
 * their Linear layers run on mmdeer_gemm; these are the row operators (mmdeer/fusions.py is the call sequence).
 *
 * Softmax over S <= 8 stacked feature rows of one sample and their weighted sum.  P(b, s, :) = P + b ldp + s sp (elements, D
 * columns each).  Logits: P(b, s, :) . w_att + b_att[0] (AttentionFusion.forward, fusion.py:523: the Linear(D, 1) `attention`)
 * when w_att != NULL, else logits[b ld_logits + s] (AdaptiveFusionGating.forward, fusion.py:470-489: strategy_selector's output
 * before its Softmax).  Forward writes weights8 (fp32 [B][8], zeros beyond S) and out; backward reads weights8 and dout and
 * writes dP (same addressing as P; includes the path through w_att) and dlogits8 (act [B][8], zeros beyond S). */
typedef struct mmdeer_softmax_mix_args {
  const void* P; int64_t ldp, sp;
  int32_t S, D, B, act_f32;
  const float* w_att; const float* b_att;
  const float* logits; int32_t ld_logits;
  float* weights8;
  void* out; int32_t ld_out;
  const void* dout; int32_t ld_dout;
  void* dP; void* dlogits8;
  void* stream;
} mmdeer_softmax_mix_args;
int mmdeer_softmax_mix_fwd(const mmdeer_softmax_mix_args* a);
int mmdeer_softmax_mix_bwd(const mmdeer_softmax_mix_args* a);
/* z[b][i J + j] = x1[b][i] x2[b][j] (act [B][I J], dense): nn.Bilinear (fusion.py:536, 546) = mmdeer_gemm(z, weight read as
 * [out][I J]).  Backward: dx1[b][i] = sum_j dz[b][i J + j] x2[b][j], dx2[b][j] = sum_i dz[b][i J + j] x1[b][i]  (J <= 1024). */
int mmdeer_outer_fwd(const void* x1, int ld1, const void* x2, int ld2, void* z, int B, int I, int J, int act_f32, void* stream);
int mmdeer_outer_bwd(const void* dz, const void* x1, int ld1, const void* x2, int ld2, void* dx1, int ldd1, void* dx2, int ldd2, int B, int I,
                     int J, int act_f32, void* stream);

/* The whole eval forward as ONE call: 25 launches per batch (26 in bf16 mode), the three encoders / the layers that
 * share an input side by side in grouped GEMM launches.  `mmdeer_stackb_weights` is the device-side operand image the
 * host builds once per parameter update from the reference's state_dict (mmdeer/stackb.py does it): matrices ("W") in
 * the compute dtype (fp32 when compute_f32 != 0, else bf16), row-major [out][in] as nn.Linear stores them, stacked
 * where layers run in one launch; vectors fp32. */
typedef struct mmdeer_stackb_weights {
  int32_t audio_dim, video_dim, text_dim;   /* ModelConfig input widths, multiples of 4 */
  int32_t encoder_layers;                   /* ResidualBlocks per encoder */
  int32_t audio_ld;             /* row stride of enc_in_w[0]: audio_dim in fp32; bf16: a multiple of 64, columns >= audio_dim zero */
  const void* enc_in_w[3];      /* W [256][audio_ld | video_dim | text_dim]      <m>_encoder.input_projection.0.weight */
  const float* enc_in_vec;      /* [3][3][256]  per modality: .0.bias, .2.weight, .2.bias */
  const void* enc_res_w;        /* W [layers][3][256][256]                       encoder_layers.<l>.layers.0.weight per modality */
  const float* enc_res_vec;     /* [layers][3][3][256]  per layer and modality: layers.0.bias, layers.3.weight, layers.3.bias */
  const void* enc_out_w;        /* W [3][256][256]                               output_projection.weight */
  const float* enc_out_b;       /* [3][256] */
  const void* value_w;          /* W [512][256]  self_attention.value_proj over cross_attention.value_proj */
  const float* value_b;         /* [512] */
  const void* attn_out_w;       /* W [2][256][256]  self / cross output_proj */
  const float* attn_out_b;      /* [2][256] */
  const void* est_w1;  const float* est_b1;   /* W [128][256]   uncertainty_estimator.estimator.0 */
  const void* est_w2;  const float* est_b2;   /* W [64][128]    .3 */
  const float* est_w3; const float* est_b3;   /* [64], [1]      .5 */
  const void* wn_w1;   const float* wn_b1;    /* W [256][768]: the feature columns of weight_network.0.weight */
  const float* wn_w1_unc;                     /* [256][3]: its three uncertainty columns */
  const float* wn_w2;  const float* wn_b2;    /* [3][256], [3]  weight_network.3 */
  const void* av_w0;   const void* av_w4;     /* W [512][512] each  fusion_module.av_fusion.0 / .4 */
  const float* av_vec;                        /* [4][512]: .0.bias, .3.weight, .3.bias, .4.bias */
  const void* tri_w0;  const void* tri_w4;    /* W [512][768], [512][512]  trimodal_fusion.0 / .4 */
  const float* tri_vec;                       /* [4][512] */
  const void* gate_w;  const float* gate_b;   /* W [512][768], [512]  fusion_gate.0 */
  const void* head_w0; const float* head_b0;  /* W [768][512], [768]: evidence_network.0 of valence, arousal, dominance stacked */
  const void* head_w3; const float* head_b3;  /* W [3][128][256], [3][128] */
  const void* head_w6; const float* head_b6;  /* W [3][4][128],  [3][4] */
  const float* calibration[7];                /* temperature [3]; calibration_network w1 [32], b1 [32], w2 [16][32], b2 [16], w3 [16], b3 [1] */
} mmdeer_stackb_weights;

typedef struct mmdeer_stackb_forward_args {
  int32_t batch;
  int32_t compute_f32;            /* 1: exact-fp32 MFMA path; 0: bf16 operands, fp32 accumulation */
  const float* audio;             /* [B][audio_dim] fp32, dense */
  const float* video;             /* [B][video_dim] */
  const float* text;              /* [B][text_dim] */
  const mmdeer_stackb_weights* weights;
  void* workspace;                /* >= mmdeer_stackb_workspace_bytes(batch, compute_f32, audio_ld), 256-byte aligned */
  size_t workspace_bytes;
  float* planes;                  /* [8][B][3]: mu, nu, alpha, beta, aleatoric, epistemic, total, calibrated */
  float* attention_weights;       /* [B][3] */
  float* modality_uncertainties;  /* [B][3] */
  float* fused_features;          /* [B][512] or NULL */
  void* stream;
} mmdeer_stackb_forward_args;
size_t mmdeer_stackb_workspace_bytes(int batch, int compute_f32, int audio_ld);
int mmdeer_stackb_forward(const mmdeer_stackb_forward_args* a);

/* ---- row-local layer chains as an operator (csrc/chain.hip) -------------------------------------------------------------
 * A run of Linear (+ReLU +Dropout) (+LayerNorm | LayerNorm backward) layers that are local to a sample -- Stack B's residual
 * encoders, attention value / output projections, fusion stages and evidence heads (reference complete_project.py:60-118,
 * 120-184, 307-418) and their backward passes -- as ONE launch: a workgroup keeps 16 (or 32) samples' rows in LDS and walks the
 * layers, only the weights stream.  bf16 activations and weights, fp32 accumulation and vectors; results are those of the same
 * layers run one by one through mmdeer_gemm / mmdeer_layernorm_fwd / _bwd / mmdeer_add_masked, bit for bit.
 *
 * Weights are read from FRAGMENT-MAJOR images (mmdeer_repack, layout 1) of the [N][K] matrix a segment multiplies by (forward:
 * the nn.Linear weight; dX = dY W: its transpose [K_lin][N_lin], i.e. N = in_features, K = out_features).
 * A layer is one or more segments writing disjoint column ranges of one output panel; the last carries end_layer = 1.
 * Limits: <= MMDEER_CHAIN_MAX_SEGS segments (so as many layers at most), 16 bias / gamma / beta vectors of 4864 floats in total;
 * N % 64 == 0, K in {64, 128, 256, 384, 512, 768 (16-sample workgroups only)}; <= 4 column tiles per segment, of 128 columns, or
 * of 64 when N % 128 != 0 (then K must be 128 or 256); panel width <= 768 columns (16-sample workgroups) or 512 (32-sample).
 * Writes, for r < rows, of each layer end: stash[r][0, nout) -- or [0, stash_split) and stash2[r][0, nout - stash_split) --,
 * xln[r][0, nout), mean[r], rstd[r], lnb_dz[r][0, nout), and lnb_partial[w][0, 2 nout) for w < mmdeer_chain_workgroups(rows,
 * samples_per_workgroup); nothing else (rows = 0 writes nothing).  Rows of X, mask_y, lnb_y, lnb_mean, lnb_rstd past `rows`, columns
 * of X past K0 and columns of mask_y outside [mask_col0, mask_col0 + N) are never read into a stored output.  Refuses (-1, writing
 * nothing, message in mmdeer_last_error()) unless: 1 <= nseg <= MMDEER_CHAIN_MAX_SEGS and the last segment ends its layer;
 * rows >= 0; samples_per_workgroup 0, 16 or 32; the limits above; X and W 16-byte aligned, ldx % 8 == 0, ldx >= K0; kin_off and
 * nout_off non-negative multiples of 64 with kin_off + K <= the input panel's width and nout_off + N <= nout; 0 <= drop_shift < 32;
 * bias 16-byte aligned; mask_y 8-byte aligned, ld_mask and mask_col0 multiples of 4, mask_col0 >= 0, ld_mask >= mask_col0 + N;
 * stash 16-byte aligned, ld_stash % 8 == 0 and ld_stash >= the widest part it stores; stash_split only on a plain stash (no
 * LayerNorm), a multiple of 8 in (0, nout), with a 16-byte aligned stash2; a LayerNorm (forward or backward) of width 256 or 512 with
 * every pointer given and gamma / beta / xln / lnb_y / lnb_dz / lnb_partial 16-byte aligned; residual only where the layer keeps
 * its input's width; res_add / res_dup only on a segment that is its layer alone (N = nout = 256, nout_off 0), res_add only behind a
 * layer that wrote the bypass copy (res_dup). */
#define MMDEER_CHAIN_MAX_SEGS 12
typedef struct mmdeer_chain_seg {
  const void* W;            /* fragment-major image of the segment's [N][K] bf16 matrix */
  const float* bias;        /* [N] or NULL */
  int32_t N, K;
  int32_t kin_off, nout_off;/* first input / output panel column (multiples of 64) */
  int32_t relu;
  int32_t drop_site, drop_shift, dcol_off;   /* drop_site < 0: no dropout; the mask is hash(seed, offset, site, row, (dcol_off + n) >> shift) */
  const void* mask_y;       /* backward: out *= (Y[row][mask_col0 + n] > 0) * mask_scale (ReLU + dropout of the forward layer below), or NULL */
  int32_t ld_mask, mask_col0;
  float mask_scale;
  int32_t res_add, res_dup; /* backward of a residual block (256-wide layers): add columns 256 + n of the input panel; write the result
                               at columns 256 + n of the output panel as well */
  int32_t end_layer;
  /* end_layer only: */
  int32_t nout;             /* width of the finished panel */
  void* stash; int32_t ld_stash;             /* the finished (pre-LayerNorm) rows -> stash[row][ld_stash], or NULL */
  void* stash2; int32_t stash_split;         /* columns >= stash_split go to stash2[row][ld_stash] instead (0: none) */
  const float* gamma; const float* beta;     /* LayerNorm of the finished panel in place (nout 256 or 512), or NULL */
  void* xln; float* mean; float* rstd;       /* its outputs: rows [row][nout] (with the residual when set), statistics [row] */
  int32_t residual;         /* LayerNorm rows + the layer's input panel (x + LayerNorm(...)) */
  const float* lnb_gamma;   /* non-NULL instead of gamma: LayerNorm BACKWARD of the finished panel (= d out of the LayerNorm) */
  const void* lnb_y; const float* lnb_mean; const float* lnb_rstd;   /* the forward's pre-LayerNorm rows [row][nout], statistics */
  void* lnb_dz;             /* result rows [row][nout] */
  float* lnb_partial;       /* [mmdeer_chain_workgroups][2][nout] column sums of d * xhat and d (gamma / beta gradients; fold over workgroups) */
  float lnb_mask_scale;     /* > 0: the (y > 0) * scale mask of the Linear-ReLU-Dropout in front of the LayerNorm */
} mmdeer_chain_seg;
typedef struct mmdeer_chain_args {
  const void* X;            /* input rows [rows][ldx] bf16 */
  int32_t ldx, K0;          /* leading dimension, width (multiple of 64) */
  int32_t rows;             /* every row is a sample of its own */
  int32_t samples_per_workgroup;   /* 0: the library's choice (16 up to 4096 rows, 32 above); 16 or 32 */
  int32_t nseg;
  float dropout_p;          /* ONE probability for every dropout site of the chain */
  uint64_t seed, offset;
  const uint64_t* offset_dev;
  mmdeer_chain_seg seg[MMDEER_CHAIN_MAX_SEGS];
  void* debug;              /* diagnostic builds (-DMMDEER_STAMPS) only: uint64[512] buffer for in-kernel cycle stamps; NULL otherwise */
  void* stream;
} mmdeer_chain_args;
int mmdeer_chain(const mmdeer_chain_args* a);
int mmdeer_chain_workgroups(int rows, int samples_per_workgroup);

/* Derived bf16 images of bf16 matrices, any number of jobs in as few launches as possible (64 jobs each).  Job j restates the
 * matrix S = src[j] ([rows][cols], row stride ld_src, columns >= cols_valid read as zero) or, with transpose, S^T, in layout 0
 * (row-major at dst[j] with row stride ld_dst, starting at column dst_col) or layout 1 (fragment-major, what mmdeer_chain streams:
 * rows of the image % 16 == 0, columns % 64 == 0).  Writes the images, nothing else.  Every job is checked before the first launch,
 * so a refused call (-1) writes nothing; refused unless every job has a src, a 16-byte aligned dst, rows, cols > 0,
 * 0 <= cols_valid <= cols, ld_src >= cols_valid, image columns % 8 == 0, layout 0 or 1, and for layout 0 ld_dst and dst_col
 * multiples of 8 with dst_col + image columns <= ld_dst. */
typedef struct mmdeer_repack_job {
  const void* src; void* dst;
  int32_t ld_src, rows, cols, cols_valid, transpose, layout, ld_dst, dst_col;
} mmdeer_repack_job;
int mmdeer_repack(const mmdeer_repack_job* jobs, int n, void* stream);

/* ---- gradient exchange: the data-parallel step has ONE exchange, of the flat gradient buffer: one
 * all-reduce, or reduce-scatter + all-gather (every rank reduces 1/N of the buffer from all peers at once and then fetches
 * the other shards: all seven xGMI links of a GPU carry data at the same time, where a ring is bound by one link).  These wrap an RCCL communicator for hosts without torch.distributed; RCCL is bound at run time (dlopen), so
 * the library loads without it and these calls then fail with a message.  Rank 0 draws the id, the host distributes
 * its MMDEER_COMM_ID_BYTES bytes to the other ranks by whatever side channel it has (file, socket, MPI, a
 * torch.distributed broadcast), every rank calls mmdeer_comm_init with its HIP device current.  mmdeer_allreduce works
 * in place on `count` elements of fp32 (dtype_f32 != 0) or bf16, sum or average, enqueued on `stream` (capturable). */
#define MMDEER_COMM_ID_BYTES 128
typedef struct mmdeer_comm mmdeer_comm;
int mmdeer_comm_unique_id(void* id_out);
int mmdeer_comm_init(mmdeer_comm** comm, int rank, int world_size, const void* id);
int mmdeer_comm_destroy(mmdeer_comm* comm);
int mmdeer_allreduce(void* buf, long long count, int dtype_f32, int average, mmdeer_comm* comm, void* stream);
int mmdeer_comm_rank(const mmdeer_comm* comm);    /* -1 for NULL */
int mmdeer_comm_world(const mmdeer_comm* comm);
/* Reduce-scatter: `send` holds world * recv_count elements; rank r receives the sum (or mean) over ranks of elements
 * [r * recv_count, (r + 1) * recv_count) in `recv` (in place when recv == send + r * recv_count).  All-gather: every rank
 * contributes send_count elements, `recv` receives world * send_count (rank r's at r * send_count; in place when
 * send == recv + rank * send_count).  Enqueue-only on `stream`, capturable like mmdeer_allreduce. */
int mmdeer_reduce_scatter(const void* send, void* recv, long long recv_count, int dtype_f32, int average, mmdeer_comm* comm, void* stream);
int mmdeer_allgather(const void* send, void* recv, long long send_count, int dtype_f32, mmdeer_comm* comm, void* stream);

/* sizeof() of an argument struct of this header by its name without the mmdeer_ prefix ("gemm_args", "chain_args", "chain_seg",
 * "repack_job", "forward_args", "backward_args", "adamw_args", "adamw_flat_args", "stackb_attn_train_args", "stackb_attn_args",
 * "stackb_forward_args", "stackb_weights", "softmax_mix_args", "lstm_seq_args", "temporal_pool_args", "evidence_tail_args",
 * "token_embed_args", "token_pool_args", "token_stats_args"; of mmdeer_video.h: "conv3_time_args", "bn_time_args"); -1 for an unknown name.  A binding in another language checks its
 * own layout against it at load time (mmdeer/_lib.py does). */
long long mmdeer_sizeof(const char* struct_name);

/* fp32 <-> bf16 conversion of a contiguous device buffer (n % 4 == 0) */
int mmdeer_convert(const void* src, int src_f32, void* dst, int dst_f32, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMDEER_H_ */
