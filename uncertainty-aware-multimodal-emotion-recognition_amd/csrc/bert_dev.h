// The BERT trunk's shared pieces: what bert.hip (forward) and bert_bwd.hip (backward) both state -- the attention tiles and their
// fragments, the row layout of the one-wave-per-row LayerNorm, the GELU constant and the host checks.
// Rows are batch-major: row b * L + t.
//
// Attention in bf16 runs on mfma_f32_32x32x16_bf16 with two waves per workgroup, a wave owning 32 rows of the workgroup's 64 (queries
// in the forward and dq kernels, keys in dkdv).  A lane keeps its own row as the B fragments of the four k-steps in registers
// (load_row_frags); the other side comes through LDS in row-major tiles with 144-byte rows (stage_rows: the 16-byte fragment reads
// of 16 lanes then fall into 16 distinct bank groups).  The product is therefore TRANSPOSED -- S^T = K Q^T in the forward and dq,
// S = Q K^T in dkdv -- and a lane holds 16 scores of ONE row of its own: the two lane halves hold the two halves of the block's 32
// rows of the other side, register i of lane half h being row (i & 3) + 8 (i >> 2) + 4 h of the block.  Per-row softmax state (m, l,
// lse, delta) is so a per-lane scalar, and the accumulator tile, converted to bf16, is the B operand of the product that sums over
// those rows: registers 8 s .. 8 s + 7 are the fragment of k-step s, whose element j is row 16 s + 8 (j >> 2) + 4 h + (j & 3).  The A
// operand of that product is read in the same order (frag_t: two 8-byte reads) from a tile staged transposed, [d][row]
// (stage_transposed), because that product sums over rows where the tile in memory runs over d.  Rows past L are zero-filled in
// LDS; which keys are valid travels as one byte per key of the tile (the key-validity helpers), and a block of 32 keys without a
// valid one is skipped by a ballot.
// Attention in fp32 is parity, not speed: one thread per owned row, the other side in pairs of LDS tiles of 32 rows (stage_rows_f32) that
// every lane reads at the same address, a broadcast.
//
// Row LayerNorm (embed, add_ln and add_ln's backward): one wave per row of N <= 1024 columns.  Lane l owns the 4-element chunks
// l, l + 64, l + 128, l + 192 that lie inside the row (ln_chunk), keeps them in registers (bert_ln_load) and makes two passes over
// them (mean, then the centred sum of squares), both summed over the wave by DPP in a fixed order.
//
// Kept apart on purpose:
//   the online-softmax updates   the forward sums l from the probabilities ROUNDED to bf16 (its stored row is then a convex
//                                combination of V rows); the dq kernel's pass 0 sums the unrounded exponentials and carries the
//                                delta accumulator along.  Different arithmetic, not one update written twice.
//   ln_rows.h                    its rows are 256 or 512 bf16 columns on 32 lanes with eps 1e-5 baked in, and the layer chains must
//                                keep storing its bits.
//   the row statistics           bert.hip's bert_ln_row and bert_bwd.hip's add + LN backward each write the two passes out.  As one
//                                function they compile alike, and today they do not: the compiler contracts the forward's
//                                v - mean and its squares into fused multiply-adds and not the backward's, so the backward's mean
//                                and rstd differ from the forward's in the last bit, and sharing moves the bits the backward stores.
//   token_pool.hip, attention.hip  other pools over a sequence with tiles of their own; they are not the trunk's.
//   the GELU loops               the two chunk loops are four lines each; a loop taking a functor would be longer than both, so only
//                                the erf constant is shared.
#pragma once
#include <math.h>

#include "../../include/mmdeer_bert.h"
#include "elem.h"

namespace mmdeer {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BERT_HD = MMDEER_BERT_HEAD_DIM;   // 64
constexpr int AT_OWN = 64;      // rows of the tile a workgroup owns (queries in the forward and dq, keys in dkdv)
constexpr int AT_K = 128;       // keys per LDS tile of the bf16 forward and dq kernels
constexpr int AT_Q = 64;        // queries per LDS tile of the bf16 dkdv kernel
constexpr int ROW_LD = 72;      // bf16 elements per row of a row-major tile: 64 + 8 of padding
constexpr int KT_LD = 132;      // bf16 elements per row of a transposed tile of AT_K rows: 128 + 4 of padding
constexpr int QT_LD = 68;       // bf16 elements per row of a transposed tile of AT_Q rows: 64 + 4 of padding
constexpr int AT_F = 32;        // rows per LDS tile of the fp32 kernels

// blockIdx.x = (b * heads + head) * ntile + tile
struct AttnBlock {
  int b, head, tile;
};
__device__ __forceinline__ AttnBlock attn_block(int heads, int ntile) {
  const unsigned x = blockIdx.x;
  return AttnBlock{(int)(x / (ntile * heads)), (int)((x / ntile) % heads), (int)(x % ntile)};
}

// ------------------------------------------------------------------------------------------------ bf16 tiles (128 threads)
// row-major tile: 16-byte chunk c of row `row` of `rows` rows, zero past L.  src points at the head's 64 columns of token 0.
__device__ __forceinline__ void stage_rows(bf16_t* dst, const bf16_t* src, int ld, int t0, int rows, int L, int tid) {
  for (int i = tid; i < rows * 8; i += 128) {
    const int row = i >> 3, c = i & 7;
    u32x4 val{0u, 0u, 0u, 0u};
    if (t0 + row < L) val = *reinterpret_cast<const u32x4*>(src + (long long)(t0 + row) * ld + 8 * c);
    *reinterpret_cast<u32x4*>(dst + row * ROW_LD + 8 * c) = val;
  }
}
// transposed tile [d][row], row stride ld_t: chunk c of the rows 2 rp and 2 rp + 1, one dword per d
__device__ __forceinline__ void stage_transposed(bf16_t* dst, int ld_t, const bf16_t* src, int ld, int t0, int rows, int L, int tid) {
  for (int i = tid; i < (rows / 2) * 8; i += 128) {
    const int row = 2 * (i >> 3), c = i & 7;
    u32x4 va{0u, 0u, 0u, 0u}, vc{0u, 0u, 0u, 0u};
    if (t0 + row < L) va = *reinterpret_cast<const u32x4*>(src + (long long)(t0 + row) * ld + 8 * c);
    if (t0 + row + 1 < L) vc = *reinterpret_cast<const u32x4*>(src + (long long)(t0 + row + 1) * ld + 8 * c);
    const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wc[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      *reinterpret_cast<unsigned*>(dst + (8 * c + 2 * e) * ld_t + row) = (wa[e] & 0xFFFFu) | (wc[e] << 16);
      *reinterpret_cast<unsigned*>(dst + (8 * c + 2 * e + 1) * ld_t + row) = (wa[e] >> 16) | (wc[e] & 0xFFFF0000u);
    }
  }
}
// the A fragment of k-step s2 from a transposed tile, in the accumulator's row order: rows 16 s2 + 4 h + {0..3} and + 8
__device__ __forceinline__ bf16x8 frag_t(const bf16_t* p) {
  const u32x2 lo = *reinterpret_cast<const u32x2*>(p), hi = *reinterpret_cast<const u32x2*>(p + 8);
  return __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
}
// this lane's row of 64 bf16 as the B fragments of the four k-steps; zeros for a row past L, whose pointer is not dereferenced
__device__ __forceinline__ void load_row_frags(bf16x8 (&f)[4], const bf16_t* row, bool live, int h) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 raw{0u, 0u, 0u, 0u};
    if (live) raw = *reinterpret_cast<const u32x4*>(row + 16 * ks + 8 * h);
    f[ks] = __builtin_bit_cast(bf16x8, raw);
  }
}
// the lane's accumulator tile (register 4 g + e is column 32 t + 8 g + 4 h + e of its row) times `scale` into its row
__device__ __forceinline__ void store_tile(bf16_t* out, long long off, const f32x16 (&o)[2], int h, float scale) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st4<false>(out, off + 32 * t + 8 * g + 4 * h,
                 f32x4{o[t][4 * g] * scale, o[t][4 * g + 1] * scale, o[t][4 * g + 2] * scale, o[t][4 * g + 3] * scale});
}

// Key validity of a tile of AT_K keys, one byte per key.  mask points at the sample's token 0.
__device__ __forceinline__ void stage_valid(unsigned char* vb, const float* mask, int k0, int L, int tid) {
  if (tid < AT_K) vb[tid] = (k0 + tid < L && mask[k0 + tid] != 0.f) ? 1 : 0;
}
// the bytes of this lane's 16 keys of block kb: register i is key 32 kb + (i & 3) + 8 (i >> 2) + 4 h of the tile
__device__ __forceinline__ void load_valid(unsigned (&vw)[4], const unsigned char* vb, int kb, int h) {
#pragma unroll
  for (int g = 0; g < 4; ++g) vw[g] = *reinterpret_cast<const unsigned*>(vb + 32 * kb + 8 * g + 4 * h);
}
// no valid key in the block (wave-uniform)
__device__ __forceinline__ bool none_valid(const unsigned (&vw)[4]) {
  return __builtin_amdgcn_ballot_w64((vw[0] | vw[1] | vw[2] | vw[3]) != 0u) == 0ull;
}
__device__ __forceinline__ bool key_valid(const unsigned (&vw)[4], int i) { return ((vw[i >> 2] >> (8 * (i & 3))) & 0xFFu) != 0u; }

// ------------------------------------------------------------------------------------------------ fp32 tiles (64 threads)
// Two tiles of AT_F rows of 64 floats from token t0 on, zero past L; each src points at the head's 64 columns of token 0.  Every fp32
// kernel stages a pair (K and V, or Q and dO), and one loop over both keeps two loads in flight per step: staged one array at a
// time the fp32 forward took 5 % longer and the fp32 backward 7 %.
__device__ __forceinline__ void stage_rows_f32(float* dst0, const float* src0, int ld0, float* dst1, const float* src1, int ld1, int t0, int L,
                                               int tid) {
  for (int i = tid; i < AT_F * 16; i += 64) {
    const int row = i >> 4, c = i & 15;
    f32x4 v0{0.f, 0.f, 0.f, 0.f}, v1{0.f, 0.f, 0.f, 0.f};
    if (t0 + row < L) {
      v0 = *reinterpret_cast<const f32x4*>(src0 + (long long)(t0 + row) * ld0 + 4 * c);
      v1 = *reinterpret_cast<const f32x4*>(src1 + (long long)(t0 + row) * ld1 + 4 * c);
    }
    *reinterpret_cast<f32x4*>(dst0 + row * BERT_HD + 4 * c) = v0;
    *reinterpret_cast<f32x4*>(dst1 + row * BERT_HD + 4 * c) = v1;
  }
}

// ------------------------------------------------------------------------------------------------ row LayerNorm
// chunk j of this lane, present while it is below N / 4; absent chunks hold zeros
__device__ __forceinline__ int ln_chunk(int lane, int j) { return lane + 64 * j; }

// v = this lane's chunks of row y (+ row x, where x is given); oy, ox: the rows' element offsets
template <bool F32>
__device__ __forceinline__ void bert_ln_load(f32x4 (&v)[4], const void* y, long long oy, const void* x, long long ox, int lane, int nq) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = ln_chunk(lane, j);
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < nq) {
      v[j] = ld4<F32>(y, oy + 4 * c);
      if (x) v[j] += ld4<F32>(x, ox + 4 * c);
    }
  }
}

// ------------------------------------------------------------------------------------------------ GELU
constexpr float GELU_RSQRT2 = 0.70710678118654752440f;      // erf's argument is x / sqrt(2)

// ------------------------------------------------------------------------------------------------ host checks
constexpr long long TWO31 = 1ll << 31;
inline bool finite_nonneg(float e) { return e >= 0.f && e <= 3.0e38f; }     // false for a NaN
inline bool hidden_ok(int H) { return H >= BERT_HD && H % BERT_HD == 0 && H <= MMDEER_BERT_MAX_HIDDEN; }
inline bool ln_n_ok(int N) { return N >= 4 && N % 4 == 0 && N <= MMDEER_BERT_MAX_HIDDEN; }
inline bool ld_ok(int ld, int n, int k) { return ld >= n && ld % k == 0; }                 // a leading dimension >= n, a multiple of k
inline bool under_2_31(long long rows, int ld) { return rows * ld < TWO31; }              // an operand of `rows` rows
// 0 for a shape the attention calls take, else the number of the check that refuses it
inline int attn_shape_fault(int B, int L, int H) {
  if (!hidden_ok(H)) return 1;
  if (!(B >= 0 && L >= 0 && (L >= 1 || B == 0))) return 2;
  return L <= MMDEER_BERT_MAX_TOKENS ? 0 : 3;
}
// the same as the three checks of call `op`
inline int attn_shape_check(const char* op, int B, int L, int H) {
  const int fault = attn_shape_fault(B, L, H);
  MMDEER_CHECK(fault != 1, "%s: unsupported H = %d (a multiple of 64, 64 .. %d)", op, H, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(fault != 2, "%s: bad shape (B %d, L %d: L >= 1 with B > 0)", op, B, L);
  MMDEER_CHECK(fault != 3, "%s: L = %d is above %d tokens", op, L, MMDEER_BERT_MAX_TOKENS);
  return 0;
}
// workgroups of the row kernels (4 waves, a wave per row) and of the elementwise kernels (256 threads, a thread per 4-element chunk)
inline unsigned row_grid(long long rows) { return (unsigned)((rows + 3) / 4 < 65536 ? (rows + 3) / 4 : 65536); }
inline unsigned chunk_grid(long long chunks) { return (unsigned)((chunks + 255) / 256 < 16384 ? (chunks + 255) / 256 : 16384); }

}  // namespace
}  // namespace mmdeer
