// Device code of the grouped MFMA GEMM (included by gemm_nt.hip / gemm_nx.hip / gemm_tt.hip).
// One kernel instantiation per (compute type, tile, transposition, A source mode, B source mode): the K loop is
// straight-line code, so hipcc's s_waitcnt insertion keeps the global loads of the next K-tile in flight across
// the MFMAs of the current one.  (With the source modes as runtime switches -- inside or around the loop -- the
// control-flow joins made it wait for every load before the LDS reads: ~3700 cycles per K-tile.)
#pragma once
#include "gemm_tile.h"
#include "stamps.h"

namespace mmdeer {
namespace {

constexpr int LDS_ROW = 144;  // bytes: 128 B of K + 16 B pad

// u32x4 / u32x2 / f32x4 are native clang vectors (not HIP's uint4/float4 union structs): they stay SSA values, so the
// register tiles below are never materialised in scratch or promoted to LDS.

__device__ __forceinline__ u32x4 zero4() { return u32x4{0u, 0u, 0u, 0u}; }

// Load one 16-byte compute chunk (EPC elements of CT) from a source of element type ST.
// `valid` = number of in-range elements (0, 4 or 8; callers guarantee multiples of 4).  An out-of-range piece
// reads `safe` (an in-bounds, 16-byte-aligned address of the same operand) instead: every load is unconditional
// and NOTHING is computed on the loaded registers here, so the compiler can leave all loads of a K-tile in
// flight across the MFMAs of the previous tile and wait only at the LDS store.  (A load under a per-lane branch,
// or a select/AND on its result, made hipcc wait for each load right where it was issued: ~3500 cycles/K-step.)
// Garbage read through `safe` is harmless for rows beyond M / N (those outputs are never stored); the K tail is
// zeroed by tile_lstore.  Only the fp32 -> bf16 source path converts at load time.
template <typename CT, typename ST, bool VEC16>
__device__ __forceinline__ u32x4 load_chunk(const ST* p, const ST* safe, int valid) {
  const bool ok0 = valid >= 4, ok1 = valid >= 8;
  if constexpr (sizeof(CT) == 4) {   // fp32 compute, fp32 source: one 16-byte load
    return *reinterpret_cast<const u32x4*>(ok0 ? p : safe);
  } else if constexpr (sizeof(ST) == 4) {   // bf16 compute, fp32 source: two 16-byte loads, RNE convert
    const f32x4 a = *reinterpret_cast<const f32x4*>(ok0 ? p : safe);
    const f32x4 b = *reinterpret_cast<const f32x4*>(ok1 ? p + 4 : safe);
    return u32x4{pack_bf2(a.x, a.y), pack_bf2(a.z, a.w), pack_bf2(b.x, b.y), pack_bf2(b.z, b.w)};
  } else if constexpr (VEC16) {   // bf16 source, 16-byte aligned rows, extent % 8 == 0: valid is 0 or 8
    return *reinterpret_cast<const u32x4*>(ok1 ? p : safe);
  } else {   // bf16 source with 8-byte aligned rows (K = 84): two 8-byte loads
    const u32x2 a = *reinterpret_cast<const u32x2*>(ok0 ? p : safe);
    const u32x2 b = *reinterpret_cast<const u32x2*>(ok1 ? p + 4 : safe);
    return u32x4{a.x, a.y, b.x, b.y};
  }
}

// Register tile of one operand: four named 16-byte registers (named, not an indexed array: a loop-indexed
// array is only split into registers after unrolling, and by then store sinking has made its indices dynamic).
struct RTile { u32x4 r0, r1, r2, r3; };

__device__ __forceinline__ unsigned word_of(const u32x4& v, int i) {
  return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w));
}
__device__ __forceinline__ u32x4 and4(const u32x4& v, unsigned m) { return u32x4{v.x & m, v.y & m, v.z & m, v.w & m}; }

// ---- global -> registers for one operand tile of ROWS rows x (128 B of K); straight-line, no branches
template <typename CT, typename ST, int ROWS, bool TRANS, bool VEC16>
__device__ __forceinline__ RTile tile_gload(const ST* base, const ST* safe, long long ld, int rows_valid, int k0, int K, int tid) {
  constexpr int EPC = Elem<CT>::EPC, KT = Elem<CT>::KT;
  RTile t;
  t.r0 = t.r1 = t.r2 = t.r3 = zero4();
  if constexpr (!TRANS) {
    // operand stored [row][k]: 8 lanes cover one 128-byte row segment (full cache line per row)
    const int kc = tid & 7, ke = k0 + kc * EPC, rem = K - ke;
    const int kvalid = rem >= EPC ? EPC : (rem > 0 ? rem : 0);
    const int row = tid >> 3;
    const ST* p = base + (long long)row * ld + ke;
    t.r0 = load_chunk<CT, ST, VEC16>(p, safe, row < rows_valid ? kvalid : 0);
    if constexpr (ROWS >= 64) t.r1 = load_chunk<CT, ST, VEC16>(p + 32 * ld, safe, row + 32 < rows_valid ? kvalid : 0);
    if constexpr (ROWS >= 128) {
      t.r2 = load_chunk<CT, ST, VEC16>(p + 64 * ld, safe, row + 64 < rows_valid ? kvalid : 0);
      t.r3 = load_chunk<CT, ST, VEC16>(p + 96 * ld, safe, row + 96 < rows_valid ? kvalid : 0);
    }
  } else {
    // operand stored [k][row]: each thread takes 4 consecutive k x EPC consecutive rows
    // (threads beyond UNITS still issue clamped loads: their registers are never stored to LDS)
    constexpr int QN = KT / 4, UNITS = QN * (ROWS / EPC);
    const int q = tid % QN, c0 = (tid / QN) * EPC;
    const int rem = (tid < UNITS) ? rows_valid - c0 : 0;
    const int cvalid = rem >= EPC ? EPC : (rem > 0 ? rem : 0);
    const int k = k0 + 4 * q;
    const ST* p = base + (long long)k * ld + c0;
    t.r0 = load_chunk<CT, ST, VEC16>(p, safe, (k < K) ? cvalid : 0);
    t.r1 = load_chunk<CT, ST, VEC16>(p + ld, safe, (k + 1 < K) ? cvalid : 0);
    t.r2 = load_chunk<CT, ST, VEC16>(p + 2 * ld, safe, (k + 2 < K) ? cvalid : 0);
    t.r3 = load_chunk<CT, ST, VEC16>(p + 3 * ld, safe, (k + 3 < K) ? cvalid : 0);
  }
  return t;
}

// Row origins of a gathered A operand (conv2d.hip): row (tid >> 3) + 32 j of this thread's tile starts o<j> elements behind the
// tile's origin instead of (row) * ld.  The origins of rows beyond rows_valid are never used: those rows read `safe`.
struct RowGather { long long o0, o1, o2, o3; };

// tile_gload of a row-major operand whose rows are gathered
template <typename CT, typename ST, int ROWS, bool VEC16>
__device__ __forceinline__ RTile tile_gload_rows(const ST* base, const ST* safe, const RowGather& rg, int rows_valid, int k0, int K, int tid) {
  constexpr int EPC = Elem<CT>::EPC;
  RTile t;
  t.r0 = t.r1 = t.r2 = t.r3 = zero4();
  const int kc = tid & 7, ke = k0 + kc * EPC, rem = K - ke;
  const int kvalid = rem >= EPC ? EPC : (rem > 0 ? rem : 0);
  const int row = tid >> 3;
  const ST* p = base + ke;
  t.r0 = load_chunk<CT, ST, VEC16>(p + rg.o0, safe, row < rows_valid ? kvalid : 0);
  if constexpr (ROWS >= 64) t.r1 = load_chunk<CT, ST, VEC16>(p + rg.o1, safe, row + 32 < rows_valid ? kvalid : 0);
  if constexpr (ROWS >= 128) {
    t.r2 = load_chunk<CT, ST, VEC16>(p + rg.o2, safe, row + 64 < rows_valid ? kvalid : 0);
    t.r3 = load_chunk<CT, ST, VEC16>(p + rg.o3, safe, row + 96 < rows_valid ? kvalid : 0);
  }
  return t;
}

// Zero the part of a register tile that lies beyond K (only called for a partial last K-tile).
template <typename CT, bool TRANS>
__device__ __forceinline__ RTile tile_ktail_mask(RTile t, int k0, int K, int tid) {
  constexpr int EPC = Elem<CT>::EPC, KT = Elem<CT>::KT;
  if constexpr (!TRANS) {
    const int rem = K - (k0 + (tid & 7) * EPC);   // in-range elements of this lane's chunk (same for r0..r3)
    const unsigned mlo = rem >= EPC / 2 ? 0xFFFFFFFFu : 0u, mhi = rem >= EPC ? 0xFFFFFFFFu : 0u;
    // fp32: the chunk is 4 elements, valid is 0 or 4 -> mlo == mhi would need rem >= 4; EPC/2 = 2 < 4 is still exact
    // because rem is a multiple of 4.  bf16: low 8 bytes = elements 0-3, high 8 bytes = elements 4-7.
    auto m = [&](const u32x4& v) { return u32x4{v.x & mlo, v.y & mlo, v.z & mhi, v.w & mhi}; };
    t.r0 = m(t.r0); t.r1 = m(t.r1); t.r2 = m(t.r2); t.r3 = m(t.r3);
  } else {
    const int k = k0 + 4 * (tid % (KT / 4));
    t.r0 = and4(t.r0, k < K ? 0xFFFFFFFFu : 0u);
    t.r1 = and4(t.r1, k + 1 < K ? 0xFFFFFFFFu : 0u);
    t.r2 = and4(t.r2, k + 2 < K ? 0xFFFFFFFFu : 0u);
    t.r3 = and4(t.r3, k + 3 < K ? 0xFFFFFFFFu : 0u);
  }
  return t;
}

// ---- registers -> LDS tile ([row][k], LDS_ROW bytes per row)
template <typename CT, int ROWS, bool TRANS>
__device__ __forceinline__ void tile_lstore(unsigned char* t, const RTile& v, int tid) {
  constexpr int EPC = Elem<CT>::EPC, KT = Elem<CT>::KT;
  if constexpr (!TRANS) {
    unsigned char* d = t + (tid >> 3) * LDS_ROW + (tid & 7) * 16;
    *reinterpret_cast<u32x4*>(d) = v.r0;
    if constexpr (ROWS >= 64) *reinterpret_cast<u32x4*>(d + 32 * LDS_ROW) = v.r1;
    if constexpr (ROWS >= 128) {
      *reinterpret_cast<u32x4*>(d + 64 * LDS_ROW) = v.r2;
      *reinterpret_cast<u32x4*>(d + 96 * LDS_ROW) = v.r3;
    }
  } else {
    constexpr int QN = KT / 4, UNITS = QN * (ROWS / EPC);
    if (tid < UNITS) {
      const int q = tid % QN, c0 = (tid / QN) * EPC;
      if constexpr (sizeof(CT) == 4) {
        // 4x4 fp32 transpose is pure register renaming: row e of the LDS tile gets element e of the 4 k-rows
        unsigned char* d = t + c0 * LDS_ROW + q * 16;
        *reinterpret_cast<u32x4*>(d) = u32x4{v.r0.x, v.r1.x, v.r2.x, v.r3.x};
        *reinterpret_cast<u32x4*>(d + LDS_ROW) = u32x4{v.r0.y, v.r1.y, v.r2.y, v.r3.y};
        *reinterpret_cast<u32x4*>(d + 2 * LDS_ROW) = u32x4{v.r0.z, v.r1.z, v.r2.z, v.r3.z};
        *reinterpret_cast<u32x4*>(d + 3 * LDS_ROW) = u32x4{v.r0.w, v.r1.w, v.r2.w, v.r3.w};
      } else {
        // 4x8 bf16 transpose: LDS row (c0+e) receives the 4 k-values of column e, packed in 8 bytes
        unsigned char* d = t + c0 * LDS_ROW + q * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int w = e >> 1, sh = (e & 1) * 16;
          unsigned h0 = (word_of(v.r0, w) >> sh) & 0xFFFFu, h1 = (word_of(v.r1, w) >> sh) & 0xFFFFu;
          unsigned h2 = (word_of(v.r2, w) >> sh) & 0xFFFFu, h3 = (word_of(v.r3, w) >> sh) & 0xFFFFu;
          *reinterpret_cast<u32x2*>(d + e * LDS_ROW) = u32x2{h0 | (h1 << 16), h2 | (h3 << 16)};
        }
      }
    }
  }
}

template <typename CT>
__device__ __forceinline__ f32x4 mma_chunk(const u32x4& a, const u32x4& b, f32x4 acc) {
  if constexpr (sizeof(CT) == 2) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else {
    // lane (i = l&15, g = l>>4) holds k = 16s + 4g + t in element t: A and B use the same permutation of k
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    return acc;
  }
}

template <typename CT>
__device__ __forceinline__ float chunk_sum(const u32x4& a) {
  if constexpr (sizeof(CT) == 4) {
    return (__uint_as_float(a.x) + __uint_as_float(a.y)) + (__uint_as_float(a.z) + __uint_as_float(a.w));
  } else {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned w = word_of(a, i);
      s += __uint_as_float(w << 16) + __uint_as_float(w & 0xFFFF0000u);
    }
    return s;
  }
}

// stamps.h: wave 0 of workgroup 0, 6 stamps per K-tile for the first 16 tiles
#define STAMP(slot) \
  MMDEER_STAMP(ka.stamps, (kt - ka.kt0) * 8 + (slot), blockIdx.x == 0 && threadIdx.x == 0 && (kt - ka.kt0) < 16)

// source element type / vector width of a compile-time loader mode
template <typename CT, int MODE> struct SrcOf { typedef bf16_t type; static constexpr bool V16 = (MODE == SRC_BF16_V16); };
template <typename CT> struct SrcOf<CT, SRC_F32> { typedef float type; static constexpr bool V16 = true; };

// Fast operand loader for the interior K-tiles of a "regular" tile: per-thread source pointers are computed and
// clamped ONCE (an out-of-range row points at the operand's first row), and every K-tile only issues its loads and
// advances the pointers by a constant.  A clamped pointer advances too: it stays inside row / column 0 of the
// operand for as long as whole K-tiles remain, which is exactly the range this loader is used for.
template <typename CT, int ROWS, bool TRANS, int MODE>
struct FastLoader {
  typedef typename SrcOf<CT, MODE>::type ST;
  static constexpr bool V16 = SrcOf<CT, MODE>::V16;
  static constexpr int EPC = Elem<CT>::EPC, KT = Elem<CT>::KT;
  const ST *p0, *p1, *p2, *p3;
  long long step;

  // true when every chunk of the tile is either fully in range or fully out of range
  __device__ __forceinline__ static bool regular(int rows_valid) {
    return !TRANS || rows_valid >= ROWS || (rows_valid % EPC) == 0;
  }
  __device__ __forceinline__ void init(const void* opnd, long long off, long long ld, int rows_valid, int k0, int tid) {
    const ST* base = reinterpret_cast<const ST*>(opnd) + off;
    const ST* safe = reinterpret_cast<const ST*>(opnd);
    if constexpr (!TRANS) {
      const int row = tid >> 3;
      const long long ko = k0 + (tid & 7) * EPC;
      p0 = (row < rows_valid ? base + (long long)row * ld : safe) + ko;
      p1 = (row + 32 < rows_valid ? base + (long long)(row + 32) * ld : safe) + ko;
      p2 = (row + 64 < rows_valid ? base + (long long)(row + 64) * ld : safe) + ko;
      p3 = (row + 96 < rows_valid ? base + (long long)(row + 96) * ld : safe) + ko;
      step = KT;
    } else {
      constexpr int QN = KT / 4, UNITS = QN * (ROWS / EPC);
      const int q = tid % QN, c0 = (tid / QN) * EPC;
      const bool ok = tid < UNITS && c0 < rows_valid;
      const ST* b = (ok ? base + c0 : safe) + (long long)(k0 + 4 * q) * ld;
      p0 = b; p1 = b + ld; p2 = b + 2 * ld; p3 = b + 3 * ld;
      step = (long long)KT * ld;
    }
  }
  // init for a row-major operand whose rows are gathered (RowGather)
  __device__ __forceinline__ void init_rows(const void* opnd, long long off, const RowGather& rg, int rows_valid, int k0, int tid) {
    static_assert(!TRANS, "gathered rows: row-major operands only");
    const ST* base = reinterpret_cast<const ST*>(opnd) + off;
    const ST* safe = reinterpret_cast<const ST*>(opnd);
    const int row = tid >> 3;
    const long long ko = k0 + (tid & 7) * EPC;
    p0 = (row < rows_valid ? base + rg.o0 : safe) + ko;
    p1 = (row + 32 < rows_valid ? base + rg.o1 : safe) + ko;
    p2 = (row + 64 < rows_valid ? base + rg.o2 : safe) + ko;
    p3 = (row + 96 < rows_valid ? base + rg.o3 : safe) + ko;
    step = KT;
  }
  __device__ __forceinline__ u32x4 ld1(const ST* p) const {
    if constexpr (sizeof(CT) == 4) {
      return *reinterpret_cast<const u32x4*>(p);
    } else if constexpr (sizeof(ST) == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p);
      const f32x4 b = *reinterpret_cast<const f32x4*>(p + 4);
      return u32x4{pack_bf2(a.x, a.y), pack_bf2(a.z, a.w), pack_bf2(b.x, b.y), pack_bf2(b.z, b.w)};
    } else if constexpr (V16) {
      return *reinterpret_cast<const u32x4*>(p);
    } else {
      const u32x2 a = *reinterpret_cast<const u32x2*>(p);
      const u32x2 b = *reinterpret_cast<const u32x2*>(p + 4);
      return u32x4{a.x, a.y, b.x, b.y};
    }
  }
  __device__ __forceinline__ RTile load() {
    RTile t;
    t.r0 = t.r1 = t.r2 = t.r3 = zero4();
    if constexpr (!TRANS) {
      t.r0 = ld1(p0); p0 += step;
      if constexpr (ROWS >= 64) { t.r1 = ld1(p1); p1 += step; }
      if constexpr (ROWS >= 128) { t.r2 = ld1(p2); p2 += step; t.r3 = ld1(p3); p3 += step; }
    } else {
      t.r0 = ld1(p0); t.r1 = ld1(p1); t.r2 = ld1(p2); t.r3 = ld1(p3);
      p0 += step; p1 += step; p2 += step; p3 += step;
    }
    return t;
  }
};

struct KArgs {
  unsigned long long* stamps;
  const void* A;
  const void* B;
  long long a_off, b_off, lda, ldb;
  int a_rows, b_rows, K, kt0, kt1;
  bool do_bsum;
};

// The K loop of one workgroup.  Per K-tile: issue the global loads of tile t+1, multiply tile t out of LDS,
// then -- and only then -- wait for the loads and store them to the other LDS buffer; one barrier per K-tile.
// Whole K-tiles of regular tiles go through the FastLoader; a ragged last K-tile (K = 84, odd batch sizes as the
// reduction dimension) and irregular edge tiles take the generic clamped loader.
// AG: the rows of A are gathered -- row j of the tile starts ag.o<j> elements behind A + a_off (ka.lda is unused).
template <typename CT, int BM, int BN, bool TA, bool TB, int AM, int BMODE, int TM, int TN, bool AG = false>
__device__ __forceinline__ void k_loop(const KArgs& ka, unsigned char* lds, f32x4 (&acc)[TM][TN], float (&bsum)[TM],
                                       const RowGather& ag = RowGather{}) {
  constexpr int KT = Elem<CT>::KT;
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int A_BYTES = BM * LDS_ROW, B_BYTES = BN * LDS_ROW, STAGE = A_BYTES + B_BYTES;
  typedef typename SrcOf<CT, AM>::type AST;
  typedef typename SrcOf<CT, BMODE>::type BST;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;
  const int K = ka.K, kt0 = ka.kt0, kt1 = ka.kt1;
  if (kt0 >= kt1) { __syncthreads(); return; }

  RTile ra, rb;
  auto gload_generic = [&](int k0) __attribute__((always_inline)) {
    const AST* ab = reinterpret_cast<const AST*>(ka.A);
    const BST* bb = reinterpret_cast<const BST*>(ka.B);
    if constexpr (AG) ra = tile_gload_rows<CT, AST, BM, SrcOf<CT, AM>::V16>(ab + ka.a_off, ab, ag, ka.a_rows, k0, K, tid);
    else ra = tile_gload<CT, AST, BM, TA, SrcOf<CT, AM>::V16>(ab + ka.a_off, ab, ka.lda, ka.a_rows, k0, K, tid);
    rb = tile_gload<CT, BST, BN, TB, SrcOf<CT, BMODE>::V16>(bb + ka.b_off, bb, ka.ldb, ka.b_rows, k0, K, tid);
  };
  auto lstore = [&](int buf) __attribute__((always_inline)) {
    tile_lstore<CT, BM, TA>(lds + buf * STAGE, ra, tid);
    tile_lstore<CT, BN, TB>(lds + buf * STAGE + A_BYTES, rb, tid);
  };
  auto ktail = [&](int k0) __attribute__((always_inline)) {
    ra = tile_ktail_mask<CT, TA>(ra, k0, K, tid);
    rb = tile_ktail_mask<CT, TB>(rb, k0, K, tid);
  };
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
      if (ka.do_bsum) {
#pragma unroll
        for (int i = 0; i < TM; ++i) bsum[i] += chunk_sum<CT>(fa[i]);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = mma_chunk<CT>(fa[i], fb[j], acc[i][j]);
    }
  };

  // tiles [kt0, kfull) are whole K-tiles; kfull == kt0 when this tile cannot use the fast loader
  const bool regular = FastLoader<CT, BM, TA, AM>::regular(ka.a_rows) && FastLoader<CT, BN, TB, BMODE>::regular(ka.b_rows);
  int kfull = K / KT;
  if (kfull > kt1) kfull = kt1;
  if (!regular || kfull < kt0) kfull = kt0;

  int kt = kt0;
  // ---- prologue: tile kt0 into LDS buffer 0
  FastLoader<CT, BM, TA, AM> fa_;
  FastLoader<CT, BN, TB, BMODE> fb_;
  if (kt0 < kfull) {
    if constexpr (AG) fa_.init_rows(ka.A, ka.a_off, ag, ka.a_rows, kt0 * KT, tid);
    else fa_.init(ka.A, ka.a_off, ka.lda, ka.a_rows, kt0 * KT, tid);
    fb_.init(ka.B, ka.b_off, ka.ldb, ka.b_rows, kt0 * KT, tid);
    ra = fa_.load();
    rb = fb_.load();
  } else {
    gload_generic(kt0 * KT);
    if (kt0 * KT + KT > K) ktail(kt0 * KT);
  }
  lstore(0);
  __syncthreads();
  // ---- main loop: the NEXT tile is a whole K-tile -> pointer-bump loads, no masking
  for (; kt + 1 < kfull; ++kt) {
    const int cur = (kt - kt0) & 1;
    STAMP(0);
    ra = fa_.load();
    rb = fb_.load();
    STAMP(1);
    compute(cur);
    STAMP(2);
    MMDEER_STAMP_DRAIN();
    STAMP(3);
    lstore(cur ^ 1);
    STAMP(4);
    __syncthreads();
    STAMP(5);
  }
  // ---- tail: at most the last whole tile plus a ragged one (or every tile of an irregular edge tile)
  for (; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    const bool more = kt + 1 < kt1;
    if (more) gload_generic((kt + 1) * KT);
    compute(cur);
    if (more) {
      if ((kt + 1) * KT + KT > K) ktail((kt + 1) * KT);
      lstore(cur ^ 1);
    }
    __syncthreads();
  }
}

constexpr int cmax(int a, int b) { return a > b ? a : b; }

// Epilogue shared by the register-staged and the LDS-DMA kernels: accumulators -> fp32 staging in LDS (the K loop
// must have ended with a barrier: the operand tiles are dead) -> one thread per 4 consecutive columns applies
// bias / ReLU / dropout / (Y > 0) mask and issues coalesced 8- or 16-byte stores.
template <int BM, int BN, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue(const GemmGroup& g, const __attribute__((address_space(4))) GemmProblem& p,
                                              unsigned char* lds, f32x4 (&acc)[TM][TN], int z, int slice, int row0, int col0) {
  constexpr int WTM = BM / 2, WTN = BN / 2;
  constexpr int SPAD = BN + 4;  // fp32 staging row stride (elements)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;
  const int M = p.M, N = p.N;
  const bool sliced = p.splitk > 1;
  // ---- epilogue phase 1: accumulators -> fp32 staging (the K loop ended with a barrier: tiles are dead)
  float* S = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        S[(wm * WTM + i * 16 + lg * 4 + r) * SPAD + wn * WTN + j * 16 + li] = acc[i][j][r];
  __syncthreads();

  // ---- phase 2: one thread per 4 consecutive columns
  const DropCtx dc = g.drop;
  const long long c_base = (long long)z * p.sC;
  if (sliced) {
    float* cs = p.slab_c + (long long)slice * p.slab_stride + c_base;
#pragma unroll 2
    for (int c = tid; c < BM * BN / 4; c += 256) {
      const int row = c / (BN / 4), cc = c - row * (BN / 4);
      const int gr = row0 + row, gc = col0 + cc * 4;
      if (gr >= M || gc >= N) continue;
      *reinterpret_cast<f32x4*>(cs + (long long)gr * p.ldc + gc) = *reinterpret_cast<const f32x4*>(S + row * SPAD + cc * 4);
    }
    return;
  }
  // 256 is a multiple of BN/4, so a thread keeps ONE column chunk (cc) for all its rows: the bias chunk, the
  // dropout key and every descriptor field are loaded once, outside the row loop
  const int cc = tid % (BN / 4), gc = col0 + cc * 4;
  const bool col_ok = gc < N;
  f32x4 bias4{0.f, 0.f, 0.f, 0.f};
  if (p.bias && col_ok) bias4 = *reinterpret_cast<const f32x4*>(p.bias + (long long)z * p.sBias + gc);
  const int relu = p.relu, accumulate = p.accumulate, c_f32 = p.c_f32, y_f32 = p.y_f32, shift = p.drop_shift;
  const int site = p.drop_site >= 0 ? p.drop_site : p.regen_site;
  const unsigned dkey = site >= 0 ? drop_key(dc, site) : 0u;
  const unsigned dcol = (unsigned)(gc + z * N);   // batched problems: the column index continues across the batch
  const void* Yp = p.Y;
  void* Cp = p.C;
  const long long ldc = p.ldc, ldy = p.ldy, y_base = (long long)z * p.sY;
  const float ms = p.mask_scale;
#pragma unroll 4
  for (int row = tid / (BN / 4); row < BM; row += 256 / (BN / 4)) {
    const int gr = row0 + row;
    if (gr >= M || !col_ok) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(S + row * SPAD + cc * 4);
    v += bias4;
    if (relu) v = relu4(v);
    if (site >= 0) v = drop4(v, ((unsigned)gr * 0x9E3779B1u) ^ dkey, dcol, shift, dc);
    if (Yp) {
      const long long yo = y_base + (long long)gr * ldy + gc;
      float y0, y1, y2, y3;   // four scalars across the join: one vector value there changes the register assignment
      if (y_f32) {
        const f32x4 y = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(Yp) + yo);
        y0 = y.x; y1 = y.y; y2 = y.z; y3 = y.w;
      } else {
        const f32x4 y = bf4_to_f32(*reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(Yp) + yo));
        y0 = y.x; y1 = y.y; y2 = y.z; y3 = y.w;
      }
      v.x = y0 > 0.f ? v.x * ms : 0.f; v.y = y1 > 0.f ? v.y * ms : 0.f;
      v.z = y2 > 0.f ? v.z * ms : 0.f; v.w = y3 > 0.f ? v.w * ms : 0.f;
    }
    const long long co = c_base + (long long)gr * ldc + gc;
    if (c_f32) {
      float* cp = reinterpret_cast<float*>(Cp) + co;
      if (accumulate) {
        f32x4 o = *reinterpret_cast<const f32x4*>(cp);
        v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
      }
      *reinterpret_cast<f32x4*>(cp) = v;
    } else {
      *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(Cp) + co) = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
    }
  }
}

// second launch-bound argument = waves per SIMD the register allocator must leave room for:
// 64x64 tiles run 3 workgroups per CU (LDS 36 KiB each), the larger tiles 2.
// Epilogue straight from the accumulators.  The kernels below issue their MFMAs with the operands swapped
// (D[n][m] += W-fragment x A-fragment), so a lane holds FOUR CONSECUTIVE COLUMNS n of one output row m:
// acc[i][j] = C[m = row0 + wm*WTM + 16 i + li][n = col0 + wn*WTN + 16 j + 4 lg + {0..3}].  Bias, ReLU, dropout, the
// (Y > 0) mask and the store are lane-local: no LDS staging, no barrier, one 8-byte (bf16) / 16-byte (fp32) store
// per accumulator.  bias4[j] was loaded before the K loop.
template <int TM, int TN, int WTM, int WTN, bool HAS_Y>
__device__ __forceinline__ void epilogue_direct(const GemmGroup& g, const __attribute__((address_space(4))) GemmProblem& p,
                                                f32x4 (&acc)[TM][TN], const f32x4 (&bias4)[TN], int z, int row0, int col0,
                                                int wm, int wn, int li, int lg) {
  const int M = p.M, N = p.N;
  const DropCtx dc = g.drop;
  const int relu = p.relu, accumulate = p.accumulate, c_f32 = p.c_f32, y_f32 = p.y_f32, shift = p.drop_shift;
  const int site = p.drop_site >= 0 ? p.drop_site : p.regen_site;
  const unsigned dkey = site >= 0 ? drop_key(dc, site) : 0u;
  const void* Yp = HAS_Y ? p.Y : nullptr;   // HAS_Y = false: the caller guarantees p.Y == null (saves TM*TN*4 registers)
  void* Cp = p.C;
  const long long ldc = p.ldc, ldy = p.ldy, c_base = (long long)z * p.sC, y_base = (long long)z * p.sY;
  const float ms = p.mask_scale;
  const int nb = col0 + wn * WTN + 4 * lg, mb = row0 + wm * WTM + li;
  // mask source first: all loads in flight together
  f32x4 yv[HAS_Y ? TM : 1][HAS_Y ? TN : 1];
  if constexpr (HAS_Y) if (Yp) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int m = mb + 16 * i, n = nb + 16 * j;
        yv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (m < M && n < N) {
          const long long yo = y_base + (long long)m * ldy + n;
          if (y_f32) yv[i][j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(Yp) + yo);
          else yv[i][j] = bf4_to_f32(*reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(Yp) + yo));
        }
      }
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = mb + 16 * i;
    if (m >= M) continue;
    const unsigned rk = ((unsigned)m * 0x9E3779B1u) ^ dkey;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = nb + 16 * j;
      if (n >= N) continue;   // N % 4 == 0: a 4-column group is all in or all out
      f32x4 v = acc[i][j] + bias4[j];
      if (relu) v = relu4(v);
      // batched problems: the column index continues across the batch
      if (site >= 0) v = drop4(v, rk, (unsigned)(n + z * N), shift, dc);
      if constexpr (HAS_Y) if (Yp) {
        const f32x4 y = yv[i][j];
        v.x = y.x > 0.f ? v.x * ms : 0.f; v.y = y.y > 0.f ? v.y * ms : 0.f;
        v.z = y.z > 0.f ? v.z * ms : 0.f; v.w = y.w > 0.f ? v.w * ms : 0.f;
      }
      const long long co = c_base + (long long)m * ldc + n;
      if (c_f32) {
        float* cp = reinterpret_cast<float*>(Cp) + co;
        if (accumulate) v += *reinterpret_cast<const f32x4*>(cp);
        *reinterpret_cast<f32x4*>(cp) = v;
      } else {
        *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(Cp) + co) = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
      }
    }
  }
}

template <typename CT, int BM, int BN, bool TA, bool TB, int AM, int BMODE>
__global__ __launch_bounds__(256, (BM * BN <= 64 * 64) ? 3 : 2) void gemm_group_kernel(const GemmGroup g) {
  constexpr int KT = Elem<CT>::KT;
  constexpr int WTM = BM / 2, WTN = BN / 2, TM = WTM / 16, TN = WTN / 16;
  constexpr int A_BYTES = BM * LDS_ROW, B_BYTES = BN * LDS_ROW, STAGE = A_BYTES + B_BYTES;
  constexpr int SPAD = BN + 4;  // fp32 staging row stride (elements)
  constexpr int LDS_BYTES = cmax(2 * STAGE, BM * SPAD * 4);
  __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 15, lg = lane >> 4;

  int bid = blockIdx.x;
  if (g.xcd_remap) bid = xcd_contiguous(bid, gridDim.x);
  TileAt at;
  const __attribute__((address_space(4))) GemmProblem& p = *locate_tile(g, bid, 0, at);
  const int z = at.z, slice = at.slice, tmb = at.tmb, tnb = at.tnb;
  const int row0 = tmb * BM, col0 = tnb * BN;
  const int M = p.M, N = p.N, K = p.K;

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) bsum[i] = 0.f;
  const bool do_bsum = (p.bias_grad != nullptr) && (tnb == 0) && (wn == 0);

  // K-tile range of this slice
  const int nk_all = (K + KT - 1) / KT;
  const int nk_per = (nk_all + p.splitk - 1) / p.splitk;
  const int kt0 = slice * nk_per;
  const int kt1 = (kt0 + nk_per < nk_all) ? kt0 + nk_per : nk_all;

  KArgs ka;
  ka.stamps = g.stamps;
  ka.A = p.A; ka.B = p.B;
  // element offsets of this tile's first operand row (k = 0)
  ka.a_off = (long long)z * p.sA + (TA ? (long long)row0 : (long long)row0 * p.lda);
  ka.b_off = (long long)z * p.sB + (TB ? (long long)col0 : (long long)col0 * p.ldb);
  ka.lda = p.lda; ka.ldb = p.ldb;
  ka.a_rows = M - row0; ka.b_rows = N - col0;
  ka.K = K; ka.kt0 = kt0; ka.kt1 = kt1; ka.do_bsum = do_bsum;
  k_loop<CT, BM, BN, TA, TB, AM, BMODE>(ka, lds, acc, bsum);

  const bool sliced = p.splitk > 1;
  // ---- bias gradient (dW problems): row sums of op(A) over this slice of the reduction
  if (do_bsum) {
    float* bg = sliced ? p.slab_b + (long long)slice * p.slab_stride : p.bias_grad;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      float v = bsum[i];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      int r = row0 + wm * WTM + i * 16 + li;
      if (lg == 0 && r < M) bg[(long long)z * p.sBiasGrad + r] = v;
    }
  }

  gemm_epilogue<BM, BN>(g, p, lds, acc, z, slice, row0, col0);
}

template <typename CT, int BM, int BN, bool TA, bool TB, int AM, int BMODE>
int launch_variant(const GemmGroup& g, int total, hipStream_t stream) {
  hipLaunchKernelGGL((gemm_group_kernel<CT, BM, BN, TA, TB, AM, BMODE>), dim3(total), dim3(256), 0, stream, g);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

// dispatch over the three tile shapes for one (transposition, mode pair)
template <typename CT, bool TA, bool TB, int AM, int BMODE>
int launch_tiles(const GemmGroup& g, int total, const GemmRoute& r, hipStream_t stream) {
  if (r.BM == 64) return launch_variant<CT, 64, 64, TA, TB, AM, BMODE>(g, total, stream);
  if (r.BN == 64) return launch_variant<CT, 128, 64, TA, TB, AM, BMODE>(g, total, stream);
  return launch_variant<CT, 128, 128, TA, TB, AM, BMODE>(g, total, stream);
}

// The launcher of one transposition's register-staged kernels: fp32 compute, or one instantiation per bf16 source-mode pair of
// PAIRS (gemm.h: GEMM_MODE_PAIRS_*; launch_gemm_group has refused every other pair)
#define GEMM_REG_LAUNCH_PAIR(a, b) \
  if (am == a && bm == b) return launch_tiles<bf16_t, TA, TB, a, b>(g, total, r, s);
#define GEMM_REG_LAUNCHER(name, ta, tb, PAIRS)                                                                        \
  int name(const GemmGroup& g, int total, const GemmRoute& r, int compute_f32, hipStream_t s) {                       \
    constexpr bool TA = ta, TB = tb;                                                                                  \
    const int am = g.p[0].a_mode, bm = g.p[0].b_mode;                                                                 \
    if (compute_f32) return launch_tiles<float, TA, TB, SRC_F32, SRC_F32>(g, total, r, s);                            \
    PAIRS(GEMM_REG_LAUNCH_PAIR)                                                                                       \
    set_error("gemm: source-mode pair (%d,%d) is not instantiated for trans=(%d,%d)", am, bm, (int)TA, (int)TB);      \
    return -1;                                                                                                        \
  }

}  // namespace
}  // namespace mmdeer
