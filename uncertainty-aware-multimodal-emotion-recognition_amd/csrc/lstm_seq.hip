// Temporal audio encoder (reference src/models/encoders.py:376-389 at T > 1): the recurrence of one bidirectional
// nn.LSTM layer over all T steps, forward and backpropagation through time, and the attention pool over time.
//
// Recurrence (mmdeer_lstm_seq_fwd / _bwd).  A workgroup owns BT batch rows of ONE direction and steps through all T in
// one launch; no workgroup ever waits on another.  Its 4 waves own 64 hidden units each, with all four gates of them
// (256 gate columns), so the cell update runs in registers on the MFMA accumulators and c stays in fp32 registers.
//   forward:  pre_t = xg_t + h_{t-1} W_hh^T      h_{t-1}: LDS [BT][H] (double-buffered, one barrier per step)
//   backward: dh_rec = dgates_{t'} W_hh          dgates_{t'}: LDS [BT][4H] (two barriers per step)
// W_hh (forward) and W_hh^T (backward) are read from L2 every step: row-major images in the compute dtype that
// mmdeer_lstm_seq_pack writes once per forward from the fp32 parameters.  Each lane reads 16 contiguous bytes of one
// image row per MFMA operand fragment.  bf16: v_mfma_f32_16x16x32_bf16, BT = 32;  fp32: v_mfma_f32_16x16x4_f32 (four per
// 16-byte fragment, k permuted identically in both operands), BT = 16.
//
// Pool (mmdeer_temporal_pool_fwd / _bwd): one wave per sample, s_t = w2 . tanh(z_t) + b2, softmax over t (max-subtracted,
// online), attended = sum_t a_t h_t.  The backward writes the pool's share of dh (a_t dout; the score path reaches h through
// dz W1, a GEMM of the caller), dz, dw2 (per-workgroup partials folded in index order by a second launch: deterministic) and
// db2 = 0: b2 shifts every score of a sample equally, so the softmax does not depend on it.
#include "../../include/mmdeer.h"
#include "../../include/mmdeer_seqlen.h"
#include "elem.h"
#include "rowops.h"

namespace mmdeer {
namespace {

constexpr int SEQ_H = 256;          // hidden units per direction (the reference's hidden_dim 512 / 2)
constexpr int SEQ_G = 4 * SEQ_H;    // gate columns per direction

template <bool F32> struct SeqCfg;
template <> struct SeqCfg<false> {
  typedef bf16_t E;
  static constexpr int MT = 2, BT = 32, EPL = 8;   // 16-row M tiles per workgroup, rows, elements per 16-byte fragment
};
template <> struct SeqCfg<true> {
  typedef float E;
  static constexpr int MT = 1, BT = 16, EPL = 4;
};

// LEN (include/mmdeer_seqlen.h): the same kernels on the plain struct plus `lengths`; LEN = false is the plain entry's code
template <bool LEN> struct SeqArgsT { typedef mmdeer_lstm_seq_args type; };
template <> struct SeqArgsT<true> { typedef mmdeer_lstm_seq_len_args type; };
template <bool LEN> struct PoolArgsT { typedef mmdeer_temporal_pool_args type; };
template <> struct PoolArgsT<true> { typedef mmdeer_temporal_pool_len_args type; };

// the valid steps of batch row b: lengths[b] clamped to [0, T]; rows past B have none
__device__ __forceinline__ int seq_len_of(const int32_t* lengths, int b, int B, int T) {
  return b < B ? min(max(lengths[b], 0), T) : 0;
}

// 1 - x^2 of the backward's cell update.  In the plain kernel the compiler leaves it a product and a subtraction; under the LEN
// predicate it would fuse 1 - tg^2 into one fma and the gate gradients would differ from the plain entry's in the last bit.  LEN
// states the plain kernel's two roundings (the bit-for-bit test of full lengths against lengths=None holds the two together).
template <bool LEN>
__device__ __forceinline__ float one_minus_sq(float x) {
  if constexpr (LEN) {
#pragma clang fp contract(off)
    const float q = x * x;
    return 1.f - q;
  } else {
    return 1.f - x * x;
  }
}

template <bool F32>
__device__ __forceinline__ f32x4 mma16(const u32x4& a, const u32x4& b, f32x4 acc) {
  if constexpr (!F32) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  } else {
    // lane (l & 15, g = l >> 4) holds k = 16 s + 4 g + e in element e, in A and B alike
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    return acc;
  }
}

// image[d][n][k] = W_d[n][k], image_t[d][k][n] = W_d[n][k] (compute dtype); W_d fp32 [4H][H]
template <bool F32>
__global__ __launch_bounds__(256) void lstm_seq_pack_kernel(const float* wf, const float* wr, void* img, void* img_t) {
  const long long per = (long long)SEQ_G * SEQ_H, total = 2 * per;
  for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += gridDim.x * 256ll) {
    const int d = (int)(e / per);
    const long long r = e - d * per;
    const int n = (int)(r / SEQ_H), k = (int)(r - (long long)n * SEQ_H);
    const float v = (d ? wr : wf)[r];
    st1<F32>(img, e, v);
    if (img_t) st1<F32>(img_t, d * per + (long long)k * SEQ_G + n, v);
  }
}

// grid (ceil(B / BT), 2): blockIdx.y = direction.  Rows of xg / h / the tape are t * B + b (time-major).
// LEN: row b runs its own n_b steps (the reverse direction from t = n_b - 1): at t >= n_b its c stands still, xg is not read and 0 goes
// to h in memory and in the LDS tile, so a row that starts late starts from zero state.  The workgroup steps to TL = the largest n_b
// of its rows (uniform, formed once) and stores the h rows t >= TL as zeros afterwards.
template <bool F32, bool LEN = false>
__global__ __launch_bounds__(256) void lstm_seq_fwd_kernel(typename SeqArgsT<LEN>::type a) {
  typedef SeqCfg<F32> Cf;
  typedef typename Cf::E E;
  constexpr int H = SEQ_H, G4 = SEQ_G, MT = Cf::MT, BT = Cf::BT, EPL = Cf::EPL, KC = 4 * EPL, LDS_LD = H + EPL;
  __shared__ __attribute__((aligned(16))) E hs[2][BT * LDS_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = blockIdx.y, lr = lane & 15, lg = lane >> 4;
  const int b0 = blockIdx.x * BT, T = a.T, B = a.B;
  const E* W = reinterpret_cast<const E*>(a.w_hh) + (long long)d * G4 * H;
  const bool tape = a.tape_gates != nullptr;
  float cst[MT][4][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt)
#pragma unroll
      for (int i = 0; i < 4; ++i) cst[m][jt][i] = 0.f;
  int TL = T;
  int nl[MT][4];                                   // LEN: the lengths of the rows this lane owns
  if constexpr (LEN) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) nl[m][i] = seq_len_of(a.lengths, b0 + m * 16 + lg * 4 + i, B, T);
    TL = 0;
    for (int r = 0; r < BT; ++r) TL = max(TL, seq_len_of(a.lengths, b0 + r, B, T));
    TL = __builtin_amdgcn_readfirstlane(TL);
  }

  for (int s = 0; s < TL; ++s) {
    const int t = d == 0 ? s : TL - 1 - s;
    f32x4 acc[MT][4][4];   // [m][gate][16-unit tile]
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[m][g][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s > 0) {                                   // h_{-1} = 0: the first step has no recurrent product
      const E* hp = hs[(s - 1) & 1];
#pragma unroll 2
      for (int kc = 0; kc < H / KC; ++kc) {
        u32x4 af[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = *reinterpret_cast<const u32x4*>(hp + (m * 16 + lr) * LDS_LD + kc * KC + lg * EPL);
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int jt = 0; jt < 4; ++jt) {
            const u32x4 bf = *reinterpret_cast<const u32x4*>(W + (long long)(g * H + w * 64 + jt * 16 + lr) * H + kc * KC + lg * EPL);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m][g][jt] = mma16<F32>(af[m], bf, acc[m][g][jt]);
          }
      }
    }
    E* hn = hs[s & 1];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = m * 16 + lg * 4 + i, b = b0 + r, j = w * 64 + jt * 16 + lr;
          float hv = 0.f;
          if (b < B) {
            const long long row = (long long)t * B + b;
            bool live = true;
            if constexpr (LEN) live = t < nl[m][i];
            if (live) {
              const long long xo = row * a.ld_xg + d * G4 + j;
              const float si = sigmoidf_(acc[m][0][jt][i] + ld1<F32>(a.xg, xo));
              const float sf = sigmoidf_(acc[m][1][jt][i] + ld1<F32>(a.xg, xo + H));
              const float tg = tanhf(acc[m][2][jt][i] + ld1<F32>(a.xg, xo + 2 * H));
              const float so = sigmoidf_(acc[m][3][jt][i] + ld1<F32>(a.xg, xo + 3 * H));
              const float c = sf * cst[m][jt][i] + si * tg;
              cst[m][jt][i] = c;
              hv = so * tanhf(c);
              if (tape) {
                float* gt = a.tape_gates + row * (2 * G4) + d * G4 + j;
                gt[0] = si; gt[H] = sf; gt[2 * H] = tg; gt[3 * H] = so;
                a.tape_c[row * (2 * H) + d * H + j] = c;
              }
            }
            st1<F32>(a.h, row * a.ld_h + d * H + j, hv);
          }
          st1<F32>(hn, r * LDS_LD + j, hv);       // rows past B stay zero: the MFMA reads whole tiles
        }
    __syncthreads();
  }
  if constexpr (LEN) {
    for (int t = TL; t < T; ++t)                   // the steps no row of this workgroup has: pad_packed_sequence's zeros
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + m * 16 + lg * 4 + i, j = w * 64 + jt * 16 + lr;
            if (b < B) st1<F32>(a.h, ((long long)t * B + b) * a.ld_h + d * H + j, 0.f);
          }
  }
}

// Backpropagation through time, one direction per blockIdx.y, steps in the order opposite to the forward's.
//   dh_t = dh_out_t + dgates_{t'} W_hh      (t' = the step the forward ran after t)
//   dc_t = dh_t o_t (1 - tanh^2 c_t) + dc_{t'} f_{t'}
// LEN: the same bound TL and per-row predicate; at t >= n_b the row's dgates are 0 (stored, and in the LDS tile) and its carry stands
// still; the reverse direction's row b has a previous state only while t + 1 < n_b.
template <bool F32, bool LEN = false>
__global__ __launch_bounds__(256) void lstm_seq_bwd_kernel(typename SeqArgsT<LEN>::type a) {
  typedef SeqCfg<F32> Cf;
  typedef typename Cf::E E;
  constexpr int H = SEQ_H, G4 = SEQ_G, MT = Cf::MT, BT = Cf::BT, EPL = Cf::EPL, KC = 4 * EPL, LDS_LD = G4 + EPL;
  __shared__ __attribute__((aligned(16))) E gs[BT * LDS_LD];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, d = blockIdx.y, lr = lane & 15, lg = lane >> 4;
  const int b0 = blockIdx.x * BT, T = a.T, B = a.B;
  const E* WT = reinterpret_cast<const E*>(a.w_hh_t) + (long long)d * H * G4;
  float carry[MT][4][4];
  f32x4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      acc[m][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) carry[m][jt][i] = 0.f;
    }
  int TL = T;
  int nl[MT][4];
  if constexpr (LEN) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int i = 0; i < 4; ++i) nl[m][i] = seq_len_of(a.lengths, b0 + m * 16 + lg * 4 + i, B, T);
    TL = 0;
    for (int r = 0; r < BT; ++r) TL = max(TL, seq_len_of(a.lengths, b0 + r, B, T));
    TL = __builtin_amdgcn_readfirstlane(TL);
  }

  for (int s = 0; s < TL; ++s) {
    const int t = d == 0 ? TL - 1 - s : s;
    const bool has_prev_all = d == 0 ? t > 0 : t < T - 1;   // the forward's state before step t (else c = 0)
    const int tp = d == 0 ? t - 1 : t + 1;
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int r = m * 16 + lg * 4 + i, b = b0 + r, j = w * 64 + jt * 16 + lr;
          float dg[4] = {0.f, 0.f, 0.f, 0.f};
          if (b < B) {
            const long long row = (long long)t * B + b;
            bool live = true, has_prev = has_prev_all;
            if constexpr (LEN) {
              live = t < nl[m][i];
              has_prev = d == 0 ? t > 0 : t + 1 < nl[m][i];
            }
            if (live) {
              const float dh = ld1<F32>(a.dh_out, row * a.ld_dh + d * H + j) + acc[m][jt][i];
              const float* gt = a.tape_gates + row * (2 * G4) + d * G4 + j;
              const float si = gt[0], sf = gt[H], tg = gt[2 * H], so = gt[3 * H];
              const float c = a.tape_c[row * (2 * H) + d * H + j];
              const float cp = has_prev ? a.tape_c[((long long)tp * B + b) * (2 * H) + d * H + j] : 0.f;
              const float tc = tanhf(c);
              const float dc = dh * so * one_minus_sq<LEN>(tc) + carry[m][jt][i];
              carry[m][jt][i] = dc * sf;
              dg[0] = dc * tg * si * (1.f - si);
              dg[1] = dc * cp * sf * (1.f - sf);
              dg[2] = dc * si * one_minus_sq<LEN>(tg);
              dg[3] = dh * tc * so * (1.f - so);
            }
            const long long go = row * a.ld_dg + d * G4 + j;
#pragma unroll
            for (int g = 0; g < 4; ++g) st1<F32>(a.dgates, go + g * H, dg[g]);
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) st1<F32>(gs, r * LDS_LD + g * H + j, dg[g]);
        }
    __syncthreads();
    if (s + 1 < TL) {
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) acc[m][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int kc = 0; kc < G4 / KC; ++kc) {
        u32x4 af[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) af[m] = *reinterpret_cast<const u32x4*>(gs + (m * 16 + lr) * LDS_LD + kc * KC + lg * EPL);
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) {
          const u32x4 bf = *reinterpret_cast<const u32x4*>(WT + (long long)(w * 64 + jt * 16 + lr) * G4 + kc * KC + lg * EPL);
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][jt] = mma16<F32>(af[m], bf, acc[m][jt]);
        }
      }
    }
    __syncthreads();
  }
  if constexpr (LEN) {
    for (int t = TL; t < T; ++t)                   // the steps no row of this workgroup has: zero gate gradients
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int jt = 0; jt < 4; ++jt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + m * 16 + lg * 4 + i, j = w * 64 + jt * 16 + lr;
            if (b < B) {
              const long long go = ((long long)t * B + b) * a.ld_dg + d * G4 + j;
#pragma unroll
              for (int g = 0; g < 4; ++g) st1<F32>(a.dgates, go + g * H, 0.f);
            }
          }
  }
}

// ---- attention pool over time: one wave per sample; lane l owns z columns 4l .. 4l+3 and h columns 8l .. 8l+7
template <bool F32, typename Args>
__device__ __forceinline__ float pool_score(const Args& a, long long row, const f32x4& w2, float b2, int lane) {
  const f32x4 tz = tanh4(ld4<F32>(a.z, row * a.ld_z + lane * 4));
  return wave_sum(w2.x * tz.x + w2.y * tz.y + w2.z * tz.z + w2.w * tz.w) + b2;
}

// LEN: the softmax runs over t < n_b; the weights at t >= n_b are stored as zeros; n_b = 0 stores a zero row
template <bool F32, bool LEN = false>
__global__ __launch_bounds__(256) void temporal_pool_fwd_kernel(typename PoolArgsT<LEN>::type a) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;
  const int T = a.T, B = a.B;
  int n = T;
  if constexpr (LEN) n = seq_len_of(a.lengths, b, B, T);
  const f32x4 w2 = *reinterpret_cast<const f32x4*>(a.w2 + lane * 4);
  const float b2 = a.b2[0];
  float mx = -INFINITY, l = 0.f;
  for (int t = 0; t < n; ++t) {                    // online max / normaliser
    const float s = pool_score<F32>(a, (long long)t * B + b, w2, b2, lane);
    const float mn = fmaxf(mx, s);
    l = l * expf(mx - mn) + expf(s - mn);
    mx = mn;
  }
  const float inv = LEN && n == 0 ? 0.f : 1.f / l; // an empty sample: nothing to normalise, a zero row below
  f32x4 o0{0.f, 0.f, 0.f, 0.f}, o1{0.f, 0.f, 0.f, 0.f};
  for (int t = 0; t < n; ++t) {
    const long long row = (long long)t * B + b;
    const float at = expf(pool_score<F32>(a, row, w2, b2, lane) - mx) * inv;
    if (lane == 0) a.weights[(long long)b * T + t] = at;
    o0 += at * ld4<F32>(a.h, row * a.ld_h + lane * 8);
    o1 += at * ld4<F32>(a.h, row * a.ld_h + lane * 8 + 4);
  }
  if constexpr (LEN)
    for (int t = n + lane; t < T; t += 64) a.weights[(long long)b * T + t] = 0.f;
  st4<F32>(a.attended, (long long)b * a.ld_att + lane * 8, o0);
  st4<F32>(a.attended, (long long)b * a.ld_att + lane * 8 + 4, o1);
}

constexpr int POOL_BWD_WG = 256;   // workgroups of the backward: one fp32 [256] partial of dw2 each

// LEN: the sums run over t < n_b; dh and dz rows t >= n_b are stored as zeros
template <bool F32, bool LEN = false>
__global__ __launch_bounds__(256) void temporal_pool_bwd_kernel(typename PoolArgsT<LEN>::type a) {
  __shared__ f32x4 red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, T = a.T, B = a.B;
  const f32x4 w2 = *reinterpret_cast<const f32x4*>(a.w2 + lane * 4);
  f32x4 pw{0.f, 0.f, 0.f, 0.f};
  for (int b = blockIdx.x * 4 + w; b < B; b += gridDim.x * 4) {
    const f32x4 d0 = ld4<F32>(a.dout, (long long)b * a.ld_dout + lane * 8), d1 = ld4<F32>(a.dout, (long long)b * a.ld_dout + lane * 8 + 4);
    int n = T;
    if constexpr (LEN) n = seq_len_of(a.lengths, b, B, T);
    float dot = 0.f;                               // sum_t a_t (dout . h_t)
    for (int t = 0; t < n; ++t) {
      const long long row = (long long)t * B + b;
      const f32x4 h0 = ld4<F32>(a.h, row * a.ld_h + lane * 8), h1 = ld4<F32>(a.h, row * a.ld_h + lane * 8 + 4);
      const f32x4 p = d0 * h0 + d1 * h1;
      dot += a.weights[(long long)b * T + t] * wave_sum(p.x + p.y + p.z + p.w);
    }
    for (int t = 0; t < n; ++t) {
      const long long row = (long long)t * B + b;
      const float at = a.weights[(long long)b * T + t];
      const f32x4 h0 = ld4<F32>(a.h, row * a.ld_h + lane * 8), h1 = ld4<F32>(a.h, row * a.ld_h + lane * 8 + 4);
      const f32x4 p = d0 * h0 + d1 * h1;
      const float ds = at * (wave_sum(p.x + p.y + p.z + p.w) - dot);
      st4<F32>(a.dh, row * a.ld_dh + lane * 8, at * d0);
      st4<F32>(a.dh, row * a.ld_dh + lane * 8 + 4, at * d1);
      const f32x4 tz = tanh4(ld4<F32>(a.z, row * a.ld_z + lane * 4));
      st4<F32>(a.dz, row * a.ld_dz + lane * 4, ds * w2 * (1.f - tz * tz));
      pw += ds * tz;
    }
    if constexpr (LEN) {
      const f32x4 zero{0.f, 0.f, 0.f, 0.f};
      for (int t = n; t < T; ++t) {
        const long long row = (long long)t * B + b;
        st4<F32>(a.dh, row * a.ld_dh + lane * 8, zero);
        st4<F32>(a.dh, row * a.ld_dh + lane * 8 + 4, zero);
        st4<F32>(a.dz, row * a.ld_dz + lane * 4, zero);
      }
    }
  }
  red[w][lane] = pw;
  __syncthreads();
  if (w == 0)
    *reinterpret_cast<f32x4*>(a.scratch + blockIdx.x * 256 + lane * 4) = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
}

int check_seq(const mmdeer_lstm_seq_args* a, bool bwd, const char* op) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->T >= 0 && a->B >= 0, "%s: bad shape T=%d B=%d", op, a->T, a->B);
  MMDEER_CHECK(a->hidden == SEQ_H, "%s: hidden must be %d (got %d)", op, SEQ_H, a->hidden);
  MMDEER_CHECK(a->ndir == 2, "%s: ndir must be 2 (got %d)", op, a->ndir);
  if (a->T == 0 || a->B == 0) return 0;
  const int el = a->act_f32 ? 4 : 8;              // elements per 16 bytes
  if (!bwd) {
    MMDEER_CHECK(a->xg && a->w_hh && a->h, "%s: NULL pointer (xg, w_hh, h)", op);
    MMDEER_CHECK(!a->tape_gates == !a->tape_c, "%s: tape_gates and tape_c go together", op);
    MMDEER_CHECK(a->ld_xg >= 2 * SEQ_G && a->ld_h >= 2 * SEQ_H, "%s: leading dimensions too small (ld_xg=%d ld_h=%d)", op, a->ld_xg, a->ld_h);
    MMDEER_CHECK(al16(a->w_hh) && al16(a->tape_gates) && al16(a->tape_c), "%s: misaligned pointer (w_hh / tape need 16 bytes)", op);
    MMDEER_CHECK(al16(a->xg) && al16(a->h) && a->ld_xg % el == 0 && a->ld_h % el == 0,
                 "%s: misaligned pointer or leading dimension (xg / h rows need 16 bytes)", op);
  } else {
    MMDEER_CHECK(a->w_hh_t && a->tape_gates && a->tape_c && a->dh_out && a->dgates, "%s: NULL pointer (w_hh_t, tape, dh_out, dgates)", op);
    MMDEER_CHECK(a->ld_dh >= 2 * SEQ_H && a->ld_dg >= 2 * SEQ_G, "%s: leading dimensions too small (ld_dh=%d ld_dg=%d)", op, a->ld_dh, a->ld_dg);
    MMDEER_CHECK(al16(a->w_hh_t) && al16(a->tape_gates) && al16(a->tape_c), "%s: misaligned pointer (w_hh_t / tape need 16 bytes)", op);
    MMDEER_CHECK(al16(a->dh_out) && al16(a->dgates) && a->ld_dh % el == 0 && a->ld_dg % el == 0,
                 "%s: misaligned pointer or leading dimension (dh_out / dgates rows need 16 bytes)", op);
  }
  return 0;
}

int check_pool(const mmdeer_temporal_pool_args* a, bool bwd, const char* op) {
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->T >= 0 && a->B >= 0, "%s: bad shape T=%d B=%d", op, a->T, a->B);
  MMDEER_CHECK(a->hidden == SEQ_H, "%s: hidden must be %d (got %d)", op, SEQ_H, a->hidden);
  if (a->T == 0 || a->B == 0) return 0;
  const int el = a->act_f32 ? 4 : 8;
  MMDEER_CHECK(a->h && a->z && a->w2 && a->weights, "%s: NULL pointer (h, z, w2, weights)", op);
  MMDEER_CHECK(a->ld_h >= 2 * SEQ_H && a->ld_z >= SEQ_H, "%s: leading dimensions too small (ld_h=%d ld_z=%d)", op, a->ld_h, a->ld_z);
  MMDEER_CHECK(al16(a->h) && al16(a->z) && al16(a->w2) && a->ld_h % el == 0 && a->ld_z % el == 0,
               "%s: misaligned pointer or leading dimension (h, z, w2)", op);
  if (!bwd) {
    MMDEER_CHECK(a->b2 && a->attended, "%s: NULL pointer (b2, attended)", op);
    MMDEER_CHECK(a->ld_att >= 2 * SEQ_H, "%s: leading dimensions too small (ld_att=%d)", op, a->ld_att);
    MMDEER_CHECK(al16(a->attended) && a->ld_att % el == 0, "%s: misaligned pointer or leading dimension (attended)", op);
  } else {
    MMDEER_CHECK(a->dout && a->dh && a->dz && a->dw2 && a->db2 && a->scratch, "%s: NULL pointer (dout, dh, dz, dw2, db2, scratch)", op);
    MMDEER_CHECK(a->ld_dout >= 2 * SEQ_H && a->ld_dh >= 2 * SEQ_H && a->ld_dz >= SEQ_H,
                 "%s: leading dimensions too small (ld_dout=%d ld_dh=%d ld_dz=%d)", op, a->ld_dout, a->ld_dh, a->ld_dz);
    MMDEER_CHECK(al16(a->dout) && al16(a->dh) && al16(a->dz) && al16(a->scratch) && a->ld_dout % el == 0 && a->ld_dh % el == 0 &&
                 a->ld_dz % el == 0, "%s: misaligned pointer or leading dimension (dout, dh, dz, scratch)", op);
  }
  return 0;
}

// the _len structs are their counterparts with `lengths` appended: the counterpart's checks run on the leading fields
static_assert(offsetof(mmdeer_lstm_seq_len_args, lengths) == sizeof(mmdeer_lstm_seq_args) &&
              offsetof(mmdeer_lstm_seq_len_args, stream) == offsetof(mmdeer_lstm_seq_args, stream), "mmdeer_lstm_seq_len_args layout");
static_assert(offsetof(mmdeer_temporal_pool_len_args, lengths) == sizeof(mmdeer_temporal_pool_args) &&
              offsetof(mmdeer_temporal_pool_len_args, stream) == offsetof(mmdeer_temporal_pool_args, stream), "mmdeer_temporal_pool_len_args layout");

int check_seq_len(const mmdeer_lstm_seq_len_args* a, bool bwd, const char* op) {
  if (check_seq(reinterpret_cast<const mmdeer_lstm_seq_args*>(a), bwd, op) != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  MMDEER_CHECK(a->lengths && al4(a->lengths), "%s: lengths is NULL or not 4-byte aligned", op);
  return 0;
}

int check_pool_len(const mmdeer_temporal_pool_len_args* a, bool bwd, const char* op) {
  if (check_pool(reinterpret_cast<const mmdeer_temporal_pool_args*>(a), bwd, op) != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  MMDEER_CHECK(a->lengths && al4(a->lengths), "%s: lengths is NULL or not 4-byte aligned", op);
  return 0;
}

// the LEN = true instantiation of a kernel of this file, by act_f32
#define MMDEER_LAUNCH_ACT_LEN(kernel, act_f32, grid, block, stream, ...)                       \
  do {                                                                                          \
    if (act_f32) hipLaunchKernelGGL((kernel<true, true>), grid, block, 0, stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((kernel<false, true>), grid, block, 0, stream, __VA_ARGS__);        \
    MMDEER_HIP(hipGetLastError());                                                              \
  } while (0)

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_lstm_seq_pack(const float* w_hh_fwd, const float* w_hh_rev, int hidden, void* image, void* image_t, int act_f32, void* stream) {
  MMDEER_CHECK(hidden == SEQ_H, "lstm_seq_pack: hidden must be %d (got %d)", SEQ_H, hidden);
  MMDEER_CHECK(w_hh_fwd && w_hh_rev && image, "lstm_seq_pack: NULL pointer (w_hh_fwd, w_hh_rev, image)");
  const unsigned grid = 1024;
  MMDEER_LAUNCH_ACT(lstm_seq_pack_kernel, act_f32, dim3(grid), dim3(256), (hipStream_t)stream, w_hh_fwd, w_hh_rev, image, image_t);
  return 0;
}

int mmdeer_lstm_seq_fwd(const mmdeer_lstm_seq_args* a) {
  if (check_seq(a, false, "lstm_seq_fwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const int bt = a->act_f32 ? SeqCfg<true>::BT : SeqCfg<false>::BT;
  const dim3 grid((unsigned)((a->B + bt - 1) / bt), 2);
  MMDEER_LAUNCH_ACT(lstm_seq_fwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_lstm_seq_bwd(const mmdeer_lstm_seq_args* a) {
  if (check_seq(a, true, "lstm_seq_bwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const int bt = a->act_f32 ? SeqCfg<true>::BT : SeqCfg<false>::BT;
  const dim3 grid((unsigned)((a->B + bt - 1) / bt), 2);
  MMDEER_LAUNCH_ACT(lstm_seq_bwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_temporal_pool_fwd(const mmdeer_temporal_pool_args* a) {
  if (check_pool(a, false, "temporal_pool_fwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const dim3 grid((unsigned)((a->B + 3) / 4));
  MMDEER_LAUNCH_ACT(temporal_pool_fwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_temporal_pool_bwd(const mmdeer_temporal_pool_args* a) {
  if (check_pool(a, true, "temporal_pool_bwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  int nwg = (a->B + 3) / 4;
  if (nwg > POOL_BWD_WG) nwg = POOL_BWD_WG;
  MMDEER_LAUNCH_ACT(temporal_pool_bwd_kernel, a->act_f32, dim3(nwg), dim3(256), (hipStream_t)a->stream, *a);
  hipLaunchKernelGGL(fold_wg_partials_kernel<256>, dim3(1), dim3(256), 0, (hipStream_t)a->stream, a->scratch, nwg, a->dw2, a->db2);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

// ---- the same operators with per-sample lengths (include/mmdeer_seqlen.h): same grids, the LEN = true instantiations
int mmdeer_lstm_seq_len_fwd(const mmdeer_lstm_seq_len_args* a) {
  if (check_seq_len(a, false, "lstm_seq_len_fwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const int bt = a->act_f32 ? SeqCfg<true>::BT : SeqCfg<false>::BT;
  const dim3 grid((unsigned)((a->B + bt - 1) / bt), 2);
  MMDEER_LAUNCH_ACT_LEN(lstm_seq_fwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_lstm_seq_len_bwd(const mmdeer_lstm_seq_len_args* a) {
  if (check_seq_len(a, true, "lstm_seq_len_bwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const int bt = a->act_f32 ? SeqCfg<true>::BT : SeqCfg<false>::BT;
  const dim3 grid((unsigned)((a->B + bt - 1) / bt), 2);
  MMDEER_LAUNCH_ACT_LEN(lstm_seq_bwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_temporal_pool_len_fwd(const mmdeer_temporal_pool_len_args* a) {
  if (check_pool_len(a, false, "temporal_pool_len_fwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  const dim3 grid((unsigned)((a->B + 3) / 4));
  MMDEER_LAUNCH_ACT_LEN(temporal_pool_fwd_kernel, a->act_f32, grid, dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_temporal_pool_len_bwd(const mmdeer_temporal_pool_len_args* a) {
  if (check_pool_len(a, true, "temporal_pool_len_bwd") != 0) return -1;
  if (a->T == 0 || a->B == 0) return 0;
  int nwg = (a->B + 3) / 4;
  if (nwg > POOL_BWD_WG) nwg = POOL_BWD_WG;
  MMDEER_LAUNCH_ACT_LEN(temporal_pool_bwd_kernel, a->act_f32, dim3(nwg), dim3(256), (hipStream_t)a->stream, *a);
  hipLaunchKernelGGL(fold_wg_partials_kernel<256>, dim3(1), dim3(256), 0, (hipStream_t)a->stream, a->scratch, nwg, a->dw2, a->db2);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
