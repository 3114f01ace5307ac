// The BERT trunk's forward operators (include/mmdeer_bert.h; reference: transformers.BertModel as src/models/encoders.py:553-761
// instantiates it): the embedding sum + LayerNorm, masked multi-head self-attention, residual add + LayerNorm and the erf GELU.
// The trunk's Linear layers are mmdeer_gemm calls (mmdeer/bert.py).  Rows are batch-major: row b * L + t.
//
// Row LayerNorm (embed, add_ln): one wave per row of N <= 1024 columns.  Lane l owns the 4-element chunks l, l + 64, l + 128, l + 192
// that lie inside the row, keeps them in registers and makes two passes over them (mean, then the centred sum of squares), both
// summed over the wave by DPP in a fixed order.  ln_rows.h does not fit: its rows are 256 or 512 bf16 columns on 32 lanes with
// eps 1e-5 baked in, and the layer chains must keep storing its bits.
//
// Attention, bf16 (bert_attn_bf16_kernel): one workgroup of two waves per (sample, head, 64 query rows); a wave owns 32 query
// rows, its Q fragments stay in registers.  The head's K and V slices come through LDS in tiles of 128 keys: K row-major with 144-byte
// rows (18 KB; the 16-byte fragment reads of 16 lanes then fall into 16 distinct bank groups), V TRANSPOSED ([d][key], 264-byte
// rows, 16.5 KB) because the second product sums over keys.  Per block of 32 keys: S^T = K Q^T on mfma_f32_32x32x16_bf16 (A = K,
// B = Q: a lane then holds 16 scores of ONE query, the two lane halves the two halves of the block's keys), masked keys set to -inf,
// the running maximum m and sum l of the softmax in fp32, and O^T += V^T P^T with the accumulator tile of S^T as the B operand --
// registers 8 s .. 8 s + 7 converted to bf16 are the fragment of k-step s, whose element j of lane half h is key
// 16 s + 8 (j >> 2) + 4 h + (j & 3), so the V^T fragment is read in that order (two 8-byte LDS reads).  l is summed from the ROUNDED
// probabilities, so the stored row is a convex combination of V rows whatever the rounding of P.  A block without a valid key is
// skipped (a ballot: wave-uniform).  Keys past L are zero-filled in LDS and invalid; query rows past L are computed on zeros and not stored.
//
// Attention, fp32 (bert_attn_f32_kernel): parity, not speed.  One thread per query row (64 per workgroup), q and the accumulator
// in registers, K and V in tiles of 32 keys in LDS (every lane reads the same address: a broadcast), the same running softmax
// key by key.
#include <math.h>

#include "../../include/mmdeer_bert.h"
#include "elem.h"

namespace mmdeer {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BERT_HD = MMDEER_BERT_HEAD_DIM;   // 64
constexpr int AT_Q = 64;        // query rows per workgroup
constexpr int AT_K = 128;       // keys per LDS tile (bf16 kernel)
constexpr int KS_LD = 72;       // bf16 elements per K row in LDS: 64 + 8 of padding
constexpr int VT_LD = 132;      // bf16 elements per V^T row in LDS: 128 keys + 4 of padding
constexpr int AT_KF = 32;       // keys per LDS tile (fp32 kernel)

// ------------------------------------------------------------------------------------------------ row LayerNorm
// v: this lane's chunks of the row (chunk c = lane + 64 j, present while c < N / 4; absent chunks hold zeros).
template <bool F32>
__device__ __forceinline__ void bert_ln_row(const f32x4 (&v)[4], int lane, int N, const float* gamma, const float* beta, float eps,
                                            void* out, long long off) {
  const int nq = N >> 2;
  const float inv_n = 1.0f / (float)N;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  const float mu = wave_sum(s) * inv_n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (lane + 64 * j < nq) {
      const f32x4 d = v[j] - mu;
      q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
  const float rs = 1.0f / sqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = lane + 64 * j;
    if (c < nq) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c), b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
      st4<F32>(out, off + 4 * c, (v[j] - mu) * rs * g + b);
    }
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void bert_embed_kernel(mmdeer_bert_embed_args a, long long rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = a.H >> 2;
  for (long long r = (long long)blockIdx.x * 4 + w; r < rows; r += (long long)gridDim.x * 4) {
    const long long raw = a.ids[r], traw = a.type_ids ? a.type_ids[r] : 0;
    const long long id = raw < 0 ? 0 : (raw > a.V - 1 ? a.V - 1 : raw), tt = traw < 0 ? 0 : (traw > a.T - 1 ? a.T - 1 : traw);
    const long long t = r % a.L;                       // < P: the host refuses L > P
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nq)
        v[j] = (*reinterpret_cast<const f32x4*>(a.word + id * a.H + 4 * c) + *reinterpret_cast<const f32x4*>(a.type + tt * a.H + 4 * c)) +
               *reinterpret_cast<const f32x4*>(a.pos + t * a.H + 4 * c);     // HF's order: (word + type) + position
    }
    bert_ln_row<F32>(v, lane, a.H, a.gamma, a.beta, a.eps, a.x, r * a.ld_x);
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void bert_add_ln_kernel(mmdeer_bert_add_ln_args a) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = a.N >> 2;
  for (long long r = (long long)blockIdx.x * 4 + w; r < a.M; r += (long long)gridDim.x * 4) {
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nq) {
        v[j] = ld4<F32>(a.y, r * a.ld_y + 4 * c);
        if (a.x) v[j] += ld4<F32>(a.x, r * a.ld_x + 4 * c);
      }
    }
    bert_ln_row<F32>(v, lane, a.N, a.gamma, a.beta, a.eps, a.out, r * a.ld_out);
  }
}

// ------------------------------------------------------------------------------------------------ GELU
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

template <bool F32>
__global__ __launch_bounds__(256) void bert_gelu_kernel(mmdeer_bert_gelu_args a, long long chunks) {
  const int nq = a.N >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const long long r = i / nq;
    const int c = (int)(i - r * nq);
    const f32x4 v = ld4<F32>(a.x, r * a.ld_x + 4 * c);
    st4<F32>(a.out, r * a.ld_out + 4 * c, f32x4{gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w)});
  }
}

// ------------------------------------------------------------------------------------------------ attention, bf16
// grid: ((b * heads + head) * nqt + qt); 128 threads
__global__ __launch_bounds__(128) void bert_attn_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask, bf16_t* __restrict__ ctx,
                                                             int L, int H, int ld_qkv, int ld_ctx, int nqt) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_K * KS_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[BERT_HD * VT_LD];
  __shared__ __attribute__((aligned(16))) unsigned char vb[AT_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int heads = H / BERT_HD;
  const int qt = blockIdx.x % nqt, head = (blockIdx.x / nqt) % heads, b = blockIdx.x / (nqt * heads);
  const long long row0 = (long long)b * L;
  const int q = qt * AT_Q + wave * 32 + r;                    // this lane's query row (token index)
  const bool wave_live = qt * AT_Q + wave * 32 < L;           // wave-uniform: a wave without a query row only stages
  const bf16_t* kbase = qkv + row0 * ld_qkv + H + head * BERT_HD;
  const bf16_t* vbase = kbase + H;

  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 raw{0u, 0u, 0u, 0u};
    if (q < L) raw = *reinterpret_cast<const u32x4*>(qkv + (row0 + q) * ld_qkv + head * BERT_HD + 16 * ks + 8 * h);
    qf[ks] = __builtin_bit_cast(bf16x8, raw);
  }
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[0][i] = o[1][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int k0 = 0; k0 < L; k0 += AT_K) {
    if (k0) __syncthreads();                                  // the tile before has been read
    for (int i = tid; i < AT_K * 8; i += 128) {               // K: 16-byte chunk c of key `key`
      const int key = i >> 3, c = i & 7;
      u32x4 val{0u, 0u, 0u, 0u};
      if (k0 + key < L) val = *reinterpret_cast<const u32x4*>(kbase + (long long)(k0 + key) * ld_qkv + 8 * c);
      *reinterpret_cast<u32x4*>(Ks + key * KS_LD + 8 * c) = val;
    }
    for (int i = tid; i < (AT_K / 2) * 8; i += 128) {         // V^T: chunk c of the keys 2 kp and 2 kp + 1, one dword per d
      const int key = 2 * (i >> 3), c = i & 7;
      u32x4 va{0u, 0u, 0u, 0u}, vc{0u, 0u, 0u, 0u};
      if (k0 + key < L) va = *reinterpret_cast<const u32x4*>(vbase + (long long)(k0 + key) * ld_qkv + 8 * c);
      if (k0 + key + 1 < L) vc = *reinterpret_cast<const u32x4*>(vbase + (long long)(k0 + key + 1) * ld_qkv + 8 * c);
      const unsigned wa[4] = {va.x, va.y, va.z, va.w}, wc[4] = {vc.x, vc.y, vc.z, vc.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        *reinterpret_cast<unsigned*>(Vt + (8 * c + 2 * e) * VT_LD + key) = (wa[e] & 0xFFFFu) | (wc[e] << 16);
        *reinterpret_cast<unsigned*>(Vt + (8 * c + 2 * e + 1) * VT_LD + key) = (wa[e] >> 16) | (wc[e] & 0xFFFF0000u);
      }
    }
    if (tid < AT_K) vb[tid] = (k0 + tid < L && mask[row0 + k0 + tid] != 0.f) ? 1 : 0;
    __syncthreads();
    if (!wave_live) continue;

    for (int kb = 0; kb < AT_K / 32 && k0 + 32 * kb < L; ++kb) {
      // validity of this lane's 16 keys: register i is key 32 kb + (i & 3) + 8 (i >> 2) + 4 h of the tile
      unsigned vw[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) vw[g] = *reinterpret_cast<const unsigned*>(vb + 32 * kb + 8 * g + 4 * h);
      if (__builtin_amdgcn_ballot_w64((vw[0] | vw[1] | vw[2] | vw[3]) != 0u) == 0ull) continue;     // no valid key in the block
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (32 * kb + r) * KS_LD + 16 * ks + 8 * h);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
      }
      float bm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const bool valid = ((vw[i >> 2] >> (8 * (i & 3))) & 0xFFu) != 0u;
        s[i] = valid ? s[i] * 0.125f : -INFINITY;
        bm = fmaxf(bm, s[i]);
      }
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      const float m_new = fmaxf(m, bm);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;   // (a valid key has a finite score, so m_new is finite here; kept for a -inf score)
      const float alpha = __expf(m - m_ref);                  // m = -inf before the first valid key: 0, and o = l = 0
      bf16x8 pf[2];
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const __bf16 p = (__bf16)__expf(s[i] - m_ref);        // a masked key: exp(-inf) = 0 exactly
        pf[i >> 3][i & 7] = p;
        ps += (float)p;
      }
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = m_new;
#pragma unroll
      for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const bf16_t* vp = Vt + (32 * t + r) * VT_LD + 32 * kb + 16 * s2 + 4 * h;
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vp), hi = *reinterpret_cast<const u32x2*>(vp + 8);
          const bf16x8 vf = __builtin_bit_cast(bf16x8, u32x4{lo.x, lo.y, hi.x, hi.y});
          o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s2], o[t], 0, 0, 0);
        }
    }
  }
  if (wave_live && q < L) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;               // a sample without a valid key: zeros
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g)
        st4<false>(ctx, (row0 + q) * ld_ctx + head * BERT_HD + 32 * t + 8 * g + 4 * h,
                   f32x4{o[t][4 * g] * inv, o[t][4 * g + 1] * inv, o[t][4 * g + 2] * inv, o[t][4 * g + 3] * inv});
  }
}

// ------------------------------------------------------------------------------------------------ attention, fp32
// grid as above; 64 threads, thread = query row
__global__ __launch_bounds__(64) void bert_attn_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask, float* __restrict__ ctx,
                                                           int L, int H, int ld_qkv, int ld_ctx, int nqt) {
  __shared__ __attribute__((aligned(16))) float Kf[AT_KF * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Vf[AT_KF * BERT_HD];
  __shared__ float mk[AT_KF];
  const int tid = threadIdx.x;
  const int heads = H / BERT_HD;
  const int qt = blockIdx.x % nqt, head = (blockIdx.x / nqt) % heads, b = blockIdx.x / (nqt * heads);
  const long long row0 = (long long)b * L;
  const int q = qt * AT_Q + tid;
  const float* kbase = qkv + row0 * ld_qkv + H + head * BERT_HD;
  const float* vbase = kbase + H;
  f32x4 qv[16], acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    qv[c] = acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < L) qv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + q) * ld_qkv + head * BERT_HD + 4 * c) * 0.125f;   // exact: a power of two
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < L; k0 += AT_KF) {
    if (k0) __syncthreads();
    for (int i = tid; i < AT_KF * 16; i += 64) {
      const int key = i >> 4, c = i & 15;
      f32x4 kv{0.f, 0.f, 0.f, 0.f}, vv{0.f, 0.f, 0.f, 0.f};
      if (k0 + key < L) {
        kv = *reinterpret_cast<const f32x4*>(kbase + (long long)(k0 + key) * ld_qkv + 4 * c);
        vv = *reinterpret_cast<const f32x4*>(vbase + (long long)(k0 + key) * ld_qkv + 4 * c);
      }
      *reinterpret_cast<f32x4*>(Kf + key * BERT_HD + 4 * c) = kv;
      *reinterpret_cast<f32x4*>(Vf + key * BERT_HD + 4 * c) = vv;
    }
    if (tid < AT_KF) mk[tid] = k0 + tid < L ? mask[row0 + k0 + tid] : 0.f;
    __syncthreads();
    for (int key = 0; key < AT_KF; ++key) {
      if (mk[key] == 0.f) continue;                           // the same for every thread
      f32x4 d4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 16; ++c) d4 += qv[c] * *reinterpret_cast<const f32x4*>(Kf + key * BERT_HD + 4 * c);
      const float s = (d4.x + d4.y) + (d4.z + d4.w);
      const float m_new = fmaxf(m, s);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = expf(m - m_ref), p = expf(s - m_ref);
      l = l * alpha + p;
      m = m_new;
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = acc[c] * alpha + p * *reinterpret_cast<const f32x4*>(Vf + key * BERT_HD + 4 * c);
    }
  }
  if (q < L) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x4*>(ctx + (row0 + q) * ld_ctx + head * BERT_HD + 4 * c) = acc[c] * inv;
  }
}

bool finite_nonneg(float e) { return e >= 0.f && e <= 3.0e38f; }     // false for a NaN
bool hidden_ok(int H) { return H >= BERT_HD && H % BERT_HD == 0 && H <= MMDEER_BERT_MAX_HIDDEN; }
constexpr long long TWO31 = 1ll << 31;

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bert_embed_fwd(const mmdeer_bert_embed_args* a) {
  MMDEER_CHECK(a, "bert_embed_fwd: NULL args");
  MMDEER_CHECK(hidden_ok(a->H), "bert_embed_fwd: unsupported H = %d (a multiple of 64, 64 .. %d)", a->H, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->B >= 0 && a->L >= 0 && a->V >= 1 && a->P >= 1 && a->T >= 1, "bert_embed_fwd: bad shape (B %d, L %d, V %d, P %d, T %d)", a->B,
               a->L, a->V, a->P, a->T);
  MMDEER_CHECK(a->L <= a->P, "bert_embed_fwd: L = %d is above max_position_embeddings P = %d", a->L, a->P);
  MMDEER_CHECK(a->ld_x >= a->H && a->ld_x % 4 == 0, "bert_embed_fwd: bad leading dimension ld_x = %d (>= H, a multiple of 4)", a->ld_x);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_embed_fwd: eps must be finite and >= 0");
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(rows * a->ld_x < TWO31, "bert_embed_fwd: x has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->ids && a->word && a->pos && a->type && a->gamma && a->beta && a->x,
               "bert_embed_fwd: NULL pointer (ids, word, pos, type, gamma, beta, x)");
  MMDEER_CHECK(al8(a->ids) && al8(a->type_ids) && al16(a->word) && al16(a->pos) && al16(a->type) && al16(a->gamma) && al16(a->beta) &&
                   al_act4(a->act_f32, {a->x}),
               "bert_embed_fwd: misaligned pointer (ids 8 bytes; tables, gamma, beta 16 bytes; x 4 act elements)");
  const unsigned grid = (unsigned)((rows + 3) / 4 < 65536 ? (rows + 3) / 4 : 65536);
  MMDEER_LAUNCH_ACT(bert_embed_kernel, a->act_f32, dim3(grid), dim3(256), (hipStream_t)a->stream, *a, rows);
  return 0;
}

int mmdeer_bert_attn_fwd(const mmdeer_bert_attn_args* a) {
  MMDEER_CHECK(a, "bert_attn_fwd: NULL args");
  MMDEER_CHECK(hidden_ok(a->H), "bert_attn_fwd: unsupported H = %d (a multiple of 64, 64 .. %d)", a->H, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->B >= 0 && a->L >= 0 && (a->L >= 1 || a->B == 0), "bert_attn_fwd: bad shape (B %d, L %d: L >= 1 with B > 0)", a->B, a->L);
  MMDEER_CHECK(a->L <= MMDEER_BERT_MAX_TOKENS, "bert_attn_fwd: L = %d is above %d tokens", a->L, MMDEER_BERT_MAX_TOKENS);
  MMDEER_CHECK(a->ld_qkv >= 3 * a->H && a->ld_qkv % 8 == 0, "bert_attn_fwd: bad leading dimension ld_qkv = %d (>= 3 H, a multiple of 8)", a->ld_qkv);
  MMDEER_CHECK(a->ld_ctx >= a->H && a->ld_ctx % 4 == 0, "bert_attn_fwd: bad leading dimension ld_ctx = %d (>= H, a multiple of 4)", a->ld_ctx);
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(rows * a->ld_qkv < TWO31 && rows * a->ld_ctx < TWO31, "bert_attn_fwd: qkv or ctx has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->qkv && a->mask && a->ctx, "bert_attn_fwd: NULL pointer (qkv, mask, ctx)");
  MMDEER_CHECK(al16(a->qkv) && al4(a->mask) && al_act4(a->act_f32, {a->ctx}),
               "bert_attn_fwd: misaligned pointer (qkv 16 bytes, mask 4 bytes, ctx 4 act elements)");
  const int nqt = (a->L + AT_Q - 1) / AT_Q;
  const unsigned grid = (unsigned)((long long)a->B * (a->H / BERT_HD) * nqt);     // < 2^31 / 192
  if (a->act_f32)
    hipLaunchKernelGGL(bert_attn_f32_kernel, dim3(grid), dim3(64), 0, (hipStream_t)a->stream, (const float*)a->qkv, a->mask, (float*)a->ctx, a->L,
                       a->H, a->ld_qkv, a->ld_ctx, nqt);
  else
    hipLaunchKernelGGL(bert_attn_bf16_kernel, dim3(grid), dim3(128), 0, (hipStream_t)a->stream, (const bf16_t*)a->qkv, a->mask, (bf16_t*)a->ctx,
                       a->L, a->H, a->ld_qkv, a->ld_ctx, nqt);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_bert_add_ln_fwd(const mmdeer_bert_add_ln_args* a) {
  MMDEER_CHECK(a, "bert_add_ln_fwd: NULL args");
  MMDEER_CHECK(a->N >= 4 && a->N % 4 == 0 && a->N <= MMDEER_BERT_MAX_HIDDEN, "bert_add_ln_fwd: unsupported N = %d (a multiple of 4, 4 .. %d)", a->N,
               MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->M >= 0, "bert_add_ln_fwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(a->ld_y >= a->N && a->ld_y % 4 == 0 && a->ld_out >= a->N && a->ld_out % 4 == 0 && (!a->x || (a->ld_x >= a->N && a->ld_x % 4 == 0)),
               "bert_add_ln_fwd: bad leading dimension (ld_y %d, ld_x %d, ld_out %d: >= N, multiples of 4)", a->ld_y, a->ld_x, a->ld_out);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_add_ln_fwd: eps must be finite and >= 0");
  MMDEER_CHECK((long long)a->M * a->ld_y < TWO31 && (long long)a->M * a->ld_out < TWO31 && (!a->x || (long long)a->M * a->ld_x < TWO31),
               "bert_add_ln_fwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->y && a->gamma && a->beta && a->out, "bert_add_ln_fwd: NULL pointer (y, gamma, beta, out)");
  MMDEER_CHECK(al16(a->gamma) && al16(a->beta) && al_act4(a->act_f32, {a->y, a->x, a->out}),
               "bert_add_ln_fwd: misaligned pointer (gamma, beta 16 bytes; y, x, out 4 act elements)");
  const unsigned grid = (unsigned)((a->M + 3) / 4 < 65536 ? (a->M + 3) / 4 : 65536);
  MMDEER_LAUNCH_ACT(bert_add_ln_kernel, a->act_f32, dim3(grid), dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_bert_gelu_fwd(const mmdeer_bert_gelu_args* a) {
  MMDEER_CHECK(a, "bert_gelu_fwd: NULL args");
  MMDEER_CHECK(a->N >= 4 && a->N % 4 == 0, "bert_gelu_fwd: unsupported N = %d (a multiple of 4)", a->N);
  MMDEER_CHECK(a->M >= 0, "bert_gelu_fwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(a->ld_x >= a->N && a->ld_x % 4 == 0 && a->ld_out >= a->N && a->ld_out % 4 == 0,
               "bert_gelu_fwd: bad leading dimension (ld_x %d, ld_out %d: >= N, multiples of 4)", a->ld_x, a->ld_out);
  MMDEER_CHECK((long long)a->M * a->ld_x < TWO31 && (long long)a->M * a->ld_out < TWO31, "bert_gelu_fwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->x && a->out, "bert_gelu_fwd: NULL pointer (x, out)");
  MMDEER_CHECK(al_act4(a->act_f32, {a->x, a->out}), "bert_gelu_fwd: misaligned pointer (x, out: 4 act elements)");
  const long long chunks = (long long)a->M * (a->N / 4);
  const unsigned grid = (unsigned)((chunks + 255) / 256 < 16384 ? (chunks + 255) / 256 : 16384);
  MMDEER_LAUNCH_ACT(bert_gelu_kernel, a->act_f32, dim3(grid), dim3(256), (hipStream_t)a->stream, *a, chunks);
  return 0;
}

}  // extern "C"
