// The BERT trunk's operators with their dropout sites inside (include/mmdeer_bert_drop.h; reference: transformers.BertModel in
// train() with hidden_dropout_prob and attention_probs_dropout_prob): the embedding LayerNorm, the attention forward and its two
// backward launches, and the residual add + LayerNorm pair.  Separate kernels on bert_dev.h's tiles, fragments and row layout, so
// that bert.hip and bert_bwd.hip are compiled from the text they had: the plain entries keep their code and their bits.
//
// The mask is common.h's counter hash: element (row, col) of a site is kept iff mix32(rk ^ (col * 0x85EBCA77u)) < thresh with the row
// key rk = (row * 0x9E3779B1u) ^ drop_key(seed, offset, site); m = keep * scale.  Regenerated wherever it is needed, never stored.
//   hidden sites     row = the operand's row b * L + t, col = the column n; four columns at a time through drop4 (no shift)
//   attention site   row = (b * heads + head) * L + query, col = key.  In the bf16 forward and dq kernels a lane holds 16 keys of ONE
//                    query: rk is a per-lane scalar and an element costs one mix32.  In dkdv a lane holds 16 queries of ONE key:
//                    the column term is the per-lane scalar.
// Attention applies keep alone to the operands and the factor 1 / (1 - p) in fp32 to the accumulators (the header has the algebra):
// the softmax sum l and the log-sum-exp are those of the undropped probabilities.
//
// The key is formed ON THE DEVICE, once per wave before its first element: every kernel takes the DropCtx and the site and calls
// common.h's drop_key, whose operands are kernel arguments and -- where the context carries offset_dev -- one 64-bit word behind a
// uniform pointer: a scalar load and four mix32 in scalar registers.  The plain entries are the NULL-counter case of the same kernels.
// No kernel of this file writes the counter.
#include "../../include/mmdeer_bert_drop.h"
#include "../../include/mmdeer_graph.h"

#include "../../include/mmdeer_bert_bwd.h"
#include "bert_dev.h"

namespace mmdeer {
namespace {

constexpr int DF_LD = 68;       // floats per dO row in LDS of the fp32 dq kernel (bert_bwd.hip's)
constexpr int LN_PARTS = MMDEER_BERT_LN_BWD_PARTS;

__device__ __forceinline__ unsigned row_key(unsigned row, unsigned key) { return (row * 0x9E3779B1u) ^ key; }
__device__ __forceinline__ bool kept(unsigned rk, unsigned col, unsigned thresh) { return mix32(rk ^ (col * 0x85EBCA77u)) < thresh; }

// ------------------------------------------------------------------------------------------------ row LayerNorm
// bert.hip's bert_ln_row; DROP: the stored value is the normalised one times m of (row key rk, column)
template <bool F32, bool DROP>
__device__ __forceinline__ void ln_row(const f32x4 (&v)[4], int lane, int N, const float* gamma, const float* beta, float eps, void* out,
                                       long long off, unsigned rk, const DropCtx& dc) {
  const int nq = N >> 2;
  const float inv_n = 1.0f / (float)N;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  const float mu = wave_sum(s) * inv_n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ln_chunk(lane, j) < nq) {
      const f32x4 d = v[j] - mu;
      q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
    }
  const float rs = 1.0f / sqrtf(wave_sum(q) * inv_n + eps);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = ln_chunk(lane, j);
    if (c < nq) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c), b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
      f32x4 o = (v[j] - mu) * rs * g + b;
      if constexpr (DROP) o = drop4(o, rk, 4u * c, 0, dc);
      st4<F32>(out, off + 4 * c, o);
    }
  }
}

// v = this lane's chunks of drop(row y) (+ row x, where x is given)
template <bool F32>
__device__ __forceinline__ void ln_load_drop(f32x4 (&v)[4], const void* y, long long oy, const void* x, long long ox, int lane, int nq, unsigned rk,
                                             const DropCtx& dc) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = ln_chunk(lane, j);
    v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (c < nq) {
      v[j] = drop4(ld4<F32>(y, oy + 4 * c), rk, 4u * c, 0, dc);
      if (x) v[j] += ld4<F32>(x, ox + 4 * c);
    }
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void bert_embed_drop_kernel(mmdeer_bert_embed_drop_args a, long long rows, DropCtx dc) {
  const unsigned key = drop_key(dc, a.site);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = a.H >> 2;
  for (long long r = (long long)blockIdx.x * 4 + w; r < rows; r += (long long)gridDim.x * 4) {
    const long long raw = a.ids[r], traw = a.type_ids ? a.type_ids[r] : 0;
    const long long id = raw < 0 ? 0 : (raw > a.V - 1 ? a.V - 1 : raw), tt = traw < 0 ? 0 : (traw > a.T - 1 ? a.T - 1 : traw);
    const long long t = r % a.L;                       // < P: the host refuses L > P
    f32x4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = ln_chunk(lane, j);
      v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c < nq)
        v[j] = (*reinterpret_cast<const f32x4*>(a.word + id * a.H + 4 * c) + *reinterpret_cast<const f32x4*>(a.type + tt * a.H + 4 * c)) +
               *reinterpret_cast<const f32x4*>(a.pos + t * a.H + 4 * c);     // HF's order: (word + type) + position
    }
    ln_row<F32, true>(v, lane, a.H, a.gamma, a.beta, a.eps, a.x, r * a.ld_x, row_key((unsigned)r, key), dc);
  }
}

template <bool F32>
__global__ __launch_bounds__(256) void bert_drop_add_ln_kernel(mmdeer_bert_drop_add_ln_args a, DropCtx dc) {
  const unsigned key = drop_key(dc, a.site);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * 4 + w; r < a.M; r += (long long)gridDim.x * 4) {
    f32x4 v[4];
    ln_load_drop<F32>(v, a.y, r * a.ld_y, a.x, r * a.ld_x, lane, a.N >> 2, row_key((unsigned)r, key), dc);
    ln_row<F32, false>(v, lane, a.N, a.gamma, a.beta, a.eps, a.out, r * a.ld_out, 0u, dc);
  }
}

// ------------------------------------------------------------------------------------------------ attention forward, bf16
// bert.hip's bert_attn_bf16_kernel with the keep decision on the operand of the second product.  grid, threads and LDS are its.
__global__ __launch_bounds__(128) void bert_attn_drop_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask,
                                                                  bf16_t* __restrict__ ctx, int L, int H, int ld_qkv, int ld_ctx, int nqt,
                                                                  DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_K * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[BERT_HD * KT_LD];
  __shared__ __attribute__((aligned(16))) unsigned char vb[AT_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + wave * 32 + r;             // this lane's query row (token index)
  const bool wave_live = blk.tile * AT_OWN + wave * 32 < L;    // wave-uniform: a wave without a query row only stages
  const bool live = q < L;
  const unsigned rk = row_key((unsigned)((blk.b * heads + blk.head) * L + q), key);
  const bf16_t* kbase = qkv + row0 * ld_qkv + H + blk.head * BERT_HD;
  const bf16_t* vbase = kbase + H;

  bf16x8 qf[4];
  load_row_frags(qf, qkv + (row0 + (live ? q : 0)) * ld_qkv + blk.head * BERT_HD, live, h);
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[0][i] = o[1][i] = 0.f;
  float m = -INFINITY, l = 0.f;

  for (int k0 = 0; k0 < L; k0 += AT_K) {
    if (k0) __syncthreads();                                  // the tile before has been read
    stage_rows(Ks, kbase, ld_qkv, k0, AT_K, L, tid);
    stage_transposed(Vt, KT_LD, vbase, ld_qkv, k0, AT_K, L, tid);
    stage_valid(vb, mask + row0, k0, L, tid);
    __syncthreads();
    if (!wave_live) continue;

    for (int kb = 0; kb < AT_K / 32 && k0 + 32 * kb < L; ++kb) {
      unsigned vw[4];
      load_valid(vw, vb, kb, h);
      if (none_valid(vw)) continue;
      f32x16 s;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (32 * kb + r) * ROW_LD + 16 * ks + 8 * h);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
      }
      float bm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s[i] = key_valid(vw, i) ? s[i] * 0.125f : -INFINITY;
        bm = fmaxf(bm, s[i]);
      }
      bm = fmaxf(bm, __shfl_xor(bm, 32));
      const float m_new = fmaxf(m, bm);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __expf(m - m_ref);                  // m = -inf before the first valid key: 0, and o = l = 0
      const unsigned j0 = (unsigned)(k0 + 32 * kb + 4 * h);   // register i is key j0 + (i & 3) + 8 (i >> 2)
      bf16x8 pf[2];
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const __bf16 p = (__bf16)__expf(s[i] - m_ref);        // a masked key: exp(-inf) = 0 exactly
        ps += (float)p;                                       // l: over the undropped, rounded probabilities
        pf[i >> 3][i & 7] = kept(rk, j0 + (i & 3) + 8 * (i >> 2), thresh) ? p : (__bf16)0.f;
      }
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = m_new;
#pragma unroll
      for (int i = 0; i < 16; ++i) { o[0][i] *= alpha; o[1][i] *= alpha; }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t(Vt + (32 * t + r) * KT_LD + 32 * kb + 16 * s2 + 4 * h), pf[s2], o[t], 0, 0, 0);
    }
  }
  // no valid key, or every valid key dropped: zeros
  if (wave_live && live) store_tile(ctx, (row0 + q) * ld_ctx + blk.head * BERT_HD, o, h, l > 0.f ? scale / l : 0.f);
}

// ------------------------------------------------------------------------------------------------ attention forward, fp32
__global__ __launch_bounds__(64) void bert_attn_drop_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask, float* __restrict__ ctx,
                                                                int L, int H, int ld_qkv, int ld_ctx, int nqt, DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) float Kf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Vf[AT_F * BERT_HD];
  __shared__ float mk[AT_F];
  const int tid = threadIdx.x;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + tid;
  const unsigned rk = row_key((unsigned)((blk.b * heads + blk.head) * L + q), key);
  const float* kbase = qkv + row0 * ld_qkv + H + blk.head * BERT_HD;
  const float* vbase = kbase + H;
  f32x4 qv[16], acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    qv[c] = acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q < L) qv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + q) * ld_qkv + blk.head * BERT_HD + 4 * c) * 0.125f;   // exact: a power of two
  }
  float m = -INFINITY, l = 0.f;
  for (int k0 = 0; k0 < L; k0 += AT_F) {
    if (k0) __syncthreads();
    stage_rows_f32(Kf, kbase, ld_qkv, Vf, vbase, ld_qkv, k0, L, tid);
    if (tid < AT_F) mk[tid] = k0 + tid < L ? mask[row0 + k0 + tid] : 0.f;
    __syncthreads();
    for (int kk = 0; kk < AT_F; ++kk) {
      if (mk[kk] == 0.f) continue;                            // the same for every thread
      f32x4 d4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 16; ++c) d4 += qv[c] * *reinterpret_cast<const f32x4*>(Kf + kk * BERT_HD + 4 * c);
      const float s = (d4.x + d4.y) + (d4.z + d4.w);
      const float m_new = fmaxf(m, s);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = expf(m - m_ref), p = expf(s - m_ref);
      l = l * alpha + p;                                      // over the undropped probabilities
      m = m_new;
      const float pk = kept(rk, (unsigned)(k0 + kk), thresh) ? p : 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) acc[c] = acc[c] * alpha + pk * *reinterpret_cast<const f32x4*>(Vf + kk * BERT_HD + 4 * c);
    }
  }
  if (q < L) {
    const float inv = l > 0.f ? scale / l : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x4*>(ctx + (row0 + q) * ld_ctx + blk.head * BERT_HD + 4 * c) = acc[c] * inv;
  }
}

// ------------------------------------------------------------------------------------------------ attention backward, bf16: dQ
// bert_bwd.hip's bert_attn_dq_bf16_kernel with keep on dP: pass 0 sums delta' = sum P k dP, pass 1 forms P (k dP - delta'), and the
// factor 1 / (1 - p) goes on the accumulator with the 1 / 8.  ws: lse [B * heads * L], then delta'.
__global__ __launch_bounds__(128) void bert_attn_drop_dq_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask,
                                                                     const bf16_t* __restrict__ dctx, bf16_t* __restrict__ dqkv,
                                                                     float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx,
                                                                     int ld_dqkv, int nqt, long long nstat, DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_K * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vs[AT_K * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Kt[BERT_HD * KT_LD];
  __shared__ __attribute__((aligned(16))) unsigned char vb[AT_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + wave * 32 + r;                      // this lane's query row
  const bool wave_live = blk.tile * AT_OWN + wave * 32 < L;             // wave-uniform: a wave without a query row only stages
  const bool live = q < L;
  const unsigned rk = row_key((unsigned)((blk.b * heads + blk.head) * L + q), key);
  const bf16_t* kbase = qkv + row0 * ld_qkv + H + blk.head * BERT_HD;
  const bf16_t* vbase = kbase + H;

  bf16x8 qf[4], dof[4];
  load_row_frags(qf, qkv + (row0 + (live ? q : 0)) * ld_qkv + blk.head * BERT_HD, live, h);
  load_row_frags(dof, dctx + (row0 + (live ? q : 0)) * ld_dctx + blk.head * BERT_HD, live, h);
  f32x16 o[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) o[0][i] = o[1][i] = 0.f;
  float m = -INFINITY, l = 0.f, dacc = 0.f, lse = INFINITY, delta = 0.f;

  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < L; k0 += AT_K) {
      __syncthreads();                                        // the tile before has been read
      stage_rows(Ks, kbase, ld_qkv, k0, AT_K, L, tid);
      stage_rows(Vs, vbase, ld_qkv, k0, AT_K, L, tid);
      if (pass) stage_transposed(Kt, KT_LD, kbase, ld_qkv, k0, AT_K, L, tid);
      stage_valid(vb, mask + row0, k0, L, tid);
      __syncthreads();
      if (!wave_live) continue;
      for (int kb = 0; kb < AT_K / 32 && k0 + 32 * kb < L; ++kb) {
        unsigned vw[4];
        load_valid(vw, vb, kb, h);
        if (none_valid(vw)) continue;
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (32 * kb + r) * ROW_LD + 16 * ks + 8 * h);
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(Vs + (32 * kb + r) * ROW_LD + 16 * ks + 8 * h);
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, dof[ks], dp, 0, 0, 0);
        }
        const unsigned j0 = (unsigned)(k0 + 32 * kb + 4 * h);            // register i is key j0 + (i & 3) + 8 (i >> 2)
#pragma unroll
        for (int i = 0; i < 16; ++i) dp[i] = kept(rk, j0 + (i & 3) + 8 * (i >> 2), thresh) ? dp[i] : 0.f;      // k o dP, the same in both passes
        if (pass == 0) {
          float bm = -INFINITY;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            s[i] = key_valid(vw, i) ? s[i] * 0.125f : -INFINITY;
            bm = fmaxf(bm, s[i]);
          }
          bm = fmaxf(bm, __shfl_xor(bm, 32));
          const float m_new = fmaxf(m, bm);
          const float m_ref = m_new == -INFINITY ? 0.f : m_new;
          float ps = 0.f, pd = 0.f;
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float e = __expf(s[i] - m_ref);                        // a masked key: exp(-inf) = 0 exactly
            ps += e;
            pd = fmaf(e, dp[i], pd);
          }
          ps += __shfl_xor(ps, 32);
          pd += __shfl_xor(pd, 32);
          const float alpha = __expf(m - m_ref);                         // m = -inf before the first valid key: 0, and l = dacc = 0
          l = l * alpha + ps;
          dacc = dacc * alpha + pd;
          m = m_new;
        } else {
          bf16x8 dsf[2];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const float p = key_valid(vw, i) ? __expf(s[i] * 0.125f - lse) : 0.f;   // lse = +inf (no valid key): 0
            dsf[i >> 3][i & 7] = (__bf16)(p * (dp[i] - delta));
          }
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int t = 0; t < 2; ++t)
              o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t(Kt + (32 * t + r) * KT_LD + 32 * kb + 16 * s2 + 4 * h), dsf[s2], o[t], 0, 0, 0);
        }
      }
    }
    if (pass == 0) {
      lse = l > 0.f ? m + __logf(l) : INFINITY;
      delta = l > 0.f ? dacc / l : 0.f;
      if (live && h == 0) {
        const long long at = ((long long)blk.b * heads + blk.head) * L + q;
        ws[at] = lse;
        ws[nstat + at] = delta;
      }
    }
  }
  if (wave_live && live) store_tile(dqkv, (row0 + q) * ld_dqkv + blk.head * BERT_HD, o, h, 0.125f * scale);
}

// ------------------------------------------------------------------------------------------------ attention backward, bf16: dK, dV
// bert_bwd.hip's bert_attn_dkdv_bf16_kernel: a lane holds 16 queries of ONE key, so the column term of the hash is the lane's scalar
__global__ __launch_bounds__(128) void bert_attn_drop_dkdv_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask,
                                                                       const bf16_t* __restrict__ dctx, bf16_t* __restrict__ dqkv,
                                                                       const float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx,
                                                                       int ld_dqkv, int nkt, long long nstat, DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) bf16_t Qs[AT_Q * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Os[AT_Q * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[BERT_HD * QT_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Ot[BERT_HD * QT_LD];
  __shared__ __attribute__((aligned(16))) float lse_s[AT_Q];
  __shared__ __attribute__((aligned(16))) float del_s[AT_Q];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nkt);
  const long long row0 = (long long)blk.b * L;
  const int kcol = blk.tile * AT_OWN + wave * 32 + r;                   // this lane's key
  const bool live = kcol < L;
  const bool valid = live && mask[row0 + (live ? kcol : 0)] != 0.f;
  const bool wave_work = __builtin_amdgcn_ballot_w64(valid) != 0ull;      // wave-uniform: a wave without a valid key only stages
  const unsigned ck = ((unsigned)kcol * 0x85EBCA77u) ^ key;             // the column's share of the hash
  const unsigned qrow0 = (unsigned)((blk.b * heads + blk.head) * L);    // the mask row of query 0
  const bf16_t* qbase = qkv + row0 * ld_qkv + blk.head * BERT_HD;
  const bf16_t* obase = dctx + row0 * ld_dctx + blk.head * BERT_HD;
  const float* lse_g = ws + ((long long)blk.b * heads + blk.head) * L;

  bf16x8 kf[4], vf[4];
  load_row_frags(kf, qkv + (row0 + (live ? kcol : 0)) * ld_qkv + H + blk.head * BERT_HD, live, h);
  load_row_frags(vf, qkv + (row0 + (live ? kcol : 0)) * ld_qkv + 2 * H + blk.head * BERT_HD, live, h);
  f32x16 dk[2], dv[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) dk[0][i] = dk[1][i] = dv[0][i] = dv[1][i] = 0.f;

  for (int q0 = 0; q0 < L; q0 += AT_Q) {
    __syncthreads();                                          // the tile before has been read
    stage_rows(Qs, qbase, ld_qkv, q0, AT_Q, L, tid);
    stage_rows(Os, obase, ld_dctx, q0, AT_Q, L, tid);
    stage_transposed(Qt, QT_LD, qbase, ld_qkv, q0, AT_Q, L, tid);
    stage_transposed(Ot, QT_LD, obase, ld_dctx, q0, AT_Q, L, tid);
    if (tid < AT_Q) {
      const bool in = q0 + tid < L;
      lse_s[tid] = in ? lse_g[q0 + tid] : INFINITY;           // a query past L: P = 0
      del_s[tid] = in ? lse_g[nstat + q0 + tid] : 0.f;
    }
    __syncthreads();
    if (!wave_work) continue;
    for (int qb = 0; qb < AT_Q / 32 && q0 + 32 * qb < L; ++qb) {
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = dp[i] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const bf16x8 qa = *reinterpret_cast<const bf16x8*>(Qs + (32 * qb + r) * ROW_LD + 16 * ks + 8 * h);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa, kf[ks], s, 0, 0, 0);
        const bf16x8 oa = *reinterpret_cast<const bf16x8*>(Os + (32 * qb + r) * ROW_LD + 16 * ks + 8 * h);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa, vf[ks], dp, 0, 0, 0);
      }
      // register i is query 32 qb + (i & 3) + 8 (i >> 2) + 4 h of the tile
      const unsigned qr = qrow0 + (unsigned)(q0 + 32 * qb + 4 * h);
      bf16x8 pf[2], dsf[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 ls = *reinterpret_cast<const f32x4*>(lse_s + 32 * qb + 8 * g + 4 * h);
        const f32x4 dl = *reinterpret_cast<const f32x4*>(del_s + 32 * qb + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          const bool k = mix32(((qr + 8 * g + e) * 0x9E3779B1u) ^ ck) < thresh;
          const float p = valid ? __expf(s[i] * 0.125f - ls[e]) : 0.f;
          pf[i >> 3][i & 7] = (__bf16)(k ? p : 0.f);
          dsf[i >> 3][i & 7] = (__bf16)(p * ((k ? dp[i] : 0.f) - dl[e]));
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          dv[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t(Ot + (32 * t + r) * QT_LD + 32 * qb + 16 * s2 + 4 * h), pf[s2], dv[t], 0, 0, 0);
          dk[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t(Qt + (32 * t + r) * QT_LD + 32 * qb + 16 * s2 + 4 * h), dsf[s2], dk[t], 0, 0, 0);
        }
    }
  }
  if (live) {
    store_tile(dqkv, (row0 + kcol) * ld_dqkv + H + blk.head * BERT_HD, dk, h, 0.125f * scale);
    store_tile(dqkv, (row0 + kcol) * ld_dqkv + 2 * H + blk.head * BERT_HD, dv, h, scale);
  }
}

// ------------------------------------------------------------------------------------------------ attention backward, fp32
// bert_bwd.hip's two fp32 kernels with the same keep decisions and the factor on the stored rows
__global__ __launch_bounds__(64) void bert_attn_drop_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask,
                                                                   const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                   float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx, int ld_dqkv,
                                                                   int nqt, long long nstat, DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) float Kf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Vf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Df[AT_OWN * DF_LD];      // thread t's dO row at t * DF_LD: read by its owner alone
  __shared__ float mk[AT_F];
  const int tid = threadIdx.x;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + tid;
  const bool live = q < L;
  const unsigned rk = row_key((unsigned)((blk.b * heads + blk.head) * L + q), key);
  const float* kbase = qkv + row0 * ld_qkv + H + blk.head * BERT_HD;
  const float* vbase = kbase + H;
  f32x4 qv[16], acc[16];
  float* dov = Df + tid * DF_LD;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    f32x4 d{0.f, 0.f, 0.f, 0.f};
    qv[c] = acc[c] = d;
    if (live) {
      qv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + q) * ld_qkv + blk.head * BERT_HD + 4 * c) * 0.125f;     // exact: a power of two
      d = *reinterpret_cast<const f32x4*>(dctx + (row0 + q) * ld_dctx + blk.head * BERT_HD + 4 * c);
    }
    *reinterpret_cast<f32x4*>(dov + 4 * c) = d;
  }
  float m = -INFINITY, l = 0.f, dacc = 0.f, lse = INFINITY, delta = 0.f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int k0 = 0; k0 < L; k0 += AT_F) {
      __syncthreads();
      stage_rows_f32(Kf, kbase, ld_qkv, Vf, vbase, ld_qkv, k0, L, tid);
      if (tid < AT_F) mk[tid] = k0 + tid < L ? mask[row0 + k0 + tid] : 0.f;
      __syncthreads();
      for (int kk = 0; kk < AT_F; ++kk) {
        if (mk[kk] == 0.f) continue;                          // the same for every thread
        f32x4 d4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) d4 += qv[c] * *reinterpret_cast<const f32x4*>(Kf + kk * BERT_HD + 4 * c);
        const float s = (d4.x + d4.y) + (d4.z + d4.w);
        f32x4 e4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) e4 += *reinterpret_cast<const f32x4*>(dov + 4 * c) * *reinterpret_cast<const f32x4*>(Vf + kk * BERT_HD + 4 * c);
        const float dpr = (e4.x + e4.y) + (e4.z + e4.w);
        // the hash behind both dot products, where few registers are live: scheduled among their LDS reads it cost two VGPRs parked
        // in AGPRs at 256; behind this barrier the kernel has 228 and parks none
        __builtin_amdgcn_sched_barrier(0);
        const float dp = kept(rk, (unsigned)(k0 + kk), thresh) ? dpr : 0.f;       // k dP, the same in both passes
        if (pass == 0) {
          const float m_new = fmaxf(m, s);                    // s is finite, so m_new is
          const float alpha = expf(m - m_new), e = expf(s - m_new);
          l = l * alpha + e;
          dacc = fmaf(e, dp, dacc * alpha);
          m = m_new;
        } else {
          const float ds = expf(s - lse) * (dp - delta);
#pragma unroll
          for (int c = 0; c < 16; ++c) acc[c] += ds * *reinterpret_cast<const f32x4*>(Kf + kk * BERT_HD + 4 * c);
        }
      }
    }
    if (pass == 0) {
      lse = l > 0.f ? m + logf(l) : INFINITY;
      delta = l > 0.f ? dacc / l : 0.f;
      if (live) {
        const long long at = ((long long)blk.b * heads + blk.head) * L + q;
        ws[at] = lse;
        ws[nstat + at] = delta;
      }
    }
  }
  if (live) {
    const float f = 0.125f * scale;
#pragma unroll
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x4*>(dqkv + (row0 + q) * ld_dqkv + blk.head * BERT_HD + 4 * c) = acc[c] * f;
  }
}

__global__ __launch_bounds__(64) void bert_attn_drop_dkdv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask,
                                                                     const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                     const float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx,
                                                                     int ld_dqkv, int nkt, long long nstat, DropCtx dc, int site) {
  const unsigned key = drop_key(dc, site), thresh = dc.thresh;
  const float scale = dc.scale;
  __shared__ __attribute__((aligned(16))) float Qf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Of[AT_F * BERT_HD];
  __shared__ float lse_s[AT_F];
  __shared__ float del_s[AT_F];
  const int tid = threadIdx.x;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nkt);
  const long long row0 = (long long)blk.b * L;
  const int kcol = blk.tile * AT_OWN + tid;
  const bool live = kcol < L;
  const bool valid = live && mask[row0 + (live ? kcol : 0)] != 0.f;
  const unsigned ck = ((unsigned)kcol * 0x85EBCA77u) ^ key;
  const unsigned qrow0 = (unsigned)((blk.b * heads + blk.head) * L);
  const float* qbase = qkv + row0 * ld_qkv + blk.head * BERT_HD;
  const float* obase = dctx + row0 * ld_dctx + blk.head * BERT_HD;
  const float* lse_g = ws + ((long long)blk.b * heads + blk.head) * L;
  f32x4 kv[16], vv[16], dk[16], dv[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    kv[c] = vv[c] = dk[c] = dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
      kv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + kcol) * ld_qkv + H + blk.head * BERT_HD + 4 * c) * 0.125f;
      vv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + kcol) * ld_qkv + 2 * H + blk.head * BERT_HD + 4 * c);
    }
  }
  for (int q0 = 0; q0 < L; q0 += AT_F) {
    __syncthreads();
    stage_rows_f32(Qf, qbase, ld_qkv, Of, obase, ld_dctx, q0, L, tid);
    if (tid < AT_F) {
      const bool in = q0 + tid < L;
      lse_s[tid] = in ? lse_g[q0 + tid] : INFINITY;
      del_s[tid] = in ? lse_g[nstat + q0 + tid] : 0.f;
    }
    __syncthreads();
    const int nq = L - q0 < AT_F ? L - q0 : AT_F;
    for (int qi = 0; qi < nq; ++qi) {
      const float ls = lse_s[qi];
      if (ls == INFINITY) continue;                           // the same for every thread: a sample without a valid key
      f32x4 d4{0.f, 0.f, 0.f, 0.f}, e4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        d4 += kv[c] * *reinterpret_cast<const f32x4*>(Qf + qi * BERT_HD + 4 * c);
        e4 += vv[c] * *reinterpret_cast<const f32x4*>(Of + qi * BERT_HD + 4 * c);
      }
      const bool k = mix32(((qrow0 + (unsigned)(q0 + qi)) * 0x9E3779B1u) ^ ck) < thresh;
      const float p = valid ? expf(((d4.x + d4.y) + (d4.z + d4.w)) - ls) : 0.f;
      const float ds = p * ((k ? (e4.x + e4.y) + (e4.z + e4.w) : 0.f) - del_s[qi]);
      const float pk = k ? p : 0.f;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        dv[c] += pk * *reinterpret_cast<const f32x4*>(Of + qi * BERT_HD + 4 * c);
        dk[c] += ds * *reinterpret_cast<const f32x4*>(Qf + qi * BERT_HD + 4 * c);
      }
    }
  }
  if (live) {
    const float f = 0.125f * scale;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      *reinterpret_cast<f32x4*>(dqkv + (row0 + kcol) * ld_dqkv + H + blk.head * BERT_HD + 4 * c) = dk[c] * f;
      *reinterpret_cast<f32x4*>(dqkv + (row0 + kcol) * ld_dqkv + 2 * H + blk.head * BERT_HD + 4 * c) = dv[c] * scale;
    }
  }
}

// ------------------------------------------------------------------------------------------------ drop + add + LayerNorm backward
// bert_bwd.hip's bert_add_ln_bwd_kernel on s = drop(y) + x, with the second store dy = ds o m; the partial sums and
// bert_ln_fold_kernel's fixed order are restated here because that kernel is local to its file.
template <bool F32>
__global__ __launch_bounds__(256) void bert_drop_add_ln_bwd_kernel(mmdeer_bert_drop_add_ln_bwd_args a, int sums, DropCtx dc) {
  const unsigned key = drop_key(dc, a.site);
  __shared__ __attribute__((aligned(16))) float part[3][2 * MMDEER_BERT_MAX_HIDDEN];      // waves 1 .. 3: [dgamma | dbeta]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nq = a.N >> 2;
  const float inv_n = 1.0f / (float)a.N;
  f32x4 sg[4], sb[4], gam[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    sg[j] = sb[j] = gam[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (ln_chunk(lane, j) < nq) gam[j] = *reinterpret_cast<const f32x4*>(a.gamma + 4 * ln_chunk(lane, j));
  }
  for (long long r = (long long)blockIdx.x * 4 + w; r < a.M; r += (long long)gridDim.x * 4) {
    const unsigned rk = row_key((unsigned)r, key);
    f32x4 v[4], G[4];
    ln_load_drop<F32>(v, a.y, r * a.ld_y, a.x, r * a.ld_x, lane, nq, rk, dc);
    bert_ln_load<F32>(G, a.g, r * a.ld_g, a.g2, r * a.ld_g2, lane, nq);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mu = wave_sum(s) * inv_n;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ln_chunk(lane, j) < nq) {
        const f32x4 d = v[j] - mu;
        q += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
      }
    const float rs = 1.0f / sqrtf(wave_sum(q) * inv_n + a.eps);
    float c1 = 0.f, c2 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ln_chunk(lane, j) < nq) {
        v[j] = (v[j] - mu) * rs;                              // xhat
        const f32x4 gg = G[j] * gam[j], gx = gg * v[j];
        c1 += (gg.x + gg.y) + (gg.z + gg.w);
        c2 += (gx.x + gx.y) + (gx.z + gx.w);
        sg[j] += G[j] * v[j];
        sb[j] += G[j];
      }
    }
    c1 = wave_sum(c1) * inv_n;
    c2 = wave_sum(c2) * inv_n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = ln_chunk(lane, j);
      if (c < nq) {
        const f32x4 ds = (G[j] * gam[j] - c1 - v[j] * c2) * rs;
        st4<F32>(a.ds, r * a.ld_ds + 4 * c, ds);
        st4<F32>(a.dy, r * a.ld_dy + 4 * c, drop4(ds, rk, 4u * c, 0, dc));
      }
    }
  }
  if (!sums) return;                                          // the same for every thread
  if (w > 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = ln_chunk(lane, j);
      if (c < nq) {
        *reinterpret_cast<f32x4*>(&part[w - 1][4 * c]) = sg[j];
        *reinterpret_cast<f32x4*>(&part[w - 1][a.N + 4 * c]) = sb[j];
      }
    }
  }
  __syncthreads();
  if (w == 0) {
    float* dst = a.scratch + (long long)blockIdx.x * 2 * a.N;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = ln_chunk(lane, j);
      if (c < nq) {
        f32x4 tg = sg[j], tb = sb[j];
        for (int k = 0; k < 3; ++k) {                         // wave order
          tg += *reinterpret_cast<const f32x4*>(&part[k][4 * c]);
          tb += *reinterpret_cast<const f32x4*>(&part[k][a.N + 4 * c]);
        }
        *reinterpret_cast<f32x4*>(dst + 4 * c) = tg;
        *reinterpret_cast<f32x4*>(dst + a.N + 4 * c) = tb;
      }
    }
  }
}

// thread (g, cc) adds the partials g, g + 16, ... of chunk cc in that order, then thread (0, cc) the 16 group sums in group order
__global__ __launch_bounds__(256) void bert_drop_ln_fold_kernel(const float* __restrict__ scratch, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int N, int nblk) {
  __shared__ __attribute__((aligned(16))) float red[16][16 * 4];
  const int cc = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cc;                         // chunk of the 2 N columns
  const bool in = c < N / 2;
  f32x4 t{0.f, 0.f, 0.f, 0.f};
  if (in)
    for (int k = g; k < nblk; k += 16) t += *reinterpret_cast<const f32x4*>(scratch + (long long)k * 2 * N + 4 * c);
  *reinterpret_cast<f32x4*>(&red[g][4 * cc]) = t;
  __syncthreads();
  if (g == 0 && in) {
    for (int j = 1; j < 16; ++j) t += *reinterpret_cast<const f32x4*>(&red[j][4 * cc]);
    float* dst = 4 * c < N ? dgamma + 4 * c : dbeta + (4 * c - N);
    *reinterpret_cast<f32x4*>(dst) = t;
  }
}

int ln_blocks(int M) { return (M + 3) / 4 < LN_PARTS ? (M + 3) / 4 : LN_PARTS; }

// the refusals every entry adds to its counterpart's
int drop_check(const char* op, float p, int site) {
  MMDEER_CHECK(p >= 0.f && p < 1.f, "%s: dropout_p must be finite and in [0, 1)", op);      // false for a NaN
  MMDEER_CHECK(site >= 0, "%s: site must be >= 0 (got %d)", op, site);
  return 0;
}
// ... and a device counter that a 64-bit load cannot take (the host never dereferences it)
int counter_check(const char* op, const uint64_t* offset_dev) {
  MMDEER_CHECK(((uintptr_t)offset_dev & 7) == 0, "%s: offset_dev must be 8-byte aligned", op);
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_bert_embed_drop_fwd(const mmdeer_bert_embed_drop_args* a) { return mmdeer_bert_embed_drop_fwd_dev(a, nullptr); }

int mmdeer_bert_embed_drop_fwd_dev(const mmdeer_bert_embed_drop_args* a, const uint64_t* offset_dev) {
  MMDEER_CHECK(a, "bert_embed_drop_fwd: NULL args");
  TRY(drop_check("bert_embed_drop_fwd", a->dropout_p, a->site));
  TRY(counter_check("bert_embed_drop_fwd", offset_dev));
  if (a->dropout_p == 0.f) {
    mmdeer_bert_embed_args p{a->ids, a->type_ids, a->word, a->pos, a->type, a->gamma, a->beta, a->x, a->eps,
                             a->B,   a->L,        a->H,    a->V,   a->P,    a->T,     a->ld_x, a->act_f32, a->stream};
    return mmdeer_bert_embed_fwd(&p);
  }
  MMDEER_CHECK(hidden_ok(a->H), "bert_embed_drop_fwd: unsupported H = %d (a multiple of 64, 64 .. %d)", a->H, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->B >= 0 && a->L >= 0 && a->V >= 1 && a->P >= 1 && a->T >= 1, "bert_embed_drop_fwd: bad shape (B %d, L %d, V %d, P %d, T %d)",
               a->B, a->L, a->V, a->P, a->T);
  MMDEER_CHECK(a->L <= a->P, "bert_embed_drop_fwd: L = %d is above max_position_embeddings P = %d", a->L, a->P);
  MMDEER_CHECK(ld_ok(a->ld_x, a->H, 4), "bert_embed_drop_fwd: bad leading dimension ld_x = %d (>= H, a multiple of 4)", a->ld_x);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_embed_drop_fwd: eps must be finite and >= 0");
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_x), "bert_embed_drop_fwd: x has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->ids && a->word && a->pos && a->type && a->gamma && a->beta && a->x,
               "bert_embed_drop_fwd: NULL pointer (ids, word, pos, type, gamma, beta, x)");
  MMDEER_CHECK(al8(a->ids) && al8(a->type_ids) && al16(a->word) && al16(a->pos) && al16(a->type) && al16(a->gamma) && al16(a->beta) &&
                   al_act4(a->act_f32, {a->x}),
               "bert_embed_drop_fwd: misaligned pointer (ids 8 bytes; tables, gamma, beta 16 bytes; x 4 act elements)");
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, offset_dev);
  MMDEER_LAUNCH_ACT(bert_embed_drop_kernel, a->act_f32, dim3(row_grid(rows)), dim3(256), (hipStream_t)a->stream, *a, rows, dc);
  return 0;
}

int mmdeer_bert_attn_drop_fwd(const mmdeer_bert_attn_drop_args* a) { return mmdeer_bert_attn_drop_fwd_dev(a, nullptr); }

int mmdeer_bert_attn_drop_fwd_dev(const mmdeer_bert_attn_drop_args* a, const uint64_t* offset_dev) {
  MMDEER_CHECK(a, "bert_attn_drop_fwd: NULL args");
  TRY(drop_check("bert_attn_drop_fwd", a->dropout_p, a->site));
  TRY(counter_check("bert_attn_drop_fwd", offset_dev));
  if (a->dropout_p == 0.f) {
    mmdeer_bert_attn_args p{a->qkv, a->mask, a->ctx, a->B, a->L, a->H, a->ld_qkv, a->ld_ctx, a->act_f32, a->stream};
    return mmdeer_bert_attn_fwd(&p);
  }
  TRY(attn_shape_check("bert_attn_drop_fwd", a->B, a->L, a->H));
  MMDEER_CHECK(ld_ok(a->ld_qkv, 3 * a->H, 8), "bert_attn_drop_fwd: bad leading dimension ld_qkv = %d (>= 3 H, a multiple of 8)", a->ld_qkv);
  MMDEER_CHECK(ld_ok(a->ld_ctx, a->H, 4), "bert_attn_drop_fwd: bad leading dimension ld_ctx = %d (>= H, a multiple of 4)", a->ld_ctx);
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_qkv) && under_2_31(rows, a->ld_ctx), "bert_attn_drop_fwd: qkv or ctx has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->qkv && a->mask && a->ctx, "bert_attn_drop_fwd: NULL pointer (qkv, mask, ctx)");
  MMDEER_CHECK(al16(a->qkv) && al4(a->mask) && al_act4(a->act_f32, {a->ctx}),
               "bert_attn_drop_fwd: misaligned pointer (qkv 16 bytes, mask 4 bytes, ctx 4 act elements)");
  const int nqt = (a->L + AT_OWN - 1) / AT_OWN;
  const unsigned grid = (unsigned)((long long)a->B * (a->H / BERT_HD) * nqt);     // < 2^31 / 192
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, offset_dev);
  if (a->act_f32)
    hipLaunchKernelGGL(bert_attn_drop_f32_kernel, dim3(grid), dim3(64), 0, (hipStream_t)a->stream, (const float*)a->qkv, a->mask, (float*)a->ctx,
                       a->L, a->H, a->ld_qkv, a->ld_ctx, nqt, dc, a->site);
  else
    hipLaunchKernelGGL(bert_attn_drop_bf16_kernel, dim3(grid), dim3(128), 0, (hipStream_t)a->stream, (const bf16_t*)a->qkv, a->mask,
                       (bf16_t*)a->ctx, a->L, a->H, a->ld_qkv, a->ld_ctx, nqt, dc, a->site);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_bert_drop_add_ln_fwd(const mmdeer_bert_drop_add_ln_args* a) { return mmdeer_bert_drop_add_ln_fwd_dev(a, nullptr); }

int mmdeer_bert_drop_add_ln_fwd_dev(const mmdeer_bert_drop_add_ln_args* a, const uint64_t* offset_dev) {
  MMDEER_CHECK(a, "bert_drop_add_ln_fwd: NULL args");
  TRY(drop_check("bert_drop_add_ln_fwd", a->dropout_p, a->site));
  TRY(counter_check("bert_drop_add_ln_fwd", offset_dev));
  if (a->dropout_p == 0.f) {
    mmdeer_bert_add_ln_args p{a->y, a->x, a->gamma, a->beta, a->out, a->eps, a->M, a->N, a->ld_y, a->ld_x, a->ld_out, a->act_f32, a->stream};
    return mmdeer_bert_add_ln_fwd(&p);
  }
  MMDEER_CHECK(ln_n_ok(a->N), "bert_drop_add_ln_fwd: unsupported N = %d (a multiple of 4, 4 .. %d)", a->N, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->M >= 0, "bert_drop_add_ln_fwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(ld_ok(a->ld_y, a->N, 4) && ld_ok(a->ld_out, a->N, 4) && (!a->x || ld_ok(a->ld_x, a->N, 4)),
               "bert_drop_add_ln_fwd: bad leading dimension (ld_y %d, ld_x %d, ld_out %d: >= N, multiples of 4)", a->ld_y, a->ld_x, a->ld_out);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_drop_add_ln_fwd: eps must be finite and >= 0");
  MMDEER_CHECK(under_2_31(a->M, a->ld_y) && under_2_31(a->M, a->ld_out) && (!a->x || under_2_31(a->M, a->ld_x)),
               "bert_drop_add_ln_fwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->y && a->gamma && a->beta && a->out, "bert_drop_add_ln_fwd: NULL pointer (y, gamma, beta, out)");
  MMDEER_CHECK(al16(a->gamma) && al16(a->beta) && al_act4(a->act_f32, {a->y, a->x, a->out}),
               "bert_drop_add_ln_fwd: misaligned pointer (gamma, beta 16 bytes; y, x, out 4 act elements)");
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, offset_dev);
  MMDEER_LAUNCH_ACT(bert_drop_add_ln_kernel, a->act_f32, dim3(row_grid(a->M)), dim3(256), (hipStream_t)a->stream, *a, dc);
  return 0;
}

long long mmdeer_bert_attn_drop_bwd_workspace(int32_t B, int32_t L, int32_t H) { return mmdeer_bert_attn_bwd_workspace(B, L, H); }

int mmdeer_bert_attn_drop_bwd(const mmdeer_bert_attn_drop_bwd_args* a) { return mmdeer_bert_attn_drop_bwd_dev(a, nullptr); }

int mmdeer_bert_attn_drop_bwd_dev(const mmdeer_bert_attn_drop_bwd_args* a, const uint64_t* offset_dev) {
  MMDEER_CHECK(a, "bert_attn_drop_bwd: NULL args");
  TRY(drop_check("bert_attn_drop_bwd", a->dropout_p, a->site));
  TRY(counter_check("bert_attn_drop_bwd", offset_dev));
  if (a->dropout_p == 0.f) {
    mmdeer_bert_attn_bwd_args p{a->qkv, a->mask, a->dctx, a->dqkv, a->workspace, a->workspace_bytes, a->B, a->L, a->H, a->ld_qkv, a->ld_dctx,
                                a->ld_dqkv, a->act_f32, a->stream};
    return mmdeer_bert_attn_bwd(&p);
  }
  TRY(attn_shape_check("bert_attn_drop_bwd", a->B, a->L, a->H));
  MMDEER_CHECK(ld_ok(a->ld_qkv, 3 * a->H, 8), "bert_attn_drop_bwd: bad leading dimension ld_qkv = %d (>= 3 H, a multiple of 8)", a->ld_qkv);
  MMDEER_CHECK(ld_ok(a->ld_dqkv, 3 * a->H, 8), "bert_attn_drop_bwd: bad leading dimension ld_dqkv = %d (>= 3 H, a multiple of 8)", a->ld_dqkv);
  MMDEER_CHECK(ld_ok(a->ld_dctx, a->H, 8), "bert_attn_drop_bwd: bad leading dimension ld_dctx = %d (>= H, a multiple of 8)", a->ld_dctx);
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_qkv) && under_2_31(rows, a->ld_dqkv) && under_2_31(rows, a->ld_dctx),
               "bert_attn_drop_bwd: qkv, dqkv or dctx has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->qkv && a->mask && a->dctx && a->dqkv && a->workspace, "bert_attn_drop_bwd: NULL pointer (qkv, mask, dctx, dqkv, workspace)");
  const long long need = mmdeer_bert_attn_bwd_workspace(a->B, a->L, a->H);
  MMDEER_CHECK(a->workspace_bytes >= need, "bert_attn_drop_bwd: workspace too small (%lld bytes, %lld needed)", a->workspace_bytes, need);
  MMDEER_CHECK(al16(a->qkv) && al16(a->dctx) && al16(a->dqkv) && al16(a->workspace) && al4(a->mask),
               "bert_attn_drop_bwd: misaligned pointer (qkv, dctx, dqkv, workspace 16 bytes; mask 4 bytes)");
  const int heads = a->H / BERT_HD, nt = (a->L + AT_OWN - 1) / AT_OWN;
  const long long nstat = (long long)a->B * heads * a->L;
  const unsigned grid = (unsigned)((long long)a->B * heads * nt);       // < 2^31 / 192
  hipStream_t st = (hipStream_t)a->stream;
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, offset_dev);
  if (a->act_f32) {
    hipLaunchKernelGGL(bert_attn_drop_dq_f32_kernel, dim3(grid), dim3(64), 0, st, (const float*)a->qkv, a->mask, (const float*)a->dctx,
                       (float*)a->dqkv, a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat, dc, a->site);
    MMDEER_HIP(hipGetLastError());
    hipLaunchKernelGGL(bert_attn_drop_dkdv_f32_kernel, dim3(grid), dim3(64), 0, st, (const float*)a->qkv, a->mask, (const float*)a->dctx,
                       (float*)a->dqkv, (const float*)a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat, dc, a->site);
  } else {
    hipLaunchKernelGGL(bert_attn_drop_dq_bf16_kernel, dim3(grid), dim3(128), 0, st, (const bf16_t*)a->qkv, a->mask, (const bf16_t*)a->dctx,
                       (bf16_t*)a->dqkv, a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat, dc, a->site);
    MMDEER_HIP(hipGetLastError());
    hipLaunchKernelGGL(bert_attn_drop_dkdv_bf16_kernel, dim3(grid), dim3(128), 0, st, (const bf16_t*)a->qkv, a->mask, (const bf16_t*)a->dctx,
                       (bf16_t*)a->dqkv, (const float*)a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat, dc, a->site);
  }
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_bert_drop_add_ln_bwd_scratch(int32_t M, int32_t N) { return mmdeer_bert_add_ln_bwd_scratch(M, N); }

int mmdeer_bert_drop_add_ln_bwd(const mmdeer_bert_drop_add_ln_bwd_args* a) { return mmdeer_bert_drop_add_ln_bwd_dev(a, nullptr); }

int mmdeer_bert_drop_add_ln_bwd_dev(const mmdeer_bert_drop_add_ln_bwd_args* a, const uint64_t* offset_dev) {
  MMDEER_CHECK(a, "bert_drop_add_ln_bwd: NULL args");
  TRY(drop_check("bert_drop_add_ln_bwd", a->dropout_p, a->site));
  TRY(counter_check("bert_drop_add_ln_bwd", offset_dev));
  MMDEER_CHECK(ln_n_ok(a->N), "bert_drop_add_ln_bwd: unsupported N = %d (a multiple of 4, 4 .. %d)", a->N, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->M >= 0, "bert_drop_add_ln_bwd: bad shape (M %d)", a->M);
  auto ld4_ok = [&](int ld) { return ld_ok(ld, a->N, 4); };
  MMDEER_CHECK(ld4_ok(a->ld_y) && ld4_ok(a->ld_g) && ld4_ok(a->ld_ds) && ld4_ok(a->ld_dy) && (!a->x || ld4_ok(a->ld_x)) && (!a->g2 || ld4_ok(a->ld_g2)),
               "bert_drop_add_ln_bwd: bad leading dimension (ld_y %d, ld_x %d, ld_g %d, ld_g2 %d, ld_ds %d, ld_dy %d: >= N, multiples of 4)", a->ld_y,
               a->ld_x, a->ld_g, a->ld_g2, a->ld_ds, a->ld_dy);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_drop_add_ln_bwd: eps must be finite and >= 0");
  auto small = [&](int ld) { return under_2_31(a->M, ld); };
  MMDEER_CHECK(small(a->ld_y) && small(a->ld_g) && small(a->ld_ds) && small(a->ld_dy) && (!a->x || small(a->ld_x)) && (!a->g2 || small(a->ld_g2)),
               "bert_drop_add_ln_bwd: an operand has 2^31 elements or more");
  MMDEER_CHECK(!a->dgamma == !a->dbeta, "bert_drop_add_ln_bwd: dgamma and dbeta go together (both or neither)");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->y && a->g && a->gamma && a->ds && a->dy, "bert_drop_add_ln_bwd: NULL pointer (y, g, gamma, ds, dy)");
  const int sums = a->dgamma != nullptr;
  const long long need = (long long)ln_blocks(a->M) * 2 * a->N;
  MMDEER_CHECK(!sums || a->scratch, "bert_drop_add_ln_bwd: NULL pointer (scratch, needed for dgamma and dbeta)");
  MMDEER_CHECK(!sums || a->scratch_elems >= need, "bert_drop_add_ln_bwd: scratch too small (%lld elements, %lld needed)", a->scratch_elems, need);
  MMDEER_CHECK(al16(a->gamma) && al16(a->dgamma) && al16(a->dbeta) && (!sums || al16(a->scratch)) &&
                   al_act4(a->act_f32, {a->y, a->x, a->g, a->g2, a->ds, a->dy}),
               "bert_drop_add_ln_bwd: misaligned pointer (gamma, dgamma, dbeta, scratch 16 bytes; y, x, g, g2, ds, dy 4 act elements)");
  if (a->dropout_p == 0.f) {
    // the plain entry's bits in both: dy first, without the sums and from the untouched g (ds may alias g or g2), then ds
    mmdeer_bert_add_ln_bwd_args p{a->y,   a->x,    a->g,   a->g2,   a->gamma, a->dy,    nullptr,  nullptr,    nullptr, 0,
                                  a->eps, a->M,    a->N,   a->ld_y, a->ld_x,  a->ld_g,  a->ld_g2, a->ld_dy,   a->act_f32, a->stream};
    TRY(mmdeer_bert_add_ln_bwd(&p));
    p.ds = a->ds; p.ld_ds = a->ld_ds; p.dgamma = a->dgamma; p.dbeta = a->dbeta; p.scratch = a->scratch; p.scratch_elems = a->scratch_elems;
    return mmdeer_bert_add_ln_bwd(&p);
  }
  const unsigned grid = sums ? (unsigned)ln_blocks(a->M) : row_grid(a->M);
  const DropCtx dc = make_drop(a->dropout_p, a->seed, a->offset, offset_dev);
  MMDEER_LAUNCH_ACT(bert_drop_add_ln_bwd_kernel, a->act_f32, dim3(grid), dim3(256), (hipStream_t)a->stream, *a, sums, dc);
  if (sums) {
    hipLaunchKernelGGL(bert_drop_ln_fold_kernel, dim3((a->N / 2 + 15) / 16), dim3(256), 0, (hipStream_t)a->stream, (const float*)a->scratch,
                       a->dgamma, a->dbeta, a->N, (int)grid);
    MMDEER_HIP(hipGetLastError());
  }
  return 0;
}

}  // extern "C"
