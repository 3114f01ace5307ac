// The BERT trunk's backward operators (include/mmdeer_bert_bwd.h): the gradients of bert.hip's attention, residual add + LayerNorm
// and erf GELU.  The Linear layers' gradients are mmdeer_gemm calls (mmdeer/bert.py).  Rows are batch-major: row b * L + t.
//
// Attention.  With lse_i the log-sum-exp of row i's valid scores, P_ij = exp(S_ij - lse_i) needs no second normalisation, and
// delta_i = sum_j P_ij dP_ij turns the softmax backward into dS = P o (dP - delta).  delta is summed from the kernel's own P and dP
// (a running sum rescaled with the running maximum, divided by the running sum at the end), not from the stored forward output:
// with a single valid key P = 1 and delta = dP to the bit, so dS, dQ and dK are exact zeros as in exact arithmetic.  Two launches,
// each output element with one owner:
//   dq kernel    one workgroup per (sample, head, 64 queries), the forward kernel's shape.  Pass 0 walks the keys for the running
//                maximum, sum and delta and leaves lse and delta in the workspace; pass 1 walks them again for dQ.
//   dkdv kernel  one workgroup per (sample, head, 64 keys), walks the queries in tiles of 64 with lse and delta from the workspace.
// bf16, on bert_dev.h's tiles and fragments (a product is computed TRANSPOSED so that its accumulator tile is the B operand of the
// product that sums over its rows):
//   dq:    S^T = K Q^T and dP^T = V dO^T (A from the row-major K and V tiles, B = this lane's Q and dO rows in registers): a lane holds
//          16 keys of ONE query, so lse and delta are per-lane scalars; dQ^T += K^T dS^T with K^T from the transposed tile.
//   dkdv:  S = Q K^T and dP = dO V^T (A from the row-major Q and dO tiles, B = this lane's K and V rows in registers): a lane holds
//          16 queries of ONE key; dV^T += dO^T P and dK^T += Q^T dS with Q^T and dO^T from the transposed tiles.
// A block of 32 keys (dq) or a wave's 32 keys (dkdv) without a valid key is skipped by a ballot.  A sample without a valid key has
// lse = +inf, so every P is exp(-inf) = 0 and all of dqkv is zero; a masked key's P is set to 0, so its dK and dV are zero.
// Rows past L are zero-filled in LDS (lse = +inf for such a query) and never stored.
// fp32: plain FMA, one thread per query (dq) and one per key (dkdv), K / V and Q / dO in LDS tiles of 32 rows read as broadcasts.
//
// add + LN backward: bert_dev.h's row layout, the forward's two passes for mean and rstd (written out: see the kernel), then two more
// wave sums for the row's means of G gamma and G gamma xhat.  A wave keeps the column sums of its rows in registers; the four waves of a workgroup
// add theirs through LDS in wave order and the workgroup stores one partial pair; bert_ln_fold_kernel adds the partials in a fixed
// order (16 interleaved groups, then the groups).  Which rows a workgroup owns depends on M alone.
#include "../../include/mmdeer_bert_bwd.h"
#include "bert_dev.h"

namespace mmdeer {
namespace {

constexpr int DF_LD = 68;       // floats per dO row in LDS of the fp32 dq kernel: 64 + 4, so that the threads' rows start in different banks
constexpr int LN_PARTS = MMDEER_BERT_LN_BWD_PARTS;

// ------------------------------------------------------------------------------------------------ attention backward, bf16: dQ
// grid: ((b * heads + head) * nqt + qt); 128 threads.  ws: lse [B * heads * L], then delta [B * heads * L].
__global__ __launch_bounds__(128) void bert_attn_dq_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask,
                                                                const bf16_t* __restrict__ dctx, bf16_t* __restrict__ dqkv,
                                                                float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx, int ld_dqkv,
                                                                int nqt, long long nstat) {
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
  if (wave_live && live) store_tile(dqkv, (row0 + q) * ld_dqkv + blk.head * BERT_HD, o, h, 0.125f);
}

// ------------------------------------------------------------------------------------------------ attention backward, bf16: dK, dV
// grid: ((b * heads + head) * nkt + kt); 128 threads
__global__ __launch_bounds__(128) void bert_attn_dkdv_bf16_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ mask,
                                                                  const bf16_t* __restrict__ dctx, bf16_t* __restrict__ dqkv,
                                                                  const float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx,
                                                                  int ld_dqkv, int nkt, long long nstat) {
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
  const int key = blk.tile * AT_OWN + wave * 32 + r;                    // this lane's key
  const bool live = key < L;
  const bool valid = live && mask[row0 + (live ? key : 0)] != 0.f;
  const bool wave_work = __builtin_amdgcn_ballot_w64(valid) != 0ull;      // wave-uniform: a wave without a valid key only stages
  const bf16_t* qbase = qkv + row0 * ld_qkv + blk.head * BERT_HD;
  const bf16_t* obase = dctx + row0 * ld_dctx + blk.head * BERT_HD;
  const float* lse_g = ws + ((long long)blk.b * heads + blk.head) * L;

  bf16x8 kf[4], vf[4];
  load_row_frags(kf, qkv + (row0 + (live ? key : 0)) * ld_qkv + H + blk.head * BERT_HD, live, h);
  load_row_frags(vf, qkv + (row0 + (live ? key : 0)) * ld_qkv + 2 * H + blk.head * BERT_HD, live, h);
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
      bf16x8 pf[2], dsf[2];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 ls = *reinterpret_cast<const f32x4*>(lse_s + 32 * qb + 8 * g + 4 * h);
        const f32x4 dl = *reinterpret_cast<const f32x4*>(del_s + 32 * qb + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int i = 4 * g + e;
          const float p = valid ? __expf(s[i] * 0.125f - ls[e]) : 0.f;
          pf[i >> 3][i & 7] = (__bf16)p;
          dsf[i >> 3][i & 7] = (__bf16)(p * (dp[i] - dl[e]));
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
    store_tile(dqkv, (row0 + key) * ld_dqkv + H + blk.head * BERT_HD, dk, h, 0.125f);
    store_tile(dqkv, (row0 + key) * ld_dqkv + 2 * H + blk.head * BERT_HD, dv, h, 1.0f);
  }
}

// ------------------------------------------------------------------------------------------------ attention backward, fp32
// grid as the bf16 dq kernel's; 64 threads, thread = query row
__global__ __launch_bounds__(64) void bert_attn_dq_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask,
                                                              const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                              float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx, int ld_dqkv,
                                                              int nqt, long long nstat) {
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
      for (int key = 0; key < AT_F; ++key) {
        if (mk[key] == 0.f) continue;                         // the same for every thread
        f32x4 d4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) d4 += qv[c] * *reinterpret_cast<const f32x4*>(Kf + key * BERT_HD + 4 * c);
        const float s = (d4.x + d4.y) + (d4.z + d4.w);
        f32x4 e4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 16; ++c) e4 += *reinterpret_cast<const f32x4*>(dov + 4 * c) * *reinterpret_cast<const f32x4*>(Vf + key * BERT_HD + 4 * c);
        const float dp = (e4.x + e4.y) + (e4.z + e4.w);
        if (pass == 0) {
          const float m_new = fmaxf(m, s);                    // s is finite, so m_new is
          const float alpha = expf(m - m_new), e = expf(s - m_new);
          l = l * alpha + e;
          dacc = fmaf(e, dp, dacc * alpha);
          m = m_new;
        } else {
          const float ds = expf(s - lse) * (dp - delta);
#pragma unroll
          for (int c = 0; c < 16; ++c) acc[c] += ds * *reinterpret_cast<const f32x4*>(Kf + key * BERT_HD + 4 * c);
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
#pragma unroll
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x4*>(dqkv + (row0 + q) * ld_dqkv + blk.head * BERT_HD + 4 * c) = acc[c] * 0.125f;
  }
}

// grid as the bf16 dkdv kernel's; 64 threads, thread = key
__global__ __launch_bounds__(64) void bert_attn_dkdv_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask,
                                                                const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                const float* __restrict__ ws, int L, int H, int ld_qkv, int ld_dctx,
                                                                int ld_dqkv, int nkt, long long nstat) {
  __shared__ __attribute__((aligned(16))) float Qf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Of[AT_F * BERT_HD];
  __shared__ float lse_s[AT_F];
  __shared__ float del_s[AT_F];
  const int tid = threadIdx.x;
  const int heads = H / BERT_HD;
  const AttnBlock blk = attn_block(heads, nkt);
  const long long row0 = (long long)blk.b * L;
  const int key = blk.tile * AT_OWN + tid;
  const bool live = key < L;
  const bool valid = live && mask[row0 + (live ? key : 0)] != 0.f;
  const float* qbase = qkv + row0 * ld_qkv + blk.head * BERT_HD;
  const float* obase = dctx + row0 * ld_dctx + blk.head * BERT_HD;
  const float* lse_g = ws + ((long long)blk.b * heads + blk.head) * L;
  f32x4 kv[16], vv[16], dk[16], dv[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    kv[c] = vv[c] = dk[c] = dv[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
      kv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + key) * ld_qkv + H + blk.head * BERT_HD + 4 * c) * 0.125f;
      vv[c] = *reinterpret_cast<const f32x4*>(qkv + (row0 + key) * ld_qkv + 2 * H + blk.head * BERT_HD + 4 * c);
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
      const float p = valid ? expf(((d4.x + d4.y) + (d4.z + d4.w)) - ls) : 0.f;
      const float ds = p * (((e4.x + e4.y) + (e4.z + e4.w)) - del_s[qi]);
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        dv[c] += p * *reinterpret_cast<const f32x4*>(Of + qi * BERT_HD + 4 * c);
        dk[c] += ds * *reinterpret_cast<const f32x4*>(Qf + qi * BERT_HD + 4 * c);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      *reinterpret_cast<f32x4*>(dqkv + (row0 + key) * ld_dqkv + H + blk.head * BERT_HD + 4 * c) = dk[c] * 0.125f;
      *reinterpret_cast<f32x4*>(dqkv + (row0 + key) * ld_dqkv + 2 * H + blk.head * BERT_HD + 4 * c) = dv[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ add + LayerNorm backward
// grid: nblk workgroups of 4 waves; row r belongs to wave (r & 3) of workgroup (r >> 2) % nblk.  SUMS: the column sums are formed.
template <bool F32>
__global__ __launch_bounds__(256) void bert_add_ln_bwd_kernel(mmdeer_bert_add_ln_bwd_args a, int sums) {
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
    f32x4 v[4], G[4];
    bert_ln_load<F32>(v, a.y, r * a.ld_y, a.x, r * a.ld_x, lane, nq);
    bert_ln_load<F32>(G, a.g, r * a.ld_g, a.g2, r * a.ld_g2, lane, nq);
    // Mean and rstd in bert_ln_row's two passes, written out here and NOT shared with it: the compiler contracts the forward's
    // v - mu (and its squares) into fused multiply-adds and leaves these apart, so the two round differently in the last bit.  One
    // function called from both compiles to the forward's form here and moves the bits this kernel has stored so far.
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
      if (c < nq) st4<F32>(a.ds, r * a.ld_ds + 4 * c, (G[j] * gam[j] - c1 - v[j] * c2) * rs);
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

// A workgroup folds 16 of the 4-column chunks of [dgamma | dbeta]: thread (g, cc) adds the partials g, g + 16, ... of chunk cc in that
// order, then thread (0, cc) adds the 16 group sums in group order.  A fixed order, whatever the grid.
__global__ __launch_bounds__(256) void bert_ln_fold_kernel(const float* __restrict__ scratch, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           int N, int nblk) {
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

// ------------------------------------------------------------------------------------------------ GELU backward
__device__ __forceinline__ float gelu_erf_grad(float x) {
  return 0.5f * (1.0f + erff(x * GELU_RSQRT2)) + x * (0.39894228040143267794f * expf(-0.5f * x * x));
}

template <bool F32>
__global__ __launch_bounds__(256) void bert_gelu_bwd_kernel(mmdeer_bert_gelu_bwd_args a, long long chunks) {
  const int nq = a.N >> 2;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < chunks; i += (long long)gridDim.x * 256) {
    const long long r = i / nq;
    const int c = (int)(i - r * nq);
    const f32x4 v = ld4<F32>(a.x, r * a.ld_x + 4 * c), g = ld4<F32>(a.g, r * a.ld_g + 4 * c);
    st4<F32>(a.dx, r * a.ld_dx + 4 * c, f32x4{g.x * gelu_erf_grad(v.x), g.y * gelu_erf_grad(v.y), g.z * gelu_erf_grad(v.z), g.w * gelu_erf_grad(v.w)});
  }
}

long long attn_ws_bytes(int B, int L, int H) { return 2ll * B * (H / BERT_HD) * L * (long long)sizeof(float); }
int ln_blocks(int M) { return (M + 3) / 4 < LN_PARTS ? (M + 3) / 4 : LN_PARTS; }

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

long long mmdeer_bert_attn_bwd_workspace(int32_t B, int32_t L, int32_t H) {
  if (attn_shape_fault(B, L, H)) return -1;
  return attn_ws_bytes(B, L, H);
}

int mmdeer_bert_attn_bwd(const mmdeer_bert_attn_bwd_args* a) {
  MMDEER_CHECK(a, "bert_attn_bwd: NULL args");
  TRY(attn_shape_check("bert_attn_bwd", a->B, a->L, a->H));
  MMDEER_CHECK(ld_ok(a->ld_qkv, 3 * a->H, 8), "bert_attn_bwd: bad leading dimension ld_qkv = %d (>= 3 H, a multiple of 8)", a->ld_qkv);
  MMDEER_CHECK(ld_ok(a->ld_dqkv, 3 * a->H, 8), "bert_attn_bwd: bad leading dimension ld_dqkv = %d (>= 3 H, a multiple of 8)", a->ld_dqkv);
  MMDEER_CHECK(ld_ok(a->ld_dctx, a->H, 8), "bert_attn_bwd: bad leading dimension ld_dctx = %d (>= H, a multiple of 8)", a->ld_dctx);
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_qkv) && under_2_31(rows, a->ld_dqkv) && under_2_31(rows, a->ld_dctx),
               "bert_attn_bwd: qkv, dqkv or dctx has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->qkv && a->mask && a->dctx && a->dqkv && a->workspace, "bert_attn_bwd: NULL pointer (qkv, mask, dctx, dqkv, workspace)");
  MMDEER_CHECK(a->workspace_bytes >= attn_ws_bytes(a->B, a->L, a->H), "bert_attn_bwd: workspace too small (%lld bytes, %lld needed)",
               a->workspace_bytes, attn_ws_bytes(a->B, a->L, a->H));
  MMDEER_CHECK(al16(a->qkv) && al16(a->dctx) && al16(a->dqkv) && al16(a->workspace) && al4(a->mask),
               "bert_attn_bwd: misaligned pointer (qkv, dctx, dqkv, workspace 16 bytes; mask 4 bytes)");
  const int heads = a->H / BERT_HD, nt = (a->L + AT_OWN - 1) / AT_OWN;
  const long long nstat = (long long)a->B * heads * a->L;
  const unsigned grid = (unsigned)((long long)a->B * heads * nt);       // < 2^31 / 192
  hipStream_t st = (hipStream_t)a->stream;
  if (a->act_f32) {
    hipLaunchKernelGGL(bert_attn_dq_f32_kernel, dim3(grid), dim3(64), 0, st, (const float*)a->qkv, a->mask, (const float*)a->dctx,
                       (float*)a->dqkv, a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat);
    MMDEER_HIP(hipGetLastError());
    hipLaunchKernelGGL(bert_attn_dkdv_f32_kernel, dim3(grid), dim3(64), 0, st, (const float*)a->qkv, a->mask, (const float*)a->dctx,
                       (float*)a->dqkv, (const float*)a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat);
  } else {
    hipLaunchKernelGGL(bert_attn_dq_bf16_kernel, dim3(grid), dim3(128), 0, st, (const bf16_t*)a->qkv, a->mask, (const bf16_t*)a->dctx,
                       (bf16_t*)a->dqkv, a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat);
    MMDEER_HIP(hipGetLastError());
    hipLaunchKernelGGL(bert_attn_dkdv_bf16_kernel, dim3(grid), dim3(128), 0, st, (const bf16_t*)a->qkv, a->mask, (const bf16_t*)a->dctx,
                       (bf16_t*)a->dqkv, (const float*)a->workspace, a->L, a->H, a->ld_qkv, a->ld_dctx, a->ld_dqkv, nt, nstat);
  }
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_bert_add_ln_bwd_scratch(int32_t M, int32_t N) {
  if (!ln_n_ok(N) || M < 0) return -1;
  return (long long)ln_blocks(M) * 2 * N;
}

int mmdeer_bert_add_ln_bwd(const mmdeer_bert_add_ln_bwd_args* a) {
  MMDEER_CHECK(a, "bert_add_ln_bwd: NULL args");
  MMDEER_CHECK(ln_n_ok(a->N), "bert_add_ln_bwd: unsupported N = %d (a multiple of 4, 4 .. %d)", a->N, MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->M >= 0, "bert_add_ln_bwd: bad shape (M %d)", a->M);
  auto ld4_ok = [&](int ld) { return ld_ok(ld, a->N, 4); };
  MMDEER_CHECK(ld4_ok(a->ld_y) && ld4_ok(a->ld_g) && ld4_ok(a->ld_ds) && (!a->x || ld4_ok(a->ld_x)) && (!a->g2 || ld4_ok(a->ld_g2)),
               "bert_add_ln_bwd: bad leading dimension (ld_y %d, ld_x %d, ld_g %d, ld_g2 %d, ld_ds %d: >= N, multiples of 4)", a->ld_y, a->ld_x,
               a->ld_g, a->ld_g2, a->ld_ds);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_add_ln_bwd: eps must be finite and >= 0");
  auto small = [&](int ld) { return under_2_31(a->M, ld); };
  MMDEER_CHECK(small(a->ld_y) && small(a->ld_g) && small(a->ld_ds) && (!a->x || small(a->ld_x)) && (!a->g2 || small(a->ld_g2)),
               "bert_add_ln_bwd: an operand has 2^31 elements or more");
  MMDEER_CHECK(!a->dgamma == !a->dbeta, "bert_add_ln_bwd: dgamma and dbeta go together (both or neither)");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->y && a->g && a->gamma && a->ds, "bert_add_ln_bwd: NULL pointer (y, g, gamma, ds)");
  const int sums = a->dgamma != nullptr;
  const long long need = (long long)ln_blocks(a->M) * 2 * a->N;
  MMDEER_CHECK(!sums || a->scratch, "bert_add_ln_bwd: NULL pointer (scratch, needed for dgamma and dbeta)");
  MMDEER_CHECK(!sums || a->scratch_elems >= need, "bert_add_ln_bwd: scratch too small (%lld elements, %lld needed)", a->scratch_elems, need);
  MMDEER_CHECK(al16(a->gamma) && al16(a->dgamma) && al16(a->dbeta) && (!sums || al16(a->scratch)) && al_act4(a->act_f32, {a->y, a->x, a->g, a->g2, a->ds}),
               "bert_add_ln_bwd: misaligned pointer (gamma, dgamma, dbeta, scratch 16 bytes; y, x, g, g2, ds 4 act elements)");
  const unsigned grid = sums ? (unsigned)ln_blocks(a->M) : row_grid(a->M);
  MMDEER_LAUNCH_ACT(bert_add_ln_bwd_kernel, a->act_f32, dim3(grid), dim3(256), (hipStream_t)a->stream, *a, sums);
  if (sums) {
    hipLaunchKernelGGL(bert_ln_fold_kernel, dim3((a->N / 2 + 15) / 16), dim3(256), 0, (hipStream_t)a->stream, (const float*)a->scratch, a->dgamma,
                       a->dbeta, a->N, (int)grid);
    MMDEER_HIP(hipGetLastError());
  }
  return 0;
}

int mmdeer_bert_gelu_bwd(const mmdeer_bert_gelu_bwd_args* a) {
  MMDEER_CHECK(a, "bert_gelu_bwd: NULL args");
  MMDEER_CHECK(a->N >= 4 && a->N % 4 == 0, "bert_gelu_bwd: unsupported N = %d (a multiple of 4)", a->N);
  MMDEER_CHECK(a->M >= 0, "bert_gelu_bwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(ld_ok(a->ld_x, a->N, 4) && ld_ok(a->ld_g, a->N, 4) && ld_ok(a->ld_dx, a->N, 4),
               "bert_gelu_bwd: bad leading dimension (ld_x %d, ld_g %d, ld_dx %d: >= N, multiples of 4)", a->ld_x, a->ld_g, a->ld_dx);
  MMDEER_CHECK(under_2_31(a->M, a->ld_x) && under_2_31(a->M, a->ld_g) && under_2_31(a->M, a->ld_dx),
               "bert_gelu_bwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->x && a->g && a->dx, "bert_gelu_bwd: NULL pointer (x, g, dx)");
  MMDEER_CHECK(al_act4(a->act_f32, {a->x, a->g, a->dx}), "bert_gelu_bwd: misaligned pointer (x, g, dx: 4 act elements)");
  const long long chunks = (long long)a->M * (a->N / 4);
  MMDEER_LAUNCH_ACT(bert_gelu_bwd_kernel, a->act_f32, dim3(chunk_grid(chunks)), dim3(256), (hipStream_t)a->stream, *a, chunks);
  return 0;
}

}  // extern "C"
