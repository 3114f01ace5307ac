// The BERT trunk's forward operators (include/mmdeer_bert.h; reference: transformers.BertModel as src/models/encoders.py:553-761
// instantiates it): the embedding sum + LayerNorm, masked multi-head self-attention, residual add + LayerNorm and the erf GELU.
// The trunk's Linear layers are mmdeer_gemm calls (mmdeer/bert.py).  Rows are batch-major: row b * L + t.
//
// The tiles, fragments and row layout are bert_dev.h's; what is the forward's own:
//
// Attention, bf16 (bert_attn_bf16_kernel): one workgroup per (sample, head, 64 query rows), the Q fragments in registers.  The head's
// K and V slices come through LDS in tiles of 128 keys: K row-major (18 KB), V TRANSPOSED (16.5 KB) because the second product sums
// over keys.  Per block of 32 keys: S^T = K Q^T, masked keys set to -inf, the running maximum m and sum l of the softmax in fp32, and
// O^T += V^T P^T with the accumulator tile of S^T as the B operand.  l is summed from the ROUNDED probabilities, so the stored row is
// a convex combination of V rows whatever the rounding of P.  Query rows past L are computed on zeros and not stored.
//
// Attention, fp32 (bert_attn_f32_kernel): q and the accumulator in registers, K and V in LDS tiles of 32 keys, the same running
// softmax key by key.
#include "bert_dev.h"

namespace mmdeer {
namespace {

// ------------------------------------------------------------------------------------------------ row LayerNorm
// v: this lane's chunks of the row
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
      const int c = ln_chunk(lane, j);
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
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * 4 + w; r < a.M; r += (long long)gridDim.x * 4) {
    f32x4 v[4];
    bert_ln_load<F32>(v, a.y, r * a.ld_y, a.x, r * a.ld_x, lane, a.N >> 2);
    bert_ln_row<F32>(v, lane, a.N, a.gamma, a.beta, a.eps, a.out, r * a.ld_out);
  }
}

// ------------------------------------------------------------------------------------------------ GELU
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * GELU_RSQRT2)); }

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
  __shared__ __attribute__((aligned(16))) bf16_t Ks[AT_K * ROW_LD];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[BERT_HD * KT_LD];
  __shared__ __attribute__((aligned(16))) unsigned char vb[AT_K];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const AttnBlock blk = attn_block(H / BERT_HD, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + wave * 32 + r;             // this lane's query row (token index)
  const bool wave_live = blk.tile * AT_OWN + wave * 32 < L;    // wave-uniform: a wave without a query row only stages
  const bool live = q < L;
  const bf16_t* kbase = qkv + row0 * ld_qkv + H + blk.head * BERT_HD;
  const bf16_t* vbase = kbase + H;

  // load_row_frags' four loads, written out: through that helper the compiler folds them into two branches and waits for the first
  // load before the staging below starts, one memory latency per workgroup (0.4 us of 8 at B = 8, where a workgroup is all a CU has)
  bf16x8 qf[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 raw{0u, 0u, 0u, 0u};
    if (live) raw = *reinterpret_cast<const u32x4*>(qkv + (row0 + q) * ld_qkv + blk.head * BERT_HD + 16 * ks + 8 * h);
    qf[ks] = __builtin_bit_cast(bf16x8, raw);
  }
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
        for (int t = 0; t < 2; ++t)
          o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_t(Vt + (32 * t + r) * KT_LD + 32 * kb + 16 * s2 + 4 * h), pf[s2], o[t], 0, 0, 0);
    }
  }
  if (wave_live && live) store_tile(ctx, (row0 + q) * ld_ctx + blk.head * BERT_HD, o, h, l > 0.f ? 1.0f / l : 0.f);     // no valid key: zeros
}

// ------------------------------------------------------------------------------------------------ attention, fp32
// grid as above; 64 threads, thread = query row
__global__ __launch_bounds__(64) void bert_attn_f32_kernel(const float* __restrict__ qkv, const float* __restrict__ mask, float* __restrict__ ctx,
                                                           int L, int H, int ld_qkv, int ld_ctx, int nqt) {
  __shared__ __attribute__((aligned(16))) float Kf[AT_F * BERT_HD];
  __shared__ __attribute__((aligned(16))) float Vf[AT_F * BERT_HD];
  __shared__ float mk[AT_F];
  const int tid = threadIdx.x;
  const AttnBlock blk = attn_block(H / BERT_HD, nqt);
  const long long row0 = (long long)blk.b * L;
  const int q = blk.tile * AT_OWN + tid;
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
    for (int key = 0; key < AT_F; ++key) {
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
    for (int c = 0; c < 16; ++c) *reinterpret_cast<f32x4*>(ctx + (row0 + q) * ld_ctx + blk.head * BERT_HD + 4 * c) = acc[c] * inv;
  }
}

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
  MMDEER_CHECK(ld_ok(a->ld_x, a->H, 4), "bert_embed_fwd: bad leading dimension ld_x = %d (>= H, a multiple of 4)", a->ld_x);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_embed_fwd: eps must be finite and >= 0");
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_x), "bert_embed_fwd: x has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->ids && a->word && a->pos && a->type && a->gamma && a->beta && a->x,
               "bert_embed_fwd: NULL pointer (ids, word, pos, type, gamma, beta, x)");
  MMDEER_CHECK(al8(a->ids) && al8(a->type_ids) && al16(a->word) && al16(a->pos) && al16(a->type) && al16(a->gamma) && al16(a->beta) &&
                   al_act4(a->act_f32, {a->x}),
               "bert_embed_fwd: misaligned pointer (ids 8 bytes; tables, gamma, beta 16 bytes; x 4 act elements)");
  MMDEER_LAUNCH_ACT(bert_embed_kernel, a->act_f32, dim3(row_grid(rows)), dim3(256), (hipStream_t)a->stream, *a, rows);
  return 0;
}

int mmdeer_bert_attn_fwd(const mmdeer_bert_attn_args* a) {
  MMDEER_CHECK(a, "bert_attn_fwd: NULL args");
  TRY(attn_shape_check("bert_attn_fwd", a->B, a->L, a->H));
  MMDEER_CHECK(ld_ok(a->ld_qkv, 3 * a->H, 8), "bert_attn_fwd: bad leading dimension ld_qkv = %d (>= 3 H, a multiple of 8)", a->ld_qkv);
  MMDEER_CHECK(ld_ok(a->ld_ctx, a->H, 4), "bert_attn_fwd: bad leading dimension ld_ctx = %d (>= H, a multiple of 4)", a->ld_ctx);
  const long long rows = (long long)a->B * a->L;
  MMDEER_CHECK(under_2_31(rows, a->ld_qkv) && under_2_31(rows, a->ld_ctx), "bert_attn_fwd: qkv or ctx has 2^31 elements or more");
  if (rows == 0) return 0;
  MMDEER_CHECK(a->qkv && a->mask && a->ctx, "bert_attn_fwd: NULL pointer (qkv, mask, ctx)");
  MMDEER_CHECK(al16(a->qkv) && al4(a->mask) && al_act4(a->act_f32, {a->ctx}),
               "bert_attn_fwd: misaligned pointer (qkv 16 bytes, mask 4 bytes, ctx 4 act elements)");
  const int nqt = (a->L + AT_OWN - 1) / AT_OWN;
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
  MMDEER_CHECK(ln_n_ok(a->N), "bert_add_ln_fwd: unsupported N = %d (a multiple of 4, 4 .. %d)", a->N,
               MMDEER_BERT_MAX_HIDDEN);
  MMDEER_CHECK(a->M >= 0, "bert_add_ln_fwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(ld_ok(a->ld_y, a->N, 4) && ld_ok(a->ld_out, a->N, 4) && (!a->x || ld_ok(a->ld_x, a->N, 4)),
               "bert_add_ln_fwd: bad leading dimension (ld_y %d, ld_x %d, ld_out %d: >= N, multiples of 4)", a->ld_y, a->ld_x, a->ld_out);
  MMDEER_CHECK(finite_nonneg(a->eps), "bert_add_ln_fwd: eps must be finite and >= 0");
  MMDEER_CHECK(under_2_31(a->M, a->ld_y) && under_2_31(a->M, a->ld_out) && (!a->x || under_2_31(a->M, a->ld_x)),
               "bert_add_ln_fwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->y && a->gamma && a->beta && a->out, "bert_add_ln_fwd: NULL pointer (y, gamma, beta, out)");
  MMDEER_CHECK(al16(a->gamma) && al16(a->beta) && al_act4(a->act_f32, {a->y, a->x, a->out}),
               "bert_add_ln_fwd: misaligned pointer (gamma, beta 16 bytes; y, x, out 4 act elements)");
  MMDEER_LAUNCH_ACT(bert_add_ln_kernel, a->act_f32, dim3(row_grid(a->M)), dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_bert_gelu_fwd(const mmdeer_bert_gelu_args* a) {
  MMDEER_CHECK(a, "bert_gelu_fwd: NULL args");
  MMDEER_CHECK(a->N >= 4 && a->N % 4 == 0, "bert_gelu_fwd: unsupported N = %d (a multiple of 4)", a->N);
  MMDEER_CHECK(a->M >= 0, "bert_gelu_fwd: bad shape (M %d)", a->M);
  MMDEER_CHECK(ld_ok(a->ld_x, a->N, 4) && ld_ok(a->ld_out, a->N, 4),
               "bert_gelu_fwd: bad leading dimension (ld_x %d, ld_out %d: >= N, multiples of 4)", a->ld_x, a->ld_out);
  MMDEER_CHECK(under_2_31(a->M, a->ld_x) && under_2_31(a->M, a->ld_out), "bert_gelu_fwd: an operand has 2^31 elements or more");
  if (a->M == 0) return 0;
  MMDEER_CHECK(a->x && a->out, "bert_gelu_fwd: NULL pointer (x, out)");
  MMDEER_CHECK(al_act4(a->act_f32, {a->x, a->out}), "bert_gelu_fwd: misaligned pointer (x, out: 4 act elements)");
  const long long chunks = (long long)a->M * (a->N / 4);
  MMDEER_LAUNCH_ACT(bert_gelu_kernel, a->act_f32, dim3(chunk_grid(chunks)), dim3(256), (hipStream_t)a->stream, *a, chunks);
  return 0;
}

}  // extern "C"
