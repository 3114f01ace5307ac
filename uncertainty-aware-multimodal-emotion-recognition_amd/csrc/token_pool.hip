// Temporal text encoder (reference src/models/encoders.py:648-746, the no-BERT configuration and the BERT branch downstream of
// last_hidden_state): token gather with deterministic table gradients, the masked attention pool over tokens and the
// per-sample token statistics ("linguistic features").  Rows are batch-major: row b * L + t.
//
// A 768-wide row is 96 pieces of 8 elements: lane l of a wave owns piece l and, for l < 32, piece 64 + l, so every global
// access of an activation row is one 16-byte load (bf16) or two (fp32).  A 384-wide score row is 48 pieces: lanes 0 .. 47.
//
// Gather (mmdeer_token_embed_fwd / _bwd): one wave per row.  The table gradients use no floating-point atomics:
//   d_pos[p]  one workgroup per position, its four waves take the samples b = w, w + 4, ... in order and are merged in wave order
//   d_emb[id] the rows are grouped by id with the library's stable mmdeer_sort_pairs (key = the clamped id as fp32; masked rows
//             and id 0, the padding row, get the key V and sort behind every real id); one wave per distinct id sums its run
//             in row order.  Rows that no valid token names stay at the zeros of the memset that precedes the launch.
//
// Pool (mmdeer_token_pool_fwd / _bwd): one workgroup per sample, its four waves split the tokens (t = w, w + 4, ...).  Scores
// go through the weights buffer (L is arbitrary, so they are not kept in LDS); the waves' maxima, normalisers and accumulators
// are merged through LDS in wave order.  dw2: per-workgroup partials folded in index order by a second launch; db2 = 0.
//
// Statistics (mmdeer_token_stats): one workgroup per sample, ids in LDS, O(L^2) duplicate count, integer LDS atomics only.
#include "../../include/mmdeer.h"
#include "elem.h"
#include "rowops.h"

namespace mmdeer {
namespace {

constexpr int TOK_E = 768;           // embedding width (bert_hidden_size)
constexpr int TOK_A = 384;           // score layer width (E / 2)
constexpr int TOK_ZL = TOK_A / 8;    // lanes that own a piece of a score row
constexpr int TOK_STATS_MAX_L = 2048;
constexpr long long TOK_MAX_ROWS = 1ll << 20;   // mmdeer_sort_pairs' limit
constexpr float TOK_EPS = 1e-10f;

// one 768-wide row in a wave: v[0], v[1] = piece `lane`, v[2], v[3] = piece 64 + lane (lanes 0 .. 31, zero elsewhere)
template <bool F32>
__device__ __forceinline__ void ld_row(const void* base, long long row_off, int lane, f32x4 (&v)[4]) {
  ld8<F32>(base, row_off + lane * 8, v[0], v[1]);
  v[2] = v[3] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (lane < 32) ld8<F32>(base, row_off + 512 + lane * 8, v[2], v[3]);
}
template <bool F32>
__device__ __forceinline__ void st_row(void* base, long long row_off, int lane, const f32x4 (&v)[4]) {
  st8<F32>(base, row_off + lane * 8, v[0], v[1]);
  if (lane < 32) st8<F32>(base, row_off + 512 + lane * 8, v[2], v[3]);
}
__device__ __forceinline__ float dot_row(const f32x4 (&a)[4], const f32x4 (&b)[4]) {
  const f32x4 p = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  return wave_sum((p.x + p.y) + (p.z + p.w));
}

// ------------------------------------------------------------------------------------------------ gather
// one wave per row (grid-stride).  Tables: x = (emb[clamp(id)] + pos[min(t, P - 1)]) * m and ids32 = the clamped id;
// src: x = src * m.  m = (mask != 0).
template <bool F32>
__global__ __launch_bounds__(256) void token_embed_fwd_kernel(mmdeer_token_embed_args a, long long rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * 4 + w; r < rows; r += (long long)gridDim.x * 4) {
    const bool m = a.mask[r] != 0.f;
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.emb) {
      const long long raw = a.ids[r];
      const int id = raw < 0 ? 0 : (raw > a.V - 1 ? a.V - 1 : (int)raw);
      if (lane == 0) a.ids32[r] = id;
      if (m) {
        const int t = (int)(r % a.L), p = t < a.P - 1 ? t : a.P - 1;
        f32x4 e[4], q[4];
        ld_row<true>(a.emb, (long long)id * TOK_E, lane, e);
        ld_row<true>(a.pos, (long long)p * TOK_E, lane, q);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = e[k] + q[k];
      }
    } else if (m) {
      ld_row<true>(a.src, r * a.ld_src, lane, v);
    }
    st_row<F32>(a.x, r * a.ld_x, lane, v);
  }
}

// d_src = dx * m (fp32), one wave per row
template <bool F32>
__global__ __launch_bounds__(256) void token_embed_dsrc_kernel(mmdeer_token_embed_args a, long long rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long r = (long long)blockIdx.x * 4 + w; r < rows; r += (long long)gridDim.x * 4) {
    f32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.mask[r] != 0.f) ld_row<F32>(a.dx, r * a.ld_dx, lane, v);
    st_row<true>(a.d_src, r * a.ld_dsrc, lane, v);
  }
}

// d_pos[p] = sum over b (and, for p = P - 1, over t >= P - 1) of dx * m.  grid P; wave w takes b = w, w + 4, ...
template <bool F32>
__global__ __launch_bounds__(256) void token_embed_dpos_kernel(mmdeer_token_embed_args a) {
  __shared__ f32x4 red[4][64][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = blockIdx.x, L = a.L;
  const int t0 = p, t1 = p == a.P - 1 ? L : (p + 1 < L ? p + 1 : L);     // [t0, t1): empty when p >= L
  f32x4 acc[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int b = w; b < a.B; b += 4)
    for (int t = t0; t < t1; ++t) {
      const long long r = (long long)b * L + t;
      if (a.mask[r] != 0.f) {
        f32x4 v[4];
        ld_row<F32>(a.dx, r * a.ld_dx, lane, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] += v[k];
      }
    }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[w][lane][k] = acc[k];
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = ((red[0][lane][k] + red[1][lane][k]) + red[2][lane][k]) + red[3][lane][k];
    st_row<true>(a.d_pos, (long long)p * TOK_E, lane, acc);
  }
}

// sort key of a row: its clamped id, or V (behind every id) when the row is masked or names the padding row 0
__global__ __launch_bounds__(256) void token_embed_keys_kernel(const int* ids32, const float* mask, long long rows, int V, float* keys) {
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long long)gridDim.x * 256) {
    const int id = ids32[r];
    keys[r] = (mask[r] != 0.f && id != 0) ? (float)id : (float)V;
  }
}

// sorted: mmdeer_sort_pairs' (key image << 32 | row) pairs, ascending.  One wave per run of equal keys, summed in row order.
template <bool F32>
__global__ __launch_bounds__(256) void token_embed_demb_kernel(mmdeer_token_embed_args a, const unsigned long long* sorted, long long rows) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long i = (long long)blockIdx.x * 4 + w; i < rows; i += (long long)gridDim.x * 4) {
    const unsigned key = (unsigned)(sorted[i] >> 32);
    if (i > 0 && (unsigned)(sorted[i - 1] >> 32) == key) continue;          // not the head of its run
    const int id = (int)__uint_as_float(key & 0x7FFFFFFFu);                 // image of a non-negative float: bits | sign
    if (id <= 0 || id >= a.V) continue;                                     // the masked / padding run
    f32x4 acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long long j = i; j < rows; ++j) {
      const unsigned long long e = sorted[j];
      if ((unsigned)(e >> 32) != key) break;
      const long long r = (long long)(unsigned)(e & 0xFFFFFFFFull);
      f32x4 v[4];
      ld_row<F32>(a.dx, r * a.ld_dx, lane, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += v[k];
    }
    st_row<true>(a.d_emb, (long long)id * TOK_E, lane, acc);
  }
}

// ------------------------------------------------------------------------------------------------ pool
template <bool F32>
__global__ __launch_bounds__(256) void token_pool_fwd_kernel(mmdeer_token_pool_args a) {
  __shared__ float redm[4], redl[4], reds[4];
  __shared__ f32x4 red[4][64][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
  const long long row0 = (long long)blockIdx.x * L;
  float* wts = a.weights + row0;
  const float* mk = a.mask + row0;
  f32x4 w2lo{0.f, 0.f, 0.f, 0.f}, w2hi{0.f, 0.f, 0.f, 0.f};
  if (lane < TOK_ZL) ld8<true>(a.w2, lane * 8, w2lo, w2hi);
  const float b2 = a.b2[0];
  // scores of this wave's tokens -> weights[t]; running max
  float mx = -INFINITY;
  for (int t = w; t < L; t += 4) {
    float s = 0.f;
    if (lane < TOK_ZL) {
      f32x4 zl, zh;
      ld8<F32>(a.z, (row0 + t) * a.ld_z + lane * 8, zl, zh);
      const f32x4 q = w2lo * tanh4(zl) + w2hi * tanh4(zh);
      s = (q.x + q.y) + (q.z + q.w);
    }
    s = wave_sum(s) + b2;
    if (lane == 0) wts[t] = s;
    mx = fmaxf(mx, s);
  }
  if (lane == 0) redm[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
  // softmax over ALL L positions; S = sum of the valid ones' probabilities
  float l = 0.f, sm = 0.f;
  for (int t = threadIdx.x; t < L; t += 256) {
    const float e = expf(wts[t] - mx);
    l += e;
    if (mk[t] != 0.f) sm += e;
  }
  l = wave_sum(l);
  sm = wave_sum(sm);
  if (lane == 0) { redl[w] = l; reds[w] = sm; }
  __syncthreads();
  l = ((redl[0] + redl[1]) + redl[2]) + redl[3];
  sm = ((reds[0] + reds[1]) + reds[2]) + reds[3];
  const float S = sm / l;
  for (int t = threadIdx.x; t < L; t += 256) {
    const float p = expf(wts[t] - mx) / l;
    if (a.probs) a.probs[row0 + t] = p;
    wts[t] = mk[t] != 0.f ? p / (S + TOK_EPS) : 0.f;
  }
  __syncthreads();
  // attended = sum_t a_t x_t; rows of weight zero (masked) are not read
  f32x4 o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int t = w; t < L; t += 4) {
    const float at = wts[t];
    if (at != 0.f) {
      f32x4 v[4];
      ld_row<F32>(a.x, (row0 + t) * a.ld_x, lane, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] += at * v[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[w][lane][k] = o[k];
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = ((red[0][lane][k] + red[1][lane][k]) + red[2][lane][k]) + red[3][lane][k];
    st_row<F32>(a.attended, (long long)blockIdx.x * a.ld_att, lane, o);
  }
}

constexpr int TOK_POOL_BWD_WG = 1024;   // workgroups of the backward at most: one fp32 [384] partial of dw2 each

// ds_t = p_t (m_t (da_t - c) - c eps) / (S + eps), da_t = dout . x_t, c = sum_u a_u da_u, S = sum_u p_u m_u
template <bool F32>
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(mmdeer_token_pool_args a) {
  __shared__ float redc[4], redS[4];
  __shared__ f32x4 redw[4][TOK_ZL][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, L = a.L;
  f32x4 w2lo{0.f, 0.f, 0.f, 0.f}, w2hi{0.f, 0.f, 0.f, 0.f}, pwlo{0.f, 0.f, 0.f, 0.f}, pwhi{0.f, 0.f, 0.f, 0.f};
  if (lane < TOK_ZL) ld8<true>(a.w2, lane * 8, w2lo, w2hi);
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const long long row0 = (long long)b * L;
    const float* wts = a.weights + row0;
    const float* pr = a.probs + row0;
    const float* mk = a.mask + row0;
    f32x4 d[4];
    ld_row<F32>(a.dout, (long long)b * a.ld_dout, lane, d);
    float c = 0.f, S = 0.f;
    for (int t = w; t < L; t += 4) {
      const float at = wts[t];
      if (mk[t] != 0.f) S += pr[t];
      if (at != 0.f) {
        f32x4 v[4];
        ld_row<F32>(a.x, (row0 + t) * a.ld_x, lane, v);
        c += at * dot_row(d, v);
      }
    }
    if (lane == 0) { redc[w] = c; redS[w] = S; }
    __syncthreads();
    c = ((redc[0] + redc[1]) + redc[2]) + redc[3];
    S = ((redS[0] + redS[1]) + redS[2]) + redS[3];
    const float inv = 1.f / (S + TOK_EPS);
    for (int t = w; t < L; t += 4) {
      const float at = wts[t];
      float g = -c * TOK_EPS;
      if (mk[t] != 0.f) {
        f32x4 v[4];
        ld_row<F32>(a.x, (row0 + t) * a.ld_x, lane, v);
        g += dot_row(d, v) - c;
      }
      const float ds = pr[t] * g * inv;
      f32x4 o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) o[k] = at * d[k];
      st_row<F32>(a.dx, (row0 + t) * a.ld_dx, lane, o);
      if (lane < TOK_ZL) {
        f32x4 zl, zh;
        ld8<F32>(a.z, (row0 + t) * a.ld_z + lane * 8, zl, zh);
        const f32x4 tl = tanh4(zl), th = tanh4(zh);
        st8<F32>(a.dz, (row0 + t) * a.ld_dz + lane * 8, ds * w2lo * (1.f - tl * tl), ds * w2hi * (1.f - th * th));
        pwlo += ds * tl;
        pwhi += ds * th;
      }
    }
    __syncthreads();                     // redc / redS are rewritten by the next sample
  }
  if (lane < TOK_ZL) { redw[w][lane][0] = pwlo; redw[w][lane][1] = pwhi; }
  __syncthreads();
  if (w == 0 && lane < TOK_ZL) {
    float* out = a.scratch + (long long)blockIdx.x * TOK_A + lane * 8;
    *reinterpret_cast<f32x4*>(out) = ((redw[0][lane][0] + redw[1][lane][0]) + redw[2][lane][0]) + redw[3][lane][0];
    *reinterpret_cast<f32x4*>(out + 4) = ((redw[0][lane][1] + redw[1][lane][1]) + redw[2][lane][1]) + redw[3][lane][1];
  }
}

// ------------------------------------------------------------------------------------------------ statistics
// out[b][0..5] = n / max_length, u / max(n, 1), n / (id_max + 1), c_max, #{999 <= id <= 1030} / max(n, 1),
// #{100 <= id <= 999} / max(n, 1); out[b][6..15] = 0.  n = 0: all zeros.
__global__ __launch_bounds__(256) void token_stats_kernel(mmdeer_token_stats_args a) {
  __shared__ int sid[TOK_STATS_MAX_L];
  __shared__ unsigned char sv[TOK_STATS_MAX_L];
  __shared__ int acc[6];     // n, u, c_max, id_max, punct, special
  const int L = a.L, b = blockIdx.x;
  if (threadIdx.x < 6) acc[threadIdx.x] = threadIdx.x == 3 ? -1 : 0;
  for (int t = threadIdx.x; t < L; t += 256) {
    sid[t] = a.ids[(long long)b * L + t];
    sv[t] = a.mask[(long long)b * L + t] != 0.f;
  }
  __syncthreads();
  int n = 0, u = 0, cmax = 0, idmax = -1, punct = 0, special = 0;
  for (int i = threadIdx.x; i < L; i += 256) {
    if (!sv[i]) continue;
    const int id = sid[i];
    int c = 0, first = 1;
    for (int j = 0; j < L; ++j)
      if (sv[j] && sid[j] == id) {
        ++c;
        if (j < i) first = 0;
      }
    ++n;
    u += first;
    cmax = c > cmax ? c : cmax;
    idmax = id > idmax ? id : idmax;
    punct += id >= 999 && id <= 1030;
    special += id >= 100 && id <= 999;
  }
  if (n) {
    atomicAdd(&acc[0], n); atomicAdd(&acc[1], u); atomicMax(&acc[2], cmax); atomicMax(&acc[3], idmax);
    atomicAdd(&acc[4], punct); atomicAdd(&acc[5], special);
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int nn = acc[0];
    const float den = (float)(nn > 1 ? nn : 1);
    float v = 0.f;
    if (nn > 0) {
      switch (threadIdx.x) {
        case 0: v = (float)nn / (float)a.max_length; break;
        case 1: v = (float)acc[1] / den; break;
        case 2: v = (float)nn / (float)(acc[3] + 1); break;
        case 3: v = (float)acc[2]; break;
        case 4: v = (float)acc[4] / den; break;
        case 5: v = (float)acc[5] / den; break;
        default: break;
      }
    }
    a.out[(long long)b * a.ld_out + threadIdx.x] = v;
  }
}

// ------------------------------------------------------------------------------------------------ host checks
unsigned row_grid(long long rows) {
  long long g = (rows + 3) / 4;
  return (unsigned)(g > 2048 ? 2048 : g);
}

int check_embed(const mmdeer_token_embed_args* a, bool bwd) {
  const char* op = bwd ? "token_embed_bwd" : "token_embed_fwd";
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->B >= 0 && a->L >= 0, "%s: bad shape B=%d L=%d", op, a->B, a->L);
  MMDEER_CHECK(a->width == TOK_E, "%s: width must be %d (got %d)", op, TOK_E, a->width);
  if (a->B == 0 || a->L == 0) return 0;
  const int el = a->act_f32 ? 4 : 8;
  const bool tables = bwd ? (a->d_emb || a->d_pos) : (a->emb || a->pos);
  MMDEER_CHECK(a->mask, "%s: NULL pointer (mask)", op);
  MMDEER_CHECK(al4(a->mask), "%s: misaligned pointer (mask)", op);
  if (!bwd) {
    MMDEER_CHECK(a->x, "%s: NULL pointer (x)", op);
    MMDEER_CHECK(a->ld_x >= TOK_E, "%s: leading dimension too small (ld_x=%d)", op, a->ld_x);
    MMDEER_CHECK(al16(a->x) && a->ld_x % el == 0, "%s: misaligned pointer or leading dimension (x rows need 16 bytes)", op);
    if (tables) {
      MMDEER_CHECK(a->emb && a->pos && a->ids && a->ids32, "%s: NULL pointer (emb, pos, ids, ids32 go together)", op);
      MMDEER_CHECK(!a->src, "%s: either the tables or src, not both", op);
      MMDEER_CHECK(a->V >= 1 && a->V < (1 << 24) && a->P >= 1, "%s: need 1 <= V < 2^24 and P >= 1 (V=%d P=%d)", op, a->V, a->P);
      MMDEER_CHECK(al16(a->emb) && al16(a->pos) && al8(a->ids) && al4(a->ids32), "%s: misaligned pointer (emb, pos, ids, ids32)", op);
    } else {
      MMDEER_CHECK(a->src, "%s: NULL pointer (the tables or src)", op);
      MMDEER_CHECK(a->ld_src >= TOK_E, "%s: leading dimension too small (ld_src=%d)", op, a->ld_src);
      MMDEER_CHECK(al16(a->src) && a->ld_src % 4 == 0, "%s: misaligned pointer or leading dimension (src rows need 16 bytes)", op);
    }
  } else {
    MMDEER_CHECK(a->dx, "%s: NULL pointer (dx)", op);
    MMDEER_CHECK(a->ld_dx >= TOK_E, "%s: leading dimension too small (ld_dx=%d)", op, a->ld_dx);
    MMDEER_CHECK(al16(a->dx) && a->ld_dx % el == 0, "%s: misaligned pointer or leading dimension (dx rows need 16 bytes)", op);
    if (tables) {
      MMDEER_CHECK(a->d_emb && a->d_pos && a->ids32 && a->scratch, "%s: NULL pointer (d_emb, d_pos, ids32, scratch go together)", op);
      MMDEER_CHECK(!a->d_src, "%s: either the table gradients or d_src, not both", op);
      MMDEER_CHECK(a->V >= 1 && a->V < (1 << 24) && a->P >= 1, "%s: need 1 <= V < 2^24 and P >= 1 (V=%d P=%d)", op, a->V, a->P);
      MMDEER_CHECK((long long)a->B * a->L <= TOK_MAX_ROWS, "%s: B * L = %lld is above the limit of %lld rows (the stable sort's)", op,
                   (long long)a->B * a->L, TOK_MAX_ROWS);
      MMDEER_CHECK(al16(a->d_emb) && al16(a->d_pos) && al4(a->ids32) && al16(a->scratch), "%s: misaligned pointer (d_emb, d_pos, ids32, scratch)", op);
      MMDEER_CHECK(a->scratch_bytes >= mmdeer_token_embed_bwd_scratch((long long)a->B * a->L), "%s: scratch of %lld bytes, %lld needed", op,
                   a->scratch_bytes, mmdeer_token_embed_bwd_scratch((long long)a->B * a->L));
    } else {
      MMDEER_CHECK(a->d_src, "%s: NULL pointer (the table gradients or d_src)", op);
      MMDEER_CHECK(a->ld_dsrc >= TOK_E, "%s: leading dimension too small (ld_dsrc=%d)", op, a->ld_dsrc);
      MMDEER_CHECK(al16(a->d_src) && a->ld_dsrc % 4 == 0, "%s: misaligned pointer or leading dimension (d_src rows need 16 bytes)", op);
    }
  }
  return 0;
}

int check_tpool(const mmdeer_token_pool_args* a, bool bwd) {
  const char* op = bwd ? "token_pool_bwd" : "token_pool_fwd";
  MMDEER_CHECK(a, "%s: NULL argument struct", op);
  MMDEER_CHECK(a->B >= 0 && a->L >= 0, "%s: bad shape B=%d L=%d", op, a->B, a->L);
  MMDEER_CHECK(a->width == TOK_E && a->att_width == TOK_A, "%s: widths must be %d and %d (got %d and %d)", op, TOK_E, TOK_A, a->width, a->att_width);
  if (a->B == 0 || a->L == 0) return 0;
  const int el = a->act_f32 ? 4 : 8;
  MMDEER_CHECK(a->x && a->z && a->mask && a->w2 && a->weights, "%s: NULL pointer (x, z, mask, w2, weights)", op);
  MMDEER_CHECK(a->ld_x >= TOK_E && a->ld_z >= TOK_A, "%s: leading dimensions too small (ld_x=%d ld_z=%d)", op, a->ld_x, a->ld_z);
  MMDEER_CHECK(al16(a->x) && al16(a->z) && al16(a->w2) && al4(a->mask) && al4(a->weights) && al4(a->probs) && a->ld_x % el == 0 && a->ld_z % el == 0,
               "%s: misaligned pointer or leading dimension (x, z, w2, mask, weights, probs)", op);
  if (!bwd) {
    MMDEER_CHECK(a->b2 && a->attended, "%s: NULL pointer (b2, attended)", op);
    MMDEER_CHECK(a->ld_att >= TOK_E, "%s: leading dimensions too small (ld_att=%d)", op, a->ld_att);
    MMDEER_CHECK(al16(a->attended) && al4(a->b2) && a->ld_att % el == 0, "%s: misaligned pointer or leading dimension (attended, b2)", op);
  } else {
    MMDEER_CHECK(a->probs && a->dout && a->dx && a->dz && a->dw2 && a->db2 && a->scratch, "%s: NULL pointer (probs, dout, dx, dz, dw2, db2, scratch)", op);
    MMDEER_CHECK(a->ld_dout >= TOK_E && a->ld_dx >= TOK_E && a->ld_dz >= TOK_A, "%s: leading dimensions too small (ld_dout=%d ld_dx=%d ld_dz=%d)", op,
                 a->ld_dout, a->ld_dx, a->ld_dz);
    MMDEER_CHECK(al16(a->dout) && al16(a->dx) && al16(a->dz) && al16(a->scratch) && al4(a->dw2) && al4(a->db2) && a->ld_dout % el == 0 &&
                 a->ld_dx % el == 0 && a->ld_dz % el == 0, "%s: misaligned pointer or leading dimension (dout, dx, dz, scratch, dw2, db2)", op);
  }
  return 0;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

long long mmdeer_token_embed_bwd_scratch(long long rows) {
  if (rows <= 0 || rows > TOK_MAX_ROWS) return 0;
  const long long r16 = (rows + 3) / 4 * 4;                 // fp32 keys and int32 order, each padded to 16 bytes
  return r16 * 4 * 2 + mmdeer_sort_pairs_scratch(rows);
}

int mmdeer_token_embed_fwd(const mmdeer_token_embed_args* a) {
  if (check_embed(a, false) != 0) return -1;
  if (a->B == 0 || a->L == 0) return 0;
  const long long rows = (long long)a->B * a->L;
  MMDEER_LAUNCH_ACT(token_embed_fwd_kernel, a->act_f32, dim3(row_grid(rows)), dim3(256), (hipStream_t)a->stream, *a, rows);
  return 0;
}

int mmdeer_token_embed_bwd(const mmdeer_token_embed_args* a) {
  if (check_embed(a, true) != 0) return -1;
  if (a->B == 0 || a->L == 0) return 0;
  const long long rows = (long long)a->B * a->L;
  hipStream_t st = (hipStream_t)a->stream;
  if (a->d_src) {
    MMDEER_LAUNCH_ACT(token_embed_dsrc_kernel, a->act_f32, dim3(row_grid(rows)), dim3(256), st, *a, rows);
    return 0;
  }
  MMDEER_LAUNCH_ACT(token_embed_dpos_kernel, a->act_f32, dim3(a->P), dim3(256), st, *a);
  const long long r16 = (rows + 3) / 4 * 4;
  float* keys = (float*)a->scratch;
  int* order = (int*)(keys + r16);
  void* sorted = (void*)(order + r16);
  MMDEER_HIP(hipMemsetAsync(a->d_emb, 0, (size_t)a->V * TOK_E * sizeof(float), st));
  const long long kg = (rows + 255) / 256;
  hipLaunchKernelGGL(token_embed_keys_kernel, dim3((unsigned)(kg > 2048 ? 2048 : kg)), dim3(256), 0, st, a->ids32, a->mask, rows, a->V, keys);
  MMDEER_HIP(hipGetLastError());
  TRY(mmdeer_sort_pairs(keys, 1, rows, order, sorted, mmdeer_sort_pairs_scratch(rows), a->stream));
  MMDEER_LAUNCH_ACT(token_embed_demb_kernel, a->act_f32, dim3(row_grid(rows)), dim3(256), st, *a, (const unsigned long long*)sorted, rows);
  return 0;
}

int mmdeer_token_pool_fwd(const mmdeer_token_pool_args* a) {
  if (check_tpool(a, false) != 0) return -1;
  if (a->B == 0 || a->L == 0) return 0;
  MMDEER_LAUNCH_ACT(token_pool_fwd_kernel, a->act_f32, dim3(a->B), dim3(256), (hipStream_t)a->stream, *a);
  return 0;
}

int mmdeer_token_pool_bwd(const mmdeer_token_pool_args* a) {
  if (check_tpool(a, true) != 0) return -1;
  if (a->B == 0 || a->L == 0) return 0;
  const int nwg = a->B < TOK_POOL_BWD_WG ? a->B : TOK_POOL_BWD_WG;
  MMDEER_LAUNCH_ACT(token_pool_bwd_kernel, a->act_f32, dim3(nwg), dim3(256), (hipStream_t)a->stream, *a);
  hipLaunchKernelGGL(fold_wg_partials_kernel<TOK_A>, dim3(1), dim3(TOK_A), 0, (hipStream_t)a->stream, a->scratch, nwg, a->dw2, a->db2);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_token_stats(const mmdeer_token_stats_args* a) {
  MMDEER_CHECK(a, "token_stats: NULL argument struct");
  MMDEER_CHECK(a->B >= 0 && a->L >= 0, "token_stats: bad shape B=%d L=%d", a->B, a->L);
  MMDEER_CHECK(a->L <= TOK_STATS_MAX_L, "token_stats: L = %d is above the limit of %d tokens (the ids of a sample are held in LDS)", a->L, TOK_STATS_MAX_L);
  if (a->B == 0 || a->L == 0) return 0;
  MMDEER_CHECK(a->ids && a->mask && a->out, "token_stats: NULL pointer (ids, mask, out)");
  MMDEER_CHECK(a->max_length >= 1, "token_stats: max_length must be >= 1 (got %d)", a->max_length);
  MMDEER_CHECK(a->ld_out >= 16, "token_stats: leading dimension too small (ld_out=%d)", a->ld_out);
  MMDEER_CHECK(al4(a->ids) && al4(a->mask) && al4(a->out), "token_stats: misaligned pointer (ids, mask, out)");
  hipLaunchKernelGGL(token_stats_kernel, dim3(a->B), dim3(256), 0, (hipStream_t)a->stream, *a);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
