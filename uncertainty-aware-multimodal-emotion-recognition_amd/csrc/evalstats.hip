// mmdeer -- on-device statistics of the DEER evaluator (reference src/training/evaluation.py:135-355, 492-530, 578-682):
// the streaming CCC / Pearson / MAE / RMSE sums and the quantile-binned calibration error of the validation loop, bootstrap
// moments and percentile intervals, a stable sort with tie-averaged ranks (Spearman), the bin tables of the evaluator's
// calibration error, and the table UncertaintyAnalyzer (:358-482) is computed from.  The (N, D) prediction / target /
// uncertainty arrays stay in HBM; what reaches the host is ci[D][2], a few moment sums and the bin tables.  Every reduction
// has a fixed partition and a fixed-order fold and uses no floating-point atomics: two launches on the same inputs give
// bit-identical results.
#include "common.h"

namespace mmdeer {
namespace {

// ---- shared by the kernels below: block fold, float image, order-statistic selection -------------------------------------------
// Fixed-order LDS tree over the 256 lanes of a workgroup, `rows` rows in the same steps: lane tid adds lane tid + off for
// off = 128, 64, ..., 1, so a sum has the same bits whatever else is folded next to it.  Row k's sum is in sm[k][0] afterwards.
// Opens with a barrier (the callers' writes need none of their own) and ends behind one.
__device__ __forceinline__ void tree_sum_256(double (*sm)[256], int rows, int tid) {
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off)
      for (int k = 0; k < rows; ++k) sm[k][tid] += sm[k][tid + off];
    __syncthreads();
  }
}
// The row count at compile time (unrolled).  NM > 0: the NM rows of float extrema in sf, which the caller must then pass, are
// folded in the same steps -- even rows as minima, odd rows as maxima, so they come in (min, max) pairs.
template <int NS, int NM = 0>
__device__ __forceinline__ void tree_sum_256(double (*sm)[256], int tid, float (*sf)[256] = nullptr) {
  static_assert(NS >= 1 && NM >= 0 && NM % 2 == 0, "rows of sums, and (min, max) pairs of extrema");
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int k = 0; k < NS; ++k) sm[k][tid] += sm[k][tid + off];
#pragma unroll
      for (int k = 0; k < NM; ++k) sf[k][tid] = (k & 1) ? fmaxf(sf[k][tid], sf[k][tid + off]) : fminf(sf[k][tid], sf[k][tid + off]);
    }
    __syncthreads();
  }
}

// order-preserving image of a float in the unsigned integers (-inf < ... < -0.0 < +0.0 < ... < +inf; NaN by its bits), and back
__device__ __forceinline__ unsigned float_image(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float image_float(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// The k-th smallest (k from 0) of the 32-bit keys of elements [0, n), by a workgroup of 256 lanes: 4 passes of 8 bits over integer
// histograms -- exact and deterministic.  key(i, out) writes element i's key and returns true, or returns false to skip i; k must
// be below the number of elements it keeps.  Every lane returns the selected key.
struct RadixScratch {
  unsigned hist[256];
  unsigned digit;
  long long k;
};
template <typename KeyFn>
__device__ __forceinline__ unsigned radix_select_256(long long n, long long k, RadixScratch& rs, int tid, KeyFn key) {
  unsigned prefix = 0u, mask = 0u;
  for (int pass = 3; pass >= 0; --pass) {
    const int shift = 8 * pass;
    rs.hist[tid] = 0u;
    __syncthreads();
    for (long long i = tid; i < n; i += 256) {
      unsigned x;
      if (!key(i, x)) continue;
      if ((x & mask) == prefix) atomicAdd(&rs.hist[(x >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      long long cum = 0;
      unsigned d = 0;
      for (; d < 255u; ++d) {
        if (k < cum + (long long)rs.hist[d]) break;
        cum += rs.hist[d];
      }
      rs.digit = d; rs.k = k - cum;
    }
    __syncthreads();
    prefix |= rs.digit << shift; mask |= 255u << shift; k = rs.k;
    __syncthreads();
  }
  return prefix;
}

// ---- streaming evaluation statistics (reference src/utils/metrics.py:59-125, src/training/training.py:
//      316-353): per emotion dimension the sufficient statistics of CCC / Pearson / MAE / RMSE, accumulated in fp64
//      across validation batches, so the (N, 3) prediction arrays never travel to the host.
//      acc[d][8] += {n, sum p, sum t, sum p^2, sum t^2, sum p t, sum |p - t|, sum (p - t)^2} over the rows where neither
//      value is NaN (the reference masks them).  Block 3 writes the per-sample mean |error| and mean uncertainty that
//      the quantile-binned calibration error needs (2 floats per sample instead of 9).
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const float* pred, const float* target, const float* unc,
                                                              double* acc, float* sample_err, float* sample_unc, int B) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 3) {
    if (!sample_err && !sample_unc) return;
    for (int b = tid; b < B; b += 256) {
      float e = 0.f, u = 0.f;
      for (int d = 0; d < 3; ++d) {
        e += fabsf(pred[b * 3 + d] - target[b * 3 + d]);
        if (unc) u += unc[b * 3 + d];
      }
      if (sample_err) sample_err[b] = e / 3.f;
      if (sample_unc) sample_unc[b] = u / 3.f;
    }
    return;
  }
  __shared__ double sm[8][256];
  const int d = blockIdx.x;
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int b = tid; b < B; b += 256) {
    const float pf = pred[b * 3 + d], tf = target[b * 3 + d];
    if (pf != pf || tf != tf) continue;
    const double p = pf, t = tf, e = p - t;
    s[0] += 1.0; s[1] += p; s[2] += t; s[3] += p * p; s[4] += t * t; s[5] += p * t; s[6] += fabs(e); s[7] += e * e;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) sm[k][tid] = s[k];
  tree_sum_256<8>(sm, tid);
  if (tid < 8) acc[d * 8 + tid] += sm[tid][0];   // calls on one stream are ordered: a plain read-modify-write
}

// ---- quantile-binned calibration error (reference src/utils/metrics.py:214-279) on per-sample device arrays --------------
// The reference bins the per-sample mean uncertainty by its own quantiles (np.quantile, linear interpolation) and compares,
// per bin, mean(1 - uncertainty) with mean(1 - error).  Two launches keep it on the device: an exact order-statistic
// selection for the 2 (nq) ranks np.quantile interpolates between, and the bin sums against the edges the host derives from
// those 2 nq values.  A sample counts when its error and uncertainty are not NaN and the uncertainty is finite (:243).
__device__ __forceinline__ bool ece_valid(float e, float u) { return e == e && u == u && fabsf(u) != __builtin_inff(); }

// block b: quantile r = b >> 1 (q_r = linspace(0, 1, nq)[r]), neighbour (b & 1): the floor(q (n - 1))-th smallest valid
// uncertainty or the one after it, by a 4-pass radix selection (8 bits per pass, integer histograms: exact, deterministic)
__global__ __launch_bounds__(256) void eval_quantile_select_kernel(const float* err, const float* unc, long long n, int nq,
                                                                   float* vals, double* frac, long long* nvalid) {
  __shared__ RadixScratch rs;
  __shared__ unsigned long long s_cnt;
  const int tid = threadIdx.x, r = blockIdx.x >> 1, which = blockIdx.x & 1;
  if (tid == 0) s_cnt = 0ull;
  __syncthreads();
  unsigned long long c = 0;
  for (long long i = tid; i < n; i += 256) c += ece_valid(err[i], unc[i]) ? 1ull : 0ull;
  atomicAdd(&s_cnt, c);
  __syncthreads();
  const long long nv = (long long)s_cnt;
  if (nv == 0) {
    if (tid == 0) { vals[2 * r + which] = 0.f; if (!which) { frac[r] = 0.0; if (r == 0) *nvalid = 0; } }
    return;
  }
  const double q = (r == nq - 1) ? 1.0 : (double)r * (1.0 / (double)(nq - 1));      // np.linspace(0, 1, nq)[r]
  const double virt = q * (double)(nv - 1);                                        // np.quantile, method 'linear'
  const long long lo = (long long)floor(virt);
  const long long k = which ? (lo + 1 < nv ? lo + 1 : nv - 1) : lo;
  const unsigned sel = radix_select_256(n, k, rs, tid, [&](long long i, unsigned& key) {
    const float u = unc[i];
    key = float_image(u);
    return ece_valid(err[i], u);
  });
  if (tid == 0) {
    vals[2 * r + which] = image_float(sel);
    if (!which) { frac[r] = virt - (double)lo; if (r == 0) *nvalid = nv; }
  }
}

// bins[i] = {count, sum (1 - u), sum (1 - e)} over the valid samples with edges[i] <= u < edges[i + 1] (nb <= 16).  One
// workgroup, per-thread accumulators in LDS, fixed-order tree reduction: deterministic.
constexpr int ECE_MAX_BINS = 16;
__global__ __launch_bounds__(256) void eval_ece_bins_kernel(const float* err, const float* unc, long long n, const double* edges,
                                                            int nb, double* bins) {
  __shared__ double sm[ECE_MAX_BINS * 3][256];
  __shared__ double ed[ECE_MAX_BINS + 1];
  const int tid = threadIdx.x;
  if (tid <= nb) ed[tid] = edges[tid];
  for (int j = 0; j < nb * 3; ++j) sm[j][tid] = 0.0;
  __syncthreads();
  for (long long i = tid; i < n; i += 256) {
    const float e = err[i], uf = unc[i];
    if (!ece_valid(e, uf)) continue;
    const double u = (double)uf;
    for (int b = 0; b < nb; ++b) {
      if (u >= ed[b] && u < ed[b + 1]) {
        sm[3 * b][tid] += 1.0; sm[3 * b + 1][tid] += 1.0 - u; sm[3 * b + 2][tid] += 1.0 - (double)e;
        break;
      }
    }
  }
  tree_sum_256(sm, nb * 3, tid);
  if (tid < nb * 3) bins[tid] = sm[tid][0];
}

// ---- bootstrap draws: integer-only, restated bit for bit in mmdeer/synth.py (bootstrap_indices) --------------------------
__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned long long boot_key(unsigned long long seed, unsigned r) {
  return splitmix64(seed + (unsigned long long)r * 0xD1B54A32D192ED03ull);
}
// row drawn by replicate key `key` at draw i: the high 32 bits of the hash scaled to [0, N) (stays inside 64 bits, N < 2^32)
__device__ __forceinline__ unsigned boot_index(unsigned long long key, unsigned long long i, unsigned N) {
  return (unsigned)(((splitmix64(key + i) >> 32) * (unsigned long long)N) >> 32);
}

constexpr int BOOT_MAX_SPLIT = 64;     // workgroups per replicate, at most
constexpr int BOOT_SPLIT_DRAWS = 8192; // draws per workgroup the split aims at
__host__ __forceinline__ int boot_split(long long N) {   // a function of N alone: the partition never depends on the device
  long long s = (N + BOOT_SPLIT_DRAWS - 1) / BOOT_SPLIT_DRAWS;
  return (int)(s < 1 ? 1 : (s > BOOT_MAX_SPLIT ? BOOT_MAX_SPLIT : s));
}

// one 32-byte row per sample: (p0, t0, p1, t1 | p2, t2, -, -); a draw is two aligned 16-byte reads that serve all dimensions.
// Dimensions >= D hold NaN, which the accumulation skips like any NaN pair.
__global__ __launch_bounds__(256) void boot_repack_kernel(const float* pred, const float* target, int N, int D, float4* table) {
  const float nan = __builtin_nanf("");
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
    float v[6];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      v[2 * d] = d < D ? pred[i * D + d] : nan;
      v[2 * d + 1] = d < D ? target[i * D + d] : nan;
    }
    table[2 * i] = make_float4(v[0], v[1], v[2], v[3]);
    table[2 * i + 1] = make_float4(v[4], v[5], 0.f, 0.f);
  }
}

struct BootAcc {
  double s[6];             // n, sum p, sum t, sum p^2, sum t^2, sum pt
  float pmin, pmax, tmin, tmax;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = 0.0;
    pmin = tmin = __builtin_inff(); pmax = tmax = -__builtin_inff();
  }
  __device__ __forceinline__ void add(float pf, float tf) {
    if (pf != pf || tf != tf) return;
    const double p = pf, t = tf;
    s[0] += 1.0; s[1] += p; s[2] += t; s[3] += p * p; s[4] += t * t; s[5] += p * t;
    pmin = fminf(pmin, pf); pmax = fmaxf(pmax, pf); tmin = fminf(tmin, tf); tmax = fmaxf(tmax, tf);
  }
};

// workgroup (r, s): draws [s * per, (s + 1) * per) of replicate r, draw i on lane (i - first) % 256; fixed-order LDS tree.
// part[r][s][3][6], mm[r][s][3][4] = {min p, max p, min t, max t} of the drawn valid values.
__global__ __launch_bounds__(256) void boot_partial_kernel(const float4* __restrict__ table, int N, int S, unsigned long long seed,
                                                           double* part, float* mm) {
  __shared__ double sm[18][256];
  __shared__ float sf[12][256];
  const int tid = threadIdx.x, r = blockIdx.x, s = blockIdx.y;
  const unsigned long long key = boot_key(seed, (unsigned)r);
  const long long per = ((long long)N + S - 1) / S;
  const long long i0 = (long long)s * per;
  long long i1 = i0 + per;
  if (i1 > N) i1 = N;
  BootAcc a[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) a[d].init();
  long long i = i0 + tid;
  // four draws of a lane in flight at once (eight independent 16-byte reads); they are added in draw order all the same
  for (; i + 3 * 256 < i1; i += 4 * 256) {
    float4 x[4], y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const unsigned j = boot_index(key, (unsigned long long)(i + u * 256), (unsigned)N);
      x[u] = table[2 * (size_t)j]; y[u] = table[2 * (size_t)j + 1];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { a[0].add(x[u].x, x[u].y); a[1].add(x[u].z, x[u].w); a[2].add(y[u].x, y[u].y); }
  }
  for (; i < i1; i += 256) {
    const unsigned j = boot_index(key, (unsigned long long)i, (unsigned)N);
    const float4 x = table[2 * (size_t)j], y = table[2 * (size_t)j + 1];
    a[0].add(x.x, x.y); a[1].add(x.z, x.w); a[2].add(y.x, y.y);
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sm[d * 6 + k][tid] = a[d].s[k];
    sf[d * 4][tid] = a[d].pmin; sf[d * 4 + 1][tid] = a[d].pmax; sf[d * 4 + 2][tid] = a[d].tmin; sf[d * 4 + 3][tid] = a[d].tmax;
  }
  tree_sum_256<18, 12>(sm, tid, sf);
  const size_t base = (size_t)r * S + s;
  if (tid < 18) part[base * 18 + tid] = sm[tid][0];
  if (tid >= 64 && tid < 76) mm[base * 12 + (tid - 64)] = sf[tid - 64][0];
}

// mom[r][d][6] = the S partial sums added in order s = 0, 1, ...; flags[r][d]: bit 0 the drawn valid p are all equal, bit 1
// the same for t, bit 2 both and the two constants are equal (the CCC's denominator is then exactly zero).
__global__ __launch_bounds__(64) void boot_fold_kernel(const double* part, const float* mm, int S, int D, double* mom, int* flags) {
  const int tid = threadIdx.x, r = blockIdx.x;
  if (tid < 18) {
    const int d = tid / 6, k = tid % 6;
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += part[((size_t)r * S + s) * 18 + tid];
    if (d < D) mom[((size_t)r * D + d) * 6 + k] = v;
  } else if (tid >= 32 && tid < 32 + D) {
    const int d = tid - 32;
    float pmin = __builtin_inff(), pmax = -__builtin_inff(), tmin = __builtin_inff(), tmax = -__builtin_inff();
    for (int s = 0; s < S; ++s) {
      const float* m = mm + ((size_t)r * S + s) * 12 + d * 4;
      pmin = fminf(pmin, m[0]); pmax = fmaxf(pmax, m[1]); tmin = fminf(tmin, m[2]); tmax = fmaxf(tmax, m[3]);
    }
    const int pc = pmin == pmax, tc = tmin == tmax;
    flags[(size_t)r * D + d] = pc | (tc << 1) | ((pc && tc && pmin == tmin) << 2);
  }
}

// ---- bootstrap intervals: metric per replicate, NaN dropped, sort, np.percentile (linear) ------------------------------------
constexpr int CI_MAX_R = 4096;
enum { METRIC_CCC = 0, METRIC_PEARSON = 1 };

// the value the reference's metric function returns for one replicate (evaluation.py:617-622, 656-682; scipy.stats.pearsonr
// is NaN for a constant sample and raises for fewer than two values, which the caller drops like a NaN)
__device__ double boot_metric(const double* m, int flag, int N, int metric) {
  const double nan = __builtin_nan("");
  const double n = m[0];
  if (metric == METRIC_CCC) {
    if (n < 2.0) return 0.0;
  } else {
    if (n < (double)N || N < 2) return nan;    // a drawn NaN row is not masked on this path: pearsonr returns NaN
  }
  const bool is_const = (flag & 3) != 0;
  if (metric == METRIC_CCC && (flag & 4)) return 0.0;     // both constant and equal: the denominator is exactly 0
  if (is_const) return nan;
  const double mp = m[1] / n, mt = m[2] / n;
  const double vp = m[3] / n - mp * mp, vt = m[4] / n - mt * mt, cov = m[5] / n - mp * mt;
  double rho = cov / sqrt(vp * vt);
  if (rho > 1.0) rho = 1.0;
  if (rho < -1.0) rho = -1.0;
  if (metric != METRIC_CCC) return rho;
  const double den = vp + vt + (mp - mt) * (mp - mt);
  if (den == 0.0) return 0.0;
  return 2.0 * rho * sqrt(vt * vp) / den;
}

// numpy's _lerp (np.percentile, method 'linear'), without contraction into fused multiply-adds
__device__ __forceinline__ double np_lerp(double a, double b, double t) {
  const double d = __dsub_rn(b, a);
  double r = __dadd_rn(a, __dmul_rn(d, t));
  if (t >= 0.5) r = __dsub_rn(b, __dmul_rn(d, __dsub_rn(1.0, t)));
  return d == 0.0 ? a : r;
}
__device__ double np_percentile_sorted(const double* v, int n, double q) {
  const double virt = __dmul_rn((double)(n - 1), q);
  int lo = (int)floor(virt);
  if (lo > n - 1) lo = n - 1;
  if (lo < 0) lo = 0;
  const int hi = lo + 1 < n ? lo + 1 : n - 1;
  return np_lerp(v[lo], v[hi], __dsub_rn(virt, (double)lo));
}
// The same two steps for a caller that fetches the two order statistics itself, with contraction switched off: the _rn
// intrinsics above are plain operators to this compiler, which may fuse a product into the sum that follows, and
// fma(10, 0.95, -9) is 0.49999999999999956 where numpy has 0.5.  Results equal to np.percentile bit for bit need every
// product rounded first.
__device__ __forceinline__ double np_percentile_position(int n, double q, int* lo_out, int* hi_out) {
#pragma clang fp contract(off)
  const double virt = (double)(n - 1) * q;
  int lo = (int)floor(virt);
  if (lo > n - 1) lo = n - 1;
  if (lo < 0) lo = 0;
  *lo_out = lo;
  *hi_out = lo + 1 < n ? lo + 1 : n - 1;
  return virt - (double)lo;
}
__device__ __forceinline__ double np_lerp_strict(double a, double b, double t) {
#pragma clang fp contract(off)
  const double d = b - a;
  double r = a + d * t;
  if (t >= 0.5) r = b - d * (1.0 - t);
  return d == 0.0 ? a : r;
}

// one workgroup per dimension: R <= 4096 replicate values in LDS, NaN replaced by +inf (sorted to the end and not counted),
// bitonic sort, the two percentiles over the nkept values that remain
__global__ __launch_bounds__(256) void boot_ci_kernel(const double* mom, const int* flags, int N, int D, int R, int metric, double q_lo,
                                                      double q_hi, double* ci, int* nkept) {
  __shared__ double v[CI_MAX_R];
  __shared__ int cnt[256];
  const int tid = threadIdx.x, d = blockIdx.x;
  int P = 1;
  while (P < R) P <<= 1;
  int c = 0;
  for (int r = tid; r < P; r += 256) {
    double x = __builtin_inf();
    if (r < R) {
      const double val = boot_metric(mom + ((size_t)r * D + d) * 6, flags[(size_t)r * D + d], N, metric);
      if (val == val) { x = val; ++c; }
    }
    v[r] = x;
  }
  cnt[tid] = c;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) cnt[tid] += cnt[tid + off];
    __syncthreads();
  }
  const int nk = cnt[0];
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const double a = v[i], b = v[l];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { v[i] = b; v[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    nkept[d] = nk;
    ci[2 * d] = nk ? np_percentile_sorted(v, nk, q_lo) : 0.0;
    ci[2 * d + 1] = nk ? np_percentile_sorted(v, nk, q_hi) : 0.0;
  }
}

// ---- stable sort of fp32 keys: np.argsort(kind='stable') -------------------------------------------------------------------
// Composite 64-bit keys (order-preserving image of the float) << 32 | original index, sorted ascending by a bitonic network:
// the total order (key, index) is that of a stable sort.  -0.0 and +0.0 share one image (they compare equal), every NaN maps
// to the largest image (numpy sorts NaN last, in index order).  Padding to the next power of two is all-ones.
constexpr long long SORT_MAX_N = 1ll << 20;
constexpr int SORT_TILE = 2048;        // elements one workgroup sorts / merges in LDS

__device__ __forceinline__ unsigned sort_image(float f) {
  if (f != f) return 0xFFFFFFFFu;
  return float_image(__float_as_uint(f) == 0x80000000u ? 0.f : f);
}

// blockIdx.y = column c: keys + c * col_step -> a + c * P (mmdeer_sort_pairs has one column; the network kernels alike)
__global__ __launch_bounds__(256) void sort_init_kernel(const float* keys, long long stride, long long col_step, long long n, long long P,
                                                        unsigned long long* a) {
  keys += (long long)blockIdx.y * col_step;
  a += (long long)blockIdx.y * P;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256)
    a[i] = i < n ? (((unsigned long long)sort_image(keys[i * stride]) << 32) | (unsigned long long)i) : ~0ull;
}

// all steps (k, j) with j < SORT_TILE for k from k_first to k_last, on the tile of SORT_TILE elements this workgroup owns
__global__ __launch_bounds__(256) void sort_tile_kernel(unsigned long long* a, long long P, long long k_first, long long k_last) {
  __shared__ unsigned long long t[SORT_TILE];
  const int tid = threadIdx.x;
  a += (long long)blockIdx.y * P;
  const long long base = (long long)blockIdx.x * SORT_TILE;
  const int len = (int)(P < SORT_TILE ? P : SORT_TILE);
  for (int i = tid; i < len; i += 256) t[i] = a[base + i];
  __syncthreads();
  for (long long k = k_first; k <= k_last; k <<= 1) {
    int j = (int)((k >> 1) < len ? (k >> 1) : (len >> 1));
    for (; j > 0; j >>= 1) {
      for (int i = tid; i < len; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = t[i], y = t[l];
          const bool up = ((base + i) & k) == 0;
          if ((x > y) == up) { t[i] = y; t[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < len; i += 256) a[base + i] = t[i];
}

// one step (k, j) with j >= SORT_TILE in global memory
__global__ __launch_bounds__(256) void sort_step_kernel(unsigned long long* a, long long P, long long k, long long j) {
  a += (long long)blockIdx.y * P;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < P; i += (long long)gridDim.x * 256) {
    const long long l = i ^ j;
    if (l > i) {
      const unsigned long long x = a[i], y = a[l];
      const bool up = (i & k) == 0;
      if ((x > y) == up) { a[i] = y; a[l] = x; }
    }
  }
}

__global__ __launch_bounds__(256) void sort_order_kernel(const unsigned long long* a, long long n, int* order) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    order[i] = (int)(unsigned)(a[i] & 0xFFFFFFFFull);
}

// tie-averaged 1-based ranks (scipy.stats.rankdata, 'average'): position k of the sorted array belongs to the run of equal
// key images [lo, hi), found by two binary searches; its rank is the mean of lo + 1 .. hi.  NaN keys form one run at the end.
__global__ __launch_bounds__(256) void average_ranks_kernel(const unsigned long long* a, long long n, double* ranks) {
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long long)gridDim.x * 256) {
    const unsigned long long e = a[k];
    const unsigned img = (unsigned)(e >> 32);
    long long lo = 0, hi = k;                 // first position whose image is >= img
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((unsigned)(a[mid] >> 32) < img) lo = mid + 1; else hi = mid;
    }
    const long long first = lo;
    lo = k + 1; hi = n;                       // first position whose image is > img
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if ((unsigned)(a[mid] >> 32) <= img) lo = mid + 1; else hi = mid;
    }
    ranks[(unsigned)(e & 0xFFFFFFFFull)] = 0.5 * (double)(first + 1 + lo);
  }
}

// out[3] = {sum a'^2, sum b'^2, sum a'b'} of the ranks centred by (n + 1) / 2: one workgroup, fixed order
__global__ __launch_bounds__(256) void rank_moments_kernel(const double* ra, const double* rb, long long n, double* out) {
  __shared__ double sm[3][256];
  const int tid = threadIdx.x;
  const double c = 0.5 * (double)(n + 1);
  double s[3] = {0.0, 0.0, 0.0};
  for (long long i = tid; i < n; i += 256) {
    const double x = ra[i] - c, y = rb[i] - c;
    s[0] += x * x; s[1] += y * y; s[2] += x * y;
  }
  for (int k = 0; k < 3; ++k) sm[k][tid] = s[k];
  tree_sum_256<3>(sm, tid);
  if (tid < 3) out[tid] = sm[tid][0];
}

// ---- calibration bins of CalibrationAnalyzer.compute_ece (evaluation.py:492-530) -------------------------------------------
constexpr int CAL_MAX_BINS = 32;
constexpr int CAL_STATS = 4;   // per dimension: {max uncertainty, error threshold, bad flag, threshold is NaN}

// workgroup (d, which): which = 0, 1 -> the two middle order statistics of |p - t| by a 4-pass radix selection (8 bits per
// pass, integer histograms: exact); which = 2 -> max of unc and the "non-finite uncertainty" flag.  sel[d][4] (floats)
__global__ __launch_bounds__(256) void cal_select_kernel(const float* pred, const float* target, const float* unc, long long n, int D,
                                                         float* sel) {
  __shared__ RadixScratch rs;
  __shared__ float fm[256];
  __shared__ unsigned s_bad;
  const int tid = threadIdx.x, d = blockIdx.x, which = blockIdx.y;
  if (which == 2) {
    float m = -__builtin_inff();
    unsigned bad = 0u;
    for (long long i = tid; i < n; i += 256) {
      const float u = unc[i * D + d];
      if (u != u || fabsf(u) == __builtin_inff()) bad = 1u; else m = fmaxf(m, u);
    }
    fm[tid] = m;
    if (tid == 0) s_bad = 0u;
    __syncthreads();
    if (bad) atomicOr(&s_bad, 1u);
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) fm[tid] = fmaxf(fm[tid], fm[tid + off]);
      __syncthreads();
    }
    if (tid == 0) { sel[d * 4 + 2] = fm[0]; sel[d * 4 + 3] = s_bad ? 1.f : 0.f; }
    return;
  }
  // a NaN error makes np.median NaN: mark it by a NaN order statistic
  if (tid == 0) s_bad = 0u;
  __syncthreads();
  unsigned bad = 0u;
  for (long long i = tid; i < n; i += 256) {
    const float e = fabsf(pred[i * D + d] - target[i * D + d]);
    if (e != e) bad = 1u;
  }
  if (bad) atomicOr(&s_bad, 1u);
  __syncthreads();
  if (s_bad) {
    if (tid == 0) sel[d * 4 + which] = __builtin_nanf("");
    return;
  }
  const unsigned sel_key = radix_select_256(n, which ? n / 2 : (n - 1) / 2, rs, tid, [&](long long i, unsigned& key) {
    key = float_image(fabsf(pred[i * D + d] - target[i * D + d]));
    return true;
  });
  if (tid == 0) sel[d * 4 + which] = image_float(sel_key);
}

// workgroup (d, rule * nb + b): {count, sum conf, sum acc} of bin b under rule 0 ([lo, hi), last bin closed: the reference's
// weights) or rule 1 ((lo, hi], first bin closed below: sklearn's calibration_curve).  Confidence and threshold in float32
// exactly as numpy forms them (np.max(u) + 1e-8, u / max, 1.0 - ..., np.median: all float32, division correctly rounded);
// the comparison with the float64 edges in float64.  Block (d, 0) also writes stats[d].
__global__ __launch_bounds__(256) void cal_bins_kernel(const float* pred, const float* target, const float* unc, long long n, int D,
                                                       const double* edges, int nb, const float* sel, double* stats, double* bins) {
  __shared__ double sm[3][256];
  __shared__ unsigned s_out;
  const int tid = threadIdx.x, d = blockIdx.x, rule = blockIdx.y / nb, b = blockIdx.y % nb;
  const float umax = sel[d * 4 + 2] + 1e-8f;
  const float thr = (sel[d * 4] + sel[d * 4 + 1]) / 2.0f;       // odd n: the same value twice -> itself
  const double lo = edges[b], hi = edges[b + 1];
  if (tid == 0) s_out = 0u;
  __syncthreads();
  double s[3] = {0.0, 0.0, 0.0};
  unsigned out = 0u;
  for (long long i = tid; i < n; i += 256) {
    const float cf = 1.0f - unc[i * D + d] / umax;
    const float e = fabsf(pred[i * D + d] - target[i * D + d]);
    const double c = (double)cf;
    if (!(c >= 0.0 && c <= 1.0)) out = 1u;       // calibration_curve refuses probabilities outside [0, 1]
    bool in;
    if (rule == 0) in = c >= lo && (c < hi || (b == nb - 1 && c <= hi));
    else in = (b == 0 || c > lo) && (b == nb - 1 || c <= hi);
    if (in) { s[0] += 1.0; s[1] += c; s[2] += (e <= thr) ? 1.0 : 0.0; }
  }
  if (out) atomicOr(&s_out, 1u);
  for (int k = 0; k < 3; ++k) sm[k][tid] = s[k];
  tree_sum_256<3>(sm, tid);
  if (tid < 3) bins[(((size_t)d * 2 + rule) * nb + b) * 3 + tid] = sm[tid][0];
  if (blockIdx.y == 0 && tid == 0) {
    stats[d * CAL_STATS] = (double)sel[d * 4 + 2];
    stats[d * CAL_STATS + 1] = (double)thr;
    stats[d * CAL_STATS + 2] = (sel[d * 4 + 3] != 0.f || s_out) ? 1.0 : 0.0;
    stats[d * CAL_STATS + 3] = (thr != thr) ? 1.0 : 0.0;
  }
}

// ---- uncertainty table of UncertaintyAnalyzer (evaluation.py:358-482) --------------------------------------------------------
// Per dimension, of u = unc[:, d] and e = |pred - target|[:, d] (the float32 subtraction): moments, the sums of e over the
// n_keep[k] least uncertain samples (stable ascending order of u, NaN last) and np.percentile of u.  table[d][UNC_TABLE]:
//   0 n | 1 sum u | 2 sum e | 3 sum (u - mean u)^2 | 4 sum (e - mean e)^2 | 5 sum (u - mean u)(e - mean e) | 6 mean u
//   7 population variance of u | 8 min u | 9 max u | 10 min e | 11 max e | 12 flags (1: a NaN in u, 2: a NaN in e) | 13-15 zero
//   16 + k: sum of e over the first n_keep[k] sorted positions | 32 + k: np.percentile(u, 100 levels[k]), NaN with a NaN in u
// The centred sums take a second pass over the column: with u = 1e-3 + 1e-6 x the raw sums would cancel seven digits.
constexpr int UNC_MAX_CUTS = 16;
constexpr int UNC_MAX_Q = 8;
constexpr int UNC_TABLE = 40;
constexpr int UNC_CHUNK = 2048;      // sorted positions per workgroup of the prefix gather: the partition depends on N alone
constexpr int UNC_P1 = 7;            // per workgroup of the first pass: sum u, sum e, min u, max u, min e, max e, flags
struct UncCuts {
  long long keep[UNC_MAX_CUTS];
  double q[UNC_MAX_Q];
  int n_cuts, n_q;
};
__host__ __forceinline__ int unc_chunks(long long N) { return (int)((N + UNC_CHUNK - 1) / UNC_CHUNK); }

// workgroup (s, d): rows [s * per, (s + 1) * per), row i on lane (i - first) % 256.  Minima and maxima skip NaN (fminf would
// drop it silently); the flag carries it and the last kernel writes NaN, as np.min / np.max do.
__global__ __launch_bounds__(256) void unc_sums_kernel(const float* pred, const float* target, const float* unc, int N, int D, int S,
                                                       double* part1) {
  __shared__ double sm[2][256];
  __shared__ float sf[4][256];
  __shared__ unsigned s_flags;
  const int tid = threadIdx.x, s = blockIdx.x, d = blockIdx.y;
  const int per = (N + S - 1) / S;
  const int i0 = s * per, i1 = i0 + per < N ? i0 + per : N;
  double su = 0.0, se = 0.0;
  float umin = __builtin_inff(), umax = -__builtin_inff(), emin = __builtin_inff(), emax = -__builtin_inff();
  unsigned flags = 0u;
  if (tid == 0) s_flags = 0u;
  for (int i = i0 + tid; i < i1; i += 256) {
    const float u = unc[(size_t)i * D + d];
    const float e = fabsf(pred[(size_t)i * D + d] - target[(size_t)i * D + d]);
    su += (double)u; se += (double)e;
    if (u != u) flags |= 1u; else { umin = fminf(umin, u); umax = fmaxf(umax, u); }
    if (e != e) flags |= 2u; else { emin = fminf(emin, e); emax = fmaxf(emax, e); }
  }
  sm[0][tid] = su; sm[1][tid] = se;
  sf[0][tid] = umin; sf[1][tid] = umax; sf[2][tid] = emin; sf[3][tid] = emax;
  __syncthreads();                                   // s_flags is zero for everyone
  if (flags) atomicOr(&s_flags, flags);
  tree_sum_256<2, 4>(sm, tid, sf);
  double* out = part1 + ((size_t)d * S + s) * UNC_P1;
  if (tid < 2) out[tid] = sm[tid][0];
  else if (tid < 6) out[tid] = (double)sf[tid - 2][0];
  else if (tid == 6) out[6] = (double)s_flags;
}

// the S <= 64 first-pass partials of dimension d into LDS, one lane each; folded from there in order s = 0, 1, ... by one
// lane (a fold straight from HBM would wait for one load after the other)
__device__ __forceinline__ void unc_stage_part1(const double* part1, int S, int d, int tid, double (*sp)[UNC_P1]) {
  for (int i = tid; i < S * UNC_P1; i += blockDim.x) sp[i / UNC_P1][i % UNC_P1] = part1[(size_t)d * S * UNC_P1 + i];
}
__device__ __forceinline__ double unc_fold(const double (*sp)[UNC_P1], int S, int k) {
  double v = 0.0;
  for (int s = 0; s < S; ++s) v += sp[s][k];
  return v;
}

// second pass, same partition: part2[d][s][3] = sums of (u - mean u)^2, (e - mean e)^2 and their product
__global__ __launch_bounds__(256) void unc_centred_kernel(const float* pred, const float* target, const float* unc, int N, int D, int S,
                                                          const double* part1, double* part2) {
  __shared__ double sm[3][256];
  __shared__ double sp[BOOT_MAX_SPLIT][UNC_P1];
  __shared__ double s_mean[2];
  const int tid = threadIdx.x, s = blockIdx.x, d = blockIdx.y;
  unc_stage_part1(part1, S, d, tid, sp);
  __syncthreads();
  if (tid < 2) s_mean[tid] = unc_fold(sp, S, tid) / (double)N;
  __syncthreads();
  const double mu = s_mean[0], me = s_mean[1];
  const int per = (N + S - 1) / S;
  const int i0 = s * per, i1 = i0 + per < N ? i0 + per : N;
  double a[3] = {0.0, 0.0, 0.0};
  for (int i = i0 + tid; i < i1; i += 256) {
    const double du = (double)unc[(size_t)i * D + d] - mu;
    const double de = (double)fabsf(pred[(size_t)i * D + d] - target[(size_t)i * D + d]) - me;
    a[0] += du * du; a[1] += de * de; a[2] += du * de;
  }
  for (int k = 0; k < 3; ++k) sm[k][tid] = a[k];
  tree_sum_256<3>(sm, tid);
  if (tid < 3) part2[((size_t)d * S + s) * 3 + tid] = sm[tid][0];
}

// workgroup (c, d): sorted positions [c * UNC_CHUNK, (c + 1) * UNC_CHUNK) of column d, cut by the n_keep into segments
// [n_keep[k - 1], n_keep[k]); seg[d][c][k] = the sum of e over segment k inside this chunk, e gathered through the sorted
// index.  Position pos goes to lane (pos - first of the segment here) % 256; fixed LDS tree.  A NaN error stays a NaN sum.
__global__ __launch_bounds__(256) void unc_prefix_kernel(const unsigned long long* a, long long P, const float* pred, const float* target,
                                                         int N, int D, int C, UncCuts cuts, double* seg) {
  __shared__ double sm[1][256];
  const int tid = threadIdx.x, c = blockIdx.x, d = blockIdx.y;
  const unsigned long long* ad = a + (long long)d * P;
  const long long pos0 = (long long)c * UNC_CHUNK;
  const long long pos1 = pos0 + UNC_CHUNK < N ? pos0 + UNC_CHUNK : N;
  long long lo = 0;
  for (int k = 0; k < cuts.n_cuts; ++k) {
    const long long hi = cuts.keep[k];
    const long long b0 = lo > pos0 ? lo : pos0, b1 = hi < pos1 ? hi : pos1;
    double total = 0.0;
    if (b0 < b1) {                                  // the same for every lane
      double v = 0.0;
      for (long long pos = b0 + tid; pos < b1; pos += 256) {
        const size_t row = (size_t)(unsigned)(ad[pos] & 0xFFFFFFFFull);       // < N: the padding sorts behind position N - 1
        v += (double)fabsf(pred[row * D + d] - target[row * D + d]);
      }
      sm[0][tid] = v;
      tree_sum_256<1>(sm, tid);
      total = sm[0][0];
      __syncthreads();
    }
    if (tid == 0) seg[((size_t)d * C + c) * UNC_MAX_CUTS + k] = total;
    lo = hi;
  }
}

// one workgroup per dimension folds everything in a fixed order and writes table[d].  Segment sums: lane (part, k) adds
// column k over the part-th sixteenth of the chunks, lane k the sixteen parts in order, then the running sum over k.
__global__ __launch_bounds__(256) void unc_final_kernel(const unsigned long long* a, long long P, const float* unc, int N, int D, int S, int C,
                                                        UncCuts cuts, const double* part1, const double* part2, const double* seg,
                                                        double* table) {
  __shared__ double sp[BOOT_MAX_SPLIT][UNC_P1];
  __shared__ double sq[BOOT_MAX_SPLIT][3];
  __shared__ double sg[16][UNC_MAX_CUTS];
  __shared__ double st[UNC_MAX_CUTS];
  const int tid = threadIdx.x, d = blockIdx.x;
  const unsigned long long* ad = a + (long long)d * P;
  double* out = table + (size_t)d * UNC_TABLE;
  const double nan = __builtin_nan("");
  unc_stage_part1(part1, S, d, tid, sp);
  for (int i = tid; i < S * 3; i += 256) sq[i / 3][i % 3] = part2[(size_t)d * S * 3 + i];
  {
    const int k = tid % UNC_MAX_CUTS, part = tid / UNC_MAX_CUTS, per = (C + 15) / 16;
    const int c1 = (part + 1) * per < C ? (part + 1) * per : C;
    double v = 0.0;
    for (int c = part * per; c < c1; ++c) v += seg[((size_t)d * C + c) * UNC_MAX_CUTS + k];
    sg[part][k] = k < cuts.n_cuts ? v : 0.0;          // entries past n_cuts were never written
  }
  __syncthreads();
  if (tid < UNC_MAX_CUTS) {
    double v = 0.0;
    for (int part = 0; part < 16; ++part) v += sg[part][tid];
    st[tid] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const double su = unc_fold(sp, S, 0), se = unc_fold(sp, S, 1);
    double umin = __builtin_inf(), umax = -__builtin_inf(), emin = __builtin_inf(), emax = -__builtin_inf();
    unsigned flags = 0u;
    for (int s = 0; s < S; ++s) {
      umin = fmin(umin, sp[s][2]); umax = fmax(umax, sp[s][3]); emin = fmin(emin, sp[s][4]); emax = fmax(emax, sp[s][5]);
      flags |= (unsigned)sp[s][6];
    }
    out[0] = (double)N; out[1] = su; out[2] = se; out[6] = su / (double)N;
    out[8] = (flags & 1u) ? nan : umin; out[9] = (flags & 1u) ? nan : umax;
    out[10] = (flags & 2u) ? nan : emin; out[11] = (flags & 2u) ? nan : emax;
    out[12] = (double)flags; out[13] = 0.0; out[14] = 0.0; out[15] = 0.0;
  } else if (tid < 4) {
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += sq[s][tid - 1];
    out[2 + tid] = v;
    if (tid == 1) out[7] = v / (double)N;
  } else if (tid >= 64 && tid < 64 + UNC_MAX_CUTS) {
    const int k = tid - 64;
    double v = 0.0;
    for (int j = 0; j <= k; ++j) v += st[j];
    out[16 + k] = k < cuts.n_cuts ? v : 0.0;
  } else if (tid >= 128 && tid < 128 + UNC_MAX_Q) {
    const int k = tid - 128;
    double q = -1.0;
    for (int j = 0; j < cuts.n_q; ++j)
      if (j == k) q = cuts.q[j];
    double v = 0.0;
    if (q >= 0.0) {
      const bool has_nan = (unsigned)(ad[N - 1] >> 32) == 0xFFFFFFFFu;       // NaN sorts last
      int lo, hi;
      const double t = np_percentile_position(N, q, &lo, &hi);
      const double x = (double)unc[(size_t)(unsigned)(ad[lo] & 0xFFFFFFFFull) * D + d];
      const double y = (double)unc[(size_t)(unsigned)(ad[hi] & 0xFFFFFFFFull) * D + d];
      v = has_nan ? nan : np_lerp_strict(x, y, t);
    }
    out[32 + k] = v;
  }
}

inline unsigned grid_for(long long n, long long cap = 4096) {
  long long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// composite keys of `columns` key columns into a[columns][P] and the bitonic network over all of them: one launch per step
// whatever the number of columns
inline void launch_sort(const float* keys, long long stride, long long col_step, long long n, long long P, unsigned columns,
                        unsigned long long* a, hipStream_t st) {
  hipLaunchKernelGGL(sort_init_kernel, dim3(grid_for(P), columns), dim3(256), 0, st, keys, stride, col_step, n, P, a);
  const unsigned tiles = (unsigned)(P <= SORT_TILE ? 1 : P / SORT_TILE);
  // k <= SORT_TILE: every step stays inside a tile
  hipLaunchKernelGGL(sort_tile_kernel, dim3(tiles, columns), dim3(256), 0, st, a, P, 2ll, P < SORT_TILE ? P : (long long)SORT_TILE);
  for (long long k = 2ll * SORT_TILE; k <= P; k <<= 1) {
    for (long long j = k >> 1; j >= SORT_TILE; j >>= 1)
      hipLaunchKernelGGL(sort_step_kernel, dim3(grid_for(P), columns), dim3(256), 0, st, a, P, k, j);
    hipLaunchKernelGGL(sort_tile_kernel, dim3(tiles, columns), dim3(256), 0, st, a, P, k, k);
  }
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

int mmdeer_eval_accumulate(const float* pred, const float* target, const float* unc, double* acc, float* sample_err,
                           float* sample_unc, int B, void* stream) {
  MMDEER_CHECK(B >= 0, "eval_accumulate: batch must be >= 0 (got %d)", B);
  if (B == 0) return 0;
  MMDEER_CHECK(pred && target && acc, "eval_accumulate: pred / target / acc must be non-NULL");
  MMDEER_CHECK(!sample_unc || unc, "eval_accumulate: sample_unc needs unc");
  hipLaunchKernelGGL(eval_accumulate_kernel, dim3(4), dim3(256), 0, (hipStream_t)stream, pred, target, unc, acc, sample_err, sample_unc, B);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_eval_quantile_select(const float* err, const float* unc, long long n, int nq, float* vals, double* frac,
                                long long* nvalid, void* stream) {
  MMDEER_CHECK(err && unc && vals && frac && nvalid, "eval_quantile_select: NULL argument");
  MMDEER_CHECK(n > 0 && nq >= 2 && nq <= 64, "eval_quantile_select: need n > 0 and 2 <= nq <= 64 (got n = %lld, nq = %d)", n, nq);
  hipLaunchKernelGGL(eval_quantile_select_kernel, dim3(2 * nq), dim3(256), 0, (hipStream_t)stream, err, unc, n, nq, vals, frac, nvalid);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_eval_ece_bins(const float* err, const float* unc, long long n, const double* edges, int n_bins, double* bins,
                         void* stream) {
  MMDEER_CHECK(err && unc && edges && bins, "eval_ece_bins: NULL argument");
  MMDEER_CHECK(n > 0 && n_bins >= 1 && n_bins <= ECE_MAX_BINS, "eval_ece_bins: need n > 0 and 1 <= n_bins <= %d (got %d)", ECE_MAX_BINS, n_bins);
  hipLaunchKernelGGL(eval_ece_bins_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, err, unc, n, edges, n_bins, bins);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_bootstrap_scratch(long long N, int R) {
  if (N <= 0 || R <= 0) return 0;
  const long long S = boot_split(N);
  // repacked table | partial sums [R][S][18] doubles | partial min / max [R][S][12] floats
  return N * 32 + (long long)R * S * 18 * 8 + (long long)R * S * 12 * 4;
}

int mmdeer_bootstrap_moments(const float* pred, const float* target, long long N, int D, int R, unsigned long long seed, double* mom,
                             int* flags, void* scratch, long long scratch_bytes, void* stream) {
  MMDEER_CHECK(pred && target && mom && flags && scratch, "bootstrap_moments: NULL argument");
  MMDEER_CHECK(N >= 1 && N < (1ll << 31), "bootstrap_moments: need 1 <= N < 2^31 (got %lld)", N);
  MMDEER_CHECK(D >= 1 && D <= 3, "bootstrap_moments: need 1 <= D <= 3 (got %d)", D);
  MMDEER_CHECK(R >= 1 && R <= CI_MAX_R, "bootstrap_moments: need 1 <= R <= %d (got %d)", CI_MAX_R, R);
  MMDEER_CHECK(scratch_bytes >= mmdeer_bootstrap_scratch(N, R), "bootstrap_moments: scratch of %lld bytes, %lld needed", scratch_bytes,
               mmdeer_bootstrap_scratch(N, R));
  MMDEER_CHECK(((uintptr_t)scratch & 15) == 0, "bootstrap_moments: scratch must be 16-byte aligned");
  const int S = boot_split(N);
  float4* table = (float4*)scratch;
  double* part = (double*)((char*)scratch + N * 32);
  float* mm = (float*)((char*)part + (size_t)R * S * 18 * 8);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(boot_repack_kernel, dim3(grid_for(N)), dim3(256), 0, st, pred, target, (int)N, D, table);
  hipLaunchKernelGGL(boot_partial_kernel, dim3(R, S), dim3(256), 0, st, (const float4*)table, (int)N, S, seed, part, mm);
  hipLaunchKernelGGL(boot_fold_kernel, dim3(R), dim3(64), 0, st, (const double*)part, (const float*)mm, S, D, mom, flags);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_bootstrap_ci(const double* mom, const int* flags, long long N, int D, int R, int metric, double q_lo, double q_hi, double* ci,
                        int* nkept, void* stream) {
  MMDEER_CHECK(mom && flags && ci && nkept, "bootstrap_ci: NULL argument");
  MMDEER_CHECK(N >= 1 && N < (1ll << 31), "bootstrap_ci: need 1 <= N < 2^31 (got %lld)", N);
  MMDEER_CHECK(D >= 1 && D <= 3, "bootstrap_ci: need 1 <= D <= 3 (got %d)", D);
  MMDEER_CHECK(R >= 1 && R <= CI_MAX_R, "bootstrap_ci: need 1 <= R <= %d (got %d)", CI_MAX_R, R);
  MMDEER_CHECK(metric == METRIC_CCC || metric == METRIC_PEARSON, "bootstrap_ci: metric must be 0 (CCC) or 1 (Pearson), got %d", metric);
  MMDEER_CHECK(q_lo >= 0.0 && q_lo <= 1.0 && q_hi >= 0.0 && q_hi <= 1.0, "bootstrap_ci: quantile levels must lie in [0, 1]");
  hipLaunchKernelGGL(boot_ci_kernel, dim3(D), dim3(256), 0, (hipStream_t)stream, mom, flags, (int)N, D, R, metric, q_lo, q_hi, ci, nkept);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_sort_pairs_scratch(long long n) {
  if (n <= 0 || n > SORT_MAX_N) return 0;
  long long P = 1;
  while (P < n) P <<= 1;
  return P * 8;
}

int mmdeer_sort_pairs(const float* keys, long long stride, long long n, int* order, void* scratch, long long scratch_bytes, void* stream) {
  MMDEER_CHECK(keys && order && scratch, "sort_pairs: NULL argument");
  MMDEER_CHECK(n >= 1, "sort_pairs: need n >= 1 (got %lld)", n);
  MMDEER_CHECK(n <= SORT_MAX_N, "sort_pairs: n = %lld is above the limit of %lld keys", n, SORT_MAX_N);
  MMDEER_CHECK(stride >= 1, "sort_pairs: stride must be >= 1 (got %lld)", stride);
  MMDEER_CHECK(scratch_bytes >= mmdeer_sort_pairs_scratch(n), "sort_pairs: scratch of %lld bytes, %lld needed", scratch_bytes,
               mmdeer_sort_pairs_scratch(n));
  MMDEER_CHECK(((uintptr_t)scratch & 7) == 0, "sort_pairs: scratch must be 8-byte aligned");
  long long P = 1;
  while (P < n) P <<= 1;
  unsigned long long* a = (unsigned long long*)scratch;
  hipStream_t st = (hipStream_t)stream;
  launch_sort(keys, stride, 0, n, P, 1, a, st);
  hipLaunchKernelGGL(sort_order_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const unsigned long long*)a, n, order);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_average_ranks(const void* sorted, long long n, double* ranks, void* stream) {
  MMDEER_CHECK(sorted && ranks, "average_ranks: NULL argument");
  MMDEER_CHECK(n >= 1 && n <= SORT_MAX_N, "average_ranks: need 1 <= n <= %lld (got %lld)", SORT_MAX_N, n);
  hipLaunchKernelGGL(average_ranks_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)sorted, n, ranks);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_rank_moments(const double* ranks_a, const double* ranks_b, long long n, double* out, void* stream) {
  MMDEER_CHECK(ranks_a && ranks_b && out, "rank_moments: NULL argument");
  MMDEER_CHECK(n >= 1, "rank_moments: need n >= 1 (got %lld)", n);
  hipLaunchKernelGGL(rank_moments_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, ranks_a, ranks_b, n, out);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_calibration_bins_scratch(int D) { return D >= 1 && D <= 3 ? (long long)D * 4 * 4 : 0; }

int mmdeer_calibration_bins(const float* pred, const float* target, const float* unc, long long N, int D, const double* edges, int n_bins,
                            double* stats, double* bins, void* scratch, void* stream) {
  MMDEER_CHECK(pred && target && unc && edges && stats && bins && scratch, "calibration_bins: NULL argument");
  MMDEER_CHECK(N >= 1 && N < (1ll << 31), "calibration_bins: need 1 <= N < 2^31 (got %lld)", N);
  MMDEER_CHECK(D >= 1 && D <= 3, "calibration_bins: need 1 <= D <= 3 (got %d)", D);
  MMDEER_CHECK(n_bins >= 1 && n_bins <= CAL_MAX_BINS, "calibration_bins: need 1 <= n_bins <= %d (got %d)", CAL_MAX_BINS, n_bins);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cal_select_kernel, dim3(D, 3), dim3(256), 0, st, pred, target, unc, N, D, (float*)scratch);
  hipLaunchKernelGGL(cal_bins_kernel, dim3(D, 2 * n_bins), dim3(256), 0, st, pred, target, unc, N, D, edges, n_bins, (const float*)scratch,
                     stats, bins);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

long long mmdeer_uncertainty_table_scratch(long long N, int D) {
  if (N < 2 || N > SORT_MAX_N || D < 1 || D > 3) return 0;
  long long P = 1;
  while (P < N) P <<= 1;
  // sorted pairs [D][P] | first-pass partials [D][S][7] | centred partials [D][S][3] | segment sums [D][C][16]: all doubles wide
  return (long long)D * 8 * (P + (long long)boot_split(N) * (UNC_P1 + 3) + (long long)unc_chunks(N) * UNC_MAX_CUTS);
}

int mmdeer_uncertainty_table(const float* pred, const float* target, const float* unc, long long N, int D, const long long* n_keep,
                             int n_cuts, const double* levels, int n_q, double* table, void* scratch, long long scratch_bytes,
                             void* stream) {
  MMDEER_CHECK(pred && target && unc && table && scratch, "uncertainty_table: NULL argument");
  MMDEER_CHECK(N >= 2, "uncertainty_table: need N >= 2 (got %lld)", N);
  MMDEER_CHECK(N <= SORT_MAX_N, "uncertainty_table: N = %lld is above the limit of %lld samples (the device sort)", N, SORT_MAX_N);
  MMDEER_CHECK(D >= 1 && D <= 3, "uncertainty_table: need 1 <= D <= 3 (got %d)", D);
  MMDEER_CHECK(n_cuts >= 0 && n_cuts <= UNC_MAX_CUTS, "uncertainty_table: need 0 <= n_cuts <= %d (got %d)", UNC_MAX_CUTS, n_cuts);
  MMDEER_CHECK(n_q >= 0 && n_q <= UNC_MAX_Q, "uncertainty_table: need 0 <= n_q <= %d (got %d)", UNC_MAX_Q, n_q);
  MMDEER_CHECK((n_cuts == 0 || n_keep) && (n_q == 0 || levels), "uncertainty_table: NULL argument");
  UncCuts cuts = {};
  cuts.n_cuts = n_cuts; cuts.n_q = n_q;
  for (int k = 0; k < n_cuts; ++k) {
    MMDEER_CHECK(n_keep[k] >= 0 && n_keep[k] <= N, "uncertainty_table: n_keep[%d] = %lld lies outside [0, N = %lld]", k, n_keep[k], N);
    MMDEER_CHECK(k == 0 || n_keep[k] >= n_keep[k - 1], "uncertainty_table: n_keep must be ascending (n_keep[%d] = %lld after %lld)", k,
                 n_keep[k], n_keep[k - 1]);
    cuts.keep[k] = n_keep[k];
  }
  for (int k = 0; k < n_q; ++k) {
    MMDEER_CHECK(levels[k] >= 0.0 && levels[k] <= 1.0, "uncertainty_table: quantile levels must lie in [0, 1] (levels[%d])", k);
    cuts.q[k] = levels[k];
  }
  MMDEER_CHECK(scratch_bytes >= mmdeer_uncertainty_table_scratch(N, D), "uncertainty_table: scratch of %lld bytes, %lld needed",
               scratch_bytes, mmdeer_uncertainty_table_scratch(N, D));
  MMDEER_CHECK(((uintptr_t)scratch & 7) == 0, "uncertainty_table: scratch must be 8-byte aligned");
  long long P = 1;
  while (P < N) P <<= 1;
  const int S = boot_split(N), C = unc_chunks(N);
  unsigned long long* a = (unsigned long long*)scratch;
  double* part1 = (double*)(a + (size_t)D * P);
  double* part2 = part1 + (size_t)D * S * UNC_P1;
  double* seg = part2 + (size_t)D * S * 3;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(unc_sums_kernel, dim3(S, D), dim3(256), 0, st, pred, target, unc, (int)N, D, S, part1);
  hipLaunchKernelGGL(unc_centred_kernel, dim3(S, D), dim3(256), 0, st, pred, target, unc, (int)N, D, S, (const double*)part1, part2);
  launch_sort(unc, (long long)D, 1, N, P, (unsigned)D, a, st);      // the D columns by the same launches
  hipLaunchKernelGGL(unc_prefix_kernel, dim3(C, D), dim3(256), 0, st, (const unsigned long long*)a, P, pred, target, (int)N, D, C, cuts, seg);
  hipLaunchKernelGGL(unc_final_kernel, dim3(D), dim3(256), 0, st, (const unsigned long long*)a, P, unc, (int)N, D, S, C, cuts,
                     (const double*)part1, (const double*)part2, (const double*)seg, table);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
