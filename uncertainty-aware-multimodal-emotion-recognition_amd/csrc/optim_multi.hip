// Clip + AdamW over any list of fp32 tensors (include/mmdeer_optim.h: mmdeer_adamw_multi): the optimiser step of everything that
// trains through autograd into ordinary .grad tensors.  Two launches: sum-of-squares partials over the listed gradients, then the
// update (every block folds the partials itself, in a fixed order: deterministic, no host round trip for the norm) with the mirrors.
// The tensor records live in a device table (more of them than kernel arguments hold); the per-step scalars -- the classes' lr,
// weight decay and bias corrections, betas, eps, clip and scale -- are kernel arguments.
//
// mmdeer_adamw_multi_dev (the DEV instantiations) is the same step for a captured HIP graph: the classes' lr, weight decay and step
// COUNT live in device memory.  Block 0 of launch one adds 1 to every class's count; launch two reads the new count across the
// kernel boundary (no block of it races the bump), and each of its blocks forms the bias corrections once, before its first chunk,
// into LDS, from where the chunk loop takes its class through readfirstlane.  Its table upload is made of launches alone: the records
// ride in the kernel arguments of multi_table_kernel, a batch per launch, and multi_chunkmap_kernel derives chunk -> tensor from the
// records' first chunks -- nothing reads host memory after the call, nothing waits, and a stream capture records all of it.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <vector>

#include "../../include/mmdeer.h"
#include "../../include/mmdeer_optim.h"
#include "../../include/mmdeer_graph.h"
#include "optim.h"

namespace mmdeer {
namespace {

constexpr int MULTI_CHUNK = MMDEER_ADAMW_MULTI_CHUNK;        // elements per chunk: 256 lanes x 4
constexpr int MULTI_NPART = MMDEER_ADAMW_MULTI_SCRATCH;      // the most blocks of the sum-of-squares pass == partials folded by every update block
constexpr int MULTI_MAX_GRID = 256 * 8;                      // update blocks: 8 per CU, the rest by stride over the chunks
static_assert(MULTI_CHUNK == 1024 && MULTI_NPART == 2048, "a chunk is one 16-byte group per lane of a 256-lane block; a lane folds 8 partials");

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// One tensor as the kernels read it.  Groups of 4 elements are counted from the 16-byte boundary at or below the parameter's first
// element: group q of the tensor holds elements 4 q - head .. 4 q - head + 3 (those inside [0, count)), so every group but the first
// and the last is a whole, 16-byte aligned f32x4 of the parameter.
struct MultiTensor {
  float* p;
  const float* g;
  void* mirror;
  float* m;
  float* v;
  long long count;
  int chunk0;          // the tensor's first chunk
  int head;            // elements of the parameter's 16-byte group that lie BELOW its first element: (address / 4) mod 4
  int cls;
  int flags;           // VEC: gradient, moments and mirror sit at the parameter's offset modulo 4 elements; MIRROR_F32
};
static_assert(sizeof(MultiTensor) == 64, "the device table is laid out in 64-byte records");
enum { MT_VEC = 1, MT_MIRROR_F32 = 2 };

struct MultiClass { float lr, wd, bc1, bc2; };
struct MultiArgs {
  const MultiTensor* tensors;
  const int* chunk_tensor;       // chunk -> tensor
  float* partials;
  float* norm_out;
  int nchunks, npart;
  float beta1, beta2, eps, max_norm, grad_scale;
  MultiClass cls[MMDEER_ADAMW_MULTI_MAX_CLASSES];
  mmdeer_adamw_multi_class_dev* cls_dev;     // DEV: the classes in device memory (cls is then unused)
  int ncls;
};
static_assert(sizeof(MultiArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// the DEV upload: a batch of records in the kernel arguments
constexpr int TABLE_BATCH = 60;
struct TableBatch {
  MultiTensor* dst;            // the table's record of rec[0]
  int n, pad;
  MultiTensor rec[TABLE_BATCH];
};
static_assert(sizeof(TableBatch) <= 4096, "kernel arguments are limited to 4 KiB");

// the four elements of group q of a tensor stream (zeros outside the tensor); `whole`: an aligned f32x4 inside the tensor
__device__ __forceinline__ f32x4 load4(const float* base, long long e0, long long count, bool whole) {
  if (whole) return *reinterpret_cast<const f32x4*>(base + e0);
  f32x4 r{0.f, 0.f, 0.f, 0.f};
  if (e0 >= 0 && e0 < count) r.x = base[e0];
  if (e0 + 1 >= 0 && e0 + 1 < count) r.y = base[e0 + 1];
  if (e0 + 2 >= 0 && e0 + 2 < count) r.z = base[e0 + 2];
  if (e0 + 3 >= 0 && e0 + 3 < count) r.w = base[e0 + 3];
  return r;
}
__device__ __forceinline__ void store4(float* base, long long e0, long long count, bool whole, f32x4 x) {
  if (whole) {
    *reinterpret_cast<f32x4*>(base + e0) = x;
    return;
  }
  if (e0 >= 0 && e0 < count) base[e0] = x.x;
  if (e0 + 1 >= 0 && e0 + 1 < count) base[e0 + 1] = x.y;
  if (e0 + 2 >= 0 && e0 + 2 < count) base[e0 + 2] = x.z;
  if (e0 + 3 >= 0 && e0 + 3 < count) base[e0 + 3] = x.w;
}
__device__ __forceinline__ void store4_bf16(bf16_t* base, long long e0, long long count, bool whole, f32x4 x) {
  if (whole) {
    *reinterpret_cast<u32x2*>(base + e0) = u32x2{pack_bf2(x.x, x.y), pack_bf2(x.z, x.w)};
    return;
  }
  if (e0 >= 0 && e0 < count) base[e0] = f2bf(x.x);
  if (e0 + 1 >= 0 && e0 + 1 < count) base[e0 + 1] = f2bf(x.y);
  if (e0 + 2 >= 0 && e0 + 2 < count) base[e0 + 2] = f2bf(x.z);
  if (e0 + 3 >= 0 && e0 + 3 < count) base[e0 + 3] = f2bf(x.w);
}

// The record of chunk c's tensor, every field wave-uniform (in SGPRs): the chunk index is uniform, but the compiler cannot know that
// the table is not written by the kernel's own stores, so it would keep the record in VGPRs and index the classes by one.
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
template <typename P>
__device__ __forceinline__ P uni64(P x) {
  const unsigned long long u = (unsigned long long)x;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return (P)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float unif(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ MultiTensor tensor_of(const MultiArgs& a, int c) {
  const MultiTensor& R = a.tensors[uni(a.chunk_tensor[c])];
  return {uni64(R.p), uni64(R.g), uni64(R.mirror), uni64(R.m), uni64(R.v), uni64(R.count), uni(R.chunk0), uni(R.head), uni(R.cls), uni(R.flags)};
}

// sum over the block's 256 lanes in a fixed order (a pairwise tree: lanes, waves), result in every lane
__device__ __forceinline__ float block_sum256(float a, float* sm) {
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// Launch one.  Block b takes chunks b, b + grid, ...; lane t of it group t of each, summed serially in that order; then the block's
// pairwise tree.  One partial per block.
// DEV: block 0 also advances every class's step count, which no block of this launch reads.
template <bool DEV>
__global__ __launch_bounds__(256) void multi_sumsq_kernel(const MultiArgs a) {
#pragma clang fp contract(off)
  __shared__ float sm[4];
  if constexpr (DEV) {
    if (blockIdx.x == 0 && (int)threadIdx.x < a.ncls) a.cls_dev[threadIdx.x].step += 1;
  }
  float acc = 0.f;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const MultiTensor T = tensor_of(a, c);
    const long long count = T.count;
    const long long e0 = ((long long)(c - T.chunk0) * 256 + threadIdx.x) * 4 - T.head;
    const bool whole = (T.flags & MT_VEC) && e0 >= 0 && e0 + 4 <= count;
    if (e0 + 4 > 0 && e0 < count) {
      const f32x4 g = load4(T.g, e0, count, whole);
      acc += (g.x * g.x + g.y * g.y) + (g.z * g.z + g.w * g.w);
    }
  }
  acc = block_sum256(acc, sm);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = acc;
}

// beta^n for the bias corrections of the DEV step: repeated squaring in float64, rounded once to float32 (within half an ulp of
// the exact power, plus float64's own rounding of at most 62 products: the host's powf is allowed one ulp)
__device__ __forceinline__ float pow_int(float beta, int n) {
  double b = (double)beta, r = 1.0;
  for (; n > 0; n >>= 1) {
    if (n & 1) r *= b;
    b *= b;
  }
  return (float)r;
}

// Launch two.
template <bool DEV>
__global__ __launch_bounds__(256) void multi_update_kernel(const MultiArgs a) {
  __shared__ float sm[4];
  __shared__ MultiClass scls[MMDEER_ADAMW_MULTI_MAX_CLASSES];
  if constexpr (DEV) {      // once per block: lane c forms class c's corrections from the count launch one left; block_sum256's barrier orders it
    if ((int)threadIdx.x < a.ncls) {
      const mmdeer_adamw_multi_class_dev K = a.cls_dev[threadIdx.x];
      scls[threadIdx.x] = {K.lr, K.weight_decay, 1.f - pow_int(a.beta1, K.step), 1.f - pow_int(a.beta2, K.step)};
    }
  }
  float clip;
  {
#pragma clang fp contract(off)
    // the norm from the partials: lane t folds partials 8 t .. 8 t + 7 pairwise (zeros past npart), then the block's tree
    const int i = threadIdx.x * 8;
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = i + j < a.npart ? a.partials[i + j] : 0.f;
    const float ss = block_sum256(((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7])), sm);
    const float norm = sqrtf(ss) * fabsf(a.grad_scale);
    clip = a.max_norm > 0.f ? fminf(1.f, a.max_norm / (norm + 1e-6f)) : 1.f;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.norm_out) *a.norm_out = norm;
  }
  AdamCoef k;
  k.gs = clip * a.grad_scale; k.b1 = a.beta1; k.b2 = a.beta2; k.eps = a.eps;
  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    const MultiTensor T = tensor_of(a, c);
    const long long count = T.count;
    const long long e0 = ((long long)(c - T.chunk0) * 256 + threadIdx.x) * 4 - T.head;
    if (e0 + 4 <= 0 || e0 >= count) continue;
    const int flags = T.flags;
    const bool whole = (flags & MT_VEC) && e0 >= 0 && e0 + 4 <= count;
    MultiClass K;
    if constexpr (DEV) {
      const MultiClass S = scls[T.cls];
      K = {unif(S.lr), unif(S.wd), unif(S.bc1), unif(S.bc2)};
    } else {
      K = a.cls[T.cls];
    }
    k.wd = K.wd; k.ibc1 = 1.f / K.bc1; k.isbc2 = 1.f / sqrtf(K.bc2);
    f32x4 p = load4(T.p, e0, count, whole);
    const f32x4 g = load4(T.g, e0, count, whole);
    f32x4 m = load4(T.m, e0, count, whole), v = load4(T.v, e0, count, whole);
    adamw_update4(p, g, m, v, K.lr, k);
    store4(T.p, e0, count, whole, p);
    store4(T.m, e0, count, whole, m);
    store4(T.v, e0, count, whole, v);
    if (T.mirror) {
      if (flags & MT_MIRROR_F32) store4((float*)T.mirror, e0, count, whole, p);
      else store4_bf16((bf16_t*)T.mirror, e0, count, whole, p);
    }
  }
}

// The DEV upload, launch by launch: thread t of a batch writes dword t of its records ...
__global__ __launch_bounds__(256) void multi_table_kernel(const TableBatch b) {
  constexpr int W = sizeof(MultiTensor) / 4;
  const unsigned* src = reinterpret_cast<const unsigned*>(b.rec);
  unsigned* dst = reinterpret_cast<unsigned*>(b.dst);
  for (int t = threadIdx.x; t < b.n * W; t += blockDim.x) dst[t] = src[t];
}
// ... then thread c finds chunk c's tensor: the LAST record whose first chunk is <= c (records are in chunk order; one without
// elements shares its first chunk with the next and is passed over; those behind the last chunk start at nchunks)
__global__ __launch_bounds__(256) void multi_chunkmap_kernel(const MultiTensor* __restrict__ t, int n, int* __restrict__ chunk_tensor, int nchunks) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nchunks) return;
  int lo = 0, hi = n;                      // first record with chunk0 > c in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid].chunk0 <= c) lo = mid + 1; else hi = mid;
  }
  chunk_tensor[c] = lo - 1;                // >= 0: record 0 starts at chunk 0
}

std::atomic<long long> g_uploads{0}, g_dev_uploads{0}, g_blocking{0};

inline int head_of(const void* p, int elem_bytes) { return (int)(((uintptr_t)p / (uintptr_t)elem_bytes) & 3); }
inline long long chunks_of(const mmdeer_adamw_multi_tensor& t) {
  return t.count > 0 ? (t.count + head_of(t.param, 4) + MULTI_CHUNK - 1) / MULTI_CHUNK : 0;
}

// the records' own checks (what mmdeer_adamw_multi_table_bytes can see); -> total chunks
int check_records(const mmdeer_adamw_multi_tensor* ts, int n, long long* total_chunks) {
  MMDEER_CHECK(n >= 0, "adamw_multi: ntensors must be >= 0 (got %d)", n);
  MMDEER_CHECK(n == 0 || ts, "adamw_multi: tensors is NULL");
  long long c = 0;
  for (int i = 0; i < n; ++i) {
    MMDEER_CHECK(ts[i].count >= 0 && ts[i].count < (1ll << 40), "adamw_multi: tensor %d: count %lld", i, ts[i].count);
    c += chunks_of(ts[i]);
  }
  MMDEER_CHECK(c < (1ll << 31), "adamw_multi: %lld chunks are more than an int holds", c);
  *total_chunks = c;
  return 0;
}
inline long long table_bytes(int n, long long chunks) { return ((long long)n * (long long)sizeof(MultiTensor) + chunks * 4 + 15) / 16 * 16; }

// what both entries take, whichever struct it came in
struct MultiCall {
  const mmdeer_adamw_multi_tensor* tensors;
  int n, nclasses;
  float *exp_avg, *exp_avg_sq;
  long long moment_elems;
  void* table;
  long long table_bytes;
  int upload;
  float *scratch, *grad_norm;
  float beta1, beta2, eps, max_grad_norm, grad_scale;
  hipStream_t stream;
};
template <typename A>
MultiCall call_of(const A* a) {
  return {a->tensors, a->ntensors, a->nclasses, a->exp_avg, a->exp_avg_sq, a->moment_elems, a->table, a->table_bytes, a->upload,
          a->scratch, a->grad_norm, a->beta1, a->beta2, a->eps, a->max_grad_norm, a->grad_scale, (hipStream_t)a->stream};
}

// the refusals the two entries share, before the classes' own; -> total chunks
int check_call(const MultiCall& a, long long* total_chunks) {
  long long chunks = 0;
  TRY(check_records(a.tensors, a.n, &chunks));
  MMDEER_CHECK(a.nclasses >= 1 && a.nclasses <= MMDEER_ADAMW_MULTI_MAX_CLASSES, "adamw_multi: 1..%d classes (got %d)",
               MMDEER_ADAMW_MULTI_MAX_CLASSES, a.nclasses);
  MMDEER_CHECK(a.beta1 >= 0.f && a.beta1 < 1.f && a.beta2 >= 0.f && a.beta2 < 1.f, "adamw_multi: betas must lie in [0, 1)");
  MMDEER_CHECK(std::isfinite(a.eps) && a.eps > 0.f, "adamw_multi: eps must be finite and positive");
  MMDEER_CHECK(std::isfinite(a.grad_scale) && std::isfinite(a.max_grad_norm), "adamw_multi: grad_scale and max_grad_norm must be finite");
  *total_chunks = chunks;
  return 0;
}

// ... and behind them: buffers, table and every record
int check_tensors(const MultiCall& a, long long chunks) {
  const int n = a.n;
  MMDEER_CHECK(a.exp_avg && a.exp_avg_sq && al4(a.exp_avg) && al4(a.exp_avg_sq) && a.moment_elems >= 0,
               "adamw_multi: exp_avg / exp_avg_sq must be non-NULL and 4-byte aligned");
  MMDEER_CHECK(a.scratch && al4(a.scratch), "adamw_multi: scratch must be non-NULL");
  MMDEER_CHECK(al4(a.grad_norm), "adamw_multi: grad_norm must be 4-byte aligned");
  MMDEER_CHECK(a.table && al16(a.table), "adamw_multi: table must be non-NULL and 16-byte aligned");
  MMDEER_CHECK(a.table_bytes >= table_bytes(n, chunks), "adamw_multi: the table needs %lld bytes (got %lld)", table_bytes(n, chunks), a.table_bytes);
  std::vector<std::pair<long long, long long>> ranges;       // moment ranges of the tensors with elements
  ranges.reserve(n);
  for (int i = 0; i < n; ++i) {
    const mmdeer_adamw_multi_tensor& t = a.tensors[i];
    MMDEER_CHECK(t.param && t.grad && al4(t.param) && al4(t.grad), "adamw_multi: tensor %d: param / grad must be non-NULL and 4-byte aligned", i);
    MMDEER_CHECK(t.mirror_f32 ? al4(t.mirror) : ((uintptr_t)t.mirror & 1) == 0, "adamw_multi: tensor %d: misaligned mirror", i);
    MMDEER_CHECK(t.cls >= 0 && t.cls < a.nclasses, "adamw_multi: tensor %d: class %d is outside 0..%d", i, t.cls, a.nclasses - 1);
    MMDEER_CHECK(t.moment_off >= 0 && t.moment_off <= a.moment_elems && t.count <= a.moment_elems - t.moment_off,
                 "adamw_multi: tensor %d: moments [%lld, +%lld) pass the buffers' %lld elements", i, t.moment_off, t.count, a.moment_elems);
    if (t.count > 0) ranges.emplace_back(t.moment_off, t.count);
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i)
    MMDEER_CHECK(ranges[i - 1].first + ranges[i - 1].second <= ranges[i].first, "adamw_multi: moment ranges overlap at element %lld", ranges[i].first);
  return 0;
}

// record i of the table as the kernels read it; c: its first chunk
MultiTensor record_of(const MultiCall& a, int i, int c) {
  const mmdeer_adamw_multi_tensor& t = a.tensors[i];
  const int head = head_of(t.param, 4);
  float* m = a.exp_avg + t.moment_off;
  float* v = a.exp_avg_sq + t.moment_off;
  const bool vec = head_of(t.grad, 4) == head && head_of(m, 4) == head && head_of(v, 4) == head &&
                   (!t.mirror || head_of(t.mirror, t.mirror_f32 ? 4 : 2) == head);
  return {t.param, t.grad, t.mirror, m, v, t.count, c, head, t.cls, (vec ? MT_VEC : 0) | (t.mirror_f32 ? MT_MIRROR_F32 : 0)};
}

MultiArgs kernel_args(const MultiCall& a, long long chunks) {
  MultiArgs k{};
  k.tensors = (MultiTensor*)a.table; k.chunk_tensor = (const int*)((MultiTensor*)a.table + a.n); k.partials = a.scratch; k.norm_out = a.grad_norm;
  k.nchunks = (int)chunks; k.npart = (int)std::min<long long>(chunks, MULTI_NPART);
  k.beta1 = a.beta1; k.beta2 = a.beta2; k.eps = a.eps; k.max_norm = a.max_grad_norm; k.grad_scale = a.grad_scale;
  return k;
}

}  // namespace
}  // namespace mmdeer

using namespace mmdeer;

extern "C" {

long long mmdeer_adamw_multi_table_bytes(const mmdeer_adamw_multi_tensor* tensors, int32_t ntensors) {
  long long chunks = 0;
  if (check_records(tensors, ntensors, &chunks) != 0) return -1;
  return table_bytes(ntensors, chunks);
}

long long mmdeer_adamw_multi_uploads(void) { return g_uploads.load(); }
long long mmdeer_adamw_multi_dev_uploads(void) { return g_dev_uploads.load(); }
long long mmdeer_adamw_multi_blocking_calls(void) { return g_blocking.load(); }

int mmdeer_adamw_multi(const mmdeer_adamw_multi_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  const MultiCall call = call_of(a);
  const int n = call.n;
  long long chunks = 0;
  TRY(check_call(call, &chunks));
  MultiClass cls[MMDEER_ADAMW_MULTI_MAX_CLASSES] = {};
  for (int c = 0; c < a->nclasses; ++c) {
    const mmdeer_adamw_multi_class& K = a->classes[c];
    MMDEER_CHECK(K.step >= 1, "adamw_multi: class %d: step must be >= 1 (got %d)", c, K.step);
    MMDEER_CHECK(std::isfinite(K.lr) && K.lr > 0.f, "adamw_multi: class %d: lr must be finite and positive", c);
    MMDEER_CHECK(std::isfinite(K.weight_decay) && K.weight_decay >= 0.f, "adamw_multi: class %d: weight_decay must be finite and >= 0", c);
    cls[c] = {K.lr, K.weight_decay, 1.f - powf(a->beta1, (float)K.step), 1.f - powf(a->beta2, (float)K.step)};
  }
  TRY(check_tensors(call, chunks));
  if (chunks == 0) return 0;
  hipStream_t s = call.stream;
  if (a->upload) {
    std::vector<unsigned char> img((size_t)table_bytes(n, chunks), 0);
    MultiTensor* ht = (MultiTensor*)img.data();
    int* hc = (int*)(ht + n);
    int c = 0;
    for (int i = 0; i < n; ++i) {
      ht[i] = record_of(call, i, c);
      for (long long j = chunks_of(a->tensors[i]); j > 0; --j) hc[c++] = i;
    }
    // ordered on the stream behind the launches of earlier calls that read the table; the image is the library's until the wait returns
    MMDEER_HIP(hipMemcpyAsync(a->table, img.data(), img.size(), hipMemcpyHostToDevice, s));
    g_blocking.fetch_add(1);
    MMDEER_HIP(hipStreamSynchronize(s));
    g_uploads.fetch_add(1);
  }
  MultiArgs k = kernel_args(call, chunks);
  for (int c = 0; c < a->nclasses; ++c) k.cls[c] = cls[c];
  hipLaunchKernelGGL(multi_sumsq_kernel<false>, dim3(k.npart), dim3(256), 0, s, k);
  MMDEER_HIP(hipGetLastError());
  hipLaunchKernelGGL(multi_update_kernel<false>, dim3((int)std::min<long long>(chunks, MULTI_MAX_GRID)), dim3(256), 0, s, k);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

int mmdeer_adamw_multi_dev(const mmdeer_adamw_multi_dev_args* a) {
  MMDEER_CHECK(a != nullptr, "args is NULL");
  const MultiCall call = call_of(a);
  const int n = call.n;
  long long chunks = 0;
  TRY(check_call(call, &chunks));
  MMDEER_CHECK(a->classes && al16(a->classes), "adamw_multi_dev: classes must be non-NULL device memory, 16-byte aligned");
  TRY(check_tensors(call, chunks));
  if (chunks == 0) return 0;
  hipStream_t s = call.stream;
  MultiArgs k = kernel_args(call, chunks);
  k.cls_dev = (mmdeer_adamw_multi_class_dev*)a->classes; k.ncls = a->nclasses;
  if (a->upload) {
    // launches alone: the records ride in kernel arguments (copied at launch, or into the graph node under capture)
    TableBatch b{};
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += TABLE_BATCH) {
      b.dst = (MultiTensor*)a->table + i0;
      b.n = std::min(TABLE_BATCH, n - i0);
      for (int i = 0; i < b.n; ++i) {
        b.rec[i] = record_of(call, i0 + i, c);
        c += (int)chunks_of(a->tensors[i0 + i]);
      }
      hipLaunchKernelGGL(multi_table_kernel, dim3(1), dim3(256), 0, s, b);
      MMDEER_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(multi_chunkmap_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (const MultiTensor*)a->table, n,
                       (int*)((MultiTensor*)a->table + n), (int)chunks);
    MMDEER_HIP(hipGetLastError());
    g_dev_uploads.fetch_add(1);
  }
  hipLaunchKernelGGL(multi_sumsq_kernel<true>, dim3(k.npart), dim3(256), 0, s, k);
  MMDEER_HIP(hipGetLastError());
  hipLaunchKernelGGL(multi_update_kernel<true>, dim3((int)std::min<long long>(chunks, MULTI_MAX_GRID)), dim3(256), 0, s, k);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // extern "C"
