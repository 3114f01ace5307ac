// mmdeer -- activation elements as fp32, from bf16 or fp32 storage chosen by `template <bool F32>`: 1, 4 or 8 consecutive
// elements from element index idx of `base`.  The 4- and 8-wide forms are vector accesses: idx must keep them aligned (8 bytes for
// 4 bf16, 16 bytes otherwise).  Plain stores; the one write-through form is st4_wt, so a kernel that wants it says so by name.
#pragma once
#include "common.h"

namespace mmdeer {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool F32>
__device__ __forceinline__ float ld1(const void* base, long long idx) {
  if constexpr (F32) return reinterpret_cast<const float*>(base)[idx];
  else return bf2f(reinterpret_cast<const bf16_t*>(base)[idx]);
}
template <bool F32>
__device__ __forceinline__ void st1(void* base, long long idx, float v) {
  if constexpr (F32) reinterpret_cast<float*>(base)[idx] = v;
  else reinterpret_cast<bf16_t*>(base)[idx] = f2bf(v);
}

template <bool F32>
__device__ __forceinline__ f32x4 ld4(const void* base, long long idx) {
  if constexpr (F32) {
    return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(base) + idx);
  } else {
    const u32x2 a = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(base) + idx);
    return f32x4{__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xFFFF0000u), __uint_as_float(a.y << 16),
                 __uint_as_float(a.y & 0xFFFF0000u)};
  }
}
template <bool F32>
__device__ __forceinline__ void st4(void* base, long long idx, f32x4 v) {
  if constexpr (F32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(base) + idx) = v;
  else *reinterpret_cast<u32x2*>(reinterpret_cast<bf16_t*>(base) + idx) = u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)};
}

// st4 written through (common.h: store_wt*).  It pays where a wave writes whole rows contiguously -- full cache lines that the launch
// does not read again; anywhere else use st4.  The 16-byte form carries its own s_nop 1 (finding 8): keep it in store_wt16.
template <bool F32>
__device__ __forceinline__ void st4_wt(void* base, long long idx, f32x4 v) {
  if constexpr (F32) {
    store_wt16(reinterpret_cast<float*>(base) + idx, v);
  } else {
    store_wt8(reinterpret_cast<bf16_t*>(base) + idx, u32x2{pack_bf2(v.x, v.y), pack_bf2(v.z, v.w)});
  }
}

// one 16-byte access in bf16, two in fp32
template <bool F32>
__device__ __forceinline__ void ld8(const void* base, long long idx, f32x4& lo, f32x4& hi) {
  if constexpr (F32) {
    const float* p = reinterpret_cast<const float*>(base) + idx;
    lo = *reinterpret_cast<const f32x4*>(p);
    hi = *reinterpret_cast<const f32x4*>(p + 4);
  } else {
    const u32x4 v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16_t*>(base) + idx);
    lo = f32x4{__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u)};
    hi = f32x4{__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xFFFF0000u), __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xFFFF0000u)};
  }
}
template <bool F32>
__device__ __forceinline__ void st8(void* base, long long idx, const f32x4& lo, const f32x4& hi) {
  if constexpr (F32) {
    float* p = reinterpret_cast<float*>(base) + idx;
    *reinterpret_cast<f32x4*>(p) = lo;
    *reinterpret_cast<f32x4*>(p + 4) = hi;
  } else {
    *reinterpret_cast<u32x4*>(reinterpret_cast<bf16_t*>(base) + idx) =
        u32x4{pack_bf2(lo.x, lo.y), pack_bf2(lo.z, lo.w), pack_bf2(hi.x, hi.y), pack_bf2(hi.z, hi.w)};
  }
}
// the same 8 elements for a caller that keeps them in an array
template <bool F32>
__device__ __forceinline__ void ld8(const void* base, long long idx, float (&x)[8]) {
  f32x4 lo, hi;
  ld8<F32>(base, idx, lo, hi);
  x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
}
template <bool F32>
__device__ __forceinline__ void st8(void* base, long long idx, const float (&x)[8]) {
  st8<F32>(base, idx, f32x4{x[0], x[1], x[2], x[3]}, f32x4{x[4], x[5], x[6], x[7]});
}

// four bf16 in two dwords -> fp32 (exact), and ReLU / tanh on four values
__device__ __forceinline__ f32x4 bf4_to_f32(u32x2 y) {
  return f32x4{__uint_as_float(y.x << 16), __uint_as_float(y.x & 0xFFFF0000u), __uint_as_float(y.y << 16), __uint_as_float(y.y & 0xFFFF0000u)};
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }

__device__ __forceinline__ f32x4 tanh4(f32x4 v) { return f32x4{tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w)}; }

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // F.softplus, threshold 20
__device__ __forceinline__ float softplus_grad(float x) {
#pragma clang fp contract(off)   // one rounding per operation in every kernel that uses it (nig_dev.h: nig_dx)
  if (x > 20.f) return 1.f;
  const float z = expf(x);
  return z / (z + 1.f);
}

}  // namespace mmdeer
