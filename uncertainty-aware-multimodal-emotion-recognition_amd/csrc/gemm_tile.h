// mmdeer -- from a workgroup number to its (problem, batch z, K-slice, tile) and the problem's descriptor, for the grouped GEMM
// kernels.  The descriptor is read straight from the kernarg segment (constant address space, scalar loads): indexing the
// by-value GemmGroup with a runtime index would make the compiler spill a private copy of it.
#pragma once
#include <stddef.h>
#include "gemm.h"
#include "pipe.h"

namespace mmdeer {

typedef const __attribute__((address_space(4))) unsigned char* karg_ptr;
typedef const __attribute__((address_space(4))) GemmProblem* desc_ptr;

struct TileAt { int pi, z, slice, tmb, tnb; };

// g_off = byte offset of `g` inside the kernel's kernarg segment
__device__ __forceinline__ desc_ptr locate_tile(const GemmGroup& g, int bid, int g_off, TileAt& t) {
  int pi = 0;
#pragma unroll
  for (int i = 1; i < GEMM_MAX_PROBLEMS; ++i)
    if (i < g.nprob && bid >= g.tile_start[i]) pi = i;
  karg_ptr kbase = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + g_off;
  const __attribute__((address_space(4))) GemmProblem& p =
      *(desc_ptr)(kbase + __builtin_offsetof(GemmGroup, p) + (size_t)pi * sizeof(GemmProblem));
  const int local = bid - g.tile_start[pi];
  const int per_slice = p.tiles_m * p.tiles_n;
  const int per_batch = per_slice * p.splitk;
  t.pi = pi;
  t.z = local / per_batch;
  const int rem_b = local - t.z * per_batch;
  t.slice = rem_b / per_slice;
  const int rem = rem_b - t.slice * per_slice;
  t.tmb = rem / p.tiles_n; t.tnb = rem - t.tmb * p.tiles_n;
  return &p;
}

// ---- the "problem 0 preloaded" form (gemm_glds.hip, gemm_nt256.hip): what the two kernels share around their lookup.
// Problem 0 of the launch travels as plain scalar kernel arguments: they lead the kernarg segment and are preloaded into SGPRs by
// the command processor (-mllvm -amdgpu-kernarg-preload-count), so a workgroup of problem 0 -- all of them in most launches --
// computes its DMA addresses without waiting for a single kernarg fetch (measured before: ~3000 cycles from wave start to the
// first DMA, two dependent cold scalar loads).  Workgroups of the other problems of a group (bid >= nt0) read their descriptor
// from `g`.  nt0 = 0 disables the fast path (batched problem 0).
// Two blocks stay written out in both kernels, because as shared functions the same statements compile differently there: the
// lookup itself (other address arithmetic in the prologue) and the bias prefetch behind the DMA prologue (1-7 more VGPRs).  The
// bias chunks are tracked loads, younger than the prologue DMAs: the first counted waits of the loop are merely stricter than
// needed, never too weak.
struct NtKernargs {   // mirror of the kernels' parameter list (for the offset of `g` in the kernarg segment)
  const bf16_t* A;
  const bf16_t* B;
  int M, N, nk, lda, ldb, tiles_n, nt0, nwg;
  GemmGroup g;
};
// offset of the last parameter of a kernel, each placed at its natural alignment as the kernarg segment lays them out
template <typename... Args>
constexpr size_t last_kernarg_offset(void (*)(Args...)) {
  size_t off = 0, last = 0;
  ((last = off = (off + alignof(Args) - 1) / alignof(Args) * alignof(Args), off += sizeof(Args)), ...);
  return last;
}

// Warm the scalar cache with the problem's descriptor lines: the epilogue reads ~20 fields of it, which would otherwise miss
// (cold, ~1000 cycles) at the very end of the kernel.  Asm loads so that they are issued where this stands; the results are
// dead, the registers stay reserved until warm_wait() after the K loop.
__device__ __forceinline__ void warm_descriptor(desc_ptr pp, unsigned& w0, unsigned& w1, unsigned& w2, unsigned& w3) {
  asm volatile("s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %4, 0x40\n\ts_load_dword %2, %4, 0x80\n\ts_load_dword %3, %4, 0xbc"
               : "=&s"(w0), "=&s"(w1), "=&s"(w2), "=&s"(w3) : "s"(pp) : "memory");
}
__device__ __forceinline__ void warm_wait(unsigned w0, unsigned w1, unsigned w2, unsigned w3) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(w0), "s"(w1), "s"(w2), "s"(w3) : "memory");
}

// host: launch a preloaded-form kernel over `total` tiles, stages of 2^kshift elements of K
template <typename... Args>
static int launch_nt_preloaded(void (*kernel)(Args...), const GemmGroup& g, int total, int kshift, int block, hipStream_t stream) {
  static_assert(last_kernarg_offset(static_cast<void (*)(Args...)>(nullptr)) == offsetof(NtKernargs, g),
                "NtKernargs mirrors the parameter list of the preloaded-form kernels");
  const GemmProblem& q = g.p[0];
  const int nt0 = q.batch == 1 ? g.tile_start[1] : 0;   // tile_start[nprob..] = total
  hipLaunchKernelGGL(kernel, dim3(total), dim3(block), 0, stream, reinterpret_cast<const bf16_t*>(q.A),
                     reinterpret_cast<const bf16_t*>(q.B), q.M, q.N, q.K >> kshift, q.lda, q.ldb, q.tiles_n, nt0,
                     g.xcd_remap ? total : 0, g);
  MMDEER_HIP(hipGetLastError());
  return 0;
}

}  // namespace mmdeer
