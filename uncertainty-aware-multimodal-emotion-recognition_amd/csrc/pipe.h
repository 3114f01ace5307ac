// mmdeer -- what the K loop of an LDS-DMA kernel is made of (gemm_glds, gemm_nt256, gemm_tt256, gemm_ln, tri_fused; chain.hip
// takes the waits and the DMA).  Each helper is ONE statement of such a loop; the rules they carry are stated here, once:
//
//  1. Ordering.  An LDS-DMA (global_load_lds) is ordered for a ds_read only by the ISSUING wave's vmcnt plus a barrier the reader
//     has passed.  An iteration therefore waits, by count, until its own pieces of the tile it needs have landed (wait_tiles:
//     vmcnt = pieces of the younger tiles still allowed in flight), then passes a barrier -- which also proves that every wave
//     finished reading the slot about to be refilled -- and only then issues the next DMA.
//  2. A raw barrier (__builtin_amdgcn_s_barrier), never __syncthreads(): the latter drains vmcnt to 0 and with it the ring.
//  3. LDS reads of a ring as inline asm (lds_read128, lds_tr_read).  Through a plain load or the builtin the compiler cannot tell
//     the read from the LDS-DMA writes in flight and drains vmcnt to 0 after every DMA issue (no prefetch left); asm reads are
//     invisible to that pass, so their waits are placed by hand as well.
//  4. A hand-placed wait names the registers it protects ("+v" operands: wait_lgkm0, and the vmcnt waits behind
//     gload16_untracked): otherwise nothing keeps the compiler from scheduling a use of them above the wait, or from reusing a
//     dead destination while its load is still in flight.
//  5. Stores of more than 8 bytes from inline asm end in s_nop 1 (common.h: store_wt16).
#pragma once
#include "elem.h"

namespace mmdeer {

// at most N vector-memory operations of this wave still in flight
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// the own pieces of a tile have landed once at most `younger` whole tiles (LPT DMA instructions per wave each) issued after it
// are still in flight; a ring never has more than MAXY of them, so `younger` beyond that waits for MAXY tiles
template <int LPT, int MAXY>
__device__ __forceinline__ void wait_tiles(int younger) {
  static_assert(MAXY >= 1 && MAXY <= 7 && MAXY * LPT <= 63, "cases below; vmcnt is a 6-bit counter");
  if (younger >= MAXY) wait_vm<MAXY * LPT>();
  else if (MAXY > 6 && younger == 6) wait_vm<6 * LPT>();
  else if (MAXY > 5 && younger == 5) wait_vm<5 * LPT>();
  else if (MAXY > 4 && younger == 4) wait_vm<4 * LPT>();
  else if (MAXY > 3 && younger == 3) wait_vm<3 * LPT>();
  else if (MAXY > 2 && younger == 2) wait_vm<2 * LPT>();
  else if (MAXY > 1 && younger == 1) wait_vm<LPT>();
  else wait_vm<0>();
}

// LDS address as the integer the ds_* instructions take
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p;
}

// untracked LDS reads (rule 3); the data is valid after a wait_lgkm0 that names it
__device__ __forceinline__ u32x4 lds_read128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 lds_read128(unsigned addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
// transposed read: the hardware transposes a 4-row x 16-column block of bf16
template <int OFF>
__device__ __forceinline__ u32x2 lds_tr_read(unsigned addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void wait_lgkm0(u32x4& a, u32x4& b) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b)::"memory");
}
__device__ __forceinline__ void wait_lgkm0(u32x4& a, u32x4& b, u32x4& c, u32x4& d) {
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)::"memory");
}

// LDS-DMA, 16 bytes per lane: lane l's 16 bytes at global_src land at lds_dst + 16 l (lds_dst wave-uniform: it travels in M0)
__device__ __forceinline__ void lds_dma16(const void* global_src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)global_src,
                                   (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

// 16-byte global load the compiler does not track (bias and table rows requested in front of a DMA prologue: a tracked load would
// make it drain the DMA queue at the first use).  Loads retire in order; the counted vmcnt wait that covers this one names dst.
__device__ __forceinline__ void gload16_untracked(f32x4& dst, const void* p) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD).  Renumbered, each XCD owns a contiguous range
// of the nwg tiles: neighbouring tiles share an operand panel, which is then fetched into ONE XCD's L2 instead of all eight
// (speed only -- any placement is correct).
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, x = bid & 7, idx = bid >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + idx;
}

}  // namespace mmdeer
