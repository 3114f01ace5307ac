// mmdeer -- in-kernel time stamps of the diagnostic build (-DMMDEER_STAMPS: build.build_stamps(), read by tools/*_stamps.py by
// slot position).  Without the flag all three expand to nothing.  A kernel aliases them under a short name with its own buffer,
// slot layout and guard.  Place a stamp only where lgkmcnt is (nearly) 0: its wait drains the scalar / LDS queue.
//   MMDEER_STAMP(buf, slot, who)   shader-clock sample (s_memtime) of the lanes `who` selects into buf[slot], if buf is not null
//   MMDEER_WGSTAMP(buf, index, who)  the same from the 100 MHz real-time counter (s_memrealtime: comparable across XCDs), for
//                                  per-workgroup begin / end stamps; a guard of its own: the kernels bound the index differently
//   MMDEER_STAMP_DRAIN()           vmcnt(0) in front of a closing stamp: the kernel's stores are part of what it times
// MMDEER_STAMPS_LOOP additionally enables the stamps inside a K loop (they lengthen it: a build of their own).
#pragma once

#ifdef MMDEER_STAMPS
#define MMDEER_STAMP(buf, slot, who)                                                       \
  do {                                                                                     \
    if ((buf) && (who)) {                                                                  \
      unsigned long long t_;                                                               \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
      (buf)[slot] = t_;                                                                    \
    }                                                                                      \
  } while (0)
#define MMDEER_WGSTAMP(buf, index, who)                                                    \
  do {                                                                                     \
    if ((buf) && (who)) {                                                                  \
      unsigned long long t_;                                                               \
      asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");       \
      (buf)[index] = t_;                                                                   \
    }                                                                                      \
  } while (0)
#define MMDEER_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define MMDEER_STAMP(buf, slot, who) do {} while (0)
#define MMDEER_WGSTAMP(buf, index, who) do {} while (0)
#define MMDEER_STAMP_DRAIN() do {} while (0)
#endif
