// marlnav_debug.h - diagnostic builds: per-phase stamps (MARLNAV_STAMPS=1, scripts/kstamps.py) and phase truncation (MARLNAV_AB); both compile to nothing otherwise.
// Part of libmarlnav.so: included once, by marlnav_step.hip (one translation
// unit), inside its anonymous namespace.
#pragma once

// Diagnostic build (MARLNAV_STAMPS=1, scripts/kstamps.py): lane 0 of every
// wave records s_memrealtime / s_memtime at each phase boundary into a
// buffer registered with marlnav_debug_stamps().
#ifndef MARLNAV_STAMPS
#define MARLNAV_STAMPS 0
#endif
#if MARLNAV_STAMPS
__device__ unsigned long long *g_stamps;
// global (not flat) stores: a flat store also counts in lgkmcnt, so the next
// LDS wait would wait for the stamp's write to reach memory
typedef __attribute__((address_space(1))) unsigned long long stamp_t;
#define STAMP_PTR(off) ((stamp_t *)(g_stamps) + (off))
#define STAMP(k)                                                                   \
    do {                                                                           \
        if (lane == 0) {                                                           \
            stamp_t *sp_ = STAMP_PTR((size_t)gw * 24);                             \
            sp_[2 * (k)] = wall_clock64();                                         \
            sp_[2 * (k) + 1] = clock64();                                          \
        }                                                                          \
    } while (0)
// extra realtime-only stamps at slots 20..23 (diagnostic sub-phases): the
// per-env / re-init sub-phases (STAMPX), or with MARLNAV_SUBSTAMPS=1 the
// env-block kernel's stage and observe sub-phases (STAMPS_S) instead
#ifndef MARLNAV_SUBSTAMPS
#define MARLNAV_SUBSTAMPS 0
#endif
#define STAMP_SLOT_(k)                                                             \
    do {                                                                           \
        if (lane == 0) *STAMP_PTR((size_t)gw * 24 + 20 + (k)) = wall_clock64();    \
    } while (0)
#if MARLNAV_SUBSTAMPS
#define STAMPX(k) \
    do {          \
    } while (0)
// MARLNAV_SUBSTAMPS=2: slot 23 is "this wave's last staging load issued"
// (STAMP_ISSUED) instead of "row computed" (STAMPS_S(3)). The time is held
// in SGPRs and stored with the end-of-kernel stamps: a store at the issue
// point would be a VMEM operation younger than the wave's own action load,
// and the counted vmcnt wait that follows could then return before the load.
#if MARLNAV_SUBSTAMPS == 2
#define STAMPS_S(k)                       \
    do {                                  \
        if ((k) != 3) STAMP_SLOT_(k);     \
    } while (0)
#define STAMP_ISSUED_DECL unsigned long long t_issued = 0
#define STAMP_ISSUED() \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_issued)::"memory")
#define STAMP_ISSUED_STORE()                                           \
    do {                                                               \
        if (lane == 0) *STAMP_PTR((size_t)gw * 24 + 23) = t_issued;    \
    } while (0)
#else
#define STAMPS_S(k) STAMP_SLOT_(k)
#endif
#else
#define STAMPX(k) STAMP_SLOT_(k)
#define STAMPS_S(k) \
    do {            \
    } while (0)
#endif
#else
#define STAMPS_S(k) \
    do {            \
    } while (0)
#define STAMPX(k) \
    do {          \
    } while (0)
#define STAMP(k) \
    do {         \
    } while (0)
#endif
#ifndef STAMP_ISSUED
#define STAMP_ISSUED_DECL \
    do {                  \
    } while (0)
#define STAMP_ISSUED() \
    do {               \
    } while (0)
#define STAMP_ISSUED_STORE() \
    do {                     \
    } while (0)
#endif

// Phase-truncation builds (-DMARLNAV_AB=bits; 0 in the product build): the
// step kernels end early, so a phase's cost is the difference of two builds
// (scripts/valu_census.sh). Not bit-exact.
//   bit    the env-block and pair-split kernels ...
//   4096   return at the entry (the launch alone)
//   8192   return after the stage barrier
//   16384  return after the observation
//   32768  return after the per-env phase (split kernel)
//   2      run every phase but skip the final row / state stores
#ifndef MARLNAV_AB
#define MARLNAV_AB 0
#endif

// The pieces of the fixed env-block instantiations' staging prologue
// (kernel_block.h BlockFixed::prologue), one bit each, all on in the product
// build; -DMARLNAV_PROLOGUE=bits builds a library with a subset, so a piece
// is measured apart (profiles/stage_prologue_ab.txt). Every subset is
// bit-exact.
//   1   the own-action load from an SGPR base and a 32-bit lane offset
//   2   staging destinations as LDS-address-space pointers
//   4   partial spans under a literal exec mask (takes the LDS pointers of
//       bit 2 with it: the masked instruction's M0 is written from one)
//   8   the own-action wait count a constant per wave
//   16  the stage-time draw's obstacle index from the wave index
//   32  the reward terms' short divisions compiled in (terms_fast)
#ifndef MARLNAV_PROLOGUE
#define MARLNAV_PROLOGUE 63
#endif
