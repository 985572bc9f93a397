/* csrc/wave_lds.h -- what the kernels that run a transform per WAVEFRONT share (channelizer_fft.hip, band_scope.hip): the workgroup's dynamic LDS and the
 * point at which the lanes of one wavefront may read what other lanes of it wrote to LDS.  tests/hostshim_wave64 defines both macros its own way before this
 * header is read (lanes as fibers), which is why each is guarded. */
#ifndef AIRBAND_CSRC_WAVE_LDS_H
#define AIRBAND_CSRC_WAVE_LDS_H

/* the workgroup's dynamic LDS (tests/hostshim_wave64 gives the host build a static array instead) */
#if !defined(AB_DYNAMIC_LDS_BYTES)
#define AB_DYNAMIC_LDS_BYTES(name) extern __shared__ __attribute__((aligned(16))) uint8_t name[]
#endif

/* Lanes of ONE wavefront exchange data through LDS: a wavefront's LDS operations execute in order, so what is NEEDED is that the compiler keeps them in
 * program order across the exchange (the two wavefront-scope fences around the wave barrier: no instruction).  tests/hostshim_wave64 makes the lanes, which it
 * runs as fibers, meet here. */
#if !defined(AB_WAVE_SYNC)
/* Round 5: every exchange also WAITS until the wavefront's own LDS operations have completed (s_waitcnt lgkmcnt(0)) before any lane reads what another lane wrote.
 * In-order execution of one wavefront's LDS instructions already orders them; the wait takes the kernel off that assumption, at 0 (u8, fft 512) to 2.3 % (CF32, fft 4096) of
 * its time (profiles/r05_misc/fft_*.json, f32_4096_*.json).  It is NOT a fix for round 4's rare wrong transforms: round 5 reproduced those at will -- they need a SECOND PROCESS
 * running this library's long int8 launches on the same GPU, they happen with this wait and with one wavefront per workgroup, they spare the shuffle kernel, and the same kind of
 * fault then hits the main path's CTCSS chain (profiles/r05_event_hunt.md).  One process per GPU: never seen.  What failed turned out to be packed-f32 instructions (lanes 48 - 63 of a
 * result); the library is built without them (_build.py, DEVICE_FLAGS) and the events are gone.  -DAB_WAVE_SYNC_NO_WAIT builds the kernel without the wait. */
#if defined(AB_WAVE_SYNC_NO_WAIT)
#define AB_WAVE_SYNC_EXTRA() (void)0
#else
#define AB_WAVE_SYNC_EXTRA() __builtin_amdgcn_s_waitcnt(0xc07f) /* vmcnt(63) expcnt(7) lgkmcnt(0) */
#endif
#define AB_WAVE_SYNC()                                           \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        AB_WAVE_SYNC_EXTRA();                                    \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)
#endif

#endif
