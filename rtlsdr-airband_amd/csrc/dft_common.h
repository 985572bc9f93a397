/* csrc/dft_common.h -- what the staging variants of the int8 matrix-core channelizer share (channelizer_dft.hip: one contiguous image of 16 hops;
 * channelizer_dft_wide.hip: one row per hop): the wait-count ladders, the MFMA wrapper of the ablation builds and the A-fragment readers; through mfma_front.h, the host's opt-in to more than 64 KiB of LDS.
 *
 * Ablation switches (experiment builds only, AIRBAND_EXTRA_DEFINES; the results are WRONG by construction, only the launch time is of interest): AB_ABL_NO_DMA,
 * AB_ABL_NO_MFMA, AB_ABL_NO_STORE and AB_ABL_NO_LDS take the HBM reads, the matrix pipe, the output stores or the A-fragment reads out of the int8 kernel.  They are how
 * its cost is taken apart (profiles/r04_experiments.md) and they stay; experiments that were measured and not adopted do not -- docs/KERNEL_HISTORY.md keeps those. */
#ifndef AIRBAND_CSRC_DFT_COMMON_H
#define AIRBAND_CSRC_DFT_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfma_front.h"

namespace airband {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

/* s_waitcnt vmcnt(n) for a run-time (wave-uniform) n: the instruction takes an immediate.  Waiting for FEWER operations than n to be
 * outstanding is always safe (it waits longer), so this is a ladder of compares, not a switch: the compiler lowers a 25-way switch to a
 * cascade of ~25 scalar instructions and ten branches per tile, while the counts that occur in the steady state of a launch are one or
 * two values near the top (hi ladder: three staging buffers, transfers two or three steps ahead) or 0..3 (lo ladder: two buffers). */
#define AB_W(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")
__device__ __forceinline__ void wait_vmcnt_lo(int n) {
    if (n <= 0) AB_W(0);
    else if (n == 1) AB_W(1);
    else if (n == 2) AB_W(2);
    else if (n == 3) AB_W(3);
    else if (n < 6) AB_W(4);
    else if (n < 8) AB_W(6);
    else if (n < 12) AB_W(8);
    else AB_W(12);
}
__device__ __forceinline__ void wait_vmcnt(int n) {
    if (n >= 18) AB_W(18);
    else if (n >= 16) AB_W(16);
    else if (n >= 14) AB_W(14);
    else if (n >= 12) AB_W(12);
    else if (n >= 10) AB_W(10);
    else if (n >= 8) AB_W(8);
    else if (n >= 6) AB_W(6);
    else wait_vmcnt_lo(n);
}
#undef AB_W

__device__ __forceinline__ v4i ab_mfma(v4i x, v4i b, v4i acc) {
#if defined(AB_ABL_NO_MFMA)
    asm volatile("" ::"v"(x), "v"(b)); /* the operands stay alive (their loads are not optimised away), the matrix pipe stays idle */
    acc.x ^= x.x;
    return acc;
#else
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(x, b, acc, 0, 0, 0);
#endif
}

/* the integer digit sums of a tile: three balanced base-256 digits of the coefficient table; h*: the CS16 high-byte plane */
struct TileAcc {
    v4i a0, a1, a2, h0, h1, h2;
};
/* Recombination of the digit sums in single precision: every accumulator is an exact integer below 2^24 (exact as a float), and
 *     value = ((acc2 * 2^16 + acc1 * 2^8 + acc0) + corr) * unscale          [+ 2^8 * the same of the high-byte plane for CS16]
 * is three fused multiply-adds with the constants folded -- rounding at 2^-24 of partial sums that are never larger than the result's own full scale, the same error
 * class as the final conversion to float (tests/test_gpu_parity.py, stage-1 bar 1e-5 relative RMS).  The scale factors are the same number on every lane -- scalar
 * registers.  flipmask: u8 -> b - 128 as int8 in front of the MFMAs; s8 is int8 already, and has no offset to restore (cu = 0). */
struct Recombine {
    int flipmask;
    float u0, u1, u2, cu, w0, w1, w2; /* w*: CS16 high-byte plane */
};
__device__ __forceinline__ float uni_f(double v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((float)v))); }
__device__ __forceinline__ Recombine recombine(double unscale, double corr, int sfmt) {
    Recombine k;
    k.flipmask = sfmt == AIRBAND_SFMT_S8 ? 0 : (int)0x80808080;
    k.u0 = uni_f(unscale); k.u1 = uni_f(unscale * 256.0); k.u2 = uni_f(unscale * 65536.0);
    k.cu = sfmt == AIRBAND_SFMT_S8 ? 0.0f : (float)(corr * unscale);
    k.w0 = k.u1; k.w1 = k.u2; k.w2 = uni_f(unscale * 16777216.0);
    return k;
}
/* digit sums -> value r of the lane's four (hops grp * 4 .. + 3 of its column) */
template <bool S16>
__device__ __forceinline__ float digit_value(const TileAcc& A, Recombine k, int r) {
    float y = __builtin_fmaf((float)A.a0[r], k.u0, k.cu);
    y = __builtin_fmaf((float)A.a1[r], k.u1, y);
    y = __builtin_fmaf((float)A.a2[r], k.u2, y);
    if (S16) {
        y = __builtin_fmaf((float)A.h0[r], k.w0, y);
        y = __builtin_fmaf((float)A.h1[r], k.w1, y);
        y = __builtin_fmaf((float)A.h2[r], k.w2, y);
    }
    return y;
}

/* Window pieces: the partial sums of pieces 1 .. NP-1 reach wave 0 through LDS, exch = [tile parity][piece - 1][lane] x 4 floats; wave 0 adds them to its own */
template <int NP>
__device__ __forceinline__ void piece_sum(const float4* exch, int t, int lane, float* val) {
    const float4* ex = exch + (t & 1) * (NP - 1) * 64;
#pragma unroll
    for (int q = 0; q < NP - 1; q++) {
        const float4 o = ex[q * 64 + lane];
        val[0] += o.x; val[1] += o.y; val[2] += o.z; val[3] += o.w;
    }
}

template <int AL>
__device__ __forceinline__ v4i lds_read16(const uint8_t* p) {
#if defined(AB_ABL_NO_LDS)
    v4i z = {(int)(uintptr_t)p, 1, 2, 3};
    asm volatile("" : "+v"(z));
    return z;
#endif
    if (AL >= 16) return *reinterpret_cast<const v4i*>(p);
    /* (round 5, measured and dropped: ONE unaligned ds_read_b128 per fragment instead of the assembled reads below -- gfx950 under HSA runs with unaligned DS
     * access and the compiler itself emits that instruction for a 16-byte LDS load of alignment 2 -- is correct and 58 % SLOWER at 250-byte hops: 13.97 against
     * 8.85 ms per launch, profiles/r05_misc/r2000k_*.json; a misaligned wide LDS access is served a few bytes at a time) */
    if (AL == 8) {
        typedef int v2i __attribute__((ext_vector_type(2)));
        const v2i lo = *reinterpret_cast<const v2i*>(p), hi = *reinterpret_cast<const v2i*>(p + 8);
        return (v4i){lo.x, lo.y, hi.x, hi.y};
    }
    if (AL == 4) {
        const int* q = reinterpret_cast<const int*>(p);
        return (v4i){q[0], q[1], q[2], q[3]};
    }
    /* AL == 2: any even address (u8 / s8 hops of an odd number of samples: 2.0 MS/s at WAVE_RATE 16000 is 125 samples = 250 bytes).  The five
     * aligned dwords that hold the 16 bytes, funnelled through v_alignbyte_b32 with the lane's own byte offset (0 or 2): 5 LDS reads + 4 vector
     * instructions per fragment where the aligned variants need one read.  The last dword's upper bytes lie past the fragment and are shifted out. */
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3u);
    const int* q = reinterpret_cast<const int*>(p - sh); /* (pointer arithmetic, not an integer round trip: the compiler must keep seeing an LDS address -- a flat load would also count in vmcnt) */
    const unsigned d0 = (unsigned)q[0], d1 = (unsigned)q[1], d2 = (unsigned)q[2], d3 = (unsigned)q[3], d4 = (unsigned)q[4];
    return (v4i){(int)__builtin_amdgcn_alignbyte(d1, d0, sh), (int)__builtin_amdgcn_alignbyte(d2, d1, sh), (int)__builtin_amdgcn_alignbyte(d3, d2, sh),
                 (int)__builtin_amdgcn_alignbyte(d4, d3, sh)};
}

}  // namespace

}  // namespace airband
#endif
