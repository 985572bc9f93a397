/* csrc/audio_sample.h -- the per-sample functions of the encoded outputs, shared by audio_pack.hip (channel rows) and mixer_gate.hip (mixer rows): the float
 * step and the two G.711 laws of include/airband_hip.h ("encoded audio collect").  One float32 multiplication per sample -- the files that include this are
 * compiled with -ffp-contract=off: nothing may fuse it with the rounding behind it -- everything after it is integer arithmetic. */
#pragma once

#include <hip/hip_runtime.h>

namespace airband {

/* the sample as an integer in -32767 .. 32767; NaN is 0 and not clipped, anything beyond full scale (the infinities too) is clipped */
__device__ __forceinline__ int audio_q(float x, int& n_clipped) {
    if (x != x) return 0;
    const float v = x * 32767.0f;
    if (v > 32767.0f || v < -32767.0f) {
        n_clipped++;
        return v < 0.0f ? -32767 : 32767;
    }
    return (int)rintf(v); /* to nearest, ties to even (v_rndne_f32) */
}

/* position of the highest set bit; m > 0 */
__device__ __forceinline__ int audio_msb(unsigned m) { return 31 - __builtin_clz(m); }

/* G.711 mu-law of q: the segment is the position of m's highest bit (m = 33 .. 8192: bit 5 is segment 0, bit 13 -- 8192 alone -- the out-of-range code) */
__device__ __forceinline__ unsigned audio_ulaw(int q) {
    const int p = q >> 2;
    const unsigned mask = p < 0 ? 0x7Fu : 0xFFu;
    const int mag = p < 0 ? -p : p;
    const unsigned m = (unsigned)(mag < 8159 ? mag : 8159) + 33u;
    const int seg = audio_msb(m) - 5;
    const unsigned code = seg >= 8 ? 0x7Fu : ((unsigned)seg << 4) | ((m >> (seg + 1)) & 0xFu);
    return code ^ mask;
}

/* G.711 A-law of q: m = 0 .. 4095 (4096 and beyond would be the out-of-range code); segments 0 and 1 share the shift */
__device__ __forceinline__ unsigned audio_alaw(int q) {
    const int p = q >> 3;
    const unsigned mask = p >= 0 ? 0xD5u : 0x55u;
    const unsigned m = (unsigned)(p >= 0 ? p : -p - 1);
    const int top = audio_msb(m | 1u) - 4;
    const int seg = top > 0 ? top : 0;
    const unsigned code = seg >= 8 ? 0x7Fu : ((unsigned)seg << 4) | ((m >> (seg < 2 ? 1 : seg)) & 0xFu);
    return code ^ mask;
}

}  // namespace airband
