/* csrc/audio_decimate.h -- the output decimation's filter (include/airband_hip.h, "output decimation"): the 47-tap half-band FIR in Q15, ONCE, for the host
 * and the device, and the filter core the kernels share: "S in LDS -> four outputs per lane".  audio_decimate.hip (channel rows) is its one user today; it is
 * written over two int16 streams in LDS and knows nothing of rows, lists or formats, so that mixer_gate.hip's pack can use it for frames of left / right later.
 * Integers only: an int32 accumulator cannot overflow (sum |h| * 32767 + 16384 < 2^31), so every summation order gives the same bits. */
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace airband {

constexpr int AUDIO_DECIMATE_TAPS = 47;    /* AIRBAND_AUDIO_DECIMATE_TAPS */
constexpr int AUDIO_DECIMATE_HIST = 46;    /* q values a channel carries from batch to batch */
constexpr int AUDIO_DECIMATE_CENTRE = 16384; /* h[23] */
/* h[23 +- d] for d = 1, 3, .. 23; every other tap but the centre is 0.  A Kaiser window (beta 5.5) on the ideal half-band, rounded to Q15, the two inner taps
 * adjusted so that the sum of all 47 is exactly 32768 */
constexpr int AUDIO_DECIMATE_SIDE[12] = {10383, -3332, 1853, -1178, 781, -520, 339, -213, 126, -68, 32, -11};

/* h[j], j = 0 .. 46 */
constexpr int audio_decimate_tap(int j) {
    const int d = j < 23 ? 23 - j : j - 23;
    return d == 0 ? AUDIO_DECIMATE_CENTRE : ((d & 1) ? AUDIO_DECIMATE_SIDE[d >> 1] : 0);
}
/* the polyphase form: y[n] = sum_{k = 0 .. 23} audio_decimate_even_tap(k) * S[2 n + 2 k]  +  16384 * S[2 n + 23] */
constexpr int audio_decimate_even_tap(int k) { return audio_decimate_tap(2 * k); }
/* even taps 2 p and 2 p + 1 as the two int16 halves of a dword, the lower index in the lower half */
constexpr unsigned audio_decimate_tap_pair(int p) {
    return ((unsigned)audio_decimate_even_tap(2 * p) & 0xFFFFu) | ((unsigned)audio_decimate_even_tap(2 * p + 1) << 16);
}

#if defined(__HIPCC__)
/* a.lo * b.lo + a.hi * b.hi + c over the signed int16 halves of two dwords (v_dot2_i32_i16 where the compiler has it for the target; the same integers without) */
#if defined(__HIP_DEVICE_COMPILE__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_sdot2)
#define AUDIO_DECIMATE_SDOT2 1
#endif
#endif
__device__ __forceinline__ int audio_decimate_dot2(unsigned a, unsigned b, int c) {
#if defined(AUDIO_DECIMATE_SDOT2)
    typedef short dec_v2s __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(dec_v2s, a), __builtin_bit_cast(dec_v2s, b), c, false);
#else
    return c + (int)(short)(a & 0xFFFFu) * (int)(short)(b & 0xFFFFu) + (int)(short)(a >> 16) * (int)(short)(b >> 16);
#endif
}

/* Outputs 4 v .. 4 v + 3 of one stream S (the history's 46 q values followed by the row's), deinterleaved in LDS:
 *   even[m]   = S[2 m]       8-byte aligned at m = 0; read as dwords even[4 v .. 4 v + 27] -- the int16 at 4 v + 27 is read and not used, it must be there;
 *   centre[n] = S[2 n + 23]  8-byte aligned at n = 0; read centre[4 v .. 4 v + 3].
 * y[i] is output 4 v + i: (acc + 16384) >> 15 clamped to +-32767; n_clamped counts the outputs the clamp changed.  Outputs 4 v and 4 v + 2 take their twelve
 * tap pairs from whole dwords of `even`, 4 v + 1 and 4 v + 3 from the thirteen dwords that straddle them (one funnel shift each, shared by both). */
__device__ __forceinline__ void audio_decimate_four(const short* even, const short* centre, int v, int y[4], int& n_clamped) {
    const unsigned* e32 = reinterpret_cast<const unsigned*>(even + 4 * v);
    unsigned w[14], s[13];
#pragma unroll
    for (int i = 0; i < 14; i++) w[i] = e32[i];
#pragma unroll
    for (int i = 0; i < 13; i++) s[i] = (w[i] >> 16) | (w[i + 1] << 16);
    const unsigned* c32 = reinterpret_cast<const unsigned*>(centre + 4 * v);
    const unsigned c01 = c32[0], c23 = c32[1];
    int acc[4];
    acc[0] = AUDIO_DECIMATE_CENTRE * (int)(short)(c01 & 0xFFFFu);
    acc[1] = AUDIO_DECIMATE_CENTRE * (int)(short)(c01 >> 16);
    acc[2] = AUDIO_DECIMATE_CENTRE * (int)(short)(c23 & 0xFFFFu);
    acc[3] = AUDIO_DECIMATE_CENTRE * (int)(short)(c23 >> 16);
#pragma unroll
    for (int p = 0; p < 12; p++) {
        const unsigned taps = audio_decimate_tap_pair(p);
        acc[0] = audio_decimate_dot2(w[p], taps, acc[0]);
        acc[1] = audio_decimate_dot2(s[p], taps, acc[1]);
        acc[2] = audio_decimate_dot2(w[p + 1], taps, acc[2]);
        acc[3] = audio_decimate_dot2(s[p + 1], taps, acc[3]);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = (acc[i] + 16384) >> 15; /* arithmetic shift */
        const int c = r > 32767 ? 32767 : (r < -32767 ? -32767 : r);
        n_clamped += c != r;
        y[i] = c;
    }
}
#endif /* __HIPCC__ */

}  // namespace airband
