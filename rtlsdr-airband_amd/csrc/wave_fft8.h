/* csrc/wave_fft8.h -- the butterfly and twiddle device functions of the wavefront FFT's exchange kernel (channelizer_fft.hip, channelizer_fft8_kernel), shared with
 * the band scope (band_scope.hip), whose 256- and 512-point transforms are that kernel's: the same values in the same order, so that a channel's bin reads the
 * same in both (tests/test_gpu_band_scope.py holds them to 2 ulp of each other). */
#ifndef AIRBAND_CSRC_WAVE_FFT8_H
#define AIRBAND_CSRC_WAVE_FFT8_H

namespace airband {

namespace {

constexpr int XS = 72;                    /* complex values per row of a wavefront's exchange buffer: 64 + 8, so that two rows land in different banks */
constexpr int XBUF_BYTES = 8 * XS * 8;    /* eight rows */

constexpr float kPi = 3.14159265358979323846f;

__device__ __forceinline__ int bitrev(int v, int bits) { return (int)(__brev((unsigned)v) >> (32 - bits)); }

typedef float v2f __attribute__((ext_vector_type(2))); /* (re, im).  Until round 5 arithmetic on these became v_pk_*_f32; the library is now built WITHOUT packed-f32 instructions
                                                         (_build.py, DEVICE_FLAGS: beside another process's long launches they leave lanes 48 - 63 wrong now and then), so a pair is two scalar operations */

/* x * w with the twiddle as the pair w = (c, s), wr = i w = (-s, c): (x.re, x.re) * w + (x.im, x.im) * wr -- two multiplies and two FMAs (one packed
 * multiply and one packed FMA in a build with packed-f32 instructions; left to itself the compiler spends five instructions on a complex product: it does not negate one half of a packed operand) */
__device__ __forceinline__ v2f cmul(const v2f x, const v2f w, const v2f wr) { return __builtin_elementwise_fma(x.xx, w, x.yy * wr); }
__device__ __forceinline__ v2f rot_i(const v2f w) { return v2f{-w.y, w.x}; }

/* P-point radix-2 decimation-in-frequency FFT in registers, constant twiddles; output in bit-reversed register order */
template <int P>
__device__ __forceinline__ void fft_dif(v2f (&x)[P]) {
#pragma unroll
    for (int half = P / 2; half >= 1; half >>= 1) {
#pragma unroll
        for (int base = 0; base < P; base += 2 * half) {
#pragma unroll
            for (int j = 0; j < half; j++) {
                const int i0 = base + j, i1 = i0 + half;
                const v2f u = x[i0], v = x[i1];
                x[i0] = u + v;
                const v2f d = u - v;
                const float ang = -kPi * (float)j / (float)half; /* W_(2 half)^j: a compile-time constant after unrolling */
                const float wc = __builtin_cosf(ang), ws = __builtin_sinf(ang);
                if (j == 0) x[i1] = d;
                else if (2 * j == half) x[i1] = d.yx * v2f{1.0f, -1.0f}; /* -i: (im, -re), a packed multiply that contracts into the next butterfly's add */
                else x[i1] = cmul(d, v2f{wc, ws}, v2f{-ws, wc});
            }
        }
    }
}

}  // namespace

}  // namespace airband

#endif
