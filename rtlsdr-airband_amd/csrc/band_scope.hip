/* csrc/band_scope.hip -- the band scope: averaged (and peak) full-band power spectra per dongle, a handful of windows per batch.
 *
 * For K windows of a batch (airband_hip_set_band_scope: window j is the FFT window of the batch's new hop (j * WAVE_BATCH) / K) and every bin k of the
 * transform the channelizer defines (reference: src/rtl_airband.cpp:316-351 sample -> float, :402-455 window, :460 the forward FFT; unnormalised, natural
 * bin order -- the indexing of airband_hip_channel_stats.bin):
 *     mean[k] = (1 / K) * sum over j of |X_j[k]|^2,      peak[k] = max over j of |X_j[k]|^2.
 * Nothing of stage 1 is reused or changed: the kernel reads the batch's input span beside it.
 *
 * Mapping (wave64, CDNA4): one workgroup per selected dongle, four wavefronts; wavefront w takes windows w, w + 4, ...
 *   * the wavefront stages ITS window's raw bytes into its own LDS region -- the window alone, 16 bytes per lane from the aligned byte at or in front of
 *     it, never the bytes between two windows: every hop works alike, 250 bytes (2.0 MS/s u8) or 20 000 (20 MS/s CF32);
 *   * converts with the sample scale and window table the wavefront FFT uses (ChannelizerArgs::window / twiddle: the handle's one copy) and runs the
 *     transform in registers: with fft_size = P x 64, lane l holds samples r * 64 + l, a transform over r inside the lane, the twiddles W_N^(l k1), then
 *     a 64-point transform ACROSS the lanes.  fft 256 and 512: the transform of channelizer_fft.hip's exchange kernel, statement for statement, from the
 *     functions the two share (wave_fft8.h) -- the 64 points as two radix-8 passes with two transposes through an exchange buffer in the wavefront's
 *     region -- so that on a handle whose channelizer is that kernel a channel's bin holds the SAME complex value here and there
 *     (tests/test_gpu_band_scope.py: the scope against read_bins() squared, 2 ulp).  fft 1024 and up: six radix-2 stages with __shfl_xor like its shuffle
 *     kernel, no LDS beside the window; bin k1 + P k2 ends up in the register of k1 of lane bitrev6(k2);
 *   * adds re^2 + im^2 to the sum and max registers of its bins.
 * Bins in passes.  P values per lane fit registers up to P = 16 (fft 1024; sum and max are 2 P more).  Beyond, the bins are walked in NP = P / 16 passes of
 * Q = 16 values of k1 per lane -- pass p holds k1 = p + NP t, t = 0 .. 15.  With r = r1 + Q r2:
 *     Y[p + NP t] = sum over r1 < Q of  W_Q^(r1 t) * { W_P^(r1 p) * sum over r2 < NP of x[r1 + Q r2] W_NP^(r2 p) },
 * i.e. NP multiply-adds per r1 straight from LDS (twiddles that are the same for every lane: scalar loads), then a Q-point transform in the lane.  The pass
 * is the OUTER loop and a window is staged again in every pass (from the L2: K windows of at most 64 KiB per dongle), so that no instantiation holds more
 * than 16 complex values, 16 sums and 16 maxima per lane: nothing spills (scripts/isa_count.py).
 * After a pass's windows the wavefronts leave their sums and maxima in their LDS regions, in bin order; wavefront 0 adds them IN WAVE ORDER and stores.
 * One pass (fft_size up to 1024): consecutive lanes store consecutive bins, whole 128-byte lines.  NP passes: a pass's bins are NP apart, a line fills up
 * over the passes.
 * Summation order is therefore fixed -- ascending window inside a wavefront, then wavefronts ascending -- and there are no atomics: equal input, equal bits.
 *
 * LDS.  A region is one window + 32 bytes (alignment slack) -- behind the 4 608-byte exchange buffer at fft 256 / 512 -- at least the 2 x Q x 64 floats of the
 * pass's partial results.  THE RULE: four wavefronts
 * while four regions fit a CU's 160 KiB, else two, else one (scope_waves()).  CF32 at fft 8192 is 64 KiB a window: two wavefronts; everything else: four.
 *
 * A dongle that is switched off (airband_hip_device_enable) is skipped: its rows keep what they held.  Where the handle keeps two sets of rows (the scope of
 * the batch being collected and of the batch in flight) "what they held" is in the OTHER set, and the workgroup copies it over.
 *
 * Arithmetic: float32, FMA contraction allowed (as the wavefront FFT: ~1e-7 of the bins' RMS from a float64 transform).
 * tests/test_host_band_scope.py runs this file on the CPU (lanes as fibers) against a float64 evaluation of the defining sum.
 */
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "wave_fft8.h"
#include "wave_lds.h"

namespace airband {

namespace {

constexpr int SCOPE_LDS_MAX = 160 * 1024;

/* complex sample n of the staged window, converted and multiplied by w = window[n] x sample scale (src/rtl_airband.cpp:316-324,402-455; the expressions
 * of channelizer_fft.hip) */
template <int FMT>
__device__ __forceinline__ void scope_sample(const uint8_t* wp, int n, float w, float& re, float& im) {
    if (FMT == AIRBAND_SFMT_U8) {
        const unsigned v = *reinterpret_cast<const unsigned short*>(wp + 2 * n);
        re = ((float)(v & 0xffu) - 127.5f) * w;
        im = ((float)(v >> 8) - 127.5f) * w;
    } else if (FMT == AIRBAND_SFMT_S8) {
        const char2 v = *reinterpret_cast<const char2*>(wp + 2 * n); /* i / 128 for every byte, -128 included (channelizer_fft.hip) */
        re = (float)v.x * w;
        im = (float)v.y * w;
    } else if (FMT == AIRBAND_SFMT_S16) {
        const short2 v = *reinterpret_cast<const short2*>(wp + 4 * n);
        re = (float)v.x * w;
        im = (float)v.y * w;
    } else {
        const float2 v = *reinterpret_cast<const float2*>(wp + 8 * n);
        re = v.x * w;
        im = v.y * w;
    }
}

/* LOGP: log2(fft_size / 64); LOGQ: log2 of the values of k1 a lane holds per pass */
template <int LOGP, int LOGQ, int FMT>
__device__ __forceinline__ void scope_body(const ScopeArgs& a, uint8_t* lds_all) {
    constexpr int P = 1 << LOGP, Q = 1 << LOGQ, NP = P / Q;
    constexpr int N = P * 64;
    constexpr bool EXCH = LOGP <= 3; /* 256 and 512 points: the exchange kernel's transform (wave_fft8.h), value for value */
    const int lane = threadIdx.x & 63;
    const int wave = (int)(threadIdx.x >> 6), n_waves = (int)(blockDim.x >> 6);
    const int row = blockIdx.x;
    const int d = a.dev_of_row[row];
    const DevConst dev = a.dev[d];
    if (dev.disabled) { /* block-uniform, in front of every barrier */
        if (a.mean && a.prev_mean)
            for (int k = threadIdx.x; k < N; k += blockDim.x) a.mean[(long)row * N + k] = a.prev_mean[(long)row * N + k];
        if (a.peak && a.prev_peak)
            for (int k = threadIdx.x; k < N; k += blockDim.x) a.peak[(long)row * N + k] = a.prev_peak[(long)row * N + k];
        return;
    }
    const int bps2 = 2 * a.bytes_per_sample;
    const long win_bytes = (long)N * bps2;
    uint8_t* const region = lds_all + (long)wave * a.region_bytes;
    uint8_t* const stage = region + (EXCH ? XBUF_BYTES : 0); /* the exchange buffer first, the window behind it */
    const float pre = FMT == AIRBAND_SFMT_U8 ? (1.0f / 127.5f) : FMT == AIRBAND_SFMT_S8 ? (1.0f / 128.0f) : dev.scale;
    const uint8_t* const span = a.iq + (long)d * a.iq_stride;
    const long span_bytes = ((long)(a.span_hops - 1) * a.hop_samples + N) * bps2; /* what the API promises of the dongle's span */

    /* one pass: window x scale in registers */
    float win[NP == 1 ? P : 1];
    if (NP == 1) {
#pragma unroll
        for (int r = 0; r < P; r++) win[r] = a.window[r * 64 + lane] * pre;
    }
    /* cross-lane stage twiddles: distance dd = 32 >> st, W_(2dd)^(lane mod dd); lanes with the bit clear use 1 (channelizer_fft.hip) */
    float cwr[6], cwi[6];
#pragma unroll
    for (int st = 0; st < 6; st++) {
        const int dd = 32 >> st;
        const float2 w = a.twiddle[(lane & (dd - 1)) * (N / (2 * dd))];
        const bool lower = (lane & dd) != 0;
        cwr[st] = lower ? w.x : 1.0f;
        cwi[st] = lower ? w.y : 0.0f;
    }

    /* 256 and 512 points: the constants of channelizer_fft8_kernel<LOGP, 0> -- W_N^(lane k1) by register, W_64^(b c), and the lane's places in the exchange buffer */
    constexpr int PX = EXCH ? P : 1;
    v2f etw[PX], etwr[PX], ecw[8], ecwr[8];
    v2f* const xb = reinterpret_cast<v2f*>(region);
    const int b8 = lane & 7, jx = (lane >> 3) & (P - 1);
    v2f* const x_w1 = xb + lane;
    v2f* const x_r1 = xb + jx * XS + b8;
    v2f* const x_w2 = xb + jx * XS + b8 * 9;
    v2f* const x_r2 = xb + jx * XS + b8;
    v2f* const x_w3 = xb + jx * XS + b8;
    if (EXCH) {
#pragma unroll
        for (int rho = 0; rho < PX; rho++) {
            const float2 w = a.twiddle[(lane * bitrev(rho, LOGP)) & (N - 1)];
            etw[rho] = v2f{w.x, w.y};
            etwr[rho] = rot_i(etw[rho]);
        }
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const float2 w = a.twiddle[(b8 * bitrev(t, 3) * P) & (N - 1)];
            ecw[t] = v2f{w.x, w.y};
            ecwr[t] = rot_i(ecw[t]);
        }
    }

#pragma unroll 1
    for (int p = 0; p < NP; p++) {
        /* W_N^(lane k1) for the k1 = p + NP bitrev(rho) register rho holds after the in-lane transform */
        float twr[Q], twi[Q];
#pragma unroll
        for (int rho = 0; rho < Q; rho++) {
            const int k1 = p + NP * bitrev(rho, LOGQ);
            const float2 w = a.twiddle[(lane * k1) & (N - 1)];
            twr[rho] = w.x;
            twi[rho] = w.y;
        }
        float sum[Q], mx[Q];
#pragma unroll
        for (int rho = 0; rho < Q; rho++) sum[rho] = mx[rho] = 0.0f;

        for (int j = wave; j < a.n_windows; j += n_waves) { /* ascending windows */
            /* ---- stage window j: coalesced 16 B per lane, HBM / L2 -> this wavefront's region ---- */
            const long begin = (long)(a.first_hop + (int)(((long)j * a.wave_batch) / a.n_windows)) * a.hop_samples * bps2;
            const uint8_t* src = span + begin;
            const long mis = (long)((uintptr_t)src & 15);
            const uint8_t* src_al = src - mis;
            const long n16 = (win_bytes + mis + 15) >> 4;
            /* 16-byte pieces that would start in front of the dongle's span or end past it are fetched byte by byte: nothing outside the documented span is touched */
            const long avail_begin = begin == 0 ? mis : 0;
            const long avail_end = span_bytes - begin + mis; /* relative to src_al */
            AB_WAVE_SYNC(); /* every lane is done with the window before */
            for (long i = lane; i < n16; i += 64) {
                const long o = i << 4;
                if (o >= avail_begin && o + 16 <= avail_end) {
                    *reinterpret_cast<uint4*>(stage + o) = *reinterpret_cast<const uint4*>(src_al + o);
                } else {
                    for (int b = 0; b < 16; b++) stage[o + b] = (o + b >= avail_begin && o + b < avail_end) ? src_al[o + b] : (uint8_t)0;
                }
            }
            AB_WAVE_SYNC();
            const uint8_t* wp = stage + mis;

            if (EXCH) {
                /* channelizer_fft8_kernel's transform, statement for statement: in-lane FFT over r, the lane twiddles, the 64-point FFT over the lanes as 8 x 8
                 * (two radix-8 passes and two transposes through the exchange buffer).  The buffer then holds bin k1 + P k2 at [register index of k1][k2]. */
                v2f x[PX];
#pragma unroll
                for (int r = 0; r < PX; r++) {
                    float vr, vi;
                    scope_sample<FMT>(wp, r * 64 + lane, win[r], vr, vi);
                    x[r] = v2f{vr, vi};
                }
                fft_dif<PX>(x);
#pragma unroll
                for (int g = 0; g < PX; g += 4) {
                    v2f t[4];
#pragma unroll
                    for (int rho = g; rho < g + 4; rho++) t[rho - g] = x[rho].yy * etwr[rho];
#pragma unroll
                    for (int rho = g; rho < g + 4; rho++)
                        if (rho > 0) x[rho] = __builtin_elementwise_fma(x[rho].xx, etw[rho], t[rho - g]);
                }
#pragma unroll
                for (int jr = 0; jr < PX; jr++) x_w1[jr * XS] = x[jr];
                AB_WAVE_SYNC();
                v2f z[8];
#pragma unroll
                for (int i = 0; i < 8; i++) z[i] = x_r1[8 * i];
                AB_WAVE_SYNC();
                fft_dif<8>(z);
#pragma unroll
                for (int g = 0; g < 8; g += 4) {
                    v2f u[4];
#pragma unroll
                    for (int t = g; t < g + 4; t++) u[t - g] = z[t].yy * ecwr[t];
#pragma unroll
                    for (int t = g; t < g + 4; t++)
                        if (t > 0) z[t] = __builtin_elementwise_fma(z[t].xx, ecw[t], u[t - g]);
                }
#pragma unroll
                for (int t = 0; t < 8; t++) x_w2[bitrev(t, 3)] = z[t];
                AB_WAVE_SYNC();
#pragma unroll
                for (int i = 0; i < 8; i++) z[i] = x_r2[9 * i];
                AB_WAVE_SYNC();
                fft_dif<8>(z);
#pragma unroll
                for (int t = 0; t < 8; t++) x_w3[8 * bitrev(t, 3)] = z[t];
                AB_WAVE_SYNC();
#pragma unroll
                for (int rho = 0; rho < PX; rho++) { /* register rho: bin bitrev(rho) + P lane */
                    const v2f v = xb[rho * XS + lane];
                    const float pw = v.x * v.x + v.y * v.y;
                    sum[rho] += pw;
                    mx[rho] = fmaxf(mx[rho], pw);
                }
                continue; /* (the next window's staging, or the partial results, wait for these reads: AB_WAVE_SYNC) */
            }
            float xr[Q], xi[Q];
            if (NP == 1) {
#pragma unroll
                for (int r = 0; r < P; r++) scope_sample<FMT>(wp, r * 64 + lane, win[r], xr[r], xi[r]);
            } else {
#pragma unroll
                for (int r1 = 0; r1 < Q; r1++) xr[r1] = xi[r1] = 0.0f;
#pragma unroll 1
                for (int r2 = 0; r2 < NP; r2++) { /* a loop, not unrolled: sixteen samples and window values in flight, not all P */
                    const float2 w = a.twiddle[(r2 * p * (N / NP)) & (N - 1)]; /* W_NP^(r2 p): the same on every lane */
#pragma unroll
                    for (int r1 = 0; r1 < Q; r1++) {
                        const int n = (r1 + Q * r2) * 64 + lane;
                        float vr, vi;
                        scope_sample<FMT>(wp, n, a.window[n] * pre, vr, vi);
                        xr[r1] += vr * w.x - vi * w.y;
                        xi[r1] += vr * w.y + vi * w.x;
                    }
                }
#pragma unroll
                for (int r1 = 1; r1 < Q; r1++) {
                    const float2 w1 = a.twiddle[(r1 * p * 64) & (N - 1)]; /* W_P^(r1 p) */
                    const float tr = xr[r1] * w1.x - xi[r1] * w1.y;
                    xi[r1] = xr[r1] * w1.y + xi[r1] * w1.x;
                    xr[r1] = tr;
                }
            }
            /* in-lane Q-point DIF FFT (output in bit-reversed register order), as channelizer_fft.hip's shuffle kernel */
#pragma unroll
            for (int half = Q / 2; half >= 1; half >>= 1) {
#pragma unroll
                for (int base = 0; base < Q; base += 2 * half) {
#pragma unroll
                    for (int jj = 0; jj < half; jj++) {
                        const int i0 = base + jj, i1 = i0 + half;
                        const float ar = xr[i0], ai = xi[i0], br = xr[i1], bi = xi[i1];
                        xr[i0] = ar + br;
                        xi[i0] = ai + bi;
                        const float dr = ar - br, di = ai - bi;
                        const float ang = -kPi * (float)jj / (float)half; /* W_(2 half)^jj: a compile-time constant after unrolling */
                        const float wc = __builtin_cosf(ang), ws = __builtin_sinf(ang);
                        if (jj == 0) {
                            xr[i1] = dr;
                            xi[i1] = di;
                        } else if (2 * jj == half) { /* -i */
                            xr[i1] = di;
                            xi[i1] = -dr;
                        } else {
                            xr[i1] = dr * wc - di * ws;
                            xi[i1] = dr * ws + di * wc;
                        }
                    }
                }
            }
            /* per-lane twiddles W_N^(lane k1) */
#pragma unroll
            for (int rho = 0; rho < Q; rho++) {
                if (NP == 1 && rho == 0) continue; /* k1 = 0 */
                const float tr = xr[rho] * twr[rho] - xi[rho] * twi[rho];
                const float ti = xr[rho] * twi[rho] + xi[rho] * twr[rho];
                xr[rho] = tr;
                xi[rho] = ti;
            }
            /* 64-point DIF FFT across the lanes: six radix-2 stages with __shfl_xor butterflies */
#pragma unroll
            for (int st = 0; st < 6; st++) {
                const int dd = 32 >> st;
                const float sgn = (lane & dd) ? -1.0f : 1.0f;
#pragma unroll
                for (int rho = 0; rho < Q; rho++) {
                    const float pr_ = __shfl_xor(xr[rho], dd);
                    const float pi_ = __shfl_xor(xi[rho], dd);
                    const float tr = fmaf(xr[rho], sgn, pr_);
                    const float ti = fmaf(xi[rho], sgn, pi_);
                    xr[rho] = tr * cwr[st] - ti * cwi[st];
                    xi[rho] = tr * cwi[st] + ti * cwr[st];
                }
            }
#pragma unroll
            for (int rho = 0; rho < Q; rho++) {
                const float pw = xr[rho] * xr[rho] + xi[rho] * xi[rho];
                sum[rho] += pw;
                mx[rho] = fmaxf(mx[rho], pw);
            }
        }

        /* ---- the wavefronts' partial results, in the pass's bin order m = t + Q k2 (bin k = p + NP m), then wavefront 0 in wave order ---- */
        AB_WAVE_SYNC(); /* the last window has been read */
        float* part = reinterpret_cast<float*>(region);
        const int k2 = EXCH ? lane : bitrev(lane, 6);
#pragma unroll
        for (int rho = 0; rho < Q; rho++) {
            const int m = bitrev(rho, LOGQ) + Q * k2;
            part[m] = sum[rho];
            part[Q * 64 + m] = mx[rho];
        }
        __syncthreads();
        if (wave == 0) {
            const float inv = 1.0f / (float)a.n_windows;
#pragma unroll 1
            for (int i = 0; i < Q; i++) {
                const int m = i * 64 + lane;
                float s = 0.0f, x = 0.0f;
                for (int w = 0; w < n_waves; w++) {
                    const float* pw = reinterpret_cast<const float*>(lds_all + (long)w * a.region_bytes);
                    s += pw[m];
                    x = fmaxf(x, pw[Q * 64 + m]);
                }
                const long o = (long)row * N + p + NP * m;
                if (a.mean) a.mean[o] = s * inv;
                if (a.peak) a.peak[o] = x;
            }
        }
        if (NP > 1) __syncthreads(); /* the regions are staged into again */
    }
}

template <int LOGP, int LOGQ>
__global__ __launch_bounds__(256) void band_scope_kernel(ScopeArgs a) {
    AB_DYNAMIC_LDS_BYTES(lds_scope);
    switch (a.sfmt) { /* the format is the launch's: chosen once */
        case AIRBAND_SFMT_U8: scope_body<LOGP, LOGQ, AIRBAND_SFMT_U8>(a, lds_scope); break;
        case AIRBAND_SFMT_S8: scope_body<LOGP, LOGQ, AIRBAND_SFMT_S8>(a, lds_scope); break;
        case AIRBAND_SFMT_S16: scope_body<LOGP, LOGQ, AIRBAND_SFMT_S16>(a, lds_scope); break;
        default: scope_body<LOGP, LOGQ, AIRBAND_SFMT_F32>(a, lds_scope); break;
    }
}

template <int LOGP, int LOGQ>
void scope_launch_one(const ScopeArgs& a, int waves, hipStream_t stream) {
    const size_t lds = (size_t)waves * a.region_bytes;
    if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&band_scope_kernel<LOGP, LOGQ>), hipFuncAttributeMaxDynamicSharedMemorySize, SCOPE_LDS_MAX);
    hipLaunchKernelGGL((band_scope_kernel<LOGP, LOGQ>), dim3((unsigned)a.n_rows), dim3(64 * waves), lds, stream, a);
}

}  // namespace

/* bytes of one wavefront's LDS region: the window and its alignment slack (a multiple of 16), at least a pass's partial sums and maxima */
long scope_region_bytes(int fft_log, int bytes_per_sample) {
    const long win = (((1L << fft_log) * 2 * bytes_per_sample + 32) + 15) & ~15L;
    const int logq = fft_log - 6 < 4 ? fft_log - 6 : 4;
    const long part = 2L * (64L << logq) * (long)sizeof(float);
    const long need = win + (fft_log <= 9 ? XBUF_BYTES : 0); /* 256 / 512 points: the exchange buffer in front of the window */
    return need > part ? need : part;
}

/* THE RULE: four wavefronts while four regions fit a CU's 160 KiB, else two, else one */
int scope_waves(int fft_log, int bytes_per_sample) {
    const long r = scope_region_bytes(fft_log, bytes_per_sample);
    return 4 * r <= SCOPE_LDS_MAX ? 4 : 2 * r <= SCOPE_LDS_MAX ? 2 : 1;
}

void launch_band_scope(const ScopeArgs& a_in, hipStream_t stream) {
    ScopeArgs a = a_in;
    a.region_bytes = (int)scope_region_bytes(a.fft_log, a.bytes_per_sample);
    const int waves = scope_waves(a.fft_log, a.bytes_per_sample);
    if (a.n_rows <= 0 || a.n_windows <= 0) return;
    switch (a.fft_log - 6) { /* <values per lane, values per lane and pass> */
        case 2: scope_launch_one<2, 2>(a, waves, stream); break;
        case 3: scope_launch_one<3, 3>(a, waves, stream); break;
        case 4: scope_launch_one<4, 4>(a, waves, stream); break;
        case 5: scope_launch_one<5, 4>(a, waves, stream); break;
        case 6: scope_launch_one<6, 4>(a, waves, stream); break;
        case 7: scope_launch_one<7, 4>(a, waves, stream); break;
        default: break;
    }
}

}  // namespace airband
