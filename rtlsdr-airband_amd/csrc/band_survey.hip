/* csrc/band_survey.hip -- the band survey: what a host would work out of a band scope row, worked out where the row is (airband_hip_set_band_survey).
 *
 * For every scope row P[0 .. N) of ONE trace (N = fft_size, natural bin order; band_scope.hip writes it just in front of this kernel on the same stream) --
 * every value compared BY ITS BIT PATTERN as an unsigned 32-bit integer: the float order for the non-negative floats the scope produces, a total order that
 * indexes nothing for any other bits --
 *     floor      the value of rank r = min(N - 1, N * floor_permille / 1000) in ascending order (0-based)
 *     threshold  floor * threshold_ratio: the ONE float operation of this file
 *     max_power, max_bin   the largest value, the lowest bin among equals
 *     n_over     bins with P[k] > threshold
 *     peaks      bins with P[k] > threshold, P[k] >= P[k - 1] and P[k] > P[k + 1] (circular: a plateau counts once, at its last bin) that are not COVERED --
 *                within guard_bins (circular distance) of the prepare-time bin of a channel configured on the dongle; guard_bins < 0: nothing is covered --
 *                n_peaks of them, the max_peaks strongest listed by power descending, equal powers by ascending bin, {-1, 0} behind them.
 * capi.band_survey_reference() (rtlsdr-airband_amd/capi.py) is this definition in numpy; tests/test_host_band_survey.py runs this file on the CPU against it.
 *
 * Mapping (wave64, CDNA4): one workgroup of four wavefronts per row; thread t owns bins t, t + 256, ... (at most 32 at fft 8192).
 *   * the row goes to LDS as bit patterns, 16 bytes per lane (at most 32 KiB); the dongle's channel bins (at most AB_MAX_CH_PER_DEV) once beside it;
 *   * the rank by a four-pass 8-bit radix select from the top byte down: a 256-entry LDS histogram (integer LDS adds) of the values that share the prefix
 *     found so far, thread t takes entry t, an inclusive scan over the 256 counts (shuffles inside a wavefront, four totals through LDS), and the one thread
 *     whose interval holds the rank publishes its byte and the rank inside it;
 *   * one pass over the thread's bins with both neighbours from LDS (consecutive lanes, consecutive banks): over, local maximum, covered -> a count, a
 *     register mask of the thread's peaks, its best peak and its largest value as 64-bit keys (bits << 32) | (N - 1 - bin): larger power first, then the
 *     LOWER bin, and no two bins share a key;
 *   * min(n_peaks, max_peaks) rounds of a workgroup maximum of the threads' best keys (cross-lane inside a wavefront, four keys through LDS in two alternating
 *     sets: one barrier a round); the owner of the winner strikes it from its mask and looks up its next best.
 * Integer arithmetic throughout but for the threshold, no global atomics, results written by ordinary stores of the lanes that hold them, nothing depends on
 * the order in which lanes or wavefronts arrive: equal input, equal bits.  Every index into the row is masked to N - 1, every histogram index to 255 and the
 * winner's bin comes out of the low half of a key, which only ever holds N - 1 - bin: no bit pattern in a row can send an access outside the row.
 * A switched-off dongle needs nothing here: band_scope.hip has left (or carried over) its last row, and the same row gives the same survey.
 */
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"
#include "wave_lds.h"

namespace airband {

namespace {

constexpr int SURVEY_THREADS = 256, SURVEY_WAVES = SURVEY_THREADS / 64;
/* LDS behind the row: histogram [256], keys [3][SURVEY_WAVES] (the first reduction, then two alternating sets), wave totals [4], the selected byte and rank [2 (+2)],
 * the wavefronts' counts [4], the dongle's channel bins [AB_MAX_CH_PER_DEV] */
constexpr int SV_HIST = 0, SV_KEYS = SV_HIST + 256 * 4, SV_WTOT = SV_KEYS + 3 * SURVEY_WAVES * 8, SV_SEL = SV_WTOT + SURVEY_WAVES * 4, SV_CNT = SV_SEL + 16,
              SV_CHAN = SV_CNT + SURVEY_WAVES * 4, SV_EXTRA = SV_CHAN + AB_MAX_CH_PER_DEV * 4;

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max_key(u64 k) {
    unsigned hi = (unsigned)(k >> 32), lo = (unsigned)k;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned ohi = __shfl_xor(hi, d), olo = __shfl_xor(lo, d);
        const bool take = ohi > hi || (ohi == hi && olo > lo);
        hi = take ? ohi : hi;
        lo = take ? olo : lo;
    }
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 max4(const u64* p) {
    const u64 a = p[0] > p[1] ? p[0] : p[1], b = p[2] > p[3] ? p[2] : p[3];
    return a > b ? a : b;
}

}  // namespace

__global__ __launch_bounds__(SURVEY_THREADS) void band_survey_kernel(SurveyArgs a) {
    AB_DYNAMIC_LDS_BYTES(lds_survey);
    const int N = 1 << a.fft_log, NM = N - 1;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = (int)blockIdx.x;
    unsigned* const bits = reinterpret_cast<unsigned*>(lds_survey);
    uint8_t* const extra = lds_survey + (long)N * 4;
    int* const hist = reinterpret_cast<int*>(extra + SV_HIST);
    u64* const keys = reinterpret_cast<u64*>(extra + SV_KEYS);
    unsigned* const wtot = reinterpret_cast<unsigned*>(extra + SV_WTOT);
    unsigned* const sel = reinterpret_cast<unsigned*>(extra + SV_SEL);
    unsigned* const cntw = reinterpret_cast<unsigned*>(extra + SV_CNT);
    int* const chan = reinterpret_cast<int*>(extra + SV_CHAN);

    /* ---- the row (bit patterns) and the dongle's channel bins -> LDS ---- */
    const uint4* const src = reinterpret_cast<const uint4*>(a.rows + (long)row * N);
    for (int i = tid; i < N / 4; i += SURVEY_THREADS) reinterpret_cast<uint4*>(bits)[i] = src[i];
    const int b0 = a.bin_first[row];
    int nb = a.bin_first[row + 1] - b0;
    nb = nb > AB_MAX_CH_PER_DEV ? AB_MAX_CH_PER_DEV : nb;
    for (int i = tid; i < nb; i += SURVEY_THREADS) chan[i] = a.bins[b0 + i] & NM;
    hist[tid] = 0;
    __syncthreads();

    /* ---- rank a.rank by radix select: the top byte first ---- */
    unsigned prefix = 0, known = 0, r = (unsigned)a.rank;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int k = tid; k < N; k += SURVEY_THREADS) {
            const unsigned v = bits[k];
            if ((v & known) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1);
        }
        __syncthreads();
        const unsigned c = (unsigned)hist[tid];
        unsigned incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, (unsigned)d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; w++) incl += wtot[w];
        hist[tid] = 0; /* entry t is read by thread t alone: ready for the next pass */
        if (incl - c <= r && r < incl) { /* exactly one thread: the counts sum to more than r */
            sel[0] = (unsigned)tid;
            sel[1] = r - (incl - c);
        }
        __syncthreads();
        prefix |= sel[0] << shift;
        known |= 255u << shift;
        r = sel[1];
    }
    const unsigned floor_bits = prefix;
    const unsigned thr = __float_as_uint(__uint_as_float(floor_bits) * a.ratio);

    /* ---- over, local maximum, covered ---- */
    unsigned mine = 0, count = 0; /* bit j: bin tid + 256 j is a peak; count: bins over | peaks << 16 (at most 8 192 and 4 096 a row) */
    u64 best = 0, top = 0;        /* a peak's key is above 2^32 (its value is above the threshold): 0 is "none" */
    {
        int j = 0;
        for (int k = tid; k < N; k += SURVEY_THREADS, j++) {
            const unsigned v = bits[k];
            const u64 key = ((u64)v << 32) | (unsigned)(NM - k);
            top = key > top ? key : top;
            if (v > thr) {
                count += 1u;
                if (v >= bits[(k - 1) & NM] && v > bits[(k + 1) & NM]) {
                    bool covered = false;
                    if (a.guard_bins >= 0)
                        for (int i = 0; i < nb; i++) {
                            int d = k - chan[i];
                            d = d < 0 ? -d : d;
                            d = d < N - d ? d : N - d;
                            covered = covered || d <= a.guard_bins;
                        }
                    if (!covered) {
                        mine |= 1u << j;
                        count += 1u << 16;
                        best = key > best ? key : best;
                    }
                }
            }
        }
    }
    top = wave_max_key(top);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d);
    if (lane == 0) {
        keys[wave] = top;
        cntw[wave] = count;
    }
    __syncthreads();
    top = max4(keys);
    count = cntw[0] + cntw[1] + cntw[2] + cntw[3];
    const int n_over = (int)(count & 0xffffu), n_peaks = (int)(count >> 16);
    if (tid == 0) {
        airband_hip_band_summary s;
        s.floor = __uint_as_float(floor_bits);
        s.threshold = __uint_as_float(thr);
        s.max_power = __uint_as_float((unsigned)(top >> 32));
        s.max_bin = NM - (int)((unsigned)top & (unsigned)NM);
        s.n_over = n_over;
        s.n_peaks = n_peaks;
        s.reserved[0] = s.reserved[1] = 0;
        a.summary[row] = s;
    }

    /* ---- the strongest peaks, one workgroup maximum each ---- */
    airband_hip_band_peak* const out = a.peaks + (long)row * a.max_peaks;
    const int n_out = n_peaks < a.max_peaks ? n_peaks : a.max_peaks; /* the same in every thread */
#pragma unroll 1
    for (int i = 0; i < n_out; i++) {
        u64* const set = keys + SURVEY_WAVES * (1 + (i & 1)); /* written again two rounds on: every thread has passed the barrier between */
        const u64 w = wave_max_key(best);
        if (lane == 0) set[wave] = w;
        __syncthreads();
        const u64 win = max4(set);
        const int bin = NM - (int)((unsigned)win & (unsigned)NM);
        if (tid == 0) {
            airband_hip_band_peak p;
            p.bin = bin;
            p.power = __uint_as_float((unsigned)(win >> 32));
            out[i] = p;
        }
        if ((bin & (SURVEY_THREADS - 1)) == tid) { /* the owner: strike it, find the next best of its peaks */
            mine &= ~(1u << (bin >> 8));
            best = 0;
            for (unsigned m = mine; m; m &= m - 1) {
                const int k = tid + SURVEY_THREADS * __builtin_ctz(m);
                const u64 key = ((u64)bits[k & NM] << 32) | (unsigned)(NM - (k & NM));
                best = key > best ? key : best;
            }
        }
    }
    for (int i = n_out + tid; i < a.max_peaks; i += SURVEY_THREADS) {
        airband_hip_band_peak p;
        p.bin = -1;
        p.power = 0.0f;
        out[i] = p;
    }
}

size_t survey_lds_bytes(int fft_log) { return ((size_t)4 << fft_log) + SV_EXTRA; }

void launch_band_survey(const SurveyArgs& a, hipStream_t stream) {
    if (a.n_rows <= 0 || a.fft_log < 8 || a.fft_log > 13) return; /* 256 threads own whole bins from fft 256 on; 8 192 bins are 32 a thread, the register mask's width */
    hipLaunchKernelGGL(band_survey_kernel, dim3((unsigned)a.n_rows), dim3(SURVEY_THREADS), survey_lds_bytes(a.fft_log), stream, a);
}

}  // namespace airband
