/* csrc/band_watch.hip -- the band watch: the temporal layer over the band survey (airband_hip_set_band_watch).  Per scope row a small table of carrier
 * tracks, advanced once per batch by the row's survey, and one fleet-wide packed list of the batch's events.
 *
 * For every row, with T = max_tracks slots (FREE, TENTATIVE, CONFIRMED), the survey's list peaks[0 .. min(n_peaks, max_peaks)) in its own order and the watch
 * batch number k (include/airband_hip.h has the normative text) --
 *     1. every peak {b, p} in list order: among the tracks that were live at the start of the batch and are not matched yet, the one with the smallest circular
 *        distance min(|b - t|, N - |b - t|) <= match_bins, the lowest slot among equals, takes it (bin = b, power = p, max_power = the larger BIT PATTERN,
 *        misses = 0, hits saturating + 1, last_batch = k; tentative with hits >= confirm_hits: confirmed, an APPEAR event); no such track: the lowest slot that
 *        was free at the start of the batch and is not taken yet is filled (tentative, hits = 1; confirm_hits == 1: confirmed, APPEAR); no such slot: dropped + 1;
 *     2. every track live at the start and not matched, in slot order: misses saturating + 1; tentative: freed; confirmed with misses >= release_misses: a
 *        VANISH event, freed.  A slot freed here was not free at the start: it is not reused in this batch.
 * capi.band_watch_reference() (rtlsdr-airband_amd/capi.py) is this definition in plain Python; tests/test_host_band_watch.py runs this file on the CPU against it.
 *
 * Mapping (wave64, CDNA4).
 * band_watch_kernel: ONE WAVEFRONT per row, four rows per workgroup, no workgroup barrier and no LDS.  A row is at most 64 slots and 64 peaks and its work is
 * one dependent chain (a peak's match depends on what the peaks before it took): there is nothing for a second wavefront to do, and 65 536 rows are 65 536
 * wavefronts -- 64 per SIMD of 256 CUs, which is what hides the latency of each row's few loads.
 *   * lane s holds slot s in registers (24 bytes), lane i holds peak i; the peak loop is wave-uniform, at most 64 rounds, a peak broadcast by readlane;
 *   * every lane forms the key (distance << 8) | slot, all-ones when its slot is not eligible; a cross-lane minimum (six shuffles) picks the match: the
 *     smallest distance, then the lowest slot, and no two lanes share a key;
 *   * the lowest free slot is the lowest set bit of a ballot;
 *   * events are written by the lane that owns the track into the row's slice of a staging area [rows][max_peaks + T], at an index taken from a running
 *     wave-uniform counter (step 1: one event a round at most; step 2: the rank of the lane in the ballot of the vanishing tracks = slot order);
 *   * the row record is written by lane 0.
 * A switched-off dongle (DevConst::disabled, as band_scope.hip recognises it) is not advanced: its table and counters are carried over unchanged -- from the
 * other set where the handle keeps two -- with n_events = 0.
 * band_watch_pack_kernel: ONE workgroup packs the rows' events into events[] in row order by a carried prefix sum of the rows' n_events (band_pack.h, shared with
 * the band follow's list of changes).
 * Integer arithmetic throughout (powers are handled as bit patterns), no atomics, every store by the lane that holds the value: equal input, equal bytes.
 * Every index into the staging area is below max_peaks + T by construction (at most one event per peak round, at most one per slot) and checked again where it
 * is used; n_peaks and a row's n_events are clamped to the sizes the buffers have before anything is indexed with them.
 */
#include <hip/hip_runtime.h>

#include "band_pack.h"
#include "common.h"
#include "kernels.h"

namespace airband {

namespace {

constexpr int WATCH_ROWS = 4, WATCH_THREADS = 64 * WATCH_ROWS;
constexpr unsigned NO_KEY = 0xffffffffu;

typedef unsigned long long u64;

__device__ __forceinline__ unsigned wave_min_key(unsigned k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(k, d);
        k = o < k ? o : k;
    }
    return k;
}

__device__ __forceinline__ void free_slot(airband_hip_band_track& t) {
    t.bin = -1;
    t.power = __uint_as_float(0u);
    t.max_power = __uint_as_float(0u);
    t.first_batch = t.last_batch = 0;
    t.hits = 0;
    t.misses = 0;
    t.state = AIRBAND_WATCH_FREE;
}

}  // namespace

__global__ __launch_bounds__(WATCH_THREADS) void band_watch_kernel(WatchArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int row = (int)blockIdx.x * WATCH_ROWS + ((int)threadIdx.x >> 6);
    if (row >= a.n_rows) return; /* wavefront-uniform */
    const int T = a.max_tracks, N = 1 << a.fft_log, cap = a.max_peaks + T;
    const bool mine = lane < T;
    airband_hip_band_track t;
    free_slot(t);
    if (mine) t = a.tracks_in[(long)row * T + lane];
    airband_hip_band_watch_row rr = a.rows_in[row];
    const int d = a.dev_of_row[row];
    if (a.dev[d].disabled) { /* wavefront-uniform: frozen, carried over */
        if (mine) a.tracks_out[(long)row * T + lane] = t;
        if (lane == 0) {
            rr.n_events = 0;
            a.rows_out[row] = rr;
        }
        return;
    }
    airband_hip_band_event* const stage = a.stage + (long)row * cap;
    const bool live0 = mine && t.state != AIRBAND_WATCH_FREE, free0 = mine && t.state == AIRBAND_WATCH_FREE;
    bool matched = false, taken = false;

    int np = a.summary[row].n_peaks;
    np = np < 0 ? 0 : np;
    np = np > a.max_peaks ? a.max_peaks : np;
    np = __builtin_amdgcn_readfirstlane(np);
    int pbin = -1;
    unsigned ppow = 0;
    if (lane < np) {
        const airband_hip_band_peak p = a.peaks[(long)row * a.max_peaks + lane];
        pbin = p.bin;
        ppow = __float_as_uint(p.power);
    }

    /* ---- 1. the peaks in list order ---- */
    int ne = 0, dropped = 0; /* wavefront-uniform */
#pragma unroll 1
    for (int i = 0; i < np; i++) {
        const int b = (int)__builtin_amdgcn_readlane(pbin, i);
        const unsigned p = (unsigned)__builtin_amdgcn_readlane(ppow, i);
        unsigned key = NO_KEY;
        if (live0 && !matched) {
            int dist = b - t.bin;
            dist = dist < 0 ? -dist : dist;
            dist = dist < N - dist ? dist : N - dist;
            if (dist >= 0 && dist <= a.match_bins) key = ((unsigned)dist << 8) | (unsigned)lane;
        }
        const unsigned win = wave_min_key(key);
        bool emit = false;
        if (win != NO_KEY) {
            if ((unsigned)lane == (win & 255u)) {
                const unsigned mx = __float_as_uint(t.max_power);
                t.bin = b;
                t.power = __uint_as_float(p);
                t.max_power = __uint_as_float(p > mx ? p : mx);
                t.misses = 0;
                t.hits = (uint16_t)(t.hits < 65535 ? t.hits + 1 : 65535);
                t.last_batch = a.batch;
                matched = true;
                if (t.state == AIRBAND_WATCH_TENTATIVE && (int)t.hits >= a.confirm_hits) {
                    t.state = AIRBAND_WATCH_CONFIRMED;
                    emit = true;
                }
            }
        } else {
            const u64 fm = __ballot(free0 && !taken);
            if (fm == 0) {
                dropped++;
            } else if (lane == __builtin_ctzll(fm)) {
                t.bin = b;
                t.power = t.max_power = __uint_as_float(p);
                t.first_batch = t.last_batch = a.batch;
                t.hits = 1;
                t.misses = 0;
                t.state = AIRBAND_WATCH_TENTATIVE;
                taken = true;
                if (a.confirm_hits <= 1) {
                    t.state = AIRBAND_WATCH_CONFIRMED;
                    emit = true;
                }
            }
        }
        const u64 em = __ballot(emit); /* one lane at most */
        if (emit && ne < cap) {
            airband_hip_band_event e;
            e.dev = d;
            e.bin = b;
            e.power = __uint_as_float(p);
            e.kind = AIRBAND_WATCH_APPEAR;
            e.track = (uint8_t)lane;
            e.batches = t.hits;
            stage[ne] = e;
        }
        ne += em != 0 ? 1 : 0;
    }

    /* ---- 2. the tracks nothing matched, in slot order ---- */
    bool vanish = false;
    airband_hip_band_event ev;
    if (live0 && !matched) {
        t.misses = (uint8_t)(t.misses < 255 ? t.misses + 1 : 255);
        if (t.state == AIRBAND_WATCH_TENTATIVE) {
            free_slot(t);
        } else if ((int)t.misses >= a.release_misses) {
            const uint32_t span = t.last_batch - t.first_batch + 1u;
            vanish = true;
            ev.dev = d;
            ev.bin = t.bin;
            ev.power = t.max_power;
            ev.kind = AIRBAND_WATCH_VANISH;
            ev.track = (uint8_t)lane;
            ev.batches = (uint16_t)(span < 65535u ? span : 65535u);
            free_slot(t);
        }
    }
    const u64 vm = __ballot(vanish);
    if (vanish) {
        const int at = ne + __builtin_popcountll(vm & ((1ull << lane) - 1ull));
        if (at < cap) stage[at] = ev;
    }
    ne += __builtin_popcountll(vm);

    /* ---- the table and the row record ---- */
    const u64 live = __ballot(mine && t.state != AIRBAND_WATCH_FREE), conf = __ballot(mine && t.state == AIRBAND_WATCH_CONFIRMED);
    if (mine) a.tracks_out[(long)row * T + lane] = t;
    if (lane == 0) {
        rr.n_live = __builtin_popcountll(live);
        rr.n_confirmed = __builtin_popcountll(conf);
        rr.n_events = ne < cap ? ne : cap;
        rr.dropped += dropped;
        a.rows_out[row] = rr;
    }
}

__global__ __launch_bounds__(PACK_THREADS) void band_watch_pack_kernel(WatchArgs a) {
    pack_rows(&a.rows_out[0].n_events, (int)(sizeof(airband_hip_band_watch_row) / sizeof(int)), reinterpret_cast<const uint4*>(a.stage), a.max_peaks + a.max_tracks,
              reinterpret_cast<uint4*>(a.events), a.max_events, a.n_events, a.n_rows);
}

void launch_band_watch(const WatchArgs& a, hipStream_t stream) {
    if (a.n_rows <= 0 || a.max_tracks < 1 || a.max_tracks > 64 || a.max_peaks < 1 || a.max_peaks > 64) return;
    hipLaunchKernelGGL(band_watch_kernel, dim3((unsigned)((a.n_rows + WATCH_ROWS - 1) / WATCH_ROWS)), dim3(WATCH_THREADS), 0, stream, a);
    hipLaunchKernelGGL(band_watch_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, stream, a);
}

}  // namespace airband
