// tests/host_watch_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_band_watch.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the band watch's source itself -- csrc/band_watch.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its two kernels with their
// wavefront semantics on the CPU (lanes as fibers; shuffles, ballots and barriers as rendezvous points), launched by the file's own launch_band_watch().
// A stand-alone program: `host_watch <cases file> <results file>`.  The cases file holds sequences of batches (parameters, then per batch which rows are
// switched off and the rows' survey lists); the results file gets, per batch, what the kernels left: tracks, row records, the event count and the events.  The
// test compares those bytes with capi.band_watch_reference().  Every buffer the kernels write is poisoned first, and the events buffer carries a guard zone
// behind max_events that must come back untouched.  Having its own main, the same file is what runs under a host sanitizer.
//
// Cases file (little-endian int32 unless noted): n_cases, then per case
//     n_rows fft_log max_peaks max_tracks match_bins confirm_hits release_misses max_events n_batches two_sets pack first_batch has_init dev_of_row[n_rows]
//     has_init != 0: tracks [n_rows][max_tracks] and rows [n_rows] the first batch starts from (else: every slot free, zero records)
//     kind 0, per batch:  disabled[n_rows]  n_peaks[n_rows]  peaks[n_rows][max_peaks] {int32 bin, uint32 power bits}
//     kind 1 (pack == 2: the pack kernel alone, one launch):  n_events[n_rows], then the rows' events, n_events[row] records of 16 bytes each
// Results file, per batch: tracks [n_rows][max_tracks] (24 bytes), rows [n_rows] (16 bytes), and
//     pack == 0: the staged events of every row, rows[row].n_events records each;  pack != 0: int32 n_events, then min(n_events, max_events) records.
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/band_watch.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD = 64; // events behind max_events that nothing may write

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_watch", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int n_rows = in.i32(), fft_log = in.i32(), max_peaks = in.i32(), T = in.i32(), M = in.i32(), C = in.i32(), R = in.i32(), E = in.i32(), n_batches = in.i32(),
                  two_sets = in.i32(), pack = in.i32();
        const unsigned first_batch = (unsigned)in.i32();
        const int has_init = in.i32();
        if (n_rows < 1 || max_peaks < 1 || max_peaks > 64 || T < 1 || T > 64 || E < 1) return 2;
        const int cap = max_peaks + T;
        std::vector<int> dev_of_row((size_t)n_rows);
        in.take(dev_of_row.data(), 4 * (size_t)n_rows);
        int n_dev = 0;
        for (int d : dev_of_row) n_dev = d + 1 > n_dev ? d + 1 : n_dev;
        std::vector<DevConst> dev((size_t)n_dev);
        std::memset(dev.data(), 0, sizeof(DevConst) * dev.size());
        airband_hip_band_track* tracks[2] = {aligned<airband_hip_band_track>((size_t)n_rows * T), aligned<airband_hip_band_track>((size_t)n_rows * T)};
        airband_hip_band_watch_row* rows[2] = {aligned<airband_hip_band_watch_row>(n_rows), aligned<airband_hip_band_watch_row>(n_rows)};
        airband_hip_band_event* stage = aligned<airband_hip_band_event>((size_t)n_rows * cap);
        airband_hip_band_event* events = aligned<airband_hip_band_event>((size_t)E + GUARD);
        airband_hip_band_summary* summary = aligned<airband_hip_band_summary>(n_rows);
        airband_hip_band_peak* peaks = aligned<airband_hip_band_peak>((size_t)n_rows * max_peaks);
        for (int q = 0; q < 2; q++) {
            std::memset(rows[q], 0, sizeof(rows[q][0]) * n_rows);
            std::memset(tracks[q], 0, sizeof(tracks[q][0]) * n_rows * T);
            for (int i = 0; i < n_rows * T; i++) tracks[q][i].bin = -1;
        }
        if (has_init) { // where batch 0 reads its tables from: the other set where there are two
            const int q = two_sets ? 1 : 0;
            in.take(tracks[q], sizeof(tracks[q][0]) * (size_t)n_rows * T);
            in.take(rows[q], sizeof(rows[q][0]) * (size_t)n_rows);
        }
        WatchArgs a;
        std::memset(&a, 0, sizeof(a));
        a.dev = dev.data();
        a.dev_of_row = dev_of_row.data();
        a.summary = summary;
        a.peaks = peaks;
        a.stage = stage;
        a.events = events;
        a.n_rows = n_rows;
        a.fft_log = fft_log;
        a.max_peaks = max_peaks;
        a.max_tracks = T;
        a.match_bins = M;
        a.confirm_hits = C;
        a.release_misses = R;
        a.max_events = E;
        int count = 0;
        a.n_events = &count;
        for (int b = 0; b < n_batches; b++) {
            const int set = two_sets ? (b & 1) : 0, prev = two_sets ? set ^ 1 : 0;
            a.tracks_in = tracks[prev];
            a.rows_in = rows[prev];
            a.tracks_out = tracks[set];
            a.rows_out = rows[set];
            a.batch = first_batch + (unsigned)b;
            std::memset(stage, 0xEE, sizeof(stage[0]) * n_rows * cap);
            std::memset(events, 0xEE, sizeof(events[0]) * ((size_t)E + GUARD));
            count = (int)0xEEEEEEEE;
            if (pack == 2) { // the pack kernel alone: the rows' counts and staged events come from the file
                for (int r = 0; r < n_rows; r++) rows[set][r].n_events = in.i32();
                for (int r = 0; r < n_rows; r++) {
                    int n = rows[set][r].n_events;
                    n = n < 0 ? 0 : n > cap ? cap : n;
                    in.take(stage + (size_t)r * cap, sizeof(stage[0]) * (size_t)n);
                }
                hipLaunchKernelGGL(band_watch_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, nullptr, a);
            } else {
                for (int r = 0; r < n_rows; r++) dev[(size_t)dev_of_row[r]].disabled = in.i32();
                std::memset(summary, 0, sizeof(summary[0]) * n_rows);
                for (int r = 0; r < n_rows; r++) summary[r].n_peaks = in.i32();
                in.take(peaks, sizeof(peaks[0]) * (size_t)n_rows * max_peaks);
                if (two_sets) { // every entry of the set written to must be written
                    std::memset(tracks[set], 0xEE, sizeof(tracks[set][0]) * n_rows * T);
                    std::memset(rows[set], 0xEE, sizeof(rows[set][0]) * n_rows);
                }
                if (pack) launch_band_watch(a, nullptr);
                else hipLaunchKernelGGL(band_watch_kernel, dim3((unsigned)((n_rows + WATCH_ROWS - 1) / WATCH_ROWS)), dim3(WATCH_THREADS), 0, nullptr, a);
            }
            std::fwrite(tracks[set], sizeof(tracks[set][0]), (size_t)n_rows * T, out);
            std::fwrite(rows[set], sizeof(rows[set][0]), n_rows, out);
            if (pack) {
                std::fwrite(&count, 4, 1, out);
                const int kept = count < 0 ? 0 : count < E ? count : E;
                std::fwrite(events, sizeof(events[0]), kept, out);
                if (!untouched(events, sizeof(events[0]) * (size_t)kept, sizeof(events[0]) * ((size_t)E + GUARD), 0xEE)) {
                    std::fprintf(stderr, "host_watch: case %d batch %d wrote behind the %d events it kept\n", c, b, kept);
                    return 1;
                }
            } else {
                for (int r = 0; r < n_rows; r++) {
                    int n = rows[set][r].n_events;
                    n = n < 0 ? 0 : n > cap ? cap : n;
                    std::fwrite(stage + (size_t)r * cap, sizeof(stage[0]), n, out);
                }
            }
        }
        for (int q = 0; q < 2; q++) {
            std::free(tracks[q]);
            std::free(rows[q]);
        }
        std::free(stage);
        std::free(events);
        std::free(summary);
        std::free(peaks);
    }
    std::fclose(out);
    return 0;
}
