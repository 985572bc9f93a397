// tests/host_follow_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_band_follow.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the band follow's source itself -- csrc/band_follow.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its two kernels with their
// wavefront semantics on the CPU (lanes as fibers; shuffles, ballots and barriers as rendezvous points), launched by the file's own launch_band_follow().
// A stand-alone program: `host_follow <cases file> <results file>`.  The cases file holds sequences of batches (the rows' followers, then per batch which rows
// are switched off and the rows' track tables as a watch would have left them); the results file gets, per batch, what the kernels left.  The test compares
// those bytes with capi.band_follow_reference().  The staging area and the list are poisoned before every batch, the list carries a guard zone behind
// max_changes that must come back untouched, and the followers' demod slots are spread over a ChanState array whose other entries must keep their poison.
// Having its own main, the same file is what runs under a host sanitizer.
//
// Cases file (little-endian int32): n_cases, then per case
//     n_rows fft_log max_tracks max_changes n_batches first_batch n_follow  dev_of_row[n_rows]  fol_range[n_rows][2]  home[n_follow]  channel[n_follow]
//     per batch:  disabled[n_rows]  tracks[n_rows][max_tracks] (24 bytes each)
// Results file, per batch: followers [n_follow] (16 bytes), rows [n_rows] (16 bytes), int32 bin[n_follow] (ChanState::bin of the followers' slots), int32 the
//     re-tune stamp, int32 n_changes, then min(n_changes, max_changes) records of 16 bytes.  The stamp of batch b is b + 1.
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/band_follow.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD = 64;        // changes behind max_changes that nothing may write
constexpr int POISON_BIN = -77;  // ChanState::bin of a slot that is no follower's

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_follow", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int n_rows = in.i32(), fft_log = in.i32(), T = in.i32(), E = in.i32(), n_batches = in.i32();
        const unsigned first_batch = (unsigned)in.i32();
        const int n_follow = in.i32();
        if (n_rows < 1 || T < 1 || T > 64 || E < 1 || n_follow < 1) return 2;
        std::vector<int> dev_of_row((size_t)n_rows), range((size_t)n_rows * 2), home((size_t)n_follow), channel((size_t)n_follow), slot((size_t)n_follow);
        in.take(dev_of_row.data(), 4 * (size_t)n_rows);
        in.take(range.data(), 8 * (size_t)n_rows);
        in.take(home.data(), 4 * (size_t)n_follow);
        in.take(channel.data(), 4 * (size_t)n_follow);
        int n_dev = 0, most = 0;
        for (int d : dev_of_row) n_dev = d + 1 > n_dev ? d + 1 : n_dev;
        for (int r = 0; r < n_rows; r++) most = range[(size_t)r * 2 + 1] > most ? range[(size_t)r * 2 + 1] : most;
        const int cap = most + T, n_slots = 3 * n_follow + 2;
        std::vector<DevConst> dev((size_t)n_dev);
        std::memset(dev.data(), 0, sizeof(DevConst) * dev.size());
        std::vector<ChanState> cs((size_t)n_slots);
        std::memset(cs.data(), 0, sizeof(ChanState) * cs.size());
        for (ChanState& s : cs) s.bin = POISON_BIN;
        airband_hip_band_follower* followers = aligned<airband_hip_band_follower>(n_follow);
        std::memset(followers, 0, sizeof(followers[0]) * n_follow);
        for (int i = 0; i < n_follow; i++) {
            slot[(size_t)i] = 3 * i + 1;
            cs[(size_t)slot[(size_t)i]].bin = home[(size_t)i];
            followers[i].channel = channel[(size_t)i];
            followers[i].bin = home[(size_t)i];
            followers[i].track = -1;
        }
        airband_hip_band_track* tracks = aligned<airband_hip_band_track>((size_t)n_rows * T);
        airband_hip_band_follow_row* rows = aligned<airband_hip_band_follow_row>(n_rows);
        std::memset(rows, 0, sizeof(rows[0]) * n_rows);
        airband_hip_band_follow_change* stage = aligned<airband_hip_band_follow_change>((size_t)n_rows * cap);
        airband_hip_band_follow_change* changes = aligned<airband_hip_band_follow_change>((size_t)E + GUARD);
        int count = 0, stamp = 0;
        FollowArgs a;
        std::memset(&a, 0, sizeof(a));
        a.dev = dev.data();
        a.dev_of_row = dev_of_row.data();
        a.tracks = tracks;
        a.fol_range = range.data();
        a.fol_slot = slot.data();
        a.fol_home = home.data();
        a.followers = followers;
        a.rows = rows;
        a.stage = stage;
        a.changes = changes;
        a.n_changes = &count;
        a.cs = cs.data();
        a.moved_epoch = &stamp;
        a.n_rows = n_rows;
        a.n_follow = n_follow;
        a.n_slots = n_slots;
        a.fft_log = fft_log;
        a.max_tracks = T;
        a.cap = cap;
        a.max_changes = E;
        for (int b = 0; b < n_batches; b++) {
            for (int r = 0; r < n_rows; r++) dev[(size_t)dev_of_row[r]].disabled = in.i32();
            in.take(tracks, sizeof(tracks[0]) * (size_t)n_rows * T);
            a.batch = first_batch + (unsigned)b;
            a.epoch = b + 1;
            std::memset(stage, 0xEE, sizeof(stage[0]) * n_rows * cap);
            std::memset(changes, 0xEE, sizeof(changes[0]) * ((size_t)E + GUARD));
            count = (int)0xEEEEEEEE;
            launch_band_follow(a, nullptr);
            std::fwrite(followers, sizeof(followers[0]), n_follow, out);
            std::fwrite(rows, sizeof(rows[0]), n_rows, out);
            for (int i = 0; i < n_follow; i++) std::fwrite(&cs[(size_t)slot[(size_t)i]].bin, 4, 1, out);
            std::fwrite(&stamp, 4, 1, out);
            std::fwrite(&count, 4, 1, out);
            const int kept = count < 0 ? 0 : count < E ? count : E;
            std::fwrite(changes, sizeof(changes[0]), kept, out);
            if (!untouched(changes, sizeof(changes[0]) * (size_t)kept, sizeof(changes[0]) * ((size_t)E + GUARD), 0xEE)) {
                std::fprintf(stderr, "host_follow: case %d batch %d wrote behind the %d changes it kept\n", c, b, kept);
                return 1;
            }
            for (int s = 0; s < n_slots; s++)
                if (s % 3 != 1 && cs[(size_t)s].bin != POISON_BIN) {
                    std::fprintf(stderr, "host_follow: case %d batch %d wrote the bin of slot %d, which is no follower's\n", c, b, s);
                    return 1;
                }
        }
        std::free(followers);
        std::free(tracks);
        std::free(rows);
        std::free(stage);
        std::free(changes);
    }
    std::fclose(out);
    return 0;
}
