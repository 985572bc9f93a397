// tests/host_scan_control_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_scan_control.py with the host clang++ into a temporary directory; never part
// of, linked into or loaded by the library).
// Compiles scan control's source itself -- csrc/scan_control.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its two kernels with their wavefront
// semantics on the CPU (lanes as fibers; shuffles and barriers as rendezvous points), launched by the file's own launch_scan_control().
// A stand-alone program: `host_scan_control <cases file> <results file>`.  The cases file holds sequences of batches (the lists, their start states, then per batch
// which dongles are switched off, every channel's axcindicate and the holds set before the batch); the results file gets, per batch, what the kernels left.  The
// test compares those bytes with capi.scan_control_reference().  The staging area, the counts, the switch list and the record list are poisoned before every
// batch, and the record list carries a guard zone behind max_records that must come back untouched.  Having its own main, the same file is what runs under a
// host sanitizer.
//
// Cases file (little-endian int32 unless said): n_cases, then per case
//     n_lists n_dev n_ch idle_batches dwell_batches max_records n_batches first_batch   lists[n_lists][5] (dev ext slot first_entry n)   state[n_lists] (16 bytes each)
//     per batch:  disabled[n_dev]   axc[n_ch] bytes, padded to a multiple of four   hold[n_lists] (-2: leave the list's hold as it is)
// Results file, per batch: state [n_lists] (16 bytes), int32 sw[n_lists][3], int32 n_records, then min(n_records, max_records) records of 16 bytes.
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/scan_control.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD = 64; // records behind max_records that nothing may write

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_scan_control", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int n_lists = in.i32(), n_dev = in.i32(), n_ch = in.i32(), idle = in.i32(), dwell = in.i32(), E = in.i32(), n_batches = in.i32();
        const unsigned first_batch = (unsigned)in.i32();
        if (n_lists < 1 || n_dev < 1 || n_ch < 1 || idle < 1 || dwell < 1 || E < 1) return 2;
        std::vector<ScanCtlList> lists((size_t)n_lists);
        std::memset(lists.data(), 0, sizeof(ScanCtlList) * lists.size());
        for (ScanCtlList& l : lists) {
            l.dev = in.i32();
            l.ext = in.i32();
            l.slot = in.i32();
            l.first_entry = in.i32();
            l.n = in.i32();
        }
        airband_hip_scan_state* state = aligned<airband_hip_scan_state>(n_lists);
        in.take(state, sizeof(state[0]) * (size_t)n_lists);
        std::vector<DevConst> dev((size_t)n_dev);
        std::memset(dev.data(), 0, sizeof(DevConst) * dev.size());
        const size_t axc_bytes = ((size_t)n_ch + 3) / 4 * 4;
        std::vector<uint8_t> axc(axc_bytes);
        airband_hip_scan_event* stage = aligned<airband_hip_scan_event>(n_lists);
        airband_hip_scan_event* events = aligned<airband_hip_scan_event>((size_t)E + GUARD);
        std::vector<int> stage_n((size_t)n_lists), sw((size_t)n_lists * 3);
        int count = 0;
        ScanControlArgs a;
        std::memset(&a, 0, sizeof(a));
        a.dev = dev.data();
        a.axc = axc.data();
        a.lists = lists.data();
        a.state = state;
        a.stage = stage;
        a.stage_n = stage_n.data();
        a.sw = sw.data();
        a.events = events;
        a.n_events = &count;
        a.n_lists = n_lists;
        a.n_dev = n_dev;
        a.n_ch = n_ch;
        a.idle_batches = idle;
        a.dwell_batches = dwell;
        a.max_records = E;
        for (int b = 0; b < n_batches; b++) {
            for (int d = 0; d < n_dev; d++) dev[(size_t)d].disabled = in.i32();
            in.take(axc.data(), axc_bytes);
            for (int i = 0; i < n_lists; i++) {
                const int hold = in.i32();
                if (hold != -2) state[i].hold = (int16_t)hold;
            }
            a.batch = first_batch + (unsigned)b;
            std::memset(stage, 0xEE, sizeof(stage[0]) * (size_t)n_lists);
            std::memset(events, 0xEE, sizeof(events[0]) * ((size_t)E + GUARD));
            std::memset(stage_n.data(), 0xEE, sizeof(int) * stage_n.size());
            std::memset(sw.data(), 0xEE, sizeof(int) * sw.size());
            count = (int)0xEEEEEEEE;
            launch_scan_control(a, nullptr);
            std::fwrite(state, sizeof(state[0]), (size_t)n_lists, out);
            std::fwrite(sw.data(), sizeof(int), sw.size(), out);
            std::fwrite(&count, 4, 1, out);
            const int kept = count < 0 ? 0 : count < E ? count : E;
            std::fwrite(events, sizeof(events[0]), (size_t)kept, out);
            if (!untouched(events, sizeof(events[0]) * (size_t)kept, sizeof(events[0]) * ((size_t)E + GUARD), 0xEE)) {
                std::fprintf(stderr, "host_scan_control: case %d batch %d wrote behind the %d records it kept\n", c, b, kept);
                return 1;
            }
        }
        std::free(state);
        std::free(stage);
        std::free(events);
    }
    std::fclose(out);
    return 0;
}
