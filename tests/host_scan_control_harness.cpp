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

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// ---- what the shim lacks and band_pack.h uses: integer shuffles (as tests/host_follow_harness.cpp's) ----
static inline unsigned ab_emu_shfl_u32(unsigned v, int src) {
    ab_emu::Group& g = ab_emu::my_wave();
    const unsigned my = ab_emu::rendezvous(g, ab_emu::my_lane(), v);
    return (src >= 0 && src < 64 && g.put[my & 1][src]) ? g.slot[my & 1][src] : v;
}
static inline unsigned __shfl_up(unsigned v, unsigned delta) { return ab_emu_shfl_u32(v, ab_emu::my_lane() - (int)delta); }

#include "../rtlsdr-airband_amd/csrc/scan_control.hip"

using namespace airband;

namespace {

struct Reader {
    std::vector<unsigned char> d;
    size_t at = 0;
    void take(void* out, size_t n) {
        if (at + n > d.size()) {
            std::fprintf(stderr, "host_scan_control: cases file ends early\n");
            std::exit(2);
        }
        std::memcpy(out, d.data() + at, n);
        at += n;
    }
    int i32() {
        int v;
        take(&v, 4);
        return v;
    }
};

template <class T>
T* aligned(size_t n) { // 16-byte records are moved 16 bytes at a time
    void* p = std::aligned_alloc(64, ((n ? n : 1) * sizeof(T) + 63) / 64 * 64);
    if (!p) std::exit(3);
    return static_cast<T*>(p);
}

constexpr int GUARD = 64; // records behind max_records that nothing may write

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: host_scan_control <cases> <results>\n");
        return 2;
    }
    Reader in;
    {
        FILE* f = std::fopen(argv[1], "rb");
        if (!f) return 2;
        unsigned char buf[1 << 16];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) in.d.insert(in.d.end(), buf, buf + n);
        std::fclose(f);
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
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
            const unsigned char* g = reinterpret_cast<const unsigned char*>(events + kept);
            for (size_t i = 0; i < sizeof(events[0]) * ((size_t)E + GUARD - (size_t)kept); i++)
                if (g[i] != 0xEE) {
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
