// tests/host_mixer_spool_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_mixer_spool.py with the host clang++ into a temporary directory; never part
// of, linked into or loaded by the library).
// The mixer spool's device code on the CPU: csrc/tx_spool.hip compiled through tests/hostshim_wave64/hip/hip_runtime.h (lanes as fibers; ballots, shuffles and
// barriers as rendezvous points) and launched by the file's own launch_spool_step(), launch_spool_flush() and launch_spool_collect(), with a SpoolArgs filled the
// way the driver fills it for a MIXER spool: n_ch = the mixer count, the verdict mask and the per-workgroup counts as the mixer gate's passes leave them, rows of
// W * B samples (1 000 .. 8 000 bytes) and the pack's records with their stereo flags, wave_batch = B frames.  What the mixer gate leaves for a step is made here
// in plain C++ from the script's gate bytes and has_signal flags by the gate's rule (active = ALWAYS, or SIGNAL and (signal or prev); prev = signal).
// A stand-alone program: `host_mixer_spool <script file> <results file>`.  The test compares the results with capi.transmission_spool_reference() byte for byte.
// Having its own main, the same file is what runs under a host sanitizer: every buffer is exactly as large as the handle would make it.
//
// Script file (little-endian): int32 n_mixers max_rows row_bytes frames pool_rows export_rows max_records min_batches idle_batches max_batches; uint8
// gate[n_mixers]; uint8 spool[n_mixers]; then operations until the file ends: int32 op --
//     0 step:    uint8 has_signal[n_mixers]; the listed rows (the first max_rows active mixers, ascending): row_bytes bytes and a 16-byte record each
//     1 flush
//     2 collect
// Results file: per collect int32 n, n_rows, n_waiting, n records of 48 bytes, n_rows rows; at the end the eight uint64 counters.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// ---- what the shim lacks and tx_spool.hip uses: an integer shuffle, population counts, atomics (one fiber runs at a time) ----
static inline unsigned __shfl_up(unsigned v, unsigned delta) {
    ab_emu::Group& g = ab_emu::my_wave();
    const unsigned my = ab_emu::rendezvous(g, ab_emu::my_lane(), v);
    const int src = ab_emu::my_lane() - (int)delta;
    return src >= 0 && g.put[my & 1][src] ? g.slot[my & 1][src] : v;
}
static inline int __popcll(unsigned long long m) { return __builtin_popcountll(m); }
template <class T>
static inline T atomicAdd(T* p, T v) {
    const T old = *p;
    *p = old + v;
    return old;
}
static inline int atomicMax(int* p, int v) {
    const int old = *p;
    if (v > old) *p = v;
    return old;
}

#include "../rtlsdr-airband_amd/csrc/tx_spool.hip"

using namespace airband;

namespace {

struct Reader {
    std::vector<unsigned char> d;
    size_t at = 0;
    bool done() const { return at >= d.size(); }
    void take(void* out, size_t n) {
        if (at + n > d.size()) {
            std::fprintf(stderr, "host_mixer_spool: script file ends early\n");
            std::exit(2);
        }
        if (n) std::memcpy(out, d.data() + at, n);
        at += n;
    }
    int i32() {
        int v;
        take(&v, 4);
        return v;
    }
};

template <class T>
T* make(size_t n, int fill) { // exactly n elements (a sanitizer sees the first byte behind them), 64-byte aligned as hipMalloc's are: rows are moved 8 bytes at a time
    const size_t bytes = (n ? n : 1) * sizeof(T);
    void* p = std::aligned_alloc(64, (bytes + 63) / 64 * 64);
    if (!p) std::exit(3);
    std::memset(p, fill, (bytes + 63) / 64 * 64);
    return static_cast<T*>(p);
}

constexpr int BLOCK = 1024; // the mixer gate's workgroup (gate_passes.h: GATE_BLOCK)
constexpr uint8_t GATE_SIGNAL = 1, GATE_ALWAYS = 2;

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: host_mixer_spool <script> <results>\n");
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
    const int n_mix = in.i32(), max_rows = in.i32(), row_bytes = in.i32(), frames = in.i32(), pool_rows = in.i32(), export_rows = in.i32(),
              max_records = in.i32(), min_batches = in.i32(), idle_batches = in.i32(), max_batches = in.i32();
    // a mixer row is W * B samples of 1 or 2 bytes, B = 1 000 or 2 000, W = 1 or 2
    if (n_mix < 1 || max_rows < 1 || max_rows > n_mix || row_bytes < 1000 || row_bytes > 8000 || row_bytes % frames || pool_rows < 1 || max_records < 1 ||
        max_batches < 1 || export_rows < max_batches + 1)
        return 2;
    const size_t nm = ((size_t)n_mix + 63) / 64, nb = ((size_t)n_mix + BLOCK - 1) / BLOCK;
    std::vector<uint8_t> gate((size_t)n_mix), prev((size_t)n_mix, 0), sig((size_t)n_mix);
    in.take(gate.data(), (size_t)n_mix);
    uint8_t* spool = make<uint8_t>((size_t)n_mix, 0);
    in.take(spool, (size_t)n_mix);
    SpoolArgs a;
    std::memset(&a, 0, sizeof(a));
    a.spool = spool;
    a.chan = make<SpoolChan>((size_t)n_mix, 0);
    a.ctl = make<SpoolCtl>(1, 0);
    a.ctl->free_top = pool_rows;
    a.ctl->room = max_records;
    a.close_mask = make<unsigned long long>(nm, 0);
    a.app_mask = make<unsigned long long>(nm, 0);
    a.close_count = make<int>(nb, 0);
    a.app_count = make<int>(nb, 0);
    unsigned long long* gate_mask = make<unsigned long long>(nm, 0); // MixerGateArgs::mask
    int* gate_count = make<int>(nb, 0);                              // MixerGateArgs::block_count
    a.gate_mask = gate_mask;
    a.gate_count = gate_count;
    a.free_stack = make<int>((size_t)pool_rows, 0);
    for (int i = 0; i < pool_rows; i++) a.free_stack[i] = i;
    a.next = make<int>((size_t)pool_rows, 0x7B); // links nobody set are far out of range
    a.pool = make<uint8_t>((size_t)pool_rows * row_bytes, 0xEE);
    a.copy_list = make<int>(2 * (size_t)max_rows, 0x7B);
    uint8_t* pack_out = make<uint8_t>((size_t)max_rows * row_bytes, 0xEE);                // MixerPackArgs::out
    airband_hip_audio_row* pack_info = make<airband_hip_audio_row>((size_t)max_rows, 0xEE); // MixerPackArgs::info
    a.enc_audio = pack_out;
    a.enc_info = pack_info;
    a.fin = make<airband_hip_transmission>((size_t)max_records, 0xEE);
    a.exp_records = make<airband_hip_transmission>((size_t)max_records, 0xEE);
    a.exp_head = make<int>((size_t)max_records, 0x7B);
    a.exp_src = make<int>((size_t)export_rows, 0x7B);
    a.exp_audio = make<uint8_t>((size_t)export_rows * row_bytes, 0xEE);
    a.n_ch = n_mix;
    a.max_rows = max_rows;
    a.pool_rows = pool_rows;
    a.export_rows = export_rows;
    a.max_records = max_records;
    a.row_bytes = row_bytes;
    a.wave_batch = frames;
    a.min_batches = (uint32_t)min_batches;
    a.idle_batches = (uint32_t)idle_batches;
    a.max_batches = (uint32_t)max_batches;
    uint32_t steps = 0;
    while (!in.done()) {
        const int op = in.i32();
        a.k = steps;
        if (op == 0) {
            in.take(sig.data(), (size_t)n_mix);
            // what mixer_gate_select_kernel / mixer_gate_index_kernel and the pack leave: verdicts, counts per workgroup, the first max_rows rows and records
            std::memset(gate_mask, 0, nm * 8);
            std::memset(gate_count, 0, nb * 4);
            std::memset(pack_out, 0xEE, (size_t)max_rows * row_bytes);
            std::memset(pack_info, 0xEE, (size_t)max_rows * sizeof(pack_info[0]));
            int listed = 0;
            for (int m = 0; m < n_mix; m++) {
                const bool signal = sig[m] != 0;
                const bool active = gate[m] == GATE_ALWAYS || (gate[m] == GATE_SIGNAL && (signal || prev[m]));
                prev[m] = signal;
                if (!active) continue;
                gate_mask[m >> 6] |= 1ull << (m & 63);
                gate_count[m / BLOCK]++;
                if (listed < max_rows) {
                    in.take(pack_out + (size_t)listed * row_bytes, (size_t)row_bytes);
                    in.take(pack_info + listed, sizeof(pack_info[0]));
                    if (pack_info[listed].channel != m) {
                        std::fprintf(stderr, "host_mixer_spool: step %u lists mixer %d, the script's record says %d\n", steps, m, pack_info[listed].channel);
                        return 1;
                    }
                    listed++;
                }
            }
            launch_spool_step(a, nullptr);
            steps++;
        } else if (op == 1) {
            launch_spool_flush(a, nullptr);
        } else if (op == 2) {
            std::memset(a.exp_audio, 0xEE, (size_t)export_rows * row_bytes);
            launch_spool_collect(a, nullptr);
            const int* e = a.ctl->exp;
            if (e[0] < 0 || e[0] > max_records || e[1] < 0 || e[1] > export_rows) {
                std::fprintf(stderr, "host_mixer_spool: collect counts out of range: %d %d %d\n", e[0], e[1], e[2]);
                return 1;
            }
            std::fwrite(e, 4, 3, out);
            std::fwrite(a.exp_records, sizeof(a.exp_records[0]), (size_t)e[0], out);
            std::fwrite(a.exp_audio, (size_t)row_bytes, (size_t)e[1], out);
            for (size_t i = (size_t)e[1] * row_bytes; i < (size_t)export_rows * row_bytes; i++)
                if (a.exp_audio[i] != 0xEE) {
                    std::fprintf(stderr, "host_mixer_spool: the gather wrote export byte %zu, behind the %d rows it exported\n", i, e[1]);
                    return 1;
                }
        } else {
            return 2;
        }
    }
    const SpoolCtl& t = *a.ctl;
    const unsigned long long counters[8] = {steps, t.open_now, (unsigned long long)t.fin_count, (unsigned long long)t.free_top,
                                            t.finished_total, t.dropped, t.rows_stored, t.rows_lost};
    std::fwrite(counters, 8, 8, out);
    std::fclose(out);
    return 0;
}
