// tests/host_spool_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_transmission_spool.py and tests/test_host_mixer_spool.py through tests/hostbed.py
// into a temporary directory; never part of, linked into or loaded by the library).
// Compiles the transmission spool's source itself -- csrc/tx_spool.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernels with their
// wavefront semantics on the CPU (lanes as fibers; ballots, shuffles and barriers as rendezvous points), launched by the file's own launch_spool_step(),
// launch_spool_flush() and launch_spool_collect(), with a SpoolArgs filled the way the driver fills it.  What the passes in front leave for a step -- the verdict
// mask, the per-workgroup counts, the encoded rows and their records -- is made here in plain C++, in one of two modes:
//     0, a CHANNEL spool: from the step's selection bytes, as the gate and the encoder leave it; rows of any multiple of four bytes.
//     1, a MIXER spool: n_ch = the mixer count, wave_batch = B frames, rows of W * B samples (1 000 .. 8 000 bytes), records with their stereo flags; the
//        selection is derived from the script's gate bytes and the step's has_signal flags by the mixer gate's rule (active = ALWAYS, or SIGNAL and (signal or
//        prev); prev = signal), and a listed record must name the mixer it is listed for.
// A stand-alone program: `host_spool <script file> <results file>`.  The tests compare the results with capi.transmission_spool_reference() byte for byte.
// Having its own main, the same file is what runs under a host sanitizer: every buffer is exactly as large as the handle would make it.
//
// Script file (little-endian): int32 mode n_ch max_rows row_bytes wave_batch pool_rows export_rows max_records min_batches idle_batches max_batches;
// mode 1: uint8 gate[n_ch]; uint8 spool[n_ch]; then operations until the file ends: int32 op --
//     0 step:    uint8 selected[n_ch] (mode 1: has_signal[n_ch]); the listed rows (the first max_rows selected, ascending): row_bytes bytes and a 16-byte record each
//     1 flush
//     2 collect
// Results file: per collect int32 n, n_rows, n_waiting, n records of 48 bytes, n_rows rows; at the end the eight uint64 counters.
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/tx_spool.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

namespace {

constexpr int BLOCK = 1024; // the workgroup of the per-channel passes in front: gate.hip's and the mixer gate's (gate_passes.h: GATE_BLOCK)
constexpr uint8_t GATE_SIGNAL = 1, GATE_ALWAYS = 2;

}  // namespace

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_spool", in, out);
    const int mixers = in.i32(), n_ch = in.i32(), max_rows = in.i32(), row_bytes = in.i32(), wave_batch = in.i32(), pool_rows = in.i32(), export_rows = in.i32(),
              max_records = in.i32(), min_batches = in.i32(), idle_batches = in.i32(), max_batches = in.i32();
    if ((mixers != 0 && mixers != 1) || n_ch < 1 || max_rows < 1 || max_rows > n_ch || wave_batch < 1 || pool_rows < 1 || max_records < 1 || max_batches < 1 ||
        export_rows < max_batches + 1)
        return 2;
    // a channel row is wave_batch samples of 1 or 2 bytes; a mixer row is W * B samples of 1 or 2 bytes, B = 1 000 or 2 000, W = 1 or 2
    if (mixers ? (row_bytes < 1000 || row_bytes > 8000 || row_bytes % wave_batch) : (row_bytes < 4 || row_bytes % 4)) return 2;
    const size_t nm = ((size_t)n_ch + 63) / 64, nb = ((size_t)n_ch + BLOCK - 1) / BLOCK;
    std::vector<uint8_t> gate((size_t)n_ch), prev((size_t)n_ch, 0), sel((size_t)n_ch);
    if (mixers) in.take(gate.data(), (size_t)n_ch);
    uint8_t* spool = make<uint8_t>((size_t)n_ch, 0);
    in.take(spool, (size_t)n_ch);
    SpoolArgs a;
    std::memset(&a, 0, sizeof(a));
    a.spool = spool;
    a.chan = make<SpoolChan>((size_t)n_ch, 0);
    a.ctl = make<SpoolCtl>(1, 0);
    a.ctl->free_top = pool_rows;
    a.ctl->room = max_records;
    a.close_mask = make<unsigned long long>(nm, 0);
    a.app_mask = make<unsigned long long>(nm, 0);
    a.close_count = make<int>(nb, 0);
    a.app_count = make<int>(nb, 0);
    unsigned long long* gate_mask = make<unsigned long long>(nm, 0); // GateArgs / MixerGateArgs::mask
    int* gate_count = make<int>(nb, 0);                              // ... ::block_count
    a.gate_mask = gate_mask;
    a.gate_count = gate_count;
    a.free_stack = make<int>((size_t)pool_rows, 0);
    for (int i = 0; i < pool_rows; i++) a.free_stack[i] = i;
    a.next = make<int>((size_t)pool_rows, 0x7B); // links nobody set are far out of range
    a.pool = make<uint8_t>((size_t)pool_rows * row_bytes, 0xEE);
    a.copy_list = make<int>(2 * (size_t)max_rows, 0x7B);
    uint8_t* enc_audio = make<uint8_t>((size_t)max_rows * row_bytes, 0xEE);                 // AudioPackArgs::audio / MixerPackArgs::out
    airband_hip_audio_row* enc_info = make<airband_hip_audio_row>((size_t)max_rows, 0xEE); // ... ::info
    a.enc_audio = enc_audio;
    a.enc_info = enc_info;
    a.fin = make<airband_hip_transmission>((size_t)max_records, 0xEE);
    a.exp_records = make<airband_hip_transmission>((size_t)max_records, 0xEE);
    a.exp_head = make<int>((size_t)max_records, 0x7B);
    a.exp_src = make<int>((size_t)export_rows, 0x7B);
    a.exp_audio = make<uint8_t>((size_t)export_rows * row_bytes, 0xEE);
    a.n_ch = n_ch;
    a.max_rows = max_rows;
    a.pool_rows = pool_rows;
    a.export_rows = export_rows;
    a.max_records = max_records;
    a.row_bytes = row_bytes;
    a.wave_batch = wave_batch;
    a.min_batches = (uint32_t)min_batches;
    a.idle_batches = (uint32_t)idle_batches;
    a.max_batches = (uint32_t)max_batches;
    uint32_t steps = 0;
    while (!in.done()) {
        const int op = in.i32();
        a.k = steps;
        if (op == 0) {
            in.take(sel.data(), (size_t)n_ch);
            if (mixers) // has_signal came; the selection is the mixer gate's rule on it
                for (int m = 0; m < n_ch; m++) {
                    const bool signal = sel[m] != 0;
                    sel[m] = gate[m] == GATE_ALWAYS || (gate[m] == GATE_SIGNAL && (signal || prev[m]));
                    prev[m] = signal;
                }
            // what the select / index passes and the encoder or the pack leave: verdicts, counts per workgroup, the first max_rows rows and records
            std::memset(gate_mask, 0, nm * 8);
            std::memset(gate_count, 0, nb * 4);
            std::memset(enc_audio, 0xEE, (size_t)max_rows * row_bytes);
            std::memset(enc_info, 0xEE, (size_t)max_rows * sizeof(enc_info[0]));
            int listed = 0;
            for (int c = 0; c < n_ch; c++) {
                if (!sel[c]) continue;
                gate_mask[c >> 6] |= 1ull << (c & 63);
                gate_count[c / BLOCK]++;
                if (listed == max_rows) continue;
                in.take(enc_audio + (size_t)listed * row_bytes, (size_t)row_bytes);
                in.take(enc_info + listed, sizeof(enc_info[0]));
                if (mixers && enc_info[listed].channel != c) {
                    std::fprintf(stderr, "host_spool: step %u lists mixer %d, the script's record says %d\n", steps, c, enc_info[listed].channel);
                    return 1;
                }
                listed++;
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
                std::fprintf(stderr, "host_spool: collect counts out of range: %d %d %d\n", e[0], e[1], e[2]);
                return 1;
            }
            std::fwrite(e, 4, 3, out);
            std::fwrite(a.exp_records, sizeof(a.exp_records[0]), (size_t)e[0], out);
            std::fwrite(a.exp_audio, (size_t)row_bytes, (size_t)e[1], out);
            if (!untouched(a.exp_audio, (size_t)e[1] * row_bytes, (size_t)export_rows * row_bytes, 0xEE)) {
                std::fprintf(stderr, "host_spool: the gather wrote export bytes behind the %d rows it exported\n", e[1]);
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
