// tests/host_mixer_rtp_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_mixer_rtp.py through tests/hostbed.py into a temporary directory; never part
// of, linked into or loaded by the library).
// Compiles the RTP packet stream's source itself -- csrc/rtp_stream.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernels with their
// wavefront semantics on the CPU the way the MIXER stream runs them: rows of wave_batch frames of `width` samples, RtpArgs::width_shift set from it, and the
// flush step in which the mask and the counts are NULL.  The state lives here from step to step, as it lives on the handle.  What the passes in front leave for a
// step -- the mixer gate's verdict mask, its per-workgroup counts, the pack's rows -- is made here in plain C++ from the step's selection bytes.
// A stand-alone program: `host_mixer_rtp <script file> <results file>`.  The tests compare the results with capi.rtp_stream_reference(width=...) byte for byte.
// Having its own main, the same file is what runs under a host sanitizer: every buffer is exactly as large as the handle would make it, except that the records
// and the slots have GUARD more entries, poisoned, which must come back untouched.
//
// Script file (little-endian): int32 n_mixers max_rows wave_batch sample_bytes width frame_samples max_packets grid; airband_hip_rtp_source sources[n_mixers];
// then operations until the file ends: int32 op --
//     0 step:  uint8 selected[n_mixers]; the listed rows (the first max_rows selected, ascending): wave_batch * width * sample_bytes bytes each
//     1 step with a damaged work list: the same input; between the scan and the write pass every work item's mixer, row and first slot are set far out of
//       range.  Nothing is written to the results: the step must only stay inside its buffers (the guards, and the sanitizers).  Ends the script.
//     2 flush: no input; the three launches with no mask and no counts, k = the steps so far, which does not advance.  The rows still hold the last step's.
// Results file: per step or flush int32 count, n = min(count, max_packets) records of 16 bytes, n slots of slot_bytes (bytes the step did not write are 0xEE),
// the state of every mixer (16 bytes each); at the end four uint64: packets, dropped, octets, lost_rows.
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/rtp_stream.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

namespace {
constexpr int GUARD = 4;
}

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_mixer_rtp", in, out);
    const int n = in.i32(), max_rows = in.i32(), B = in.i32(), sb = in.i32(), W = in.i32(), F = in.i32(), max_packets = in.i32(), grid = in.i32();
    if (n < 1 || max_rows < 1 || max_rows > n || B < 4 || B % 4 || (sb != 1 && sb != 2) || (W != 1 && W != 2) || F < 40 || F % 4 || F > B || 12 + F * W * sb > 1472 ||
        max_packets < 1 || grid < 1)
        return 2;
    int gcd = B, rest = F;
    while (rest) {
        const int t = gcd % rest;
        gcd = rest;
        rest = t;
    }
    const int fb = sb * W, carry_cap = F - gcd, carry_stride = carry_cap * fb, slot = (12 + F * fb + 15) / 16 * 16;
    const size_t nm = ((size_t)n + 63) / 64, nb = ((size_t)n + GATE_BLOCK - 1) / GATE_BLOCK, row_bytes = (size_t)B * fb;
    airband_hip_rtp_source* sources = make<airband_hip_rtp_source>((size_t)n, 0);
    in.take(sources, (size_t)n * sizeof(sources[0]));
    std::vector<uint8_t> sel((size_t)n);
    RtpArgs a;
    std::memset(&a, 0, sizeof(a));
    a.sources = sources;
    a.state = make<airband_hip_rtp_state>((size_t)n, 0);
    for (int c = 0; c < n; c++)
        if (sources[c].stream) a.state[c].seq = sources[c].seq0;
    a.carry = make<uint8_t>((size_t)n * carry_stride + 4, 0);
    a.ctl = make<RtpCtl>(1, 0);
    a.plan = make<RtpPlan>((size_t)n, 0x7B);
    a.blocks = make<RtpBlock>(nb, 0x7B);
    a.work = make<RtpWork>((size_t)n, 0x7B);
    unsigned long long* gate_mask = make<unsigned long long>(nm, 0);
    int* gate_count = make<int>(nb, 0);
    uint8_t* enc_audio = make<uint8_t>((size_t)max_rows * row_bytes, 0xEE);
    a.gate_mask = gate_mask;
    a.gate_count = gate_count;
    a.enc_audio = enc_audio;
    a.records = make<airband_hip_rtp_packet>((size_t)max_packets + GUARD, 0xEE);
    a.packets = make<uint8_t>(((size_t)max_packets + GUARD) * slot, 0xEE);
    a.n_ch = n;
    a.max_rows = max_rows;
    a.wave_batch = B;
    a.frame_samples = F;
    a.sample_bytes = sb;
    a.width_shift = W == 2 ? 1 : 0;
    a.carry_cap = carry_cap;
    a.carry_stride = carry_stride;
    a.slot_bytes = slot;
    a.max_packets = max_packets;
    uint32_t steps = 0;
    unsigned ops = 0;
    while (!in.done()) {
        const int op = in.i32();
        if (op < 0 || op > 2) return 2;
        a.k = steps;
        std::memset(a.records, 0xEE, ((size_t)max_packets + GUARD) * sizeof(a.records[0]));
        std::memset(a.packets, 0xEE, ((size_t)max_packets + GUARD) * slot);
        if (op == 2) {
            a.gate_mask = nullptr; /* the driver's flush: nobody is listed, neither pointer may be followed */
            a.gate_count = nullptr;
            launch_rtp_step(a, grid, nullptr);
            a.gate_mask = gate_mask;
            a.gate_count = gate_count;
        } else {
            in.take(sel.data(), (size_t)n);
            std::memset(gate_mask, 0, nm * 8);
            std::memset(gate_count, 0, nb * 4);
            std::memset(enc_audio, 0xEE, (size_t)max_rows * row_bytes);
            int listed = 0;
            for (int c = 0; c < n; c++) {
                if (!sel[c]) continue;
                gate_mask[c >> 6] |= 1ull << (c & 63);
                gate_count[c / GATE_BLOCK]++;
                if (listed == max_rows) continue;
                in.take(enc_audio + (size_t)listed * row_bytes, row_bytes);
                listed++;
            }
            if (op == 0) {
                launch_rtp_step(a, grid, nullptr);
            } else {
                hipLaunchKernelGGL(rtp_count_kernel, dim3((unsigned)nb), dim3(GATE_BLOCK), 0, nullptr, a);
                hipLaunchKernelGGL(rtp_scan_kernel, dim3((unsigned)nb), dim3(GATE_BLOCK), 0, nullptr, a);
                for (int i = 0; i < n; i++) {
                    a.work[i].channel = (i & 1) ? 0x7FFFFFF0 : -5;
                    a.work[i].row = 0x7FFFFFF0;
                    a.work[i].first = (i & 2) ? -7 : 0x7FFFFFF0;
                }
                a.ctl->n_work = 0x7FFFFFF0;
                for (int c = 0; c < n; c++) a.state[c].carry = 0xFFFF;
                hipLaunchKernelGGL(rtp_write_kernel, dim3((unsigned)grid), dim3(64), 0, nullptr, a);
            }
            steps++;
        }
        ops++;
        const size_t np = (size_t)max_packets;
        if (!untouched(a.records, np * sizeof(a.records[0]), (np + GUARD) * sizeof(a.records[0]), 0xEE) || !untouched(a.packets, np * slot, (np + GUARD) * slot, 0xEE)) {
            std::fprintf(stderr, "host_mixer_rtp: operation %u wrote behind the %d records or slots the buffers hold\n", ops - 1, max_packets);
            return 1;
        }
        if (op == 1) break;
        const int count = a.ctl->n_packets;
        if (count < 0) {
            std::fprintf(stderr, "host_mixer_rtp: operation %u counts %d packets\n", ops - 1, count);
            return 1;
        }
        const size_t kept = (size_t)(count < max_packets ? count : max_packets);
        std::fwrite(&count, 4, 1, out);
        std::fwrite(a.records, sizeof(a.records[0]), kept, out);
        std::fwrite(a.packets, (size_t)slot, kept, out);
        std::fwrite(a.state, sizeof(a.state[0]), (size_t)n, out);
        if (!untouched(a.records, kept * sizeof(a.records[0]), np * sizeof(a.records[0]), 0xEE) || !untouched(a.packets, kept * slot, np * slot, 0xEE)) {
            std::fprintf(stderr, "host_mixer_rtp: operation %u wrote records or slots behind the %zu it counts\n", ops - 1, kept);
            return 1;
        }
    }
    const RtpCtl& t = *a.ctl;
    const unsigned long long counters[4] = {t.packets, t.dropped, t.octets, t.lost_rows};
    std::fwrite(counters, 8, 4, out);
    std::fclose(out);
    std::free(gate_mask); /* a script that ends with a flush leaves no launch behind that still names these two */
    std::free(gate_count);
    return 0;
}
