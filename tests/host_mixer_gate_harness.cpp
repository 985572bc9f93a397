// tests/host_mixer_gate_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_mixer_gate.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the mixer gate's source itself -- csrc/mixer_gate.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernels with their wavefront
// semantics on the CPU (lanes as fibers; ballots, shuffles and barriers as rendezvous points), launched by the file's own launch_mixer_gate_list() and
// launch_mixer_pack().  A stand-alone program: `host_mixer_gate <cases file> <results file>`.  The test compares the results with capi.mixer_gate_reference()
// byte for byte.  The list, the packed rows and the records are poisoned and carry a guard zone behind max_rows: every byte behind what a step was to write must
// come back untouched.  Having its own main, the same file is what runs under a host sanitizer.
//
// Cases file (little-endian): int32 n_cases, then per case
//     int32 encoding width wave_batch n_mixers max_rows grid n_steps listed;  uint8 gate[n_mixers];  uint8 stereo[n_mixers];
//     listed != 0: int32 count, int32 index[max_rows] (a list given instead of built: its tail may hold mixers out of range the kernel must never follow);
//     then per step: uint8 has_signal[n_mixers], float32 left[n_mixers][wave_batch], float32 right[n_mixers][wave_batch]
//   listed == 0: every step runs select, index and pack; `prev` is carried from step to step.
//   listed != 0: every step runs the pack alone on the given list and count.
// Results file, per case and step: int32 count, int32 kept = min(max(count, 0), max_rows), int32 index[kept], the kept rows (width * wave_batch samples of 4, 2 or 1
// bytes each), and for an encoding other than float32 the kept records (16 bytes each).
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/mixer_gate.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD_ROWS = 3; // rows / list entries behind max_rows that nothing may write

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_mixer_gate", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int encoding = in.i32(), W = in.i32(), B = in.i32(), n_mix = in.i32(), max_rows = in.i32(), grid = in.i32(), n_steps = in.i32(), listed = in.i32();
        if (B < 4 || B % 4 || n_mix < 1 || max_rows < 1 || grid < 1 || encoding < 0 || encoding > 3 || (W != 1 && W != 2) || n_steps < 1) return 2;
        std::vector<uint8_t> gate((size_t)n_mix), stereo((size_t)n_mix), prev((size_t)n_mix, 0), signal((size_t)n_mix);
        in.take(gate.data(), (size_t)n_mix);
        in.take(stereo.data(), (size_t)n_mix);
        const size_t total_rows = (size_t)max_rows + GUARD_ROWS;
        std::vector<int> index(total_rows, (int)0xEEEEEEEE), given;
        int given_count = 0;
        if (listed) {
            given_count = in.i32();
            given.resize((size_t)max_rows);
            in.take(given.data(), 4 * (size_t)max_rows);
        }
        const int nb = (n_mix + GATE_BLOCK - 1) / GATE_BLOCK;
        std::vector<unsigned long long> mask(((size_t)n_mix + 63) / 64 + 1, 0xEEEEEEEEEEEEEEEEull);
        std::vector<int> block_count((size_t)nb + 1, (int)0xEEEEEEEE);
        const size_t sample_bytes = encoding == AIRBAND_AUDIO_F32 ? 4 : (encoding == AIRBAND_AUDIO_S16 ? 2 : 1), row_bytes = (size_t)W * B * sample_bytes;
        float* left = aligned<float>((size_t)n_mix * B);
        float* right = aligned<float>((size_t)n_mix * B);
        unsigned char* rows = aligned<unsigned char>(total_rows * row_bytes);
        airband_hip_audio_row* info = aligned<airband_hip_audio_row>(total_rows);
        for (int k = 0; k < n_steps; k++) {
            in.take(signal.data(), (size_t)n_mix);
            in.take(left, 4 * (size_t)n_mix * B);
            in.take(right, 4 * (size_t)n_mix * B);
            std::memset(rows, 0xEE, total_rows * row_bytes);
            std::memset(info, 0xEE, total_rows * sizeof(info[0]));
            int count_mem = 0;
            if (listed) {
                count_mem = given_count;
                std::memcpy(index.data(), given.data(), 4 * (size_t)max_rows);
            } else {
                std::fill(index.begin(), index.end(), (int)0xEEEEEEEE);
                MixerGateArgs g;
                g.gate = gate.data();
                g.has_signal = signal.data();
                g.prev = prev.data();
                g.mask = mask.data();
                g.block_count = block_count.data();
                g.index = index.data();
                g.count = &count_mem;
                g.n_mixers = n_mix;
                g.max_rows = max_rows;
                launch_mixer_gate_list(g, nullptr);
                if (mask.back() != 0xEEEEEEEEEEEEEEEEull || block_count.back() != (int)0xEEEEEEEE) {
                    std::fprintf(stderr, "host_mixer_gate: case %d step %d wrote behind the ballots or the workgroup counts\n", c, k);
                    return 1;
                }
            }
            MixerPackArgs a;
            std::memset(&a, 0, sizeof(a));
            a.index = index.data();
            a.count = &count_mem;
            a.n_rows = 0;
            a.max_rows = max_rows;
            a.n_mixers = n_mix;
            a.left = left;
            a.right = right;
            a.stereo = stereo.data();
            a.reserved_all = 0;
            a.out = rows;
            a.info = info;
            a.wave_batch = B;
            a.encoding = encoding;
            a.width = W;
            launch_mixer_pack(a, grid, nullptr);
            const int kept = count_mem < 0 ? 0 : (count_mem < max_rows ? count_mem : max_rows);
            std::fwrite(&count_mem, 4, 1, out);
            std::fwrite(&kept, 4, 1, out);
            std::fwrite(index.data(), 4, (size_t)kept, out);
            std::fwrite(rows, row_bytes, (size_t)kept, out);
            if (encoding != AIRBAND_AUDIO_F32) std::fwrite(info, sizeof(info[0]), (size_t)kept, out);
            if (!listed && !untouched(index.data(), 4 * (size_t)kept, 4 * total_rows, 0xEE)) {
                std::fprintf(stderr, "host_mixer_gate: case %d step %d wrote the list behind the %d entries it kept\n", c, k, kept);
                return 1;
            }
            if (!untouched(rows, (size_t)kept * row_bytes, total_rows * row_bytes, 0xEE)) {
                std::fprintf(stderr, "host_mixer_gate: case %d step %d wrote a row behind the %d rows it kept\n", c, k, kept);
                return 1;
            }
            const size_t info_from = encoding == AIRBAND_AUDIO_F32 ? 0 : (size_t)kept * sizeof(info[0]);
            if (!untouched(info, info_from, total_rows * sizeof(info[0]), 0xEE)) {
                std::fprintf(stderr, "host_mixer_gate: case %d step %d wrote a record it was not to write (%d rows kept)\n", c, k, kept);
                return 1;
            }
        }
        std::free(left);
        std::free(right);
        std::free(rows);
        std::free(info);
    }
    std::fclose(out);
    return 0;
}
