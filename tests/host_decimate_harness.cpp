// tests/host_decimate_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_audio_decimate.py with the host clang++ into a temporary directory; never part
// of, linked into or loaded by the library).
// Compiles the output decimation's source itself -- csrc/audio_decimate.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernels with their
// wavefront semantics on the CPU (lanes as fibers; shuffles and the wavefront's LDS exchanges as rendezvous points), launched by the file's own
// launch_audio_decimate() with the dynamic LDS audio_decimate_lds_bytes() asks for (the shim checks that nothing is written behind it).
// A stand-alone program: `host_decimate <cases file> <results file>`.  The test compares the results with capi.audio_decimate_reference() byte for byte.  Every
// buffer the kernel writes is poisoned and carries a guard zone: the bytes behind the rows, records, histories and stamps it was to write must come back untouched.
// Having its own main, the same file is what runs under a host sanitizer.
//
// Cases file (little-endian): int32 n_cases, then per case
//     int32 encoding wave_batch n_ch max_rows grid mode n_steps
//     mode 1: int16 history[n_ch][46]
//     per step: int32 count;  mode 2: int32 index[max_rows];  float32 rows[n_ch][wave_batch]
//   mode 0: airband_hip_decimate_audio() without a history -- row r is source row r, count rows, dense, no history, no stamps;
//   mode 1: the same with a history, read and written back;
//   mode 2: the gate's form -- row r is channel index[r], the count is read from memory, the source rows are pitched and padded like the handle's, histories and
//           stamps start zeroed and step s runs with k = s + 1.
// Results file, per case: per step int32 kept = min(max(count, 0), max_rows), the kept rows' audio (wave_batch / 2 * 2 or * 1 bytes each), the kept records (16
// bytes each); behind the last step, mode 1 and 2: int16 history[n_ch][46]; mode 2: uint32 stamp[n_ch].
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/audio_decimate.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD_ROWS = 3;   // rows (and channels) behind the last one that nothing may write
constexpr int PAD = 28;         // floats in front of a pitched source row (AB_OUT_PAD)
constexpr int H = AUDIO_DECIMATE_HIST;

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_decimate", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int encoding = in.i32(), B = in.i32(), n_ch = in.i32(), max_rows = in.i32(), grid = in.i32(), mode = in.i32(), n_steps = in.i32();
        if (B < 8 || B % 8 || n_ch < 1 || max_rows < 1 || grid < 1 || encoding < 1 || encoding > 3 || mode < 0 || mode > 2 || n_steps < 1) return 2;
        const bool listed = mode == 2;
        const long stride = listed ? ((long)B + PAD + 100 + 31) / 32 * 32 : B;
        const int pad = listed ? PAD : 0;
        const size_t row_bytes = (size_t)(B / 2) * (encoding == AIRBAND_AUDIO_S16 ? 2 : 1), total_rows = (size_t)max_rows + GUARD_ROWS, total_ch = (size_t)n_ch + GUARD_ROWS;
        float* src = aligned<float>((size_t)n_ch * stride);
        unsigned char* audio = make<unsigned char>(total_rows * row_bytes, 0xEE);
        airband_hip_audio_row* info = make<airband_hip_audio_row>(total_rows, 0xEE);
        int16_t* hist = make<int16_t>(total_ch * H, 0xEE);
        uint32_t* stamp = make<uint32_t>(total_ch, 0xEE);
        if (mode == 1) in.take(hist, sizeof(int16_t) * (size_t)n_ch * H);
        if (mode == 2) {
            std::memset(hist, 0, sizeof(int16_t) * (size_t)n_ch * H);
            std::memset(stamp, 0, sizeof(uint32_t) * (size_t)n_ch);
        }
        std::vector<int> index((size_t)max_rows);
        for (int s = 0; s < n_steps; s++) {
            const int count = in.i32();
            if (listed) in.take(index.data(), 4 * (size_t)max_rows);
            for (size_t i = 0; i < (size_t)n_ch * stride; i++) src[i] = 7777.0f; // what lies between the rows clips: reading it would show
            for (int r = 0; r < n_ch; r++) in.take(src + (size_t)r * stride + pad, 4 * (size_t)B);
            std::memset(audio, 0xEE, total_rows * row_bytes);
            std::memset(info, 0xEE, total_rows * sizeof(info[0]));
            int count_mem = count;
            AudioDecimateArgs a;
            std::memset(&a, 0, sizeof(a));
            a.index = listed ? index.data() : nullptr;
            a.count = listed ? &count_mem : nullptr;
            a.n_rows = listed ? 0 : count;
            a.max_rows = max_rows;
            a.n_ch = n_ch;
            a.src = src;
            a.src_stride = stride;
            a.src_pad = pad;
            a.audio = audio;
            a.info = info;
            a.hist = mode ? hist : nullptr;
            a.stamp = listed ? stamp : nullptr;
            a.k = (uint32_t)s + 1u;
            a.wave_batch = B;
            a.encoding = encoding;
            launch_audio_decimate(a, grid, nullptr);
            const int kept = count < 0 ? 0 : (count < max_rows ? count : max_rows);
            std::fwrite(&kept, 4, 1, out);
            std::fwrite(audio, row_bytes, (size_t)kept, out);
            std::fwrite(info, sizeof(info[0]), (size_t)kept, out);
            if (!untouched(audio, (size_t)kept * row_bytes, total_rows * row_bytes, 0xEE)) {
                std::fprintf(stderr, "host_decimate: case %d step %d wrote audio bytes behind the %d rows it kept\n", c, s, kept);
                return 1;
            }
            if (!untouched(info, (size_t)kept * sizeof(info[0]), total_rows * sizeof(info[0]), 0xEE)) {
                std::fprintf(stderr, "host_decimate: case %d step %d wrote a record behind the %d rows it kept\n", c, s, kept);
                return 1;
            }
        }
        if (mode) std::fwrite(hist, sizeof(int16_t) * H, (size_t)n_ch, out);
        if (listed) std::fwrite(stamp, sizeof(uint32_t), (size_t)n_ch, out);
        if (!untouched(hist, mode ? sizeof(int16_t) * (size_t)n_ch * H : 0, sizeof(int16_t) * total_ch * H, 0xEE)) {
            std::fprintf(stderr, "host_decimate: case %d wrote a history it was not given\n", c);
            return 1;
        }
        if (!untouched(stamp, listed ? sizeof(uint32_t) * (size_t)n_ch : 0, sizeof(uint32_t) * total_ch, 0xEE)) {
            std::fprintf(stderr, "host_decimate: case %d wrote a stamp it was not given\n", c);
            return 1;
        }
        std::free(src);
        std::free(audio);
        std::free(info);
        std::free(hist);
        std::free(stamp);
    }
    std::fclose(out);
    return 0;
}
