// tests/host_audio_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_audio_pack.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the encoder's source itself -- csrc/audio_pack.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernels with their wavefront
// semantics on the CPU (lanes as fibers; shuffles as rendezvous points), launched by the file's own launch_audio_pack().
// A stand-alone program: `host_audio <cases file> <results file>`.  The test compares the results with capi.audio_encode_reference() byte for byte.  The audio
// buffer and the records are poisoned and carry a guard zone behind max_rows: every byte behind the rows the kernel was to write must come back untouched.
// Having its own main, the same file is what runs under a host sanitizer.
//
// Cases file (little-endian): int32 n_cases, then per case
//     int32 encoding wave_batch n_ch max_rows count grid listed;  listed != 0: int32 index[max_rows];  float32 rows[n_ch][wave_batch]
//   listed != 0: the gate's form -- row r is channel index[r], the count is read from memory, the source rows are pitched and padded like the handle's;
//   listed == 0: airband_hip_encode_audio()'s form -- row r is source row r, count rows, dense.
// Results file, per case: int32 kept = min(max(count, 0), max_rows), the kept rows' audio (wave_batch * 2 or * 1 bytes each), the kept records (16 bytes each).
#include <hip/hip_runtime.h>

#include "../rtlsdr-airband_amd/csrc/audio_pack.hip"
#include "host_program.h"

using namespace airband;
using namespace host_program;

constexpr int GUARD_ROWS = 3;   // rows behind max_rows that nothing may write
constexpr int PAD = 28;         // floats in front of a pitched source row (AB_OUT_PAD)

int main(int argc, char** argv) {
    Reader in;
    FILE* out;
    open_io(argc, argv, "host_audio", in, out);
    const int n_cases = in.i32();
    for (int c = 0; c < n_cases; c++) {
        const int encoding = in.i32(), B = in.i32(), n_ch = in.i32(), max_rows = in.i32(), count = in.i32(), grid = in.i32(), listed = in.i32();
        if (B < 4 || B % 4 || n_ch < 1 || max_rows < 1 || grid < 1 || encoding < 1 || encoding > 3) return 2;
        std::vector<int> index((size_t)max_rows);
        if (listed) in.take(index.data(), 4 * (size_t)max_rows);
        const long stride = listed ? ((long)B + PAD + 100 + 31) / 32 * 32 : B;
        const int pad = listed ? PAD : 0;
        float* src = aligned<float>((size_t)n_ch * stride);
        for (size_t i = 0; i < (size_t)n_ch * stride; i++) src[i] = 7777.0f; // what lies between the rows clips: reading it would show
        for (int r = 0; r < n_ch; r++) in.take(src + (size_t)r * stride + pad, 4 * (size_t)B);
        const size_t row_bytes = (size_t)B * (encoding == AIRBAND_AUDIO_S16 ? 2 : 1), total_rows = (size_t)max_rows + GUARD_ROWS;
        unsigned char* audio = make<unsigned char>(total_rows * row_bytes, 0xEE);
        airband_hip_audio_row* info = make<airband_hip_audio_row>(total_rows, 0xEE);
        int count_mem = count;
        AudioPackArgs a;
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
        a.wave_batch = B;
        a.encoding = encoding;
        launch_audio_pack(a, grid, nullptr);
        const int kept = count < 0 ? 0 : (count < max_rows ? count : max_rows);
        std::fwrite(&kept, 4, 1, out);
        std::fwrite(audio, row_bytes, (size_t)kept, out);
        std::fwrite(info, sizeof(info[0]), (size_t)kept, out);
        if (!untouched(audio, (size_t)kept * row_bytes, total_rows * row_bytes, 0xEE)) {
            std::fprintf(stderr, "host_audio: case %d wrote audio bytes behind the %d rows it kept\n", c, kept);
            return 1;
        }
        if (!untouched(info, (size_t)kept * sizeof(info[0]), total_rows * sizeof(info[0]), 0xEE)) {
            std::fprintf(stderr, "host_audio: case %d wrote a record behind the %d rows it kept\n", c, kept);
            return 1;
        }
        std::free(src);
        std::free(audio);
        std::free(info);
    }
    std::fclose(out);
    return 0;
}
