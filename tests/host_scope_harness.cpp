// tests/host_scope_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_band_scope.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the band scope's source itself -- csrc/band_scope.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernel with its wavefront
// semantics on the CPU (lanes as fibers; shuffles, barriers and a wavefront's LDS exchanges as rendezvous points), launched by the file's own
// launch_band_scope().  The test compares the rows it leaves with a float64 evaluation of the defining sum.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rtlsdr-airband_amd/csrc/band_scope.hip"
#include "../rtlsdr-airband_amd/csrc/params.h"

using namespace airband;

extern "C" {

// iq: [n_dev] spans of iq_stride bytes holding first_hop + wave_batch hops (+ the last window's tail).  mask [n_dev] or null.  mean / peak: [rows][fft_size], or null.
// window_out [fft_size].  Returns the number of rows, < 0 on error.
int hostscope_run(const airband_hip_config* cfg, const uint8_t* iq, long iq_stride, int first_hop, int n_windows, const uint8_t* mask, float* mean, float* peak,
                  float* window_out) {
    Plan p;
    const int rc = build_plan(cfg, p);
    if (rc != 0) return rc;
    std::vector<int> dev_of_row;
    for (int d = 0; d < p.n_dev; d++)
        if (!mask || mask[d]) dev_of_row.push_back(d);
    ScopeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.iq = iq;
    a.iq_stride = iq_stride;
    a.dev = p.dev.data();
    a.dev_of_row = dev_of_row.data();
    a.window = p.window.data();
    a.twiddle = reinterpret_cast<const float2*>(p.twiddle.data());
    a.mean = mean;
    a.peak = peak;
    a.n_rows = (int)dev_of_row.size();
    a.fft_log = p.fft_log;
    a.hop_samples = p.dev[0].hop_samples;
    a.bytes_per_sample = p.dev[0].bytes_per_sample;
    a.sfmt = p.dev[0].sfmt;
    a.first_hop = first_hop;
    a.span_hops = first_hop + p.wave_batch;
    a.wave_batch = p.wave_batch;
    a.n_windows = n_windows;
    launch_band_scope(a, nullptr);
    for (int i = 0; i < p.fft_size; i++) window_out[i] = p.window[i];
    return a.n_rows;
}

int hostscope_waves(int fft_log, int bytes_per_sample) { return scope_waves(fft_log, bytes_per_sample); }
long hostscope_region_bytes(int fft_log, int bytes_per_sample) { return scope_region_bytes(fft_log, bytes_per_sample); }

int hostscope_geometry(const airband_hip_config* cfg, int* hop_samples, int* wave_batch) {
    Plan p;
    if (build_plan(cfg, p) != 0) return -1;
    *hop_samples = p.dev[0].hop_samples;
    *wave_batch = p.wave_batch;
    return 0;
}
}
