// tests/host_survey_harness.cpp -- TEST HARNESS ONLY (built by tests/test_host_band_survey.py with the host clang++ into a temporary directory; never part of,
// linked into or loaded by the library).
// Compiles the band survey's source itself -- csrc/band_survey.hip, through tests/hostshim_wave64/hip/hip_runtime.h -- and runs its kernel with its wavefront
// semantics on the CPU (lanes as fibers; shuffles and barriers as rendezvous points), launched by the file's own launch_band_survey().  The test compares what
// it leaves with capi.band_survey_reference().  The shim's dynamic LDS carries a guard zone behind the launch's bytes: a write past them aborts.
// With -DHOSTSURVEY_MAIN the file is a stand-alone program (its own main, rows from a fixed generator against a plain C++ evaluation of the definition): the form
// in which this code can be run under a host sanitizer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../rtlsdr-airband_amd/csrc/band_survey.hip"

using namespace airband;

extern "C" {

// rows [n_rows][1 << fft_log] (any alignment: copied to a 16-byte aligned buffer, as device rows are), bin_first [n_rows + 1], bins: a row's channel bins.
// summary [n_rows], peaks [n_rows][max_peaks].  Returns 0.
int hostsurvey_run(const float* rows, int n_rows, int fft_log, const int* bin_first, const int* bins, int max_peaks, int floor_permille, float ratio, int guard_bins,
                   airband_hip_band_summary* summary, airband_hip_band_peak* peaks) {
    const size_t N = (size_t)1 << fft_log;
    float* al = static_cast<float*>(std::aligned_alloc(64, n_rows * N * sizeof(float)));
    if (!al) return -1;
    std::memcpy(al, rows, n_rows * N * sizeof(float));
    SurveyArgs a;
    std::memset(&a, 0, sizeof(a));
    a.rows = al;
    a.bin_first = bin_first;
    a.bins = bins;
    a.summary = summary;
    a.peaks = peaks;
    a.n_rows = n_rows;
    a.fft_log = fft_log;
    a.max_peaks = max_peaks;
    const long r = ((long)N * floor_permille) / 1000; // the rank airband_hip_set_band_survey() hands the kernel
    a.rank = (int)(r < (long)N - 1 ? r : (long)N - 1);
    a.guard_bins = guard_bins;
    a.ratio = ratio;
    launch_band_survey(a, nullptr);
    std::free(al);
    return 0;
}

long hostsurvey_lds_bytes(int fft_log) { return (long)survey_lds_bytes(fft_log); }
}

#ifdef HOSTSURVEY_MAIN
// the definition of include/airband_hip.h, plainly
static void plain(const unsigned* u, int N, const std::vector<int>& bins, int max_peaks, int permille, float ratio, int guard, airband_hip_band_summary& s,
                  std::vector<airband_hip_band_peak>& pk) {
    std::vector<unsigned> o(u, u + N);
    std::sort(o.begin(), o.end());
    const unsigned fl = o[std::min<long>(N - 1, (long)N * permille / 1000)];
    float f, t;
    std::memcpy(&f, &fl, 4);
    t = f * ratio;
    unsigned tb;
    std::memcpy(&tb, &t, 4);
    int mb = 0;
    std::vector<std::pair<unsigned long long, int>> found;
    s.n_over = 0;
    for (int k = 0; k < N; k++) {
        if (u[k] > u[mb]) mb = k;
        if (!(u[k] > tb)) continue;
        s.n_over++;
        if (!(u[k] >= u[(k + N - 1) % N] && u[k] > u[(k + 1) % N])) continue;
        bool covered = false;
        for (int b : bins) covered = covered || (guard >= 0 && std::min(std::abs(k - b), N - std::abs(k - b)) <= guard);
        if (!covered) found.push_back({((unsigned long long)u[k] << 32) | (unsigned)(N - 1 - k), k});
    }
    std::sort(found.rbegin(), found.rend());
    s.floor = f;
    s.threshold = t;
    std::memcpy(&s.max_power, &u[mb], 4);
    s.max_bin = mb;
    s.n_peaks = (int)found.size();
    s.reserved[0] = s.reserved[1] = 0;
    pk.assign(max_peaks, airband_hip_band_peak{-1, 0.0f});
    for (int i = 0; i < max_peaks && i < (int)found.size(); i++) {
        pk[i].bin = found[i].second;
        std::memcpy(&pk[i].power, &u[found[i].second], 4);
    }
}

int main() {
    unsigned long long x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (unsigned)(x >> 16); };
    int bad = 0, runs = 0;
    for (int fft_log : {8, 9, 10, 13})
        for (int kind = 0; kind < 3; kind++) {
            const int N = 1 << fft_log, n_rows = 2, max_peaks = kind == 2 ? 64 : 5;
            std::vector<unsigned> u((size_t)n_rows * N);
            const unsigned four[4] = {0x3f800000u, 0x41200000u, 0x42c80000u, 0x00000000u};
            for (auto& v : u) v = kind == 0 ? rnd() : kind == 1 ? four[rnd() & 3] : (0x3f800000u + (rnd() & 0xfffffu));
            std::vector<int> bin_first = {0, 3, 4}, bins = {1, N / 2, N - 5, 17};
            std::vector<airband_hip_band_summary> s(n_rows);
            std::vector<airband_hip_band_peak> p((size_t)n_rows * max_peaks);
            const int permille = kind == 0 ? 500 : kind == 1 ? 250 : 0;
            hostsurvey_run(reinterpret_cast<const float*>(u.data()), n_rows, fft_log, bin_first.data(), bins.data(), max_peaks, permille, 1.5f, kind == 2 ? -1 : 3, s.data(), p.data());
            for (int r = 0; r < n_rows; r++, runs++) {
                airband_hip_band_summary ws;
                std::vector<airband_hip_band_peak> wp;
                plain(u.data() + (size_t)r * N, N, std::vector<int>(bins.begin() + bin_first[r], bins.begin() + bin_first[r + 1]), max_peaks, permille, 1.5f, kind == 2 ? -1 : 3, ws, wp);
                if (std::memcmp(&ws, &s[r], sizeof(ws)) || std::memcmp(wp.data(), &p[(size_t)r * max_peaks], sizeof(wp[0]) * max_peaks)) {
                    std::printf("MISMATCH fft %d kind %d row %d\n", N, kind, r);
                    bad++;
                }
            }
        }
    std::printf("%d rows, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
