/* csrc/driver_band.cpp -- the band outputs of the host driver: scope, survey, watch and follow (airband_hip_set_band_* / _collect_band_* / _device_band_*), and
 * their launches around stage 1 and behind the demod kernels (hooks of airband_hip.cpp: launch_front, run_back_half). */
#include "driver.h"

using namespace airband;

/* The band scope of the batch whose stage 1 goes on stream s (airband_hip_set_band_scope): it depends on the batch's input only, like AFC's one-hop spectrum
 * (airband_hip.cpp, launch_last_hop_spectrum).  scope_fork() in front of stage 1: the kernel runs on the scope's own stream beside it.  scope_join() behind stage 1: s waits for it, so that EVERY point
 * that declares the batch's input consumed by recording an event on s behind stage 1 -- ev_stage_read of the host ring, front_done of pipelined and run-ahead
 * handles, the stream order a run-ahead batch's next stage 1 relies on -- is behind the scope's reads too, and the batch's results, which wait for stage 1, are
 * complete only once the scope is.  On a CALLER's stream there is no fork: the kernel goes on that stream behind stage 1. */
static bool scope_on_side(const airband_hip_handle* h, hipStream_t s) { return s == h->stream || s == h->front; }

static ScopeArgs scope_args(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r) {
    BandScope& sc = h->scope;
    const Plan& p = h->plan;
    const int set = (int)(sc.launches % (uint64_t)sc.n_sets);
    ScopeArgs a;
    a.iq = (const uint8_t*)d_iq;
    a.iq_stride = (long)stride_bytes;
    a.dev = h->d_dev.p;
    a.dev_of_row = sc.d_dev_of_row.p;
    a.window = h->d_window.p;
    a.twiddle = reinterpret_cast<const float2*>(h->d_twiddle.p);
    a.mean = sc.d_mean[set].p;
    a.peak = sc.d_peak[set].p;
    a.prev_mean = sc.n_sets > 1 ? sc.d_mean[set ^ 1].p : nullptr;
    a.prev_peak = sc.n_sets > 1 ? sc.d_peak[set ^ 1].p : nullptr;
    a.n_rows = sc.n_rows;
    a.fft_log = p.fft_log;
    a.hop_samples = p.dev[0].hop_samples;
    a.bytes_per_sample = p.dev[0].bytes_per_sample;
    a.sfmt = p.dev[0].sfmt;
    a.first_hop = r.n_hops - h->B; /* the first batch's AGC_EXTRA lead-in hops are never selected */
    a.span_hops = r.n_hops;
    a.wave_batch = h->B;
    a.n_windows = sc.windows;
    a.region_bytes = 0;
    return a;
}

/* The band survey of the same batch (airband_hip_set_band_survey): directly behind the scope's kernel on whatever stream that went to, so that stream order alone
 * makes the rows complete, a switched-off dongle's carried-over row included.  Its results go to the set the scope's rows went to. */
static void launch_survey_behind_scope(airband_hip_handle* h, const ScopeArgs& sa, hipStream_t s) {
    BandScope& sc = h->scope;
    BandSurvey& sv = sc.survey;
    if (sv.max_peaks <= 0) return;
    const int set = (int)(sc.launches % (uint64_t)sc.n_sets);
    SurveyArgs a;
    a.rows = sv.trace == AIRBAND_SCOPE_MEAN ? sa.mean : sa.peak;
    a.bin_first = sv.d_bin_first.p;
    a.bins = sv.d_bins.p;
    a.summary = sv.d_summary[set].p;
    a.peaks = sv.d_peaks[set].p;
    a.n_rows = sc.n_rows;
    a.fft_log = sa.fft_log;
    a.max_peaks = sv.max_peaks;
    a.rank = sv.rank;
    a.guard_bins = sv.guard_bins;
    a.ratio = sv.ratio;
    launch_band_survey(a, s);
    /* the band watch of the same batch (airband_hip_set_band_watch), behind the survey it reads: the tables of the launch before are in the other set */
    BandWatch& w = sv.watch;
    if (w.max_tracks <= 0) return;
    const int prev = sc.n_sets > 1 ? set ^ 1 : set;
    WatchArgs wa;
    wa.dev = h->d_dev.p;
    wa.dev_of_row = sc.d_dev_of_row.p;
    wa.summary = a.summary;
    wa.peaks = a.peaks;
    wa.tracks_in = w.d_tracks[prev].p;
    wa.rows_in = w.d_rows[prev].p;
    wa.tracks_out = w.d_tracks[set].p;
    wa.rows_out = w.d_rows[set].p;
    wa.stage = w.d_stage.p;
    wa.events = w.d_events[set].p;
    wa.n_events = w.d_count[set].p;
    wa.n_rows = sc.n_rows;
    wa.fft_log = sa.fft_log;
    wa.max_peaks = sv.max_peaks;
    wa.max_tracks = w.max_tracks;
    wa.match_bins = w.match_bins;
    wa.confirm_hits = w.confirm_hits;
    wa.release_misses = w.release_misses;
    wa.max_events = w.max_events;
    wa.batch = w.batch++;
    launch_band_watch(wa, s);
}

/* rows [r0, r0 + n) of a survey array of `per_row` elements a row -> the entries of the selected dongles among [first_dev, first_dev + n_dev): ONE copy, straight into
 * the caller's array where every dongle of the range is selected, through a host vector otherwise.  Entries of the other dongles are set to `blank`. */
template <class T>
static int collect_survey_rows(airband_hip_handle* h, const T* d_src, size_t per_row, int first_dev, int n_dev, T* out, const T& blank, hipStream_t s) {
    const BandScope& sc = h->scope;
    int r0 = -1, n = 0;
    for (int i = 0; i < n_dev; i++)
        if (sc.row_of_dev[first_dev + i] >= 0) {
            if (r0 < 0) r0 = sc.row_of_dev[first_dev + i];
            n++; /* rows are dense in ascending dongle order: the range's rows are r0 .. r0 + n - 1 */
        }
    std::vector<T> tmp(n == n_dev ? 0 : (size_t)n * per_row);
    T* const dst = n == n_dev ? out : tmp.data();
    if (n) HIP_TRY(h, hipMemcpyAsync(dst, d_src + (size_t)r0 * per_row, (size_t)n * per_row * sizeof(T), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    for (int i = 0; n != n_dev && i < n_dev; i++) { /* dealt out from the host vector */
        const int row = sc.row_of_dev[first_dev + i];
        if (row < 0) std::fill(out + (size_t)i * per_row, out + (size_t)(i + 1) * per_row, blank);
        else std::copy(tmp.begin() + (size_t)(row - r0) * per_row, tmp.begin() + (size_t)(row - r0 + 1) * per_row, out + (size_t)i * per_row);
    }
    return AIRBAND_HIP_OK;
}

/* the scope's kernel and what hangs on it on stream `on`, and ev_done behind them.  Front batch front_batches then has its scope in set (launches % n_sets); the
 * set becomes the current one with the batch's back half (run_back_half) */
static int launch_scope_on(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r, hipStream_t on) {
    BandScope& sc = h->scope;
    const ScopeArgs sa = scope_args(h, d_iq, stride_bytes, r);
    launch_band_scope(sa, on);
    launch_survey_behind_scope(h, sa, on);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("band scope launch: ") + hipGetErrorString(e));
    HIP_TRY(h, hipEventRecord(sc.ev_done, on), AIRBAND_HIP_ERUNTIME);
    sc.set_of_front[h->front_batches & 1] = (int)(sc.launches % (uint64_t)sc.n_sets);
    sc.launches++;
    return AIRBAND_HIP_OK;
}

static airband_hip_band_track blank_track() {
    airband_hip_band_track none;
    std::memset(&none, 0, sizeof(none));
    none.bin = -1;
    return none;
}

int airband::scope_fork(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r, hipStream_t s) {
    BandScope& sc = h->scope;
    if (!has_scope(h) || !scope_on_side(h, s)) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipEventRecord(sc.ev_fork, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamWaitEvent(sc.stream, sc.ev_fork, 0), AIRBAND_HIP_ERUNTIME);
    if (h->ev_last && h->ev_last_pending) HIP_TRY(h, hipStreamWaitEvent(sc.stream, h->ev_last, 0), AIRBAND_HIP_ERUNTIME); /* a batch (and its scope) on a caller's stream */
    return launch_scope_on(h, d_iq, stride_bytes, r, sc.stream);
}

int airband::scope_join(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r, hipStream_t s) {
    BandScope& sc = h->scope;
    if (!has_scope(h)) return AIRBAND_HIP_OK;
    if (scope_on_side(h, s)) {
        HIP_TRY(h, hipStreamWaitEvent(s, sc.ev_done, 0), AIRBAND_HIP_ERUNTIME);
        return AIRBAND_HIP_OK;
    }
    /* the caller's stream, behind stage 1 -- and behind the scope launch before this one, whose rows a switched-off dongle's are carried over from */
    if (sc.launches > 0) HIP_TRY(h, hipStreamWaitEvent(s, sc.ev_done, 0), AIRBAND_HIP_ERUNTIME);
    return launch_scope_on(h, d_iq, stride_bytes, r, s);
}

/* The band follow of the batch whose back half goes on stream s (airband_hip_set_band_follow), behind its demod kernels.  It reads the track tables the batch's
 * watch left, and the watch ran on the scope's stream: s is behind that already (scope_join() made the stage-1 stream wait for the scope, and a handle with
 * followers runs both halves of a batch on one stream), said again here because this is the point that depends on it.  The watch batch number of this batch is
 * the last one launched: such a handle never has a second stage 1 in flight. */
void airband::launch_follow_behind_demod(airband_hip_handle* h, int* moved_epoch, int epoch, hipStream_t s) {
    BandScope& sc = h->scope;
    BandWatch& w = sc.survey.watch;
    BandFollow& fo = w.follow;
    if (scope_on_side(h, s)) (void)hipStreamWaitEvent(s, sc.ev_done, 0);
    FollowArgs a;
    a.dev = h->d_dev.p;
    a.dev_of_row = sc.d_dev_of_row.p;
    a.tracks = w.d_tracks[sc.cur].p;
    a.fol_range = fo.d_range.p;
    a.fol_slot = fo.d_slot.p;
    a.fol_home = fo.d_home.p;
    a.followers = fo.d_followers.p;
    a.rows = fo.d_rows.p;
    a.stage = fo.d_stage.p;
    a.changes = fo.d_changes.p;
    a.n_changes = fo.d_count.p;
    a.cs = h->d_cs.p;
    a.moved_epoch = moved_epoch;
    a.epoch = epoch;
    a.n_rows = sc.n_rows;
    a.n_follow = (int)h->plan.follow_ext.size();
    a.n_slots = h->n_slots;
    a.fft_log = h->plan.fft_log;
    a.max_tracks = w.max_tracks;
    a.cap = fo.cap;
    a.max_changes = fo.max_changes;
    a.batch = w.batch - 1u;
    launch_band_follow(a, s);
}

extern "C" {

int airband_hip_set_band_scope(airband_hip_handle* h, const uint8_t* dev_mask, int32_t windows_per_batch, uint32_t traces) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const Plan& p = h->plan;
    if (windows_per_batch < 1 || windows_per_batch > h->B) return fail(h, AIRBAND_HIP_EINVAL, "windows_per_batch must lie in 1 .. WAVE_BATCH");
    if (traces == 0 || (traces & ~(uint32_t)(AIRBAND_SCOPE_MEAN | AIRBAND_SCOPE_PEAK))) return fail(h, AIRBAND_HIP_EINVAL, "traces must be a non-empty set of AIRBAND_SCOPE_* bits");
    BandScope sc;
    sc.row_of_dev.assign((size_t)p.n_dev, -1);
    std::vector<int> dev_of_row;
    for (int d = 0; d < p.n_dev; d++)
        if (!dev_mask || dev_mask[d]) {
            sc.row_of_dev[d] = (int)dev_of_row.size();
            dev_of_row.push_back(d);
        }
    if (dev_of_row.empty()) return fail(h, AIRBAND_HIP_EINVAL, "the mask selects no dongle");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the band scope is set before the first batch");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the handle and moved in whole: a failed allocation leaves the handle as it was */
    sc.windows = windows_per_batch;
    sc.traces = traces;
    sc.n_rows = (int)dev_of_row.size();
    sc.n_sets = deep_rings(h) ? 2 : 1; /* where the next stage 1 may run before this batch's results are collected (the validity rule of the result buffers) */
    const size_t n = (size_t)sc.n_rows * (size_t)h->N;
    hipError_t e = upload(sc.d_row_of_dev, sc.row_of_dev);
    if (e == hipSuccess) e = upload(sc.d_dev_of_row, dev_of_row);
    for (int q = 0; q < sc.n_sets; q++) {
        if (e == hipSuccess && (traces & AIRBAND_SCOPE_MEAN)) e = sc.d_mean[q].alloc_zeroed(n);
        if (e == hipSuccess && (traces & AIRBAND_SCOPE_PEAK)) e = sc.d_peak[q].alloc_zeroed(n);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* the zeros are in place before a kernel on another stream writes the rows */
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&sc.stream.v, hipStreamNonBlocking);
    if (e == hipSuccess) e = sc.ev_fork.ensure();
    if (e == hipSuccess) e = sc.ev_done.ensure();
    if (e != hipSuccess) return alloc_failed(h, e, "band scope buffers: ");
    h->scope = std::move(sc);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_band_scope(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, float* mean, float* peak) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    if (!has_scope(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCOPE);
    if (!dev_range_ok(h, first_dev, n_dev)) return fail(h, AIRBAND_HIP_EINVAL, "device range out of bounds");
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    const size_t N = (size_t)h->N;
    float* const out[2] = {mean, peak};
    const float* const src[2] = {sc.d_mean[sc.cur].p, sc.d_peak[sc.cur].p};
    for (int t = 0; t < 2; t++) {
        if (!out[t]) continue;
        for (int i = 0; i < n_dev;) { /* runs of selected dongles are runs of rows: one copy each */
            const int row = src[t] ? sc.row_of_dev[first_dev + i] : -1;
            int j = i + 1;
            if (row < 0) { /* not selected (or a trace the scope does not keep): zeros */
                std::memset(out[t] + (size_t)i * N, 0, N * sizeof(float));
            } else {
                while (j < n_dev && sc.row_of_dev[first_dev + j] >= 0) j++;
                HIP_TRY(h, hipMemcpyAsync(out[t] + (size_t)i * N, src[t] + (size_t)row * N, (size_t)(j - i) * N * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
            }
            i = j;
        }
    }
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_device_band_scope(airband_hip_handle* h, float** d_mean, float** d_peak, int32_t** d_row_of_dev) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    if (!has_scope(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCOPE);
    if (d_mean) *d_mean = sc.d_mean[sc.cur].p;
    if (d_peak) *d_peak = sc.d_peak[sc.cur].p;
    if (d_row_of_dev) *d_row_of_dev = sc.d_row_of_dev.p;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_band_survey(airband_hip_handle* h, uint32_t trace, int32_t max_peaks, int32_t floor_permille, float threshold_ratio, int32_t guard_bins) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const Plan& p = h->plan;
    BandScope& sc = h->scope;
    if (!has_scope(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCOPE);
    if ((trace != AIRBAND_SCOPE_MEAN && trace != AIRBAND_SCOPE_PEAK) || !(sc.traces & trace))
        return fail(h, AIRBAND_HIP_EINVAL, "trace must be exactly one AIRBAND_SCOPE_* bit the scope keeps");
    if (max_peaks < 1 || max_peaks > 64) return fail(h, AIRBAND_HIP_EINVAL, "max_peaks must lie in 1 .. 64");
    if (floor_permille < 0 || floor_permille > 1000) return fail(h, AIRBAND_HIP_EINVAL, "floor_permille must lie in 0 .. 1000");
    if (!std::isfinite(threshold_ratio) || !(threshold_ratio > 0.0f)) return fail(h, AIRBAND_HIP_EINVAL, "threshold_ratio must be finite and above 0");
    if (guard_bins < -1 || guard_bins > h->N / 2) return fail(h, AIRBAND_HIP_EINVAL, "guard_bins must lie in -1 .. fft_size / 2");
    if (p.fft_log < 8 || p.fft_log > 13) return fail(h, AIRBAND_HIP_EINVAL, "the band survey takes fft sizes 256 .. 8192");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the band survey is set before the first batch");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the handle and moved in whole: a failed allocation leaves the handle, its scope and an earlier survey as they were */
    BandSurvey sv;
    sv.trace = trace;
    sv.rank = (int)std::min<int64_t>((int64_t)h->N - 1, (int64_t)h->N * floor_permille / 1000);
    sv.guard_bins = guard_bins;
    sv.ratio = threshold_ratio;
    std::vector<int> bin_first(1, 0), bins;
    for (int d = 0; d < p.n_dev; d++) {
        if (sc.row_of_dev[d] < 0) continue;
        for (int j = 0; j < p.dev[d].n_ch; j++) bins.push_back(p.cc[p.chan_base[d] + j].base_bin); /* the prepare-time bin: slot [0] of airband_hip_channel_constants() */
        bin_first.push_back((int)bins.size());
    }
    const std::vector<airband_hip_band_peak> none((size_t)sc.n_rows * (size_t)max_peaks, airband_hip_band_peak{-1, 0.0f});
    hipError_t e = upload(sv.d_bin_first, bin_first);
    if (e == hipSuccess) e = upload(sv.d_bins, bins);
    for (int q = 0; q < sc.n_sets; q++) {
        if (e == hipSuccess) e = sv.d_summary[q].alloc_zeroed((size_t)sc.n_rows);
        if (e == hipSuccess) e = upload(sv.d_peaks[q], none);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* the initial values are in place before a kernel on another stream writes the rows */
    if (e != hipSuccess) return alloc_failed(h, e, "band survey buffers: ");
    sv.max_peaks = max_peaks;
    sc.survey = std::move(sv);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_band_survey(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_band_summary* summary, airband_hip_band_peak* peaks) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    const BandSurvey& sv = sc.survey;
    if (!has_survey(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SURVEY);
    if (!dev_range_ok(h, first_dev, n_dev)) return fail(h, AIRBAND_HIP_EINVAL, "device range out of bounds");
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    int rc = summary ? collect_survey_rows(h, sv.d_summary[sc.cur].p, 1, first_dev, n_dev, summary, airband_hip_band_summary{}, s) : AIRBAND_HIP_OK;
    if (rc == AIRBAND_HIP_OK && peaks) rc = collect_survey_rows(h, sv.d_peaks[sc.cur].p, (size_t)sv.max_peaks, first_dev, n_dev, peaks, airband_hip_band_peak{-1, 0.0f}, s);
    return rc;
}

int airband_hip_device_band_survey(airband_hip_handle* h, airband_hip_band_summary** d_summary, airband_hip_band_peak** d_peaks) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    if (!has_survey(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SURVEY);
    if (d_summary) *d_summary = sc.survey.d_summary[sc.cur].p;
    if (d_peaks) *d_peaks = sc.survey.d_peaks[sc.cur].p;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_band_watch(airband_hip_handle* h, int32_t max_tracks, int32_t match_bins, int32_t confirm_hits, int32_t release_misses, int64_t max_events) {
    if (!h) return AIRBAND_HIP_EINVAL;
    BandScope& sc = h->scope;
    BandSurvey& sv = sc.survey;
    if (!has_survey(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SURVEY);
    if (max_tracks < 1 || max_tracks > 64) return fail(h, AIRBAND_HIP_EINVAL, "max_tracks must lie in 1 .. 64");
    if (match_bins < 0 || match_bins > h->N / 2) return fail(h, AIRBAND_HIP_EINVAL, "match_bins must lie in 0 .. fft_size / 2");
    if (confirm_hits < 1 || confirm_hits > 255) return fail(h, AIRBAND_HIP_EINVAL, "confirm_hits must lie in 1 .. 255");
    if (release_misses < 1 || release_misses > 255) return fail(h, AIRBAND_HIP_EINVAL, "release_misses must lie in 1 .. 255");
    const int64_t per_row = (int64_t)max_tracks + sv.max_peaks, most = (int64_t)sc.n_rows * per_row;
    if (max_events < 1 || max_events > most || max_events > INT32_MAX) return fail(h, AIRBAND_HIP_EINVAL, "max_events must lie in 1 .. rows * (max_tracks + max_peaks)");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the band watch is set before the first batch");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the handle and moved in whole: a failed allocation leaves the handle, its survey and an earlier watch as they were */
    BandWatch w;
    w.match_bins = match_bins;
    w.confirm_hits = confirm_hits;
    w.release_misses = release_misses;
    w.max_events = (int)max_events;
    const std::vector<airband_hip_band_track> free_slots((size_t)sc.n_rows * (size_t)max_tracks, blank_track());
    hipError_t e = w.d_stage.alloc((size_t)most);
    for (int q = 0; q < sc.n_sets; q++) {
        if (e == hipSuccess) e = upload(w.d_tracks[q], free_slots);
        if (e == hipSuccess) e = w.d_rows[q].alloc_zeroed((size_t)sc.n_rows);
        if (e == hipSuccess) e = w.d_events[q].alloc_zeroed((size_t)max_events);
        if (e == hipSuccess) e = w.d_count[q].alloc_zeroed(1);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* the initial values are in place before a kernel on another stream reads the tables */
    if (e != hipSuccess) return alloc_failed(h, e, "band watch buffers: ");
    w.max_tracks = max_tracks;
    sv.watch = std::move(w);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_band_events(airband_hip_handle* h, int64_t* n_events, airband_hip_band_event* events) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    const BandWatch& w = sc.survey.watch;
    if (!has_watch(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_WATCH);
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    return collect_counted(h, w.d_count[sc.cur].p, (int64_t)sc.n_rows * (w.max_tracks + sc.survey.max_peaks), w.max_events, "event count out of range: ", n_events, w.d_events[sc.cur].p, events, s);
}

int airband_hip_collect_band_tracks(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_band_watch_row* rows, airband_hip_band_track* tracks) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    const BandWatch& w = sc.survey.watch;
    if (!has_watch(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_WATCH);
    if (!dev_range_ok(h, first_dev, n_dev)) return fail(h, AIRBAND_HIP_EINVAL, "device range out of bounds");
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    int rc = rows ? collect_survey_rows(h, w.d_rows[sc.cur].p, 1, first_dev, n_dev, rows, airband_hip_band_watch_row{}, s) : AIRBAND_HIP_OK;
    if (rc == AIRBAND_HIP_OK && tracks) rc = collect_survey_rows(h, w.d_tracks[sc.cur].p, (size_t)w.max_tracks, first_dev, n_dev, tracks, blank_track(), s);
    return rc;
}

int airband_hip_device_band_watch(airband_hip_handle* h, int32_t** d_n_events, airband_hip_band_event** d_events, airband_hip_band_watch_row** d_rows, airband_hip_band_track** d_tracks) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandScope& sc = h->scope;
    const BandWatch& w = sc.survey.watch;
    if (!has_watch(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_WATCH);
    if (d_n_events) *d_n_events = w.d_count[sc.cur].p;
    if (d_events) *d_events = w.d_events[sc.cur].p;
    if (d_rows) *d_rows = w.d_rows[sc.cur].p;
    if (d_tracks) *d_tracks = w.d_tracks[sc.cur].p;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_band_follow(airband_hip_handle* h, int64_t max_changes) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const Plan& p = h->plan;
    BandScope& sc = h->scope;
    BandWatch& w = sc.survey.watch;
    if (!has_watch(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_WATCH);
    const int64_t n_follow = (int64_t)p.follow_ext.size();
    if (n_follow == 0) return fail(h, AIRBAND_HIP_EINVAL, "the handle has no followers (airband_hip_prepare_follow)");
    const int64_t most = n_follow + (int64_t)sc.n_rows * w.max_tracks;
    if (max_changes < 1 || max_changes > most || max_changes > INT32_MAX) return fail(h, AIRBAND_HIP_EINVAL, "max_changes must lie in 1 .. followers + rows * max_tracks");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the band follow is set before the first batch");
    if (sc.n_sets != 1) return fail(h, AIRBAND_HIP_EINVAL, "a handle with followers keeps one set of scope rows"); /* (it never runs ahead: airband_hip_prepare_follow) */
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* the followers in prepare order are in ascending dongle order, as the scope's rows are: a row's followers are one range */
    std::vector<int> range((size_t)sc.n_rows * 2, 0), slot, home;
    std::vector<airband_hip_band_follower> start;
    int most_per_row = 0;
    for (size_t i = 0; i < p.follow_ext.size(); i++) {
        const int ext = p.follow_ext[i];
        const ChanConst& c = p.cc[(size_t)ext];
        const int row = sc.row_of_dev[(size_t)c.dev];
        if (row >= 0) {
            if (range[(size_t)row * 2 + 1]++ == 0) range[(size_t)row * 2] = (int)i;
            most_per_row = std::max(most_per_row, range[(size_t)row * 2 + 1]);
        }
        slot.push_back(h->ext_to_slot[(size_t)ext]);
        home.push_back(c.base_bin);
        airband_hip_band_follower f;
        std::memset(&f, 0, sizeof(f));
        f.channel = ext;
        f.bin = c.base_bin;
        f.track = -1;
        start.push_back(f);
    }
    /* built beside the handle and moved in whole: a failed allocation leaves the handle, its watch and an earlier follow as they were */
    BandFollow fo;
    fo.cap = most_per_row + w.max_tracks;
    hipError_t e = upload(fo.d_range, range);
    if (e == hipSuccess) e = upload(fo.d_slot, slot);
    if (e == hipSuccess) e = upload(fo.d_home, home);
    if (e == hipSuccess) e = upload(fo.d_followers, start);
    if (e == hipSuccess) e = fo.d_rows.alloc_zeroed((size_t)sc.n_rows);
    if (e == hipSuccess) e = fo.d_stage.alloc((size_t)sc.n_rows * (size_t)fo.cap);
    if (e == hipSuccess) e = fo.d_changes.alloc_zeroed((size_t)max_changes);
    if (e == hipSuccess) e = fo.d_count.alloc_zeroed(1);
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* the initial values are in place before a kernel on another stream reads them */
    if (e != hipSuccess) return alloc_failed(h, e, "band follow buffers: ");
    fo.max_changes = (int)max_changes;
    w.follow = std::move(fo);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_band_follow_changes(airband_hip_handle* h, int64_t* n_changes, airband_hip_band_follow_change* changes) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandFollow& fo = h->scope.survey.watch.follow;
    if (!has_follow(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_FOLLOW);
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    return collect_counted(h, fo.d_count.p, (int64_t)h->scope.n_rows * fo.cap, fo.max_changes, "change count out of range: ", n_changes, fo.d_changes.p, changes, s);
}

int airband_hip_collect_band_followers(airband_hip_handle* h, airband_hip_band_follower* followers, airband_hip_band_follow_row* rows) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandFollow& fo = h->scope.survey.watch.follow;
    if (!has_follow(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_FOLLOW);
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    if (followers) {
        HIP_TRY(h, hipMemcpyAsync(followers, fo.d_followers.p, fo.d_followers.n * sizeof(airband_hip_band_follower), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    }
    if (rows) return collect_survey_rows(h, fo.d_rows.p, 1, 0, h->plan.n_dev, rows, airband_hip_band_follow_row{}, s);
    return AIRBAND_HIP_OK;
}

int airband_hip_device_band_follow(airband_hip_handle* h, int32_t** d_n_changes, airband_hip_band_follow_change** d_changes, airband_hip_band_follower** d_followers, airband_hip_band_follow_row** d_rows) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const BandFollow& fo = h->scope.survey.watch.follow;
    if (!has_follow(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_FOLLOW);
    if (d_n_changes) *d_n_changes = fo.d_count.p;
    if (d_changes) *d_changes = fo.d_changes.p;
    if (d_followers) *d_followers = fo.d_followers.p;
    if (d_rows) *d_rows = fo.d_rows.p;
    return AIRBAND_HIP_OK;
}

} /* extern "C" */
