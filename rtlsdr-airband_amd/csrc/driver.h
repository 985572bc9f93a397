/* csrc/driver.h -- what the files of the host driver share (airband_hip.cpp and driver_*.cpp): error reporting, the steps every entry point of an optional output
 * repeats, and the hooks through which the batch path (airband_hip.cpp) reaches the feature files.  The helpers are static: the library exports none of them. */
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "handle.h"

namespace airband {

/* the ring rows a batch's stage 1 produces */
struct FrontRows {
    int first_row, n_hops;
};

/* what a transmission spool or an RTP stream reads of its source after the source's step: the channel spool and the channel stream of the output gate and the
 * encoder, the mixer spool and the mixer stream of the mixer gate and the mixer pack */
struct SpoolSource {
    const unsigned long long* mask; /* the gate's verdicts */
    const int* block_count;         /* ... and its per-workgroup counts */
    const uint8_t* audio;           /* the listed rows, encoded */
    const airband_hip_audio_row* info;
    int n, max_rows;                /* items (channels / mixers), the list's capacity */
    int frames;                     /* wave_batch: `first` of a transmission without a stored row; the frames of a row the RTP stream cuts */
    int width;                      /* samples per frame: 1 for channels, the mixer gate's W */
};

#pragma GCC visibility push(hidden)
extern thread_local std::string g_prepare_error; /* airband_hip.cpp: the message of a failure without a handle (airband_hip_last_error(NULL)) */
/* the hooks of the batch path (airband_hip.cpp: launch_front, run_back_half), by the file that defines them.  driver_band.cpp: the scope (with its survey and watch) around stage 1, the follow behind the demod kernels */
int scope_fork(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r, hipStream_t s);
int scope_join(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r, hipStream_t s);
void launch_follow_behind_demod(airband_hip_handle* h, int* moved_epoch, int epoch, hipStream_t s);
/* driver_gate.cpp: the gate, the encoder and the spool's step behind the emit / mixer launches */
void launch_gate_behind_mix(airband_hip_handle* h, hipStream_t s);
/* driver_gate.cpp: the spool's host side over a TransmissionSpool and its source, ONE path for the channel spool and the mixer spool (driver_mix.cpp): a set
 * call's checks, allocate and initialise, the step, collect, flush, counters, device views */
int spool_check(airband_hip_handle* h, const uint8_t* spool, const std::vector<uint8_t>& gate, const char* item, int64_t pool_rows, int64_t export_rows,
                int64_t max_records, int32_t max_batches, std::vector<uint8_t>* mask);
int spool_build(airband_hip_handle* h, TransmissionSpool& sp, const std::vector<uint8_t>& mask, int max_rows, size_t row_bytes, int64_t pool_rows, int64_t export_rows,
                int64_t max_records, int32_t min_batches, int32_t idle_batches, int32_t max_batches, const char* what);
void spool_step(TransmissionSpool& sp, const SpoolSource& src, hipStream_t s);
int spool_collect(airband_hip_handle* h, const TransmissionSpool& sp, const SpoolSource& src, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting);
int spool_flush(airband_hip_handle* h, const TransmissionSpool& sp, const SpoolSource& src);
int spool_counters(airband_hip_handle* h, const TransmissionSpool& sp, airband_hip_spool_counters* out);
void spool_device_views(const TransmissionSpool& sp, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export);
/* driver_gate.cpp: the RTP stream's host side over an RtpStream and its source, ONE path for the channel stream and the mixer stream (driver_mix.cpp): a set
 * call's checks with allocate and initialise (`gate`: the source's gate bytes; `item`: "channel" / "mixer"; `what` ends with ": "), the step, the flush step,
 * collect (the count, the records and slots it keeps, then `extra_bytes` from d_extra to `extra`: axcindicate / has_signal, ONE synchronize), state, counters,
 * device views */
int rtp_slot_bytes_checked(int32_t encoding, int32_t frame_samples, int32_t width);
int rtp_build(airband_hip_handle* h, RtpStream& r, const airband_hip_rtp_source* sources, const std::vector<uint8_t>& gate, const char* item, int32_t encoding,
              const SpoolSource& src, int32_t frame_samples, int64_t max_packets, const char* what);
void rtp_step(RtpStream& r, const SpoolSource& src, hipStream_t s);
int rtp_flush(airband_hip_handle* h, RtpStream& r, const SpoolSource& src);
int rtp_collect(airband_hip_handle* h, const RtpStream& r, const SpoolSource& src, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets,
                const void* d_extra, void* extra, size_t extra_bytes);
int rtp_state(airband_hip_handle* h, const RtpStream& r, const SpoolSource& src, int64_t first, int64_t n, airband_hip_rtp_state* state, const char* item);
int rtp_counters(airband_hip_handle* h, const RtpStream& r, airband_hip_rtp_counters* out);
void rtp_device_views(const RtpStream& r, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state);
/* driver_mix.cpp: what the batch's mixer sums are launched with; one mixer input switched on or off in the grouped arrays (airband_hip_device_enable) */
MixArgs mix_args(const airband_hip_handle* h);
hipError_t write_mix_input(airband_hip_handle* h, int k);
/* driver_mix.cpp: the mixer gate's step (list, pack) behind whatever wrote the sums last on s: the batch (run_back_half) or airband_hip_mixer_gate_step() */
void launch_mixer_gate_step(airband_hip_handle* h, hipStream_t s);
/* driver_scan.cpp: prepare's step for handles with scan lists, the entries of a front batch, the exchange in front of the demod kernels, the hops behind them */
int prep_scan(airband_hip_handle* h);
void scan_latch(airband_hip_handle* h, uint64_t k, int first_row, int n_rows);
int scan_before_demod(airband_hip_handle* h, hipStream_t s);
void launch_scan_control_behind_demod(airband_hip_handle* h, hipStream_t s);
#pragma GCC visibility pop

static inline int fail(airband_hip_handle* h, int code, const std::string& msg) {
    if (h) h->error = msg;
    else g_prepare_error = msg;
    return code;
}

#define HIP_TRY(h, expr, code)                                                                                   \
    do {                                                                                                         \
        hipError_t e_ = (expr);                                                                                  \
        if (e_ != hipSuccess) return fail(h, code, std::string(#expr) + ": " + hipGetErrorString(e_));           \
    } while (0)

/* the HIP_TRY()s of prepare name this instead of the handle, which does not outlive a failure: the message goes to the thread's prepare error */
constexpr airband_hip_handle* PREPARING = nullptr;

template <class T>
static hipError_t upload(DevBuf<T>& b, const std::vector<T>& v) {
    hipError_t e = b.alloc(v.size());
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

/* Results of a batch that ran on a caller's stream: make the handle's own stream (on which collect / read_* / the stats kernel
 * are issued) wait for it on the GPU. */
static inline void order_behind_last_batch(airband_hip_handle* h) {
    if (h->ev_last && h->ev_last_pending) (void)hipStreamWaitEvent(h->stream, h->ev_last, 0);
}

/* what a call does first before it copies or launches on the handle's own stream, `s` from here on: the handle's device, and behind such a batch */
#define ON_OWN_STREAM(h, s)                                       \
    hipStream_t s = (h)->stream;                                  \
    HIP_TRY(h, hipSetDevice((h)->hip_device), AIRBAND_HIP_ENODEV); \
    order_behind_last_batch(h)

/* Work was enqueued on stream s.  If that is not the handle's own stream (a caller's: handed to process_device, or the one the last batch ran on), what the
 * handle does next on its own -- collect / read_* / synchronize / release, the next batch's sums -- has to come behind it: ev_last marks the place. */
static inline int results_enqueued_on(airband_hip_handle* h, hipStream_t s) {
    if (s == h->stream) return AIRBAND_HIP_OK;
    HIP_TRY(h, h->ev_last.ensure(), AIRBAND_HIP_ENODEV);
    HIP_TRY(h, hipEventRecord(h->ev_last, s), AIRBAND_HIP_ERUNTIME);
    h->ev_last_pending = true;
    return AIRBAND_HIP_OK;
}

/* the stream on which the last batch's mixer sums become final */
static inline hipStream_t results_stream(airband_hip_handle* h) { return h->pipeline ? h->stream : (h->last_stream ? h->last_stream : h->stream); }

/* stage 1 of the next batch may be written while stage 2 still reads this one: rings two batches deep, a front stream, the channelizer held to five wavefronts per CU */
static inline bool deep_rings(const airband_hip_handle* h) { return h->pipeline || h->run_ahead; }

/* the optional outputs: is it there, and what a call says where it is not */
static inline bool has_scope(const airband_hip_handle* h) { return h->scope.windows > 0; }
static inline bool has_survey(const airband_hip_handle* h) { return has_scope(h) && h->scope.survey.max_peaks > 0; }
static inline bool has_watch(const airband_hip_handle* h) { return has_survey(h) && h->scope.survey.watch.max_tracks > 0; }
static inline bool has_follow(const airband_hip_handle* h) { return has_watch(h) && h->scope.survey.watch.follow.max_changes > 0; }
static inline bool has_gate(const airband_hip_handle* h) { return h->gate.max_rows > 0; }
static inline bool has_encoding(const airband_hip_handle* h) { return has_gate(h) && h->gate.enc.encoding != AIRBAND_AUDIO_F32; }
static inline bool has_decimation(const airband_hip_handle* h) { return has_encoding(h) && h->gate.enc.dec.factor == 2; }
static inline bool has_spool(const airband_hip_handle* h) { return has_encoding(h) && h->gate.enc.spool.pool_rows > 0; }
static inline bool has_rtp(const airband_hip_handle* h) { return has_encoding(h) && h->gate.enc.rtp.max_packets > 0; }
static inline bool has_mixer_gate(const airband_hip_handle* h) { return h->mix.n_mixers > 0 && h->mix_gate.max_rows > 0; }
static inline bool has_mixer_spool(const airband_hip_handle* h) { return has_mixer_gate(h) && h->mix_gate.spool.pool_rows > 0; }
static inline bool has_mixer_rtp(const airband_hip_handle* h) { return has_mixer_gate(h) && h->mix_gate.rtp.max_packets > 0; }
static inline bool has_scan_control(const airband_hip_handle* h) { return h->scan_ctl.idle_batches > 0; }
constexpr const char* NO_SCOPE = "the handle has no band scope (airband_hip_set_band_scope)";
constexpr const char* NO_SURVEY = "the handle has no band survey (airband_hip_set_band_survey)";
constexpr const char* NO_WATCH = "the handle has no band watch (airband_hip_set_band_watch)";
constexpr const char* NO_FOLLOW = "the handle has no band follow (airband_hip_set_band_follow)";
constexpr const char* NO_GATE = "the handle has no output gate (airband_hip_set_output_gate)";
constexpr const char* NO_ENCODING = "the handle has no output encoding (airband_hip_set_output_encoding)";
constexpr const char* NO_SPOOL = "the handle has no transmission spool (airband_hip_set_transmission_spool)";
constexpr const char* NO_RTP = "the handle has no RTP stream (airband_hip_set_rtp_stream)";
constexpr const char* NO_MIXER_GATE = "the handle has no mixer gate (airband_hip_set_mixer_gate)";
constexpr const char* NO_MIXER_SPOOL = "the handle has no mixer spool (airband_hip_set_mixer_spool)";
constexpr const char* NO_MIXER_RTP = "the handle has no mixer RTP stream (airband_hip_set_mixer_rtp_stream)";
constexpr const char* NO_SCAN_CONTROL = "scan control is off (airband_hip_set_scan_control)";

/* they are set before the first batch (the message stays a literal at each fail(): "the band watch is set before the first batch") */
static inline bool started(const airband_hip_handle* h) { return h->front_batches > 0 || h->batches_done > 0; }
static inline bool dev_range_ok(const airband_hip_handle* h, int32_t first_dev, int32_t n_dev) { return first_dev >= 0 && n_dev >= 0 && (int64_t)first_dev + n_dev <= h->plan.n_dev; }

/* a set_*() whose allocations ended with `e`: the failed allocation is this call's error, reported here, not the next launch's.  `what` ends with ": " */
static inline int alloc_failed(airband_hip_handle* h, hipError_t e, const char* what) {
    (void)hipGetLastError();
    return fail(h, AIRBAND_HIP_ENOMEM, std::string(what) + hipGetErrorString(e));
}

/* How long a list is is on the device: the count first, checked against the most the kernels can have written (`what` ends with ": ") and reported whole, then
 * exactly those records, as many as the list keeps (`cap`).  Without `out` the count alone: one copy, one synchronize. */
template <class T>
static int collect_counted(airband_hip_handle* h, const int* d_count, int64_t most, int cap, const char* what, int64_t* n_out, const T* d_records, T* out, hipStream_t s) {
    int count = 0;
    HIP_TRY(h, hipMemcpyAsync(&count, d_count, sizeof(int), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (count < 0 || (int64_t)count > most) return fail(h, AIRBAND_HIP_ERUNTIME, what + std::to_string(count));
    if (n_out) *n_out = count;
    const size_t n = (size_t)(count < cap ? count : cap);
    if (out && n) {
        HIP_TRY(h, hipMemcpyAsync(out, d_records, n * sizeof(T), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    }
    return AIRBAND_HIP_OK;
}

}  // namespace airband
