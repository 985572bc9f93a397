/* csrc/driver_gate.cpp -- the gated outputs of the host driver: the output gate, the encoding of its rows, airband_hip_encode_audio and the transmission spool
 * (airband_hip_set_output_gate / _set_output_encoding / _set_transmission_spool and their collect / device entry points), and their launches behind the emit and
 * mixer launches of a batch (hook of airband_hip.cpp: run_back_half).  The spool's host side is written over a TransmissionSpool and a SpoolSource: the mixer
 * spool (driver_mix.cpp: airband_hip_set_mixer_spool and its collect / flush / counters / device entry points) goes through the same functions.  The RTP packet
 * stream (airband_hip_set_rtp_stream and its collect / state / counters / device entry points) is a second reader of the encoder's rows, beside the spool; its
 * host side is written over an RtpStream and a SpoolSource in the same way, and the mixer RTP stream (driver_mix.cpp: airband_hip_set_mixer_rtp_stream and its
 * entry points) goes through it.  The output decimation (airband_hip_set_output_decimation / _encoded_row_samples / _decimate_audio) halves the encoder's rows:
 * its kernel is launched in the encoder's place, and the spool and the stream read rows of half the length. */
#include "audio_decimate.h" /* AUDIO_DECIMATE_HIST */
#include "driver.h"

using namespace airband;

static GateArgs gate_args(const airband_hip_handle* h) {
    const OutputGate& g = h->gate;
    GateArgs a;
    a.gate = g.d_gate.p;
    a.axc = h->d_out_axc.p;
    a.prev = g.d_prev.p;
    a.mask = g.d_mask.p;
    a.block_count = g.d_block_count.p;
    a.index = g.d_index.p;
    a.count = g.d_count.p;
    a.n_ch = h->plan.total_ch;
    a.max_rows = g.max_rows;
    a.out_wave = h->d_out_wave.p;
    a.out_iq = h->d_out_iq.p;
    a.rows = g.d_rows.p;
    a.iq_rows = g.d_iq_rows.p;
    a.wave_stride = h->wave_stride;
    a.wave_batch = h->B;
    return a;
}

/* the gate's list and count, the rows the gather reads (airband_hip_set_output_encoding) */
static AudioPackArgs audio_pack_args(const airband_hip_handle* h) {
    const OutputGate& g = h->gate;
    AudioPackArgs a;
    a.index = g.d_index.p;
    a.count = g.d_count.p;
    a.n_rows = 0;
    a.max_rows = g.max_rows;
    a.n_ch = h->plan.total_ch;
    a.src = h->d_out_wave.p;
    a.src_stride = h->wave_stride;
    a.src_pad = AB_OUT_PAD;
    a.audio = g.enc.d_audio.p;
    a.info = g.enc.d_info.p;
    a.wave_batch = h->B;
    a.encoding = g.enc.encoding;
    return a;
}

/* samples of an encoded row: wave_batch, or half of it behind the output decimation (airband_hip_encoded_row_samples) */
static int encoded_row_samples(const airband_hip_handle* h) { return has_decimation(h) ? h->B / 2 : h->B; }

/* the same list, count and source rows, the channels' carried values; k: the step's number (airband_hip_set_output_decimation) */
static AudioDecimateArgs audio_decimate_args(const airband_hip_handle* h, uint32_t k) {
    const OutputGate& g = h->gate;
    AudioDecimateArgs a;
    a.index = g.d_index.p;
    a.count = g.d_count.p;
    a.n_rows = 0;
    a.max_rows = g.max_rows;
    a.n_ch = h->plan.total_ch;
    a.src = h->d_out_wave.p;
    a.src_stride = h->wave_stride;
    a.src_pad = AB_OUT_PAD;
    a.audio = g.enc.d_audio.p;
    a.info = g.enc.d_info.p;
    a.hist = g.enc.dec.d_hist.p;
    a.stamp = g.enc.dec.d_stamp.p;
    a.k = k;
    a.wave_batch = h->B;
    a.encoding = g.enc.encoding;
    return a;
}

/* what the channel spool reads: the output gate's verdicts and the encoder's rows (airband_hip_set_transmission_spool) */
static SpoolSource channel_spool_source(const airband_hip_handle* h) {
    const OutputGate& g = h->gate;
    SpoolSource src;
    src.mask = g.d_mask.p;
    src.block_count = g.d_block_count.p;
    src.audio = g.enc.d_audio.p;
    src.info = g.enc.d_info.p;
    src.n = h->plan.total_ch;
    src.max_rows = g.max_rows;
    src.frames = encoded_row_samples(h);
    src.width = 1;
    return src;
}

/* ---- the spool's host side, over a TransmissionSpool and its source: the channel spool (below) and the mixer spool (driver_mix.cpp) go through these ---- */
/* the spool's own buffers, the source's verdicts, rows and records; k: the step's number */
static SpoolArgs spool_args(const TransmissionSpool& sp, const SpoolSource& src, uint32_t k) {
    SpoolArgs a;
    a.spool = sp.d_spool.p;
    a.chan = sp.d_chan.p;
    a.ctl = sp.d_ctl.p;
    a.close_mask = sp.d_close_mask.p;
    a.app_mask = sp.d_app_mask.p;
    a.close_count = sp.d_close_count.p;
    a.app_count = sp.d_app_count.p;
    a.gate_mask = src.mask;
    a.gate_count = src.block_count;
    a.free_stack = sp.d_free_stack.p;
    a.next = sp.d_next.p;
    a.pool = sp.d_pool.p;
    a.copy_list = sp.d_copy_list.p;
    a.enc_audio = src.audio;
    a.enc_info = src.info;
    a.fin = sp.d_fin.p;
    a.exp_records = sp.d_exp_records.p;
    a.exp_head = sp.d_exp_head.p;
    a.exp_src = sp.d_exp_src.p;
    a.exp_audio = sp.d_exp_audio.p;
    a.n_ch = src.n;
    a.max_rows = src.max_rows;
    a.pool_rows = sp.pool_rows;
    a.export_rows = sp.export_rows;
    a.max_records = sp.max_records;
    a.row_bytes = sp.row_bytes;
    a.wave_batch = src.frames;
    a.min_batches = sp.min_batches;
    a.idle_batches = sp.idle_batches;
    a.max_batches = sp.max_batches;
    a.k = k;
    return a;
}

/* the arguments of a set call, checked before the device is touched: the counts, and the mask resolved against the source's gate bytes (`item`: "channel" / "mixer") */
int airband::spool_check(airband_hip_handle* h, const uint8_t* spool, const std::vector<uint8_t>& gate, const char* item, int64_t pool_rows, int64_t export_rows,
                         int64_t max_records, int32_t max_batches, std::vector<uint8_t>* mask) {
    if (max_batches < 1) return fail(h, AIRBAND_HIP_EINVAL, "max_batches must be at least 1");
    if (export_rows < (int64_t)max_batches + 1) return fail(h, AIRBAND_HIP_EINVAL, "export_rows must be at least max_batches + 1: a collect must be able to take the longest transmission");
    if (max_records < 1) return fail(h, AIRBAND_HIP_EINVAL, "max_records must be at least 1");
    if (pool_rows > 0x7fffffff || export_rows > 0x7fffffff || max_records > 0x7fffffff / 2) return fail(h, AIRBAND_HIP_EINVAL, "pool_rows, export_rows or max_records too large to index");
    mask->assign(gate.size(), 0);
    for (size_t c = 0; c < gate.size(); c++) {
        (*mask)[c] = spool ? (spool[c] ? 1 : 0) : (gate[c] == AIRBAND_GATE_SIGNAL ? 1 : 0);
        if ((*mask)[c] && gate[c] != AIRBAND_GATE_SIGNAL)
            return fail(h, AIRBAND_HIP_EINVAL, std::string("spooled ") + item + " " + std::to_string(c) + " has a gate other than AIRBAND_GATE_SIGNAL");
    }
    return AIRBAND_HIP_OK;
}

/* allocate and initialise: `sp` is built beside what it will belong to and moved in whole by the caller, so a failed allocation leaves the handle as it was.
 * n: items of the source; max_rows: its list's capacity; row_bytes: bytes of one of its rows.  `what` ends with ": " */
int airband::spool_build(airband_hip_handle* h, TransmissionSpool& sp, const std::vector<uint8_t>& mask, int max_rows, size_t row_bytes, int64_t pool_rows,
                         int64_t export_rows, int64_t max_records, int32_t min_batches, int32_t idle_batches, int32_t max_batches, const char* what) {
    const size_t n = mask.size(), nb = (size_t)gate_blocks((int)n), nm = (n + 63) / 64;
    std::vector<int> stack((size_t)pool_rows);
    for (size_t i = 0; i < stack.size(); i++) stack[i] = (int)i;
    SpoolCtl ctl;
    std::memset(&ctl, 0, sizeof(ctl));
    ctl.free_top = (int32_t)pool_rows;
    ctl.room = (int32_t)max_records;
    hipError_t e = upload(sp.d_spool, mask);
    if (e == hipSuccess) e = upload(sp.d_free_stack, stack);
    if (e == hipSuccess) e = sp.d_ctl.alloc(1);
    if (e == hipSuccess) e = hipMemcpy(sp.d_ctl.p, &ctl, sizeof(ctl), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sp.d_chan.alloc_zeroed(n);
    if (e == hipSuccess) e = sp.d_close_mask.alloc_zeroed(nm);
    if (e == hipSuccess) e = sp.d_app_mask.alloc_zeroed(nm);
    if (e == hipSuccess) e = sp.d_close_count.alloc_zeroed(nb);
    if (e == hipSuccess) e = sp.d_app_count.alloc_zeroed(nb);
    if (e == hipSuccess) e = sp.d_next.alloc_zeroed((size_t)pool_rows);
    if (e == hipSuccess) e = sp.d_copy_list.alloc_zeroed(2 * (size_t)max_rows);
    if (e == hipSuccess) e = sp.d_pool.alloc((size_t)pool_rows * row_bytes);
    if (e == hipSuccess) e = sp.d_fin.alloc_zeroed((size_t)max_records);
    if (e == hipSuccess) e = sp.d_exp_records.alloc_zeroed((size_t)max_records);
    if (e == hipSuccess) e = sp.d_exp_head.alloc_zeroed((size_t)max_records);
    if (e == hipSuccess) e = sp.d_exp_src.alloc_zeroed((size_t)export_rows);
    if (e == hipSuccess) e = sp.d_exp_audio.alloc((size_t)export_rows * row_bytes);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr); /* the zeroes are there before a step on another stream reads them */
    if (e != hipSuccess) return alloc_failed(h, e, what);
    sp.pool_rows = (int)pool_rows;
    sp.export_rows = (int)export_rows;
    sp.max_records = (int)max_records;
    sp.row_bytes = (int)row_bytes;
    sp.min_batches = (uint32_t)min_batches;
    sp.idle_batches = (uint32_t)idle_batches;
    sp.max_batches = (uint32_t)max_batches;
    return AIRBAND_HIP_OK;
}

/* one step behind the source's rows on s (tx_spool.hip) */
void airband::spool_step(TransmissionSpool& sp, const SpoolSource& src, hipStream_t s) {
    launch_spool_step(spool_args(sp, src, sp.steps), s);
    sp.steps++;
    sp.steps_total++;
}

int airband::spool_collect(airband_hip_handle* h, const TransmissionSpool& sp, const SpoolSource& src, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting) {
    ON_OWN_STREAM(h, s);
    launch_spool_collect(spool_args(sp, src, sp.steps), s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    /* how much there is is on the device: the counts first, then exactly those records and rows */
    int32_t exp[3] = {0, 0, 0};
    HIP_TRY(h, hipMemcpyAsync(exp, sp.d_ctl.p, sizeof(exp), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (exp[0] < 0 || exp[0] > sp.max_records || exp[1] < 0 || exp[1] > sp.export_rows || exp[2] < 0 || exp[2] > sp.max_records)
        return fail(h, AIRBAND_HIP_ERUNTIME, "transmission spool counts out of range");
    if (records && exp[0]) HIP_TRY(h, hipMemcpyAsync(records, sp.d_exp_records.p, (size_t)exp[0] * sizeof(airband_hip_transmission), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (audio && exp[1]) HIP_TRY(h, hipMemcpyAsync(audio, sp.d_exp_audio.p, (size_t)exp[1] * sp.row_bytes, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (n) *n = exp[0];
    if (n_rows) *n_rows = exp[1];
    if (n_waiting) *n_waiting = exp[2];
    return AIRBAND_HIP_OK;
}

int airband::spool_flush(airband_hip_handle* h, const TransmissionSpool& sp, const SpoolSource& src) {
    ON_OWN_STREAM(h, s);
    launch_spool_flush(spool_args(sp, src, sp.steps), s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    /* a batch (or a step) that ran on a caller's stream: the next one there knows nothing of the handle's stream, so the flush is complete before this returns */
    if (h->ev_last_pending) HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband::spool_counters(airband_hip_handle* h, const TransmissionSpool& sp, airband_hip_spool_counters* out) {
    if (!out) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    ON_OWN_STREAM(h, s);
    SpoolCtl ctl;
    HIP_TRY(h, hipMemcpyAsync(&ctl, sp.d_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    out->steps = sp.steps_total;
    out->open_now = ctl.open_now;
    out->waiting_now = (uint64_t)(ctl.fin_count < 0 ? 0 : ctl.fin_count);
    out->free_rows_now = (uint64_t)(ctl.free_top < 0 ? 0 : ctl.free_top);
    out->finished_total = ctl.finished_total;
    out->dropped_transmissions = ctl.dropped;
    out->rows_stored_total = ctl.rows_stored;
    out->rows_lost_total = ctl.rows_lost;
    return AIRBAND_HIP_OK;
}

void airband::spool_device_views(const TransmissionSpool& sp, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export) {
    if (d_export_audio) *d_export_audio = sp.d_exp_audio.p;
    if (d_export_records) *d_export_records = sp.d_exp_records.p;
    if (d_n_export) *d_n_export = reinterpret_cast<int32_t*>(sp.d_ctl.p); /* SpoolCtl::exp, its first member */
}

static bool audio_encoding_known(int32_t e) { return e == AIRBAND_AUDIO_S16 || e == AIRBAND_AUDIO_ULAW || e == AIRBAND_AUDIO_ALAW; }
static size_t audio_sample_bytes(int e) { return e == AIRBAND_AUDIO_S16 ? 2 : 1; }

/* ---- the RTP stream's host side, over an RtpStream and the source whose rows it frames: the channel stream (below) and the mixer stream (driver_mix.cpp) go
 * through these ---- */
/* k: the step's number; listed: false for the flush step, in which nobody is listed (no mask, no counts) */
static RtpArgs rtp_args(const RtpStream& r, const SpoolSource& src, uint32_t k, bool listed) {
    RtpArgs a;
    a.sources = r.d_sources.p;
    a.state = r.d_state.p;
    a.carry = r.d_carry.p;
    a.ctl = r.d_ctl.p;
    a.plan = r.d_plan.p;
    a.blocks = r.d_blocks.p;
    a.work = r.d_work.p;
    a.gate_mask = listed ? src.mask : nullptr;
    a.gate_count = listed ? src.block_count : nullptr;
    a.enc_audio = src.audio;
    a.records = r.d_records.p;
    a.packets = r.d_packets.p;
    a.n_ch = src.n;
    a.max_rows = src.max_rows;
    a.wave_batch = src.frames;
    a.frame_samples = r.frame_samples;
    a.sample_bytes = r.sample_bytes;
    a.carry_cap = r.carry_cap;
    a.carry_stride = r.carry_stride;
    a.slot_bytes = r.slot_bytes;
    a.max_packets = r.max_packets;
    a.k = k;
    a.width_shift = r.width == 2 ? 1 : 0;
    return a;
}

/* one step behind the source's rows on s (rtp_stream.hip) */
void airband::rtp_step(RtpStream& r, const SpoolSource& src, hipStream_t s) {
    launch_rtp_step(rtp_args(r, src, r.steps, true), r.write_grid, s);
    r.steps++;
    r.steps_total++;
    r.has_result = true;
}

/* the step in which nobody is listed, in stream order behind the steps enqueued so far; not a step: k does not advance */
int airband::rtp_flush(airband_hip_handle* h, RtpStream& r, const SpoolSource& src) {
    ON_OWN_STREAM(h, s);
    launch_rtp_step(rtp_args(r, src, r.steps, false), r.write_grid, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    r.has_result = true;
    /* a batch (or a step) that ran on a caller's stream: the next one there knows nothing of the handle's stream, so the flush is complete before this returns */
    if (h->ev_last_pending) HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

/* the frame length's bounds (the header's): AIRBAND_HIP_OK, or the code with *why set.  width: samples per frame */
static int rtp_frame_check(int32_t encoding, int64_t frame_samples, int64_t wave_batch, int64_t width, const char** why) {
    if (!audio_encoding_known(encoding)) {
        *why = "encoding is not AIRBAND_AUDIO_S16, _ULAW or _ALAW";
        return AIRBAND_HIP_EINVAL;
    }
    if (width != 1 && width != 2) {
        *why = "width is neither 1 nor 2";
        return AIRBAND_HIP_EINVAL;
    }
    *why = "frame_samples must be a multiple of 4 with 40 <= frame_samples <= wave_batch and 12 + frame_samples * width * sample_bytes <= 1472";
    if (frame_samples % 4 || frame_samples < 40 || (wave_batch > 0 && frame_samples > wave_batch)) return AIRBAND_HIP_EBADSIZE;
    if (12 + frame_samples * width * (int64_t)audio_sample_bytes(encoding) > 1472) return AIRBAND_HIP_EBADSIZE;
    return AIRBAND_HIP_OK;
}

static int rtp_slot_bytes(int32_t encoding, int32_t frame_samples, int32_t width) {
    return (int)((12 + (size_t)frame_samples * width * audio_sample_bytes(encoding) + 15) / 16 * 16);
}

int airband::rtp_slot_bytes_checked(int32_t encoding, int32_t frame_samples, int32_t width) {
    const char* why = "";
    const int rc = rtp_frame_check(encoding, frame_samples, 0, width, &why);
    return rc != AIRBAND_HIP_OK ? rc : rtp_slot_bytes(encoding, frame_samples, width);
}

/* the most packets one step can emit: every item a whole row behind the longest carry */
static int64_t rtp_most_packets(const RtpStream& r, const SpoolSource& src) { return (int64_t)src.n * ((r.carry_cap + src.frames) / r.frame_samples); }

/* a set call's arguments checked before the device is touched, then allocate and initialise: `r` is built beside what it will belong to and moved in whole by the
 * caller, so a failed allocation leaves the handle as it was */
int airband::rtp_build(airband_hip_handle* h, RtpStream& r, const airband_hip_rtp_source* sources, const std::vector<uint8_t>& gate, const char* item, int32_t encoding,
                       const SpoolSource& src, int32_t frame_samples, int64_t max_packets, const char* what) {
    const char* why = "";
    int rc = rtp_frame_check(encoding, frame_samples, src.frames, src.width, &why);
    if (rc != AIRBAND_HIP_OK) return fail(h, rc, why);
    const int n = src.n, B = src.frames, F = frame_samples, sb = (int)audio_sample_bytes(encoding), slot = rtp_slot_bytes(encoding, F, src.width);
    int gcd = B, rest = F;
    while (rest) {
        const int t = gcd % rest;
        gcd = rest;
        rest = t;
    }
    const int carry_cap = F - gcd; /* a carry is a multiple of gcd(B, F) below F */
    const int64_t most = (int64_t)n * ((carry_cap + B) / F);
    if (max_packets < 1 || max_packets > 0x7fffffff || most > 0x7fffffff) return fail(h, AIRBAND_HIP_EINVAL, "max_packets must be at least 1, and it and the most packets of a step small enough to index");
    size_t n_streamed = 0;
    for (int c = 0; c < n; c++) {
        if (!sources[c].stream) continue;
        n_streamed++;
        if (sources[c].payload_type > 127) return fail(h, AIRBAND_HIP_EINVAL, std::string("payload_type of ") + item + " " + std::to_string(c) + " is above 127");
        if (gate[c] == AIRBAND_GATE_NEVER) return fail(h, AIRBAND_HIP_EINVAL, std::string("streamed ") + item + " " + std::to_string(c) + " has gate AIRBAND_GATE_NEVER");
    }
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    std::vector<airband_hip_rtp_source> host_src(sources, sources + n);
    std::vector<airband_hip_rtp_state> state((size_t)n);
    std::memset(state.data(), 0, state.size() * sizeof(state[0]));
    for (int c = 0; c < n; c++)
        if (host_src[c].stream) state[c].seq = host_src[c].seq0;
    const size_t carry_stride = (size_t)carry_cap * sb * src.width;
    hipError_t e = upload(r.d_sources, host_src);
    if (e == hipSuccess) e = upload(r.d_state, state);
    if (e == hipSuccess) e = r.d_carry.alloc_zeroed((size_t)n * carry_stride + 4);
    if (e == hipSuccess) e = r.d_ctl.alloc_zeroed(1);
    if (e == hipSuccess) e = r.d_plan.alloc_zeroed((size_t)n);
    if (e == hipSuccess) e = r.d_blocks.alloc_zeroed((size_t)gate_blocks(n));
    if (e == hipSuccess) e = r.d_work.alloc_zeroed((size_t)n);
    if (e == hipSuccess) e = r.d_records.alloc_zeroed((size_t)max_packets);
    if (e == hipSuccess) e = r.d_packets.alloc_zeroed((size_t)max_packets * slot);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr); /* the zeroes are there before a step on another stream reads them */
    if (e != hipSuccess) return alloc_failed(h, e, what);
    r.max_packets = (int)max_packets;
    r.frame_samples = F;
    r.sample_bytes = sb;
    r.slot_bytes = slot;
    r.carry_cap = carry_cap;
    r.carry_stride = (int)carry_stride;
    r.width = src.width;
    r.write_grid = (int)(n_streamed < 1 ? 1 : (n_streamed < 8192 ? n_streamed : 8192));
    return AIRBAND_HIP_OK;
}

/* how many packets there are is on the device: the count first, then exactly those records and slots and the caller's extra, ONE synchronize behind them; only
 * then is the count reported */
int airband::rtp_collect(airband_hip_handle* h, const RtpStream& r, const SpoolSource& src, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets,
                         const void* d_extra, void* extra, size_t extra_bytes) {
    ON_OWN_STREAM(h, s);
    int64_t count = 0;
    int rc = collect_counted<int32_t>(h, &r.d_ctl.p->n_packets, rtp_most_packets(r, src), r.max_packets, "RTP packet count out of range: ", &count, nullptr, nullptr, s);
    if (rc != AIRBAND_HIP_OK) return rc;
    const size_t n = (size_t)(count < r.max_packets ? count : r.max_packets);
    if (records && n) HIP_TRY(h, hipMemcpyAsync(records, r.d_records.p, n * sizeof(airband_hip_rtp_packet), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (packets && n) HIP_TRY(h, hipMemcpyAsync(packets, r.d_packets.p, n * (size_t)r.slot_bytes, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (extra) HIP_TRY(h, hipMemcpyAsync(extra, d_extra, extra_bytes, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (n_packets) *n_packets = count;
    return AIRBAND_HIP_OK;
}

int airband::rtp_state(airband_hip_handle* h, const RtpStream& r, const SpoolSource& src, int64_t first, int64_t n, airband_hip_rtp_state* state, const char* item) {
    if (!state) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (first < 0 || n < 0 || first + n > src.n) return fail(h, AIRBAND_HIP_EINVAL, std::string(item) + " range outside the handle's " + item + "s");
    if (n == 0) return AIRBAND_HIP_OK;
    ON_OWN_STREAM(h, s);
    HIP_TRY(h, hipMemcpyAsync(state, r.d_state.p + first, (size_t)n * sizeof(airband_hip_rtp_state), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband::rtp_counters(airband_hip_handle* h, const RtpStream& r, airband_hip_rtp_counters* out) {
    if (!out) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    ON_OWN_STREAM(h, s);
    RtpCtl ctl;
    HIP_TRY(h, hipMemcpyAsync(&ctl, r.d_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    out->steps = (int64_t)r.steps_total;
    out->packets = (int64_t)ctl.packets;
    out->dropped_packets = (int64_t)ctl.dropped;
    out->octets = (int64_t)ctl.octets;
    out->lost_rows = (int64_t)ctl.lost_rows;
    return AIRBAND_HIP_OK;
}

void airband::rtp_device_views(const RtpStream& r, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state) {
    if (d_n_packets) *d_n_packets = &r.d_ctl.p->n_packets; /* RtpCtl's first member */
    if (d_records) *d_records = r.d_records.p;
    if (d_packets) *d_packets = r.d_packets.p;
    if (d_state) *d_state = r.d_state.p;
}

/* What airband_hip_collect_active() and airband_hip_collect_active_encoded() share.  How many rows there are is on the device: the count first, then exactly those
 * rows -- the channel indices, what `rows(n, s)` enqueues of the call's own arrays, axcindicate of every channel, ONE synchronize.  Only then is the count
 * reported and the batch marked as collected: a caller that sees an error sees neither.  (A HIP_TRY inside `rows` returns from the lambda; its code is checked here.) */
template <class Rows>
static int collect_active_rows(airband_hip_handle* h, int64_t* n_active, int32_t* channel_index, char* axc_all, Rows rows) {
    const OutputGate& g = h->gate;
    ON_OWN_STREAM(h, s);
    int64_t count = 0;
    int rc = collect_counted<int32_t>(h, g.d_count.p, h->plan.total_ch, g.max_rows, "active count out of range: ", &count, nullptr, nullptr, s);
    if (rc != AIRBAND_HIP_OK) return rc;
    const size_t n = (size_t)(count < g.max_rows ? count : g.max_rows);
    if (channel_index && n) HIP_TRY(h, hipMemcpyAsync(channel_index, g.d_index.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    rc = rows(n, s);
    if (rc != AIRBAND_HIP_OK) return rc;
    if (axc_all) HIP_TRY(h, hipMemcpyAsync(axc_all, h->d_out_axc.p, (size_t)h->plan.total_ch, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (n_active) *n_active = count;
    h->results_ready = false;
    return AIRBAND_HIP_OK;
}

/* behind the emit / mixer launches of a gated handle's batch: its active channels and their rows, packed (gate.hip) ... */
void airband::launch_gate_behind_mix(airband_hip_handle* h, hipStream_t s) {
    launch_gate(gate_args(h), s);
    if (has_decimation(h)) launch_audio_decimate(audio_decimate_args(h, ++h->gate.enc.dec.steps), 0, s); /* ... and encoded at half the rate (audio_decimate.hip) */
    else if (has_encoding(h)) launch_audio_pack(audio_pack_args(h), 0, s); /* ... or encoded as they are (audio_pack.hip) */
    if (has_spool(h)) spool_step(h->gate.enc.spool, channel_spool_source(h), s); /* ... and the spool's step of this batch (tx_spool.hip) */
    if (has_rtp(h)) rtp_step(h->gate.enc.rtp, channel_spool_source(h), s);       /* ... and the RTP stream's (rtp_stream.hip): another reader of the same rows */
}

extern "C" {

int airband_hip_set_output_gate(airband_hip_handle* h, const uint8_t* gate, int64_t max_rows) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!gate) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    const Plan& p = h->plan;
    if (max_rows < 1 || max_rows > p.total_ch) return fail(h, AIRBAND_HIP_EINVAL, "max_rows must lie in 1 .. total_channels");
    for (int c = 0; c < p.total_ch; c++)
        if (gate[c] > AIRBAND_GATE_ALWAYS) return fail(h, AIRBAND_HIP_EINVAL, "gate byte of channel " + std::to_string(c) + " is not an AIRBAND_GATE_* value");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the output gate is set before the first batch");
    if (h->B % 4) return fail(h, AIRBAND_HIP_EBADSIZE, "the gather moves four samples per lane: WAVE_BATCH must be a multiple of four");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the handle and moved in whole: a failed allocation leaves the handle as it was */
    OutputGate g;
    g.gate.assign(gate, gate + p.total_ch);
    std::vector<uint8_t> bytes(g.gate);
    for (int c = 0; c < p.total_ch; c++)
        if (!h->dev_enabled[p.cc[c].dev]) bytes[c] |= AB_GATE_OFF; /* dongles that are switched off already */
    const size_t rows = (size_t)max_rows;
    hipError_t e = upload(g.d_gate, bytes);
    if (e == hipSuccess) e = g.d_prev.alloc_zeroed((size_t)p.total_ch);
    if (e == hipSuccess) e = g.d_mask.alloc(((size_t)p.total_ch + 63) / 64);
    if (e == hipSuccess) e = g.d_block_count.alloc((size_t)gate_blocks(p.total_ch));
    if (e == hipSuccess) e = g.d_index.alloc(rows);
    if (e == hipSuccess) e = g.d_count.alloc_zeroed(1);
    if (e == hipSuccess) e = g.d_rows.alloc(rows * h->B);
    if (e == hipSuccess && h->d_out_iq.p) e = g.d_iq_rows.alloc(rows * h->B * 2);
    if (e != hipSuccess) return alloc_failed(h, e, "output gate buffers: ");
    g.max_rows = (int)max_rows;
    h->gate = std::move(g);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_active(airband_hip_handle* h, int64_t* n_active, int32_t* channel_index, float* waveout, float* iq_out, char* axc_all) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const OutputGate& g = h->gate;
    if (!has_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_GATE);
    if (!h->results_ready || h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    return collect_active_rows(h, n_active, channel_index, axc_all, [&](size_t n, hipStream_t s) -> int {
        const size_t B = (size_t)h->B;
        if (waveout && n) HIP_TRY(h, hipMemcpyAsync(waveout, g.d_rows.p, n * B * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        if (iq_out && n) {
            if (g.d_iq_rows.p)
                HIP_TRY(h, hipMemcpyAsync(iq_out, g.d_iq_rows.p, n * B * 2 * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
            else
                std::memset(iq_out, 0, n * B * 2 * sizeof(float));
        }
        return AIRBAND_HIP_OK;
    });
}

int airband_hip_device_active(airband_hip_handle* h, int32_t** d_index, int32_t** d_count, float** d_rows, float** d_iq_rows) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const OutputGate& g = h->gate;
    if (!has_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_GATE);
    if (d_index) *d_index = g.d_index.p;
    if (d_count) *d_count = g.d_count.p;
    if (d_rows) *d_rows = g.d_rows.p;
    if (d_iq_rows) *d_iq_rows = g.d_iq_rows.p;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_output_encoding(airband_hip_handle* h, int32_t encoding) {
    if (!h) return AIRBAND_HIP_EINVAL;
    OutputGate& g = h->gate;
    if (!has_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_GATE);
    if (encoding != AIRBAND_AUDIO_F32 && !audio_encoding_known(encoding)) return fail(h, AIRBAND_HIP_EINVAL, "encoding is not an AIRBAND_AUDIO_* value");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the output encoding is set before the first batch");
    if (h->B % 4) return fail(h, AIRBAND_HIP_EBADSIZE, "the encoder moves four samples per lane: WAVE_BATCH must be a multiple of four");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the gate and moved in whole: a failed allocation leaves the handle as it was */
    OutputEncoding enc;
    if (encoding != AIRBAND_AUDIO_F32) {
        const size_t rows = (size_t)g.max_rows;
        hipError_t e = enc.d_audio.alloc(rows * h->B * audio_sample_bytes(encoding));
        if (e == hipSuccess) e = enc.d_info.alloc(rows);
        if (e != hipSuccess) return alloc_failed(h, e, "output encoding buffers: ");
        enc.encoding = encoding;
    }
    g.enc = std::move(enc);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_active_encoded(airband_hip_handle* h, int64_t* n_active, int32_t* channel_index, void* audio, airband_hip_audio_row* info, char* axc_all) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const OutputGate& g = h->gate;
    if (!has_encoding(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_ENCODING);
    if (!h->results_ready || h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    return collect_active_rows(h, n_active, channel_index, axc_all, [&](size_t n, hipStream_t s) -> int {
        if (audio && n) HIP_TRY(h, hipMemcpyAsync(audio, g.enc.d_audio.p, n * encoded_row_samples(h) * audio_sample_bytes(g.enc.encoding), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        if (info && n) HIP_TRY(h, hipMemcpyAsync(info, g.enc.d_info.p, n * sizeof(airband_hip_audio_row), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        return AIRBAND_HIP_OK;
    });
}

int airband_hip_device_active_encoded(airband_hip_handle* h, void** d_audio, airband_hip_audio_row** d_info) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const OutputGate& g = h->gate;
    if (!has_encoding(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_ENCODING);
    if (d_audio) *d_audio = g.enc.d_audio.p;
    if (d_info) *d_info = g.enc.d_info.p;
    return AIRBAND_HIP_OK;
}

int airband_hip_encode_audio(airband_hip_handle* h, int32_t encoding, const float* rows, int64_t n_rows, void* audio, airband_hip_audio_row* info) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!rows) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (!audio_encoding_known(encoding)) return fail(h, AIRBAND_HIP_EINVAL, "encoding is not AIRBAND_AUDIO_S16, _ULAW or _ALAW");
    if (n_rows < 0 || n_rows > 0x7fffffff / 4) return fail(h, AIRBAND_HIP_EINVAL, "n_rows out of range");
    if (h->B % 4) return fail(h, AIRBAND_HIP_EBADSIZE, "the encoder moves four samples per lane: WAVE_BATCH must be a multiple of four");
    if (n_rows == 0) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* buffers of the call's own, on the null stream: nothing of the handle is read or written */
    const size_t n = (size_t)n_rows, B = (size_t)h->B, row_bytes = B * audio_sample_bytes(encoding);
    DevBuf<float> d_rows;
    DevBuf<uint8_t> d_audio;
    DevBuf<airband_hip_audio_row> d_info;
    hipError_t e = d_rows.alloc(n * B);
    if (e == hipSuccess) e = d_audio.alloc(n * row_bytes);
    if (e == hipSuccess) e = d_info.alloc(n);
    if (e != hipSuccess) return alloc_failed(h, e, "encode_audio buffers: ");
    HIP_TRY(h, hipMemcpy(d_rows.p, rows, n * B * sizeof(float), hipMemcpyHostToDevice), AIRBAND_HIP_ERUNTIME);
    AudioPackArgs a;
    a.index = nullptr;
    a.count = nullptr;
    a.n_rows = (int)n_rows;
    a.max_rows = (int)n_rows;
    a.n_ch = (int)n_rows;
    a.src = d_rows.p;
    a.src_stride = (long)B;
    a.src_pad = 0;
    a.audio = d_audio.p;
    a.info = d_info.p;
    a.wave_batch = h->B;
    a.encoding = encoding;
    launch_audio_pack(a, 0, nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    if (audio) HIP_TRY(h, hipMemcpy(audio, d_audio.p, n * row_bytes, hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    if (info) HIP_TRY(h, hipMemcpy(info, d_info.p, n * sizeof(airband_hip_audio_row), hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(nullptr), AIRBAND_HIP_ERUNTIME); /* the buffers go with this call */
    return AIRBAND_HIP_OK;
}

int airband_hip_set_output_decimation(airband_hip_handle* h, int32_t factor) {
    if (!h) return AIRBAND_HIP_EINVAL;
    OutputGate& g = h->gate;
    if (!has_encoding(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_ENCODING);
    if (factor != 1 && factor != 2) return fail(h, AIRBAND_HIP_EINVAL, "the output decimation's factor is 1 or 2");
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the output decimation is set before the first batch");
    if (factor == 2 && h->B % 8) return fail(h, AIRBAND_HIP_EBADSIZE, "a lane makes four outputs: WAVE_BATCH / 2 must be a multiple of four");
    /* built beside the encoding and moved in whole: a failed allocation leaves the handle as it was */
    OutputDecimation dec;
    if (factor == 2) {
        HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
        hipError_t e = dec.d_hist.alloc_zeroed((size_t)h->plan.total_ch * AUDIO_DECIMATE_HIST);
        if (e == hipSuccess) e = dec.d_stamp.alloc_zeroed((size_t)h->plan.total_ch);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr); /* the zeroes are there before a step on another stream reads them */
        if (e != hipSuccess) return alloc_failed(h, e, "output decimation buffers: ");
        dec.factor = 2;
    }
    g.enc.dec = std::move(dec);
    g.enc.spool = TransmissionSpool(); /* they were sized for rows of the other length */
    g.enc.rtp = RtpStream();
    return AIRBAND_HIP_OK;
}

int airband_hip_encoded_row_samples(const airband_hip_handle* h) {
    if (!h || !has_encoding(h)) return AIRBAND_HIP_EINVAL;
    return encoded_row_samples(h);
}

int airband_hip_decimate_audio(airband_hip_handle* h, int32_t encoding, const float* rows, int64_t n_rows, int16_t* history, void* audio, airband_hip_audio_row* info) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!rows) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (!audio_encoding_known(encoding)) return fail(h, AIRBAND_HIP_EINVAL, "encoding is not AIRBAND_AUDIO_S16, _ULAW or _ALAW");
    if (n_rows < 0 || n_rows > 0x7fffffff / 4) return fail(h, AIRBAND_HIP_EINVAL, "n_rows out of range");
    if (h->B % 8) return fail(h, AIRBAND_HIP_EBADSIZE, "a lane makes four outputs: WAVE_BATCH / 2 must be a multiple of four");
    if (n_rows == 0) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* buffers of the call's own, on the null stream: nothing of the handle is read or written */
    const size_t n = (size_t)n_rows, B = (size_t)h->B, row_bytes = B / 2 * audio_sample_bytes(encoding), hist_bytes = n * AUDIO_DECIMATE_HIST * sizeof(int16_t);
    DevBuf<float> d_rows;
    DevBuf<uint8_t> d_audio;
    DevBuf<airband_hip_audio_row> d_info;
    DevBuf<int16_t> d_hist;
    hipError_t e = d_rows.alloc(n * B);
    if (e == hipSuccess) e = d_audio.alloc(n * row_bytes);
    if (e == hipSuccess) e = d_info.alloc(n);
    if (e == hipSuccess && history) e = d_hist.alloc(n * AUDIO_DECIMATE_HIST);
    if (e != hipSuccess) return alloc_failed(h, e, "decimate_audio buffers: ");
    HIP_TRY(h, hipMemcpy(d_rows.p, rows, n * B * sizeof(float), hipMemcpyHostToDevice), AIRBAND_HIP_ERUNTIME);
    if (history) HIP_TRY(h, hipMemcpy(d_hist.p, history, hist_bytes, hipMemcpyHostToDevice), AIRBAND_HIP_ERUNTIME);
    AudioDecimateArgs a;
    a.index = nullptr;
    a.count = nullptr;
    a.n_rows = (int)n_rows;
    a.max_rows = (int)n_rows;
    a.n_ch = (int)n_rows;
    a.src = d_rows.p;
    a.src_stride = (long)B;
    a.src_pad = 0;
    a.audio = d_audio.p;
    a.info = d_info.p;
    a.hist = history ? d_hist.p : nullptr;
    a.stamp = nullptr;
    a.k = 0;
    a.wave_batch = h->B;
    a.encoding = encoding;
    launch_audio_decimate(a, 0, nullptr);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    if (audio) HIP_TRY(h, hipMemcpy(audio, d_audio.p, n * row_bytes, hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    if (info) HIP_TRY(h, hipMemcpy(info, d_info.p, n * sizeof(airband_hip_audio_row), hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    if (history) HIP_TRY(h, hipMemcpy(history, d_hist.p, hist_bytes, hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(nullptr), AIRBAND_HIP_ERUNTIME); /* the buffers go with this call */
    return AIRBAND_HIP_OK;
}

int airband_hip_set_transmission_spool(airband_hip_handle* h, const uint8_t* spool, int64_t pool_rows, int64_t export_rows, int64_t max_records, int32_t min_batches, int32_t idle_batches, int32_t max_batches) {
    if (!h) return AIRBAND_HIP_EINVAL;
    OutputGate& g = h->gate;
    if (!has_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_GATE);
    if (!has_encoding(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_ENCODING);
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the transmission spool is set before the first batch");
    if (pool_rows < 0 || export_rows < 0 || max_records < 0 || min_batches < 0 || idle_batches < 0) return fail(h, AIRBAND_HIP_EINVAL, "negative count");
    if (pool_rows == 0) { /* removed */
        g.enc.spool = TransmissionSpool();
        return AIRBAND_HIP_OK;
    }
    std::vector<uint8_t> mask;
    int rc = spool_check(h, spool, g.gate, "channel", pool_rows, export_rows, max_records, max_batches, &mask);
    if (rc != AIRBAND_HIP_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* built beside the encoding and moved in whole: a failed allocation leaves the handle as it was */
    TransmissionSpool sp;
    rc = spool_build(h, sp, mask, g.max_rows, (size_t)encoded_row_samples(h) * audio_sample_bytes(g.enc.encoding), pool_rows, export_rows, max_records, min_batches, idle_batches, max_batches,
                     "transmission spool buffers: ");
    if (rc != AIRBAND_HIP_OK) return rc;
    g.enc.spool = std::move(sp);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_transmissions(airband_hip_handle* h, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SPOOL);
    return spool_collect(h, h->gate.enc.spool, channel_spool_source(h), n, records, audio, n_rows, n_waiting);
}

int airband_hip_spool_flush(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SPOOL);
    return spool_flush(h, h->gate.enc.spool, channel_spool_source(h));
}

int airband_hip_spool_counters_get(airband_hip_handle* h, airband_hip_spool_counters* out) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SPOOL);
    return spool_counters(h, h->gate.enc.spool, out);
}

int airband_hip_device_transmission_spool(airband_hip_handle* h, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_spool(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SPOOL);
    spool_device_views(h->gate.enc.spool, d_export_audio, d_export_records, d_n_export);
    return AIRBAND_HIP_OK;
}

int airband_hip_rtp_slot_bytes(int32_t encoding, int32_t frame_samples) { return rtp_slot_bytes_checked(encoding, frame_samples, 1); }

int airband_hip_set_rtp_stream(airband_hip_handle* h, const airband_hip_rtp_source* sources, int32_t frame_samples, int64_t max_packets) {
    if (!h) return AIRBAND_HIP_EINVAL;
    OutputGate& g = h->gate;
    if (!has_gate(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_GATE);
    if (!has_encoding(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_ENCODING);
    if (started(h)) return fail(h, AIRBAND_HIP_EINVAL, "the RTP stream is set before the first batch");
    if (!sources) { /* removed */
        g.enc.rtp = RtpStream();
        return AIRBAND_HIP_OK;
    }
    /* built beside the encoding and moved in whole: a failed allocation leaves the handle as it was */
    RtpStream r;
    const int rc = rtp_build(h, r, sources, g.gate, "channel", g.enc.encoding, channel_spool_source(h), frame_samples, max_packets, "RTP stream buffers: ");
    if (rc != AIRBAND_HIP_OK) return rc;
    g.enc.rtp = std::move(r);
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_rtp_packets(airband_hip_handle* h, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets, char* axc_all) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_RTP);
    if (!h->results_ready || h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    const int rc = rtp_collect(h, h->gate.enc.rtp, channel_spool_source(h), n_packets, records, packets, h->d_out_axc.p, axc_all, (size_t)h->plan.total_ch);
    if (rc != AIRBAND_HIP_OK) return rc;
    h->results_ready = false;
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_rtp_state(airband_hip_handle* h, int64_t first_channel, int64_t n_channels, airband_hip_rtp_state* state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_RTP);
    return rtp_state(h, h->gate.enc.rtp, channel_spool_source(h), first_channel, n_channels, state, "channel");
}

int airband_hip_rtp_counters_get(airband_hip_handle* h, airband_hip_rtp_counters* out) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_RTP);
    return rtp_counters(h, h->gate.enc.rtp, out);
}

int airband_hip_device_rtp_stream(airband_hip_handle* h, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_rtp(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_RTP);
    rtp_device_views(h->gate.enc.rtp, d_n_packets, d_records, d_packets, d_state);
    return AIRBAND_HIP_OK;
}

} /* extern "C" */
