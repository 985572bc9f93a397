/* csrc/handle.h -- private to the host driver (airband_hip.cpp and driver_*.cpp, which include driver.h after it): the handle behind the C ABI and the types
 * that own its HIP objects.
 *
 * Everything the handle holds on the device frees itself when the handle is deleted.  What makes that safe -- nothing of it is still in
 * flight -- is destroy()'s job (airband_hip.cpp), not these destructors'.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h> /* types and prototypes only: librccl.so is loaded on first use (airband_hip_comm_*) */

#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/airband_hip.h"
#include "common.h"
#include "kernels.h" /* ScanCtlList */
#include "params.h"

namespace airband {

/* a HIP object that is released with its owner (move-only); converts to the plain handle where HIP wants one */
template <class H, hipError_t (*Release)(H)>
struct Owned {
    H v = nullptr;
    Owned() = default;
    Owned(Owned&& o) noexcept : v(std::exchange(o.v, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        std::swap(v, o.v); /* what was here goes with o */
        return *this;
    }
    ~Owned() {
        if (v) (void)Release(v);
    }
    operator H() const { return v; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    /* the events that only order streams; created on first use where a handle may never need them */
    hipError_t ensure() { return v ? hipSuccess : hipEventCreateWithFlags(&v, hipEventDisableTiming); }
};

/* device memory, `n` elements at `p` */
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t count) {
        release();
        if (count == 0) return hipSuccess;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    hipError_t alloc_zeroed(size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess || count == 0 ? e : hipMemset(p, 0, count * sizeof(T));
    }
    /* room for `count` elements: what is there stays if it is large enough, its contents do not otherwise */
    hipError_t reserve(size_t count) { return n >= count ? hipSuccess : alloc(count); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

/* pinned host memory */
template <class T>
struct PinnedBuf : Owned<void*, hipHostFree> {
    T* get() const { return static_cast<T*>(v); }
    hipError_t alloc(size_t count) { return hipHostMalloc(&v, count * sizeof(T), hipHostMallocDefault); }
};

/* what airband_hip_set_mixers() wired up: replaced as a whole, an empty one is a handle without mixers */
struct MixerWiring {
    std::vector<int> pos;         /* connection index (order of airband_hip_set_mixers) -> position in the per-mixer grouped arrays */
    std::vector<int> chan_host;   /* grouped external channel indices, for re-enabling an input */
    std::vector<uint8_t> user_on; /* by position: airband_hip_mixer_enable_input()'s say; an input counts while this AND its dongle are on */
    int n_mixers = 0;
    int n_runs = 0;
    DevBuf<int> d_chan, d_first, d_run_first, d_run_mixer, d_first_run;
    DevBuf<float> d_run_left, d_run_right;
    DevBuf<uint8_t> d_run_signal;
    DevBuf<float> d_ml, d_mr, d_left, d_right;
    DevBuf<uint8_t> d_stereo, d_signal;
};

/* what airband_hip_set_transmission_spool() set up, a part of the encoding whose rows it keeps -- or airband_hip_set_mixer_spool(), a part of the mixer gate whose
 * rows it keeps: replaced as a whole, gone with the encoding (and so with the gate) or with the mixer gate, one without pool_rows is an encoding or a mixer gate
 * without a spool (nothing allocated, nothing launched).  Declared in front of both owners: a member's type has to be complete */
struct TransmissionSpool {
    int pool_rows = 0;         /* 0 = no spool */
    int export_rows = 0, max_records = 0, row_bytes = 0;
    uint32_t min_batches = 0, idle_batches = 0, max_batches = 0;
    uint32_t steps = 0;        /* steps enqueued so far: the next step's k */
    uint64_t steps_total = 0;
    DevBuf<uint8_t> d_spool, d_pool, d_exp_audio;
    DevBuf<SpoolChan> d_chan;
    DevBuf<SpoolCtl> d_ctl;
    DevBuf<unsigned long long> d_close_mask, d_app_mask;
    DevBuf<int> d_close_count, d_app_count, d_free_stack, d_next, d_copy_list, d_exp_head, d_exp_src;
    DevBuf<airband_hip_transmission> d_fin, d_exp_records;
};

/* what airband_hip_set_rtp_stream() set up, a part of the encoding whose rows it frames -- or airband_hip_set_mixer_rtp_stream(), a part of the mixer gate whose
 * rows it frames: replaced as a whole, gone with the encoding (and so with the gate) or with the mixer gate, one without max_packets is an encoding or a mixer
 * gate without a stream (nothing allocated, nothing launched).  Declared in front of both owners: a member's type has to be complete */
struct RtpStream {
    int max_packets = 0;       /* 0 = no stream */
    int frame_samples = 0, sample_bytes = 0, slot_bytes = 0, carry_cap = 0, carry_stride = 0; /* frame_samples and carry_cap count frames */
    int width = 1;             /* samples per frame: the source's when the stream was set */
    int write_grid = 0;        /* workgroups of the write pass: min(streamed channels, one per wavefront slot of the GPU) */
    uint32_t steps = 0;        /* steps enqueued so far: the next step's k */
    uint64_t steps_total = 0;
    bool has_result = false;   /* a step or a flush has been enqueued.  Read by the MIXER stream's collect only (its EAGAIN); the channel stream's result is tied to the batch (results_ready) */
    DevBuf<airband_hip_rtp_source> d_sources;
    DevBuf<airband_hip_rtp_state> d_state;
    DevBuf<uint8_t> d_carry, d_packets;
    DevBuf<RtpCtl> d_ctl;
    DevBuf<RtpPlan> d_plan;
    DevBuf<RtpBlock> d_blocks;
    DevBuf<RtpWork> d_work;
    DevBuf<airband_hip_rtp_packet> d_records;
};

/* what airband_hip_set_mixer_gate() set up over the wiring's sums: replaced as a whole, dropped by airband_hip_set_mixers(), one without max_rows is a handle
 * without a mixer gate (nothing allocated, nothing launched).  An encoded gate holds d_audio / d_info and no d_rows, a float gate d_rows alone. */
struct MixerGate {
    int max_rows = 0;          /* capacity of the packed buffers; 0 = no mixer gate */
    int encoding = AIRBAND_AUDIO_F32;
    int width = 1;             /* samples per frame: 2 with AIRBAND_MIXER_GATE_STEREO */
    bool manual = false;       /* AIRBAND_MIXER_GATE_MANUAL_STEP: the host enqueues the step */
    bool stepped = false;      /* a step has been enqueued: there is something to collect */
    DevBuf<uint8_t> d_gate, d_prev;
    DevBuf<unsigned long long> d_mask;
    DevBuf<int> d_block_count, d_index, d_count;
    DevBuf<float> d_rows;      /* [max_rows][width * wave_batch] */
    DevBuf<uint8_t> d_audio;   /* [max_rows][width * wave_batch] bytes, or int16 for S16 */
    DevBuf<airband_hip_audio_row> d_info;
    std::vector<uint8_t> gate; /* the caller's bytes: a spooled mixer must be AIRBAND_GATE_SIGNAL */
    TransmissionSpool spool;   /* airband_hip_set_mixer_spool: an encoded gate's, gone with the gate */
    RtpStream rtp;             /* airband_hip_set_mixer_rtp_stream: an encoded gate's, gone with the gate */
};

/* what airband_hip_set_output_encoding() set up, a part of the gate whose list it reads: replaced as a whole, gone with the gate, AIRBAND_AUDIO_F32 is a gate
 * without an encoding (nothing allocated, nothing launched) */
/* what airband_hip_set_output_decimation() set up, a part of the encoding whose rows it halves: the channels' carried filter values and the step that listed
 * each last.  The encoding's d_audio keeps its size; its rows are wave_batch / 2 samples long then */
struct OutputDecimation {
    int factor = 1;            /* 1 = none (nothing allocated, audio_pack.hip encodes); 2: audio_decimate.hip in its place, rows of wave_batch / 2 */
    uint32_t steps = 0;        /* steps enqueued so far; step numbers start at 1 (kernels.h: AudioDecimateArgs::k) */
    DevBuf<int16_t> d_hist;    /* [total_ch][46] */
    DevBuf<uint32_t> d_stamp;  /* [total_ch] */
};

struct OutputEncoding {
    TransmissionSpool spool;
    RtpStream rtp;
    OutputDecimation dec;      /* airband_hip_set_output_decimation: replaced as a whole, gone with the encoding */
    int encoding = AIRBAND_AUDIO_F32;
    DevBuf<uint8_t> d_audio; /* [max_rows][wave_batch] bytes, or int16 for S16 */
    DevBuf<airband_hip_audio_row> d_info;
};

/* what airband_hip_set_output_gate() set up: replaced as a whole, one without max_rows is a handle without a gate (nothing allocated, nothing launched) */
struct OutputGate {
    OutputEncoding enc;
    int max_rows = 0;          /* capacity of the packed buffers; 0 = no gate */
    std::vector<uint8_t> gate; /* the caller's bytes (the device copy also carries AB_GATE_OFF for the channels of dongles switched off) */
    DevBuf<uint8_t> d_gate, d_prev;
    DevBuf<unsigned long long> d_mask;
    DevBuf<int> d_block_count, d_index, d_count;
    DevBuf<float> d_rows, d_iq_rows;
};

/* what airband_hip_set_scan_control() set up (the handle's scan members, below): replaced as a whole, one without idle_batches is a handle whose lists the host
 * hops (nothing allocated, nothing launched).  While it is there the host's scan_cur / scan_held / scan_latch and the per-frequency bits of cc_slots[slot].flags of
 * the scan slots are NOT kept: the entry a slot holds is on the device (d_state, d_sw), and switching control off refreshes them. */
struct ScanControl {
    int idle_batches = 0;      /* 0 = no scan control */
    int dwell_batches = 1, max_records = 0;
    uint32_t batch = 0;        /* the control's batch number of the next launch */
    std::vector<int> list_of;  /* by control index (ascending dongle order): the list in plan.scan */
    std::vector<int> ctl_of;   /* by list in plan.scan: its control index */
    DevBuf<ScanCtlList> d_lists;
    DevBuf<airband_hip_scan_state> d_state;
    DevBuf<airband_hip_scan_event> d_stage, d_events;
    DevBuf<int> d_stage_n, d_sw, d_count;
};

/* The band outputs, like the gated ones above, are declared innermost first: each is a member of the one it reads (follow in watch in survey in scope), so that
 * replacing an outer one drops what hangs on it, and a member's type has to be complete.  Read them from BandScope upwards. */
/* what airband_hip_set_band_follow() set up, a part of the watch whose tables it reads: replaced as a whole, gone with the watch, one without max_changes is a
 * watch without a follow (nothing allocated, nothing launched).  A handle with followers never runs ahead: the scope keeps ONE set, and so does this. */
struct BandFollow {
    int max_changes = 0;       /* capacity of the fleet's list; 0 = no follow */
    int cap = 0;               /* a row's staging slice: the most followers of a row + max_tracks */
    DevBuf<int> d_range, d_slot, d_home; /* by scope row: first follower and count; by follower (prepare order): demod slot, home bin */
    DevBuf<airband_hip_band_follower> d_followers;
    DevBuf<airband_hip_band_follow_row> d_rows;
    DevBuf<airband_hip_band_follow_change> d_changes, d_stage; /* d_stage: the rows' changes between the two kernels of one launch */
    DevBuf<int> d_count;
};

/* what airband_hip_set_band_watch() set up, a part of the survey it reads: replaced as a whole, gone with the survey, one without max_tracks is a survey
 * without a watch (nothing allocated, nothing launched).  Its results follow the survey's: the same sets, the same `cur`; the tables a batch starts from are
 * the other set's where there are two. */
struct BandWatch {
    int max_tracks = 0;        /* 0 = no watch */
    BandFollow follow;
    int match_bins = 0, confirm_hits = 0, release_misses = 0, max_events = 0;
    uint32_t batch = 0;        /* the watch batch number of the next launch */
    DevBuf<airband_hip_band_track> d_tracks[2];
    DevBuf<airband_hip_band_watch_row> d_rows[2];
    DevBuf<airband_hip_band_event> d_events[2], d_stage; /* d_stage: the rows' events between the two kernels of one launch */
    DevBuf<int> d_count[2];
};

/* what airband_hip_set_band_survey() set up, a part of the scope it reads: replaced as a whole, gone with the scope, one without max_peaks is a scope without
 * a survey (nothing allocated, nothing launched).  Its results follow the scope's rows: the same sets, the same `cur`. */
struct BandSurvey {
    int max_peaks = 0;         /* 0 = no survey */
    BandWatch watch;
    uint32_t trace = 0;        /* the one AIRBAND_SCOPE_* bit whose rows are surveyed */
    int rank = 0, guard_bins = 0;
    float ratio = 0.0f;
    DevBuf<int> d_bin_first, d_bins; /* by scope row: the prepare-time bins of the dongle's channels */
    DevBuf<airband_hip_band_summary> d_summary[2];
    DevBuf<airband_hip_band_peak> d_peaks[2];
};

/* what airband_hip_set_band_scope() set up: replaced as a whole, one without windows is a handle without a scope (nothing allocated, nothing launched, no
 * stream, no event).  Handles whose next stage 1 may run before the last batch's results are collected (pipelined, run-ahead) keep TWO sets of rows: the
 * scope of front batch k goes to a set of its own and becomes the current one when the batch's back half is enqueued, as the batch's results do. */
struct BandScope {
    int windows = 0;           /* windows per batch; 0 = no scope */
    BandSurvey survey;
    uint32_t traces = 0;       /* AIRBAND_SCOPE_* */
    int n_rows = 0, n_sets = 1;
    std::vector<int> row_of_dev;
    DevBuf<int> d_row_of_dev, d_dev_of_row;
    DevBuf<float> d_mean[2], d_peak[2];
    Stream stream;             /* beside stage 1, forked where it starts and joined behind it */
    Event ev_fork, ev_done;
    uint64_t launches = 0;     /* scope launches so far: launch n writes set n % n_sets */
    int set_of_front[2] = {-1, -1}; /* by front batch k & 1: the set its scope went to, -1 for a batch without input (airband_hip_process_bins) */
    int cur = 0;               /* the set of the batch whose results are current */
};

}  // namespace airband

struct airband_hip_handle {
    airband::Plan plan;
    uint32_t flags = 0;
    int hip_device = 0;
    airband::Stream stream;
    airband::Stream side[3]; /* fused demod kinds run beside the CTCSS chain */
    airband::Event fork_ev[4];
    /* AIRBAND_HIP_FLAG_PIPELINE: stage 1 of batch k runs on `front` while stage 2 of batch k-1 runs on `stream` */
    bool pipeline = false;
    /* The default schedule of airband_hip_process_device(h, ..., NULL) on a handle without AFC channels and scan lists (and without FLAG_PIPELINE): stage 1 of batch k
     * on `front`, stage 2 of batch k on `stream` behind it IN THE SAME CALL.  Batches enqueued back to back then run stage 1 (k+1) beside stage 2 (k) -- the GPU
     * schedule of the pipelined mode with no lag on the host.  AIRBAND_HIP_RUN_AHEAD=0 at prepare: off (one-batch rings, everything on one stream). */
    bool run_ahead = false;
    bool serialise_next = false;   /* something the next batch's stage 1 depends on was enqueued on `stream` (or a batch ran elsewhere): its front waits for the stream's tail, once */
    uint64_t ahead_batches = 0;    /* batches that took the run-ahead path (airband_hip_schedule_info) */
    airband::Stream front;
    airband::Event ev_in, ev_back, ev_wait, front_done[2];
    airband::Event back_done[2];   /* run-ahead: recorded on `stream` behind the back half of batch k, at [k & 1] -- stage 1 of batch k+2 overwrites the ring rows it read */
    hipStream_t last_stream = nullptr; /* stream the last sequential batch ran on (the caller's or ours; not owned) */
    airband::Event ev_spec[2]; /* AFC on the matrix-core channelizer: the last hop's spectrum runs on a side stream beside stage 1 (fork, done) */
    airband::Event ev_last;    /* recorded behind every batch that ran on a CALLER's stream: collect / read_* / synchronize / release
                                  order themselves behind it (the caller's stream itself may be gone by then, our event is not) */
    bool ev_last_pending = false;
    int row0_front = 0;            /* ring row of the batch stage 1 writes next (== row0 when not pipelined) */
    uint64_t front_batches = 0;    /* batches whose stage 1 has been enqueued */
    /* per-stage GPU time: a pool of event sets (one per process call) harvested lazily, so that nobody has to
     * synchronise inside a run to read timings */
    static constexpr int EV_POOL = 16;
    airband::Event evp[EV_POOL][5];   /* stage 1 begin / end, stage 2 begin, demod end, batch end */
    uint8_t evp_state[EV_POOL] = {0}; /* bit 0: stage-1 pair recorded, bit 1: stage-2 pair recorded */
    double t_sum[4] = {0, 0, 0, 0};
    int64_t t_n[2] = {0, 0};          /* harvested stage-1 / stage-2 pairs */
    float t_last[4] = {0, 0, 0, 0};
    bool timings_valid = false;
    std::string error;

    /* geometry */
    int B = 0, R = 0, N = 0;
    int n_slots = 0;      /* demod slots: channels sorted by kind, every kind padded to whole 64-slot blocks */
    std::vector<int> slot_to_ext, ext_to_slot;
    int kind_first_block[AB_KIND_COUNT] = {0}, kind_n_blocks[AB_KIND_COUNT] = {0};
    int64_t hop_bytes = 0, first_batch_bytes = 0, batch_bytes = 0, lookahead_bytes = 0;
    int row0 = 0;
    int wave_stride = 0;   /* floats between two channels' rows of d_out_wave */
    uint64_t batches_done = 0;
    bool results_ready = false;
    uint64_t overruns = 0;

    /* device memory */
    airband::DevBuf<DevConst> d_dev;
    airband::DevBuf<ChanConst> d_cc;
    airband::DevBuf<ChanState> d_cs;
    airband::DevBuf<int> d_slot_to_ext, d_ext_to_slot;
    airband::DevBuf<uint8_t> d_block_kind;
    airband::DevBuf<float> d_window, d_sin, d_cos, d_twiddle;
    airband::DevBuf<float> d_window_dec; /* fft_size >= 1024: the window de-interleaved by sample index mod (fft_size / 512), for the decimated wavefront FFT (channelizer_fft.hip) */
    airband::DevBuf<float> d_mag, d_sqbuf, d_ct_coeff, d_ct_q;
    airband::DevBuf<float2> d_iq, d_iq_out, d_ct_af;
    airband::DevBuf<unsigned long long> d_ct_mask;
    int ct_first_block = 0, ct_n_blocks = 0, ct_pk_pitch = 0;
    /* AIRBAND_HIP_FLAG_REGROUP: the batch's slot order (demod.hip, "regrouping") */
    bool regroup = false;
    int regroup_mode = 1;              /* 1: channels sorted inside lockstep workgroups; 2: line groups sorted, wavefronts free-running (demod.hip) */
    airband::DevBuf<int> d_perm;       /* regroup mode 3: the batch's slot permutation (demod.hip, regroup_perm_kernel) */
    airband::DevBuf<uint8_t> d_sq_key; /* split kinds: the front kernel's note for the back kernel (had audio in this batch) */
    airband::DevBuf<uint8_t> d_trace;
    airband::DevBuf<float> d_out_wave, d_out_iq;
    airband::DevBuf<uint8_t> d_out_axc;
    airband::DevBuf<airband_hip_channel_stats> d_stats;
    airband::DevBuf<float> d_tmp_wavein, d_tmp_iqin, d_spectrum;
    bool any_afc = false, afc_spectrum_valid = false; /* process_bins() has no spectrum: AFC is skipped there */
    airband::DevBuf<uint8_t> d_tmp_trace;
    int ct_stride = 0;
    /* matrix-core channelizer */
    bool use_f32 = false;          /* CF32 dongles on the float32 matrix pipe (channelizer_f32.hip) */
    bool use_f32_wide = false;     /* use_f32, staged by channelizer_f32_wide.hip (AIRBAND_HIP_FLAG_WIDE_HOPS and a hop beyond f32_supported()'s limits) */
    airband::DevBuf<float> d_ftab;
    bool use_dft = false;
    bool use_wide = false;         /* use_dft, staged by channelizer_dft_wide.hip (AIRBAND_HIP_FLAG_WIDE_HOPS and a hop beyond dft_supported()'s limits) */
    std::string chan_reason;       /* airband_hip_channelizer_reason(): set on every branch of prep_channelizer() */
    airband::DevBuf<int> d_item_dev, d_item_group, d_item_bset, d_item_private, d_item_home; /* d_item_bset: what stage 1 reads (the re-tune kernel switches AFC groups between their home and private tables) */
    airband::DevBuf<int8_t> d_bfrag;
    airband::DevBuf<double> d_bcorr;
    airband::DevBuf<float> d_dft_partial; /* fft_size 8192: partial sums between the two passes of eight window pieces */
    airband::DevBuf<int> d_bset_bin;      /* [n_bsets][8] bin each coefficient column pair is built for (AFC re-tunes private tables on the device) */
    const void* last_iq = nullptr; /* input of the batch stage 1 ran last (AFC looks at its last hop once stage 2 has decided) */
    size_t last_iq_stride = 0;
    int last_n_hops = 0;

    /* host-ring path: one PINNED circular buffer per dongle (row d of h_ring, ring_cap bytes).  submit() copies the caller's bytes
     * straight into it -- the only CPU copy on the way -- and may be called for DIFFERENT dongles from several threads at once;
     * process() ships a batch with (at most two, where the span wraps) strided DMA transfers on a copy stream into one of two
     * device staging buffers while the kernels of the previous batch still read the other. */
    airband::PinnedBuf<uint8_t> ring_mem;                  /* the rings' memory; everybody reads it through h_ring */
    std::atomic<uint8_t*> h_ring{nullptr};                 /* published (release) by host_path_init() once ring_cap / stage_stride / the staging buffers exist; read (acquire) by submit() and process() */
    int64_t ring_cap = 0;                                  /* bytes per dongle */
    std::unique_ptr<std::atomic<uint64_t>[]> ring_wr;      /* per dongle: stream bytes accepted so far */
    uint64_t ring_rd = 0;                                  /* stream position of the next batch (common to all dongles: they advance in lockstep) */
    std::atomic<uint64_t> ring_free{0};                    /* stream position up to which the ring may be overwritten (lags ring_rd by the batch in flight) */
    airband::DevBuf<uint8_t> d_stage2[2];
    int64_t stage_stride = 0;
    airband::Stream h2d;
    airband::Event ev_h2d[2], ev_stage_read[2];
    uint64_t host_batches = 0;
    std::mutex host_init_lock;

    /* dongles switched off with airband_hip_device_enable(): skipped by the availability rule and by both stages */
    std::unique_ptr<std::atomic<uint8_t>[]> dev_enabled; /* (atomic: a feeder thread's submit() reads its dongle's flag while the demod thread switches it) */
    int n_enabled = 0;
    std::vector<ChanConst> cc_slots; /* host copy of d_cc (slot order): the VALID bit of a dongle's slots follows its enable state */

    airband::MixerWiring mix;
    airband::MixerGate mix_gate; /* airband_hip_set_mixer_gate: gone with the wiring it reads */
    airband::OutputGate gate;
    airband::BandScope scope;

    /* the mixer exchange (airband_hip_comm_*): this handle's rank in an RCCL communicator over the GPUs that hold the other dongles */
    ncclComm_t comm = nullptr;
    airband::Event ev_peer; /* airband_hip_add_mixers: "src's batch is done" for dst's stream */

    /* scan-mode devices (airband_hip_prepare_scan, scan_bank.h): nothing of this exists on a handle without scan lists */
    std::vector<int> scan_of_dev;      /* device -> its list in plan.scan, -1 */
    std::vector<int> scan_cur;         /* by list: the entry airband_hip_set_freq_index() put in force */
    std::vector<int> scan_latch[2];    /* by list: the entry of front batch k, at [k & 1] (stage 2 of a pipelined batch runs during the next call) */
    int scan_first_row[2] = {0, 0};    /* the ring rows stage 1 of front batch k produced: [first_row, first_row + n_rows) */
    int scan_n_rows[2] = {0, 0};
    std::vector<int> scan_held;        /* by list: the entry the slot holds once every exchange enqueued so far has run */
    airband::DevBuf<ChanConst> d_bank_cc;
    airband::DevBuf<ChanState> d_bank_cs;
    airband::DevBuf<float> d_bank_sq;
    airband::DevBuf<uint32_t> d_scan_mask; /* [AB_CS_DWORDS] ChanState masks, then [AB_CC_DWORDS] ChanConst masks */
    airband::DevBuf<int> d_switch[2];      /* the batch's switch list (slot, entry parked, entry brought in), two in flight */
    airband::PinnedBuf<int> h_switch[2];   /* pinned staging of the lists */
    airband::Event ev_switch[2];
    bool switch_used[2] = {false, false};
    int switch_buf = 0;
    airband::DevBuf<int> d_scan_mix_slots; /* slots of lists that mix AM and NFM entries (scan_mag_kernel) */
    airband::ScanControl scan_ctl;         /* airband_hip_set_scan_control: the GPU hops the lists */
    airband::DevBuf<ChanConst> d_fs_cc; /* airband_hip_freq_stats: one composed image, its stats row */
    airband::DevBuf<ChanState> d_fs_cs;
    airband::DevBuf<airband_hip_channel_stats> d_fs_stats;
    airband::DevBuf<int> d_fs_zero;

    /* synthetic dongles */
    airband::DevBuf<int16_t> d_sin_tab;
    airband::DevBuf<long long> d_carriers;
    int n_carriers = 0, noise_q8 = 0;
    int sig_n_plans = 1;            /* airband_hip_set_signal_plan_shift */
    unsigned sig_shift_step = 0;
};
