/* csrc/airband_hip.cpp -- the C ABI of libairband_hip.so (see include/airband_hip.h) and the host-side batch
 * driver: what demodulate() does around its two inner loops (reference: src/rtl_airband.cpp:359-400 input
 * accounting, :494/:649-669 batch hand-off), restated for "all dongles, one batch at a time" on one HIP stream.
 *
 * There is NO CPU fallback in this library: every data-path entry point needs the HIP device the handle was
 * prepared on and fails with AIRBAND_HIP_ENODEV / AIRBAND_HIP_ERUNTIME otherwise.
 *
 * Here: prepare, the batch path, the host ring, collect / read_* / timings, the signal generator; the optional outputs and the mixers: driver_*.cpp (driver.h).
 */
#include "driver.h"

/* upper bound for the int8 coefficient tables of a handle -- one per distinct group of eight bins plus one per AFC group; past it prepare() picks the wavefront-FFT
 * channelizer (override for tests) */
#ifndef AB_PRIVATE_TABLE_BUDGET
#define AB_PRIVATE_TABLE_BUDGET ((size_t)8 << 30)
#endif

/* upper bound for the float coefficient tables (CF32 dongles on the float32 matrix pipe) of a handle, host-built: 512 MiB = 8 192 distinct channel plans at fft 512 */
#ifndef AB_F32_TABLE_BUDGET
#define AB_F32_TABLE_BUDGET ((size_t)512 << 20)
#endif

using namespace airband;

thread_local std::string airband::g_prepare_error;

namespace {

/* Everything in flight must be done before the handle's memory goes away (the handle's members free themselves, handle.h): a batch enqueued on a
 * caller's stream, the front stream of a pipelined handle, the forked demod streams, the copy stream of the host ring. */
void destroy(airband_hip_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->hip_device);
    (void)airband_hip_comm_destroy(h);
    if (h->ev_last && h->ev_last_pending) (void)hipEventSynchronize(h->ev_last);
    if (h->front) (void)hipStreamSynchronize(h->front);
    for (auto& st : h->side)
        if (st) (void)hipStreamSynchronize(st);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->h2d) (void)hipStreamSynchronize(h->h2d);
    if (h->scope.stream) (void)hipStreamSynchronize(h->scope.stream);
    delete h;
}

/* airband_hip_prepare_scan() holds the handle it is building in one of these: every failure exit releases it the way airband_hip_release() would */
using HandlePtr = std::unique_ptr<airband_hip_handle, void (*)(airband_hip_handle*)>;

/* Per-stage GPU times: every batch records into its own event set; finished sets are folded into running sums here. */
void harvest_timings(airband_hip_handle* h, bool wait) {
    for (int i = 0; i < airband_hip_handle::EV_POOL; i++) {
        if (h->evp_state[i] != 3) continue;
        const Event* e = h->evp[i];
        if (wait) {
            if (hipEventSynchronize(e[4]) != hipSuccess || hipEventSynchronize(e[1]) != hipSuccess) continue;
        } else if (hipEventQuery(e[4]) != hipSuccess || hipEventQuery(e[1]) != hipSuccess) {
            continue;
        }
        float a = 0, b = 0, c = 0;
        if (hipEventElapsedTime(&a, e[0], e[1]) == hipSuccess && hipEventElapsedTime(&b, e[2], e[3]) == hipSuccess && hipEventElapsedTime(&c, e[3], e[4]) == hipSuccess) {
            h->t_last[0] = a; h->t_last[1] = b; h->t_last[2] = c; h->t_last[3] = a + b + c;
            for (int k = 0; k < 4; k++) h->t_sum[k] += h->t_last[k];
            h->t_n[0]++;
            h->timings_valid = true;
        }
        h->evp_state[i] = 0;
    }
}

Event* event_set(airband_hip_handle* h, uint64_t batch, int half) {
    const int i = (int)(batch % airband_hip_handle::EV_POOL);
    if (half == 0 && h->evp_state[i] != 0) { /* the pool wrapped around a set nobody has read yet */
        harvest_timings(h, true);
        h->evp_state[i] = 0;
    }
    h->evp_state[i] |= (uint8_t)(1u << half);
    return h->evp[i];
}

void launch_retune_tables(airband_hip_handle* h, hipStream_t s, int epoch) {
    RetuneArgs ra;
    ra.cc = h->d_cc.p;
    ra.cs = h->d_cs.p;
    ra.dev = h->d_dev.p;
    ra.ext_to_slot = h->d_ext_to_slot.p;
    ra.item_dev = h->d_item_dev.p;
    ra.item_group = h->d_item_group.p;
    ra.item_bset = h->d_item_bset.p;
    ra.item_private = h->d_item_private.p;
    ra.item_home = h->d_item_home.p;
    ra.bset_bin = h->d_bset_bin.p;
    ra.bfrag = h->d_bfrag.p;
    ra.corr = h->d_bcorr.p;
    ra.ftab = h->use_f32 ? h->d_ftab.p : nullptr;
    ra.window = h->d_window.p;
    ra.n_items = (int)h->plan.item_dev.size();
    ra.fft_size = h->plan.fft_size;
    ra.n_shared = h->plan.n_shared_bsets;
    ra.moved_epoch = h->d_bset_bin.p + (size_t)h->plan.n_bsets * 8; /* one more int behind the table */
    ra.epoch = epoch;
    launch_retune(ra, s);
}

/* the first batch also produces the AGC_EXTRA lead-in hops (waveend starts at 0, src/config.cpp:805) */
FrontRows front_rows(const airband_hip_handle* h) {
    const bool first = h->front_batches == 0;
    return {first ? 0 : AB_AGC_EXTRA, first ? h->B + AB_AGC_EXTRA : h->B};
}

/* what ChannelizerArgs, DftArgs and F32Args have in common: the input spans, the constants, the rings and the rows to produce in them */
template <class Args>
void fill_front_args(Args& a, const airband_hip_handle* h, const void* d_iq, size_t stride_bytes, int row0, FrontRows r) {
    a.iq = (const uint8_t*)d_iq;
    a.iq_stride = (long)stride_bytes;
    a.dev = h->d_dev.p;
    a.cc = h->d_cc.p;
    a.ext_to_slot = h->d_ext_to_slot.p;
    a.mag = h->d_mag.p;
    a.iq_bins = h->d_iq.p;
    a.row0 = row0;
    a.ring_rows = h->R;
    a.first_row = r.first_row;
    a.n_hops = r.n_hops;
}

/* the wavefront FFT: a batch (spectrum_only 0: last_spectrum is null on a handle without AFC channels), or one hop's spectrum alone */
ChannelizerArgs fft_args(const airband_hip_handle* h, const void* d_iq, size_t stride_bytes, int row0, FrontRows r, int spectrum_only) {
    const Plan& p = h->plan;
    ChannelizerArgs ca;
    fill_front_args(ca, h, d_iq, stride_bytes, row0, r);
    ca.cs = h->d_cs.p;
    ca.window = h->d_window.p;
    ca.window_dec = h->d_window_dec.p;
    ca.twiddle = reinterpret_cast<const float2*>(h->d_twiddle.p);
    ca.last_spectrum = h->d_spectrum.p;
    ca.n_dev = p.n_dev;
    ca.fft_log = p.fft_log;
    ca.hop_samples = p.dev[0].hop_samples;
    ca.bytes_per_sample = p.dev[0].bytes_per_sample;
    ca.sfmt = p.dev[0].sfmt;
    ca.scale = p.dev[0].scale;
    ca.max_ch = p.max_ch;
    ca.spectrum_only = spectrum_only;
    return ca;
}

F32Args f32_args(const airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r) {
    const Plan& p = h->plan;
    F32Args a;
    fill_front_args(a, h, d_iq, stride_bytes, h->row0_front, r);
    a.item_dev = h->d_item_dev.p;
    a.item_group = h->d_item_group.p;
    a.item_bset = h->d_item_bset.p;
    a.btab = h->d_ftab.p;
    a.n_items = (int)p.item_dev.size();
    a.fft_size = p.fft_size;
    a.hop_bytes = (int)h->hop_bytes;
    a.pad = f32_pad_bytes(p.dev[0].hop_samples);
    a.lds_per_buf = f32_lds_per_buf(p.fft_size, p.dev[0].hop_samples);
    a.seg = 0;
    a.n_seg = 1;
    a.partial = reinterpret_cast<float4*>(h->d_dft_partial.p);
    /* enough workgroups to fill 256 CUs x 2 even with few dongles: split each dongle's tiles */
    const int tiles = (a.n_hops + 15) / 16 + 1;
    int splits = (2048 + a.n_items - 1) / a.n_items;
    if (splits > tiles / 4) splits = tiles / 4;
    if (splits < 1) splits = 1;
    a.splits = splits;
    return a;
}

DftArgs dft_args(const airband_hip_handle* h, const void* d_iq, size_t stride_bytes, FrontRows r) {
    const Plan& p = h->plan;
    DftArgs a;
    fill_front_args(a, h, d_iq, stride_bytes, h->row0_front, r);
    a.item_dev = h->d_item_dev.p;
    a.item_group = h->d_item_group.p;
    a.item_bset = h->d_item_bset.p;
    a.bfrag = h->d_bfrag.p;
    a.corr = h->d_bcorr.p;
    /* table units -> sample units: u8 (b - 127.5) / 127.5; s8 i / 128; CS16 x / fullscale (the kernel multiplies by the dongle's 1 / fullscale) */
    a.unscale = p.dev[0].sfmt == AIRBAND_SFMT_S16 ? p.b_unscale * 127.5 : p.dev[0].sfmt == AIRBAND_SFMT_S8 ? p.b_unscale * 127.5 / 128.0 : p.b_unscale;
    a.sfmt = p.dev[0].sfmt;
    a.edge_hi_zero = p.b_edge_hi_zero ? 1 : 0;
    a.n_dev = p.n_dev;
    a.n_items = (int)p.item_dev.size();
    a.fft_size = p.fft_size;
    a.hop_bytes = (int)h->hop_bytes;
    /* the whole window is staged, also when it is worked on in pieces of 512 samples -- up to eight of them per launch (fft_size 8192: two passes) */
    const int np_total = p.fft_size > 512 ? p.fft_size / 512 : 1, np = np_total > 8 ? 8 : np_total;
    const int win_bytes = 2 * p.fft_size * p.dev[0].bytes_per_sample / np_total * np;
    a.partial = reinterpret_cast<float4*>(h->d_dft_partial.p);
    if (h->use_wide) { /* channelizer_dft_wide.hip: a staging step is one tile of 16 rows, two buffers */
        const int wb = win_bytes / np;
        a.lds_per_buf = wide_image_bytes(wb, np, dft_wide_plan(p.fft_size, (int)h->hop_bytes, p.dev[0].sfmt, nullptr, nullptr));
        a.nbuf = 2;
        a.sub = 1;
    } else {
        a.lds_per_buf = dft_lds_per_buf((int)h->hop_bytes, win_bytes, np);
        a.nbuf = dft_nbuf((int)h->hop_bytes, win_bytes, np);
        a.sub = dft_sub((int)h->hop_bytes, win_bytes, np);
    }
    /* Pipelined and run-ahead handles (stage 1 of this batch runs beside stage 2 of the batch before): eight channelizer wavefronts of ~250 registers ARE a CU's register file, and
     * stage-2 wavefronts then only get onto a CU when one of them retires.  Held to FIVE per CU (it loses ~5 % alone: 7 and 6 per CU cost nothing, 4 cost 12 %,
     * profiles/r06_occupancy/) the channelizer leaves three SIMDs a wavefront's worth of registers each: configs[2] 14.05 ms sequential, 13.77 pipelined as before,
     * 13.05 like this (13.5 / 14.0 at 4 / 6 per CU; profiles/r06_pipelined/).  The LDS it asks for and never touches is what holds it there. */
    a.extra_lds = 0;
    if (deep_rings(h) && np_total == 1) {
        const int used = a.nbuf * a.lds_per_buf, want = 28 * 1024; /* 160 KiB / 28 KiB = 5 */
        if (used < want) a.extra_lds = want - used;
    }
    /* enough waves to fill 256 CUs x 8 waves even with few dongles: split each dongle's tiles */
    const int steps = ((a.n_hops + 15) / 16 + 1 + a.sub - 1) / a.sub;
    int splits = (8192 + a.n_items - 1) / a.n_items;
    if (splits > steps / 4) splits = steps / 4;
    if (splits < 1) splits = 1;
    a.splits = splits;
    return a;
}

/* Matrix-core handles with AFC channels: the full spectrum of the batch's LAST hop, for the dongles that have one (one wavefront FFT per such dongle per
 * batch -- afc.finalize(dev, i, fftout) runs once per batch on the output of its last FFT, src/rtl_airband.cpp:626-630).  It depends on the input only, so
 * it is computed on a side stream BESIDE stage 1 (behind the previous batch's AFC, which read the buffer it overwrites) and joined in front of afc_kernel
 * (run_back_half). */
int launch_last_hop_spectrum(airband_hip_handle* h, hipStream_t s) {
    for (auto& e : h->ev_spec) HIP_TRY(h, e.ensure(), AIRBAND_HIP_ENODEV);
    (void)hipEventRecord(h->ev_spec[0], s);
    (void)hipStreamWaitEvent(h->side[0], h->ev_spec[0], 0);
    const uint8_t* last_hop = (const uint8_t*)h->last_iq + (size_t)(h->last_n_hops - 1) * (size_t)h->hop_bytes;
    launch_channelizer_fft(fft_args(h, last_hop, h->last_iq_stride, 0, FrontRows{0, 1}, 1), h->side[0]);
    (void)hipEventRecord(h->ev_spec[1], h->side[0]);
    return AIRBAND_HIP_OK;
}

/* stage 1 of front batch front_batches is in its stream: latch its scan entries, move on to the next batch's ring rows */
void front_enqueued(airband_hip_handle* h, int first_row, int n_rows) {
    scan_latch(h, h->front_batches, first_row, n_rows);
    h->row0_front = (h->row0_front + h->B) % h->R;
    h->front_batches++;
}

/* stage 2 + emit (+ mixers, + the output gate) of the batch whose stage-1 rows are already in the rings */
int run_back_half(airband_hip_handle* h, hipStream_t s) {
    const Event* ev = event_set(h, h->batches_done, 1);
    /* the band scope of this batch (computed beside its stage 1, which s is behind) is the current one from here on; a batch without input leaves it alone */
    if (h->scope.windows > 0 && h->scope.set_of_front[h->batches_done & 1] >= 0) h->scope.cur = h->scope.set_of_front[h->batches_done & 1];
    (void)hipEventRecord(ev[2], s);
    DemodArgs da;
    da.cc = h->d_cc.p;
    da.cs = h->d_cs.p;
    da.mag = h->d_mag.p;
    da.iq = h->d_iq.p;
    da.out_wave = h->d_out_wave.p; /* row starts; the kernels skip AB_OUT_PAD themselves */
    da.out_axc = h->d_out_axc.p;
    da.slot_to_ext = h->d_slot_to_ext.p;
    da.wave_stride = h->wave_stride;
    da.tail_copy = h->batches_done > 0 ? 1 : 0; /* the consumer's tail copy (src/output.cpp:920) happens after it has read a batch */
    da.iq_out = h->d_iq_out.p;
    da.sqbuf = h->d_sqbuf.p;
    da.ct_coeff = h->d_ct_coeff.p;
    da.ct_q = h->d_ct_q.p;
    da.trace = (h->flags & AIRBAND_HIP_FLAG_TRACE_SQUELCH) ? h->d_trace.p : nullptr;
    da.ct_pk_first_block = h->kind_first_block[AB_KIND_NFM_CTCSS];
    da.ct_pk_n_blocks = h->kind_n_blocks[AB_KIND_NFM_CTCSS];
    da.ct_gen_first_block = h->kind_first_block[AB_KIND_GENERIC];
    da.ct_gen_n_blocks = h->kind_n_blocks[AB_KIND_GENERIC];
    da.ct_pk_pitch = h->ct_pk_pitch;
    da.ct_ap = reinterpret_cast<unsigned*>(h->d_ct_af.p);                                                       /* one-word rows first ... */
    da.ct_af = h->d_ct_af.p + (size_t)da.ct_pk_n_blocks * AB_SLOT_BLOCK * h->ct_pk_pitch / 2;                   /* ... then the pairs of the generic kind */
    da.ct_mask = h->d_ct_mask.p;
    da.ct_first_block = h->ct_first_block;
    da.ct_n_blocks = h->ct_n_blocks;
    da.sin_lut = h->d_sin.p;
    da.cos_lut = h->d_cos.p;
    da.ct_stride = h->ct_stride;
    da.n_slots = h->n_slots;
    da.wave_batch = h->B;
    da.row0 = h->row0;
    da.ring_rows = h->R;
    da.regroup = h->regroup ? h->regroup_mode : 0;
    da.sq_key = h->d_sq_key.p;
    da.perm = (h->regroup && h->regroup_mode == 3) ? h->d_perm.p : nullptr;
    if (!h->plan.scan.empty()) {
        const int rc = scan_before_demod(h, s);
        if (rc != AIRBAND_HIP_OK) return rc;
    }
    hipStream_t side[3] = {h->side[0], h->side[1], h->side[2]};
    hipEvent_t fork_ev[4] = {h->fork_ev[0], h->fork_ev[1], h->fork_ev[2], h->fork_ev[3]};
    launch_demod(da, h->kind_first_block, h->kind_n_blocks, s, (h->flags & AIRBAND_HIP_FLAG_SERIAL_DEMOD) ? nullptr : side, fork_ev);
    /* What moves bins between this batch and the next, behind the demod kernels (they read and write ChanState) on their stream: AFC, and the band follow of a batch
     * that had a scope (a batch without input leaves the follow as it is).  Both stamp ONE epoch; the re-tune kernel runs once behind them. */
    const bool afc = h->any_afc && h->afc_spectrum_valid;
    const bool follow = h->scope.windows > 0 && h->scope.survey.watch.follow.max_changes > 0 && h->scope.set_of_front[h->batches_done & 1] >= 0;
    if (afc || follow) {
        const bool tables = h->use_dft || h->use_f32; /* the matrix-core channelizers: a channel's bin is baked into its coefficient columns */
        const int epoch = (int)(h->batches_done % 0x7fffffff) + 1; /* never 0: that is the start-up build's */
        int* const moved_epoch = tables ? h->d_bset_bin.p + (size_t)h->plan.n_bsets * 8 : nullptr;
        if (afc) { /* afc.finalize(), src/rtl_airband.cpp:626-630: may turn '*' into '<' / '>' */
            if (tables) (void)hipStreamWaitEvent(s, h->ev_spec[1], 0); /* the last hop's spectrum, computed beside stage 1 */
            launch_afc(h->d_cc.p, h->d_cs.p, h->d_spectrum.p, h->N, h->n_slots, moved_epoch, epoch, s);
        }
        if (follow) launch_follow_behind_demod(h, moved_epoch, epoch, s);
        if (tables) launch_retune_tables(h, s, epoch); /* the next batch's stage 1 reads the moved channels' new columns */
        if (afc) launch_axc(h->d_cc.p, h->d_cs.p, h->d_slot_to_ext.p, h->d_out_axc.p, h->n_slots, s);
    }
    (void)hipEventRecord(ev[3], s);
    if (h->d_out_iq.p) { /* handles with has_iq_outputs channels: raw I/Q rows -> channel-major */
        EmitArgs ea;
        ea.iq_out = h->d_iq_out.p;
        ea.slot_to_ext = h->d_slot_to_ext.p;
        ea.out_iq = h->d_out_iq.p;
        ea.n_slots = h->n_slots;
        ea.wave_batch = h->B;
        launch_emit_iq(ea, s);
    }
    if (h->mix.n_mixers > 0) launch_mix(mix_args(h), s);
    if (has_gate(h)) launch_gate_behind_mix(h, s); /* the batch's active channels and their rows packed, encoded, spooled (driver_gate.cpp) */
    if (has_mixer_gate(h) && !h->mix_gate.manual) launch_mixer_gate_step(h, s); /* the batch's active mixers and their rows packed (driver_mix.cpp); a manual gate's step is the host's to enqueue, behind its exchange */
    if (has_scan_control(h)) launch_scan_control_behind_demod(h, s); /* the lists' hops for the next batch, from this batch's axcindicate (AFC's verdict included) */
    (void)hipEventRecord(ev[4], s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("kernel launch: ") + hipGetErrorString(e));
    /* rotate the rings: this batch's last AGC_EXTRA rows become the next batch's carry */
    h->row0 = (h->row0 + h->B) % h->R;
    /* run-ahead: everything of this batch that reads the rings (the raw-I/Q emit and the mixer sums included) lies in front of this mark */
    if (h->run_ahead && s == h->stream) (void)hipEventRecord(h->back_done[h->batches_done & 1], s);
    h->batches_done++;
    if (h->results_ready) h->overruns++; /* like dev->output_overrun_count (src/rtl_airband.cpp:649-654) */
    h->results_ready = true;
    harvest_timings(h, false);
    return AIRBAND_HIP_OK;
}

/* ---- airband_hip_prepare_scan() step by step, in the order it calls them ------------------------------------------------------------- */

int prep_streams(airband_hip_handle* h) {
    HIP_TRY(PREPARING, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    int prio_lo = 0, prio_hi = 0; /* numerically lower = more urgent */
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    HIP_TRY(PREPARING, hipStreamCreateWithPriority(&h->stream.v, hipStreamNonBlocking, prio_hi), AIRBAND_HIP_ENODEV);
    for (auto& set : h->evp)
        for (auto& e : set) HIP_TRY(PREPARING, hipEventCreate(&e.v), AIRBAND_HIP_ENODEV);
    if (deep_rings(h)) {
        HIP_TRY(PREPARING, hipStreamCreateWithFlags(&h->front.v, hipStreamNonBlocking), AIRBAND_HIP_ENODEV);
        HIP_TRY(PREPARING, h->ev_in.ensure(), AIRBAND_HIP_ENODEV);
        HIP_TRY(PREPARING, h->ev_back.ensure(), AIRBAND_HIP_ENODEV);
        for (auto& e : h->front_done) HIP_TRY(PREPARING, e.ensure(), AIRBAND_HIP_ENODEV);
        if (h->run_ahead)
            for (auto& e : h->back_done) HIP_TRY(PREPARING, e.ensure(), AIRBAND_HIP_ENODEV);
    }
    for (auto& e : h->fork_ev) HIP_TRY(PREPARING, e.ensure(), AIRBAND_HIP_ENODEV);
    for (auto& st : h->side) HIP_TRY(PREPARING, hipStreamCreateWithPriority(&st.v, hipStreamNonBlocking, prio_lo), AIRBAND_HIP_ENODEV);
    return AIRBAND_HIP_OK;
}

int kind_of(const ChanConst& c) {
    if (c.flags & AB_F_IQ_OUT) return AB_KIND_GENERIC;
    const bool nfm = c.flags & AB_F_NFM, raw = c.flags & AB_F_RAW_IQ, lp = c.flags & AB_F_LOWPASS, ct = c.flags & AB_F_CTCSS;
    if (!nfm) return (!raw && !ct) ? AB_KIND_AM : AB_KIND_GENERIC;
    if (ct && lp) return AB_KIND_GENERIC;
    return ct ? AB_KIND_NFM_CTCSS : lp ? AB_KIND_NFM_LOWPASS : AB_KIND_NFM;
}

/* the demod kind of every channel (external index) */
std::vector<int> channel_kinds(const Plan& p) {
    std::vector<int> kind_ext(p.total_ch);
    for (int e = 0; e < p.total_ch; e++) kind_ext[e] = kind_of(p.cc[e]);
    /* a scan channel's kind holds for every entry of its list: their common kind, else the generic one.  NFM + lowpass becomes generic too when the
     * list has more than one entry: that kind recomputes the squelch's delay line from the channel's wavein carry (squelch_fsm.h, SqShadow), which
     * after a switch belongs to another frequency; the generic kind keeps the line, and the line is banked per entry */
    for (const ScanList& sl : p.scan) {
        int k = kind_of(p.scan_cc[sl.first_entry]);
        for (int f = 1; f < sl.n; f++)
            if (kind_of(p.scan_cc[sl.first_entry + f]) != k) k = AB_KIND_GENERIC;
        if (k == AB_KIND_NFM_LOWPASS && sl.n > 1) k = AB_KIND_GENERIC;
        kind_ext[sl.ext] = k;
    }
    return kind_ext;
}

/* demod slots (pure host): sort the channels by demod kind so that a 64-lane wavefront runs ONE code path (AM, NFM,
 * NFM+lowpass, NFM+CTCSS, everything else); kinds start on 64-slot block boundaries.  Leaves the slot images in h->cc_slots / cs_slots. */
void prep_slots(airband_hip_handle* h, std::vector<ChanState>& cs_slots, std::vector<uint8_t>& block_kind) {
    const Plan& p = h->plan;
    std::vector<ChanConst>& cc_slots = h->cc_slots;
    h->ext_to_slot.assign(p.total_ch, -1);
    const std::vector<int> kind_ext = channel_kinds(p);
    /* A switching scan channel gets a 64-slot block of its own.  The demod kernels hold the squelch's sample_count_ and delay-line cursors in scalar
     * registers (squelch_fsm.h, sq_load: "the same on every channel"), which is true of channels that run every batch, but a list entry counts only
     * the batches it was active in: at WAVE_BATCH 1 000 (= 8 mod 16) two entries' noise-floor sweeps fall 8 samples apart.  Alone in its wavefront
     * the channel's counts are uniform again.  The cost is ring space for 63 idle slots per scan channel. */
    std::vector<uint8_t> isolated(p.total_ch, 0);
    for (const ScanList& sl : p.scan)
        if (sl.n > 1) isolated[sl.ext] = 1;
    ChanConst pad_c;
    ChanState pad_s;
    std::memset(&pad_c, 0, sizeof(pad_c));
    std::memset(&pad_s, 0, sizeof(pad_s));
    pad_c.ct_slot = -1;
    pad_s.axc = ' ';
    auto pad_block = [&]() {
        while (cc_slots.size() % AB_SLOT_BLOCK) {
            h->slot_to_ext.push_back(-1);
            cc_slots.push_back(pad_c);
            cs_slots.push_back(pad_s);
        }
    };
    for (int k = 0; k < AB_KIND_COUNT; k++) {
        bool any = false;
        for (int pass = 0; pass < 2; pass++) /* the kind's channels, then its isolated scan channels, one block each */
            for (int e = 0; e < p.total_ch; e++) {
                if (kind_ext[e] != k || isolated[e] != pass) continue;
                any = true;
                if (pass) pad_block();
                h->ext_to_slot[e] = (int)cc_slots.size();
                h->slot_to_ext.push_back(e);
                cc_slots.push_back(p.cc[e]);
                cs_slots.push_back(p.cs0[e]);
            }
        if (!any) continue;
        pad_block();
        h->kind_first_block[k] = (int)block_kind.size();
        while (block_kind.size() < cc_slots.size() / AB_SLOT_BLOCK) block_kind.push_back((uint8_t)k);
        h->kind_n_blocks[k] = (int)block_kind.size() - h->kind_first_block[k];
    }
    h->n_slots = (int)cc_slots.size();
}

void prep_geometry(airband_hip_handle* h) {
    const Plan& p = h->plan;
    h->B = p.wave_batch;
    /* ring rows, whole 16-row tiles: one batch plus its AGC_EXTRA carry -- or two batches deep when stage 1 of the next batch
     * is written while stage 2 still reads this one */
    h->R = ((deep_rings(h) ? 2 : 1) * p.wave_batch + AB_AGC_EXTRA + 15) / 16 * 16; /* whole 16-hop MFMA tiles (a multiple of AB_TILE_ROWS too) */
    h->N = p.fft_size;
    h->hop_bytes = 2LL * p.dev[0].bytes_per_sample * p.dev[0].hop_samples;
    h->first_batch_bytes = h->hop_bytes * (h->B + AB_AGC_EXTRA);
    h->batch_bytes = h->hop_bytes * h->B;
    h->lookahead_bytes = 2LL * p.dev[0].bytes_per_sample * p.fft_size - h->hop_bytes;
    if (h->lookahead_bytes < 0) h->lookahead_bytes = 0;
    /* hops that are not multiples of 16 bytes (2.4 MS/s): the channelizer stages whole 16-byte pieces, the piece holding the span's last
     * byte included -- make batch + look-ahead a whole number of pieces so that callers size (and fill) their spans accordingly */
    h->lookahead_bytes += (16 - (h->batch_bytes + h->lookahead_bytes) % 16) % 16;
}

int prep_constants(airband_hip_handle* h, const std::vector<ChanState>& cs_slots, const std::vector<uint8_t>& block_kind) {
    const Plan& p = h->plan;
    HIP_TRY(PREPARING, upload(h->d_dev, p.dev), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_cc, h->cc_slots), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_cs, cs_slots), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_slot_to_ext, h->slot_to_ext), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_ext_to_slot, h->ext_to_slot), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_block_kind, block_kind), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_window, p.window), AIRBAND_HIP_ENOMEM);
    if (p.fft_size >= 1024) { /* row n2 = the window at samples n2, n2 + M, n2 + 2 M, ... (M = fft_size / 512): what transform n2 of a decimated FFT multiplies by, contiguous */
        const int M = p.fft_size / 512;
        std::vector<float> dec((size_t)p.fft_size);
        for (int n = 0; n < p.fft_size; n++) dec[(size_t)(n % M) * 512 + n / M] = p.window[n];
        HIP_TRY(PREPARING, upload(h->d_window_dec, dec), AIRBAND_HIP_ENOMEM);
    }
    HIP_TRY(PREPARING, upload(h->d_sin, p.sin_lut), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_twiddle, p.twiddle), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_cos, p.cos_lut), AIRBAND_HIP_ENOMEM);
    /* CTCSS tables: [ct_slot][detector][tone] coefficients and [ct_slot][detector][q1|q2][tone] Goertzel state, so
     * that the 52 tone lanes of demod phase 2 read one contiguous run */
    const int n_ct = (int)p.tones.size();
    h->ct_stride = n_ct;
    std::vector<float> coeff((size_t)(n_ct > 0 ? n_ct : 1) * 2 * AB_MAX_TONES, 0.0f);
    for (int s = 0; s < n_ct; s++)
        for (int k = 0; k < 2; k++)
            for (int t = 0; t < p.tones[s].n[k]; t++) coeff[((size_t)s * 2 + k) * AB_MAX_TONES + t] = p.tones[s].coeff[k][t];
    HIP_TRY(PREPARING, upload(h->d_ct_coeff, coeff), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_ct_q.alloc_zeroed((size_t)(n_ct > 0 ? n_ct : 1) * 4 * AB_MAX_TONES), AIRBAND_HIP_ENOMEM);
    return AIRBAND_HIP_OK;
}

/* the rings, with the reference's config-time prefill of the lead-in (src/config.cpp:313-316), and the hand-off buffers of the split kinds */
int prep_rings(airband_hip_handle* h) {
    const size_t ring = (size_t)h->R * h->n_slots; /* blocked: [n_slots/64][R][64] */
    HIP_TRY(PREPARING, h->d_mag.alloc(ring), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_iq.alloc_zeroed(ring), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_iq_out.alloc_zeroed((size_t)h->B * h->n_slots), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_sqbuf.alloc_zeroed((size_t)AB_SQ_BUF * h->n_slots), AIRBAND_HIP_ENOMEM);
    const float lead_in = 20.0f; /* wavein[0 .. AGC_EXTRA) = 20.0f, src/config.cpp:313-316 (as a 32-bit pattern: no host copy of the rings, 4 GB at 65 536 dongles) */
    int bits;
    std::memcpy(&bits, &lead_in, sizeof(bits));
    HIP_TRY(PREPARING, hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(h->d_mag.p), bits, ring), AIRBAND_HIP_ENOMEM);
    /* hand-off buffers of the split kinds (NFM+CTCSS and generic are adjacent in slot order) */
    h->ct_n_blocks = h->kind_n_blocks[AB_KIND_NFM_CTCSS] + h->kind_n_blocks[AB_KIND_GENERIC];
    h->ct_first_block = h->kind_n_blocks[AB_KIND_NFM_CTCSS] ? h->kind_first_block[AB_KIND_NFM_CTCSS] : h->kind_first_block[AB_KIND_GENERIC];
    if (h->ct_n_blocks > 0) {
        /* one 32-bit word per sample for the NFM + CTCSS kind (rows padded to whole 128-byte lines), (audio, flags) pairs for the generic kind */
        h->ct_pk_pitch = (h->B + 31) / 32 * 32;
        HIP_TRY(PREPARING, h->d_ct_af.alloc((size_t)h->kind_n_blocks[AB_KIND_NFM_CTCSS] * AB_SLOT_BLOCK * h->ct_pk_pitch / 2 + (size_t)h->kind_n_blocks[AB_KIND_GENERIC] * AB_SLOT_BLOCK * h->B),
                AIRBAND_HIP_ENOMEM);
        HIP_TRY(PREPARING, h->d_ct_mask.alloc((size_t)h->ct_n_blocks * (h->B / 50) * AB_SLOT_BLOCK), AIRBAND_HIP_ENOMEM);
    }
    return AIRBAND_HIP_OK;
}

/* regrouped stage 2 (demod.hip, "regrouping") */
int prep_regroup(airband_hip_handle* h) {
    /* Default (neither flag, no environment override): by residency.  A regrouped workgroup's wavefronts of closed channels spend most of the batch waiting at the
     * lockstep barriers -- without using an issue slot, but holding their registers.  While ALL of a handle's lane-per-channel wavefronts are resident at once (about
     * four to six per SIMD) that costs nothing and the 22 % of vector instructions regrouping removes are time (32 768 dongles x 8 mixed channels: stage 2 3.42 ->
     * 3.02 ms; 49 152: 4.53 -> 4.33); past that the waiting wavefronts keep the next round's out (65 536: 5.8 -> 6.05), and a chip that is not full is bound by ONE
     * wavefront's dependent chain, which regrouping does not shorten (<= 16 384: 2.48 -> 2.54) -- profiles/r06_experiments.md D. */
    int n_lane_blocks = 0;
    for (int k = 0; k < AB_KIND_COUNT; k++) n_lane_blocks += h->kind_n_blocks[k];
    int cus = 0, cur_dev = 0;
    (void)hipGetDevice(&cur_dev);
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cur_dev) != hipSuccess || cus <= 0) cus = 256;
    const double waves_per_simd = (double)n_lane_blocks / (4.0 * cus);
    const bool by_residency = waves_per_simd >= 2.75 && waves_per_simd <= 6.25;
    const char* e = getenv("AIRBAND_HIP_REGROUP");
    h->regroup = e && *e ? (*e != '0') : (h->flags & AIRBAND_HIP_FLAG_REGROUP) ? true : (h->flags & AIRBAND_HIP_FLAG_NO_REGROUP) ? false : by_residency;
    /* regrouping deals a workgroup's slots out among its wavefronts: it would put isolated scan channels (prep_slots) back into one wavefront */
    for (const ScanList& sl : h->plan.scan)
        if (sl.n > 1) h->regroup = false;
    h->regroup_mode = (e && *e == '2') ? 2 : (e && *e == '3') ? 3 : 1;
    if (h->regroup && h->regroup_mode == 3) HIP_TRY(PREPARING, h->d_perm.alloc((size_t)h->n_slots), AIRBAND_HIP_ENOMEM);
    if (h->regroup || h->ct_n_blocks > 0) { /* the front kernel's note per channel: had audio / went CLOSED in this batch (tone kernel; regrouped back kernel) */
        HIP_TRY(PREPARING, h->d_sq_key.alloc_zeroed((size_t)h->n_slots), AIRBAND_HIP_ENOMEM);
    }
    return AIRBAND_HIP_OK;
}

int prep_results(airband_hip_handle* h) {
    const Plan& p = h->plan;
    if (h->flags & AIRBAND_HIP_FLAG_TRACE_SQUELCH) HIP_TRY(PREPARING, h->d_trace.alloc_zeroed((size_t)h->B * h->n_slots), AIRBAND_HIP_ENOMEM);
    /* channel->waveout rows (src/rtl_airband.h:230): [AGC_EXTRA tail of the previous batch][WAVE_BATCH]; the consumer reads the first
     * WAVE_BATCH entries.  Config-time prefill of the lead-in as in src/config.cpp:313-316 (waveout[0..AGC_EXTRA) = 0.5). */
    h->wave_stride = (AB_OUT_PAD + AB_AGC_EXTRA + h->B + AB_OUT_RUN - 1) / AB_OUT_RUN * AB_OUT_RUN; /* whole 128-byte lines per row */
    HIP_TRY(PREPARING, h->d_out_wave.alloc_zeroed((size_t)p.total_ch * h->wave_stride), AIRBAND_HIP_ENOMEM);
    /* the lead-in columns, a few thousand rows per strided copy (not a host image of every row: 4.5 GB at 65 536 dongles) */
    const int chunk = p.total_ch < 4096 ? p.total_ch : 4096;
    const std::vector<float> lead((size_t)chunk * AB_AGC_EXTRA, 0.5f);
    for (int c = 0; c < p.total_ch; c += chunk) {
        const int rows = p.total_ch - c < chunk ? p.total_ch - c : chunk;
        HIP_TRY(PREPARING, hipMemcpy2D(h->d_out_wave.p + (size_t)c * h->wave_stride + AB_OUT_PAD, (size_t)h->wave_stride * sizeof(float), lead.data(), AB_AGC_EXTRA * sizeof(float),
                                       AB_AGC_EXTRA * sizeof(float), (size_t)rows, hipMemcpyHostToDevice),
                AIRBAND_HIP_ENOMEM);
    }
    HIP_TRY(PREPARING, h->d_out_axc.alloc((size_t)p.total_ch), AIRBAND_HIP_ENOMEM);
    bool any_iq_out = false;
    for (const ChanConst& c : p.cc) any_iq_out |= (c.flags & AB_F_IQ_OUT) != 0;
    if (any_iq_out) HIP_TRY(PREPARING, h->d_out_iq.alloc_zeroed((size_t)p.total_ch * h->B * 2), AIRBAND_HIP_ENOMEM);
    return AIRBAND_HIP_OK;
}

/* the work items of the matrix-core channelizers */
int upload_work_items(airband_hip_handle* h) {
    const Plan& p = h->plan;
    HIP_TRY(PREPARING, upload(h->d_item_dev, p.item_dev), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_item_group, p.item_group), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_item_bset, p.item_home), AIRBAND_HIP_ENOMEM); /* every channel starts on its base bin */
    return AIRBAND_HIP_OK;
}

/* ... and what the re-tune kernel needs beside them to switch a group with an AFC channel between its home and its private table */
int upload_retune_items(airband_hip_handle* h) {
    const Plan& p = h->plan;
    HIP_TRY(PREPARING, upload(h->d_item_private, p.item_bset), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_item_home, p.item_home), AIRBAND_HIP_ENOMEM);
    std::vector<int> with_epoch(p.bset_bins);
    with_epoch.push_back(0); /* the "last moved in batch" stamp: 0 = the start-up build */
    HIP_TRY(PREPARING, upload(h->d_bset_bin, with_epoch), AIRBAND_HIP_ENOMEM);
    return AIRBAND_HIP_OK;
}

/* the int8 matrix-core channelizer, unless its tables are past the budget (use_dft is cleared then) */
int prep_dft_tables(airband_hip_handle* h) {
    const Plan& p = h->plan;
    build_dft_tables(h->plan, false);
    /* One table per DISTINCT group of eight bins (shared between the work items that have it: a fleet of identical dongles has one, a fleet in which every
     * device_t derives its own bins -- src/config.cpp:666-667 -- as many as it has groups) plus one private table per group with an AFC channel.  Bounded by
     * their bytes alone (65 536 tables are 3.2 GB at fft 512, ~51 GB at fft 8192); past the budget the handle runs on the wavefront FFT.  Round 6: a COUNT used to
     * stand here (more than 4 096 distinct plans -> wavefront FFT, 7x slower), which contradicted the private tables of the AFC path right beside it. */
    const int np_t = p.fft_size > 512 ? p.fft_size / 512 : 1;
    const size_t tab_bytes = (size_t)3 * (p.fft_size > 512 ? 16 : p.fft_size / 32) * 64 * 16 * np_t;
    if ((size_t)p.n_bsets * tab_bytes > AB_PRIVATE_TABLE_BUDGET) {
        h->use_dft = false;
        return AIRBAND_HIP_OK;
    }
    int rc = upload_work_items(h);
    if (rc == AIRBAND_HIP_OK) rc = upload_retune_items(h);
    if (rc != AIRBAND_HIP_OK) return rc;
    /* the host has built the shared tables; the private ones (groups with an AFC channel) follow them, zeroed, and are built by the
     * re-tune kernel right here: every column of theirs still stands at bin -1 */
    HIP_TRY(PREPARING, h->d_bfrag.alloc_zeroed((size_t)p.n_bsets * tab_bytes), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_bcorr.alloc_zeroed((size_t)p.n_bsets * np_t * 16), AIRBAND_HIP_ENOMEM);
    if (!p.bfrag.empty()) HIP_TRY(PREPARING, hipMemcpy(h->d_bfrag.p, p.bfrag.data(), p.bfrag.size(), hipMemcpyHostToDevice), AIRBAND_HIP_ENOMEM);
    if (!p.bcorr.empty()) HIP_TRY(PREPARING, hipMemcpy(h->d_bcorr.p, p.bcorr.data(), p.bcorr.size() * sizeof(double), hipMemcpyHostToDevice), AIRBAND_HIP_ENOMEM);
    /* shared tables the host did not build (fleets with more than a few thousand distinct channel plans), then the private ones: a private table's columns
     * are copied from its home table, so the home tables come first */
    launch_build_tables(h->d_bfrag.p, h->d_bcorr.p, h->d_window.p, h->d_bset_bin.p, p.n_host_bsets, p.n_shared_bsets - p.n_host_bsets, p.fft_size, h->stream);
    if (p.n_bsets > p.n_shared_bsets) launch_retune_tables(h, h->stream, 0);
    if (p.n_bsets > p.n_host_bsets) {
        HIP_TRY(PREPARING, hipGetLastError(), AIRBAND_HIP_ENODEV);
        HIP_TRY(PREPARING, hipStreamSynchronize(h->stream), AIRBAND_HIP_ENODEV);
    }
    if (p.fft_size > 4096) /* [work items][tiles][64 lanes] float4 */
        HIP_TRY(PREPARING, h->d_dft_partial.alloc((size_t)p.item_dev.size() * dft_partial_tiles(h->B + AB_AGC_EXTRA) * 64 * 4), AIRBAND_HIP_ENOMEM);
    return AIRBAND_HIP_OK;
}

/* CF32 (SoapySDR): the float32 matrix pipe, unless its tables are past their budgets (use_f32 is cleared then).  Round 6: also with AFC channels -- a group with
 * one owns a private float table whose column pairs the re-tune kernel moves (misc_kernels.hip, build_column_pair_f32), exactly as the int8 path does; such
 * handles stayed on the wavefront FFT before. */
int prep_f32_tables(airband_hip_handle* h) {
    const Plan& p = h->plan;
    build_dft_tables(h->plan, false); /* the work items and the shared bin sets (its int8 tables are not used) */
    /* bytes, not a count: a float table is f32_nw x (2 N / 4 / f32_nw) x 64 lanes x 4 bytes = 128 N bytes -- 64 KiB at fft 512, 256 KiB at 2048.  The shared tables are
     * built on the host (params.cpp, build_f32_tables) and read once per work item per launch: past a budget the handle runs on the wavefront FFT rather than on a
     * gigabyte-sized host build; the private ones (device-built) count against the budget the int8 path's private tables have */
    const size_t ftab_each = 128u * (size_t)p.fft_size;
    h->use_f32 = (size_t)p.n_shared_bsets * ftab_each <= AB_F32_TABLE_BUDGET && (size_t)p.n_bsets * ftab_each <= AB_PRIVATE_TABLE_BUDGET;
    if (h->use_f32) {
        build_f32_tables(h->plan);
        const int rc = upload_work_items(h);
        if (rc != AIRBAND_HIP_OK) return rc;
        if (p.n_bsets > p.n_shared_bsets) { /* groups with an AFC channel: their private tables follow the shared ones, built by the re-tune kernel right here */
            const int rc_afc = upload_retune_items(h);
            if (rc_afc != AIRBAND_HIP_OK) return rc_afc;
            HIP_TRY(PREPARING, h->d_ftab.alloc_zeroed((size_t)p.n_bsets * ftab_each / sizeof(float)), AIRBAND_HIP_ENOMEM);
            HIP_TRY(PREPARING, hipMemcpy(h->d_ftab.p, p.ftab.data(), p.ftab.size() * sizeof(float), hipMemcpyHostToDevice), AIRBAND_HIP_ENOMEM);
            launch_retune_tables(h, h->stream, 0);
            HIP_TRY(PREPARING, hipGetLastError(), AIRBAND_HIP_ENODEV);
            HIP_TRY(PREPARING, hipStreamSynchronize(h->stream), AIRBAND_HIP_ENODEV);
        } else {
            HIP_TRY(PREPARING, upload(h->d_ftab, p.ftab), AIRBAND_HIP_ENOMEM);
        }
        /* fft_size 4096 / 8192: partial sums between the launches of the window's segments (channelizer_f32.hip) */
        if (f32_n_seg(p.fft_size) > 1 || (h->use_f32_wide && f32_wide_plan(p.fft_size, p.dev[0].hop_samples, nullptr, nullptr) > 1)) HIP_TRY(PREPARING, h->d_dft_partial.alloc((size_t)p.item_dev.size() * f32_partial_tiles(h->B + AB_AGC_EXTRA) * 64 * 4), AIRBAND_HIP_ENOMEM);
    }
    h->plan.bfrag.clear(); h->plan.bfrag.shrink_to_fit();
    h->plan.ftab.clear(); h->plan.ftab.shrink_to_fit();
    return AIRBAND_HIP_OK;
}

/* channelizer variant: matrix-core pruned DFT when the configuration qualifies, wavefront FFT otherwise */
int prep_channelizer(airband_hip_handle* h) {
    const Plan& p = h->plan;
    /* AFC moves bins at run time and needs the full spectrum of each batch's last hop: that is the FFT kernel's job */
    if (h->any_afc) HIP_TRY(PREPARING, h->d_spectrum.alloc((size_t)p.n_dev * p.fft_size * 2), AIRBAND_HIP_ENOMEM);
    const bool force_fft = (h->flags & AIRBAND_HIP_FLAG_FORCE_FFT) != 0;
    const int sfmt = p.dev[0].sfmt, hop_b = (int)h->hop_bytes;
    h->use_dft = !force_fft && dft_supported(p.fft_size, hop_b, sfmt, p.max_ch);
    h->use_wide = false;
    h->chan_reason = force_fft ? "FORCE_FFT" : "";
    /* Hops beyond the contiguous staging of channelizer_dft.hip (u8 / s8 above 1 024 bytes, CS16 above 1 280): the row staging of channelizer_dft_wide.hip,
     * for handles that ask for it and wherever dft_wide_plan() finds it a staging plan (whole windows, or windows in 2 / 4 k-segments: it depends on the window and, for
     * the reader of odd hops, on the hop's alignment) -- else the wavefront FFT, and the handle says why */
    bool wide_spills = false;
    const int wide_seg = force_fft || h->use_dft ? -1 : dft_wide_plan(p.fft_size, hop_b, sfmt, nullptr, &wide_spills);
    if (wide_seg >= 0) {
        const int limit = sfmt == AIRBAND_SFMT_S16 ? 1280 : 1024;
        if (!(h->flags & AIRBAND_HIP_FLAG_WIDE_HOPS))
            h->chan_reason = "hop " + std::to_string(hop_b) + " bytes > " + std::to_string(limit) + ": AIRBAND_HIP_FLAG_WIDE_HOPS not set";
        else if (wide_spills)
            h->chan_reason = "wide hops: fft " + std::to_string(p.fft_size) + " at hops of an odd number of samples: the segmented kernel spills registers and is not built";
        else if (wide_seg == 0)
            h->chan_reason = "wide hops: fft " + std::to_string(p.fft_size) + " staging does not fit LDS (" + std::to_string(dft_wide_lds(p.fft_size, hop_b, sfmt)) + " bytes > " + std::to_string(AB_DFT_WIDE_LDS_MAX) + ")";
        else
            h->use_dft = h->use_wide = true;
    }
    if (h->use_dft) {
        const int rc = prep_dft_tables(h);
        if (rc != AIRBAND_HIP_OK) return rc;
        if (!h->use_dft) { /* cleared: the tables are past their budget */
            h->use_wide = false;
            h->chan_reason = "coefficient tables past their byte budget";
        }
    }
    h->use_f32 = !h->use_dft && !force_fft && f32_supported(p.fft_size, p.dev[0].hop_samples, sfmt);
    if (h->use_f32) {
        const int rc = prep_f32_tables(h);
        if (rc != AIRBAND_HIP_OK) return rc;
        if (!h->use_f32) h->chan_reason = "coefficient tables past their byte budget";
    }
    /* CF32 hops beyond the contiguous staging of channelizer_f32.hip (a tile of 15 hops + a window no longer fits its registers or LDS: above ~3 MS/s at WAVE_RATE
     * 8000): the row staging of channelizer_f32_wide.hip for handles that ask for it -- same tables, same contraction, whatever the hop.  Inside f32_supported()'s
     * limits f32_wide_plan() returns -1 and the flag changes nothing. */
    h->use_f32_wide = false;
    if (!h->use_dft && !h->use_f32 && !force_fft && sfmt == AIRBAND_SFMT_F32 && h->chan_reason.empty()) {
        const int wide_seg = f32_wide_plan(p.fft_size, p.dev[0].hop_samples, nullptr, nullptr);
        if (wide_seg >= 0 && !(h->flags & AIRBAND_HIP_FLAG_WIDE_HOPS)) {
            h->chan_reason = "hop " + std::to_string(hop_b) + " bytes: beyond the float channelizer's tile; AIRBAND_HIP_FLAG_WIDE_HOPS not set";
        } else if (wide_seg == 0) {
            h->chan_reason = "wide hops: CF32 fft " + std::to_string(p.fft_size) + " has no staging plan";
        } else if (wide_seg > 0) {
            h->use_f32 = h->use_f32_wide = true;
            const int rc = prep_f32_tables(h);
            if (rc != AIRBAND_HIP_OK) return rc;
            if (!h->use_f32) {
                h->use_f32_wide = false;
                h->chan_reason = "coefficient tables past their byte budget";
            }
        }
    }
    if (!h->use_dft && !h->use_f32 && h->chan_reason.empty()) /* no matrix-core kernel takes the shape at all */
        h->chan_reason = sfmt == AIRBAND_SFMT_F32 ? "CF32 shape outside the float matrix-core channelizer's limits"
                                                  : "hop " + std::to_string(hop_b) + " bytes, fft " + std::to_string(p.fft_size) + ": outside the matrix-core channelizer's shapes";
    if (!h->use_dft && !h->use_f32) {
        const size_t lds = fft_lds_bytes(p.fft_log, p.dev[0].hop_samples, p.dev[0].bytes_per_sample);
        if (lds > 160 * 1024) /* e.g. F32 at 20 MS/s: a 16-hop tile of raw samples does not fit a CU's LDS */
            return fail(PREPARING, AIRBAND_HIP_EBADSIZE,
                        "sample_rate x bytes_per_sample too large for the FFT channelizer's LDS tile (" + std::to_string(lds) + " > 163840 bytes)" +
                            (sfmt == AIRBAND_SFMT_F32 && !force_fft && !(h->flags & AIRBAND_HIP_FLAG_WIDE_HOPS) && f32_wide_plan(p.fft_size, p.dev[0].hop_samples, nullptr, nullptr) > 0
                                 ? "; AIRBAND_HIP_FLAG_WIDE_HOPS not set (with it the float matrix-core channelizer takes this shape)" : ""));
    }
    return AIRBAND_HIP_OK;
}

}  // namespace

extern "C" {

const char* airband_hip_last_error(const airband_hip_handle* h) { return h ? h->error.c_str() : g_prepare_error.c_str(); }

int airband_hip_derive_constants(const airband_hip_config* cfg, int32_t channel_index, double* out_vals) {
    Plan plan;
    int rc = build_plan(cfg, plan);
    if (rc != AIRBAND_HIP_OK) return fail(nullptr, rc, plan.error);
    if (channel_index < 0 || channel_index >= plan.total_ch || !out_vals) return fail(nullptr, AIRBAND_HIP_EINVAL, "bad channel index");
    channel_constants(plan, channel_index, out_vals);
    return AIRBAND_HIP_OK;
}

int airband_hip_dft_selftest(const airband_hip_config* cfg, int32_t windows, double* max_rel_err) {
    if (!cfg || !max_rel_err) return fail(nullptr, AIRBAND_HIP_EINVAL, "NULL argument");
    Plan plan;
    const int rc = build_plan(cfg, plan);
    if (rc != AIRBAND_HIP_OK) return fail(nullptr, rc, plan.error);
    const int hop_bytes = 2 * plan.dev[0].bytes_per_sample * plan.dev[0].hop_samples;
    if (plan.uniform_hop && f32_supported(plan.fft_size, plan.dev[0].hop_samples, plan.dev[0].sfmt)) { /* CF32: the float tables of channelizer_f32.hip */
        build_dft_tables(plan);
        build_f32_tables(plan);
        *max_rel_err = f32_table_selftest(plan, windows < 1 ? 1 : windows);
        return AIRBAND_HIP_OK;
    }
    /* CF32 beyond those limits, flagged: the same tables in the order channelizer_f32_wide.hip contracts them (prep_channelizer()'s rule, f32_wide_plan()) */
    if (plan.uniform_hop && plan.dev[0].sfmt == AIRBAND_SFMT_F32 && (cfg->flags & AIRBAND_HIP_FLAG_WIDE_HOPS) &&
        f32_wide_plan(plan.fft_size, plan.dev[0].hop_samples, nullptr, nullptr) > 0) {
        build_dft_tables(plan);
        build_f32_tables(plan);
        *max_rel_err = f32_table_selftest(plan, windows < 1 ? 1 : windows, f32_wide_seg_size(plan.fft_size));
        return AIRBAND_HIP_OK;
    }
    /* the tables do not depend on the hop; whether a flagged handle takes the wide-hop kernel is prep_channelizer()'s rule, dft_wide_plan() */
    const bool wide = (cfg->flags & AIRBAND_HIP_FLAG_WIDE_HOPS) && dft_wide_plan(plan.fft_size, hop_bytes, plan.dev[0].sfmt, nullptr, nullptr) > 0;
    if (!plan.uniform_hop || !(wide || dft_supported(plan.fft_size, hop_bytes, plan.dev[0].sfmt, plan.max_ch)))
        return fail(nullptr, AIRBAND_HIP_EBADSIZE, "configuration does not take the matrix-core channelizer");
    build_dft_tables(plan);
    *max_rel_err = dft_table_selftest(plan, windows < 1 ? 1 : windows);
    return AIRBAND_HIP_OK;
}

int airband_hip_prepare(const airband_hip_config* cfg, airband_hip_handle** out) { return airband_hip_prepare_scan(cfg, nullptr, 0, out); }

int airband_hip_prepare_scan(const airband_hip_config* cfg, const airband_hip_scan_cfg* scan, int32_t n_scan, airband_hip_handle** out) {
    return airband_hip_prepare_follow(cfg, scan, n_scan, nullptr, 0, out);
}

int airband_hip_prepare_follow(const airband_hip_config* cfg, const airband_hip_scan_cfg* scan, int32_t n_scan, const int32_t* follow_channels, int32_t n_follow, airband_hip_handle** out) {
    if (!out) return fail(nullptr, AIRBAND_HIP_EINVAL, "out is NULL");
    *out = nullptr;
    HandlePtr owner(new (std::nothrow) airband_hip_handle(), destroy);
    airband_hip_handle* const h = owner.get();
    if (!h) return fail(nullptr, AIRBAND_HIP_ENOMEM, "host allocation failed");
    int rc = build_plan(cfg, h->plan);
    if (rc == AIRBAND_HIP_OK) rc = build_scan(cfg, scan, n_scan, h->plan); /* before any device is touched */
    if (rc == AIRBAND_HIP_OK) rc = build_follow(cfg, follow_channels, n_follow, h->plan);
    if (rc != AIRBAND_HIP_OK) return fail(PREPARING, rc, h->plan.error);
    const Plan& p = h->plan;
    if (!p.uniform_hop)
        return fail(PREPARING, AIRBAND_HIP_EINVAL, "all dongles of one handle must share sample format and sample_rate/WAVE_RATE hop; use one handle per class");
    for (const ChanConst& c : p.cc) h->any_afc |= c.afc != 0;
    const bool followers = !p.follow_ext.empty(); /* the band follow decides a follower's bin behind stage 2 of batch k, stage 1 of batch k+1 reads it: sequential, as with AFC */
    h->flags = cfg->flags;
    h->hip_device = cfg->hip_device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->hip_device < 0 || cfg->hip_device >= ndev)
        return fail(PREPARING, AIRBAND_HIP_ENODEV, "no usable HIP device (libairband_hip has no CPU fallback)");
    /* AFC needs stage 2's verdict on batch k before stage 1 of batch k+1 picks its bins (src/rtl_airband.cpp:222-251):
     * such handles stay sequential */
    h->pipeline = (cfg->flags & AIRBAND_HIP_FLAG_PIPELINE) && !h->any_afc && !followers;
    /* The same GPU schedule without the lag, for batches on the handle's own stream (airband_hip_process_device).  Not with AFC, for the reason above; not with scan
     * lists, whose exchange in front of the demod kernels is ordered against stage 1 by the one stream.  AIRBAND_HIP_RUN_AHEAD=0 in the environment: off (A/B
     * measurements; the handle then has the one-batch rings and the unheld channelizer of the sequential schedule). */
    const char* run_ahead_env = getenv("AIRBAND_HIP_RUN_AHEAD");
    h->run_ahead = !(cfg->flags & AIRBAND_HIP_FLAG_PIPELINE) && !h->any_afc && !followers && p.scan.empty() && !(run_ahead_env && *run_ahead_env == '0');
    rc = prep_streams(h);
    if (rc != AIRBAND_HIP_OK) return rc;
    std::vector<ChanState> cs_slots;
    std::vector<uint8_t> block_kind;
    prep_slots(h, cs_slots, block_kind);
    prep_geometry(h);
    rc = prep_constants(h, cs_slots, block_kind);
    if (rc == AIRBAND_HIP_OK) rc = prep_rings(h);
    if (rc == AIRBAND_HIP_OK) rc = prep_regroup(h);
    if (rc == AIRBAND_HIP_OK) rc = prep_results(h);
    if (rc == AIRBAND_HIP_OK) rc = prep_channelizer(h);
    if (rc != AIRBAND_HIP_OK) return rc;
    h->ring_wr.reset(new std::atomic<uint64_t>[p.n_dev]);
    for (int d = 0; d < p.n_dev; d++) h->ring_wr[d].store(0);
    h->dev_enabled.reset(new std::atomic<uint8_t>[p.n_dev]);
    for (int d = 0; d < p.n_dev; d++) h->dev_enabled[d].store(1);
    h->n_enabled = p.n_dev;
    if (!p.scan.empty()) rc = prep_scan(h);
    if (rc != AIRBAND_HIP_OK) return rc;
    *out = owner.release();
    return AIRBAND_HIP_OK;
}

void airband_hip_release(airband_hip_handle* h) { destroy(h); }

int airband_hip_get_geometry(const airband_hip_handle* h, airband_hip_geometry* g) {
    if (!h || !g) return AIRBAND_HIP_EINVAL;
    g->fft_size = h->N;
    g->wave_rate = h->plan.wave_rate;
    g->wave_batch = h->B;
    g->device_count = h->plan.n_dev;
    g->total_channels = h->plan.total_ch;
    g->max_channels = h->plan.max_ch;
    g->mixer_count = h->mix.n_mixers;
    g->wave_stride = h->wave_stride;
    g->first_batch_bytes = h->first_batch_bytes;
    g->batch_bytes = h->batch_bytes;
    g->lookahead_bytes = h->lookahead_bytes;
    return AIRBAND_HIP_OK;
}

int airband_hip_device_enable(airband_hip_handle* h, int32_t dev, int32_t enabled) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const Plan& p = h->plan;
    if (dev < 0 || dev >= p.n_dev) return fail(h, AIRBAND_HIP_EINVAL, "device index out of range");
    const uint8_t on = enabled ? 1 : 0;
    if (h->dev_enabled[dev].load() == on) return AIRBAND_HIP_OK;
    ON_OWN_STREAM(h, s);
    /* everything below is ordered on the handle's stream: the batches already enqueued still see the old state, the next one the new */
    h->plan.dev[dev].disabled = on ? 0 : 1;
    HIP_TRY(h, hipMemcpyAsync(&h->d_dev.p[dev], &h->plan.dev[dev], sizeof(DevConst), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    const int c0 = p.chan_base[dev], nc = p.dev[dev].n_ch;
    std::vector<uint8_t> blank((size_t)nc, (uint8_t)' ');
    for (int c = c0; c < c0 + nc; c++) { /* the demod kernels treat a slot without AB_F_VALID like padding: the lane leaves at once, its state stays as it is */
        const int slot = h->ext_to_slot[c];
        ChanConst& cc = h->cc_slots[slot];
        cc.flags = on ? (cc.flags | AB_F_VALID) : (cc.flags & ~AB_F_VALID);
        if (h->scan_ctl.idle_batches > 0 && !h->scan_of_dev.empty() && h->scan_of_dev[dev] >= 0) {
            /* a scan slot under scan control: the per-frequency bits of the live word are those of the entry the GPU put in force, which the host copy does not
             * follow -- only VALID is set or cleared, on the device, in stream order */
            launch_scan_set_valid(h->d_cc.p, slot, h->n_slots, on, s);
            continue;
        }
        HIP_TRY(h, hipMemcpyAsync(&h->d_cc.p[slot].flags, &cc.flags, sizeof(cc.flags), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    }
    /* channel->axcindicate of a device that is not demodulated any more: NO_SIGNAL */
    if (!on) HIP_TRY(h, hipMemcpyAsync(h->d_out_axc.p + c0, blank.data(), (size_t)nc, hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    /* a gated handle delivers none of its rows while it is off (disable_device_outputs()); the select pass also clears the channels' "had signal in the batch before" */
    std::vector<uint8_t> gate_bytes;
    if (h->gate.max_rows > 0) {
        gate_bytes.assign(h->gate.gate.begin() + c0, h->gate.gate.begin() + c0 + nc);
        if (!on)
            for (uint8_t& g : gate_bytes) g |= AB_GATE_OFF;
        HIP_TRY(h, hipMemcpyAsync(h->gate.d_gate.p + c0, gate_bytes.data(), (size_t)nc, hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    }
    /* host-ring path: a dongle that comes back joins the others at the common stream position with an empty queue -- its write cursor is put there
     * BEFORE the dongle is published as enabled (release / acquire with submit()'s load): a feeder thread that sees it enabled never sees the stale cursor */
    if (on && h->ring_wr) h->ring_wr[dev].store(h->ring_rd, std::memory_order_release);
    h->dev_enabled[dev].store(on, std::memory_order_release);
    h->n_enabled += on ? 1 : -1;
    /* its mixer connections: mixer_disable_input() for every output of the device, as disable_device_outputs() does (src/output.cpp, src/mixer.cpp:96-110) */
    for (size_t k = 0; k < h->mix.chan_host.size(); k++)
        if (p.cc[h->mix.chan_host[k]].dev == dev) HIP_TRY(h, write_mix_input(h, (int)k), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME); /* the host buffers above go out of scope */
    return AIRBAND_HIP_OK;
}

int airband_hip_gpu_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* stage 1 of the next batch (index front_batches, ring rows from row0_front) on stream s */
static int launch_front(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, hipStream_t s) {
    const FrontRows r = front_rows(h);
    const Event* ev = event_set(h, h->front_batches, 0);
    /* hipGetLastError() is sticky: whatever an earlier, unchecked call of this thread left behind (ours or the host application's) is not this launch's error */
    (void)hipGetLastError();
    h->afc_spectrum_valid = h->any_afc;
    if (h->use_f32 || h->use_dft) { /* the matrix-core channelizers leave the last hop's spectrum to the wavefront FFT */
        h->last_iq = d_iq;
        h->last_iq_stride = stride_bytes;
        h->last_n_hops = r.n_hops;
        if (h->any_afc) {
            const int rc = launch_last_hop_spectrum(h, s);
            if (rc != AIRBAND_HIP_OK) return rc;
        }
    }
    const int rc_scope = scope_fork(h, d_iq, stride_bytes, r, s);
    if (rc_scope != AIRBAND_HIP_OK) return rc_scope;
    (void)hipEventRecord(ev[0], s);
    if (h->use_f32_wide) launch_channelizer_f32_wide(f32_args(h, d_iq, stride_bytes, r), s);
    else if (h->use_f32) launch_channelizer_f32(f32_args(h, d_iq, stride_bytes, r), s);
    else if (h->use_wide) launch_channelizer_dft_wide(dft_args(h, d_iq, stride_bytes, r), s);
    else if (h->use_dft) launch_channelizer_dft(dft_args(h, d_iq, stride_bytes, r), s);
    else launch_channelizer_fft(fft_args(h, d_iq, stride_bytes, h->row0_front, r, 0), s);
    const hipError_t launch_err = hipGetLastError(); /* right behind the launch: the event record below would mask it (or be blamed for it) */
    (void)hipEventRecord(ev[1], s);
    /* a refused launch (an LDS opt-in that failed, a bad grid) is this call's error, not a puzzle for whoever synchronises next */
    if (launch_err != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("channelizer launch: ") + hipGetErrorString(launch_err));
    const int rc_join = scope_join(h, d_iq, stride_bytes, r, s);
    if (rc_join != AIRBAND_HIP_OK) return rc_join;
    front_enqueued(h, r.first_row, r.n_hops);
    return AIRBAND_HIP_OK;
}

/* airband_hip_process_device(); run_ahead_ok = false keeps a run-ahead handle's batch on the one stream (the host-ring path, whose staging buffers are ordered there) */
static int process_batch(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, void* stream, bool run_ahead_ok) {
    if (!h || !d_iq) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* hops of whole 16-byte pieces: the channelizer's transfers address the span directly, so it must start on one.  Any other hop (300, 250 bytes ...):
     * a batch of such hops cannot start on 16 bytes every time anyway (2 100 hops of 250 bytes = 525 000), the kernel stages from the aligned byte in
     * front of the span and only whole samples are asked for */
    /* ... at the alignment of the fragment reads the kernel variant for this hop uses (channelizer_dft.hip, launch_generic: the largest power of two up to 16
     * that divides the hop -- 300 bytes: 4, 600: 8, 250: 2): the staged bytes keep the span's offset from 16 bytes, and a 4- or 8-byte LDS read must not land
     * on a 2-byte boundary.  Batch offsets are multiples of the hop, so a stream that starts aligned stays aligned. */
    uintptr_t al = 16;
    while (al > 2 && (h->hop_bytes % (int64_t)al) != 0) al >>= 1;
    if (al < (uintptr_t)(2 * h->plan.dev[0].bytes_per_sample)) al = (uintptr_t)(2 * h->plan.dev[0].bytes_per_sample);
    const uintptr_t need = al - 1;
    if (h->use_f32 && !h->use_f32_wide && ((((uintptr_t)d_iq) | (uintptr_t)stride_bytes) & 15))
        return fail(h, AIRBAND_HIP_EINVAL, "d_iq and stride_bytes must be multiples of 16 (the channelizer fetches 16 bytes per lane)");
    if ((h->use_dft || h->use_f32_wide) && ((((uintptr_t)d_iq) | (uintptr_t)stride_bytes) & need)) /* (CF32 wide hops: 16, or 8 at hops of an odd number of samples) */
        return fail(h, AIRBAND_HIP_EINVAL, (h->hop_bytes % 16) == 0 ? "d_iq and stride_bytes must be multiples of 16 (the channelizer fetches 16 bytes per lane)"
                                                                    : "d_iq and stride_bytes must be multiples of the largest power of two (up to 16) that divides the hop's bytes");
    if (h->run_ahead && !stream && run_ahead_ok) {
        /* Run-ahead: stage 1 of this batch (k) on the front stream, stage 2 (k) on the handle's stream behind it, both enqueued now -- the batch's results are complete
         * in the handle's stream order exactly as on the sequential path, so collect / read_* / synchronize / stream_wait_results know nothing of it.  What the front
         * stream waits for is what stage 1 (k) really depends on, and stage 2 (k-1) is not among it: stage 1 (k-1) by stream order (the scratch the two share), and
         * the back half of batch k-2, whose ring rows it overwrites (back_done).  A caller that enqueues batches back to back therefore gets stage 1 (k+1) beside
         * stage 2 (k).  Anything else a stage 1 may depend on -- its input written by a kernel on the handle's stream, a batch that ran on another path -- has set
         * serialise_next, and the front waits for the whole of the handle's stream, once. */
        const uint64_t k = h->front_batches;
        if (h->ev_last_pending) order_behind_last_batch(h); /* an exchange or a clear on a caller's stream: this batch's sums come behind it */
        if (h->serialise_next) {
            HIP_TRY(h, hipEventRecord(h->ev_in, h->stream), AIRBAND_HIP_ERUNTIME);
            HIP_TRY(h, hipStreamWaitEvent(h->front, h->ev_in, 0), AIRBAND_HIP_ERUNTIME);
        } else if (k >= 2) {
            HIP_TRY(h, hipStreamWaitEvent(h->front, h->back_done[k & 1], 0), AIRBAND_HIP_ERUNTIME);
        }
        h->serialise_next = false;
        h->last_stream = h->stream;
        const int rc_front = launch_front(h, d_iq, stride_bytes, h->front);
        if (rc_front != AIRBAND_HIP_OK) return rc_front;
        HIP_TRY(h, hipEventRecord(h->front_done[k & 1], h->front), AIRBAND_HIP_ERUNTIME);
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->front_done[k & 1], 0), AIRBAND_HIP_ERUNTIME);
        const int rc = run_back_half(h, h->stream);
        h->ev_last_pending = false;
        h->ahead_batches++;
        return rc;
    }
    if (!h->pipeline) {
        hipStream_t s = stream ? (hipStream_t)stream : h->stream;
        h->last_stream = s;
        /* a run-ahead handle on its sequential path (a caller's stream; the host ring): stage 1 of the next run-ahead batch must not start beside this batch's */
        if (h->run_ahead) h->serialise_next = true;
        const int rc_front = launch_front(h, d_iq, stride_bytes, s);
        if (rc_front != AIRBAND_HIP_OK) return rc_front;
        const int rc = run_back_half(h, s);
        /* collect() and friends run on h->stream.  A batch of its own is in order there already, and everything an earlier mark stood for lies in front of it:
         * only a whole batch CLEARS the mark (an exchange or a clear on the handle's stream leaves it alone) */
        if (s == h->stream) h->ev_last_pending = false;
        const int rc_mark = results_enqueued_on(h, s);
        return rc_mark != AIRBAND_HIP_OK ? rc_mark : rc;
    }
    /* Pipelined: stage 1 of this batch (k) goes on the front stream and runs beside stage 2 of batch k-1, which is enqueued
     * right after it on the handle's stream.  Stage 1 (k) overwrites the ring rows stage 2 (k-2) read, and may use the
     * caller's input as soon as the caller's stream (or everything enqueued on the handle so far) has produced it. */
    hipStream_t in = stream ? (hipStream_t)stream : h->stream;
    HIP_TRY(h, hipEventRecord(h->ev_in, in), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamWaitEvent(h->front, h->ev_in, 0), AIRBAND_HIP_ERUNTIME);
    if (in != h->stream) {
        /* a caller stream orders BOTH halves: its earlier work (producing this input, consuming the previous results) is done
         * before stage 1 reads and before stage 2 overwrites the result buffers */
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_in, 0), AIRBAND_HIP_ERUNTIME);
        HIP_TRY(h, hipEventRecord(h->ev_back, h->stream), AIRBAND_HIP_ERUNTIME);
        HIP_TRY(h, hipStreamWaitEvent(h->front, h->ev_back, 0), AIRBAND_HIP_ERUNTIME);
    }
    const uint64_t k = h->front_batches;
    const int rc_front = launch_front(h, d_iq, stride_bytes, h->front);
    if (rc_front != AIRBAND_HIP_OK) return rc_front;
    HIP_TRY(h, hipEventRecord(h->front_done[k & 1], h->front), AIRBAND_HIP_ERUNTIME);
    /* nothing to demodulate yet -- the very first call, or the first call after airband_hip_flush() drained the pipeline:
     * the results of this batch appear with the next call (or flush) */
    if (h->batches_done == k) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->front_done[(k - 1) & 1], 0), AIRBAND_HIP_ERUNTIME);
    return run_back_half(h, h->stream);
}

int airband_hip_process_device(airband_hip_handle* h, const void* d_iq, size_t stride_bytes, void* stream) { return process_batch(h, d_iq, stride_bytes, stream, true); }

int airband_hip_stream_wait_results(airband_hip_handle* h, void* stream) {
    if (!h || !stream) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    HIP_TRY(h, h->ev_wait.ensure(), AIRBAND_HIP_ENODEV);
    hipStream_t res = results_stream(h);
    if (res == (hipStream_t)stream) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipEventRecord(h->ev_wait, res), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamWaitEvent((hipStream_t)stream, h->ev_wait, 0), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_flush(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!h->pipeline || h->front_batches == h->batches_done) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->front_done[(h->front_batches - 1) & 1], 0), AIRBAND_HIP_ERUNTIME);
    return run_back_half(h, h->stream);
}

/* bytes of every dongle's stream the next batch consumes (the first one with its lead-in) */
static int64_t next_batch_bytes(const airband_hip_handle* h) { return h->front_batches == 0 ? h->first_batch_bytes : h->batch_bytes; }

/* The availability rule (src/rtl_airband.cpp:394-400) applied to a whole batch: every dongle has the batch and its look-ahead.  Dongles switched off (failed
 * inputs) are not waited for: next_device() passes them by, src/rtl_airband.cpp:383-391; with every dongle switched off there is nothing to demodulate (the
 * reference exits, src/rtl_airband.cpp:377-381). */
static bool batch_available(const airband_hip_handle* h) {
    if (h->n_enabled == 0) return false;
    const int64_t need = next_batch_bytes(h) + h->lookahead_bytes;
    for (int d = 0; d < h->plan.n_dev; d++)
        if (h->dev_enabled[d] && (int64_t)(h->ring_wr[d].load(std::memory_order_acquire) - h->ring_rd) < need) return false;
    return true;
}

/* first use of the host-ring path: pinned rings, device staging, copy stream */
static int host_path_init(airband_hip_handle* h) {
    std::lock_guard<std::mutex> guard(h->host_init_lock);
    if (h->h_ring.load(std::memory_order_acquire)) return AIRBAND_HIP_OK;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    /* bounded like the reference's ring (MIN_BUF_SIZE = 2 560 000 bytes ~ 4 batches, src/rtl_airband.h:64): the first batch with its
     * lead-in, the batch in flight, one more being filled, and the look-ahead */
    h->ring_cap = (h->first_batch_bytes + 3 * h->batch_bytes + h->lookahead_bytes + 4095) / 4096 * 4096;
    h->stage_stride = (h->first_batch_bytes + h->lookahead_bytes + 255) / 256 * 256;
    for (auto& b : h->d_stage2)
        if (!b.p) HIP_TRY(h, b.alloc((size_t)h->stage_stride * h->plan.n_dev), AIRBAND_HIP_ENOMEM);
    if (!h->h2d) HIP_TRY(h, hipStreamCreateWithFlags(&h->h2d.v, hipStreamNonBlocking), AIRBAND_HIP_ENODEV);
    for (auto& e : h->ev_h2d) HIP_TRY(h, e.ensure(), AIRBAND_HIP_ENODEV);
    for (auto& e : h->ev_stage_read) HIP_TRY(h, e.ensure(), AIRBAND_HIP_ENODEV);
    HIP_TRY(h, h->ring_mem.alloc((size_t)h->ring_cap * h->plan.n_dev), AIRBAND_HIP_ENOMEM);
    h->h_ring.store(h->ring_mem.get(), std::memory_order_release); /* published last: submit() / process() test this pointer without the lock */
    return AIRBAND_HIP_OK;
}

int64_t airband_hip_submit(airband_hip_handle* h, int32_t dev, const void* iq, size_t nbytes) {
    if (!h || !iq) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (dev < 0 || dev >= h->plan.n_dev) return fail(h, AIRBAND_HIP_EINVAL, "device index out of range");
    if (!h->dev_enabled[dev]) return (int64_t)nbytes; /* a disabled dongle's bytes are dropped, as nobody reads a failed input's ring any more */
    uint8_t* ring = h->h_ring.load(std::memory_order_acquire);
    if (!ring) { /* the first submit of a handle sets the path up; concurrent first submits for different dongles serialise on the lock inside */
        const int rc = host_path_init(h);
        if (rc != AIRBAND_HIP_OK) return rc;
        ring = h->h_ring.load(std::memory_order_acquire);
    }
    const uint64_t wr = h->ring_wr[dev].load(std::memory_order_relaxed);
    const uint64_t used = wr - h->ring_free.load(std::memory_order_acquire);
    size_t take = nbytes;
    if (used + take > (uint64_t)h->ring_cap) take = (uint64_t)h->ring_cap > used ? (size_t)((uint64_t)h->ring_cap - used) : 0;
    uint8_t* row = ring + (size_t)dev * h->ring_cap;
    const size_t pos = (size_t)(wr % (uint64_t)h->ring_cap);
    const size_t first = take < (size_t)h->ring_cap - pos ? take : (size_t)h->ring_cap - pos;
    std::memcpy(row + pos, iq, first);
    if (take > first) std::memcpy(row, (const uint8_t*)iq + first, take - first);
    h->ring_wr[dev].store(wr + take, std::memory_order_release);
    return (int64_t)take;
}

/* would airband_hip_process() run a batch now?  The availability rule alone, nothing is enqueued.  -2 from airband_hip_process's own codes is not
 * used: OK = yes, EAGAIN = not yet (or every dongle is switched off). */
int airband_hip_batch_ready(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!h->h_ring.load(std::memory_order_acquire)) return AIRBAND_HIP_EAGAIN; /* nothing has been submitted yet */
    return batch_available(h) ? AIRBAND_HIP_OK : AIRBAND_HIP_EAGAIN;
}

int airband_hip_process(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    if (!h->h_ring.load(std::memory_order_acquire)) {
        const int rc = host_path_init(h);
        if (rc != AIRBAND_HIP_OK) return rc;
    }
    uint8_t* const ring = h->h_ring.load(std::memory_order_acquire);
    if (!batch_available(h)) return AIRBAND_HIP_EAGAIN;
    const int64_t consume = next_batch_bytes(h);
    const int64_t need = consume + h->lookahead_bytes;
    const int b = (int)(h->host_batches & 1);
    /* the DMA of the previous batch has left the ring: its bytes (up to the look-ahead the next batch re-reads) may be overwritten */
    if (h->host_batches > 0) {
        HIP_TRY(h, hipEventSynchronize(h->ev_h2d[b ^ 1]), AIRBAND_HIP_ERUNTIME);
        h->ring_free.store(h->ring_rd, std::memory_order_release);
    }
    /* staging buffer b was last read by the kernels of batch (k - 2) */
    if (h->host_batches >= 2) HIP_TRY(h, hipStreamWaitEvent(h->h2d, h->ev_stage_read[b], 0), AIRBAND_HIP_ERUNTIME);
    const size_t pos = (size_t)(h->ring_rd % (uint64_t)h->ring_cap);
    const size_t run = (size_t)need < (size_t)h->ring_cap - pos ? (size_t)need : (size_t)h->ring_cap - pos;
    HIP_TRY(h, hipMemcpy2DAsync(h->d_stage2[b].p, (size_t)h->stage_stride, ring + pos, (size_t)h->ring_cap, run, (size_t)h->plan.n_dev, hipMemcpyHostToDevice, h->h2d),
            AIRBAND_HIP_ERUNTIME);
    if (run < (size_t)need) /* the span wraps around the end of the rings */
        HIP_TRY(h, hipMemcpy2DAsync(h->d_stage2[b].p + run, (size_t)h->stage_stride, ring, (size_t)h->ring_cap, (size_t)need - run, (size_t)h->plan.n_dev,
                                    hipMemcpyHostToDevice, h->h2d),
                AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipEventRecord(h->ev_h2d[b], h->h2d), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_h2d[b], 0), AIRBAND_HIP_ERUNTIME);
    if (h->pipeline) HIP_TRY(h, hipStreamWaitEvent(h->front, h->ev_h2d[b], 0), AIRBAND_HIP_ERUNTIME);
    h->ring_rd += (uint64_t)consume;
    h->host_batches++;
    const int rc = process_batch(h, h->d_stage2[b].p, (size_t)h->stage_stride, nullptr, false); /* stays on the handle's stream: the DMA is what bounds this path */
    /* stage 1 of this batch (the only reader of the staging buffer) is enqueued: mark the point after which the buffer is free again */
    (void)hipEventRecord(h->ev_stage_read[b], h->pipeline ? h->front : h->stream);
    return rc;
}

int airband_hip_process_bins(airband_hip_handle* h, const float* wavein, const float* iq_in) {
    if (!h || !wavein || !iq_in) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (h->pipeline) return fail(h, AIRBAND_HIP_EINVAL, "process_bins (stage 2 only) is not available on a pipelined handle");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    const size_t n = (size_t)h->plan.total_ch * h->B;
    HIP_TRY(h, h->d_tmp_wavein.reserve(n), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, h->d_tmp_iqin.reserve(2 * n), AIRBAND_HIP_ENOMEM);
    hipStream_t s = h->stream;
    if (h->run_ahead) {
        /* the rings are written from the handle's stream here: behind the front stream's last stage 1 (the handle's stream is already, through that batch's back
         * half; said again where it matters), and the next stage 1 on the front stream behind this batch */
        if (h->ahead_batches > 0) HIP_TRY(h, hipStreamWaitEvent(s, h->front_done[(h->front_batches - 1) & 1], 0), AIRBAND_HIP_ERUNTIME);
        h->serialise_next = true;
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_tmp_wavein.p, wavein, n * sizeof(float), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemcpyAsync(h->d_tmp_iqin.p, iq_in, 2 * n * sizeof(float), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    const Event* ev = event_set(h, h->front_batches, 0);
    (void)hipEventRecord(ev[0], s);
    h->afc_spectrum_valid = false;
    launch_scatter_bins(h->d_tmp_wavein.p, h->d_tmp_iqin.p, h->d_slot_to_ext.p, h->d_cc.p, h->d_mag.p, h->d_iq.p, h->n_slots, h->B, h->row0, h->R, s);
    (void)hipEventRecord(ev[1], s);
    h->scope.set_of_front[h->front_batches & 1] = -1; /* no input to look at: the band scope stays as it is */
    front_enqueued(h, AB_AGC_EXTRA, h->B); /* the caller's rows are the batch's new ones; the carry is what the rings hold */
    return run_back_half(h, s);
}

int airband_hip_synchronize(airband_hip_handle* h) {
    if (!h) return AIRBAND_HIP_EINVAL;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    if (h->front) HIP_TRY(h, hipStreamSynchronize(h->front), AIRBAND_HIP_ERUNTIME);
    if (h->ev_last && h->ev_last_pending) HIP_TRY(h, hipEventSynchronize(h->ev_last), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

/* results of channels [first, first + n) of the batch last completed; `consume` marks the batch as collected */
static int collect_range(airband_hip_handle* h, int64_t first, int64_t n, float* waveout, float* iq_out, char* axc, airband_hip_channel_stats* stats, bool consume) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (first < 0 || n < 0 || first + n > h->plan.total_ch) return fail(h, AIRBAND_HIP_EINVAL, "channel range out of bounds");
    if (!h->results_ready && consume) return AIRBAND_HIP_EAGAIN;
    if (h->batches_done == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    const size_t nch = (size_t)n;
    if (stats && nch) {
        if (!h->d_stats.p) HIP_TRY(h, h->d_stats.alloc((size_t)h->plan.total_ch), AIRBAND_HIP_ENOMEM);
        launch_stats(h->d_cc.p, h->d_cs.p, h->d_slot_to_ext.p, h->n_slots, h->d_stats.p, s);
        HIP_TRY(h, hipMemcpyAsync(stats, h->d_stats.p + first, nch * sizeof(airband_hip_channel_stats), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    }
    if (waveout && nch)
        HIP_TRY(h, hipMemcpy2DAsync(waveout, h->B * sizeof(float), h->d_out_wave.p + (size_t)first * h->wave_stride + AB_OUT_PAD, (size_t)h->wave_stride * sizeof(float),
                                    h->B * sizeof(float), nch, hipMemcpyDeviceToHost, s),
                AIRBAND_HIP_ERUNTIME);
    if (iq_out && nch) {
        if (h->d_out_iq.p)
            HIP_TRY(h, hipMemcpyAsync(iq_out, h->d_out_iq.p + (size_t)first * h->B * 2, nch * h->B * 2 * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
        else
            std::memset(iq_out, 0, nch * h->B * 2 * sizeof(float));
    }
    if (axc && nch) HIP_TRY(h, hipMemcpyAsync(axc, h->d_out_axc.p + first, nch, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (consume) h->results_ready = false;
    return AIRBAND_HIP_OK;
}

int airband_hip_collect(airband_hip_handle* h, float* waveout, float* iq_out, char* axc, airband_hip_channel_stats* stats) {
    if (!h) return AIRBAND_HIP_EINVAL;
    return collect_range(h, 0, h->plan.total_ch, waveout, iq_out, axc, stats, true);
}

int airband_hip_collect_channels(airband_hip_handle* h, int64_t first_channel, int64_t n_channels, float* waveout, float* iq_out, char* axc,
                                 airband_hip_channel_stats* stats) {
    return collect_range(h, first_channel, n_channels, waveout, iq_out, axc, stats, false);
}

int airband_hip_device_results(airband_hip_handle* h, float** d_waveout, float** d_iq_out, uint8_t** d_axc, float** d_mix_left, float** d_mix_right,
                               uint8_t** d_mix_signal) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (d_waveout) *d_waveout = h->d_out_wave.p + AB_OUT_PAD;
    if (d_iq_out) *d_iq_out = h->d_out_iq.p;
    if (d_axc) *d_axc = h->d_out_axc.p;
    if (d_mix_left) *d_mix_left = h->mix.d_left.p;
    if (d_mix_right) *d_mix_right = h->mix.d_right.p;
    if (d_mix_signal) *d_mix_signal = h->mix.d_signal.p;
    return AIRBAND_HIP_OK;
}

static int gather_last(airband_hip_handle* h, int64_t first, int64_t nch, float* wavein, float* iq_in, uint8_t* trace) {
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    if (first < 0 || nch < 0 || first + nch > h->plan.total_ch) return fail(h, AIRBAND_HIP_EINVAL, "channel range out of bounds");
    if (h->batches_done == 0) return fail(h, AIRBAND_HIP_EAGAIN, "no batch processed yet");
    if (nch == 0) return AIRBAND_HIP_OK;
    const size_t n = (size_t)nch * h->B;
    if (wavein) HIP_TRY(h, h->d_tmp_wavein.reserve(n), AIRBAND_HIP_ENOMEM);
    if (iq_in) HIP_TRY(h, h->d_tmp_iqin.reserve(2 * n), AIRBAND_HIP_ENOMEM);
    if (trace) HIP_TRY(h, h->d_tmp_trace.reserve(n), AIRBAND_HIP_ENOMEM);
    hipStream_t s = h->stream;
    order_behind_last_batch(h);
    const int prev_row0 = (h->row0 + h->R - h->B) % h->R; /* row0 of the batch just finished */
    launch_gather_channels(h->d_mag.p, h->d_iq.p, h->d_trace.p, h->d_ext_to_slot.p, h->d_cc.p, (int)first, (int)nch, wavein ? h->d_tmp_wavein.p : nullptr,
                           iq_in ? h->d_tmp_iqin.p : nullptr, trace ? h->d_tmp_trace.p : nullptr, h->B, prev_row0, h->R, s);
    if (wavein) HIP_TRY(h, hipMemcpyAsync(wavein, h->d_tmp_wavein.p, n * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (iq_in) HIP_TRY(h, hipMemcpyAsync(iq_in, h->d_tmp_iqin.p, 2 * n * sizeof(float), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    if (trace) HIP_TRY(h, hipMemcpyAsync(trace, h->d_tmp_trace.p, n, hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_read_bins(airband_hip_handle* h, float* wavein, float* iq_in) {
    if (!h) return AIRBAND_HIP_EINVAL;
    return gather_last(h, 0, h->plan.total_ch, wavein, iq_in, nullptr);
}

int airband_hip_read_bins_channels(airband_hip_handle* h, int64_t first_channel, int64_t n_channels, float* wavein, float* iq_in) {
    if (!h) return AIRBAND_HIP_EINVAL;
    return gather_last(h, first_channel, n_channels, wavein, iq_in, nullptr);
}

int airband_hip_read_trace(airband_hip_handle* h, uint8_t* state) {
    if (!h || !state) return AIRBAND_HIP_EINVAL;
    if (!(h->flags & AIRBAND_HIP_FLAG_TRACE_SQUELCH)) return fail(h, AIRBAND_HIP_EINVAL, "handle was prepared without AIRBAND_HIP_FLAG_TRACE_SQUELCH");
    return gather_last(h, 0, h->plan.total_ch, nullptr, nullptr, state);
}

int airband_hip_read_trace_channels(airband_hip_handle* h, int64_t first_channel, int64_t n_channels, uint8_t* state) {
    if (!h || !state) return AIRBAND_HIP_EINVAL;
    if (!(h->flags & AIRBAND_HIP_FLAG_TRACE_SQUELCH)) return fail(h, AIRBAND_HIP_EINVAL, "handle was prepared without AIRBAND_HIP_FLAG_TRACE_SQUELCH");
    return gather_last(h, first_channel, n_channels, nullptr, nullptr, state);
}

int airband_hip_channel_constants(const airband_hip_handle* h, int32_t channel_index, double* out_vals) {
    if (!h || !out_vals || channel_index < 0 || channel_index >= h->plan.total_ch) return AIRBAND_HIP_EINVAL;
    channel_constants(h->plan, channel_index, out_vals);
    return AIRBAND_HIP_OK;
}

int airband_hip_read_tables(airband_hip_handle* h, int32_t first, int32_t n, airband_hip_table_info* info, void* tables, double* corr, int32_t* bset_bin, int32_t* items) {
    if (!h || !info) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (!h->use_dft && !h->use_f32) return fail(h, AIRBAND_HIP_EINVAL, "the handle runs on the wavefront FFT: it has no coefficient tables");
    const Plan& p = h->plan;
    const int N = p.fft_size;
    const size_t n_items = p.item_dev.size();
    std::memset(info, 0, sizeof(*info));
    info->n_bsets = p.n_bsets;
    info->n_shared_bsets = p.n_shared_bsets;
    info->n_items = (int32_t)n_items;
    if (h->use_dft) {
        info->n_host_bsets = p.n_host_bsets;
        info->pieces_per_table = N > 512 ? N / 512 : 1;
        info->bytes_per_table = (int64_t)3 * (N > 512 ? 16 : N / 32) * 64 * 16 * info->pieces_per_table;
        info->edge_hi_zero = p.b_edge_hi_zero ? 1 : 0;
    } else { /* build_f32_tables: the host builds every shared float table */
        info->n_host_bsets = p.n_shared_bsets;
        info->pieces_per_table = f32_n_seg(N) * f32_nw(N);
        info->bytes_per_table = (int64_t)128 * N;
    }
    std::snprintf(info->channelizer, sizeof(info->channelizer), "%s", airband_hip_channelizer_name(h));
    if (first < 0 || n < 0 || (int64_t)first + n > p.n_bsets) return fail(h, AIRBAND_HIP_EINVAL, "table range out of bounds");
    if (n == 0) return AIRBAND_HIP_OK;
    if (!tables || !corr || !bset_bin || !items) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    const int rc = airband_hip_synchronize(h);
    if (rc != AIRBAND_HIP_OK) return rc;
    const size_t each = (size_t)info->bytes_per_table, per_corr = (size_t)info->pieces_per_table * 16;
    const char* src = h->use_dft ? reinterpret_cast<const char*>(h->d_bfrag.p) : reinterpret_cast<const char*>(h->d_ftab.p);
    HIP_TRY(h, hipMemcpyAsync(tables, src + (size_t)first * each, (size_t)n * each, hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    if (h->use_dft) HIP_TRY(h, hipMemcpyAsync(corr, h->d_bcorr.p + (size_t)first * per_corr, (size_t)n * per_corr * sizeof(double), hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    /* a CF32 handle without private tables never uploaded the bins and the home / private indices: nothing on the device moves them, the plan's are the truth */
    if (h->d_bset_bin.p) HIP_TRY(h, hipMemcpyAsync(bset_bin, h->d_bset_bin.p + (size_t)first * 8, (size_t)n * 8 * sizeof(int), hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    else std::memcpy(bset_bin, p.bset_bins.data() + (size_t)first * 8, (size_t)n * 8 * sizeof(int));
    HIP_TRY(h, hipMemcpyAsync(items, h->d_item_bset.p, n_items * sizeof(int), hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    if (h->d_item_home.p) HIP_TRY(h, hipMemcpyAsync(items + n_items, h->d_item_home.p, n_items * sizeof(int), hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    else std::memcpy(items + n_items, p.item_home.data(), n_items * sizeof(int));
    if (h->d_item_private.p) HIP_TRY(h, hipMemcpyAsync(items + 2 * n_items, h->d_item_private.p, n_items * sizeof(int), hipMemcpyDeviceToHost, h->stream), AIRBAND_HIP_ERUNTIME);
    else std::memcpy(items + 2 * n_items, p.item_bset.data(), n_items * sizeof(int));
    HIP_TRY(h, hipStreamSynchronize(h->stream), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

int airband_hip_last_timings(airband_hip_handle* h, float* ms4) {
    if (!h || !ms4) return AIRBAND_HIP_EINVAL;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    harvest_timings(h, true);
    if (!h->timings_valid) return AIRBAND_HIP_EAGAIN;
    for (int k = 0; k < 4; k++) ms4[k] = h->t_last[k];
    return AIRBAND_HIP_OK;
}

int airband_hip_timing_totals(airband_hip_handle* h, double* ms4_sum, int64_t* n_batches, int32_t reset) {
    if (!h) return AIRBAND_HIP_EINVAL;
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    harvest_timings(h, true);
    if (ms4_sum)
        for (int k = 0; k < 4; k++) ms4_sum[k] = h->t_sum[k];
    if (n_batches) *n_batches = h->t_n[0];
    if (reset) {
        for (double& v : h->t_sum) v = 0.0;
        h->t_n[0] = 0;
    }
    return AIRBAND_HIP_OK;
}

#ifndef AB_BUILD_DEFINES
#define AB_BUILD_DEFINES ""
#endif
const char* airband_hip_build_info(void) { return AB_BUILD_DEFINES; }

int airband_hip_regrouped(const airband_hip_handle* h) { return (h && h->regroup) ? 1 : 0; }

int airband_hip_schedule_info(const airband_hip_handle* h, int32_t* run_ahead, int32_t* ring_batches, int32_t* channelizer_waves_per_cu, int64_t* batches_run_ahead) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (run_ahead) *run_ahead = h->run_ahead ? 1 : 0;
    if (ring_batches) *ring_batches = (h->R - AB_AGC_EXTRA) / h->B;
    if (channelizer_waves_per_cu) /* the hold is LDS the launch asks for beyond its own (dft_args) */
        *channelizer_waves_per_cu = (h->use_dft && dft_args(h, nullptr, 0, FrontRows{AB_AGC_EXTRA, h->B}).extra_lds > 0) ? 5 : 0;
    if (batches_run_ahead) *batches_run_ahead = (int64_t)h->ahead_batches;
    return AIRBAND_HIP_OK;
}

const char* airband_hip_channelizer_name(const airband_hip_handle* h) {
    return (h && h->use_dft) ? "dft_mfma_i8" : (h && h->use_f32) ? "dft_mfma_f32" : "fft_wave64";
}

const char* airband_hip_channelizer_reason(const airband_hip_handle* h) { return h ? h->chan_reason.c_str() : ""; }

int64_t airband_hip_wide_hop_lds_bytes(int32_t fft_size, int32_t hop_bytes, int32_t sample_format) { return dft_wide_lds(fft_size, hop_bytes, sample_format); }

int airband_hip_wide_hop_plan_f32(int32_t fft_size, int32_t hop_samples, int32_t* segments, int64_t* lds_bytes) {
    int seg = 0, lds = 0;
    if (f32_wide_plan(fft_size, hop_samples, &seg, &lds) <= 0) return AIRBAND_HIP_EBADSIZE; /* inside the ordinary kernel's limits, or no plan */
    if (segments) *segments = seg;
    if (lds_bytes) *lds_bytes = lds;
    return AIRBAND_HIP_OK;
}

int airband_hip_wide_hop_plan(int32_t fft_size, int32_t hop_bytes, int32_t sample_format, int32_t* segments, int64_t* lds_bytes) {
    int lds = 0;
    const int seg = dft_wide_plan(fft_size, hop_bytes, sample_format, &lds, nullptr);
    if (seg <= 0) return AIRBAND_HIP_EBADSIZE;
    if (segments) *segments = seg;
    if (lds_bytes) *lds_bytes = lds;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_signal_plan(airband_hip_handle* h, const int64_t* carriers, int32_t n_carriers, int32_t noise_q8, const int16_t* sin_table4096) {
    if (!h || !carriers || !sin_table4096 || n_carriers < 1 || n_carriers > 16) return fail(h, AIRBAND_HIP_EINVAL, "bad signal plan (1..16 carriers)");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    std::vector<long long> c(carriers, carriers + (size_t)n_carriers * 12);
    std::vector<int16_t> t(sin_table4096, sin_table4096 + 4096);
    HIP_TRY(h, upload(h->d_carriers, c), AIRBAND_HIP_ENOMEM);
    HIP_TRY(h, upload(h->d_sin_tab, t), AIRBAND_HIP_ENOMEM);
    h->n_carriers = n_carriers;
    h->noise_q8 = noise_q8;
    return AIRBAND_HIP_OK;
}

int airband_hip_set_signal_plan_shift(airband_hip_handle* h, int32_t n_plans, uint32_t shift_step) {
    if (!h || n_plans < 1 || n_plans > 65536) return fail(h, AIRBAND_HIP_EINVAL, "bad plan count (1..65536)");
    h->sig_n_plans = n_plans;
    h->sig_shift_step = shift_step;
    return AIRBAND_HIP_OK;
}

int airband_hip_generate_iq(airband_hip_handle* h, void* d_iq, size_t stride_bytes, uint64_t start_byte, size_t nbytes, uint64_t seed, int32_t device_index_offset,
                            void* stream) {
    if (!h || !d_iq) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (h->n_carriers == 0) return fail(h, AIRBAND_HIP_EINVAL, "call airband_hip_set_signal_plan first");
    if (h->plan.dev[0].sfmt != AIRBAND_SFMT_U8) return fail(h, AIRBAND_HIP_EINVAL, "the synthetic generator emits u8 I/Q");
    if ((start_byte & 1) || (nbytes & 1)) return fail(h, AIRBAND_HIP_EINVAL, "byte ranges must cover whole I/Q pairs");
    HIP_TRY(h, hipSetDevice(h->hip_device), AIRBAND_HIP_ENODEV);
    SiggenArgs a;
    a.iq = (uint8_t*)d_iq;
    a.stride = (long)stride_bytes;
    a.sin_tab = h->d_sin_tab.p;
    a.carriers = h->d_carriers.p;
    a.n_carriers = h->n_carriers;
    a.n_dev = h->plan.n_dev;
    a.dev_offset = device_index_offset;
    a.start_sample = start_byte / 2;
    a.n_samples = (long)(nbytes / 2);
    a.seed = seed;
    a.noise_q8 = h->noise_q8;
    a.n_plans = h->sig_n_plans;
    a.plan_shift_step = h->sig_shift_step;
    launch_siggen(a, stream ? (hipStream_t)stream : h->stream);
    if (!stream && h->run_ahead) h->serialise_next = true; /* the bytes may be the next batch's input: its stage 1, on the front stream, waits for this kernel */
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, AIRBAND_HIP_ERUNTIME, std::string("siggen launch: ") + hipGetErrorString(e));
    return AIRBAND_HIP_OK;
}

} /* extern "C" */
