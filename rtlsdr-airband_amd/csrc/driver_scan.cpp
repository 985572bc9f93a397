/* csrc/driver_scan.cpp -- scan-mode devices in the host driver: the bank exchange in front of the demod kernels, and scan control, where the GPU hops the lists
 * (airband_hip_set_freq_index / _set_scan_control / _scan_hold / _collect_scan_* / _freq_stats; hooks of airband_hip.cpp: prepare, front_enqueued, run_back_half). */
#include "driver.h"
#include "scan_bank.h"

using namespace airband;

static ScanExchangeArgs scan_args(airband_hip_handle* h) {
    ScanExchangeArgs a;
    a.cc = h->d_cc.p;
    a.cs = h->d_cs.p;
    a.sqbuf = h->d_sqbuf.p;
    a.bank_cc = h->d_bank_cc.p;
    a.bank_cs = h->d_bank_cs.p;
    a.bank_sq = h->d_bank_sq.p;
    a.cs_mask = h->d_scan_mask.p;
    a.cc_mask = h->d_scan_mask.p + AB_CS_DWORDS;
    a.sw = nullptr;
    a.n_switch = 0;
    a.n_slots = h->n_slots;
    a.n_entries = (int)h->plan.scan_cc.size();
    return a;
}

static ScanControlArgs scan_control_args(airband_hip_handle* h) {
    ScanControl& c = h->scan_ctl;
    ScanControlArgs a;
    a.dev = h->d_dev.p;
    a.axc = h->d_out_axc.p;
    a.lists = c.d_lists.p;
    a.state = c.d_state.p;
    a.stage = c.d_stage.p;
    a.stage_n = c.d_stage_n.p;
    a.sw = c.d_sw.p;
    a.events = c.d_events.p;
    a.n_events = c.d_count.p;
    a.n_lists = (int)c.list_of.size();
    a.n_dev = h->plan.n_dev;
    a.n_ch = h->plan.total_ch;
    a.idle_batches = c.idle_batches;
    a.dwell_batches = c.dwell_batches;
    a.max_records = c.max_records;
    a.batch = c.batch;
    return a;
}

static bool has_scan_list(const airband_hip_handle* h, int32_t dev) { return dev >= 0 && dev < h->plan.n_dev && !h->scan_of_dev.empty() && h->scan_of_dev[dev] >= 0; }

/* front batch k is being enqueued: the scan entries in force now are its entries (airband_hip_set_freq_index latches per batch) */
void airband::scan_latch(airband_hip_handle* h, uint64_t k, int first_row, int n_rows) {
    if (h->plan.scan.empty()) return;
    if (!has_scan_control(h)) h->scan_latch[k & 1] = h->scan_cur; /* (under scan control the entries are the GPU's: scan_before_demod) */
    h->scan_first_row[k & 1] = first_row;
    h->scan_n_rows[k & 1] = n_rows;
}

/* in front of the demod kernels of batch batches_done, on its stage-2 stream: the exchange of every scan channel whose latched entry is not the one its slot
 * holds (one launch for all of them), and |bin| of the lists that mix AM and NFM */
int airband::scan_before_demod(airband_hip_handle* h, hipStream_t s) {
    const int b = (int)(h->batches_done & 1);
    if (has_scan_control(h)) {
        /* scan control: the switch list is the one the decision kernel left behind the batch before (or airband_hip_set_scan_control at the start), on this
         * stream's order -- nothing is built, copied or waited for here.  One workgroup per list; an item with slot -1 leaves at the kernel's first test. */
        ScanExchangeArgs a = scan_args(h);
        a.sw = h->scan_ctl.d_sw.p;
        a.n_switch = (int)h->scan_ctl.list_of.size();
        launch_scan_exchange(a, s);
    }
    const std::vector<int>& want = h->scan_latch[b];
    const int q = h->switch_buf;
    int* list = h->h_switch[q].get();
    int n = 0;
    bool waited = false;
    for (size_t i = 0; !has_scan_control(h) && i < h->plan.scan.size(); i++) { /* the host's lists */
        if (want[i] == h->scan_held[i]) continue;
        if (!waited && h->switch_used[q]) HIP_TRY(h, hipEventSynchronize(h->ev_switch[q]), AIRBAND_HIP_ERUNTIME); /* the list of two batches ago has been read */
        waited = true;
        const ScanList& sl = h->plan.scan[i];
        const int slot = h->ext_to_slot[sl.ext];
        list[3 * n] = slot;
        list[3 * n + 1] = sl.first_entry + h->scan_held[i];
        list[3 * n + 2] = sl.first_entry + want[i];
        n++;
        h->scan_held[i] = want[i];
        /* the host copy of the slot's flags (airband_hip_device_enable rewrites the word from it) follows the entry the slot holds */
        ChanConst& hc = h->cc_slots[slot];
        hc.flags = (hc.flags & ~AB_SCAN_FREQ_FLAGS) | (h->plan.scan_cc[sl.first_entry + want[i]].flags & AB_SCAN_FREQ_FLAGS);
    }
    if (n > 0) {
        HIP_TRY(h, hipMemcpyAsync(h->d_switch[q].p, list, (size_t)n * 3 * sizeof(int), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
        ScanExchangeArgs a = scan_args(h);
        a.sw = h->d_switch[q].p;
        a.n_switch = n;
        launch_scan_exchange(a, s);
        HIP_TRY(h, hipEventRecord(h->ev_switch[q], s), AIRBAND_HIP_ERUNTIME);
        h->switch_used[q] = true;
        h->switch_buf = q ^ 1;
    }
    if (h->d_scan_mix_slots.n > 0)
        launch_scan_mag(h->d_scan_mix_slots.p, (int)h->d_scan_mix_slots.n, h->d_mag.p, h->d_iq.p, h->scan_first_row[b], h->scan_n_rows[b], h->row0, h->R, s);
    return AIRBAND_HIP_OK;
}

/* The scan control of the batch whose back half goes on stream s (airband_hip_set_scan_control), behind everything that writes the batch's axcindicate.  The
 * switch list it writes is read by the exchange in front of the NEXT batch's demod kernels, which goes on the same stream (or, where a caller changes streams
 * between batches, behind ev_last like everything else of the next batch). */
void airband::launch_scan_control_behind_demod(airband_hip_handle* h, hipStream_t s) {
    launch_scan_control(scan_control_args(h), s);
    h->scan_ctl.batch++;
}

/* scan lists: the banks, every entry's initial image, the masks, the switch lists' staging */
int airband::prep_scan(airband_hip_handle* h) {
    const Plan& p = h->plan;
    HIP_TRY(PREPARING, upload(h->d_bank_cc, p.scan_cc), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, upload(h->d_bank_cs, p.scan_cs0), AIRBAND_HIP_ENOMEM);
    HIP_TRY(PREPARING, h->d_bank_sq.alloc_zeroed(p.scan_cc.size() * AB_SQ_BUF), AIRBAND_HIP_ENOMEM);
    const AbScanMasks mk = ab_scan_masks();
    std::vector<uint32_t> masks(mk.cs, mk.cs + AB_CS_DWORDS);
    masks.insert(masks.end(), mk.cc, mk.cc + AB_CC_DWORDS);
    HIP_TRY(PREPARING, upload(h->d_scan_mask, masks), AIRBAND_HIP_ENOMEM);
    const size_t nl = p.scan.size();
    for (int q = 0; q < 2; q++) {
        HIP_TRY(PREPARING, h->d_switch[q].alloc(nl * 3), AIRBAND_HIP_ENOMEM);
        HIP_TRY(PREPARING, h->h_switch[q].alloc(nl * 3), AIRBAND_HIP_ENOMEM);
        HIP_TRY(PREPARING, h->ev_switch[q].ensure(), AIRBAND_HIP_ENODEV);
    }
    std::vector<int> mix_slots;
    h->scan_of_dev.assign(p.n_dev, -1);
    for (size_t i = 0; i < nl; i++) {
        h->scan_of_dev[p.scan[i].dev] = (int)i;
        if (p.scan[i].mixed_am_nfm) mix_slots.push_back(h->ext_to_slot[p.scan[i].ext]);
    }
    if (!mix_slots.empty()) HIP_TRY(PREPARING, upload(h->d_scan_mix_slots, mix_slots), AIRBAND_HIP_ENOMEM);
    h->scan_cur.assign(nl, 0);
    h->scan_held.assign(nl, 0);
    h->scan_latch[0].assign(nl, 0);
    h->scan_latch[1].assign(nl, 0);
    return AIRBAND_HIP_OK;
}

extern "C" {

int airband_hip_set_freq_index(airband_hip_handle* h, int32_t dev, int32_t freq_idx) {
    if (!h) return AIRBAND_HIP_EINVAL;
    if (!has_scan_list(h, dev)) return fail(h, AIRBAND_HIP_EINVAL, "device has no scan list");
    const int i = h->scan_of_dev[dev];
    if (freq_idx < 0 || freq_idx >= h->plan.scan[i].n) return fail(h, AIRBAND_HIP_EINVAL, "frequency index out of range");
    if (has_scan_control(h)) return fail(h, AIRBAND_HIP_EINVAL, "the lists are under scan control (airband_hip_set_scan_control): the GPU sets the index");
    h->scan_cur[i] = freq_idx; /* latched by the next batch that is enqueued */
    return AIRBAND_HIP_OK;
}

/* Scan control: where list i (index in plan.scan) stands once everything enqueued on the handle has run -- *idx the entry in force for the next batch, *held the
 * entry its slot holds now (they differ between a hop's decision and the exchange in front of the next batch).  Two small copies and a synchronize. */
static int scan_ctl_where(airband_hip_handle* h, int i, int* idx, int* held) {
    const ScanControl& c = h->scan_ctl;
    const int k = c.ctl_of[(size_t)i];
    const ScanList& sl = h->plan.scan[(size_t)i];
    hipStream_t s = h->stream;
    airband_hip_scan_state st;
    int sw[3];
    HIP_TRY(h, hipMemcpyAsync(&st, c.d_state.p + k, sizeof(st), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemcpyAsync(sw, c.d_sw.p + 3 * (size_t)k, sizeof(sw), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    if (st.idx < 0 || st.idx >= sl.n) return fail(h, AIRBAND_HIP_ERUNTIME, "scan control: index out of range: " + std::to_string(st.idx));
    *idx = st.idx;
    *held = st.idx;
    if (sw[0] >= 0) {
        const int old = sw[1] - sl.first_entry;
        if (old < 0 || old >= sl.n) return fail(h, AIRBAND_HIP_ERUNTIME, "scan control: switch item out of range: " + std::to_string(sw[1]));
        *held = old;
    }
    return AIRBAND_HIP_OK;
}

/* Switching scan control off: the host's mirrors take over where the GPU left every list.  The stream is idle (the caller has synchronized). */
static int scan_ctl_refresh_host(airband_hip_handle* h) {
    const ScanControl& c = h->scan_ctl;
    const size_t nl = c.list_of.size();
    std::vector<airband_hip_scan_state> st(nl);
    std::vector<int> sw(nl * 3);
    HIP_TRY(h, hipMemcpy(st.data(), c.d_state.p, nl * sizeof(st[0]), hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemcpy(sw.data(), c.d_sw.p, nl * 3 * sizeof(int), hipMemcpyDeviceToHost), AIRBAND_HIP_ERUNTIME);
    for (size_t k = 0; k < nl; k++) {
        const int i = c.list_of[k];
        const ScanList& sl = h->plan.scan[(size_t)i];
        int idx = st[k].idx, held = sw[3 * k] >= 0 ? sw[3 * k + 1] - sl.first_entry : idx;
        if (idx < 0 || idx >= sl.n || held < 0 || held >= sl.n) return fail(h, AIRBAND_HIP_ERUNTIME, "scan control: a list's index is out of range");
        h->scan_cur[(size_t)i] = h->scan_latch[0][(size_t)i] = h->scan_latch[1][(size_t)i] = idx;
        h->scan_held[(size_t)i] = held;
        ChanConst& hc = h->cc_slots[(size_t)h->ext_to_slot[(size_t)sl.ext]];
        hc.flags = (hc.flags & ~AB_SCAN_FREQ_FLAGS) | (h->plan.scan_cc[(size_t)(sl.first_entry + held)].flags & AB_SCAN_FREQ_FLAGS);
    }
    return AIRBAND_HIP_OK;
}

int airband_hip_set_scan_control(airband_hip_handle* h, int32_t idle_batches, int32_t dwell_batches, int64_t max_records) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const Plan& p = h->plan;
    if (p.scan.empty()) return fail(h, AIRBAND_HIP_EINVAL, "the handle has no scan lists (airband_hip_prepare_scan)");
    if (idle_batches < 0 || dwell_batches < 0) return fail(h, AIRBAND_HIP_EINVAL, "idle_batches and dwell_batches must not be negative");
    for (const ScanList& sl : p.scan) /* idx, hold and last of airband_hip_scan_state and the records' indices are int16 */
        if (idle_batches > 0 && sl.n > 32767) return fail(h, AIRBAND_HIP_EINVAL, "scan control takes lists of at most 32 767 entries (device " + std::to_string(sl.dev) + " has " + std::to_string(sl.n) + ")");
    ON_OWN_STREAM(h, s);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME); /* the decisions and exchanges enqueued so far have run */
    if (has_scan_control(h)) { /* on -> off, and on -> on through off: the lists keep their entries */
        const int rc = scan_ctl_refresh_host(h);
        if (rc != AIRBAND_HIP_OK) return rc;
        if (idle_batches == 0) {
            h->scan_ctl = ScanControl();
            return AIRBAND_HIP_OK;
        }
    } else if (idle_batches == 0) {
        return AIRBAND_HIP_OK;
    }
    const size_t nl = p.scan.size();
    ScanControl c; /* built beside the handle and moved in whole: a failed allocation leaves the handle as it was (an earlier control is off then, its lists the host's) */
    c.list_of.resize(nl);
    for (size_t i = 0; i < nl; i++) c.list_of[i] = (int)i;
    std::sort(c.list_of.begin(), c.list_of.end(), [&](int x, int y) { return p.scan[(size_t)x].dev < p.scan[(size_t)y].dev; });
    c.ctl_of.resize(nl);
    std::vector<ScanCtlList> lists(nl);
    std::vector<airband_hip_scan_state> start(nl);
    std::vector<int> sw(nl * 3, 0);
    /* a pipelined handle may have a batch whose stage 1 is enqueued and whose stage 2 is not: that batch runs with the entry it was enqueued with (scan_latch), and
     * the lists start from there -- an index airband_hip_set_freq_index() named after that batch was enqueued has not been latched by any batch and is dropped */
    const bool pending = h->front_batches > h->batches_done;
    for (size_t k = 0; k < nl; k++) {
        const int i = c.list_of[k];
        const ScanList& sl = p.scan[(size_t)i];
        c.ctl_of[(size_t)i] = (int)k;
        ScanCtlList& l = lists[k];
        std::memset(&l, 0, sizeof(l));
        l.dev = sl.dev;
        l.ext = sl.ext;
        l.slot = h->ext_to_slot[(size_t)sl.ext];
        l.first_entry = sl.first_entry;
        l.n = sl.n;
        airband_hip_scan_state& st = start[k];
        std::memset(&st, 0, sizeof(st));
        const int from = pending ? h->scan_latch[h->batches_done & 1][(size_t)i] : h->scan_cur[(size_t)i];
        st.idx = (int16_t)from;
        st.hold = -1;
        st.has_list = 1;
        /* that entry may not be in the slot yet: the first exchange brings it in */
        const bool move = h->scan_held[(size_t)i] != from;
        sw[3 * k] = move ? l.slot : -1;
        sw[3 * k + 1] = sl.first_entry + h->scan_held[(size_t)i];
        sw[3 * k + 2] = sl.first_entry + from;
    }
    const int64_t cap = (max_records <= 0 || max_records > (int64_t)nl) ? (int64_t)nl : max_records;
    hipError_t e = upload(c.d_lists, lists);
    if (e == hipSuccess) e = upload(c.d_state, start);
    if (e == hipSuccess) e = upload(c.d_sw, sw);
    if (e == hipSuccess) e = c.d_stage.alloc_zeroed(nl);
    if (e == hipSuccess) e = c.d_stage_n.alloc_zeroed(nl);
    if (e == hipSuccess) e = c.d_events.alloc_zeroed((size_t)cap);
    if (e == hipSuccess) e = c.d_count.alloc_zeroed(1);
    if (e == hipSuccess) e = hipDeviceSynchronize(); /* the initial values are in place before a kernel on the handle's streams reads them */
    if (e != hipSuccess) {
        const int rc = alloc_failed(h, e, "scan control buffers: ");
        h->scan_ctl = ScanControl(); /* an earlier control is off */
        return rc;
    }
    c.idle_batches = idle_batches;
    c.dwell_batches = dwell_batches < 1 ? 1 : dwell_batches;
    c.max_records = (int)cap;
    h->scan_ctl = std::move(c);
    return AIRBAND_HIP_OK;
}

int airband_hip_scan_hold(airband_hip_handle* h, int32_t dev, int32_t freq_idx) {
    if (!h) return AIRBAND_HIP_EINVAL;
    ScanControl& c = h->scan_ctl;
    if (!has_scan_control(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCAN_CONTROL);
    if (!has_scan_list(h, dev)) return fail(h, AIRBAND_HIP_EINVAL, "device has no scan list");
    const int i = h->scan_of_dev[dev];
    if (freq_idx < -1 || freq_idx >= h->plan.scan[(size_t)i].n) return fail(h, AIRBAND_HIP_EINVAL, "frequency index out of range");
    ON_OWN_STREAM(h, s);
    /* in the stream's order: behind the decisions already enqueued, in front of the next batch's */
    const int16_t hold = (int16_t)freq_idx;
    HIP_TRY(h, hipMemcpyAsync(&c.d_state.p[c.ctl_of[(size_t)i]].hold, &hold, sizeof(hold), hipMemcpyHostToDevice, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME); /* `hold` is a stack variable */
    return AIRBAND_HIP_OK;
}

int airband_hip_collect_scan_events(airband_hip_handle* h, int64_t* n_records, airband_hip_scan_event* records) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const ScanControl& c = h->scan_ctl;
    if (!has_scan_control(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCAN_CONTROL);
    if (c.batch == 0) return AIRBAND_HIP_EAGAIN;
    ON_OWN_STREAM(h, s);
    return collect_counted(h, c.d_count.p, (int64_t)c.list_of.size(), c.max_records, "record count out of range: ", n_records, c.d_events.p, records, s);
}

int airband_hip_collect_scan_state(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_scan_state* state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const ScanControl& c = h->scan_ctl;
    if (!has_scan_control(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCAN_CONTROL);
    if (!dev_range_ok(h, first_dev, n_dev)) return fail(h, AIRBAND_HIP_EINVAL, "device range out of bounds");
    if (!state || n_dev == 0) return AIRBAND_HIP_OK;
    ON_OWN_STREAM(h, s);
    /* the lists are in ascending dongle order: those of the range are one run of the array -- one copy, then dealt out to the range's dongles */
    int k0 = -1, n = 0;
    for (int d = first_dev; d < first_dev + n_dev; d++)
        if (h->scan_of_dev[(size_t)d] >= 0) {
            if (k0 < 0) k0 = c.ctl_of[(size_t)h->scan_of_dev[(size_t)d]];
            n++;
        }
    std::vector<airband_hip_scan_state> tmp((size_t)n);
    if (n) HIP_TRY(h, hipMemcpyAsync(tmp.data(), c.d_state.p + k0, (size_t)n * sizeof(tmp[0]), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    for (int d = first_dev; d < first_dev + n_dev; d++) {
        airband_hip_scan_state& o = state[d - first_dev];
        const int i = h->scan_of_dev[(size_t)d];
        if (i < 0) std::memset(&o, 0, sizeof(o));
        else o = tmp[(size_t)(c.ctl_of[(size_t)i] - k0)];
    }
    return AIRBAND_HIP_OK;
}

int airband_hip_device_scan_control(airband_hip_handle* h, int32_t** d_n_records, airband_hip_scan_event** d_records, airband_hip_scan_state** d_state) {
    if (!h) return AIRBAND_HIP_EINVAL;
    const ScanControl& c = h->scan_ctl;
    if (!has_scan_control(h)) return fail(h, AIRBAND_HIP_EINVAL, NO_SCAN_CONTROL);
    if (d_n_records) *d_n_records = c.d_count.p;
    if (d_records) *d_records = c.d_events.p;
    if (d_state) *d_state = c.d_state.p;
    return AIRBAND_HIP_OK;
}

int airband_hip_freq_stats(airband_hip_handle* h, int32_t dev, int32_t freq_idx, airband_hip_channel_stats* out) {
    if (!h || !out) return fail(h, AIRBAND_HIP_EINVAL, "NULL argument");
    if (!has_scan_list(h, dev)) return fail(h, AIRBAND_HIP_EINVAL, "device has no scan list");
    const int i = h->scan_of_dev[dev];
    const ScanList& sl = h->plan.scan[i];
    if (freq_idx < 0 || freq_idx >= sl.n) return fail(h, AIRBAND_HIP_EINVAL, "frequency index out of range");
    ON_OWN_STREAM(h, s);
    if (!h->d_fs_zero.p) {
        HIP_TRY(h, h->d_fs_cc.alloc(1), AIRBAND_HIP_ENOMEM);
        HIP_TRY(h, h->d_fs_cs.alloc(1), AIRBAND_HIP_ENOMEM);
        HIP_TRY(h, h->d_fs_stats.alloc(1), AIRBAND_HIP_ENOMEM);
        HIP_TRY(h, h->d_fs_zero.alloc(1), AIRBAND_HIP_ENOMEM);
        HIP_TRY(h, hipMemsetAsync(h->d_fs_zero.p, 0, sizeof(int), s), AIRBAND_HIP_ERUNTIME);
    }
    const int slot = h->ext_to_slot[sl.ext];
    int held = h->scan_held[i];
    if (has_scan_control(h)) { /* scan control: which entry the slot holds is on the device */
        int idx = 0;
        const int rc = scan_ctl_where(h, i, &idx, &held);
        if (rc != AIRBAND_HIP_OK) return rc;
    }
    /* the stats kernel of airband_hip_collect() on one image: the slot itself for the entry it holds, else the slot composed with the entry's bank */
    if (freq_idx == held) {
        launch_stats(h->d_cc.p + slot, h->d_cs.p + slot, h->d_fs_zero.p, 1, h->d_fs_stats.p, s);
    } else {
        launch_scan_compose(scan_args(h), slot, sl.first_entry + freq_idx, h->d_fs_cc.p, h->d_fs_cs.p, s);
        launch_stats(h->d_fs_cc.p, h->d_fs_cs.p, h->d_fs_zero.p, 1, h->d_fs_stats.p, s);
    }
    HIP_TRY(h, hipGetLastError(), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipMemcpyAsync(out, h->d_fs_stats.p, sizeof(airband_hip_channel_stats), hipMemcpyDeviceToHost, s), AIRBAND_HIP_ERUNTIME);
    HIP_TRY(h, hipStreamSynchronize(s), AIRBAND_HIP_ERUNTIME);
    return AIRBAND_HIP_OK;
}

} /* extern "C" */
