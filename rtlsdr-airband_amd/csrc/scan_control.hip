/* csrc/scan_control.hip -- scan control: the reference's controller thread (src/rtl_airband.cpp:101-139) for every scan list of a handle, on the GPU
 * (airband_hip_set_scan_control).  Per list the decision when to hop, the switch of the list's entry handed to the exchange kernel of the next batch
 * (misc_kernels.hip, scan_exchange_kernel) through a device-resident switch list, and one fleet-wide packed list of the batch's records.
 *
 * For every list, with its state {idx, hold, idle, since, last}, axc = the list's channel's axcindicate of this batch and the control's batch number k
 * (include/airband_hip.h has the normative text; a switched-off dongle and a list of fewer than two entries are frozen) --
 *     hold >= 0:       idx != hold: a HOP to hold;  idle = since = 0
 *     axc == ' ':      idle < idle_batches: idle += 1;  else since += 1, and since >= dwell_batches: a HOP to (idx + 1) % n, since = 0
 *     else:            idle == idle_batches: an ACTIVITY record (RETAG if idx != last), last = idx;  idle = since = 0
 * capi.scan_control_reference() (rtlsdr-airband_amd/capi.py) is this definition in plain Python; tests/test_host_scan_control.py runs this file on the CPU
 * against it.
 *
 * Mapping (wave64, CDNA4).  scan_control_kernel: ONE THREAD per list, workgroups of one wavefront: a list's decision is a dozen integer operations on 16 bytes
 * of state, a byte of axcindicate and its dongle's enabled flag, and lists do not talk to each other -- no LDS, no cross-lane operation, no atomics.  Every
 * thread writes its list's count (0 or 1), its record where there is one, and ALL THREE words of its switch item every batch: slot -1 where nothing switches,
 * so an item never outlives the batch it was decided in and the exchange kernel, launched with one workgroup per list, leaves at its first test.
 * scan_control_pack_kernel: the lists' records into the fleet's list in list order = dongle order (band_pack.h, cap = 1).
 * Every index is clamped to its buffer before use: the dongle to [0, n_dev), the channel to [0, n_ch), idx, hold and last to the list's [0, n); the slot and the
 * entries of a switch item are checked again by the exchange kernel against n_slots and n_entries.  Equal input, equal bytes.
 */
#include <hip/hip_runtime.h>

#include "band_pack.h"
#include "common.h"
#include "kernels.h"

namespace airband {

__global__ __launch_bounds__(64) void scan_control_kernel(ScanControlArgs a) {
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= a.n_lists) return;
    const ScanCtlList L = a.lists[i];
    int n_rec = 0, sw_slot = -1, sw_old = 0, sw_new = 0;
    const bool there = L.dev >= 0 && L.dev < a.n_dev && L.ext >= 0 && L.ext < a.n_ch && L.n >= 2;
    if (there && !a.dev[L.dev].disabled) {
        airband_hip_scan_state st = a.state[i];
        int idx = st.idx < 0 ? 0 : st.idx >= L.n ? L.n - 1 : st.idx;
        const int hold = st.hold >= L.n ? L.n - 1 : st.hold;
        int last = st.last < 0 ? 0 : st.last >= L.n ? L.n - 1 : st.last;
        int idle = st.idle, since = st.since;
        const int was = idx;
        airband_hip_scan_event rec;
        rec.dev = L.dev;
        rec.kind = 0;
        rec.flags = 0;
        rec.reserved = 0;
        rec.batch = a.batch;
        rec.freq_idx = rec.prev_idx = 0;
        if (hold >= 0) {
            if (idx != hold) {
                idx = hold;
                rec.kind = AIRBAND_SCAN_HOP;
            }
            idle = 0;
            since = 0;
        } else if (a.axc[L.ext] == (uint8_t)' ') {
            if (idle < a.idle_batches) {
                idle++;
            } else {
                since++;
                if (since >= a.dwell_batches) {
                    idx = idx + 1 >= L.n ? 0 : idx + 1;
                    since = 0;
                    rec.kind = AIRBAND_SCAN_HOP;
                }
            }
        } else {
            if (idle == a.idle_batches) {
                rec.kind = AIRBAND_SCAN_ACTIVITY;
                rec.flags = idx != last ? AIRBAND_SCAN_RETAG : 0;
                rec.freq_idx = (int16_t)idx;
                rec.prev_idx = (int16_t)last;
                last = idx;
            }
            idle = 0;
            since = 0;
        }
        if (rec.kind == AIRBAND_SCAN_HOP) {
            rec.freq_idx = (int16_t)idx;
            rec.prev_idx = (int16_t)was;
            sw_slot = L.slot;
            sw_old = L.first_entry + was;
            sw_new = L.first_entry + idx;
        }
        if (rec.kind != 0) {
            a.stage[i] = rec;
            n_rec = 1;
        }
        st.idx = (int16_t)idx;
        st.idle = idle;
        st.since = since;
        st.last = (int16_t)last;
        a.state[i] = st;
    }
    a.stage_n[i] = n_rec;
    a.sw[3 * i] = sw_slot;
    a.sw[3 * i + 1] = sw_old;
    a.sw[3 * i + 2] = sw_new;
}

__global__ __launch_bounds__(PACK_THREADS) void scan_control_pack_kernel(ScanControlArgs a) {
    pack_rows(a.stage_n, 1, reinterpret_cast<const uint4*>(a.stage), 1, reinterpret_cast<uint4*>(a.events), a.max_records, a.n_events, a.n_lists);
}

void launch_scan_control(const ScanControlArgs& a, hipStream_t stream) {
    if (a.n_lists <= 0 || a.idle_batches < 1 || a.dwell_batches < 1 || a.max_records < 1) return;
    hipLaunchKernelGGL(scan_control_kernel, dim3((unsigned)((a.n_lists + 63) / 64)), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(scan_control_pack_kernel, dim3(1), dim3(PACK_THREADS), 0, stream, a);
}

__global__ __launch_bounds__(64) void scan_set_valid_kernel(ChanConst* cc, int slot, int on) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t f = cc[slot].flags;
    cc[slot].flags = on ? (f | AB_F_VALID) : (f & ~AB_F_VALID);
}

void launch_scan_set_valid(ChanConst* cc, int slot, int n_slots, int on, hipStream_t stream) {
    if (slot < 0 || slot >= n_slots) return;
    hipLaunchKernelGGL(scan_set_valid_kernel, dim3(1), dim3(64), 0, stream, cc, slot, on);
}

}  // namespace airband
