/* csrc/scan_bank.h -- scan-mode devices: which part of a slot's state belongs to the FREQUENCY and which to the CHANNEL.
 *
 * A scan device (reference: dev->mode == R_SCAN, src/config.cpp:361-650) has one channel_t whose freqlist holds several freq_t; demodulate()
 * works on freqlist[freq_idx] (src/rtl_airband.cpp:498).  What a freq_t owns (src/rtl_airband.h:223-233: agcavgfast, ampfactor, Squelch with
 * its CTCSS detectors and delay line, active_counter, NotchFilter, LowpassFilter, modulation) is frozen while the frequency is not the active
 * one; what the channel_t owns (:234-263: wavein / waveout history, pr, pj, prev_waveout, alpha, dm_phi, dm_dphi, axcindicate, needs_raw_iq,
 * has_iq_outputs, AFC, the bin) carries on across switches.
 *
 * The library keeps ONE live ChanState / ChanConst per demod slot (the stage-2 kernels are unchanged) and a bank per scan entry.  At a switch the
 * exchange kernel (misc_kernels.hip) parks the live per-frequency dwords in the old entry's bank and brings the new entry's in, dword by dword, under
 * the masks below: all ones for a per-frequency dword, zero for a per-channel one, and the per-frequency bits only for ChanConst.flags.
 * The function ab_scan_exchange_dword() is what the kernel runs; tests/test_scan_bank.py compiles this header on the host and runs it.
 */
#ifndef AIRBAND_CSRC_SCAN_BANK_H
#define AIRBAND_CSRC_SCAN_BANK_H

#include <stddef.h>
#include <stdint.h>

#include "common.h"

#define AB_CS_DWORDS ((int)(sizeof(ChanState) / 4))
#define AB_CC_DWORDS ((int)(sizeof(ChanConst) / 4))

/* ChanConst.flags bits that a freq_t decides: the notch, the lowpass, CTCSS, a manual squelch level and the modulation.  RAW_IQ (needs_raw_iq, the
 * union over the list, src/config.cpp:671-678), IQ_OUT, QUADRI (the global -Q) and VALID (device enable) are the channel's. */
#define AB_SCAN_FREQ_FLAGS (AB_F_NOTCH | AB_F_LOWPASS | AB_F_CTCSS | AB_F_MANUAL | AB_F_NFM)

/* One dword of a live image and its bank entries: writes the per-frequency part of `live` to *park (the entry that is switched out; null for the
 * read-only ChanConst bank) and returns the live dword with the incoming entry's per-frequency part.  m = 0: the dword is the channel's, left as it is. */
static inline AB_HD uint32_t ab_scan_exchange_dword(uint32_t live, uint32_t m, uint32_t incoming, uint32_t* park) {
    if (park) *park = live & m;
    return (live & ~m) | (incoming & m);
}

/* The partition, field by field (host code: the masks are uploaded next to the banks). */
struct AbScanMasks {
    uint32_t cs[sizeof(ChanState) / 4];
    uint32_t cc[sizeof(ChanConst) / 4];
};

static inline void ab_scan_mark(uint32_t* mask, size_t off, size_t bytes, uint32_t m) {
    for (size_t b = off / 4; b < (off + bytes) / 4; b++) mask[b] = m;
}

static inline AbScanMasks ab_scan_masks() {
    AbScanMasks k;
    for (uint32_t& m : k.cs) m = 0u;
    for (uint32_t& m : k.cc) m = 0u;
#define AB_CS_FREQ(f) ab_scan_mark(k.cs, offsetof(ChanState, f), sizeof(((ChanState*)0)->f), 0xffffffffu)
#define AB_CC_FREQ(f) ab_scan_mark(k.cc, offsetof(ChanConst, f), sizeof(((ChanConst*)0)->f), 0xffffffffu)
    /* ChanState: per frequency (freq_t, src/rtl_airband.h:223-233) */
    AB_CS_FREQ(agcavgfast);     /* freq_t.agcavgfast                                   */
    AB_CS_FREQ(active_counter); /* freq_t.active_counter                               */
    AB_CS_FREQ(noise_floor);    /* freq_t.squelch: Squelch (src/squelch.h:117-158) ... */
    AB_CS_FREQ(cap);
    AB_CS_FREQ(pre_full);
    AB_CS_FREQ(pre_capped);
    AB_CS_FREQ(post_full);
    AB_CS_FREQ(post_capped);
    AB_CS_FREQ(level_cache);
    AB_CS_FREQ(using_post);
    AB_CS_FREQ(next);
    AB_CS_FREQ(cur);
    AB_CS_FREQ(delay);
    AB_CS_FREQ(low_count);
    AB_CS_FREQ(head);           /* ... the delay line's cursors (its 102 floats are banked beside) */
    AB_CS_FREQ(tail);
    AB_CS_FREQ(sample_count);
    AB_CS_FREQ(open_count);
    AB_CS_FREQ(flappy_count);
    AB_CS_FREQ(recent_open);
    AB_CS_FREQ(closed_count);
    AB_CS_FREQ(nx);             /* freq_t.notch_filter                                 */
    AB_CS_FREQ(ny);
    AB_CS_FREQ(lxr);            /* freq_t.lowpass_filter                               */
    AB_CS_FREQ(lxi);
    AB_CS_FREQ(lyr);
    AB_CS_FREQ(lyi);
    AB_CS_FREQ(ct_enough);      /* the Squelch's CTCSS detectors (src/ctcss.h:84-95)   */
    AB_CS_FREQ(ct_count);
    AB_CS_FREQ(ct_has_tone);
    AB_CS_FREQ(ct_found);
    AB_CS_FREQ(ct_not_found);
    AB_CS_FREQ(sh_nf);          /* the Squelch's delay line as the shadow holds it      */
    AB_CS_FREQ(sh_cap);
    AB_CS_FREQ(sh_capped);
    AB_CS_FREQ(sh_dly);
    /* ChanState, per channel (channel_t, src/rtl_airband.h:234-263), mask 0: pr, pj, prev_waveout, dm_phi, bin (AFC), axc (axcindicate),
     * axc_prev (what AFC captures), row_zero (what the channel's waveout row holds), pad */

    /* ChanConst: per frequency */
    k.cc[offsetof(ChanConst, flags) / 4] = AB_SCAN_FREQ_FLAGS; /* freq_t.modulation, the filters' and the squelch's switches */
    AB_CC_FREQ(ampfactor);      /* freq_t.ampfactor                                     */
    AB_CC_FREQ(notch_d0);       /* freq_t.notch_filter                                  */
    AB_CC_FREQ(notch_d1);
    AB_CC_FREQ(notch_d2);
    AB_CC_FREQ(lp_gain);        /* freq_t.lowpass_filter                                */
    AB_CC_FREQ(lp_yc0);
    AB_CC_FREQ(lp_yc1);
    AB_CC_FREQ(lp_rgain);
    AB_CC_FREQ(sq_manual_level); /* freq_t.squelch's thresholds                          */
    AB_CC_FREQ(sq_normal_ratio);
    AB_CC_FREQ(sq_flappy_ratio);
    AB_CC_FREQ(ct_slot);        /* the entry's own CTCSS tone tables and Goertzel state  */
    AB_CC_FREQ(ct_ntones);
    AB_CC_FREQ(ct_window);
    /* ChanConst, per channel, mask 0: dev, chan, ext_index, base_bin, afc, dm_dphi (derived from freqlist[0], src/config.cpp:679-712), alpha (tau), pad */
#undef AB_CS_FREQ
#undef AB_CC_FREQ
    return k;
}

#endif
