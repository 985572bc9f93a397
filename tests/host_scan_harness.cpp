// tests/host_scan_harness.cpp -- csrc/scan_bank.h and the host side of the scan lists (params.cpp, build_scan) compiled as plain C++ for
// tests/test_scan_bank.py: the per-dword move the exchange kernel runs, the field partition, and the entries' constants.
#include <cstring>
#include <vector>

#include "../rtlsdr-airband_amd/csrc/common.h"
#include "../rtlsdr-airband_amd/csrc/params.h"
#include "../rtlsdr-airband_amd/csrc/scan_bank.h"

using namespace airband;

#define FIELD(S, f) {#S, #f, (int)offsetof(S, f), (int)sizeof(((S*)0)->f)}
struct Field {
    const char* s;
    const char* name;
    int off, size;
};
static const Field kFields[] = {
    FIELD(ChanState, agcavgfast), FIELD(ChanState, pr), FIELD(ChanState, pj), FIELD(ChanState, prev_waveout), FIELD(ChanState, dm_phi),
    FIELD(ChanState, bin), FIELD(ChanState, axc), FIELD(ChanState, active_counter), FIELD(ChanState, noise_floor), FIELD(ChanState, cap),
    FIELD(ChanState, pre_full), FIELD(ChanState, pre_capped), FIELD(ChanState, post_full), FIELD(ChanState, post_capped), FIELD(ChanState, level_cache),
    FIELD(ChanState, using_post), FIELD(ChanState, next), FIELD(ChanState, cur), FIELD(ChanState, delay), FIELD(ChanState, low_count),
    FIELD(ChanState, head), FIELD(ChanState, tail), FIELD(ChanState, sample_count), FIELD(ChanState, open_count), FIELD(ChanState, flappy_count),
    FIELD(ChanState, recent_open), FIELD(ChanState, closed_count), FIELD(ChanState, nx), FIELD(ChanState, ny), FIELD(ChanState, lxr),
    FIELD(ChanState, lxi), FIELD(ChanState, lyr), FIELD(ChanState, lyi), FIELD(ChanState, ct_enough), FIELD(ChanState, ct_count),
    FIELD(ChanState, ct_has_tone), FIELD(ChanState, ct_found), FIELD(ChanState, ct_not_found), FIELD(ChanState, axc_prev), FIELD(ChanState, sh_nf),
    FIELD(ChanState, sh_cap), FIELD(ChanState, sh_capped), FIELD(ChanState, row_zero), FIELD(ChanState, sh_dly), FIELD(ChanState, pad),
    FIELD(ChanConst, flags), FIELD(ChanConst, dev), FIELD(ChanConst, chan), FIELD(ChanConst, ext_index), FIELD(ChanConst, base_bin),
    FIELD(ChanConst, afc), FIELD(ChanConst, dm_dphi), FIELD(ChanConst, alpha), FIELD(ChanConst, ampfactor), FIELD(ChanConst, notch_d0),
    FIELD(ChanConst, notch_d1), FIELD(ChanConst, notch_d2), FIELD(ChanConst, lp_gain), FIELD(ChanConst, lp_yc0), FIELD(ChanConst, lp_yc1),
    FIELD(ChanConst, sq_manual_level), FIELD(ChanConst, sq_normal_ratio), FIELD(ChanConst, sq_flappy_ratio), FIELD(ChanConst, ct_slot),
    FIELD(ChanConst, ct_ntones), FIELD(ChanConst, ct_window), FIELD(ChanConst, lp_rgain), FIELD(ChanConst, pad),
};

extern "C" {

int scan_sizes(int* out) {
    out[0] = (int)sizeof(ChanState);
    out[1] = (int)sizeof(ChanConst);
    out[2] = AB_SQ_BUF;
    return 0;
}

int scan_n_fields() { return (int)(sizeof(kFields) / sizeof(kFields[0])); }

const char* scan_field(int i, int* off, int* size, int* is_const) {
    *off = kFields[i].off;
    *size = kFields[i].size;
    *is_const = std::strcmp(kFields[i].s, "ChanConst") == 0;
    return kFields[i].name;
}

void scan_masks(uint32_t* cs, uint32_t* cc) {
    const AbScanMasks k = ab_scan_masks();
    std::memcpy(cs, k.cs, sizeof(k.cs));
    std::memcpy(cc, k.cc, sizeof(k.cc));
}

/* the exchange kernel's loop over one image (misc_kernels.hip, scan_exchange_kernel), one lane */
void scan_exchange(uint32_t* live, const uint32_t* mask, const uint32_t* incoming, uint32_t* park, int dwords) {
    for (int d = 0; d < dwords; d++) {
        const uint32_t m = mask[d];
        if (m == 0u) continue;
        live[d] = ab_scan_exchange_dword(live[d], m, incoming[d], park ? park + d : nullptr);
    }
}

/* build_plan + build_scan: rc, then for every entry its ChanConst (out_cc) and, per entry, the first fast-detector coefficient of its tone table */
int scan_plan(const airband_hip_config* cfg, const airband_hip_scan_cfg* scan, int n_scan, ChanConst* out_cc, float* tone0, int max_entries, int* n_entries,
              uint32_t* chan_flags, uint32_t* chan_dm_dphi) {
    Plan p;
    int rc = build_plan(cfg, p);
    if (rc == 0) rc = build_scan(cfg, scan, n_scan, p);
    if (rc != 0) return rc;
    *n_entries = (int)p.scan_cc.size();
    for (size_t e = 0; e < p.scan_cc.size() && (int)e < max_entries; e++) {
        out_cc[e] = p.scan_cc[e];
        tone0[e] = p.scan_cc[e].ct_slot >= 0 ? p.tones[p.scan_cc[e].ct_slot].coeff[0][0] : 0.0f;
    }
    for (size_t i = 0; i < p.scan.size(); i++) {
        chan_flags[i] = p.cc[p.scan[i].ext].flags;
        chan_dm_dphi[i] = p.cc[p.scan[i].ext].dm_dphi;
    }
    return 0;
}
}
