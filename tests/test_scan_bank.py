"""Scan-mode devices, CPU side: the C ABI of the scan lists, their validation, and the field partition of the per-frequency state banks
(csrc/scan_bank.h) compiled as plain C++ -- exactly the per-dword move the exchange kernel runs (misc_kernels.hip, scan_exchange_kernel).

The table below is this test's own classification of every ChanState / ChanConst field against the reference's structs: a field added later
without being classified here makes test_partition_covers_every_field fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "rtlsdr-airband_amd", "csrc")

F, CH = "freq", "channel"
# ChanState: freq_t (src/rtl_airband.h:223-233) vs channel_t (src/rtl_airband.h:234-263)
STATE = {
    "agcavgfast": F,       # freq_t.agcavgfast, rtl_airband.h:225
    "active_counter": F,   # freq_t.active_counter, rtl_airband.h:229
    "noise_floor": F, "cap": F, "pre_full": F, "pre_capped": F, "post_full": F, "post_capped": F, "level_cache": F,  # freq_t.squelch, rtl_airband.h:228
    "using_post": F, "next": F, "cur": F, "delay": F, "low_count": F, "head": F, "tail": F, "sample_count": F,
    "open_count": F, "flappy_count": F, "recent_open": F, "closed_count": F,
    "nx": F, "ny": F,                          # freq_t.notch_filter, rtl_airband.h:231
    "lxr": F, "lxi": F, "lyr": F, "lyi": F,    # freq_t.lowpass_filter, rtl_airband.h:232
    "ct_enough": F, "ct_count": F, "ct_has_tone": F, "ct_found": F, "ct_not_found": F,  # the squelch's CTCSS detectors (freq_t.squelch)
    "sh_nf": F, "sh_cap": F, "sh_capped": F, "sh_dly": F,  # the squelch's delay line (freq_t.squelch)
    "pr": CH, "pj": CH, "prev_waveout": CH,    # channel_t, rtl_airband.h:246-248
    "dm_phi": CH,                              # channel_t.dm_phi, rtl_airband.h:244
    "bin": CH,                                 # dev->bins[i], moved by AFC (channel_t.afc, rtl_airband.h:250)
    "axc": CH, "axc_prev": CH,                 # channel_t.axcindicate, rtl_airband.h:243
    "row_zero": CH,                            # what the channel's waveout row holds (channel_t.waveout, rtl_airband.h:238)
    "pad": CH,
}
# ChanConst
CONST = {
    "flags": "flags",                          # mixed: see FREQ_FLAGS
    "dev": CH, "chan": CH, "ext_index": CH,
    "base_bin": CH,                            # dev->base_bins[i], from freqlist[0] (src/config.cpp:666-667)
    "afc": CH,                                 # channel_t.afc, rtl_airband.h:250
    "dm_dphi": CH,                             # channel_t.dm_dphi, rtl_airband.h:245 (src/config.cpp:679-712, from freqlist[0])
    "alpha": CH,                               # channel_t.alpha (tau), rtl_airband.h:249
    "ampfactor": F,                            # freq_t.ampfactor, rtl_airband.h:226
    "notch_d0": F, "notch_d1": F, "notch_d2": F,  # freq_t.notch_filter
    "lp_gain": F, "lp_yc0": F, "lp_yc1": F, "lp_rgain": F,  # freq_t.lowpass_filter
    "sq_manual_level": F, "sq_normal_ratio": F, "sq_flappy_ratio": F,  # freq_t.squelch thresholds
    "ct_slot": F, "ct_ntones": F, "ct_window": F,  # freq_t.squelch's CTCSS tone (its own tables)
    "pad": CH,
}
# ChanConst.flags (csrc/common.h): NOTCH LOWPASS CTCSS MANUAL NFM belong to the frequency (freq_t.modulation, the filters, the squelch);
# RAW_IQ (channel_t.needs_raw_iq), IQ_OUT (channel_t.has_iq_outputs), QUADRI (global -Q), VALID (device enable) to the channel
FREQ_FLAGS = 0x1 | 0x2 | 0x4 | 0x8 | 0x40


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostscan") / "libhostscan.so")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-I" + os.path.join(REPO, "include"), "-o", out,
           os.path.join(HERE, "host_scan_harness.cpp"), os.path.join(CSRC, "params.cpp")]
    subprocess.run(cmd, check=True)
    lib = C.CDLL(out)
    lib.scan_field.restype = C.c_char_p
    lib.scan_field.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.scan_exchange.argtypes = [C.c_void_p] * 4 + [C.c_int]
    lib.scan_masks.argtypes = [C.c_void_p, C.c_void_p]
    lib.scan_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]
    return lib


def layout(lib):
    sz = (C.c_int * 3)()
    lib.scan_sizes(sz)
    fields = {"state": [], "const": []}
    for i in range(lib.scan_n_fields()):
        off, size, is_const = C.c_int(), C.c_int(), C.c_int()
        name = lib.scan_field(i, C.byref(off), C.byref(size), C.byref(is_const)).decode()
        fields["const" if is_const.value else "state"].append((name, off.value, size.value))
    return sz[0], sz[1], fields


def masks(lib, cs_bytes, cc_bytes):
    cs = np.zeros(cs_bytes // 4, np.uint32)
    cc = np.zeros(cc_bytes // 4, np.uint32)
    lib.scan_masks(cs.ctypes.data, cc.ctypes.data)
    return cs, cc


def test_partition_covers_every_field(harness):
    cs_bytes, cc_bytes, fields = layout(harness)
    for key, table, total in (("state", STATE, cs_bytes), ("const", CONST, cc_bytes)):
        names = [f[0] for f in fields[key]]
        assert sorted(names) == sorted(table), "fields not classified (or gone): %s" % (set(names) ^ set(table))
        covered = np.zeros(total, bool)
        for name, off, size in fields[key]:
            assert not covered[off:off + size].any(), name
            covered[off:off + size] = True
        assert covered.all(), "%s has bytes no listed field covers: a field was added without being classified" % key


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_exchange_moves_exactly_the_per_frequency_fields(harness, seed):
    cs_bytes, cc_bytes, fields = layout(harness)
    m_cs, m_cc = masks(harness, cs_bytes, cc_bytes)
    rng = np.random.default_rng(seed)
    for key, table, nbytes, mask, has_park in (("state", STATE, cs_bytes, m_cs, True), ("const", CONST, cc_bytes, m_cc, False)):
        n = nbytes // 4
        live0 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        incoming = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        park0 = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        live, park = live0.copy(), park0.copy()
        harness.scan_exchange(live.ctypes.data, mask.ctypes.data, incoming.ctypes.data, park.ctypes.data if has_park else None, n)
        lb, ib, l0b, pb, p0b = (a.view(np.uint8) for a in (live, incoming, live0, park, park0))
        for name, off, size in fields[key]:
            sl = slice(off, off + size)
            cls = table[name]
            if cls == F:
                assert (lb[sl] == ib[sl]).all(), "%s.%s must come from the incoming entry" % (key, name)
                if has_park:
                    assert (pb[sl] == l0b[sl]).all(), "%s.%s must be parked in the outgoing entry" % (key, name)
            elif cls == CH:
                assert (lb[sl] == l0b[sl]).all(), "%s.%s belongs to the channel and must stay" % (key, name)
                if has_park:
                    assert (pb[sl] == p0b[sl]).all(), "%s.%s: the bank is not written for a channel field" % (key, name)
            else:  # flags
                w = off // 4
                assert live[w] == (live0[w] & ~np.uint32(FREQ_FLAGS)) | (incoming[w] & np.uint32(FREQ_FLAGS))


def _cfg(pkg, channels_per_dev, wave_rate=16000):
    devs = [dict(channels=chs, sample_rate=2_560_000, centerfreq=120_000_000) for chs in channels_per_dev]
    return devs


CH0 = dict(frequency=120_100_000, modulation=0, squelch_threshold_dbfs=0)


def test_scan_symbols_declared_and_exported(pkg, built):
    header = open(os.path.join(REPO, "include", "airband_hip.h")).read()
    for name in ("airband_hip_prepare_scan", "airband_hip_set_freq_index", "airband_hip_freq_stats"):
        assert name + "(" in header
        assert name in pkg.EXPORTS
        assert hasattr(pkg.load_library(), name)
    assert C.sizeof(pkg.capi.ScanCfg) == 16


@pytest.mark.parametrize("case", ["twice", "channels", "empty", "first_differs", "afc", "tau", "iq_out", "nfm_8000", "bad_device"])
def test_invalid_scan_lists_are_rejected(pkg, built, case):
    EINVAL = pkg.capi.EINVAL
    wave_rate = 8000 if case == "nfm_8000" else 16000
    devs = [dict(channels=[CH0]), dict(channels=[dict(CH0, frequency=120_200_000)]), dict(channels=[CH0, dict(CH0, frequency=120_300_000)])]
    other = dict(CH0, frequency=120_150_000, squelch_threshold_dbfs=-40)
    scan = {0: [CH0, other]}
    if case == "twice":
        scan = pkg.make_scan({0: [CH0, other]})  # the same device twice cannot be said with a dict: two rows by hand
        sc = (pkg.capi.ScanCfg * 2)(scan[0][0], scan[0][0])
        cfg, keep = pkg.make_config(devs, wave_rate=wave_rate)
        h = C.c_void_p()
        rc = pkg.load_library().airband_hip_prepare_scan(C.byref(cfg), C.cast(sc, C.POINTER(pkg.capi.ScanCfg)), 2, C.byref(h))
        assert rc == EINVAL
        return
    if case == "channels":
        scan = {2: [CH0, other]}
    elif case == "empty":
        scan = {0: []}
    elif case == "first_differs":
        scan = {0: [dict(CH0, ampfactor=0.5), other]}
    elif case == "afc":
        scan = {0: [CH0, dict(other, afc=3)]}
    elif case == "tau":
        scan = {0: [CH0, dict(other, tau_us=50)]}
    elif case == "iq_out":
        scan = {0: [CH0, dict(other, has_iq_outputs=1)]}
    elif case == "nfm_8000":
        scan = {0: [CH0, dict(other, modulation=1)]}
    elif case == "bad_device":
        scan = {7: [CH0, other]}
    if case == "empty":
        sptr = (pkg.capi.ScanCfg * 1)(pkg.capi.ScanCfg(0, 0, None))
        cfg, keep = pkg.make_config(devs, wave_rate=wave_rate)
        h = C.c_void_p()
        rc = pkg.load_library().airband_hip_prepare_scan(C.byref(cfg), C.cast(sptr, C.POINTER(pkg.capi.ScanCfg)), 1, C.byref(h))
    else:
        rc = pkg.prepare_scan_rc(devs, scan, wave_rate=wave_rate)
    assert rc == EINVAL, rc


def test_valid_scan_list_passes_validation(pkg, built):
    devs = [dict(channels=[CH0]), dict(channels=[CH0, dict(CH0, frequency=120_300_000)])]
    rc = pkg.prepare_scan_rc(devs, {0: [CH0, dict(CH0, frequency=120_150_000, modulation=1, ctcss_freq=88.5)]}, wave_rate=16000)
    assert rc in (pkg.capi.OK, pkg.capi.ENODEV)  # validation passed; a machine without a GPU stops at the device


def test_entries_get_their_own_tone_tables_and_the_channel_the_union(pkg, harness):
    tones = [0.0, 88.5, 0.0, 127.3]
    entries = [dict(CH0, ctcss_freq=tones[0])] + [dict(CH0, frequency=120_100_000 + 25_000 * f, ctcss_freq=t, modulation=1 if f == 2 else 0)
                                                  for f, t in enumerate(tones) if f > 0]
    devs = [dict(channels=[entries[0]]), dict(channels=[dict(CH0, ctcss_freq=100.0)])]
    cfg, keep = pkg.make_config(devs, wave_rate=16000)
    sptr, n, skeep = pkg.make_scan({0: entries})
    cc_size = layout(harness)[1]
    out = (C.c_uint8 * (cc_size * 8))()
    tone0 = np.zeros(8, np.float32)
    ne = C.c_int()
    cflags = np.zeros(2, np.uint32)
    cdphi = np.zeros(2, np.uint32)
    rc = harness.scan_plan(C.byref(cfg), sptr, n, out, tone0.ctypes.data, 8, C.byref(ne), cflags.ctypes.data, cdphi.ctypes.data)
    assert rc == 0 and ne.value == 4
    _, _, fields = layout(harness)
    off = {name: o for name, o, s in fields["const"]}
    raw = np.frombuffer(bytes(out), np.uint8).reshape(8, cc_size)[:4]
    ct_slot = [int(np.frombuffer(r[off["ct_slot"]:off["ct_slot"] + 4].tobytes(), np.int32)[0]) for r in raw]
    flags = [int(np.frombuffer(r[off["flags"]:off["flags"] + 4].tobytes(), np.uint32)[0]) for r in raw]
    assert ct_slot[0] == -1 and ct_slot[2] == -1
    assert ct_slot[1] >= 0 and ct_slot[3] >= 0 and ct_slot[1] != ct_slot[3]
    assert 0 not in (ct_slot[1], ct_slot[3])  # slot 0 is device 1's channel (100 Hz)
    # each slot holds its own tone: the Goertzel coefficient of the target tone at the fast window (src/ctcss.cpp)
    rate, window = 16000.0, int(16000 * 0.05)
    for f in (1, 3):
        k = int(0.5 + window * tones[f] / rate)
        want = np.float32(2.0 * np.cos(2.0 * np.pi * k / window))
        assert abs(float(tone0[f]) - float(want)) < 1e-5, (f, tone0[f], want)
    # NFM entry: needs_raw_iq is the channel's union, and its dm_dphi is derived (from freqlist[0])
    assert cflags[0] & 0x10 and cdphi[0] != 0
    assert flags[2] & 0x40 and not flags[1] & 0x40
    assert all(fl & 0x10 for fl in flags)  # every entry's image carries the channel's RAW_IQ
