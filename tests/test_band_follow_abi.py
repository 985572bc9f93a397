"""The band follow's public interface without a GPU: the five entry points in the built library and in the header, the three structs, every validation error
of airband_hip_prepare_follow() (it returns before a device is touched), and the definition in plain Python (capi.band_follow_reference) on a sequence whose
answers are written out by hand."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_prepare_follow", "airband_hip_set_band_follow", "airband_hip_collect_band_follow_changes", "airband_hip_collect_band_followers",
         "airband_hip_device_band_follow")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.BAND_FOLLOW_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # no existing struct changed


def test_struct_sizes_and_offsets(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.BandFollower) == 16 and C.sizeof(capi.BandFollowChange) == 16 and C.sizeof(capi.BandFollowRow) == 16
    want = {capi.BandFollower: dict(channel=0, bin=4, since_batch=8, track=12, reserved=14),
            capi.BandFollowChange: dict(dev=0, channel=4, bin=8, kind=12, track=13, reserved=14),
            capi.BandFollowRow: dict(n_following=0, n_unserved=4, n_changes=8, reserved=12)}
    for struct, dtype in ((capi.BandFollower, capi.FOLLOWER_DTYPE), (capi.BandFollowChange, capi.FOLLOW_CHANGE_DTYPE), (capi.BandFollowRow, capi.FOLLOW_ROW_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct)
        assert {f[0]: getattr(struct, f[0]).offset for f in struct._fields_} == want[struct] == {n: dt.fields[n][1] for n in dt.names}
    assert (capi.FOLLOW_TUNE, capi.FOLLOW_MOVE, capi.FOLLOW_HOME) == (1, 2, 3)


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_prepare_follow(const airband_hip_config* cfg, const airband_hip_scan_cfg* scan, int32_t n_scan, const int32_t* follow_channels, int32_t n_follow, airband_hip_handle** out);",
                 "int airband_hip_set_band_follow(airband_hip_handle* h, int64_t max_changes);",
                 "int airband_hip_collect_band_follow_changes(airband_hip_handle* h, int64_t* n_changes, airband_hip_band_follow_change* changes);",
                 "int airband_hip_collect_band_followers(airband_hip_handle* h, airband_hip_band_follower* followers, airband_hip_band_follow_row* rows);",
                 "int airband_hip_device_band_follow(airband_hip_handle* h, int32_t** d_n_changes, airband_hip_band_follow_change** d_changes, airband_hip_band_follower** d_followers, airband_hip_band_follow_row** d_rows);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("} airband_hip_band_follower; /* 16 bytes */", "} airband_hip_band_follow_change; /* 16 bytes */", "} airband_hip_band_follow_row; /* 16 bytes */",
                   "#define AIRBAND_FOLLOW_TUNE 1", "#define AIRBAND_FOLLOW_MOVE 2", "#define AIRBAND_FOLLOW_HOME 3", "NFM followers are out of scope",
                   "AT THE START OF THE BATCH", "PREPARE-TIME bins", "the bin the NEXT batch is channelized at"):
        assert phrase in text, phrase
    assert "moves only with AFC" not in text


def _devices(capi, n_dev=2):
    """n_dev dongles of eight AM channels; the last two of each are the spares."""
    return [dict(channels=[dict(frequency=119_000_000 + 250_000 * j) for j in range(8)]) for _ in range(n_dev)]


def test_prepare_follow_validates_before_any_device(pkg, built):
    capi = pkg.capi
    base = _devices(capi)

    def rc(follow, devices=base, scan=None, wave_rate=8000):
        return pkg.prepare_follow_rc(devices, scan, follow, wave_rate=wave_rate)

    def bad(ch, **kw):
        devices = [dict(d, channels=[dict(c) for c in d["channels"]]) for d in base]
        devices[ch // 8]["channels"][ch % 8].update(kw)
        return devices

    for follow, devices, word in (([16], base, "out of range"), ([-1], base, "out of range"), ([6, 6], base, "ascending"), ([7, 6], base, "ascending"),
                                  ([14], bad(14, afc=2), "afc"), ([14], bad(14, bandwidth_hz=5000), "bandwidth"), ([14], bad(14, has_iq_outputs=1), "raw-I/Q")):
        code, text = rc(follow, devices)
        assert code == capi.EINVAL and word in text, (follow, code, text)
        assert "channel %d" % follow[-1] in text, text  # the text names the offending channel
    code, text = rc([6], bad(6, modulation=capi.MOD_NFM), wave_rate=16000)
    assert code == capi.EINVAL and "NFM" in text and "channel 6" in text
    # a follower on a scan device
    one = dict(frequency=120_100_000)
    code, text = rc([8], base[:1] + [dict(channels=[dict(one)])], scan={1: [one, dict(frequency=120_200_000)]})
    assert code == capi.EINVAL and "scan" in text and "channel 8" in text
    # 65 followers on one dongle: refused before a device is touched.  A dongle holds at most 64 channels and the indices are strictly ascending, so the
    # configuration itself is refused first (EBADSIZE, "channel_count must be 1..64"); build_follow()'s own count of 64 stands behind that.
    many = [dict(channels=[dict(frequency=119_000_000 + 25_000 * j) for j in range(64)]) for _ in range(2)]
    code, text = rc(list(range(65)), [dict(channels=many[0]["channels"] + [dict(frequency=121_000_000)]), many[1]])
    assert code in (capi.EINVAL, capi.EBADSIZE) and "64" in text, (code, text)
    code, text = rc(list(range(64)) + [64], many)  # 64 on dongle 0 and one on dongle 1: passes the validation (and then finds no device on a machine without one)
    assert code in (capi.OK, capi.ENODEV), (code, text)
    # NULL with a count
    L = pkg.load_library()
    cfg, keep = pkg.make_config(base, wave_rate=8000)
    h = C.c_void_p()
    assert L.airband_hip_prepare_follow(C.byref(cfg), None, 0, None, 1, C.byref(h)) == capi.EINVAL and not h


def test_without_followers_it_is_prepare_scan(pkg, built):
    """(NULL, 0): the same answer as airband_hip_prepare_scan() gives on this machine, for a good configuration and for a bad scan list."""
    capi = pkg.capi
    base = _devices(capi)
    assert pkg.prepare_follow_rc(base, None, None, wave_rate=8000)[0] == pkg.prepare_scan_rc(base, None, wave_rate=8000)
    assert pkg.prepare_follow_rc(base, None, [], wave_rate=8000)[0] == pkg.prepare_scan_rc(base, None, wave_rate=8000)
    scan = {0: [dict(frequency=1)]}  # a scan device with eight channels
    assert pkg.prepare_follow_rc(base, scan, None, wave_rate=8000)[0] == pkg.prepare_scan_rc(base, scan, wave_rate=8000) == capi.EINVAL


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    p = [C.c_void_p() for _ in range(4)]
    n = C.c_int64(7)
    assert L.airband_hip_set_band_follow(None, 4) == capi.EINVAL
    assert L.airband_hip_collect_band_follow_changes(None, C.byref(n), None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_collect_band_followers(None, None, None) == capi.EINVAL
    assert L.airband_hip_device_band_follow(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)


def _tracks(capi, T, entries):
    t = np.zeros(T, capi.TRACK_DTYPE)
    t["bin"] = -1
    for s, (state, b) in entries.items():
        t[s]["state"], t[s]["bin"] = state, b
    return t


def test_reference_by_hand(pkg):
    """Two followers (channels 6 and 7, home bins 40 and 50), four slots."""
    capi = pkg.capi
    Cf, Te = capi.WATCH_CONFIRMED, capi.WATCH_TENTATIVE
    fol = capi.band_follow_blank([6, 7], [40, 50])
    before = fol.tobytes()
    # batch 3: slots 1 and 3 confirmed, slot 0 tentative -- the followers take 1 and 3 in slot order
    f, row, ch = capi.band_follow_reference(fol, _tracks(capi, 4, {0: (Te, 9), 1: (Cf, 100), 3: (Cf, 200)}), [40, 50], 3, dev=5)
    assert fol.tobytes() == before  # its arguments are left alone
    assert f.tolist() == [(6, 100, 3, 1, 0), (7, 200, 3, 3, 0)] and row.tolist() == (2, 0, 2, 0)
    assert ch.tolist() == [(5, 6, 100, capi.FOLLOW_TUNE, 1, 0), (5, 7, 200, capi.FOLLOW_TUNE, 3, 0)]
    # batch 4: slot 1 drifts, slot 0 is confirmed and finds nobody idle
    f, row, ch = capi.band_follow_reference(f, _tracks(capi, 4, {0: (Cf, 9), 1: (Cf, 101), 3: (Cf, 200)}), [40, 50], 4, dev=5)
    assert f.tolist() == [(6, 101, 3, 1, 0), (7, 200, 3, 3, 0)] and row.tolist() == (2, 1, 1, 0)
    assert ch.tolist() == [(5, 6, 101, capi.FOLLOW_MOVE, 1, 0)]
    # batch 5: slot 3 is gone -- its follower goes home and is NOT idle at the start of the batch, so slot 0 stays unserved for one more batch
    f, row, ch = capi.band_follow_reference(f, _tracks(capi, 4, {0: (Cf, 9), 1: (Cf, 101)}), [40, 50], 5, dev=5)
    assert f.tolist() == [(6, 101, 3, 1, 0), (7, 50, 5, -1, 0)] and row.tolist() == (1, 1, 1, 0)
    assert ch.tolist() == [(5, 7, 50, capi.FOLLOW_HOME, 3, 0)]
    # batch 6: now it takes slot 0
    f, row, ch = capi.band_follow_reference(f, _tracks(capi, 4, {0: (Cf, 9), 1: (Cf, 101)}), [40, 50], 6, dev=5)
    assert f.tolist() == [(6, 101, 3, 1, 0), (7, 9, 6, 0, 0)] and row.tolist() == (2, 0, 1, 0)
    assert ch.tolist() == [(5, 7, 9, capi.FOLLOW_TUNE, 0, 0)]
    assert f.dtype == np.dtype(capi.FOLLOWER_DTYPE) and ch.dtype == np.dtype(capi.FOLLOW_CHANGE_DTYPE) and row.dtype == np.dtype(capi.FOLLOW_ROW_DTYPE)
