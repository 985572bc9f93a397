"""ctypes mirror of include/airband_hip.h (struct layouts and constants only; no logic)."""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 2
OK, ENODEV, EBADSIZE, ENOMEM, EINVAL, EAGAIN, ERUNTIME = 0, -1, -2, -3, -4, -5, -6
SFMT_U8, SFMT_S8, SFMT_S16, SFMT_F32 = 1, 2, 3, 4
MOD_AM, MOD_NFM = 0, 1
FM_FAST_ATAN2, FM_QUADRI_DEMOD = 0, 1
AGC_EXTRA = 100
FLAG_TRACE_SQUELCH, FLAG_RESERVED_2, FLAG_FORCE_FFT, FLAG_SERIAL_DEMOD, FLAG_PIPELINE, FLAG_REGROUP, FLAG_NO_REGROUP = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
FLAG_WIDE_HOPS = 0x80  # the matrix-core channelizers also take hops beyond 1 024 bytes (CS16: 1 280; CF32: beyond the float kernel's tile, ~3 MS/s at WAVE_RATE 8000): devices above ~4 MS/s
GATE_NEVER, GATE_SIGNAL, GATE_ALWAYS = 0, 1, 2  # airband_hip_set_output_gate
SCOPE_MEAN, SCOPE_PEAK = 0x1, 0x2  # airband_hip_set_band_scope: traces

BYTES_PER_SAMPLE = {SFMT_U8: 1, SFMT_S8: 1, SFMT_S16: 2, SFMT_F32: 4}


class ChannelCfg(C.Structure):
    _fields_ = [("frequency", C.c_int32), ("modulation", C.c_int32), ("afc", C.c_int32), ("squelch_threshold_dbfs", C.c_int32),
                ("squelch_snr_threshold_db", C.c_float), ("notch_freq", C.c_float), ("notch_q", C.c_float), ("ctcss_freq", C.c_float),
                ("bandwidth_hz", C.c_int32), ("ampfactor", C.c_float), ("tau_us", C.c_int32), ("has_iq_outputs", C.c_int32)]


class DeviceCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("centerfreq", C.c_int32), ("sfmt", C.c_int32), ("fullscale", C.c_float), ("tau_us", C.c_int32),
                ("channel_count", C.c_int32), ("channels", C.POINTER(ChannelCfg))]


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("flags", C.c_uint32), ("fft_size_log", C.c_int32), ("wave_rate", C.c_int32), ("fm_demod", C.c_int32),
                ("hip_device", C.c_int32), ("device_count", C.c_int32), ("devices", C.POINTER(DeviceCfg))]


class ScanCfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("freq_count", C.c_int32), ("freqs", C.POINTER(ChannelCfg))]


class MixerInput(C.Structure):
    _fields_ = [("device", C.c_int32), ("channel", C.c_int32), ("mixer", C.c_int32), ("ampfactor", C.c_float), ("balance", C.c_float)]


class Geometry(C.Structure):
    _fields_ = [("fft_size", C.c_int32), ("wave_rate", C.c_int32), ("wave_batch", C.c_int32), ("device_count", C.c_int32), ("total_channels", C.c_int32),
                ("max_channels", C.c_int32), ("mixer_count", C.c_int32), ("wave_stride", C.c_int32), ("first_batch_bytes", C.c_int64),
                ("batch_bytes", C.c_int64), ("lookahead_bytes", C.c_int64)]


class ChannelStats(C.Structure):
    _fields_ = [("noise_level", C.c_float), ("signal_level", C.c_float), ("squelch_level", C.c_float), ("agcavgfast", C.c_float),
                ("open_count", C.c_uint64), ("flappy_count", C.c_uint64), ("ctcss_count", C.c_uint64), ("no_ctcss_count", C.c_uint64),
                ("active_counter", C.c_uint64), ("bin", C.c_int32), ("squelch_state", C.c_int32), ("signal_outside_filter", C.c_int32), ("reserved", C.c_int32)]


class BandPeak(C.Structure):
    _fields_ = [("bin", C.c_int32), ("power", C.c_float)]


class BandSummary(C.Structure):
    _fields_ = [("floor", C.c_float), ("threshold", C.c_float), ("max_power", C.c_float), ("max_bin", C.c_int32), ("n_over", C.c_int32), ("n_peaks", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class BandTrack(C.Structure):
    _fields_ = [("bin", C.c_int32), ("power", C.c_float), ("max_power", C.c_float), ("first_batch", C.c_uint32), ("last_batch", C.c_uint32), ("hits", C.c_uint16),
                ("misses", C.c_uint8), ("state", C.c_uint8)]


class BandEvent(C.Structure):
    _fields_ = [("dev", C.c_int32), ("bin", C.c_int32), ("power", C.c_float), ("kind", C.c_uint8), ("track", C.c_uint8), ("batches", C.c_uint16)]


class BandWatchRow(C.Structure):
    _fields_ = [("n_live", C.c_int32), ("n_confirmed", C.c_int32), ("n_events", C.c_int32), ("dropped", C.c_int32)]


def channel_cfg(frequency, modulation=MOD_AM, afc=0, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0, ctcss_freq=0.0,
                bandwidth_hz=0, ampfactor=1.0, tau_us=-1, has_iq_outputs=0) -> ChannelCfg:
    return ChannelCfg(int(frequency), int(modulation), int(afc), int(squelch_threshold_dbfs), float(squelch_snr_threshold_db), float(notch_freq),
                      float(notch_q), float(ctcss_freq), int(bandwidth_hz), float(ampfactor), int(tau_us), int(has_iq_outputs))


def device_cfg(channels, sample_rate=2_560_000, centerfreq=120_000_000, sfmt=SFMT_U8, fullscale=0.0, tau_us=-1):
    """Returns (DeviceCfg, keepalive array). ``channels`` = list of ChannelCfg or of kwargs dicts."""
    chs = [c if isinstance(c, ChannelCfg) else channel_cfg(**c) for c in channels]
    arr = (ChannelCfg * len(chs))(*chs)
    dev = DeviceCfg(int(sample_rate), int(centerfreq), int(sfmt), float(fullscale), int(tau_us), len(chs), C.cast(arr, C.POINTER(ChannelCfg)))
    return dev, arr


# the band scope's entry points (include/airband_hip.h): argument types by symbol, applied by load_library()
_vp, _i32, _u32 = C.c_void_p, C.c_int32, C.c_uint32
BAND_SCOPE_PROTOTYPES = {
    "airband_hip_set_band_scope": [_vp, _vp, _i32, _u32],
    "airband_hip_collect_band_scope": [_vp, _i32, _i32, _vp, _vp],
    "airband_hip_device_band_scope": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}

# airband_hip_read_tables (same header): the coefficient tables of a matrix-core handle, read back for tests
class TableInfo(C.Structure):
    _fields_ = [("n_bsets", C.c_int32), ("n_shared_bsets", C.c_int32), ("n_host_bsets", C.c_int32), ("pieces_per_table", C.c_int32), ("bytes_per_table", C.c_int64),
                ("edge_hi_zero", C.c_int32), ("n_items", C.c_int32), ("channelizer", C.c_char * 16)]


TABLES_PROTOTYPES = {
    "airband_hip_read_tables": [_vp, _i32, _i32, C.POINTER(TableInfo), _vp, _vp, _vp, _vp],
}

# the band survey's (same header)
_f32 = C.c_float
BAND_SURVEY_PROTOTYPES = {
    "airband_hip_set_band_survey": [_vp, _u32, _i32, _i32, _f32, _i32],
    "airband_hip_collect_band_survey": [_vp, _i32, _i32, _vp, _vp],
    "airband_hip_device_band_survey": [_vp, C.POINTER(_vp), C.POINTER(_vp)],
}
# numpy views of airband_hip_band_peak / airband_hip_band_summary
PEAK_DTYPE = [("bin", "<i4"), ("power", "<f4")]
SUMMARY_DTYPE = [("floor", "<f4"), ("threshold", "<f4"), ("max_power", "<f4"), ("max_bin", "<i4"), ("n_over", "<i4"), ("n_peaks", "<i4"), ("reserved", "<i4", (2,))]


def band_survey_reference(row, bins, max_peaks, floor_permille, ratio, guard_bins):
    """The band survey's definition (include/airband_hip.h) on one scope row, in numpy: what airband_hip_collect_band_survey() returns for the dongle whose row of
    the surveyed trace is `row` and whose channels sit on the prepare-time bins `bins`.  Every comparison is on the values' bit patterns as unsigned integers;
    the threshold is the one float32 multiplication.  Returns dict(floor, threshold, max_power: float32; max_bin, n_over, n_peaks: int;
    peaks: [max_peaks] array of PEAK_DTYPE, {-1, 0} behind the listed ones)."""
    import numpy as np

    row = np.ascontiguousarray(row, np.float32)
    u = row.view(np.uint32)
    n = len(u)
    order = np.sort(u)
    floor = order[min(n - 1, (n * int(floor_permille)) // 1000)]
    with np.errstate(all="ignore"):
        threshold = np.array([floor], np.uint32).view(np.float32)[0] * np.float32(ratio)
    t = np.array([threshold], np.float32).view(np.uint32)[0]
    max_bin = int(np.argmax(u))  # the first among equals
    over = u > t
    is_peak = over & (u >= np.roll(u, 1)) & (u > np.roll(u, -1))
    if guard_bins >= 0:
        k = np.arange(n)
        for b in bins:
            d = np.abs(k - int(b))
            is_peak &= ~(np.minimum(d, n - d) <= guard_bins)
    at = np.flatnonzero(is_peak)
    at = at[np.lexsort((at, -u[at].astype(np.int64)))]  # power descending, then bin ascending
    peaks = np.zeros(int(max_peaks), PEAK_DTYPE)
    peaks["bin"] = -1
    m = min(len(at), int(max_peaks))
    peaks["bin"][:m] = at[:m]
    peaks["power"][:m] = row[at[:m]]
    return dict(floor=np.array([floor], np.uint32).view(np.float32)[0], threshold=np.float32(threshold), max_power=row[max_bin], max_bin=max_bin,
                n_over=int(over.sum()), n_peaks=int(len(at)), peaks=peaks)


# the band watch's (same header)
_i64 = C.c_int64
BAND_WATCH_PROTOTYPES = {
    "airband_hip_set_band_watch": [_vp, _i32, _i32, _i32, _i32, _i64],
    "airband_hip_collect_band_events": [_vp, C.POINTER(_i64), _vp],
    "airband_hip_collect_band_tracks": [_vp, _i32, _i32, _vp, _vp],
    "airband_hip_device_band_watch": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
WATCH_FREE, WATCH_TENTATIVE, WATCH_CONFIRMED = 0, 1, 2
WATCH_APPEAR, WATCH_VANISH = 1, 2
# numpy views of airband_hip_band_track / airband_hip_band_event / airband_hip_band_watch_row
TRACK_DTYPE = [("bin", "<i4"), ("power", "<f4"), ("max_power", "<f4"), ("first_batch", "<u4"), ("last_batch", "<u4"), ("hits", "<u2"), ("misses", "u1"), ("state", "u1")]
EVENT_DTYPE = [("dev", "<i4"), ("bin", "<i4"), ("power", "<f4"), ("kind", "u1"), ("track", "u1"), ("batches", "<u2")]
WATCH_ROW_DTYPE = [("n_live", "<i4"), ("n_confirmed", "<i4"), ("n_events", "<i4"), ("dropped", "<i4")]


def band_watch_blank(max_tracks):
    """The state a watch starts from: (tracks [max_tracks] of TRACK_DTYPE, every slot free; row of WATCH_ROW_DTYPE, zeros)."""
    import numpy as np

    tracks = np.zeros(int(max_tracks), TRACK_DTYPE)
    tracks["bin"] = -1
    return tracks, np.zeros((), WATCH_ROW_DTYPE)


def band_watch_reference(tracks, row, peaks, n_peaks, batch, max_tracks, match_bins, confirm_hits, release_misses, n_fft, dev=0):
    """The band watch's definition (include/airband_hip.h) for one batch of one scope row, in plain Python: the row's table `tracks` ([max_tracks] of TRACK_DTYPE)
    and record `row` (WATCH_ROW_DTYPE) as the batch before left them, the row's survey of this batch (`peaks` of PEAK_DTYPE as collect_band_survey() returns
    them, `n_peaks` the summary's count), the watch batch number `batch`.  Returns (tracks, row, events): new arrays, events of EVENT_DTYPE with `dev` in their
    first field.  A switched-off dongle is not advanced: do not call this for it.  Powers are moved and compared as bit patterns; nothing here is a float
    operation."""
    import numpy as np

    T, M, Cn, R, N, k = int(max_tracks), int(match_bins), int(confirm_hits), int(release_misses), int(n_fft), int(batch) & 0xFFFFFFFF
    tracks = np.array(tracks, TRACK_DTYPE).reshape(T).copy()
    row = np.array(row, WATCH_ROW_DTYPE).copy()
    peaks = np.ascontiguousarray(peaks, PEAK_DTYPE)
    bits = peaks["power"].view(np.uint32)

    def as_float(u):
        return np.array([u], np.uint32).view(np.float32)[0]

    def free(s):
        tracks[s] = np.zeros((), TRACK_DTYPE)
        tracks[s]["bin"] = -1

    events = []
    live0 = [int(tracks[s]["state"]) != WATCH_FREE for s in range(T)]  # at the start of the batch
    matched, taken, dropped = [False] * T, [False] * T, 0
    # 1. every peak in list order
    for i in range(min(max(int(n_peaks), 0), len(peaks))):
        b, p = int(peaks["bin"][i]), int(bits[i])
        best = None
        for s in range(T):
            if live0[s] and not matched[s]:
                d = abs(b - int(tracks[s]["bin"]))
                d = min(d, N - d)
                if d <= M and (best is None or d < best[0]):  # among equals the lowest slot
                    best = (d, s)
        if best is not None:
            s = best[1]
            t = tracks[s]
            t["bin"] = b
            t["power"] = as_float(p)
            t["max_power"] = as_float(max(p, int(t["max_power"].view(np.uint32))))
            t["misses"] = 0
            t["hits"] = min(int(t["hits"]) + 1, 65535)
            t["last_batch"] = k
            matched[s] = True
            if int(t["state"]) == WATCH_TENTATIVE and int(t["hits"]) >= Cn:
                t["state"] = WATCH_CONFIRMED
                events.append((dev, b, as_float(p), WATCH_APPEAR, s, int(t["hits"])))
            continue
        slot = next((s for s in range(T) if not live0[s] and not taken[s]), None)
        if slot is None:
            dropped += 1
            continue
        taken[slot] = True
        t = tracks[slot]
        t["bin"], t["power"], t["max_power"] = b, as_float(p), as_float(p)
        t["first_batch"] = t["last_batch"] = k
        t["hits"], t["misses"], t["state"] = 1, 0, WATCH_TENTATIVE
        if Cn <= 1:
            t["state"] = WATCH_CONFIRMED
            events.append((dev, b, as_float(p), WATCH_APPEAR, slot, 1))
    # 2. the tracks nothing matched, in slot order
    for s in range(T):
        if not live0[s] or matched[s]:
            continue
        t = tracks[s]
        t["misses"] = min(int(t["misses"]) + 1, 255)
        if int(t["state"]) == WATCH_TENTATIVE:
            free(s)
        elif int(t["misses"]) >= R:
            span = (int(t["last_batch"]) - int(t["first_batch"]) + 1) & 0xFFFFFFFF
            events.append((dev, int(t["bin"]), t["max_power"], WATCH_VANISH, s, min(65535, span)))
            free(s)
    row["n_live"] = int((tracks["state"] != WATCH_FREE).sum())
    row["n_confirmed"] = int((tracks["state"] == WATCH_CONFIRMED).sum())
    row["n_events"] = len(events)
    row["dropped"] = int(row["dropped"]) + dropped
    out = np.zeros(len(events), EVENT_DTYPE)
    for j, e in enumerate(events):
        out[j] = e
    return tracks, row, out


# the band follow's (same header)
class BandFollower(C.Structure):
    _fields_ = [("channel", C.c_int32), ("bin", C.c_int32), ("since_batch", C.c_uint32), ("track", C.c_int16), ("reserved", C.c_uint16)]


class BandFollowChange(C.Structure):
    _fields_ = [("dev", C.c_int32), ("channel", C.c_int32), ("bin", C.c_int32), ("kind", C.c_uint8), ("track", C.c_uint8), ("reserved", C.c_uint16)]


class BandFollowRow(C.Structure):
    _fields_ = [("n_following", C.c_int32), ("n_unserved", C.c_int32), ("n_changes", C.c_int32), ("reserved", C.c_int32)]


BAND_FOLLOW_PROTOTYPES = {
    "airband_hip_prepare_follow": [C.POINTER(Config), C.POINTER(ScanCfg), _i32, C.POINTER(_i32), _i32, C.POINTER(_vp)],
    "airband_hip_set_band_follow": [_vp, _i64],
    "airband_hip_collect_band_follow_changes": [_vp, C.POINTER(_i64), _vp],
    "airband_hip_collect_band_followers": [_vp, _vp, _vp],
    "airband_hip_device_band_follow": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
FOLLOW_TUNE, FOLLOW_MOVE, FOLLOW_HOME = 1, 2, 3
# numpy views of airband_hip_band_follower / airband_hip_band_follow_change / airband_hip_band_follow_row
FOLLOWER_DTYPE = [("channel", "<i4"), ("bin", "<i4"), ("since_batch", "<u4"), ("track", "<i2"), ("reserved", "<u2")]
FOLLOW_CHANGE_DTYPE = [("dev", "<i4"), ("channel", "<i4"), ("bin", "<i4"), ("kind", "u1"), ("track", "u1"), ("reserved", "<u2")]
FOLLOW_ROW_DTYPE = [("n_following", "<i4"), ("n_unserved", "<i4"), ("n_changes", "<i4"), ("reserved", "<i4")]


def band_follow_blank(channels, home_bins):
    """The state the followers start from: [len(channels)] of FOLLOWER_DTYPE, every one idle on its home bin."""
    import numpy as np

    f = np.zeros(len(channels), FOLLOWER_DTYPE)
    f["channel"], f["bin"], f["track"] = channels, home_bins, -1
    return f


def band_follow_reference(followers, tracks, home_bins, batch, dev=0):
    """The band follow's definition (include/airband_hip.h) for one batch of one scope row, in plain Python: the row's `followers` (FOLLOWER_DTYPE, ascending channel
    order) as the batch before left them, the row's table `tracks` (TRACK_DTYPE) as the watch left it after THIS batch, the followers' `home_bins`, the watch batch
    number `batch`.  Returns (followers, row, changes): new arrays; row of FOLLOW_ROW_DTYPE, changes of FOLLOW_CHANGE_DTYPE with `dev` in their first field.  A
    switched-off dongle is frozen: do not call this for it (its record keeps its counts with n_changes = 0)."""
    import numpy as np

    fol = np.array(followers, FOLLOWER_DTYPE).reshape(-1).copy()
    tracks = np.ascontiguousarray(tracks, TRACK_DTYPE).reshape(-1)
    T, k = len(tracks), int(batch) & 0xFFFFFFFF
    confirmed = [int(t["state"]) == WATCH_CONFIRMED for t in tracks]
    idle0 = [not 0 <= int(f["track"]) < T for f in fol]  # at the start of the batch
    changes = []
    # A. the followers that have a track, in follower order
    for i, f in enumerate(fol):
        s = int(f["track"])
        if idle0[i]:
            continue
        if not confirmed[s]:
            f["bin"], f["track"], f["since_batch"] = int(home_bins[i]), -1, k
            changes.append((dev, int(f["channel"]), int(f["bin"]), FOLLOW_HOME, s, 0))
        elif int(tracks[s]["bin"]) != int(f["bin"]):
            f["bin"] = int(tracks[s]["bin"])
            changes.append((dev, int(f["channel"]), int(f["bin"]), FOLLOW_MOVE, s, 0))
    # B. the confirmed slots nobody follows, in slot order
    taken, unserved = [False] * len(fol), 0
    for s in range(T):
        if not confirmed[s] or any(int(f["track"]) == s for f in fol):
            continue
        i = next((i for i in range(len(fol)) if idle0[i] and not taken[i]), None)
        if i is None:
            unserved += 1
            continue
        taken[i] = True
        f = fol[i]
        f["track"], f["bin"], f["since_batch"] = s, int(tracks[s]["bin"]), k
        changes.append((dev, int(f["channel"]), int(f["bin"]), FOLLOW_TUNE, s, 0))
    row = np.zeros((), FOLLOW_ROW_DTYPE)
    row["n_following"], row["n_unserved"], row["n_changes"] = int((fol["track"] >= 0).sum()), unserved, len(changes)
    out = np.zeros(len(changes), FOLLOW_CHANGE_DTYPE)
    for j, c in enumerate(changes):
        out[j] = c
    return fol, row, out


# scan control's (same header)
class ScanEvent(C.Structure):
    _fields_ = [("dev", C.c_int32), ("freq_idx", C.c_int16), ("prev_idx", C.c_int16), ("kind", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint16),
                ("batch", C.c_uint32)]


class ScanState(C.Structure):
    _fields_ = [("idx", C.c_int16), ("hold", C.c_int16), ("idle", C.c_int32), ("since", C.c_int32), ("last", C.c_int16), ("has_list", C.c_int16)]


SCAN_CONTROL_PROTOTYPES = {
    "airband_hip_set_scan_control": [_vp, _i32, _i32, _i64],
    "airband_hip_scan_hold": [_vp, _i32, _i32],
    "airband_hip_collect_scan_events": [_vp, C.POINTER(_i64), _vp],
    "airband_hip_collect_scan_state": [_vp, _i32, _i32, _vp],
    "airband_hip_device_scan_control": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
SCAN_HOP, SCAN_ACTIVITY = 1, 2
SCAN_RETAG = 1
NO_SIGNAL = 0x20  # channel->axcindicate of a batch without signal: ' '
# numpy views of airband_hip_scan_event / airband_hip_scan_state
SCAN_EVENT_DTYPE = [("dev", "<i4"), ("freq_idx", "<i2"), ("prev_idx", "<i2"), ("kind", "u1"), ("flags", "u1"), ("reserved", "<u2"), ("batch", "<u4")]
SCAN_STATE_DTYPE = [("idx", "<i2"), ("hold", "<i2"), ("idle", "<i4"), ("since", "<i4"), ("last", "<i2"), ("has_list", "<i2")]


def scan_control_blank(idx=0):
    """The state a list starts from when control is switched on: entry `idx` in force, no hold, has_list = 1 (a scalar of SCAN_STATE_DTYPE)."""
    import numpy as np

    st = np.zeros((), SCAN_STATE_DTYPE)
    st["idx"], st["hold"], st["has_list"] = idx, -1, 1
    return st


def scan_control_reference(state, axc, freq_count, batch, idle_batches=16, dwell_batches=2, dev=0, enabled=True):
    """Scan control's definition (include/airband_hip.h) for one batch of one scan list, in plain Python: the list's `state` (SCAN_STATE_DTYPE) as the batch
    before left it, `axc` the channel's axcindicate of this batch (a byte), `freq_count` the list's length, `batch` the control's batch number.  Returns
    (state, records): new arrays, records of SCAN_EVENT_DTYPE, none or one, with `dev` in the first field.  The entry stage 2 of the NEXT batch runs with is
    state["idx"].  A switched-off dongle (enabled=False) and a list of fewer than two entries are frozen: the state comes back as it went in, no record."""
    import numpy as np

    st = np.array(state, SCAN_STATE_DTYPE).reshape(()).copy()
    none = np.zeros(0, SCAN_EVENT_DTYPE)
    n, k = int(freq_count), int(batch) & 0xFFFFFFFF
    if not enabled or n < 2:
        return st, none
    idx, hold, idle, since, last = int(st["idx"]), int(st["hold"]), int(st["idle"]), int(st["since"]), int(st["last"])
    rec = None
    if hold >= 0:
        if idx != hold:
            rec = (dev, hold, idx, SCAN_HOP, 0, 0, k)
            idx = hold
        idle = since = 0
    elif int(axc) == NO_SIGNAL:
        if idle < int(idle_batches):
            idle += 1
        else:
            since += 1
            if since >= int(dwell_batches):
                rec = (dev, (idx + 1) % n, idx, SCAN_HOP, 0, 0, k)
                idx = (idx + 1) % n
                since = 0
    else:
        if idle == int(idle_batches):
            rec = (dev, idx, last, SCAN_ACTIVITY, SCAN_RETAG if idx != last else 0, 0, k)
            last = idx
        idle = since = 0
    st["idx"], st["idle"], st["since"], st["last"] = idx, idle, since, last
    if rec is None:
        return st, none
    out = np.zeros(1, SCAN_EVENT_DTYPE)
    out[0] = rec
    return st, out


# the encoded audio collect's (same header)
AUDIO_F32, AUDIO_S16, AUDIO_ULAW, AUDIO_ALAW = 0, 1, 2, 3
AUDIO_ENCODINGS = {"s16": AUDIO_S16, "ulaw": AUDIO_ULAW, "alaw": AUDIO_ALAW}


class AudioRow(C.Structure):
    _fields_ = [("channel", C.c_int32), ("peak", C.c_uint16), ("n_clipped", C.c_uint16), ("first", C.c_uint16), ("end", C.c_uint16), ("reserved", C.c_uint32)]


AUDIO_ENCODING_PROTOTYPES = {
    "airband_hip_set_output_encoding": [_vp, _i32],
    "airband_hip_collect_active_encoded": [_vp, C.POINTER(_i64), _vp, _vp, _vp, _vp],
    "airband_hip_device_active_encoded": [_vp, C.POINTER(_vp), C.POINTER(_vp)],
    "airband_hip_encode_audio": [_vp, _i32, _vp, _i64, _vp, _vp],
}
# numpy view of airband_hip_audio_row
AUDIO_ROW_DTYPE = [("channel", "<i4"), ("peak", "<u2"), ("n_clipped", "<u2"), ("first", "<u2"), ("end", "<u2"), ("reserved", "<u4")]
_ULAW_ENDS = (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF)
_ALAW_ENDS = (0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF)


def audio_encoding_value(encoding) -> int:
    """"s16" / "ulaw" / "alaw" or an AUDIO_* value -> the AUDIO_* value"""
    return AUDIO_ENCODINGS[encoding] if isinstance(encoding, str) else int(encoding)


def audio_quantize_reference(rows):
    """The float step of the encoded audio collect (include/airband_hip.h): (q int32 in -32767 .. 32767, clipped bool), of the shape of `rows`."""
    import numpy as np

    x = np.ascontiguousarray(rows, np.float32)
    with np.errstate(all="ignore"):
        v = x * np.float32(32767.0)  # one float32 multiplication
        nan = np.isnan(x)
        clipped = ~nan & (np.abs(v) > np.float32(32767.0))
        q = np.rint(np.where(nan | clipped, np.float32(0.0), v)).astype(np.int32)  # to nearest, ties to even
    q = np.where(clipped, np.where(v < 0, -32767, 32767), q).astype(np.int32)
    return q, clipped


def audio_law_reference(q, encoding):
    """G.711 codes (uint8) of integers q in -32768 .. 32767, by the header's definition: AUDIO_ULAW or AUDIO_ALAW."""
    import numpy as np

    q = np.asarray(q, np.int32)
    if encoding == AUDIO_ULAW:
        p = q >> 2
        mask = np.where(p < 0, 0x7F, 0xFF)
        m = np.minimum(np.abs(p), 8159) + 33
        seg = (m[..., None] > np.array(_ULAW_ENDS)).sum(-1)
        code = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 0xF))
    elif encoding == AUDIO_ALAW:
        p = q >> 3
        mask = np.where(p >= 0, 0xD5, 0x55)
        m = np.where(p >= 0, p, -p - 1)
        seg = (m[..., None] > np.array(_ALAW_ENDS)).sum(-1)
        code = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 0xF))
    else:
        raise ValueError("not a G.711 encoding: %r" % (encoding,))
    return ((code ^ mask) & 0xFF).astype(np.uint8)


def audio_encode_reference(rows, encoding):
    """The encoded audio collect's definition (include/airband_hip.h) in numpy.  rows [n][B] float32, encoding "s16" / "ulaw" / "alaw" or an AUDIO_* value ->
    (audio [n][B] int16 or uint8, info [n] of AUDIO_ROW_DTYPE with channel = the row's number)."""
    import numpy as np

    enc = audio_encoding_value(encoding)
    rows = np.ascontiguousarray(rows, np.float32)
    n, B = rows.shape
    q, clipped = audio_quantize_reference(rows)
    audio = q.astype("<i2") if enc == AUDIO_S16 else audio_law_reference(q, enc)
    info = np.zeros(n, AUDIO_ROW_DTYPE)
    info["channel"] = np.arange(n)
    nz = q != 0
    some = nz.any(axis=1)
    info["peak"] = np.abs(q).max(axis=1) if B else 0
    info["n_clipped"] = clipped.sum(axis=1)
    info["first"] = np.where(some, nz.argmax(axis=1), B)
    info["end"] = np.where(some, B - nz[:, ::-1].argmax(axis=1), 0)
    return audio, info


def audio_decode_reference(codes, encoding):
    """The standard G.711 expansion (ITU-T G.711; audioop.ulaw2lin / alaw2lin) of uint8 codes to int32 linear values on the int16 scale; the identity for S16."""
    import numpy as np

    enc = audio_encoding_value(encoding)
    if enc == AUDIO_S16:
        return np.asarray(codes).astype(np.int32)
    c = np.asarray(codes).astype(np.int32) & 0xFF
    if enc == AUDIO_ULAW:
        u = ~c & 0xFF
        t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
        return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int32)
    if enc == AUDIO_ALAW:
        a = c ^ 0x55
        t = (a & 0x0F) << 4
        seg = (a & 0x70) >> 4
        t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
        return np.where(a & 0x80, t, -t).astype(np.int32)
    raise ValueError("unknown encoding: %r" % (encoding,))


# the output decimation's (same header)
AUDIO_DECIMATION_PROTOTYPES = {
    "airband_hip_set_output_decimation": [_vp, _i32],
    "airband_hip_encoded_row_samples": [_vp],
    "airband_hip_decimate_audio": [_vp, _i32, _vp, _i64, _vp, _vp, _vp],
}
AUDIO_DECIMATE_HISTORY = 46  # q values a channel carries from batch to batch
_DECIMATE_SIDE = (10383, -3332, 1853, -1178, 781, -520, 339, -213, 126, -68, 32, -11)  # h[23 +- d], d = 1, 3, .. 23


def _decimate_taps():
    import numpy as np

    h = np.zeros(47, np.int64)
    h[23] = 16384
    for i, t in enumerate(_DECIMATE_SIDE):
        h[23 + 2 * i + 1] = h[23 - 2 * i - 1] = t
    h.setflags(write=False)
    return h


AUDIO_DECIMATE_TAPS = _decimate_taps()  # h[0 .. 46] in Q15 (AIRBAND_AUDIO_DECIMATE_TAPS values)


def audio_decimate_reference(rows, encoding, history=None):
    """The output decimation's definition (include/airband_hip.h) in numpy.  rows [n][B] float32 (B even), encoding "s16" / "ulaw" / "alaw" or an AUDIO_* value,
    history [n][46] int16 (None: zeros) -> (audio [n][B / 2] int16 or uint8, info [n] of AUDIO_ROW_DTYPE with channel = the row's number, history_out [n][46] int16)."""
    import numpy as np

    enc = audio_encoding_value(encoding)
    rows = np.ascontiguousarray(rows, np.float32)
    n, B = rows.shape
    if B % 2:
        raise ValueError("rows of an odd length: %d" % B)
    H, Bo = AUDIO_DECIMATE_HISTORY, B // 2
    hist = np.zeros((n, H), np.int64) if history is None else np.asarray(history).astype(np.int64).reshape(n, H)
    q, clipped = audio_quantize_reference(rows)
    S = np.concatenate([hist, q.astype(np.int64)], axis=1)
    acc = np.zeros((n, Bo), np.int64)
    for j, t in enumerate(AUDIO_DECIMATE_TAPS):
        if t:
            acc += int(t) * S[:, j:j + B:2]
    r = (acc + 16384) >> 15
    y = np.clip(r, -32767, 32767)
    audio = y.astype("<i2") if enc == AUDIO_S16 else audio_law_reference(y.astype(np.int32), enc)
    info = np.zeros(n, AUDIO_ROW_DTYPE)
    info["channel"] = np.arange(n)
    nz = y != 0
    some = nz.any(axis=1)
    info["peak"] = np.abs(y).max(axis=1) if Bo else 0
    info["n_clipped"] = clipped.sum(axis=1) + (y != r).sum(axis=1)
    info["first"] = np.where(some, nz.argmax(axis=1), Bo)
    info["end"] = np.where(some, Bo - nz[:, ::-1].argmax(axis=1), 0)
    return audio, info, S[:, B:].astype("<i2")


# the gated mixer collect's (same header)
MIXER_GATE_STEREO, MIXER_GATE_MANUAL_STEP = 0x1, 0x2
MIXER_GATE_PROTOTYPES = {
    "airband_hip_set_mixer_gate": [_vp, _vp, _i64, _i32, C.c_uint32],
    "airband_hip_mixer_gate_step": [_vp, _vp],
    "airband_hip_collect_active_mixers": [_vp, C.POINTER(_i64), _vp, _vp, _vp, _vp, _vp],
    "airband_hip_device_active_mixers": [_vp] + [C.POINTER(_vp)] * 5,
    "airband_hip_encode_mixer_audio": [_vp, _i32, _vp, _vp, _i64, _vp, _vp],
}


def mixer_rows_reference(left, right, encoding, stereo, mixers=None, stereo_flags=None):
    """The rows and records of the gated mixer collect (include/airband_hip.h) for the listed mixers: frames of left (stereo false) or of (left, right)
    interleaved, float32 or encoded by audio_encode_reference()'s arithmetic.  Returns (rows [n][W B] float32 / int16 / uint8, info [n] of AUDIO_ROW_DTYPE or
    None for AUDIO_F32).  mixers: default every row; stereo_flags [n_mixers]: the record's `reserved`, default 0."""
    import numpy as np

    enc = AUDIO_F32 if encoding is None else audio_encoding_value(encoding)
    left = np.ascontiguousarray(left, np.float32)
    n_all, B = left.shape
    mixers = np.arange(n_all) if mixers is None else np.asarray(mixers, np.int64)
    W = 2 if stereo else 1
    if stereo:
        right = np.ascontiguousarray(right, np.float32)
        rows = np.stack([left[mixers], right[mixers]], axis=2).reshape(len(mixers), 2 * B)  # L, R, L, R, ...
    else:
        rows = left[mixers].reshape(len(mixers), B)
    rows = np.ascontiguousarray(rows)
    if enc == AUDIO_F32:
        return rows, None
    audio, info = audio_encode_reference(rows, enc)
    info["channel"] = mixers
    # sample-indexed -> frame-indexed (nothing: first = W B -> B, end = 0 -> 0)
    info["first"] = info["first"].astype(np.int64) // W
    info["end"] = (info["end"].astype(np.int64) + W - 1) // W
    if stereo_flags is not None:
        info["reserved"] = (np.asarray(stereo_flags)[mixers] != 0).astype(np.uint32)
    return audio, info


def mixer_gate_reference(gate, max_rows, encoding, stereo, batches):
    """The gated mixer collect's definition (include/airband_hip.h) in numpy.  gate [n_mixers] GATE_* bytes; batches: a sequence of (left [n_mixers][B],
    right, has_signal [n_mixers], stereo_flags [n_mixers]) as collect_mixers() returns them at each step, in order; `prev` is carried across them and starts at
    0.  Returns one dict per batch: n_active, mixers (the first max_rows active mixers, ascending), rows (their bytes: float32 / int16 / uint8 [n][W B]) and
    info (records, None for AUDIO_F32)."""
    import numpy as np

    gate = np.asarray(gate, np.uint8)
    prev = np.zeros(len(gate), bool)
    out = []
    for left, right, has_signal, stereo_flags in batches:
        signal = np.asarray(has_signal) != 0
        active = (gate == GATE_ALWAYS) | ((gate == GATE_SIGNAL) & (signal | prev))
        prev = signal
        listed = np.flatnonzero(active)
        kept = listed[:int(max_rows)]
        rows, info = mixer_rows_reference(left, right, encoding, stereo, kept, stereo_flags)
        out.append(dict(n_active=int(len(listed)), mixers=kept.astype(np.int32), rows=rows, info=info))
    return out


# the transmission spool's (same header)
SPOOL_IDLE, SPOOL_MAX, SPOOL_FLUSH = 1, 2, 3


class Transmission(C.Structure):
    _fields_ = [("channel", C.c_int32), ("open_batch", C.c_uint32), ("last_batch", C.c_uint32), ("close_batch", C.c_uint32), ("n_rows", C.c_uint32),
                ("n_lost", C.c_uint32), ("n_clipped", C.c_uint32), ("peak", C.c_uint16), ("first", C.c_uint16), ("end", C.c_uint16), ("reason", C.c_uint16),
                ("row_offset", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class SpoolCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("steps", "open_now", "waiting_now", "free_rows_now", "finished_total", "dropped_transmissions", "rows_stored_total",
                                          "rows_lost_total")]


TRANSMISSION_SPOOL_PROTOTYPES = {
    "airband_hip_set_transmission_spool": [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32],
    "airband_hip_collect_transmissions": [_vp, C.POINTER(_i64), _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)],
    "airband_hip_spool_flush": [_vp],
    "airband_hip_spool_counters_get": [_vp, C.POINTER(SpoolCounters)],
    "airband_hip_device_transmission_spool": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
# numpy view of airband_hip_transmission
TRANSMISSION_DTYPE = [("channel", "<i4"), ("open_batch", "<u4"), ("last_batch", "<u4"), ("close_batch", "<u4"), ("n_rows", "<u4"), ("n_lost", "<u4"),
                      ("n_clipped", "<u4"), ("peak", "<u2"), ("first", "<u2"), ("end", "<u2"), ("reason", "<u2"), ("row_offset", "<u4"), ("reserved", "<u4", (2,))]
SPOOL_COUNTER_NAMES = tuple(f[0] for f in SpoolCounters._fields_)


# the mixer transmission spool's (same header): the channel spool's record, counters and definition over the mixer gate's rows
MIXER_SPOOL_PROTOTYPES = {
    "airband_hip_set_mixer_spool": [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32],
    "airband_hip_collect_mixer_transmissions": [_vp, C.POINTER(_i64), _vp, _vp, C.POINTER(_i64), C.POINTER(_i64)],
    "airband_hip_mixer_spool_flush": [_vp],
    "airband_hip_mixer_spool_counters_get": [_vp, C.POINTER(SpoolCounters)],
    "airband_hip_device_mixer_spool": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}


class mixer_gate_selection:
    """Every mixer the mixer gate's rule selects, step by step (include/airband_hip.h, "gated mixer collect", Step): what the spool's model needs as `selected`
    when the gate's count exceeds its list.  step(has_signal) -> the ascending mixers; `prev` is carried and starts at 0."""

    def __init__(self, gate):
        import numpy as np

        self.gate = np.asarray(gate, np.uint8)
        self.prev = np.zeros(len(self.gate), bool)

    def step(self, has_signal):
        import numpy as np

        signal = np.asarray(has_signal) != 0
        active = (self.gate == GATE_ALWAYS) | ((self.gate == GATE_SIGNAL) & (signal | self.prev))
        self.prev = signal
        return np.flatnonzero(active).astype(np.int32)


class transmission_spool_reference:
    """The definition of BOTH spools (include/airband_hip.h, "transmission spool" and "mixer transmission spool") in plain Python: an object that is fed, per
    step, what collect_active_encoded() of the same gate and encoding returns -- for the mixer spool what collect_active_mixers() of the same encoded mixer gate
    returns (n_active, mixers, audio, info), with wave_batch = B frames -- and that has flush(), collect() and counters() like the handle.  A finished record's
    reserved[1] is the OR of the stored records' `reserved` (0 for channels, a mixer's stereo flag).  When a mixer gate's count exceeds its list, `selected`
    comes from has_signal by the gate's rule (mixer_gate_selection).

    mask: truth value per channel (the spooled channels, resolved: the header's NULL is "every SIGNAL channel"); row_bytes: bytes of an encoded row;
    wave_batch: samples of a row.  step(n_active, channels, audio, info, selected=None): the gate's count, its list (the first max_rows selected channels,
    ascending), their encoded rows [n][...] and records [n] of AUDIO_ROW_DTYPE; `selected` is every channel the gate's rule selected, needed only when the count
    exceeds the list (the rows past max_rows are selected but not storable)."""

    def __init__(self, mask, wave_batch, pool_rows, export_rows, max_records, min_batches=8, idle_batches=4, max_batches=480):
        if max_batches < 1 or export_rows < max_batches + 1 or max_records < 1 or pool_rows < 1 or min_batches < 0 or idle_batches < 0:
            raise ValueError("parameters the handle would refuse")
        self.mask = [bool(m) for m in mask]
        self.wave_batch, self.pool_rows, self.export_rows, self.max_records = int(wave_batch), int(pool_rows), int(export_rows), int(max_records)
        self.min_batches, self.idle_batches, self.max_batches = int(min_batches), int(idle_batches), int(max_batches)
        self.steps = 0
        self.open = {}       # channel -> its running record (a dict) with "rows": the stored rows' bytes
        self.finished = []   # the finished list
        self.finished_total = self.dropped = self.rows_stored = self.rows_lost = 0

    def _held(self):
        return sum(t["n_rows"] for t in self.open.values()) + sum(t["n_rows"] for t in self.finished)

    def _finish(self, c, reason, close_batch):
        t = self.open.pop(c)
        t.update(reason=reason, close_batch=close_batch)
        if len(self.finished) >= self.max_records:
            self.dropped += 1  # its rows go back to the pool with it
        else:
            self.finished.append(t)
            self.finished_total += 1

    def step(self, n_active, channels, audio, info, selected=None):
        k = self.steps & 0xFFFFFFFF
        channels = [int(c) for c in channels]
        if selected is None:
            if int(n_active) != len(channels):
                raise ValueError("the gate selected %d channels and listed %d: pass `selected`" % (n_active, len(channels)))
            selected = channels
        selected = [int(c) for c in selected]
        if selected != sorted(selected) or selected[:len(channels)] != channels or len(selected) != int(n_active):
            raise ValueError("`selected` is not the gate's ascending selection with the list as its prefix")
        # phase A, entirely before phase B
        for c in sorted(self.open):
            t = self.open[c]
            age, quiet = (k - t["open_batch"]) & 0xFFFFFFFF, (k - t["last_batch"]) & 0xFFFFFFFF
            idle = age > self.min_batches and quiet > self.idle_batches
            if idle or age > self.max_batches:
                self._finish(c, SPOOL_IDLE if idle else SPOOL_MAX, k)
        # phase B
        free = self.pool_rows - self._held()
        row_of = {c: r for r, c in enumerate(channels)}
        j = 0
        for c in selected:
            if not self.mask[c]:
                continue
            t = self.open.get(c)
            if t is None:
                t = self.open[c] = dict(channel=c, open_batch=k, last_batch=0, n_rows=0, n_lost=0, n_clipped=0, peak=0, first=self.wave_batch, end=0, flags=0, rows=[])
            stored = False
            if c in row_of:  # storable
                stored = j < free
                j += 1
            if stored:
                r = row_of[c]
                rec = info[r]
                if int(rec["channel"]) != c:
                    raise ValueError("record %d is channel %d, the list says %d" % (r, int(rec["channel"]), c))
                t["rows"].append(audio[r].tobytes())
                t["peak"] = max(t["peak"], int(rec["peak"]))
                t["n_clipped"] = min(t["n_clipped"] + int(rec["n_clipped"]), 0xFFFFFFFF)
                if t["n_rows"] == 0:
                    t["first"] = int(rec["first"])
                t["end"] = int(rec["end"])
                t["flags"] |= int(rec["reserved"])
                t["n_rows"] += 1
                self.rows_stored += 1
            else:
                t["n_lost"] += 1
                self.rows_lost += 1
            t["last_batch"] = k
        self.steps += 1

    def flush(self):
        for c in sorted(self.open):
            self._finish(c, SPOOL_FLUSH, self.steps & 0xFFFFFFFF)

    def collect(self):
        """dict(records [n] of TRANSMISSION_DTYPE, audio: the rows' bytes concatenated, n_rows, n_waiting)"""
        import numpy as np

        n = total = 0
        while n < len(self.finished) and total + self.finished[n]["n_rows"] <= self.export_rows:
            total += self.finished[n]["n_rows"]
            n += 1
        take, self.finished = self.finished[:n], self.finished[n:]
        records = np.zeros(n, TRANSMISSION_DTYPE)
        at = 0
        for i, t in enumerate(take):
            for name in ("channel", "open_batch", "last_batch", "close_batch", "n_rows", "n_lost", "n_clipped", "peak", "first", "end", "reason"):
                records[i][name] = t[name]
            records[i]["row_offset"] = at
            records[i]["reserved"][1] = t["flags"]
            at += t["n_rows"]
        return dict(records=records, audio=b"".join(b"".join(t["rows"]) for t in take), n_rows=total, n_waiting=len(self.finished))

    def counters(self):
        return dict(steps=self.steps, open_now=len(self.open), waiting_now=len(self.finished), free_rows_now=self.pool_rows - self._held(),
                    finished_total=self.finished_total, dropped_transmissions=self.dropped, rows_stored_total=self.rows_stored, rows_lost_total=self.rows_lost)


# the RTP packet stream's (same header)
RTP_MARKER, RTP_FLUSH = 1, 2
RTP_PAYLOAD_TYPES = {AUDIO_ULAW: 0, AUDIO_ALAW: 8, AUDIO_S16: 96}  # PCMU, PCMA, and the first dynamic type for L16 at 8 or 16 kHz


class RtpSource(C.Structure):
    _fields_ = [("ssrc", C.c_uint32), ("ts0", C.c_uint32), ("seq0", C.c_uint16), ("payload_type", C.c_uint8), ("stream", C.c_uint8)]


class RtpPacket(C.Structure):
    _fields_ = [("channel", C.c_int32), ("timestamp", C.c_uint32), ("seq", C.c_uint16), ("length", C.c_uint16), ("flags", C.c_uint16), ("reserved", C.c_uint16)]


class RtpState(C.Structure):
    _fields_ = [("packets", C.c_uint32), ("octets", C.c_uint32), ("seq", C.c_uint16), ("carry", C.c_uint16), ("flags", C.c_uint32)]


class RtpCounters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("steps", "packets", "dropped_packets", "octets", "lost_rows")]


RTP_STREAM_PROTOTYPES = {
    "airband_hip_rtp_slot_bytes": [_i32, _i32],
    "airband_hip_set_rtp_stream": [_vp, _vp, _i32, _i64],
    "airband_hip_collect_rtp_packets": [_vp, C.POINTER(_i64), _vp, _vp, _vp],
    "airband_hip_collect_rtp_state": [_vp, _i64, _i64, _vp],
    "airband_hip_rtp_counters_get": [_vp, C.POINTER(RtpCounters)],
    "airband_hip_device_rtp_stream": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
# the mixer RTP stream's (same header): the channel stream's records, state, counters and definition over the mixer gate's rows
MIXER_RTP_PROTOTYPES = {
    "airband_hip_mixer_rtp_slot_bytes": [_i32, _i32, _i32],
    "airband_hip_set_mixer_rtp_stream": [_vp, _vp, _i32, _i64],
    "airband_hip_collect_mixer_rtp_packets": [_vp, C.POINTER(_i64), _vp, _vp, _vp],
    "airband_hip_collect_mixer_rtp_state": [_vp, _i64, _i64, _vp],
    "airband_hip_mixer_rtp_counters_get": [_vp, C.POINTER(RtpCounters)],
    "airband_hip_mixer_rtp_flush": [_vp],
    "airband_hip_device_mixer_rtp_stream": [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)],
}
# numpy views of airband_hip_rtp_source, _rtp_packet and _rtp_state
RTP_SOURCE_DTYPE = [("ssrc", "<u4"), ("ts0", "<u4"), ("seq0", "<u2"), ("payload_type", "u1"), ("stream", "u1")]
RTP_PACKET_DTYPE = [("channel", "<i4"), ("timestamp", "<u4"), ("seq", "<u2"), ("length", "<u2"), ("flags", "<u2"), ("reserved", "<u2")]
RTP_STATE_DTYPE = [("packets", "<u4"), ("octets", "<u4"), ("seq", "<u2"), ("carry", "<u2"), ("flags", "<u4")]
RTP_COUNTER_NAMES = tuple(f[0] for f in RtpCounters._fields_)


def mixer_rtp_slot_bytes(encoding, frame_samples, width=1) -> int:
    """slot_bytes of the header's definition ("mixer RTP stream"): 16 * ceil((12 + F * W * sample_bytes) / 16), F in frames of W samples; ValueError for what
    airband_hip_mixer_rtp_slot_bytes() refuses."""
    enc = audio_encoding_value(encoding)
    if enc not in (AUDIO_S16, AUDIO_ULAW, AUDIO_ALAW):
        raise ValueError("no encoding")
    if width not in (1, 2):
        raise ValueError("width is neither 1 nor 2")
    fb, F = (2 if enc == AUDIO_S16 else 1) * int(width), int(frame_samples)
    if F % 4 or F < 40 or 12 + F * fb > 1472:
        raise ValueError("frame_samples the handle would refuse")
    return (12 + F * fb + 15) // 16 * 16


def rtp_slot_bytes(encoding, frame_samples) -> int:
    """slot_bytes of the header's definition: 16 * ceil((12 + F * sample_bytes) / 16); ValueError for what airband_hip_rtp_slot_bytes() refuses."""
    return mixer_rtp_slot_bytes(encoding, frame_samples, 1)


class rtp_stream_reference:
    """The definition of BOTH RTP streams (include/airband_hip.h, "RTP packet stream" and "mixer RTP stream") in plain Python / numpy: a stateful object that
    is fed, per step, what collect_active_encoded() of the same gate and encoding returns -- for the mixer stream what collect_active_mixers() of the same
    encoded mixer gate returns (mixers, audio), with width = W samples per frame: rows are [n][W * wave_batch], and wave_batch, frame_samples, the carry and
    the timestamps count frames.  flush(): the step in which nobody is listed and k does not advance (the mixer stream's airband_hip_mixer_rtp_flush).

    sources: [n_channels] of RTP_SOURCE_DTYPE; encoding: "s16" / "ulaw" / "alaw" or an AUDIO_* value; wave_batch; frame_samples; max_packets.
    step(channels, audio, dropped=()): the gate's list (the first max_rows selected channels, ascending), their encoded rows [n][wave_batch] (int16 for "s16",
    else uint8) and the channels the rule selected but the list dropped past max_rows.  Returns (count, records, slots): the total (may exceed max_packets),
    records [min(count, max_packets)] of RTP_PACKET_DTYPE and slots [that many][slot_bytes] uint8, zero behind a packet's `length` (those bytes are undefined on
    the handle).  state() -> [n_channels] of RTP_STATE_DTYPE; counters() -> dict of RTP_COUNTER_NAMES."""

    def __init__(self, sources, encoding, wave_batch, frame_samples, max_packets, width=1):
        import numpy as np

        self.enc = audio_encoding_value(encoding)
        self.B, self.F, self.max_packets, self.W = int(wave_batch), int(frame_samples), int(max_packets), int(width)
        self.slot_bytes = mixer_rtp_slot_bytes(self.enc, self.F, self.W)
        if self.B % 4 or self.F > self.B or self.max_packets < 1:
            raise ValueError("parameters the handle would refuse")
        self.sb = (2 if self.enc == AUDIO_S16 else 1) * self.W  # bytes of a frame
        self.src = np.array(sources, RTP_SOURCE_DTYPE).reshape(-1).copy()
        if (self.src["payload_type"] > 127).any():
            raise ValueError("payload_type above 127")
        n = len(self.src)
        self.seq = [int(s) for s in self.src["seq0"]]
        self.carry = [b""] * n  # payload bytes as they go on the wire
        self.talking = [False] * n
        self.packets, self.octets = [0] * n, [0] * n
        self.k = 0
        self.totals = dict(packets=0, dropped_packets=0, octets=0, lost_rows=0)

    def _wire(self, row):
        import numpy as np

        row = np.ascontiguousarray(row)
        if self.enc == AUDIO_S16:
            return row.astype("<i2").astype(">i2").tobytes()  # L16 is network order
        return row.astype(np.uint8).tobytes()

    def flush(self):
        """nobody is listed: every carrying channel emits its flush packet, talking is cleared; k and `steps` do not advance.  Returns what step() returns."""
        return self.step((), (), advance=False)

    def step(self, channels, audio, dropped=(), advance=True):
        import numpy as np

        channels = [int(c) for c in channels]
        if channels != sorted(set(channels)):
            raise ValueError("the list is not ascending")
        row_of = {c: r for r, c in enumerate(channels)}
        dropped = set(int(c) for c in dropped)
        B, F, sb = self.B, self.F, self.sb
        out = []  # (channel, timestamp, seq, flags, header + payload)
        for c in range(len(self.src)):
            s = self.src[c]
            if not s["stream"]:
                continue
            if c in dropped:
                self.totals["lost_rows"] += 1
            cn = len(self.carry[c]) // sb
            ts_start = (int(s["ts0"]) + self.k * B - cn) & 0xFFFFFFFF
            emitted = []  # (timestamp, flags, payload)
            if c in row_of:
                S = self.carry[c] + self._wire(audio[row_of[c]])
                assert len(S) == (cn + B) * sb
                p = (cn + B) // F
                for j in range(p):
                    emitted.append(((ts_start + j * F) & 0xFFFFFFFF, RTP_MARKER if j == 0 and not self.talking[c] else 0, S[j * F * sb:(j + 1) * F * sb]))
                self.carry[c] = S[p * F * sb:]
                self.talking[c] = True
            else:
                if cn > 0:
                    emitted.append((ts_start, RTP_FLUSH, self.carry[c]))
                    self.carry[c] = b""
                self.talking[c] = False
            for ts, flags, payload in emitted:
                seq = self.seq[c]
                header = bytes([0x80, ((flags & RTP_MARKER) << 7) | int(s["payload_type"]), seq >> 8, seq & 0xFF]) + ts.to_bytes(4, "big") + int(s["ssrc"]).to_bytes(4, "big")
                out.append((c, ts, seq, flags, header + payload))
                self.seq[c] = (seq + 1) & 0xFFFF
                self.packets[c] = (self.packets[c] + 1) & 0xFFFFFFFF
                self.octets[c] = (self.octets[c] + len(payload)) & 0xFFFFFFFF
                self.totals["packets"] += 1
                self.totals["octets"] += len(payload)
        if advance:
            self.k += 1
        count, n = len(out), min(len(out), self.max_packets)
        self.totals["dropped_packets"] += count - n
        records = np.zeros(n, RTP_PACKET_DTYPE)
        slots = np.zeros((n, self.slot_bytes), np.uint8)
        for i, (c, ts, seq, flags, data) in enumerate(out[:n]):
            records[i] = (c, ts, seq, len(data), flags, 0)
            slots[i, :len(data)] = np.frombuffer(data, np.uint8)
        return count, records, slots

    def state(self):
        import numpy as np

        st = np.zeros(len(self.src), RTP_STATE_DTYPE)
        for c in range(len(self.src)):
            if self.src[c]["stream"]:
                st[c] = (self.packets[c], self.octets[c], self.seq[c], len(self.carry[c]) // self.sb, 1 if self.talking[c] else 0)
        return st

    def counters(self):
        return dict(steps=self.k, **self.totals)


def scope_window_hops(windows: int, wave_batch: int):
    """The batch's new hops whose FFT windows a band scope of `windows` windows per batch looks at: (j * WAVE_BATCH) / K, j = 0 .. K-1."""
    return [(j * wave_batch) // windows for j in range(windows)]
