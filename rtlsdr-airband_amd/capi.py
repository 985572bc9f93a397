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


def scope_window_hops(windows: int, wave_batch: int):
    """The batch's new hops whose FFT windows a band scope of `windows` windows per batch looks at: (j * WAVE_BATCH) / K, j = 0 .. K-1."""
    return [(j * wave_batch) // windows for j in range(windows)]
