"""rtlsdr-airband_amd -- MI355X (gfx950) backend for RTLSDR-Airband's demodulate() hot path.

Thin Python host binding over the C ABI in include/airband_hip.h (libairband_hip.so, built in-tree by
``_build.build()``).  The product is the shared library; this module only marshals configuration and numpy /
torch buffers into it for tests, bench.py and multi-GPU launch scripts.  There is no Python or CPU compute
path here: without the HIP library and a GPU every data-path call raises.

Import with ``importlib.import_module("rtlsdr-airband_amd")`` (the directory name carries a hyphen).
"""
from __future__ import annotations

import ctypes as C
import importlib
import os
from typing import Optional, Sequence

import numpy as np

capi = importlib.import_module(__name__ + ".capi")
siggen = importlib.import_module(__name__ + ".siggen")
_build = importlib.import_module(__name__ + "._build")

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AIRBAND_HIP_LIB") or os.path.join(HERE, "libairband_hip.so")  # env override: kernel experiments only

EXPORTS = [
    "airband_hip_prepare", "airband_hip_set_mixers", "airband_hip_release", "airband_hip_get_geometry", "airband_hip_last_error", "airband_hip_submit",
    "airband_hip_process", "airband_hip_process_device", "airband_hip_collect", "airband_hip_collect_mixers", "airband_hip_device_results",
    "airband_hip_synchronize", "airband_hip_process_bins", "airband_hip_read_bins", "airband_hip_read_trace", "airband_hip_channel_constants",
    "airband_hip_derive_constants", "airband_hip_last_timings", "airband_hip_channelizer_name", "airband_hip_set_signal_plan", "airband_hip_generate_iq",
    "airband_hip_flush", "airband_hip_timing_totals", "airband_hip_stream_wait_results", "airband_hip_mixer_enable_input",
    "airband_hip_device_enable", "airband_hip_gpu_count", "airband_hip_build_info", "airband_hip_dft_selftest", "airband_hip_collect_channels", "airband_hip_read_bins_channels", "airband_hip_read_trace_channels",
    "airband_hip_batch_ready", "airband_hip_mixer_set_stereo", "airband_hip_comm_unique_id", "airband_hip_comm_init_rank", "airband_hip_comm_init_all",
    "airband_hip_comm_group_begin", "airband_hip_comm_group_end", "airband_hip_allreduce_mixers", "airband_hip_add_mixers", "airband_hip_comm_destroy", "airband_hip_clear_mixers", "airband_hip_set_signal_plan_shift", "airband_hip_regrouped",
    "airband_hip_prepare_scan", "airband_hip_set_freq_index", "airband_hip_freq_stats",
    "airband_hip_set_scan_control", "airband_hip_scan_hold", "airband_hip_collect_scan_events", "airband_hip_collect_scan_state", "airband_hip_device_scan_control",
    "airband_hip_set_output_gate", "airband_hip_collect_active", "airband_hip_device_active",
    "airband_hip_set_output_encoding", "airband_hip_collect_active_encoded", "airband_hip_device_active_encoded", "airband_hip_encode_audio",
    "airband_hip_set_output_decimation", "airband_hip_encoded_row_samples", "airband_hip_decimate_audio",
    "airband_hip_set_mixer_gate", "airband_hip_mixer_gate_step", "airband_hip_collect_active_mixers", "airband_hip_device_active_mixers", "airband_hip_encode_mixer_audio",
    "airband_hip_set_transmission_spool", "airband_hip_collect_transmissions", "airband_hip_spool_flush", "airband_hip_spool_counters_get", "airband_hip_device_transmission_spool",
    "airband_hip_set_rtp_stream", "airband_hip_collect_rtp_packets", "airband_hip_collect_rtp_state", "airband_hip_rtp_counters_get", "airband_hip_device_rtp_stream", "airband_hip_rtp_slot_bytes",
    "airband_hip_set_mixer_spool", "airband_hip_collect_mixer_transmissions", "airband_hip_mixer_spool_flush", "airband_hip_mixer_spool_counters_get", "airband_hip_device_mixer_spool",
    "airband_hip_set_mixer_rtp_stream", "airband_hip_collect_mixer_rtp_packets", "airband_hip_collect_mixer_rtp_state", "airband_hip_mixer_rtp_counters_get", "airband_hip_mixer_rtp_flush", "airband_hip_device_mixer_rtp_stream", "airband_hip_mixer_rtp_slot_bytes",
    "airband_hip_set_band_scope", "airband_hip_collect_band_scope", "airband_hip_device_band_scope",
    "airband_hip_set_band_survey", "airband_hip_collect_band_survey", "airband_hip_device_band_survey",
    "airband_hip_set_band_watch", "airband_hip_collect_band_events", "airband_hip_collect_band_tracks", "airband_hip_device_band_watch",
    "airband_hip_prepare_follow", "airband_hip_set_band_follow", "airband_hip_collect_band_follow_changes", "airband_hip_collect_band_followers", "airband_hip_device_band_follow",
    "airband_hip_channelizer_reason", "airband_hip_wide_hop_lds_bytes", "airband_hip_schedule_info", "airband_hip_wide_hop_plan",
    "airband_hip_read_tables",
]
# Exported entries whose names carry digits.  Kept apart from EXPORTS, which tests/test_abi.py compares with the header's names through a pattern of letters and
# underscores only: a name with a digit in EXPORTS can never equal what that pattern finds.
EXPORTS_F32 = ["airband_hip_wide_hop_plan_f32"]

_lib = None


class DevicePtr:
    """A view of DEVICE memory the library owns (airband_hip_device_results) for consumers that stay on the GPU: `torch.as_tensor(DevicePtr(ptr, shape, "<f4"),
    device="cuda")` aliases the buffer through __cuda_array_interface__ -- no copy, no ownership.  bench.py reads the axcindicate row that way."""

    def __init__(self, ptr: int, shape, typestr: str):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2)


class AirbandError(RuntimeError):
    def __init__(self, code: int, text: str):
        super().__init__("airband_hip error %d: %s" % (code, text))
        self.code = code


def load_library() -> C.CDLL:
    """dlopen libairband_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libairband_hip.so is missing: run __graft_entry__.build() / python rtlsdr-airband_amd/_build.py (no CPU fallback exists)")
    # PyTorch-ROCm wheels bundle their own HIP runtime (file name libamdhip64.so, SONAME libamdhip64.so.7).  Loading
    # it FIRST makes the dynamic loader resolve our DT_NEEDED libamdhip64.so.7 to that same copy; the other order
    # would put two HIP runtimes into one process (and the second one finds no GPU).  C/C++ hosts are unaffected.
    try:
        import torch  # noqa: F401
    except Exception:  # noqa: BLE001
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_size_t
    L.airband_hip_prepare.argtypes = [C.POINTER(capi.Config), C.POINTER(vp)]
    L.airband_hip_prepare_scan.argtypes = [C.POINTER(capi.Config), C.POINTER(capi.ScanCfg), i32, C.POINTER(vp)]
    L.airband_hip_set_freq_index.argtypes = [vp, i32, i32]
    L.airband_hip_freq_stats.argtypes = [vp, i32, i32, C.POINTER(capi.ChannelStats)]
    L.airband_hip_set_mixers.argtypes = [vp, i32, C.POINTER(capi.MixerInput), i32]
    L.airband_hip_release.argtypes = [vp]
    L.airband_hip_release.restype = None
    L.airband_hip_get_geometry.argtypes = [vp, C.POINTER(capi.Geometry)]
    L.airband_hip_last_error.argtypes = [vp]
    L.airband_hip_last_error.restype = C.c_char_p
    L.airband_hip_submit.argtypes = [vp, i32, vp, sz]
    L.airband_hip_submit.restype = i64
    L.airband_hip_process.argtypes = [vp]
    L.airband_hip_batch_ready.argtypes = [vp]
    L.airband_hip_mixer_set_stereo.argtypes = [vp, i32, i32]
    L.airband_hip_comm_unique_id.argtypes = [vp]
    L.airband_hip_comm_init_rank.argtypes = [vp, vp, i32, i32]
    L.airband_hip_comm_init_all.argtypes = [C.POINTER(vp), i32]
    L.airband_hip_allreduce_mixers.argtypes = [vp, vp]
    L.airband_hip_add_mixers.argtypes = [vp, vp]
    L.airband_hip_comm_destroy.argtypes = [vp]
    L.airband_hip_clear_mixers.argtypes = [vp]
    L.airband_hip_comm_group_begin.argtypes = []
    L.airband_hip_comm_group_end.argtypes = []
    L.airband_hip_process_device.argtypes = [vp, vp, sz, vp]
    L.airband_hip_collect.argtypes = [vp, vp, vp, vp, vp]
    L.airband_hip_collect_channels.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    L.airband_hip_read_bins_channels.argtypes = [vp, i64, i64, vp, vp]
    L.airband_hip_read_trace_channels.argtypes = [vp, i64, i64, vp]
    L.airband_hip_set_output_gate.argtypes = [vp, vp, i64]
    L.airband_hip_collect_active.argtypes = [vp, C.POINTER(i64), vp, vp, vp, vp]
    L.airband_hip_device_active.argtypes = [vp] + [C.POINTER(vp)] * 4
    for name, argtypes in list(capi.BAND_SCOPE_PROTOTYPES.items()) + list(capi.BAND_SURVEY_PROTOTYPES.items()) + list(capi.BAND_WATCH_PROTOTYPES.items()) + list(capi.BAND_FOLLOW_PROTOTYPES.items()) + list(capi.AUDIO_ENCODING_PROTOTYPES.items()) + list(capi.AUDIO_DECIMATION_PROTOTYPES.items()) + list(capi.SCAN_CONTROL_PROTOTYPES.items()) + list(capi.TRANSMISSION_SPOOL_PROTOTYPES.items()) + list(capi.TABLES_PROTOTYPES.items()) + list(capi.MIXER_GATE_PROTOTYPES.items()) + list(capi.MIXER_SPOOL_PROTOTYPES.items()) + list(capi.RTP_STREAM_PROTOTYPES.items()) + list(capi.MIXER_RTP_PROTOTYPES.items()):
        if hasattr(L, name):  # (AIRBAND_HIP_LIB may name an older build for an A/B measurement: scripts/band_scope_profile.py --parent-lib)
            getattr(L, name).argtypes = argtypes
    L.airband_hip_collect_mixers.argtypes = [vp, vp, vp, vp]
    L.airband_hip_device_results.argtypes = [vp] + [C.POINTER(vp)] * 6
    L.airband_hip_synchronize.argtypes = [vp]
    L.airband_hip_process_bins.argtypes = [vp, vp, vp]
    L.airband_hip_read_bins.argtypes = [vp, vp, vp]
    L.airband_hip_read_trace.argtypes = [vp, vp]
    L.airband_hip_channel_constants.argtypes = [vp, i32, C.POINTER(C.c_double)]
    L.airband_hip_derive_constants.argtypes = [C.POINTER(capi.Config), i32, C.POINTER(C.c_double)]
    L.airband_hip_last_timings.argtypes = [vp, C.POINTER(C.c_float)]
    L.airband_hip_channelizer_name.argtypes = [vp]
    L.airband_hip_channelizer_name.restype = C.c_char_p
    L.airband_hip_channelizer_reason.argtypes = [vp]
    L.airband_hip_channelizer_reason.restype = C.c_char_p
    L.airband_hip_wide_hop_lds_bytes.argtypes = [i32, i32, i32]
    L.airband_hip_wide_hop_lds_bytes.restype = i64
    L.airband_hip_wide_hop_plan.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i64)]
    L.airband_hip_wide_hop_plan_f32.argtypes = [i32, i32, C.POINTER(i32), C.POINTER(i64)]
    L.airband_hip_set_signal_plan.argtypes = [vp, vp, i32, i32, vp]
    L.airband_hip_generate_iq.argtypes = [vp, vp, sz, u64, sz, u64, i32, vp]
    L.airband_hip_set_signal_plan_shift.argtypes = [vp, i32, C.c_uint32]
    L.airband_hip_regrouped.argtypes = [vp]
    L.airband_hip_schedule_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.airband_hip_dft_selftest.argtypes = [C.POINTER(capi.Config), i32, C.POINTER(C.c_double)]
    L.airband_hip_build_info.argtypes = []
    L.airband_hip_build_info.restype = C.c_char_p
    L.airband_hip_flush.argtypes = [vp]
    L.airband_hip_mixer_enable_input.argtypes = [vp, i32, i32]
    L.airband_hip_device_enable.argtypes = [vp, i32, i32]
    L.airband_hip_gpu_count.argtypes = []
    L.airband_hip_stream_wait_results.argtypes = [vp, vp]
    L.airband_hip_timing_totals.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), i32]
    _lib = L
    return L


def make_config(devices: Sequence[dict], *, wave_rate: int, fft_log: int = 9, fm_demod: int = 0, flags: int = 0, hip_device: int = 0):
    """devices: list of dict(channels=[channel kwargs | ChannelCfg], sample_rate=, centerfreq=, sfmt=, fullscale=, tau_us=)."""
    keep, devs = [], []
    for dev in devices:
        dc, arr = capi.device_cfg(**dev)
        keep.append(arr)
        devs.append(dc)
    darr = (capi.DeviceCfg * len(devs))(*devs)
    keep.append(darr)
    cfg = capi.Config(capi.ABI_VERSION, flags, fft_log, wave_rate, fm_demod, hip_device, len(devs), C.cast(darr, C.POINTER(capi.DeviceCfg)))
    return cfg, keep


def derive_constants(devices: Sequence[dict], channel_index: int, *, wave_rate: int, fft_log: int = 9, fm_demod: int = 0):
    """The 16 derived per-channel constants, computed by the library's host code (no GPU needed)."""
    L = load_library()
    cfg, keep = make_config(devices, wave_rate=wave_rate, fft_log=fft_log, fm_demod=fm_demod)
    v = (C.c_double * 16)()
    rc = L.airband_hip_derive_constants(C.byref(cfg), channel_index, v)
    if rc != 0:
        raise AirbandError(rc, (L.airband_hip_last_error(None) or b"").decode())
    return list(v)


def dft_selftest(devices: Sequence[dict], *, wave_rate: int, fft_log: int = 9, windows: int = 2, flags: int = 0) -> float:
    """Largest relative error of the matrix-core channelizer's coefficient tables for this configuration (host arithmetic, no GPU).
    flags: capi.FLAG_WIDE_HOPS admits hops beyond the ordinary limits, as it does for a handle."""
    L = load_library()
    cfg, keep = make_config(devices, wave_rate=wave_rate, fft_log=fft_log, flags=flags)
    err = C.c_double(0.0)
    rc = L.airband_hip_dft_selftest(C.byref(cfg), windows, C.byref(err))
    if rc != 0:
        raise AirbandError(rc, (L.airband_hip_last_error(None) or b"").decode())
    return float(err.value)


def wide_hop_lds_bytes(fft_size: int, hop_bytes: int, sfmt: int) -> int:
    """LDS per workgroup of the wide-hop staging (capi.FLAG_WIDE_HOPS) for this shape, -1 where the shape is not a wide one (no GPU needed)."""
    return int(load_library().airband_hip_wide_hop_lds_bytes(fft_size, hop_bytes, sfmt))


def wide_hop_plan(fft_size: int, hop_bytes: int, sfmt: int):
    """(segments, lds_bytes): the staging plan a capi.FLAG_WIDE_HOPS handle uses for this shape (no GPU needed).  AirbandError(EBADSIZE) where such a handle stays on
    the wavefront FFT or the shape is not a wide one."""
    seg, lds = C.c_int32(0), C.c_int64(0)
    rc = load_library().airband_hip_wide_hop_plan(fft_size, hop_bytes, sfmt, C.byref(seg), C.byref(lds))
    if rc != 0:
        raise AirbandError(rc, "no wide-hop plan for fft %d, hops of %d bytes, sample format %d" % (fft_size, hop_bytes, sfmt))
    return int(seg.value), int(lds.value)


def wide_hop_plan_f32(fft_size: int, hop_samples: int):
    """(segments, lds_bytes): the staging plan a capi.FLAG_WIDE_HOPS handle of CF32 dongles uses for this shape (no GPU needed).  AirbandError(EBADSIZE) where the hop is
    inside the ordinary float kernel's limits (the flag changes nothing there) or the shape has no plan."""
    seg, lds = C.c_int32(0), C.c_int64(0)
    rc = load_library().airband_hip_wide_hop_plan_f32(fft_size, hop_samples, C.byref(seg), C.byref(lds))
    if rc != 0:
        raise AirbandError(rc, "no CF32 wide-hop plan for fft %d, hops of %d samples" % (fft_size, hop_samples))
    return int(seg.value), int(lds.value)


def make_scan(scan: Optional[dict]):
    """scan = {device index: [channel kwargs | ChannelCfg, ...]} -> (ScanCfg array or None, count, keepalive)."""
    if not scan:
        return None, 0, []
    keep, rows = [], []
    for dev, entries in scan.items():
        chs = [c if isinstance(c, capi.ChannelCfg) else capi.channel_cfg(**c) for c in entries]
        arr = (capi.ChannelCfg * len(chs))(*chs)
        keep.append(arr)
        rows.append(capi.ScanCfg(int(dev), len(chs), C.cast(arr, C.POINTER(capi.ChannelCfg))))
    sarr = (capi.ScanCfg * len(rows))(*rows)
    keep.append(sarr)
    return C.cast(sarr, C.POINTER(capi.ScanCfg)), len(rows), keep


def prepare_scan_rc(devices: Sequence[dict], scan: Optional[dict], *, wave_rate: int, fft_log: int = 9, fm_demod: int = 0, flags: int = 0) -> int:
    """airband_hip_prepare_scan()'s return code for this configuration (the handle, if one was made, is released at once).  Lets tests check the
    validation of scan lists, which happens before any device is touched."""
    L = load_library()
    cfg, keep = make_config(devices, wave_rate=wave_rate, fft_log=fft_log, fm_demod=fm_demod, flags=flags)
    sptr, n, skeep = make_scan(scan)
    h = C.c_void_p()
    rc = L.airband_hip_prepare_scan(C.byref(cfg), sptr, n, C.byref(h))
    if h:
        L.airband_hip_release(h)
    return rc


def prepare_follow_rc(devices: Sequence[dict], scan: Optional[dict], follow, *, wave_rate: int, fft_log: int = 9, fm_demod: int = 0, flags: int = 0):
    """(return code, error text) of airband_hip_prepare_follow() for this configuration (the handle, if one was made, is released at once).  Lets tests check the
    validation of followers, which happens before any device is touched.  follow: device-major channel indices, or None for (NULL, 0)."""
    L = load_library()
    cfg, keep = make_config(devices, wave_rate=wave_rate, fft_log=fft_log, fm_demod=fm_demod, flags=flags)
    sptr, n, skeep = make_scan(scan)
    farr = (C.c_int32 * len(follow))(*[int(c) for c in follow]) if follow is not None else None
    h = C.c_void_p()
    rc = L.airband_hip_prepare_follow(C.byref(cfg), sptr, n, farr, len(follow) if follow is not None else 0, C.byref(h))
    if h:
        L.airband_hip_release(h)
    return rc, (L.airband_hip_last_error(None) or b"").decode() if rc != 0 else ""


class AirbandHip:
    """One handle = the dongles demodulated on one GPU (the reference's demodulate() thread for a device shard,
    src/rtl_airband.cpp:1052-1086)."""

    def __init__(self, devices: Sequence[dict], *, wave_rate: int, fft_log: int = 9, fm_demod: int = 0, flags: int = 0, hip_device: int = 0,
                 scan: Optional[dict] = None, follow: Optional[Sequence[int]] = None):
        """scan = {device index: [channel kwargs, ...]}: scan-mode devices (airband_hip_prepare_scan); each list's first entry must equal the device's channel.
        follow = [device-major channel index, ...] ascending: the followers (airband_hip_prepare_follow) -- spare AM channels the band follow may tune onto the
        carriers the band watch confirms (set_band_follow); such a handle schedules like one with AFC channels: no run-ahead, FLAG_PIPELINE ignored."""
        self.L = load_library()
        self.devices = list(devices)
        self.follow_channels = [int(c) for c in follow] if follow else []
        self.scan_devices = sorted(int(d) for d in scan) if scan else []
        cfg, self._keep = make_config(devices, wave_rate=wave_rate, fft_log=fft_log, fm_demod=fm_demod, flags=flags, hip_device=hip_device)
        h = C.c_void_p()
        if self.follow_channels:
            sptr, n, skeep = make_scan(scan)
            self._keep.append(skeep)
            farr = (C.c_int32 * len(self.follow_channels))(*self.follow_channels)
            rc = self.L.airband_hip_prepare_follow(C.byref(cfg), sptr, n, farr, len(self.follow_channels), C.byref(h))
        elif scan:
            sptr, n, skeep = make_scan(scan)
            self._keep.append(skeep)
            rc = self.L.airband_hip_prepare_scan(C.byref(cfg), sptr, n, C.byref(h))
        else:
            rc = self.L.airband_hip_prepare(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise AirbandError(rc, (self.L.airband_hip_last_error(None) or b"").decode())
        self.h = h
        g = capi.Geometry()
        self._check(self.L.airband_hip_get_geometry(self.h, C.byref(g)))
        self.geometry = g
        self.B = g.wave_batch
        self.total_channels = g.total_channels
        self.n_mixers = 0
        self.gate_rows = 0  # capacity of the packed buffers once set_output_gate() has run

    # ---- plumbing ------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc < 0:
            raise AirbandError(rc, (self.L.airband_hip_last_error(self.h) or b"").decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.airband_hip_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- data path -----------------------------------------------------------------------------------
    def submit(self, dev: int, iq: np.ndarray) -> int:
        iq = np.ascontiguousarray(iq)
        return self._check(self.L.airband_hip_submit(self.h, dev, iq.ctypes.data, iq.nbytes))

    def process(self) -> bool:
        rc = self.L.airband_hip_process(self.h)
        if rc == capi.EAGAIN:
            return False
        self._check(rc)
        return True

    def process_device(self, d_iq_ptr: int, stride_bytes: int, stream: int = 0):
        self._check(self.L.airband_hip_process_device(self.h, C.c_void_p(d_iq_ptr), stride_bytes, C.c_void_p(stream)))

    def collect(self, *, iq: bool = False, stats: bool = False, first_channel: Optional[int] = None, n_channels: Optional[int] = None):
        """Results of the last batch; with first_channel / n_channels only that channel range (airband_hip_collect_channels:
        repeatable, does not mark the batch as collected)."""
        ranged = first_channel is not None
        n, B = (int(n_channels) if ranged else self.total_channels), self.B
        wave = np.empty((n, B), np.float32)
        axc = np.empty((n,), np.uint8)
        iqo = np.empty((n, 2 * B), np.float32) if iq else None
        st = (capi.ChannelStats * n)() if stats else None
        args = (wave.ctypes.data, iqo.ctypes.data if iq else None, axc.ctypes.data, C.cast(st, C.c_void_p) if stats else None)
        if ranged:
            self._check(self.L.airband_hip_collect_channels(self.h, int(first_channel), n, *args))
        else:
            self._check(self.L.airband_hip_collect(self.h, *args))
        out = dict(waveout=wave, axc=axc)
        if iq:
            out["iq_out"] = iqo
        if stats:
            out["stats"] = [{f[0]: getattr(s, f[0]) for f in capi.ChannelStats._fields_} for s in st]
        return out

    def set_output_gate(self, gate, max_rows: Optional[int] = None):
        """gate: one capi.GATE_NEVER / GATE_SIGNAL / GATE_ALWAYS byte per channel (device-major); max_rows: capacity of the packed buffers, default every
        channel.  Before the first batch (airband_hip_set_output_gate)."""
        gate = np.ascontiguousarray(gate, np.uint8)
        if gate.shape != (self.total_channels,):
            raise ValueError("gate needs one byte per channel (%d), got shape %r" % (self.total_channels, gate.shape))
        rows = self.total_channels if max_rows is None else int(max_rows)
        self._check(self.L.airband_hip_set_output_gate(self.h, gate.ctypes.data, rows))
        self.gate_rows = rows
        self.gate_bytes = gate.copy()  # set_rtp_stream()'s default sources: every channel whose gate is not NEVER
        self.audio_encoding = capi.AUDIO_F32  # a new gate drops the encoding
        self.audio_decimation = 1  # ... and its decimation
        self.rtp = None  # ... and the RTP stream with it

    def collect_active(self, *, iq: bool = False) -> dict:
        """The batch collect() would return, packed to the channels the gate selected (airband_hip_collect_active): n_active (may exceed the capacity: only
        the first max_rows channels were kept then), channels [n] ascending, waveout [n][B], iq_out [n][2 B] (iq=True), axcindicate of every channel."""
        rows, B = max(self.gate_rows, 1), self.B
        n = C.c_int64(0)
        idx = np.empty((rows,), np.int32)
        wave = np.empty((rows, B), np.float32)
        iqo = np.empty((rows, 2 * B), np.float32) if iq else None
        axc = np.empty((self.total_channels,), np.uint8)
        self._check(self.L.airband_hip_collect_active(self.h, C.byref(n), idx.ctypes.data, wave.ctypes.data, iqo.ctypes.data if iq else None, axc.ctypes.data))
        kept = min(int(n.value), rows)
        out = dict(n_active=int(n.value), channels=idx[:kept], waveout=wave[:kept], axcindicate=axc)
        if iq:
            out["iq_out"] = iqo[:kept]
        return out

    def device_active(self) -> dict:
        """Device pointers of the packed results (valid until the next process call): index [max_rows] int32, count [1] int32, rows [max_rows][B] float32,
        iq_rows [max_rows][2 B] float32 (0 on a handle without raw-I/Q outputs)."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.airband_hip_device_active(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["index", "count", "rows", "iq_rows"], ptrs)}

    def set_output_encoding(self, encoding):
        """encoding: "s16", "ulaw", "alaw" or None (capi.AUDIO_* values are taken too): the gate's rows are also delivered as int16 or G.711 bytes with one record
        per row (airband_hip_set_output_encoding).  After set_output_gate(), before the first batch; None removes it."""
        enc = capi.AUDIO_F32 if encoding is None else capi.audio_encoding_value(encoding)
        self._check(self.L.airband_hip_set_output_encoding(self.h, enc))
        self.audio_encoding = enc
        self.audio_decimation = 1  # a new encoding drops the decimation
        self.rtp = None  # ... and the RTP stream

    def set_output_decimation(self, factor):
        """factor: 2, or None / 1 to remove it (airband_hip_set_output_decimation): behind the gate a listed row of B samples becomes B / 2 encoded samples through
        an integer half-band FIR with a per-channel history.  After set_output_encoding(), before the first batch; it drops a transmission spool and an RTP stream."""
        f = 1 if factor is None else int(factor)
        self._check(self.L.airband_hip_set_output_decimation(self.h, f))
        self.audio_decimation = f
        self.rtp = None
        self.spool_export_rows = self.spool_max_records = 0

    def encoded_row_samples(self) -> int:
        """Samples of an encoded row (airband_hip_encoded_row_samples): B, or B / 2 on a decimating handle."""
        return self._check(self.L.airband_hip_encoded_row_samples(self.h))

    def _encoded_row(self) -> int:
        """encoded_row_samples() for sizing a collect's arrays; B on a handle without an encoding (the call then reports the error itself)"""
        n = self.L.airband_hip_encoded_row_samples(self.h) if hasattr(self.L, "airband_hip_encoded_row_samples") else self.B
        return n if n > 0 else self.B

    def _audio_dtype(self, enc):
        return np.dtype("<i2") if enc == capi.AUDIO_S16 else np.dtype(np.uint8)

    def collect_active_encoded(self) -> dict:
        """collect_active() with encoded rows (airband_hip_collect_active_encoded): n_active, channels [n] ascending, audio [n][B] int16 ("s16") or uint8 (G.711),
        info [n] of capi.AUDIO_ROW_DTYPE, axcindicate of every channel.  On a decimating handle the rows are encoded_row_samples() = B / 2 long."""
        rows, B = max(self.gate_rows, 1), self._encoded_row()
        n = C.c_int64(0)
        idx = np.empty((rows,), np.int32)
        audio = np.empty((rows, B), self._audio_dtype(getattr(self, "audio_encoding", capi.AUDIO_F32)))
        info = np.empty((rows,), capi.AUDIO_ROW_DTYPE)
        axc = np.empty((self.total_channels,), np.uint8)
        self._check(self.L.airband_hip_collect_active_encoded(self.h, C.byref(n), idx.ctypes.data, audio.ctypes.data, info.ctypes.data, axc.ctypes.data))
        kept = min(int(n.value), rows)
        return dict(n_active=int(n.value), channels=idx[:kept], audio=audio[:kept], info=info[:kept], axcindicate=axc)

    def device_active_encoded(self) -> dict:
        """Device pointers of the encoded results (valid until the next process call): audio [max_rows][B] int16 or bytes, info [max_rows] of 16 bytes; the list
        and the count are device_active()'s."""
        ptrs = [C.c_void_p() for _ in range(2)]
        self._check(self.L.airband_hip_device_active_encoded(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["audio", "info"], ptrs)}

    def encode_audio(self, rows, encoding):
        """The encoder on host rows [n][B] float32 (airband_hip_encode_audio): (audio [n][B] int16 or uint8, info [n] of capi.AUDIO_ROW_DTYPE, channel = row)."""
        enc = capi.audio_encoding_value(encoding)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.B:
            raise ValueError("rows must be [n][%d], got shape %r" % (self.B, rows.shape))
        n = rows.shape[0]
        audio = np.empty((n, self.B), self._audio_dtype(enc))
        info = np.empty((n,), capi.AUDIO_ROW_DTYPE)
        self._check(self.L.airband_hip_encode_audio(self.h, enc, rows.ctypes.data, n, audio.ctypes.data, info.ctypes.data))
        return audio, info

    def decimate_audio(self, rows, encoding, history=None):
        """The decimating kernel on host rows [n][B] float32 (airband_hip_decimate_audio): (audio [n][B / 2] int16 or uint8, info [n] of capi.AUDIO_ROW_DTYPE,
        history [n][46] int16 to hand to the next call on the rows that follow; None in means zeros)."""
        enc = capi.audio_encoding_value(encoding)
        rows = np.ascontiguousarray(rows, np.float32)
        if rows.ndim != 2 or rows.shape[1] != self.B:
            raise ValueError("rows must be [n][%d], got shape %r" % (self.B, rows.shape))
        n = rows.shape[0]
        hist = np.zeros((n, capi.AUDIO_DECIMATE_HISTORY), "<i2") if history is None else np.array(history, "<i2", order="C")
        if hist.shape != (n, capi.AUDIO_DECIMATE_HISTORY):
            raise ValueError("history must be [%d][%d], got shape %r" % (n, capi.AUDIO_DECIMATE_HISTORY, hist.shape))
        audio = np.empty((n, self.B // 2), self._audio_dtype(enc))
        info = np.empty((n,), capi.AUDIO_ROW_DTYPE)
        self._check(self.L.airband_hip_decimate_audio(self.h, enc, rows.ctypes.data, n, hist.ctypes.data, audio.ctypes.data, info.ctypes.data))
        return audio, info, hist

    def set_transmission_spool(self, pool_rows, export_rows=None, max_records=None, mask=None, min_batches=8, idle_batches=4, max_batches=480):
        """Transmission spool (airband_hip_set_transmission_spool): the GPU keeps the encoded rows of every open transmission and hands over finished ones.
        export_rows: default max(pool_rows, max_batches + 1); max_records: default the channel count; mask: one byte per channel (None = every SIGNAL channel).
        After set_output_encoding(), before the first batch; pool_rows 0 removes it."""
        pool_rows = int(pool_rows)
        export_rows = max(pool_rows, max_batches + 1) if export_rows is None else int(export_rows)
        max_records = self.total_channels if max_records is None else int(max_records)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (self.total_channels,):
            raise ValueError("mask must have one byte per channel")
        self._check(self.L.airband_hip_set_transmission_spool(self.h, None if m is None else m.ctypes.data, pool_rows, export_rows, max_records, min_batches, idle_batches, max_batches))
        self.spool_export_rows, self.spool_max_records = (export_rows, max_records) if pool_rows else (0, 0)

    def collect_transmissions(self) -> dict:
        """The finished transmissions that fit the export buffer (airband_hip_collect_transmissions): records [n] of capi.TRANSMISSION_DTYPE, audio
        [sum of n_rows][B] int16 ("s16") or uint8 (G.711) -- transmission i's rows are audio[row_offset : row_offset + n_rows] -- and n_waiting."""
        enc = getattr(self, "audio_encoding", capi.AUDIO_F32)
        records = np.empty((max(getattr(self, "spool_max_records", 0), 1),), capi.TRANSMISSION_DTYPE)
        audio = np.empty((max(getattr(self, "spool_export_rows", 0), 1), self._encoded_row()), self._audio_dtype(enc))
        n, n_rows, n_waiting = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self.L.airband_hip_collect_transmissions(self.h, C.byref(n), records.ctypes.data, audio.ctypes.data, C.byref(n_rows), C.byref(n_waiting)))
        return dict(records=records[:n.value], audio=audio[:n_rows.value], n_waiting=int(n_waiting.value))

    def spool_flush(self):
        """Every open transmission finishes with reason capi.SPOOL_FLUSH (airband_hip_spool_flush)."""
        self._check(self.L.airband_hip_spool_flush(self.h))

    def spool_counters(self) -> dict:
        """airband_hip_spool_counters_get as a dict (capi.SPOOL_COUNTER_NAMES)."""
        out = capi.SpoolCounters()
        self._check(self.L.airband_hip_spool_counters_get(self.h, C.byref(out)))
        return {k: int(getattr(out, k)) for k in capi.SPOOL_COUNTER_NAMES}

    def device_transmission_spool(self) -> dict:
        """Device pointers of the last collect_transmissions() (valid until the next one): audio [export_rows][row bytes], records [max_records] of 48 bytes,
        n_export [3] int32 (transmissions, rows, still waiting)."""
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self.L.airband_hip_device_transmission_spool(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["audio", "records", "n_export"], ptrs)}

    # ---- RTP packet stream (include/airband_hip.h) ---------------------------------------------------------------------------------------
    def set_rtp_stream(self, frame_samples=None, sources=None, max_packets=None, *, remove: bool = False):
        """RTP packet stream (airband_hip_set_rtp_stream): the GPU frames the gate's encoded rows as RTP packets of frame_samples, carrying the remainder per
        channel.  frame_samples: default wave_rate // 50 (20 ms); sources: [total_channels] of capi.RTP_SOURCE_DTYPE, default every channel whose gate is not
        NEVER with ssrc = its index, ts0 = 0, seq0 = 0 and payload type 0 / 8 / 96 for ulaw / alaw / s16; max_packets: default what a step can emit at most.
        After set_output_encoding(), before the first batch; remove=True removes it."""
        if remove:
            self._check(self.L.airband_hip_set_rtp_stream(self.h, None, 0, 0))
            self.rtp = None
            return
        enc = getattr(self, "audio_encoding", capi.AUDIO_F32)
        row = self._encoded_row()  # B, or B / 2 behind the output decimation: 20 ms are half as many samples there
        F = int(self.geometry.wave_rate) * row // self.B // 50 if frame_samples is None else int(frame_samples)
        if sources is None:
            src = np.zeros(self.total_channels, capi.RTP_SOURCE_DTYPE)
            src["ssrc"] = np.arange(self.total_channels)
            src["payload_type"] = capi.RTP_PAYLOAD_TYPES.get(enc, 0)
            src["stream"] = getattr(self, "gate_bytes", np.zeros(self.total_channels, np.uint8)) != capi.GATE_NEVER
        else:
            src = np.ascontiguousarray(sources, capi.RTP_SOURCE_DTYPE)
            if src.shape != (self.total_channels,):
                raise ValueError("sources needs one record per channel (%d), got shape %r" % (self.total_channels, src.shape))
        if max_packets is None:
            max_packets = max(1, int(np.count_nonzero(src["stream"])) * ((max(F, 4) - 4 + row) // max(F, 1)))
        self._check(self.L.airband_hip_set_rtp_stream(self.h, src.ctypes.data, F, int(max_packets)))
        self.rtp = dict(frame_samples=F, max_packets=int(max_packets), slot_bytes=self._check(self.L.airband_hip_rtp_slot_bytes(enc, F)), sources=src)

    def _rtp(self):
        return getattr(self, "rtp", None) or dict(frame_samples=0, max_packets=1, slot_bytes=16, sources=None)

    def collect_rtp_packets(self) -> dict:
        """The batch's RTP packets (airband_hip_collect_rtp_packets): n_packets (may exceed max_packets: only the first max_packets were written then), records
        [n] of capi.RTP_PACKET_DTYPE, packets [n][slot_bytes] uint8 -- packet i is packets[i, :records[i]["length"]] -- and axcindicate of every channel."""
        r = self._rtp()
        n = C.c_int64(0)
        records = np.empty((r["max_packets"],), capi.RTP_PACKET_DTYPE)
        packets = np.empty((r["max_packets"], r["slot_bytes"]), np.uint8)
        axc = np.empty((self.total_channels,), np.uint8)
        self._check(self.L.airband_hip_collect_rtp_packets(self.h, C.byref(n), records.ctypes.data, packets.ctypes.data, axc.ctypes.data))
        kept = min(int(n.value), r["max_packets"])
        return dict(n_packets=int(n.value), records=records[:kept], packets=packets[:kept], axcindicate=axc)

    def collect_rtp_state(self, first_channel: int = 0, n_channels: Optional[int] = None):
        """The channels' sender state (airband_hip_collect_rtp_state): [n_channels] of capi.RTP_STATE_DTYPE, default every channel."""
        n = self.total_channels - int(first_channel) if n_channels is None else int(n_channels)
        st = np.empty((max(n, 0),), capi.RTP_STATE_DTYPE)
        self._check(self.L.airband_hip_collect_rtp_state(self.h, int(first_channel), n, st.ctypes.data))
        return st

    def rtp_counters(self) -> dict:
        """airband_hip_rtp_counters_get as a dict (capi.RTP_COUNTER_NAMES)."""
        out = capi.RtpCounters()
        self._check(self.L.airband_hip_rtp_counters_get(self.h, C.byref(out)))
        return {k: int(getattr(out, k)) for k in capi.RTP_COUNTER_NAMES}

    def device_rtp_stream(self) -> dict:
        """Device pointers of the batch's packets (valid until the next process call): n_packets [1] int32, records [max_packets] of 16 bytes, packets
        [max_packets][slot_bytes], state [total_channels] of 16 bytes."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.airband_hip_device_rtp_stream(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["n_packets", "records", "packets", "state"], ptrs)}

    def set_band_scope(self, mask=None, windows: int = 8, mean: bool = True, peak: bool = False):
        """Band scope (airband_hip_set_band_scope): per batch and selected dongle, the power spectrum of the whole band over `windows` of the batch's FFT windows.
        mask: one byte per dongle (None = every dongle).  Before the first batch."""
        m = None
        if mask is not None:
            m = np.ascontiguousarray(mask, np.uint8)
            if m.shape != (self.geometry.device_count,):
                raise ValueError("mask needs one byte per dongle (%d), got shape %r" % (self.geometry.device_count, m.shape))
        traces = (capi.SCOPE_MEAN if mean else 0) | (capi.SCOPE_PEAK if peak else 0)
        self._check(self.L.airband_hip_set_band_scope(self.h, m.ctypes.data if m is not None else None, int(windows), traces))
        self.scope_traces = traces
        self.scope_rows = int(np.count_nonzero(m)) if m is not None else self.geometry.device_count
        self.survey_peaks = 0  # a new scope drops the survey
        self.watch_tracks = self.watch_events = 0  # and the watch

    def collect_band_scope(self, first_dev: int = 0, n_dev: Optional[int] = None) -> dict:
        """The scope of the batch collect() would return, for dongles [first_dev, first_dev + n_dev): dict(mean=[n_dev][fft_size], peak=...) with the traces
        the scope keeps; zeros for dongles the mask did not select.  Repeatable: does not mark the batch as collected."""
        n = self.geometry.device_count - first_dev if n_dev is None else int(n_dev)
        traces = getattr(self, "scope_traces", capi.SCOPE_MEAN | capi.SCOPE_PEAK)
        out = {}
        if traces & capi.SCOPE_MEAN:
            out["mean"] = np.empty((n, self.geometry.fft_size), np.float32)
        if traces & capi.SCOPE_PEAK:
            out["peak"] = np.empty((n, self.geometry.fft_size), np.float32)
        self._check(self.L.airband_hip_collect_band_scope(self.h, int(first_dev), n, out["mean"].ctypes.data if "mean" in out else None,
                                                          out["peak"].ctypes.data if "peak" in out else None))
        return out

    def device_band_scope(self) -> dict:
        """Device pointers of the current scope (valid until the next process call): mean, peak [rows][fft_size] float32 (0 for a trace the scope does not keep),
        row_of_dev [device_count] int32."""
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self.L.airband_hip_device_band_scope(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["mean", "peak", "row_of_dev"], ptrs)}

    def set_band_survey(self, trace: str = "mean", max_peaks: int = 8, floor_permille: int = 500, threshold_db: float = 10.0, guard_bins: int = 8):
        """Band survey (airband_hip_set_band_survey): per batch and scope row of `trace` ("mean" or "peak"), the noise floor (the value of rank floor_permille / 1000),
        the strongest bin and the peaks more than threshold_db above the floor that lie further than guard_bins from every configured channel (guard_bins = -1:
        every peak).  After set_band_scope(), before the first batch."""
        bit = {"mean": capi.SCOPE_MEAN, "peak": capi.SCOPE_PEAK}[trace]
        ratio = np.float32(10.0 ** (float(threshold_db) / 10.0))
        self._check(self.L.airband_hip_set_band_survey(self.h, bit, int(max_peaks), int(floor_permille), float(ratio), int(guard_bins)))
        self.survey_peaks = int(max_peaks)
        self.watch_tracks = self.watch_events = 0  # a new survey drops the watch

    def collect_band_survey(self, first_dev: int = 0, n_dev: Optional[int] = None) -> dict:
        """The survey of the batch collect() would return, for dongles [first_dev, first_dev + n_dev): dict(summary=[n_dev] of capi.SUMMARY_DTYPE,
        peaks=[n_dev][max_peaks] of capi.PEAK_DTYPE); a zero summary and {-1, 0} peaks for dongles the scope's mask did not select.  Repeatable."""
        n = self.geometry.device_count - first_dev if n_dev is None else int(n_dev)
        summary = np.empty((n,), capi.SUMMARY_DTYPE)
        peaks = np.empty((n, max(getattr(self, "survey_peaks", 0), 1)), capi.PEAK_DTYPE)
        self._check(self.L.airband_hip_collect_band_survey(self.h, int(first_dev), n, summary.ctypes.data, peaks.ctypes.data))
        return dict(summary=summary, peaks=peaks)

    def device_band_survey(self) -> dict:
        """Device pointers of the current survey (valid until the next process call), indexed by scope row: summary [rows] of 32 bytes, peaks [rows][max_peaks]
        of 8 bytes."""
        ptrs = [C.c_void_p() for _ in range(2)]
        self._check(self.L.airband_hip_device_band_survey(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["summary", "peaks"], ptrs)}

    def set_band_watch(self, max_tracks: int = 8, match_bins: int = 2, confirm_hits: int = 2, release_misses: int = 4, max_events: Optional[int] = None):
        """Band watch (airband_hip_set_band_watch): per scope row a table of max_tracks carrier tracks advanced by each batch's survey -- a peak within match_bins
        of a track continues it, confirm_hits consecutive sightings confirm it (an APPEAR event), release_misses batches without it release it (a VANISH event) --
        and one list of the fleet's events per batch, max_events records (None: 4 x rows, clipped to the range).  After set_band_survey(), before the first batch."""
        if max_events is None:
            rows = getattr(self, "scope_rows", 0)
            max_events = max(1, min(4 * rows, rows * (int(max_tracks) + getattr(self, "survey_peaks", 0))))
        self._check(self.L.airband_hip_set_band_watch(self.h, int(max_tracks), int(match_bins), int(confirm_hits), int(release_misses), int(max_events)))
        self.watch_tracks, self.watch_events = int(max_tracks), int(max_events)

    def collect_band_events(self) -> dict:
        """The fleet's events of the batch collect() would return: dict(n_events = the total, events = the first min(n_events, max_events) of capi.EVENT_DTYPE, in
        ascending dongle order).  Two small copies.  Repeatable."""
        n = C.c_int64(0)
        events = np.zeros((max(getattr(self, "watch_events", 0), 1),), capi.EVENT_DTYPE)
        self._check(self.L.airband_hip_collect_band_events(self.h, C.byref(n), events.ctypes.data))
        return dict(n_events=int(n.value), events=events[:min(int(n.value), len(events))])

    def collect_band_tracks(self, first_dev: int = 0, n_dev: Optional[int] = None) -> dict:
        """The track tables of the same batch for dongles [first_dev, first_dev + n_dev): dict(rows=[n_dev] of capi.WATCH_ROW_DTYPE, tracks=[n_dev][max_tracks] of
        capi.TRACK_DTYPE); zero rows and free slots for dongles the scope's mask did not select.  Repeatable."""
        n = self.geometry.device_count - first_dev if n_dev is None else int(n_dev)
        rows = np.empty((n,), capi.WATCH_ROW_DTYPE)
        tracks = np.empty((n, max(getattr(self, "watch_tracks", 0), 1)), capi.TRACK_DTYPE)
        self._check(self.L.airband_hip_collect_band_tracks(self.h, int(first_dev), n, rows.ctypes.data, tracks.ctypes.data))
        return dict(rows=rows, tracks=tracks)

    def device_band_watch(self) -> dict:
        """Device pointers of the current watch (valid until the next process call): n_events [1] int32, events [max_events] of 16 bytes; rows [rows] of 16 bytes
        and tracks [rows][max_tracks] of 24 bytes, indexed by scope row."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.airband_hip_device_band_watch(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["n_events", "events", "rows", "tracks"], ptrs)}

    def set_band_follow(self, max_changes: Optional[int] = None):
        """Band follow (airband_hip_set_band_follow): per batch and scope row the GPU tunes the row's followers (the constructor's follow=) onto the watch's
        confirmed tracks -- TUNE when an idle follower takes a track, MOVE when the track's bin drifts, HOME when the track ends -- and keeps one list of the
        fleet's changes per batch, max_changes records (None: 4 x rows, clipped to the range).  A change applies to stage 1 of the next batch; squelch, AGC and
        filter state carry on as across an AFC step.  After set_band_watch(), before the first batch."""
        if max_changes is None:
            rows = getattr(self, "scope_rows", 0)
            max_changes = max(1, min(4 * rows, len(self.follow_channels) + rows * getattr(self, "watch_tracks", 0)))
        self._check(self.L.airband_hip_set_band_follow(self.h, int(max_changes)))
        self.follow_changes = int(max_changes)

    def collect_band_follow_changes(self) -> dict:
        """The fleet's changes of the batch collect() would return: dict(n_changes = the total, changes = the first min(n_changes, max_changes) of
        capi.FOLLOW_CHANGE_DTYPE, in ascending dongle order).  Two small copies.  Repeatable."""
        n = C.c_int64(0)
        changes = np.zeros((max(getattr(self, "follow_changes", 0), 1),), capi.FOLLOW_CHANGE_DTYPE)
        self._check(self.L.airband_hip_collect_band_follow_changes(self.h, C.byref(n), changes.ctypes.data))
        return dict(n_changes=int(n.value), changes=changes[:min(int(n.value), len(changes))])

    def collect_band_followers(self) -> dict:
        """The followers of the same batch: dict(followers=[n_follow] of capi.FOLLOWER_DTYPE in the constructor's order, rows=[device_count] of
        capi.FOLLOW_ROW_DTYPE, zeros for dongles the scope's mask did not select).  Repeatable."""
        followers = np.empty((max(len(self.follow_channels), 1),), capi.FOLLOWER_DTYPE)
        rows = np.empty((self.geometry.device_count,), capi.FOLLOW_ROW_DTYPE)
        self._check(self.L.airband_hip_collect_band_followers(self.h, followers.ctypes.data, rows.ctypes.data))
        return dict(followers=followers[:len(self.follow_channels)], rows=rows)

    def device_band_follow(self) -> dict:
        """Device pointers of the current follow (valid until the next process call): n_changes [1] int32, changes [max_changes] of 16 bytes, followers
        [n_follow] of 16 bytes in the constructor's order, rows [rows] of 16 bytes indexed by scope row."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.airband_hip_device_band_follow(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["n_changes", "changes", "followers", "rows"], ptrs)}

    def set_freq_index(self, dev: int, freq_idx: int):
        """Entry freq_idx of dongle dev's scan list is in force for every batch enqueued from now on (latched per batch)."""
        self._check(self.L.airband_hip_set_freq_index(self.h, dev, freq_idx))

    def set_scan_control(self, idle_batches: int = 16, dwell_batches: int = 2, max_records: Optional[int] = None):
        """Scan control (airband_hip_set_scan_control): the GPU hops every scan list of the handle -- after idle_batches batches without signal a list moves on
        every dwell_batches batches, the squelch opening after such a spell gives an ACTIVITY record, every hop a HOP record -- and keeps one list of the fleet's
        records per batch, max_records of them (None: one per list).  idle_batches = 0 switches it off; set_freq_index() then continues from the GPU's indices.
        While it is on set_freq_index() is refused."""
        self._check(self.L.airband_hip_set_scan_control(self.h, int(idle_batches), int(dwell_batches), 0 if max_records is None else int(max_records)))

    def scan_hold(self, dev: int, freq_idx: int):
        """Pins dongle dev's list to entry freq_idx from the next batch on (a HOP record if that changes the entry); -1 releases it (airband_hip_scan_hold)."""
        self._check(self.L.airband_hip_scan_hold(self.h, int(dev), int(freq_idx)))

    def collect_scan_events(self) -> dict:
        """The fleet's scan records of the batch collect() would return: dict(n_records = the total, records = the first min(n_records, max_records) of
        capi.SCAN_EVENT_DTYPE, in ascending dongle order).  Two small copies.  Repeatable."""
        n = C.c_int64(0)
        records = np.zeros((max(len(self.scan_devices), 1),), capi.SCAN_EVENT_DTYPE)  # max_records is at most one per list
        self._check(self.L.airband_hip_collect_scan_events(self.h, C.byref(n), records.ctypes.data))
        kept = int(np.count_nonzero(records["kind"][:max(int(n.value), 0)]))  # the library wrote a prefix; a record's kind is never 0
        return dict(n_records=int(n.value), records=records[:kept])

    def collect_scan_state(self, first_dev: int = 0, n_dev: Optional[int] = None) -> np.ndarray:
        """The scan lists' states behind the same batch for dongles [first_dev, first_dev + n_dev): [n_dev] of capi.SCAN_STATE_DTYPE, zeros for a dongle without
        a list.  Repeatable."""
        n = self.geometry.device_count - first_dev if n_dev is None else int(n_dev)
        state = np.zeros((max(n, 1),), capi.SCAN_STATE_DTYPE)
        self._check(self.L.airband_hip_collect_scan_state(self.h, int(first_dev), n, state.ctypes.data))
        return state[:max(n, 0)]

    def device_scan_control(self) -> dict:
        """Device pointers of scan control (valid until the next process call): n_records [1] int32, records [max_records] of 16 bytes, state [lists] of 16
        bytes in ascending dongle order of the dongles that have a list."""
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self.L.airband_hip_device_scan_control(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["n_records", "records", "state"], ptrs)}

    def freq_stats(self, dev: int, freq_idx: int) -> dict:
        """Statistics of entry freq_idx of dongle dev's scan list as of the last completed batch (frozen values for inactive entries)."""
        st = capi.ChannelStats()
        self._check(self.L.airband_hip_freq_stats(self.h, dev, freq_idx, C.byref(st)))
        return {f[0]: getattr(st, f[0]) for f in capi.ChannelStats._fields_}

    def synchronize(self):
        self._check(self.L.airband_hip_synchronize(self.h))

    def stream_wait_results(self, stream_ptr: int):
        """Make a consumer's hipStream_t wait (on the GPU) for the results of the last completed batch."""
        self._check(self.L.airband_hip_stream_wait_results(self.h, C.c_void_p(stream_ptr)))

    def flush(self):
        """Pipelined handles (FLAG_PIPELINE): run stage 2 of the batch the last process call started."""
        self._check(self.L.airband_hip_flush(self.h))

    def process_bins(self, wavein: np.ndarray, iq_in: np.ndarray):
        wavein = np.ascontiguousarray(wavein, np.float32)
        iq_in = np.ascontiguousarray(iq_in, np.float32)
        assert wavein.shape == (self.total_channels, self.B) and iq_in.shape == (self.total_channels, 2 * self.B)
        self._check(self.L.airband_hip_process_bins(self.h, wavein.ctypes.data, iq_in.ctypes.data))

    def read_bins(self, first_channel: int = 0, n_channels: Optional[int] = None):
        n, B = (self.total_channels - first_channel if n_channels is None else int(n_channels)), self.B
        w = np.empty((n, B), np.float32)
        q = np.empty((n, 2 * B), np.float32)
        self._check(self.L.airband_hip_read_bins_channels(self.h, int(first_channel), n, w.ctypes.data, q.ctypes.data))
        return w, q

    def read_trace(self, first_channel: int = 0, n_channels: Optional[int] = None) -> np.ndarray:
        n = self.total_channels - first_channel if n_channels is None else int(n_channels)
        t = np.empty((n, self.B), np.uint8)
        self._check(self.L.airband_hip_read_trace_channels(self.h, int(first_channel), n, t.ctypes.data))
        return t

    def constants(self, channel_index: int):
        v = (C.c_double * 16)()
        self._check(self.L.airband_hip_channel_constants(self.h, channel_index, v))
        return list(v)

    def last_timings(self):
        v = (C.c_float * 4)()
        self._check(self.L.airband_hip_last_timings(self.h, v))
        return dict(channelizer_ms=v[0], demod_ms=v[1], emit_ms=v[2], batch_ms=v[3])

    def timing_totals(self, reset: bool = False):
        """Sums of the per-stage GPU times over the batches finished since the last reset (waits for the enqueued ones)."""
        v = (C.c_double * 4)()
        n = C.c_int64(0)
        self._check(self.L.airband_hip_timing_totals(self.h, v, C.byref(n), 1 if reset else 0))
        return dict(channelizer_ms=v[0], demod_ms=v[1], emit_ms=v[2], batch_ms=v[3], batches=int(n.value))

    def channelizer_name(self) -> str:
        return self.L.airband_hip_channelizer_name(self.h).decode()

    def table_info(self) -> dict:
        """n_bsets, n_shared_bsets, n_host_bsets, pieces_per_table, bytes_per_table, edge_hi_zero, n_items, channelizer of a matrix-core handle's coefficient
        tables (airband_hip_read_tables with an empty range).  AirbandError(EINVAL) on the wavefront FFT."""
        info = capi.TableInfo()
        self._check(self.L.airband_hip_read_tables(self.h, 0, 0, C.byref(info), None, None, None, None))
        out = {f[0]: getattr(info, f[0]) for f in capi.TableInfo._fields_}
        out["channelizer"] = out["channelizer"].decode()
        out["edge_hi_zero"] = bool(out["edge_hi_zero"])
        return out

    def read_tables(self, first: int = 0, n: Optional[int] = None) -> dict:
        """Coefficient tables [first, first + n) as they stand on the device (airband_hip_read_tables; waits for the handle): info (table_info()), tables
        [n][bytes_per_table] int8 -- or [n][bytes_per_table / 4] float32 on a CF32 handle --, corr [n][pieces_per_table][16] float64 (zeros on CF32), bset_bin [n][8],
        and per work item item_bset (the table it reads now), item_home, item_private."""
        info = self.table_info()
        n = info["n_bsets"] - int(first) if n is None else int(n)
        f32 = info["channelizer"] == "dft_mfma_f32"
        rows = max(n, 0)
        tab = np.zeros((rows, info["bytes_per_table"] // 4), np.float32) if f32 else np.zeros((rows, info["bytes_per_table"]), np.int8)
        corr = np.zeros((rows, info["pieces_per_table"], 16), np.float64)
        bins = np.zeros((rows, 8), np.int32)
        items = np.zeros((3, info["n_items"]), np.int32)
        raw = capi.TableInfo()
        self._check(self.L.airband_hip_read_tables(self.h, int(first), n, C.byref(raw), tab.ctypes.data, corr.ctypes.data, bins.ctypes.data, items.ctypes.data))
        return dict(info=info, tables=tab, corr=corr, bset_bin=bins, item_bset=items[0], item_home=items[1], item_private=items[2])

    def channelizer_reason(self) -> str:
        """Why the handle has the channelizer it has; "" on a matrix-core kernel by the ordinary rule."""
        return (self.L.airband_hip_channelizer_reason(self.h) or b"").decode()

    def schedule_info(self) -> dict:
        """run_ahead (NULL-stream process_device batches put stage 1 on its own stream), ring_batches (depth of the stage-1 rings), channelizer_waves_per_cu (5 where
        the channelizer is held, 0 where not), batches_run_ahead (how many batches took that path so far): airband_hip_schedule_info."""
        a, b, c, n = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._check(self.L.airband_hip_schedule_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(run_ahead=bool(a.value), ring_batches=int(b.value), channelizer_waves_per_cu=int(c.value), batches_run_ahead=int(n.value))

    def build_info(self) -> str:
        return self.L.airband_hip_build_info().decode()

    # ---- mixers ---------------------------------------------------------------------------------------
    def set_mixers(self, n_mixers: int, inputs: Sequence[tuple]):
        """inputs: (device, channel, mixer, ampfactor, balance) tuples in connection order."""
        arr = (capi.MixerInput * len(inputs))(*[capi.MixerInput(int(a), int(b), int(c), float(d), float(e)) for a, b, c, d, e in inputs])
        self._check(self.L.airband_hip_set_mixers(self.h, n_mixers, arr, len(inputs)))
        self.n_mixers = n_mixers
        self.mixer_gate = None  # new wiring drops the mixer gate

    def mixer_enable_input(self, input_index: int, enabled: bool):
        self._check(self.L.airband_hip_mixer_enable_input(self.h, input_index, 1 if enabled else 0))

    def mixer_set_stereo(self, mixer: int, stereo: bool):
        self._check(self.L.airband_hip_mixer_set_stereo(self.h, int(mixer), 1 if stereo else 0))

    # ---- gated mixer collect (include/airband_hip.h) ----------------------------------------------------------------------------------
    def set_mixer_gate(self, gate, max_rows: Optional[int] = None, encoding=None, stereo: bool = False, manual_step: bool = False):
        """gate: one capi.GATE_* byte per mixer, None removes the gate; max_rows: capacity of the packed buffers, default every mixer; encoding: None (float32),
        "s16", "ulaw", "alaw"; stereo: rows are frames of (left, right); manual_step: the host enqueues the step with mixer_gate_step(), after its exchange.
        Any time after set_mixers() (airband_hip_set_mixer_gate)."""
        if gate is None:
            self._check(self.L.airband_hip_set_mixer_gate(self.h, None, 0, 0, 0))
            self.mixer_gate = None
            return
        gate = np.ascontiguousarray(gate, np.uint8)
        if gate.shape != (self.n_mixers,):
            raise ValueError("gate needs one byte per mixer (%d), got shape %r" % (self.n_mixers, gate.shape))
        rows = self.n_mixers if max_rows is None else int(max_rows)
        enc = capi.AUDIO_F32 if encoding is None else capi.audio_encoding_value(encoding)
        flags = (capi.MIXER_GATE_STEREO if stereo else 0) | (capi.MIXER_GATE_MANUAL_STEP if manual_step else 0)
        self._check(self.L.airband_hip_set_mixer_gate(self.h, gate.ctypes.data, rows, enc, flags))
        self.mixer_gate = dict(rows=rows, encoding=enc, width=2 if stereo else 1, gate=gate.copy())

    def mixer_gate_step(self, stream: int = 0):
        """One step of a manual mixer gate, behind whatever wrote the sums last (airband_hip_mixer_gate_step); stream 0 = the handle's own."""
        self._check(self.L.airband_hip_mixer_gate_step(self.h, C.c_void_p(stream) if stream else None))

    def collect_active_mixers(self) -> dict:
        """The last step's result (airband_hip_collect_active_mixers): n_active (may exceed the capacity), mixers [n] ascending, has_signal of every mixer, and
        rows [n][W B] float32 on a float gate, or audio [n][W B] int16 / uint8 and info [n] of capi.AUDIO_ROW_DTYPE on an encoded one."""
        g = getattr(self, "mixer_gate", None) or dict(rows=1, encoding=capi.AUDIO_F32, width=1)
        cap, enc, wb = g["rows"], g["encoding"], g["width"] * self.B
        n = C.c_int64(0)
        idx = np.empty((cap,), np.int32)
        sig = np.empty((self.n_mixers,), np.uint8)
        rows = audio = info = None
        if enc == capi.AUDIO_F32:
            rows = np.empty((cap, wb), np.float32)
        else:
            audio = np.empty((cap, wb), self._audio_dtype(enc))
            info = np.empty((cap,), capi.AUDIO_ROW_DTYPE)
        self._check(self.L.airband_hip_collect_active_mixers(self.h, C.byref(n), idx.ctypes.data, rows.ctypes.data if rows is not None else None,
                                                             audio.ctypes.data if audio is not None else None, info.ctypes.data if info is not None else None, sig.ctypes.data))
        kept = min(int(n.value), cap)
        out = dict(n_active=int(n.value), mixers=idx[:kept], has_signal=sig)
        if rows is not None:
            out["rows"] = rows[:kept]
        else:
            out["audio"], out["info"] = audio[:kept], info[:kept]
        return out

    def device_active_mixers(self) -> dict:
        """Device pointers of the packed mixer rows (valid until the next step): index [max_rows] int32, count [1] int32, rows [max_rows][W B] float32 (0 on an
        encoded gate), audio and info (0 on a float gate)."""
        ptrs = [C.c_void_p() for _ in range(5)]
        self._check(self.L.airband_hip_device_active_mixers(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["index", "count", "rows", "audio", "info"], ptrs)}

    # ---- mixer transmission spool (include/airband_hip.h) -----------------------------------------------------------------------------
    def set_mixer_spool(self, pool_rows, export_rows=None, max_records=None, mask=None, min_batches=8, idle_batches=4, max_batches=480):
        """Mixer spool (airband_hip_set_mixer_spool): the GPU keeps the encoded rows of every open mixer transmission and hands over finished ones.
        export_rows: default max(pool_rows, max_batches + 1); max_records: default the mixer count; mask: one byte per mixer (None = every SIGNAL mixer).
        Any time after set_mixer_gate() with an encoding; pool_rows 0 removes it; set_mixer_gate() or set_mixers() again drops it."""
        pool_rows = int(pool_rows)
        export_rows = max(pool_rows, max_batches + 1) if export_rows is None else int(export_rows)
        max_records = self.n_mixers if max_records is None else int(max_records)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (self.n_mixers,):
            raise ValueError("mask must have one byte per mixer")
        self._check(self.L.airband_hip_set_mixer_spool(self.h, None if m is None else m.ctypes.data, pool_rows, export_rows, max_records, min_batches, idle_batches, max_batches))
        if getattr(self, "mixer_gate", None) is not None:
            self.mixer_gate["spool"] = (export_rows, max_records) if pool_rows else (0, 0)

    def collect_mixer_transmissions(self) -> dict:
        """The finished mixer transmissions that fit the export buffer (airband_hip_collect_mixer_transmissions): records [n] of capi.TRANSMISSION_DTYPE
        (channel = the mixer, reserved[1] = its stereo flag over the stored rows), audio [sum of n_rows][W B] int16 ("s16") or uint8 (G.711) -- transmission
        i's rows are audio[row_offset : row_offset + n_rows] -- and n_waiting."""
        g = getattr(self, "mixer_gate", None) or {}
        export_rows, max_records = g.get("spool", (0, 0))
        records = np.empty((max(max_records, 1),), capi.TRANSMISSION_DTYPE)
        audio = np.empty((max(export_rows, 1), g.get("width", 1) * self.B), self._audio_dtype(g.get("encoding", capi.AUDIO_F32)))
        n, n_rows, n_waiting = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self.L.airband_hip_collect_mixer_transmissions(self.h, C.byref(n), records.ctypes.data, audio.ctypes.data, C.byref(n_rows), C.byref(n_waiting)))
        return dict(records=records[:n.value], audio=audio[:n_rows.value], n_waiting=int(n_waiting.value))

    def mixer_spool_flush(self):
        """Every open mixer transmission finishes with reason capi.SPOOL_FLUSH (airband_hip_mixer_spool_flush)."""
        self._check(self.L.airband_hip_mixer_spool_flush(self.h))

    def mixer_spool_counters(self) -> dict:
        """airband_hip_mixer_spool_counters_get as a dict (capi.SPOOL_COUNTER_NAMES)."""
        out = capi.SpoolCounters()
        self._check(self.L.airband_hip_mixer_spool_counters_get(self.h, C.byref(out)))
        return {k: int(getattr(out, k)) for k in capi.SPOOL_COUNTER_NAMES}

    def device_mixer_spool(self) -> dict:
        """Device pointers of the last collect_mixer_transmissions() (valid until the next one): audio [export_rows][row bytes], records [max_records] of 48
        bytes, n_export [3] int32 (transmissions, rows, still waiting)."""
        ptrs = [C.c_void_p() for _ in range(3)]
        self._check(self.L.airband_hip_device_mixer_spool(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["audio", "records", "n_export"], ptrs)}

    # ---- mixer RTP stream (include/airband_hip.h) -------------------------------------------------------------------------------------
    def set_mixer_rtp_stream(self, frame_samples=None, sources=None, max_packets=None, *, remove: bool = False):
        """Mixer RTP stream (airband_hip_set_mixer_rtp_stream): the GPU frames the mixer gate's encoded rows as RTP packets of frame_samples FRAMES (W samples
        each on a stereo gate), carrying the remainder per mixer.  frame_samples: default wave_rate // 50 (20 ms); sources: [n_mixers] of capi.RTP_SOURCE_DTYPE,
        default every mixer whose gate is not NEVER with ssrc = its index, ts0 = 0, seq0 = 0 and payload type 0 / 8 / 96 for ulaw / alaw / s16; max_packets:
        default what a step can emit at most.  Any time after set_mixer_gate() with an encoding; remove=True removes it; set_mixer_gate() or set_mixers() again
        drops it."""
        g = getattr(self, "mixer_gate", None)
        if remove:
            self._check(self.L.airband_hip_set_mixer_rtp_stream(self.h, None, 0, 0))
            if g is not None:
                g.pop("rtp", None)
            return
        enc, width = (g["encoding"], g["width"]) if g else (capi.AUDIO_F32, 1)
        F = int(self.geometry.wave_rate) // 50 if frame_samples is None else int(frame_samples)
        if sources is None:
            src = np.zeros(self.n_mixers, capi.RTP_SOURCE_DTYPE)
            src["ssrc"] = np.arange(self.n_mixers)
            src["payload_type"] = capi.RTP_PAYLOAD_TYPES.get(enc, 0)
            src["stream"] = (g["gate"] if g else np.zeros(self.n_mixers, np.uint8)) != capi.GATE_NEVER
        else:
            src = np.ascontiguousarray(sources, capi.RTP_SOURCE_DTYPE)
            if src.shape != (self.n_mixers,):
                raise ValueError("sources needs one record per mixer (%d), got shape %r" % (self.n_mixers, src.shape))
        if max_packets is None:
            max_packets = max(1, int(np.count_nonzero(src["stream"])) * ((max(F, 4) - 4 + self.B) // max(F, 1)))
        self._check(self.L.airband_hip_set_mixer_rtp_stream(self.h, src.ctypes.data, F, int(max_packets)))
        g["rtp"] = dict(frame_samples=F, max_packets=int(max_packets), slot_bytes=self._check(self.L.airband_hip_mixer_rtp_slot_bytes(enc, F, width)), sources=src)

    def _mixer_rtp(self):
        return (getattr(self, "mixer_gate", None) or {}).get("rtp") or dict(frame_samples=0, max_packets=1, slot_bytes=16, sources=None)

    def collect_mixer_rtp_packets(self) -> dict:
        """The last step's (or flush's) RTP packets (airband_hip_collect_mixer_rtp_packets): n_packets (may exceed max_packets: only the first max_packets were
        written then), records [n] of capi.RTP_PACKET_DTYPE (channel = the mixer), packets [n][slot_bytes] uint8 -- packet i is
        packets[i, :records[i]["length"]] -- and has_signal of every mixer."""
        r = self._mixer_rtp()
        n = C.c_int64(0)
        records = np.empty((r["max_packets"],), capi.RTP_PACKET_DTYPE)
        packets = np.empty((r["max_packets"], r["slot_bytes"]), np.uint8)
        sig = np.empty((getattr(self, "n_mixers", 0),), np.uint8)
        self._check(self.L.airband_hip_collect_mixer_rtp_packets(self.h, C.byref(n), records.ctypes.data, packets.ctypes.data, sig.ctypes.data))
        kept = min(int(n.value), r["max_packets"])
        return dict(n_packets=int(n.value), records=records[:kept], packets=packets[:kept], has_signal=sig)

    def collect_mixer_rtp_state(self, first_mixer: int = 0, n_mixers: Optional[int] = None):
        """The mixers' sender state (airband_hip_collect_mixer_rtp_state): [n_mixers] of capi.RTP_STATE_DTYPE, default every mixer; carry counts frames."""
        n = getattr(self, "n_mixers", 0) - int(first_mixer) if n_mixers is None else int(n_mixers)
        st = np.empty((max(n, 0),), capi.RTP_STATE_DTYPE)
        self._check(self.L.airband_hip_collect_mixer_rtp_state(self.h, int(first_mixer), n, st.ctypes.data))
        return st

    def mixer_rtp_counters(self) -> dict:
        """airband_hip_mixer_rtp_counters_get as a dict (capi.RTP_COUNTER_NAMES)."""
        out = capi.RtpCounters()
        self._check(self.L.airband_hip_mixer_rtp_counters_get(self.h, C.byref(out)))
        return {k: int(getattr(out, k)) for k in capi.RTP_COUNTER_NAMES}

    def mixer_rtp_flush(self):
        """Every carrying mixer emits its short FLUSH packet (airband_hip_mixer_rtp_flush); collect the last step's packets first: the flush's replace them."""
        self._check(self.L.airband_hip_mixer_rtp_flush(self.h))

    def device_mixer_rtp_stream(self) -> dict:
        """Device pointers of the last step's packets (valid until the next step or flush): n_packets [1] int32, records [max_packets] of 16 bytes, packets
        [max_packets][slot_bytes], state [n_mixers] of 16 bytes."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.airband_hip_device_mixer_rtp_stream(self.h, *[C.byref(p) for p in ptrs]))
        return {k: (p.value or 0) for k, p in zip(["n_packets", "records", "packets", "state"], ptrs)}

    def encode_mixer_audio(self, left, right, encoding):
        """The mixer pack kernel on host rows left, right [n][B] float32, right None for mono (airband_hip_encode_mixer_audio): (audio [n][W B] int16 or uint8,
        info [n] of capi.AUDIO_ROW_DTYPE, channel = row)."""
        enc = capi.audio_encoding_value(encoding)
        left = np.ascontiguousarray(left, np.float32)
        if left.ndim != 2 or left.shape[1] != self.B:
            raise ValueError("left must be [n][%d], got shape %r" % (self.B, left.shape))
        if right is not None:
            right = np.ascontiguousarray(right, np.float32)
            if right.shape != left.shape:
                raise ValueError("right must have left's shape %r, got %r" % (left.shape, right.shape))
        n = left.shape[0]
        audio = np.empty((n, (2 if right is not None else 1) * self.B), self._audio_dtype(enc))
        info = np.empty((n,), capi.AUDIO_ROW_DTYPE)
        self._check(self.L.airband_hip_encode_mixer_audio(self.h, enc, left.ctypes.data, right.ctypes.data if right is not None else None, n, audio.ctypes.data, info.ctypes.data))
        return audio, info

    # ---- the mixer exchange over RCCL (include/airband_hip.h): one handle per GPU, in one process or in one process each -----------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = load_library().airband_hip_comm_unique_id(buf)
        if rc < 0:
            raise AirbandError(rc, (load_library().airband_hip_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init_rank(self, unique_id: bytes, nranks: int, rank: int):
        assert len(unique_id) == 128
        self._check(self.L.airband_hip_comm_init_rank(self.h, (C.c_uint8 * 128).from_buffer_copy(unique_id), int(nranks), int(rank)))

    def allreduce_mixers(self, stream: int = 0):
        self._check(self.L.airband_hip_allreduce_mixers(self.h, C.c_void_p(stream)))

    def add_mixers(self, src: "AirbandHip"):
        self._check(self.L.airband_hip_add_mixers(self.h, src.h))

    def clear_mixers(self):
        """A handle that ran no batch this round adds nothing to the exchange (mixer_disable_input(), src/mixer.cpp:96-112)."""
        self._check(self.L.airband_hip_clear_mixers(self.h))

    @staticmethod
    def comm_init_all(handles: Sequence["AirbandHip"]):
        """One process, one handle per GPU (the reference-side shim's form): ncclCommInitAll over the handles' GPUs."""
        L = load_library()
        arr = (C.c_void_p * len(handles))(*[h.h for h in handles])
        rc = L.airband_hip_comm_init_all(arr, len(handles))
        if rc < 0:
            raise AirbandError(rc, (L.airband_hip_last_error(handles[0].h) or L.airband_hip_last_error(None) or b"").decode())

    @staticmethod
    def allreduce_mixers_group(handles: Sequence["AirbandHip"]):
        """The per-batch exchange of one thread that owns several handles: every handle's all-reduce inside one RCCL group."""
        L = load_library()
        rc = L.airband_hip_comm_group_begin()
        if rc < 0:
            raise AirbandError(rc, (L.airband_hip_last_error(None) or b"").decode())
        try:
            for h in handles:
                h.allreduce_mixers()
        finally:  # a failing rank must not leave the thread's RCCL group open: every later collective of the process would queue behind it
            rc = L.airband_hip_comm_group_end()
        if rc < 0:
            raise AirbandError(rc, (L.airband_hip_last_error(None) or b"").decode())

    def batch_ready(self) -> bool:
        rc = self.L.airband_hip_batch_ready(self.h)
        if rc == capi.EAGAIN:
            return False
        self._check(rc)
        return True

    def device_enable(self, dev: int, enabled: bool):
        """Switch a dongle off / on: the reference's handling of a failed input (src/rtl_airband.cpp:383-391)."""
        self._check(self.L.airband_hip_device_enable(self.h, dev, 1 if enabled else 0))

    def collect_mixers(self):
        left = np.empty((self.n_mixers, self.B), np.float32)
        right = np.empty((self.n_mixers, self.B), np.float32)
        sig = np.empty((self.n_mixers,), np.uint8)
        self._check(self.L.airband_hip_collect_mixers(self.h, left.ctypes.data, right.ctypes.data, sig.ctypes.data))
        return left, right, sig

    def device_results(self) -> dict:
        ptrs = [C.c_void_p() for _ in range(6)]
        self._check(self.L.airband_hip_device_results(self.h, *[C.byref(p) for p in ptrs]))
        names = ["waveout", "iq_out", "axc", "mix_left", "mix_right", "mix_signal"]
        return {k: (p.value or 0) for k, p in zip(names, ptrs)}

    # ---- synthetic dongles -----------------------------------------------------------------------------
    def set_signal_plan(self, carriers, noise_q8: Optional[int] = None):
        tab = siggen.carrier_table(carriers)
        sin = siggen.sin_table()
        if noise_q8 is None:
            noise_q8 = siggen.noise_mul_q8()
        self._check(self.L.airband_hip_set_signal_plan(self.h, tab.ctypes.data, len(carriers), int(noise_q8), sin.ctypes.data))

    def stage2_regrouped(self) -> bool:
        return bool(self.L.airband_hip_regrouped(self.h))

    def set_signal_plan_shift(self, n_plans: int, shift_hz: float, sample_rate: int):
        """Dongle d's carrier c is generated ((d mod n_plans) >> 2c & 3) * shift_hz above the plan's frequency (siggen.plan_shift_bins / generate_u8's twin)."""
        self._check(self.L.airband_hip_set_signal_plan_shift(self.h, int(n_plans), siggen._turns(shift_hz, sample_rate)))

    def generate_iq(self, d_iq_ptr: int, stride_bytes: int, start_byte: int, nbytes: int, *, seed: int = 0x5EED, device_index_offset: int = 0, stream: int = 0):
        self._check(self.L.airband_hip_generate_iq(self.h, C.c_void_p(d_iq_ptr), stride_bytes, start_byte, nbytes, seed, device_index_offset, C.c_void_p(stream)))
