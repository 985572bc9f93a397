"""The band scope's kernel (csrc/band_scope.hip) with its wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles, barriers and a wavefront's LDS exchanges are rendezvous points), launched by the file's own
launch_band_scope(), compared with a float64 evaluation of the defining sum -- the reference's sample-to-float conversion and window
(src/rtl_airband.cpp:316-351,402-455), numpy.fft.fft, re^2 + im^2, mean and maximum over the selected windows.  It checks the LOGIC of the code the GPU
runs (which windows, the passes over the bins, index maps, twiddles, the reduction over the wavefronts, the row layout); tests/test_gpu_band_scope.py is
what a GPU says."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hostbed

pkg = importlib.import_module("rtlsdr-airband_amd")
capi = pkg.capi
sg = pkg.siggen

# powers against float64, relative to the RMS of the row's bins: twice the bar tests/test_host_fft.py holds the wavefront FFT's bins (amplitudes) to
# against float64 -- "assert worst < 2e-6, worst" -- since d(p) / p = 2 d(a) / a
POWER_TOL = 2 * 2e-6


@pytest.fixture(scope="module")
def hostscope(tmp_path_factory):
    lib = C.CDLL(hostbed.build(["host_scope_harness.cpp", hostbed.PARAMS], tmp_path_factory.mktemp("hostscope") / "libhostscope.so", shared=True))
    vp = C.c_void_p
    lib.hostscope_run.argtypes = [C.POINTER(capi.Config), vp, C.c_long, C.c_int, C.c_int, vp, vp, vp, vp]
    lib.hostscope_geometry.argtypes = [C.POINTER(capi.Config), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.hostscope_region_bytes.restype = C.c_long
    return lib


def _samples(rng, sfmt, n):
    """n complex samples in the format's dtype + their float64 values as the reference converts them (src/rtl_airband.cpp:316-324,402-455)."""
    if sfmt == capi.SFMT_U8:
        raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        val = (raw.astype(np.float64) - 127.5) / 127.5
    elif sfmt == capi.SFMT_S8:
        raw = rng.integers(-128, 128, 2 * n).astype(np.int8)
        val = raw.astype(np.float64) / 128.0
    elif sfmt == capi.SFMT_S16:
        raw = rng.integers(-30000, 30001, 2 * n).astype(np.int16)
        val = raw.astype(np.float64) / 32768.0
    else:
        raw = (rng.standard_normal(2 * n) * 0.3).astype(np.float32)
        val = raw.astype(np.float64)
    return raw, val[0::2] + 1j * val[1::2]


FORMATS = [capi.SFMT_U8, capi.SFMT_S8, capi.SFMT_S16, capi.SFMT_F32]
# fft_log, sample rate, wave rate, windows per batch, lead-in hops in front (the first batch's AGC_EXTRA, or none)
SHAPES = [
    (8, 2_560_000, 16000, 7, 100),   # fft 256: one pass, four values per lane; 7 windows: waves 0 .. 2 take two, wave 3 one
    (9, 2_400_000, 8000, 3, 0),      # fft 512 at hops of 300 samples: windows that start off 16 bytes; fewer windows than wavefronts
    (10, 2_560_000, 16000, 8, 0),    # fft 1024: the largest single pass
    (13, 2_560_000, 8000, 5, 100),   # fft 8192: eight passes of sixteen values; CF32: 64 KiB a window, two wavefronts
]


@pytest.mark.parametrize("sfmt", FORMATS)
@pytest.mark.parametrize("fft_log,sample_rate,wave_rate,K,lead", SHAPES)
def test_scope_kernel_source_on_the_host(hostscope, sfmt, fft_log, sample_rate, wave_rate, K, lead):
    rng = np.random.default_rng(100 * fft_log + sfmt)
    N = 1 << fft_log
    n_dev = 3
    chans, _ = sg.baseline_plan(mixed=False)
    fullscale = 32768.0 if sfmt == capi.SFMT_S16 else 0.0
    devices = [dict(channels=[dict(c) for c in chans], sample_rate=sample_rate, sfmt=sfmt, fullscale=fullscale) for _ in range(n_dev)]
    cfg, keep = pkg.make_config(devices, wave_rate=wave_rate, fft_log=fft_log)
    hop, B = C.c_int(0), C.c_int(0)
    assert hostscope.hostscope_geometry(C.byref(cfg), C.byref(hop), C.byref(B)) == 0
    hop, B = hop.value, B.value
    assert hop == round(sample_rate / wave_rate)
    rows_sel = capi.scope_window_hops(K, B)
    n_samp = (lead + B - 1) * hop + N
    # only the selected windows carry samples: everything between them is a poison pattern the kernel must not depend on (it stages the windows alone)
    bpc2 = 2 * capi.BYTES_PER_SAMPLE[sfmt]
    stride = (n_samp * bpc2 + 15) // 16 * 16 + 16
    buf = np.full(n_dev * stride + 64, 0xEE, np.uint8)
    base = (-buf.ctypes.data) % 16
    vals = {}
    for d in range(n_dev):
        for j, t in enumerate(rows_sel):
            raw, v = _samples(rng, sfmt, N)
            off = base + d * stride + (lead + t) * hop * bpc2
            if j > 0 and (lead + rows_sel[j - 1]) * hop + N > (lead + t) * hop:  # windows that overlap (K = WAVE_BATCH-like spacing): keep what is there
                have = (lead + rows_sel[j - 1]) * hop + N - (lead + t) * hop
                raw = raw.copy()
                raw.view(np.uint8)[:have * bpc2] = buf[off: off + have * bpc2]
                fl = raw.astype(np.float64)
                fl = (fl - 127.5) / 127.5 if sfmt == capi.SFMT_U8 else fl / 128.0 if sfmt == capi.SFMT_S8 else fl / 32768.0 if sfmt == capi.SFMT_S16 else fl
                v = fl[0::2] + 1j * fl[1::2]
            buf[off: off + N * bpc2] = raw.view(np.uint8)
            vals[d, j] = v
    mask = np.array([1, 0, 1], np.uint8)
    mean = np.full((2, N), np.nan, np.float32)
    peak = np.full((2, N), np.nan, np.float32)
    win = np.zeros(N, np.float32)
    rc = hostscope.hostscope_run(C.byref(cfg), buf.ctypes.data + base, stride, lead, K, mask.ctypes.data, mean.ctypes.data, peak.ctypes.data, win.ctypes.data)
    assert rc == 2, rc
    assert hostscope.hostscope_waves(fft_log, capi.BYTES_PER_SAMPLE[sfmt]) == (2 if (sfmt == capi.SFMT_F32 and fft_log == 13) else 4)
    assert 4 * hostscope.hostscope_region_bytes(13, 2) <= 160 * 1024 < 4 * hostscope.hostscope_region_bytes(13, 4)
    for row, d in enumerate((0, 2)):
        pw = np.stack([np.abs(np.fft.fft(vals[d, j] * win.astype(np.float64))) ** 2 for j in range(K)])
        want_mean, want_peak = pw.mean(axis=0), pw.max(axis=0)
        rms = np.sqrt(np.mean(want_mean ** 2))
        err_m = np.sqrt(np.mean((mean[row] - want_mean) ** 2)) / rms
        err_p = np.sqrt(np.mean((peak[row] - want_peak) ** 2)) / np.sqrt(np.mean(want_peak ** 2))
        print("sfmt %d fft %d dongle %d: mean %.3g peak %.3g" % (sfmt, N, d, err_m, err_p))
        assert err_m < POWER_TOL and err_p < POWER_TOL, (err_m, err_p)
        # and bin by bin: nothing misplaced (a swapped pair of bins of similar power would hide in an RMS)
        assert np.max(np.abs(mean[row] - want_mean)) < 1e-4 * np.max(want_mean)


def test_only_one_trace(hostscope):
    """A null mean (or peak) pointer: the other trace alone is written."""
    rng = np.random.default_rng(5)
    chans, _ = sg.baseline_plan(mixed=False)
    cfg, keep = pkg.make_config([dict(channels=[dict(c) for c in chans])], wave_rate=8000, fft_log=9)
    hop, B = C.c_int(0), C.c_int(0)
    hostscope.hostscope_geometry(C.byref(cfg), C.byref(hop), C.byref(B))
    raw, v = _samples(rng, capi.SFMT_U8, (B.value - 1) * hop.value + 512)
    buf = np.zeros(raw.nbytes + 64, np.uint8)
    base = (-buf.ctypes.data) % 16
    buf[base: base + raw.nbytes] = raw
    peak = np.zeros((1, 512), np.float32)
    win = np.zeros(512, np.float32)
    assert hostscope.hostscope_run(C.byref(cfg), buf.ctypes.data + base, raw.nbytes, 0, 1, None, None, peak.ctypes.data, win.ctypes.data) == 1
    want = np.abs(np.fft.fft(v[:512] * win.astype(np.float64))) ** 2
    assert np.sqrt(np.mean((peak[0] - want) ** 2)) / np.sqrt(np.mean(want ** 2)) < POWER_TOL
