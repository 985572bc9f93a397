"""The band scope on the GPU (airband_hip_set_band_scope / _collect_band_scope / _device_band_scope, csrc/band_scope.hip): against a float64 evaluation of its
definition, against what the channelizers leave in the channels' bins, and its selection, lifetime and schedule.  Shapes: 2 - 4 dongles, 2 - 4 batches.
(tests/test_host_band_scope.py runs the kernel source on the CPU; this file is what a GPU says.)"""
import numpy as np
import pytest

import helpers
import pyoracle

pytestmark = pytest.mark.gpu

# Powers against float64, relative to the RMS of the row's bins: twice the bar the wavefront FFT's bins -- amplitudes -- are held to against a float64 FFT,
# normalised by the RMS over the bins, since d(p) / p = 2 d(a) / a.  That bar is tests/test_host_fft.py's
#     assert worst < 2e-6, worst
# (the file that compares the wavefront FFT's bins with float64; its GPU twin tests/test_gpu_wavefront_fft.py compares audio with the oracle, at 1e-4, and holds
# no bar on bins).
AMPLITUDE_TOL = 2e-6
POWER_TOL = 2 * AMPLITUDE_TOL


def _window(n_fft):
    L = pyoracle.lib()
    return np.array([L.orc_window_coeff(n_fft, i) for i in range(n_fft)], np.float64)


def _levels(capi, dev, raw):
    """A dongle's raw samples as the reference converts them (src/rtl_airband.cpp:316-324,403,421), complex float64."""
    sfmt = dev.get("sfmt", capi.SFMT_U8)
    x = raw.astype(np.float64)
    if sfmt == capi.SFMT_U8:
        x = (x - 127.5) / 127.5
    elif sfmt == capi.SFMT_S8:
        x = x / 128.0
    elif sfmt == capi.SFMT_S16:
        x = x * np.float64(np.float32(1.0) / np.float32(dev["fullscale"]))  # 1 / fullscale in float, as the reference multiplies
    return x[0::2] + 1j * x[1::2]


def _stream(capi, dev, n_samples, seed, tones=((0.11, 30.0), (-0.27, 12.0))):
    """Noise and a few steady tones in the dongle's sample format."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.float64)
    z = rng.normal(0.0, 9.0, (n_samples, 2)) @ np.array([1.0, 1j])
    for f, a in tones:
        z += a * np.exp(2j * np.pi * (f * t + rng.random()))
    u8 = np.empty(2 * n_samples, np.uint8)
    u8[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    u8[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    sfmt = dev.get("sfmt", capi.SFMT_U8)
    return helpers.convert_format(u8, sfmt, capi, dev["fullscale"] / 127.5 if sfmt == capi.SFMT_S16 else 1.0)


def _want(capi, dev, iq, b, K, B, hop, n_fft, win):
    """float64 mean and peak of batch b: window j is new hop (j B) / K; the first batch's 100 lead-in hops are never selected."""
    pw = []
    for t in capi.scope_window_hops(K, B):
        s0 = (capi.AGC_EXTRA + b * B + t) * hop
        pw.append(np.abs(np.fft.fft(_levels(capi, dev, iq[2 * s0: 2 * (s0 + n_fft)]) * win)) ** 2)
    pw = np.stack(pw)
    return pw.mean(axis=0), pw.max(axis=0)


def _rel(got, want):
    return float(np.sqrt(np.mean((got.astype(np.float64) - want) ** 2)) / np.sqrt(np.mean(want ** 2)))


def _feed(hip, iq, pos):
    for d in range(len(iq)):
        raw = iq[d].view(np.uint8)
        pos[d] += hip.submit(d, raw[pos[d]:])
    assert hip.process(), "not enough input queued"


def _n_samples(n_batches, B, hop, n_fft):
    return (n_batches * B + 100) * hop + n_fft + 8


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------------------------------
FORMATS = [
    # sample format, sample rate, WAVE_RATE, flags
    ("SFMT_U8", 2_560_000, 8000, 0),            # hop 320
    ("SFMT_U8", 2_400_000, 8000, 0),            # hop 300: windows start off 16 bytes
    ("SFMT_S8", 2_560_000, 16000, 0),
    ("SFMT_S16", 10_000_000, 8000, "WIDE"),     # hop 1 250, wide
    ("SFMT_F32", 8_000_000, 8000, "WIDE"),
]
CASES = [(f, fft_log) for f in FORMATS for fft_log in (8, 9, 10)] + [(FORMATS[4], 13)]  # + CF32 at fft 8192: 64 KiB a window, two wavefronts, eight passes


@pytest.mark.parametrize("fmt,fft_log", CASES, ids=lambda v: v if isinstance(v, int) else "%s-%d" % (v[0], v[1]))
def test_scope_against_float64(pkg, built, fmt, fft_log):
    capi = pkg.capi
    sfmt_name, sample_rate, wave_rate, wide = fmt
    sfmt = getattr(capi, sfmt_name)
    n_dev, n_batches, n_fft = 2, 2, 1 << fft_log
    devices = helpers._format_devices(capi, sfmt, sample_rate, wave_rate, n_dev)
    hop, B = round(sample_rate / wave_rate), wave_rate // 8
    iq = [_stream(capi, devices[d], _n_samples(n_batches, B, hop, n_fft), [fft_log, d, sample_rate]) for d in range(n_dev)]
    win = _window(n_fft)
    worst = 0.0
    for K in (1, 3, B):
        with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS if wide else 0) as hip:
            assert hip.B == B
            hip.set_band_scope(windows=K, mean=True, peak=True)
            pos = [0] * n_dev
            for b in range(n_batches):
                _feed(hip, iq, pos)
                got = hip.collect_band_scope()
                for d in range(n_dev):
                    wm, wp = _want(capi, devices[d], iq[d], b, K, B, hop, n_fft, win)
                    em, ep = _rel(got["mean"][d], wm), _rel(got["peak"][d], wp)
                    print("%s fft %d K %d batch %d dongle %d: mean %.3g peak %.3g" % (sfmt_name, n_fft, K, b, d, em, ep))
                    worst = max(worst, em, ep)
    assert worst < POWER_TOL, worst


# ---- 2. against the channelizer -----------------------------------------------------------------------------------------------------------------------
def _am_case(pkg, sfmt, n_dev, n_batches, fft_log=9):
    """AM channels without lowpass or raw I/Q, a transmitter on every channel."""
    return helpers.format_case(pkg, sfmt, fft_log, 2_560_000, 8000, n_dev, n_batches)


@pytest.mark.parametrize("K", [1, "B"])
@pytest.mark.parametrize("name,sfmt_name,force", [("dft_mfma_i8", "SFMT_U8", False), ("dft_mfma_f32", "SFMT_F32", False), ("fft_wave64", "SFMT_U8", True)])
def test_scope_against_the_channelizer(pkg, built, name, sfmt_name, force, K):
    """For every channel c and selected row r the scope's power in stats.bin of c is read_bins() wavein[c][r] squared: the scope's bar from (1) plus the
    channelizer's (its bins are held to AMPLITUDE_TOL of the bins' RMS, so their squares to POWER_TOL), both relative to the RMS of the row's bins.
    fft_wave64 at K = 1: 2 ulp.  Not bit equality: read_bins() returns sqrt(re^2 + im^2) from v_sqrt_f32 (within 1 ulp), whose square is up to 2 ulp from
    re^2 + im^2.  The complex bins themselves are the same: at fft 512 the scope runs the forced channelizer's own transform (channelizer_fft8_kernel's, from
    csrc/wave_fft8.h).  Measured on an MI355X: 1.20 ulp at most (with the shuffle FFT the scope runs at fft 1024 and up it was 34.6).
    The other handles, same run: dft_mfma_i8 1.2e-6 of the row's RMS (K = 1 and K = WAVE_BATCH), dft_mfma_f32 1.2e-6 and 1.8e-6, fft_wave64 6.3e-7 and 9.6e-7."""
    capi = pkg.capi
    sfmt = getattr(capi, sfmt_name)
    n_dev, n_batches = 2, 2
    devices, iq = _am_case(pkg, sfmt, n_dev, n_batches)
    assert all(c["modulation"] == 0 and c["bandwidth_hz"] == 0 and not c["has_iq_outputs"] for dev in devices for c in dev["channels"])
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_FORCE_FFT if force else 0) as hip:
        assert hip.channelizer_name() == name
        B = hip.B
        k = B if K == "B" else K
        hip.set_band_scope(windows=k, mean=True, peak=True)
        rows = capi.scope_window_hops(k, B)
        pos = [0] * n_dev
        worst, worst_ulp = 0.0, 0.0
        for b in range(n_batches):
            _feed(hip, iq, pos)
            out = hip.collect(stats=True)
            w, _ = hip.read_bins()
            got = hip.collect_band_scope()
            ch = 0
            for d in range(n_dev):
                n_ch = len(devices[d]["channels"])
                bins = [out["stats"][ch + c]["bin"] for c in range(n_ch)]
                p = w[ch:ch + n_ch][:, rows].astype(np.float64) ** 2  # [channel][selected row]
                rms_m = np.sqrt(np.mean(got["mean"][d].astype(np.float64) ** 2))
                rms_p = np.sqrt(np.mean(got["peak"][d].astype(np.float64) ** 2))
                em = np.sqrt(np.mean((got["mean"][d][bins] - p.mean(axis=1)) ** 2)) / rms_m
                ep = np.sqrt(np.mean((got["peak"][d][bins] - p.max(axis=1)) ** 2)) / rms_p
                worst = max(worst, em, ep)
                if k == 1:
                    ulp = np.abs(got["mean"][d][bins].astype(np.float64) - p[:, 0]) / np.spacing(p[:, 0].astype(np.float32)).astype(np.float64)
                    worst_ulp = max(worst_ulp, float(ulp.max()))
                ch += n_ch
            print("%s K %d batch %d: %.3g of the row's RMS%s" % (name, k, b, worst, ", %.2f ulp" % worst_ulp if k == 1 else ""))
        assert worst < 2 * POWER_TOL, worst
        if name == "fft_wave64" and k == 1:
            assert worst_ulp <= 2.0, worst_ulp


# ---- 3. selection and lifetime ------------------------------------------------------------------------------------------------------------------------
def _u8_case(pkg, n_dev, n_batches, seed=0):
    capi = pkg.capi
    devices = helpers._format_devices(capi, capi.SFMT_U8, 2_560_000, 8000, n_dev)
    iq = [_stream(capi, devices[d], _n_samples(n_batches, 1000, 320, 512), [seed, d]) for d in range(n_dev)]
    return devices, iq


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_mask_rows_and_unselected_dongles(pkg, built):
    import torch

    capi = pkg.capi
    devices, iq = _u8_case(pkg, 4, 1)
    win = _window(512)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(mask=[1, 0, 1, 0], windows=3, mean=True, peak=True)
        with pytest.raises(pkg.AirbandError) as e:  # before any batch
            hip.collect_band_scope()
        assert e.value.code == capi.EAGAIN
        _feed(hip, iq, [0] * 4)
        got = hip.collect_band_scope()
        v = hip.device_band_scope()
        assert v["mean"] and v["peak"] and v["row_of_dev"]
        rod = torch.as_tensor(pkg.DevicePtr(v["row_of_dev"], (4,), "<i4"), device="cuda").cpu().numpy()
        assert rod.tolist() == [0, -1, 1, -1]
        rows = torch.as_tensor(pkg.DevicePtr(v["mean"], (2, 512), "<f4"), device="cuda").cpu().numpy()
        assert np.array_equal(_bits(rows[0]), _bits(got["mean"][0])) and np.array_equal(_bits(rows[1]), _bits(got["mean"][2]))
        for d in (1, 3):
            assert not got["mean"][d].any() and not got["peak"][d].any()
        for d in (0, 2):
            wm, wp = _want(capi, devices[d], iq[d], 0, 3, 1000, 320, 512, win)
            assert _rel(got["mean"][d], wm) < POWER_TOL and _rel(got["peak"][d], wp) < POWER_TOL
        one = hip.collect_band_scope(first_dev=2, n_dev=1)  # a range, and again: it does not consume the batch
        assert np.array_equal(_bits(one["mean"][0]), _bits(got["mean"][2]))
        hip.collect()


@pytest.mark.parametrize("flags", ["default", "sequential"])
def test_a_disabled_dongle_keeps_its_rows(pkg, built, flags, monkeypatch):
    """Both where the handle keeps one set of rows and where it keeps two (run-ahead: the default schedule of process_device; the host ring here)."""
    capi = pkg.capi
    if flags == "sequential":
        monkeypatch.setenv("AIRBAND_HIP_RUN_AHEAD", "0")
    devices, iq = _u8_case(pkg, 3, 3, seed=3)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        assert hip.schedule_info()["ring_batches"] == (1 if flags == "sequential" else 2)
        hip.set_band_scope(windows=4, mean=True, peak=True)
        pos = [0] * 3
        _feed(hip, iq, pos)
        before = hip.collect_band_scope()
        hip.device_enable(1, False)
        for _ in range(2):  # twice: with two sets of rows the second batch writes the set the first one read
            _feed(hip, iq, pos)
            after = hip.collect_band_scope()
            for t in ("mean", "peak"):
                assert np.array_equal(_bits(after[t][1]), _bits(before[t][1])), t
                assert not np.array_equal(_bits(after[t][0]), _bits(before[t][0]))


def test_pipelined_scope_lags_with_collect(pkg, built):
    capi = pkg.capi
    n_batches = 3
    devices, iq = _u8_case(pkg, 2, n_batches, seed=5)
    seq = []
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=5, mean=True, peak=True)
        pos = [0, 0]
        for b in range(n_batches):
            _feed(hip, iq, pos)
            seq.append((hip.collect()["waveout"].copy(), hip.collect_band_scope()))
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE) as hip:
        hip.set_band_scope(windows=5, mean=True, peak=True)
        pos = [0, 0]
        got = []
        for b in range(n_batches):
            _feed(hip, iq, pos)
            if b == 0:
                with pytest.raises(pkg.AirbandError) as e:  # stage 2 of batch 0 has not been enqueued: no results, no scope
                    hip.collect_band_scope()
                assert e.value.code == capi.EAGAIN
                continue
            got.append((hip.collect()["waveout"].copy(), hip.collect_band_scope()))
        hip.flush()
        got.append((hip.collect()["waveout"].copy(), hip.collect_band_scope()))
    assert len(got) == n_batches
    for b in range(n_batches):
        assert np.array_equal(_bits(got[b][0]), _bits(seq[b][0])), b
        for t in ("mean", "peak"):
            assert np.array_equal(_bits(got[b][1][t]), _bits(seq[b][1][t])), (b, t)


@pytest.mark.parametrize("flags", [0, "PIPELINE"])
def test_staging_buffers_reused_with_other_content(pkg, built, flags):
    """The host ring's two staging buffers are written again two batches later (ev_stage_read): five batches whose content differs, the scope of batch k
    against float64 of batch k's bytes."""
    capi = pkg.capi
    n_batches, n_dev = 5, 2
    devices = helpers._format_devices(capi, capi.SFMT_U8, 2_560_000, 8000, n_dev)
    B, hop, n_fft = 1000, 320, 512
    n = _n_samples(n_batches, B, hop, n_fft)
    iq = []
    for d in range(n_dev):  # a tone that moves from batch to batch
        parts = [_stream(capi, devices[d], (B + (100 if b == 0 else 0)) * hop, [9, d, b], tones=((0.05 + 0.07 * b, 35.0),)) for b in range(n_batches)]
        iq.append(np.concatenate(parts + [_stream(capi, devices[d], n_fft + 8, [9, d, 99])]))
        assert len(iq[-1]) == 2 * n
    win = _window(n_fft)
    pipelined = flags == "PIPELINE"
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE if pipelined else 0) as hip:
        hip.set_band_scope(windows=8)
        pos = [0] * n_dev
        checked = 0
        for b in range(n_batches + (1 if pipelined else 0)):
            if b < n_batches:
                _feed(hip, iq, pos)  # enqueued back to back with the collect below: nothing waits for the scope but the library's own ordering
            else:
                hip.flush()
            k = b - 1 if pipelined else b
            if k < 0:
                continue
            got = hip.collect_band_scope()
            assert set(got) == {"mean"}
            for d in range(n_dev):
                wm, _ = _want(capi, devices[d], iq[d], k, 8, B, hop, n_fft, win)
                assert _rel(got["mean"][d], wm) < POWER_TOL, (k, d)
                assert int(np.argmax(wm)) == int(np.argmax(got["mean"][d]))  # the batch's own tone
            checked += 1
        assert checked == n_batches


def test_a_handle_without_a_scope(pkg, built):
    """collect_band_scope is EINVAL, and what collect() returns does not depend on a scope being set on another handle fed the same bytes."""
    capi = pkg.capi
    n_batches = 2
    devices, iq = helpers.format_case(pkg, capi.SFMT_U8, 9, 2_560_000, 8000, 2, n_batches)
    for dev in devices:
        dev["channels"][2]["has_iq_outputs"] = 1
    res = []
    for scope in (False, True):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            if scope:
                hip.set_band_scope(windows=8, mean=True, peak=True)
            else:
                with pytest.raises(pkg.AirbandError) as e:
                    hip.collect_band_scope()
                assert e.value.code == capi.EINVAL
                with pytest.raises(pkg.AirbandError) as e:
                    hip.device_band_scope()
                assert e.value.code == capi.EINVAL
            pos = [0, 0]
            per = []
            for b in range(n_batches):
                _feed(hip, iq, pos)
                out = hip.collect(iq=True, stats=True)
                per.append(out)
            res.append(per)
    for b in range(n_batches):
        a, s = res[0][b], res[1][b]
        assert np.array_equal(_bits(a["waveout"]), _bits(s["waveout"])) and np.array_equal(_bits(a["iq_out"]), _bits(s["iq_out"]))
        assert np.array_equal(a["axc"], s["axc"]) and a["stats"] == s["stats"]


def test_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    devices, iq = _u8_case(pkg, 2, 1)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        L = hip.L
        assert L.airband_hip_set_band_scope(None, None, 8, 1) == capi.EINVAL
        for windows, traces, mask in ((0, 1, None), (hip.B + 1, 1, None), (8, 0, None), (8, 4, None), (8, 1, np.zeros(2, np.uint8))):
            assert L.airband_hip_set_band_scope(hip.h, mask.ctypes.data if mask is not None else None, windows, traces) == capi.EINVAL
        hip.set_band_scope(windows=2)
        hip.set_band_scope(windows=hip.B, mean=False, peak=True)  # again before the first batch: replaces the setting
        _feed(hip, iq, [0, 0])
        got = hip.collect_band_scope()
        assert set(got) == {"peak"} and got["peak"].any()
        assert hip.device_band_scope()["mean"] == 0
        with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
            hip.set_band_scope(windows=2)
        assert e.value.code == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_band_scope(first_dev=1, n_dev=2)
        assert e.value.code == capi.EINVAL


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(pkg, built):
    devices, iq = _u8_case(pkg, 3, 2, seed=11)
    runs = []
    for _ in range(2):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            hip.set_band_scope(windows=7, mean=True, peak=True)
            pos = [0] * 3
            per = []
            for b in range(2):
                _feed(hip, iq, pos)
                per.append(hip.collect_band_scope())
            runs.append(per)
    for b in range(2):
        for t in ("mean", "peak"):
            assert np.array_equal(_bits(runs[0][b][t]), _bits(runs[1][b][t]))
