"""The band survey on the GPU (airband_hip_set_band_survey / _collect_band_survey / _device_band_survey, csrc/band_survey.hip): every field bit for bit what
capi.band_survey_reference() makes of the scope rows of the same batch, and its selection, lifetime and schedule, which follow the scope's.  Shapes: 2 - 3
dongles, 2 - 5 batches.  (tests/test_host_band_survey.py runs the kernel source on the CPU; this file is what a GPU says.)"""
import numpy as np
import pytest

import helpers
import survey_cases

pytestmark = pytest.mark.gpu

MAX_PEAKS, GUARD, DB = 4, 8, 10.0
RATIO = np.float32(10.0 ** (DB / 10.0))


def _stream(capi, dev, n_samples, seed, tones):
    """Noise and steady tones (frequency as a fraction of the sample rate, amplitude in u8 counts) in the dongle's sample format: tests/test_gpu_band_scope.py's."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_samples, dtype=np.float64)
    z = rng.normal(0.0, 9.0, (n_samples, 2)) @ np.array([1.0, 1j])
    for f, a in tones:
        z += a * np.exp(2j * np.pi * (f * t + rng.random()))
    u8 = np.empty(2 * n_samples, np.uint8)
    u8[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    u8[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    return helpers.convert_format(u8, dev.get("sfmt", capi.SFMT_U8), capi, 1.0)


def _feed(hip, iq, pos):
    for d in range(len(iq)):
        raw = iq[d].view(np.uint8)
        pos[d] += hip.submit(d, raw[pos[d]:])
    assert hip.process(), "not enough input queued"


def _n_samples(n_batches, B, hop, n_fft):
    return (n_batches * B + 100) * hop + n_fft + 8


def _channel_bins(hip, devices):
    out, k = [], 0
    for dev in devices:
        out.append([int(hip.constants(k + j)[0]) for j in range(len(dev["channels"]))])
        k += len(dev["channels"])
    return out


def _freq(b, n):
    return (b if b < n // 2 else b - n) / n


def _free_bins(n, taken, count):
    """`count` bins spread over the part of the band that is further than GUARD + 4 from every bin in `taken`."""
    k = np.arange(n)
    ok = np.ones(n, bool)
    for b in taken:
        d = np.abs(k - b)
        ok &= np.minimum(d, n - d) > GUARD + 4
    free = np.flatnonzero(ok)
    assert len(free) >= 8 * count, "the plan leaves no room for the tones"
    return [int(b) for b in free[np.linspace(0, len(free) - 1, count + 2).astype(int)[1:-1]]]


def _circ(b, n):
    return min(b % n, n - b % n)


def _u8_case(pkg, n_dev, n_batches, seed=0):
    """fft 512, u8, 2.56 MS/s: noise, a tone near bin 0 on every dongle and one further tone that differs by dongle."""
    capi = pkg.capi
    devices = helpers._format_devices(capi, capi.SFMT_U8, 2_560_000, 8000, n_dev)
    iq = [_stream(capi, devices[d], _n_samples(n_batches, 1000, 320, 512), [seed, d], ((_freq(2, 512), 12.0), (0.21 + 0.03 * d, 10.0))) for d in range(n_dev)]
    return devices, iq


def _same(a, b):
    return a["summary"].tobytes() == b["summary"].tobytes() and a["peaks"].tobytes() == b["peaks"].tobytes()


# ---- 1. bit for bit against the rows ---------------------------------------------------------------------------------------------------------------------
CASES = [("SFMT_U8", 2_560_000, 8, False), ("SFMT_U8", 2_560_000, 9, False), ("SFMT_U8", 2_560_000, 10, False), ("SFMT_U8", 2_560_000, 13, False),
         ("SFMT_F32", 8_000_000, 9, True)]  # + CF32 on wide hops


@pytest.mark.parametrize("trace", ["mean", "peak"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d" % (c[0], 1 << c[2]))
def test_survey_equals_the_reference_on_the_rows(pkg, built, case, trace):
    capi = pkg.capi
    sfmt_name, sample_rate, fft_log, wide = case
    n_dev, n_batches, n_fft, wave_rate = 3, 2, 1 << fft_log, 8000
    devices = helpers._format_devices(capi, getattr(capi, sfmt_name), sample_rate, wave_rate, n_dev)
    hop, B = round(sample_rate / wave_rate), wave_rate // 8
    seen = dict(more_than_listed=False, guard_matters=False, at_the_wrap=False)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS if wide else 0) as hip:
        bins = _channel_bins(hip, devices)
        iq = []
        for d in range(n_dev):
            tones = [(_freq(bins[d][2], n_fft), 12.0), (_freq(1, n_fft), 12.0)]  # on a configured channel; one bin from bin 0
            if d == 0:  # six more, spread over what the channels leave free, no two alike
                tones += [(_freq(b, n_fft), 8.0 + i) for i, b in enumerate(_free_bins(n_fft, bins[d] + [1], 6))]
            iq.append(_stream(capi, devices[d], _n_samples(n_batches, B, hop, n_fft), [fft_log, d, sample_rate], tones))
        hip.set_band_scope(windows=8, mean=True, peak=True)
        hip.set_band_survey(trace=trace, max_peaks=MAX_PEAKS, floor_permille=500, threshold_db=DB, guard_bins=GUARD)
        pos = [0] * n_dev
        for b in range(n_batches):
            _feed(hip, iq, pos)
            rows = hip.collect_band_scope()[trace]
            got = hip.collect_band_survey()
            assert got["summary"].shape == (n_dev,) and got["peaks"].shape == (n_dev, MAX_PEAKS)
            for d in range(n_dev):
                want = capi.band_survey_reference(rows[d], bins[d], MAX_PEAKS, 500, RATIO, GUARD)
                s, p = got["summary"][d], got["peaks"][d]
                print("%s fft %d %s batch %d dongle %d: floor %.4g threshold %.4g max %.4g at %d, %d over, %d peaks %s" % (
                    sfmt_name, n_fft, trace, b, d, s["floor"], s["threshold"], s["max_power"], s["max_bin"], s["n_over"], s["n_peaks"], p["bin"].tolist()))
                bad = survey_cases.differences(s, p, want)
                assert not bad, (b, d, bad)
                seen["more_than_listed"] |= int(s["n_peaks"]) > MAX_PEAKS
                seen["guard_matters"] |= bool(survey_cases.differences(s, p, capi.band_survey_reference(rows[d], bins[d], MAX_PEAKS, 500, RATIO, -1)))
                seen["at_the_wrap"] |= any(k >= 0 and _circ(int(k), n_fft) <= GUARD for k in p["bin"])
    assert all(seen.values()), seen  # no rule went unexercised


# ---- 2. the all-equal row ----------------------------------------------------------------------------------------------------------------------------
def test_all_zero_cf32_input(pkg, built):
    capi = pkg.capi
    devices = helpers._format_devices(capi, capi.SFMT_F32, 2_560_000, 8000, 2)
    iq = [np.zeros(2 * _n_samples(1, 1000, 320, 512), np.float32) for _ in range(2)]
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=4)
        hip.set_band_survey(max_peaks=MAX_PEAKS)
        _feed(hip, iq, [0, 0])
        assert not hip.collect_band_scope()["mean"].any()
        got = hip.collect_band_survey()
        for d in range(2):
            s = got["summary"][d]
            assert s.tobytes() == bytes(32)  # floor, threshold, max_power 0.0; max_bin, n_over, n_peaks 0
            assert (got["peaks"][d]["bin"] == -1).all() and not survey_cases.bits(got["peaks"][d]["power"]).any()


# ---- 3. selection ------------------------------------------------------------------------------------------------------------------------------------
def test_mask_selects_one_of_three(pkg, built):
    import torch

    capi = pkg.capi
    devices, iq = _u8_case(pkg, 3, 1)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        bins = _channel_bins(hip, devices)
        hip.set_band_scope(mask=[0, 1, 0], windows=3)
        hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
        with pytest.raises(pkg.AirbandError) as e:  # before any batch
            hip.collect_band_survey()
        assert e.value.code == capi.EAGAIN
        _feed(hip, iq, [0] * 3)
        rows = hip.collect_band_scope()["mean"]
        got = hip.collect_band_survey()
        for d in (0, 2):
            assert got["summary"][d].tobytes() == bytes(32)
            assert (got["peaks"][d]["bin"] == -1).all() and not survey_cases.bits(got["peaks"][d]["power"]).any()
        want = capi.band_survey_reference(rows[1], bins[1], MAX_PEAKS, 500, RATIO, GUARD)
        assert not survey_cases.differences(got["summary"][1], got["peaks"][1], want)
        assert got["summary"][1]["n_peaks"] >= 1
        # ranges, and again: it does not consume the batch
        one = hip.collect_band_survey(first_dev=1, n_dev=1)
        assert one["summary"].tobytes() == got["summary"][1:2].tobytes() and one["peaks"].tobytes() == got["peaks"][1:2].tobytes()
        two = hip.collect_band_survey(first_dev=1, n_dev=2)
        assert two["summary"].tobytes() == got["summary"][1:3].tobytes() and two["peaks"].tobytes() == got["peaks"][1:3].tobytes()
        none = hip.collect_band_survey(first_dev=2, n_dev=1)
        assert none["summary"].tobytes() == bytes(32) and (none["peaks"]["bin"] == -1).all()
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_band_survey(first_dev=2, n_dev=2)
        assert e.value.code == capi.EINVAL
        # the device views are indexed by scope row: one row, dongle 1's
        v = hip.device_band_survey()
        assert v["summary"] and v["peaks"]
        ds = torch.as_tensor(pkg.DevicePtr(v["summary"], (1, 8), "<i4"), device="cuda").cpu().numpy()
        dp = torch.as_tensor(pkg.DevicePtr(v["peaks"], (1, MAX_PEAKS, 2), "<i4"), device="cuda").cpu().numpy()
        assert ds.tobytes() == got["summary"][1:2].tobytes() and dp.tobytes() == got["peaks"][1:2].tobytes()
        hip.collect()


# ---- 4. a switched-off dongle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "pipelined"])
def test_a_disabled_dongle_keeps_its_survey(pkg, built, kind):
    capi = pkg.capi
    pipelined = kind == "pipelined"
    devices, iq = _u8_case(pkg, 3, 5, seed=3)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE if pipelined else 0) as hip:
        hip.set_band_scope(windows=4, mean=True, peak=True)
        hip.set_band_survey(trace="peak", max_peaks=MAX_PEAKS)
        pos = [0] * 3
        _feed(hip, iq, pos)
        if pipelined:  # the survey lags one batch: the batch in flight when the dongle goes off is the last one it takes part in
            _feed(hip, iq, pos)
        hip.device_enable(1, False)
        if pipelined:
            _feed(hip, iq, pos)
        before = hip.collect_band_survey()
        assert before["summary"][1]["n_over"] > 0
        for _ in range(2):  # twice: with two sets the second batch writes the set the first one read
            _feed(hip, iq, pos)
            after = hip.collect_band_survey()
            assert after["summary"][1].tobytes() == before["summary"][1].tobytes() and after["peaks"][1].tobytes() == before["peaks"][1].tobytes()
            for d in (0, 2):
                assert after["summary"][d].tobytes() != before["summary"][d].tobytes()


# ---- 5. pipelined ------------------------------------------------------------------------------------------------------------------------------------
def test_pipelined_survey_lags_with_collect(pkg, built):
    capi = pkg.capi
    n_batches = 3
    devices, iq = _u8_case(pkg, 2, n_batches, seed=5)
    seq = []
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=5)
        hip.set_band_survey(max_peaks=MAX_PEAKS)
        pos = [0, 0]
        for b in range(n_batches):
            _feed(hip, iq, pos)
            seq.append((hip.collect()["waveout"].copy(), hip.collect_band_survey()))
    assert not _same(seq[0][1], seq[1][1])
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE) as hip:
        hip.set_band_scope(windows=5)
        hip.set_band_survey(max_peaks=MAX_PEAKS)
        pos = [0, 0]
        got = []
        for b in range(n_batches):
            _feed(hip, iq, pos)
            if b == 0:
                with pytest.raises(pkg.AirbandError) as e:  # stage 2 of batch 0 has not been enqueued: no results, no survey
                    hip.collect_band_survey()
                assert e.value.code == capi.EAGAIN
                continue
            got.append((hip.collect()["waveout"].copy(), hip.collect_band_survey()))
        hip.flush()
        got.append((hip.collect()["waveout"].copy(), hip.collect_band_survey()))
    assert len(got) == n_batches
    for b in range(n_batches):
        assert np.array_equal(survey_cases.bits(got[b][0]), survey_cases.bits(seq[b][0])), b
        assert _same(got[b][1], seq[b][1]), b


# ---- 6. a handle without a survey --------------------------------------------------------------------------------------------------------------------
def test_a_scope_without_a_survey(pkg, built):
    """collect_band_survey is EINVAL, and neither the audio nor the scope's rows depend on a survey being set on another handle fed the same bytes."""
    capi = pkg.capi
    n_batches = 2
    devices, iq = helpers.format_case(pkg, capi.SFMT_U8, 9, 2_560_000, 8000, 2, n_batches)
    res = []
    for survey in (False, True):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            hip.set_band_scope(windows=8, mean=True, peak=True)
            if survey:
                hip.set_band_survey(max_peaks=MAX_PEAKS)
            pos = [0, 0]
            per = []
            for b in range(n_batches):
                _feed(hip, iq, pos)
                if not survey:
                    with pytest.raises(pkg.AirbandError) as e:
                        hip.collect_band_survey()
                    assert e.value.code == capi.EINVAL
                    with pytest.raises(pkg.AirbandError) as e:
                        hip.device_band_survey()
                    assert e.value.code == capi.EINVAL
                per.append((hip.collect(stats=True), hip.collect_band_scope()))
            res.append(per)
    for b in range(n_batches):
        (a, sa), (s, ss) = res[0][b], res[1][b]
        assert np.array_equal(survey_cases.bits(a["waveout"]), survey_cases.bits(s["waveout"])) and np.array_equal(a["axc"], s["axc"]) and a["stats"] == s["stats"]
        for t in ("mean", "peak"):
            assert np.array_equal(survey_cases.bits(sa[t]), survey_cases.bits(ss[t])), (b, t)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------------------
def test_set_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    devices, iq = _u8_case(pkg, 2, 1)
    M, P = capi.SCOPE_MEAN, capi.SCOPE_PEAK
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        L = hip.L
        assert L.airband_hip_set_band_survey(hip.h, M, 4, 500, 10.0, 8) == capi.EINVAL  # no scope yet
        hip.set_band_scope(windows=2)  # the mean trace alone
        bad = [(0, 4, 500, 10.0, 8), (M | P, 4, 500, 10.0, 8), (4, 4, 500, 10.0, 8), (P, 4, 500, 10.0, 8),  # not exactly one bit the scope keeps
               (M, 0, 500, 10.0, 8), (M, 65, 500, 10.0, 8), (M, 4, -1, 10.0, 8), (M, 4, 1001, 10.0, 8),
               (M, 4, 500, 0.0, 8), (M, 4, 500, -1.0, 8), (M, 4, 500, float("inf"), 8), (M, 4, 500, float("nan"), 8),
               (M, 4, 500, 10.0, -2), (M, 4, 500, 10.0, 257)]
        for args in bad:
            assert L.airband_hip_set_band_survey(hip.h, *args) == capi.EINVAL, args
        with pytest.raises(pkg.AirbandError) as e:  # none of them left a survey behind
            hip.device_band_survey()
        assert e.value.code == capi.EINVAL
        hip.set_band_survey(max_peaks=2, guard_bins=256)
        hip.set_band_survey(max_peaks=64, guard_bins=-1, floor_permille=1000)  # again before the first batch: replaces the survey
        for args in bad:  # and a refused call leaves the one that is set
            assert L.airband_hip_set_band_survey(hip.h, *args) == capi.EINVAL, args
        _feed(hip, iq, [0, 0])
        rows = hip.collect_band_scope()
        assert set(rows) == {"mean"} and rows["mean"].any()  # the scope still delivers
        got = hip.collect_band_survey()
        assert got["peaks"].shape == (2, 64)
        bins = _channel_bins(hip, devices)
        for d in range(2):
            want = capi.band_survey_reference(rows["mean"][d], bins[d], 64, 1000, RATIO, -1)
            assert not survey_cases.differences(got["summary"][d], got["peaks"][d], want)
            assert got["summary"][d]["floor"] == got["summary"][d]["max_power"] == rows["mean"][d].max()
        with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
            hip.set_band_survey()
        assert e.value.code == capi.EINVAL
        assert hip.collect_band_survey()["summary"].tobytes() == got["summary"].tobytes()
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=2)
        hip.set_band_survey()
        hip.set_band_scope(windows=3)  # a new scope drops the survey
        _feed(hip, iq, [0, 0])
        assert hip.collect_band_scope()["mean"].any()
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_band_survey()
        assert e.value.code == capi.EINVAL


# ---- 8. determinism ----------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(pkg, built):
    devices, iq = _u8_case(pkg, 3, 2, seed=11)
    runs = []
    for _ in range(2):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            hip.set_band_scope(windows=7, mean=True, peak=True)
            hip.set_band_survey(trace="peak", max_peaks=16, threshold_db=3.0, guard_bins=2)  # a low threshold: many peaks, full lists
            pos = [0] * 3
            per = []
            for b in range(2):
                _feed(hip, iq, pos)
                per.append(hip.collect_band_survey())
            runs.append(per)
    for b in range(2):
        assert _same(runs[0][b], runs[1][b])
        assert (runs[0][b]["summary"]["n_peaks"] > 0).all()
