"""The band watch on the GPU (airband_hip_set_band_watch / _collect_band_events / _collect_band_tracks / _device_band_watch, csrc/band_watch.hip): tracks, row
records, the event count and the events byte for byte what capi.band_watch_reference() makes of the handle's own surveys, batch after batch, and its selection,
lifetime and schedule, which follow the survey's -- but for a switched-off dongle, which is frozen.  Shapes: 2 - 3 dongles, 8 - 10 batches, tones keyed per batch.
(tests/test_host_band_watch.py runs the kernel source on the CPU; this file is what a GPU says.)"""
import numpy as np
import pytest

import helpers
import survey_cases

pytestmark = pytest.mark.gpu

MAX_PEAKS, GUARD = 8, 8
WATCH = dict(max_tracks=8, match_bins=2, confirm_hits=2, release_misses=2)


def _freq(b, n):
    return (b if b < n // 2 else b - n) / n


def _free_bins(n, taken, count):
    """`count` bins spread over the part of the band that is further than GUARD + 4 from every bin in `taken` (tests/test_gpu_band_survey.py's)."""
    k = np.arange(n)
    ok = np.ones(n, bool)
    for b in taken:
        d = np.abs(k - b)
        ok &= np.minimum(d, n - d) > GUARD + 4
    free = np.flatnonzero(ok)
    assert len(free) >= 8 * count, "the plan leaves no room for the tones"
    return [int(b) for b in free[np.linspace(0, len(free) - 1, count + 2).astype(int)[1:-1]]]


def _stream(capi, dev, n_samples, seed, tones, B, hop):
    """Noise of sigma 9 and tones (bin frequency as a fraction of the sample rate, amplitude in u8 counts, the batches it is keyed in or None for always) in the
    dongle's sample format.  Batch b's new hops start at hop 100 + b * B (the first batch's lead-in is in front of them)."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 9.0, (n_samples, 2)) @ np.array([1.0, 1j])
    for f, a, batches in tones:
        lo, hi = (0, n_samples) if batches is None else ((100 + batches[0] * B) * hop, min(n_samples, (100 + (batches[1] + 1) * B) * hop))
        t = np.arange(lo, hi, dtype=np.float64)
        z[lo:hi] += a * np.exp(2j * np.pi * (f * t + rng.random()))
    u8 = np.empty(2 * n_samples, np.uint8)
    u8[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    u8[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    return helpers.convert_format(u8, dev.get("sfmt", capi.SFMT_U8), capi, 1.0)


def _channel_bins(pkg, devices, wave_rate, fft_log):
    out, k = [], 0
    for dev in devices:
        out.append([int(pkg.derive_constants(devices, k + j, wave_rate=wave_rate, fft_log=fft_log)[0]) for j in range(len(dev["channels"]))])
        k += len(dev["channels"])
    return out


_CASES = {}


def _case(pkg, sfmt_name="SFMT_U8", sample_rate=2_560_000, fft_log=9, n_dev=3, n_batches=8):
    """Devices, their streams and the keyed tone's bin, made once per shape: a steady tone on every dongle, and on dongle 1 a tone in batches 1 - 4 only; on
    dongle 0 a second keyed tone in batches 2 - 5."""
    key = (sfmt_name, sample_rate, fft_log, n_dev, n_batches)
    if key not in _CASES:
        capi = pkg.capi
        wave_rate, n_fft = 8000, 1 << fft_log
        devices = helpers._format_devices(capi, getattr(capi, sfmt_name), sample_rate, wave_rate, n_dev)
        hop, B = round(sample_rate / wave_rate), wave_rate // 8
        bins = _channel_bins(pkg, devices, wave_rate, fft_log)
        n_samples = (n_batches * B + 100) * hop + n_fft + 8
        iq, keyed = [], None
        for d in range(n_dev):
            free = _free_bins(n_fft, bins[d], 3)
            tones = [(_freq(free[0], n_fft), 11.0, None)]
            if d == 1:
                keyed = free[1]
                tones.append((_freq(free[1], n_fft), 12.0, (1, 4)))
            if d == 0:
                tones.append((_freq(free[2], n_fft), 10.0, (2, 5)))
            iq.append(_stream(capi, devices[d], n_samples, [fft_log, d, sample_rate, 77], tones, B, hop))
        _CASES[key] = (devices, iq, keyed)
    return _CASES[key]


def _feed(hip, iq, pos):
    for d in range(len(iq)):
        raw = iq[d].view(np.uint8)
        pos[d] += hip.submit(d, raw[pos[d]:])
    assert hip.process(), "not enough input queued"


def _take(hip):
    return dict(survey=hip.collect_band_survey(), events=hip.collect_band_events(), tracks=hip.collect_band_tracks())


class Reference:
    """capi.band_watch_reference() advanced on collected surveys: the fleet's expected tables and events."""

    def __init__(self, capi, n_dev, n_fft, selected=None, **w):
        self.capi, self.n_dev, self.n_fft, self.w, self.k = capi, n_dev, n_fft, w, 0
        self.selected = list(range(n_dev)) if selected is None else selected
        self.tracks = np.stack([capi.band_watch_blank(w["max_tracks"])[0] for _ in range(n_dev)])
        self.rows = np.zeros(n_dev, capi.WATCH_ROW_DTYPE)

    def advance(self, survey, off=()):
        events = []
        for d in self.selected:
            if d in off:  # frozen: no events, nothing counts
                self.rows[d]["n_events"] = 0
                continue
            t, r, ev = self.capi.band_watch_reference(self.tracks[d], self.rows[d], survey["peaks"][d], int(survey["summary"]["n_peaks"][d]), self.k, self.w["max_tracks"],
                                                      self.w["match_bins"], self.w["confirm_hits"], self.w["release_misses"], self.n_fft, dev=d)
            self.tracks[d], self.rows[d] = t, r
            events.append(ev)
        self.k += 1
        return np.concatenate(events) if events else np.zeros(0, self.capi.EVENT_DTYPE)


def _check(got, ref, events, max_events, what):
    assert got["tracks"]["tracks"].tobytes() == ref.tracks.tobytes(), (what, "tracks")
    assert got["tracks"]["rows"].tobytes() == ref.rows.tobytes(), (what, "rows")
    assert got["events"]["n_events"] == len(events), (what, got["events"]["n_events"], len(events))
    assert got["events"]["events"].tobytes() == events[:max_events].tobytes(), (what, "events")


def _has(events, kind, dev, near, n_fft):
    return any(int(e["kind"]) == kind and int(e["dev"]) == dev and min(abs(int(e["bin"]) - near), n_fft - abs(int(e["bin"]) - near)) <= 1 for e in events)


# ---- 1. bit for bit on the handle's own surveys ----------------------------------------------------------------------------------------------------------
CASES = [("SFMT_U8", 2_560_000, 9, False, "mean"), ("SFMT_U8", 2_560_000, 9, False, "peak"), ("SFMT_U8", 2_560_000, 8, False, "mean"),
         ("SFMT_U8", 2_560_000, 13, False, "mean"), ("SFMT_F32", 8_000_000, 9, True, "mean")]  # + CF32 on wide hops


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%d-%s" % (c[0], 1 << c[2], c[4]))
def test_watch_equals_the_reference_on_the_surveys(pkg, built, case):
    capi = pkg.capi
    sfmt_name, sample_rate, fft_log, wide, trace = case
    n_dev, n_batches, n_fft = 3, 8, 1 << fft_log
    devices, iq, keyed = _case(pkg, sfmt_name, sample_rate, fft_log, n_dev, n_batches)
    seen = []
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS if wide else 0) as hip:
        hip.set_band_scope(windows=8, mean=True, peak=True)
        hip.set_band_survey(trace=trace, max_peaks=MAX_PEAKS, guard_bins=GUARD)
        hip.set_band_watch(**WATCH)
        max_events = hip.watch_events
        assert max_events == 4 * n_dev
        with pytest.raises(pkg.AirbandError) as e:  # before any batch
            hip.collect_band_events()
        assert e.value.code == capi.EAGAIN
        ref = Reference(capi, n_dev, n_fft, **WATCH)
        pos = [0] * n_dev
        for b in range(n_batches):
            _feed(hip, iq, pos)
            got = _take(hip)
            events = ref.advance(got["survey"])
            print("%s fft %d %s batch %d: %d events %s, live %s" % (sfmt_name, n_fft, trace, b, len(events), [(int(e["kind"]), int(e["dev"]), int(e["bin"])) for e in events],
                                                                ref.rows["n_live"].tolist()))
            _check(got, ref, events, max_events, b)
            assert _take(hip)["events"]["events"].tobytes() == got["events"]["events"].tobytes()  # repeatable: it does not consume the batch
            seen.append(events)
    # non-vacuity, on the reference's output: the tone keyed in batches 1 - 4 on dongle 1 is confirmed at batch 2 and gone at batch 6
    assert _has(seen[2], capi.WATCH_APPEAR, 1, keyed, n_fft), (keyed, seen[2])
    assert _has(seen[6], capi.WATCH_VANISH, 1, keyed, n_fft), (keyed, seen[6])
    assert not any(_has(seen[b], capi.WATCH_APPEAR, 1, keyed, n_fft) for b in (0, 1)) and not any(_has(seen[b], capi.WATCH_VANISH, 1, keyed, n_fft) for b in range(6))


# ---- 2. fewer records than events ------------------------------------------------------------------------------------------------------------------------
def test_more_events_than_records(pkg, built):
    """C = 1: every peak of the first batch is an event.  n_events is exact, the first E records are the reference's first E, the tables are complete."""
    capi = pkg.capi
    devices, iq, _ = _case(pkg)
    w = dict(WATCH, confirm_hits=1)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=8)
        hip.set_band_survey(max_peaks=MAX_PEAKS, threshold_db=6.0, guard_bins=GUARD)
        hip.set_band_watch(max_events=2, **w)
        ref = Reference(capi, 3, 512, **w)
        pos = [0] * 3
        most = 0
        for b in range(3):
            _feed(hip, iq, pos)
            got = _take(hip)
            events = ref.advance(got["survey"])
            _check(got, ref, events, 2, b)
            assert len(got["events"]["events"]) == min(2, len(events))
            most = max(most, len(events))
        assert most > 2  # the case arose


# ---- 3. lifetime -----------------------------------------------------------------------------------------------------------------------------------------
def _sequence(pkg, devices, iq, n_batches, flags=0):
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        hip.set_band_scope(windows=8)
        hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
        hip.set_band_watch(**WATCH)
        pos, out = [0] * len(devices), []
        for b in range(n_batches):
            _feed(hip, iq, pos)
            if flags & pkg.capi.FLAG_PIPELINE and b == 0:
                with pytest.raises(pkg.AirbandError) as e:  # stage 2 of batch 0 has not been enqueued: no results, no events
                    hip.collect_band_events()
                assert e.value.code == pkg.capi.EAGAIN
                continue
            out.append((hip.collect()["waveout"].copy(), _take(hip)))
        if flags & pkg.capi.FLAG_PIPELINE:
            hip.flush()
            out.append((hip.collect()["waveout"].copy(), _take(hip)))
    return out


def _same(a, b):
    return all(a[k][f].tobytes() == b[k][f].tobytes() for k, f in (("survey", "summary"), ("survey", "peaks"), ("events", "events"), ("tracks", "rows"), ("tracks", "tracks"))) \
        and a["events"]["n_events"] == b["events"]["n_events"]


def test_pipelined_watch_lags_with_collect(pkg, built):
    devices, iq, _ = _case(pkg)
    seq = _sequence(pkg, devices, iq, 8)
    got = _sequence(pkg, devices, iq, 8, flags=pkg.capi.FLAG_PIPELINE)
    assert len(got) == len(seq) == 8 and sum(s[1]["events"]["n_events"] for s in seq) >= 2
    for b in range(8):
        assert np.array_equal(survey_cases.bits(got[b][0]), survey_cases.bits(seq[b][0])), b
        assert _same(got[b][1], seq[b][1]), b


def test_process_device_on_a_callers_stream_and_process_bins(pkg, built):
    import torch

    capi = pkg.capi
    devices, iq, keyed = _case(pkg)
    n_dev, n_batches = 3, 8
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=8)
        hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
        hip.set_band_watch(**WATCH)
        g = hip.geometry
        raw = np.stack([x.view(np.uint8) for x in iq])
        stride = (raw.shape[1] + 255) // 256 * 256
        buf = torch.zeros((n_dev, stride), dtype=torch.uint8, device="cuda")
        buf[:, :raw.shape[1]] = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        ref = Reference(capi, n_dev, 512, **WATCH)
        seen = []
        for b in range(n_batches):
            off = 0 if b == 0 else g.first_batch_bytes + (b - 1) * g.batch_bytes
            hip.process_device(buf.data_ptr() + off, stride, stream.cuda_stream)
            got = _take(hip)
            events = ref.advance(got["survey"])
            _check(got, ref, events, hip.watch_events, b)
            seen.append(events)
            if b == 3:  # a batch without input: the watch stays as it is, and k does not advance
                w, q = hip.read_bins()
                hip.process_bins(w, q)
                again = _take(hip)
                assert _same(again, got)
        stream.synchronize()
        assert _has(seen[2], capi.WATCH_APPEAR, 1, keyed, 512) and _has(seen[6], capi.WATCH_VANISH, 1, keyed, 512)
        # the device views: the same bytes
        v = hip.device_band_watch()
        assert all(v.values())
        n = torch.as_tensor(pkg.DevicePtr(v["n_events"], (1,), "<i4"), device="cuda").cpu().numpy()
        t = torch.as_tensor(pkg.DevicePtr(v["tracks"], (n_dev, WATCH["max_tracks"], 6), "<i4"), device="cuda").cpu().numpy()
        r = torch.as_tensor(pkg.DevicePtr(v["rows"], (n_dev, 4), "<i4"), device="cuda").cpu().numpy()
        assert int(n[0]) == got["events"]["n_events"] and t.tobytes() == got["tracks"]["tracks"].tobytes() and r.tobytes() == got["tracks"]["rows"].tobytes()
        del buf


@pytest.mark.parametrize("kind", ["default", "sequential"])
def test_a_switched_off_dongle_is_frozen(pkg, built, kind, monkeypatch):
    """Dongle 1 off for batches 3 - 5, in the middle of its keyed tone (batches 1 - 4): confirmed at batch 2, frozen with no events and no misses while off
    (the survey repeats its stale row: no hits either), released R batches after it is back.  Where the handle keeps two sets and where it keeps one."""
    capi = pkg.capi
    if kind == "sequential":
        monkeypatch.setenv("AIRBAND_HIP_RUN_AHEAD", "0")
    devices, iq, keyed = _case(pkg, n_batches=10)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(windows=8)
        hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
        hip.set_band_watch(**WATCH)
        ref = Reference(capi, 3, 512, **WATCH)
        pos, seen, frozen = [0] * 3, [], None
        for b in range(10):
            if b == 3:
                hip.device_enable(1, False)
            if b == 6:  # back on: its ring starts again where the fleet is (what was queued for it is gone, and submit() dropped its bytes while it was off)
                hip.device_enable(1, True)
                pos[1] = hip.geometry.first_batch_bytes + 5 * hip.geometry.batch_bytes
            for d in range(3):
                if d != 1 or not 3 <= b < 6:
                    pos[d] += hip.submit(d, iq[d].view(np.uint8)[pos[d]:])
            assert hip.process(), "not enough input queued"
            got = _take(hip)
            off = (1,) if 3 <= b < 6 else ()
            events = ref.advance(got["survey"], off=off)
            _check(got, ref, events, hip.watch_events, b)
            seen.append(events)
            if b == 2:
                frozen = got["tracks"]["tracks"][1].tobytes()
                assert int(got["tracks"]["rows"][1]["n_confirmed"]) >= 1
            if off:
                assert got["tracks"]["tracks"][1].tobytes() == frozen and int(got["tracks"]["rows"][1]["n_events"]) == 0
                assert not any(int(e["dev"]) == 1 for e in got["events"]["events"])
        assert _has(seen[2], capi.WATCH_APPEAR, 1, keyed, 512)
        assert _has(seen[7], capi.WATCH_VANISH, 1, keyed, 512) and not any(_has(seen[b], capi.WATCH_VANISH, 1, keyed, 512) for b in range(7))  # its misses: batches 6 and 7


def test_mask_selects_two_of_three(pkg, built):
    capi = pkg.capi
    devices, iq, _ = _case(pkg)
    blank = capi.band_watch_blank(WATCH["max_tracks"])[0].tobytes()
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_band_scope(mask=[1, 0, 1], windows=8)
        hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
        hip.set_band_watch(**WATCH)
        assert hip.watch_events == 8
        ref = Reference(capi, 3, 512, selected=[0, 2], **WATCH)
        pos, total = [0] * 3, 0
        for b in range(8):
            _feed(hip, iq, pos)
            got = _take(hip)
            events = ref.advance(got["survey"])
            _check(got, ref, events, 8, b)
            total += len(events)
            assert got["tracks"]["tracks"][1].tobytes() == blank and got["tracks"]["rows"][1].tobytes() == bytes(16)
            assert all(int(e["dev"]) in (0, 2) for e in events)
        assert total >= 2
        one = hip.collect_band_tracks(first_dev=2, n_dev=1)  # ranges
        assert one["tracks"].tobytes() == got["tracks"]["tracks"][2:3].tobytes() and one["rows"].tobytes() == got["tracks"]["rows"][2:3].tobytes()
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_band_tracks(first_dev=2, n_dev=2)
        assert e.value.code == capi.EINVAL


# ---- 4. determinism, and a handle without a watch --------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_the_watch_changes_nothing_else(pkg, built):
    capi = pkg.capi
    devices, iq, _ = _case(pkg)
    runs = [_sequence(pkg, devices, iq, 4) for _ in range(2)]
    for b in range(4):
        assert _same(runs[0][b][1], runs[1][b][1]), b
    res = []
    for watch in (False, True):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            hip.set_band_scope(windows=8, mean=True, peak=True)
            hip.set_band_survey(max_peaks=MAX_PEAKS, guard_bins=GUARD)
            if watch:
                hip.set_band_watch(**WATCH)
            pos, per = [0] * 3, []
            for b in range(3):
                _feed(hip, iq, pos)
                if not watch:
                    for call in (hip.collect_band_events, hip.collect_band_tracks, hip.device_band_watch):
                        with pytest.raises(pkg.AirbandError) as e:
                            call()
                        assert e.value.code == capi.EINVAL
                per.append((hip.collect(stats=True), hip.collect_band_scope(), hip.collect_band_survey()))
            res.append(per)
    for b in range(3):
        (a, sa, va), (s, ss, vs) = res[0][b], res[1][b]
        assert np.array_equal(survey_cases.bits(a["waveout"]), survey_cases.bits(s["waveout"])) and np.array_equal(a["axc"], s["axc"]) and a["stats"] == s["stats"]
        for t in ("mean", "peak"):
            assert np.array_equal(survey_cases.bits(sa[t]), survey_cases.bits(ss[t])), (b, t)
        assert va["summary"].tobytes() == vs["summary"].tobytes() and va["peaks"].tobytes() == vs["peaks"].tobytes()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------------------------------------
def test_set_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    devices, iq, _ = _case(pkg)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        L = hip.L
        assert L.airband_hip_set_band_watch(hip.h, 8, 2, 2, 4, 4) == capi.EINVAL  # no scope
        hip.set_band_scope(windows=2)
        assert L.airband_hip_set_band_watch(hip.h, 8, 2, 2, 4, 4) == capi.EINVAL  # no survey
        hip.set_band_survey(max_peaks=4)
        most = 3 * (8 + 4)
        bad = [(0, 2, 2, 4, 4), (65, 2, 2, 4, 4), (8, -1, 2, 4, 4), (8, 257, 2, 4, 4), (8, 2, 0, 4, 4), (8, 2, 256, 4, 4), (8, 2, 2, 0, 4), (8, 2, 2, 256, 4),
               (8, 2, 2, 4, 0), (8, 2, 2, 4, most + 1)]
        for args in bad:
            assert L.airband_hip_set_band_watch(hip.h, *args) == capi.EINVAL, args
        with pytest.raises(pkg.AirbandError) as e:  # none of them left a watch behind
            hip.device_band_watch()
        assert e.value.code == capi.EINVAL
        hip.set_band_watch(max_tracks=64, match_bins=256, confirm_hits=255, release_misses=255, max_events=3 * 68)
        hip.set_band_watch(max_tracks=8, max_events=most)  # again before the first batch: replaces the watch
        hip.set_band_survey(max_peaks=4)  # a new survey drops the watch
        with pytest.raises(pkg.AirbandError) as e:
            hip.device_band_watch()
        assert e.value.code == capi.EINVAL
        hip.set_band_watch(**WATCH)
        _feed(hip, iq, [0] * 3)
        assert hip.collect_band_tracks()["tracks"].shape == (3, 8) and hip.collect_band_events()["n_events"] == 0  # C = 2: nothing is confirmed in batch 0
        with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
            hip.set_band_watch()
        assert e.value.code == capi.EINVAL
