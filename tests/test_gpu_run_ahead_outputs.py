"""The optional outputs -- output gate, encoded rows, transmission spool, band scope, survey and watch -- under the default schedule of NULL-stream
airband_hip_process_device() batches (run-ahead: stage 1 of batch k+1 on the front stream beside stage 2 of batch k, the band scope on a third stream), against the
single-stream schedule of a handle prepared under AIRBAND_HIP_RUN_AHEAD=0 (tests/test_gpu_run_ahead.py does this for the plain results and the mixers).

A case is its dongles, their I/Q resident in HBM, configure(h) and take(h): everything the configured outputs deliver for the batch that is ready, as a dict of byte
strings.  Three runs: S, sequential, take() after every batch; A1, run-ahead, take() after every batch, every batch S's bytes; A2, run-ahead, every batch enqueued
back to back with no host call in between, one take() after the last, S's last bytes.  The spool's transmissions are collected once, after the last batch and a
flush.  Same library, same bytes: no comparison between schedules has a tolerance.  A run-ahead handle that falls back to the sequential path fails its case
(schedule_info), and every case asserts on S that the run contained what it is for.

S itself is held to the CPU models of the feature tests (on 8 dongles for the gated outputs, on the 3 dongles of the band case): test_output_gate.expected_active,
capi.audio_encode_reference, capi.transmission_spool_reference, test_gpu_band_scope._want within its POWER_TOL -- the one toleranced comparison here --,
capi.band_survey_reference and test_gpu_band_watch.Reference.

take() reads the full rows through the ranged collect, which does not consume the batch: collect(), collect_active() and collect_active_encoded() each mark the
batch as collected and answer EAGAIN after one another.  A handle with an encoding is asked through collect_active_encoded() and delivers its float rows through
device_active(); a handle with a gate alone through collect_active(iq=True).  Every device_*() view is read back through torch and must hold the collect's bytes."""
import numpy as np
import pytest

import helpers
import survey_cases
import test_gpu_band_scope as bs
import test_gpu_band_survey as sv
import test_gpu_band_watch as bw
import test_output_gate as og
from spool_cases import REC, brief, capi
from test_gpu_run_ahead import N_MIXERS, RING, START_BATCH, WAVE_RATE, Resident, _grab, _handle, _mix, _same, _tweak

pytestmark = pytest.mark.gpu

assert RING == 3 and START_BATCH == 4  # what the batch counts below are written for: the two-deep stage-1 rings wrap while the resident batches repeat
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
IDLE, MAX, FLUSH = capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH
BAND = ("scope_mean", "scope_peak", "summary", "peaks", "n_events", "events", "watch_rows", "tracks")


def _view(pkg, torch, ptr, shape, typestr):
    return torch.as_tensor(pkg.DevicePtr(ptr, shape, typestr), device="cuda").cpu().numpy()


class Case:
    """Dongles, where their resident batches start (ptr(k), stride), and the optional outputs: configure(h) sets them, take(h) collects them."""

    def __init__(self, pkg, torch, devices, ptr, stride, wave_rate=WAVE_RATE, flags=0, mixers=False, gate=None, max_rows=None, encoding=None, spool=None,
                 scope=None, survey=None, watch=None):
        self.pkg, self.torch, self.devices, self.ptr, self.stride, self.wave_rate, self.flags, self.mixers = pkg, torch, devices, ptr, stride, wave_rate, flags, mixers
        self.gate = None if gate is None else np.asarray(gate, np.uint8)
        self.max_rows, self.encoding, self.spool, self.scope, self.survey, self.watch = max_rows, encoding, spool, scope, survey, watch
        self.side = None

    def handle(self, monkeypatch, run_ahead):
        h = _handle(self.pkg, monkeypatch, self.devices, run_ahead, flags=self.flags, mixers=self.mixers, wave_rate=self.wave_rate)
        try:
            self.configure(h)
            info = h.schedule_info()
            assert info["run_ahead"] is run_ahead and info["ring_batches"] == (2 if run_ahead else 1) and info["batches_run_ahead"] == 0, info
        except BaseException:
            h.close()
            raise
        return h

    def configure(self, h):
        if self.gate is not None:
            h.set_output_gate(self.gate, self.max_rows)
        if self.encoding:
            h.set_output_encoding(self.encoding)
        if self.spool:
            h.set_transmission_spool(**self.spool)
        if self.scope:
            h.set_band_scope(**self.scope)
        if self.survey:
            h.set_band_survey(**self.survey)
        if self.watch:
            h.set_band_watch(**self.watch)

    def take(self, h):
        pkg, torch, B, n_ch = self.pkg, self.torch, h.B, h.total_channels
        full = h.collect(iq=True, stats=True, first_channel=0, n_channels=n_ch)
        out = dict(waveout=full["waveout"].tobytes(), iq_out=full["iq_out"].tobytes(), axc=full["axc"].tobytes(), stats=repr(full["stats"]).encode())
        if self.mixers:
            out["mix_left"], out["mix_right"], out["mix_signal"] = (np.ascontiguousarray(a).tobytes() for a in h.collect_mixers())
        if self.gate is not None:
            act = h.collect_active_encoded() if self.encoding else h.collect_active(iq=True)
            kept, rows = len(act["channels"]), h.gate_rows
            v = h.device_active()
            assert int(_view(pkg, torch, v["count"], (1,), "<i4")[0]) == act["n_active"]
            assert _view(pkg, torch, v["index"], (rows,), "<i4")[:kept].tobytes() == act["channels"].tobytes()
            out.update(n_active=b"%d" % act["n_active"], channels=act["channels"].tobytes(), axc_all=act["axcindicate"].tobytes())
            out["rows"] = _view(pkg, torch, v["rows"], (rows, B), "<f4")[:kept].tobytes()
            out["iq_rows"] = _view(pkg, torch, v["iq_rows"], (rows, 2 * B), "<f4")[:kept].tobytes() if v["iq_rows"] else b""
            assert out["rows"] == full["waveout"][act["channels"]].tobytes(), "packed rows"  # copies of this batch's rows, whatever the schedule
            assert out["iq_rows"] == (full["iq_out"][act["channels"]].tobytes() if v["iq_rows"] else b""), "packed raw-I/Q rows"
            if self.encoding:
                out.update(audio=act["audio"].tobytes(), info=act["info"].tobytes())
                e = h.device_active_encoded()
                assert _view(pkg, torch, e["audio"], (rows, B), "<i2" if self.encoding == "s16" else "|u1")[:kept].tobytes() == out["audio"]
                assert _view(pkg, torch, e["info"], (rows, 16), "|u1")[:kept].tobytes() == out["info"]
            else:
                assert act["waveout"].tobytes() == out["rows"]
                assert act["iq_out"].tobytes() == out["iq_rows"] if v["iq_rows"] else not act["iq_out"].any()  # (zeros on a handle without raw-I/Q outputs)
        if self.scope:
            n_dev, N = h.geometry.device_count, h.geometry.fft_size
            sc = h.collect_band_scope()
            v = h.device_band_scope()
            sel = np.flatnonzero(_view(pkg, torch, v["row_of_dev"], (n_dev,), "<i4") >= 0)
            for t in ("mean", "peak"):
                assert (t in sc) == bool(v[t])
                if t in sc:
                    out["scope_" + t] = sc[t].tobytes()
                    assert _view(pkg, torch, v[t], (len(sel), N), "<f4").tobytes() == sc[t][sel].tobytes(), t
        if self.survey:
            got = h.collect_band_survey()
            out.update(summary=got["summary"].tobytes(), peaks=got["peaks"].tobytes())
            v = h.device_band_survey()
            assert _view(pkg, torch, v["summary"], (len(sel), 8), "<i4").tobytes() == got["summary"][sel].tobytes()
            assert _view(pkg, torch, v["peaks"], (len(sel), h.survey_peaks, 2), "<i4").tobytes() == got["peaks"][sel].tobytes()
        if self.watch:
            ev, tr = h.collect_band_events(), h.collect_band_tracks()
            out.update(n_events=b"%d" % ev["n_events"], events=ev["events"].tobytes(), watch_rows=tr["rows"].tobytes(), tracks=tr["tracks"].tobytes())
            v = h.device_band_watch()
            assert int(_view(pkg, torch, v["n_events"], (1,), "<i4")[0]) == ev["n_events"]
            assert _view(pkg, torch, v["events"], (h.watch_events, 4), "<i4")[:len(ev["events"])].tobytes() == out["events"]
            assert _view(pkg, torch, v["rows"], (len(sel), 4), "<i4").tobytes() == tr["rows"][sel].tobytes()
            assert _view(pkg, torch, v["tracks"], (len(sel), h.watch_tracks, 6), "<i4").tobytes() == tr["tracks"][sel].tobytes()
        return out

    def finish(self, h, model=None):
        """After the last batch: flush, collect until nothing waits, the counters.  With the CPU model: every call must agree with it."""
        pkg, torch = self.pkg, self.torch
        h.spool_flush()
        if model is not None:
            model.flush()
        records, audio = [], []
        for call in range(64):
            g = h.collect_transmissions()
            if model is not None:
                w = model.collect()
                assert len(g["records"]) == len(w["records"]) and g["n_waiting"] == w["n_waiting"], (call, len(g["records"]), len(w["records"]), g["n_waiting"], w["n_waiting"])
                assert g["records"].tobytes() == w["records"].tobytes(), (call, brief(g["records"][:4]), brief(w["records"][:4]))
                assert g["audio"].shape[0] == w["n_rows"] and g["audio"].tobytes() == w["audio"], (call, "audio")
            v = h.device_transmission_spool()
            n = _view(pkg, torch, v["n_export"], (3,), "<i4")
            assert n.tolist() == [len(g["records"]), g["audio"].shape[0], g["n_waiting"]]
            assert _view(pkg, torch, v["records"], (h.spool_max_records, 48), "|u1")[:len(g["records"])].tobytes() == g["records"].tobytes()
            records.append(g["records"])
            audio.append(g["audio"].tobytes())
            if g["n_waiting"] == 0:
                break
        else:
            raise AssertionError("transmissions still wait after 64 collects")
        counters = h.spool_counters()
        if model is not None:
            assert counters == model.counters(), (counters, model.counters())
        return dict(records=np.concatenate(records).tobytes(), spool_audio=b"".join(audio), counters=repr(sorted(counters.items())).encode(), calls=b"%d" % len(records))


def _equal(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in want:
        assert got[key] == want[key], "%s: %s" % (what, key)


def _drive(case, monkeypatch, run_ahead, n, take_at=None, detours=None, hooks=None, model_step=None):
    """n batches through a fresh handle.  detours: {k: "side" (process_device on a caller's stream) or (wavein, iq_in) for process_bins}; hooks: {k: f(h)} called
    right behind batch k's enqueue; take_at: the batches to take() behind (None: every one).  Returns ({k: take}, the spool's end or None)."""
    detours, hooks = detours or {}, hooks or {}
    if "side" in detours.values() and case.side is None:
        case.side = case.torch.cuda.Stream()
    with case.handle(monkeypatch, run_ahead) as h:
        takes, ahead = {}, 0
        for k in range(n):
            how = detours.get(k)
            if how is None:
                h.process_device(case.ptr(k), case.stride)
                ahead += 1 if run_ahead else 0
            elif isinstance(how, str):
                h.process_device(case.ptr(k), case.stride, case.side.cuda_stream)
            else:
                h.process_bins(*how)
            if k in hooks:
                hooks[k](h)
            if take_at is None or k in take_at:
                takes[k] = case.take(h)
                if model_step:
                    model_step(k, takes[k])
            info = h.schedule_info()
            assert info["run_ahead"] is run_ahead and info["batches_run_ahead"] == ahead, (k, info, ahead)
        end = case.finish(h, model_step.model if model_step else None) if case.spool else None
    return takes, end


def _three_runs(case, monkeypatch, n, **how):
    """S, A1 and A2; returns S's takes and its spool's end."""
    want, want_end = _drive(case, monkeypatch, False, n, **how)
    got, end = _drive(case, monkeypatch, True, n, **how)
    for k in range(n):
        _equal(got[k], want[k], "run ahead, every batch collected: batch %d" % k)
    if want_end:
        _equal(end, want_end, "run ahead, every batch collected: the spool's end")
    got, end = _drive(case, monkeypatch, True, n, take_at=(n - 1,), **how)
    _equal(got[n - 1], want[n - 1], "run ahead, %d batches back to back" % n)
    if want_end:
        _equal(end, want_end, "run ahead, back to back: the spool's end")
    return want, want_end


def _batch_bins(case, monkeypatch, k):
    """read_bins() of batch k on a sequential handle of the case: what a process_bins in place of batch k is fed"""
    with case.handle(monkeypatch, False) as h:
        for b in range(k + 1):
            h.process_device(case.ptr(b), case.stride)
        return h.read_bins()


# ---- 1. gate, encoding and spool ------------------------------------------------------------------------------------------------------------------------
N_GATED = 9  # the lead-in batch, then the two-deep ring wraps four times
SPOOL = dict(min_batches=2, idle_batches=1)
_RESIDENT = {}


def _resident(pkg, torch, n_dev):
    """the mixed plan's I/Q of test_gpu_run_ahead.py for n_dev dongles, generated once"""
    if n_dev not in _RESIDENT:
        devices, carriers = helpers.plan_devices(n_dev, True, _tweak)
        mp = pytest.MonkeyPatch()
        try:
            with _handle(pkg, mp, devices, run_ahead=False) as h:
                _RESIDENT[n_dev] = (devices, Resident(pkg, torch, h, carriers))
        finally:
            mp.undo()
    return _RESIDENT[n_dev]


def _gated_case(pkg, torch, n_dev, fmt, max_batches, max_rows, **band):
    devices, res = _resident(pkg, torch, n_dev)
    n_ch = 8 * n_dev
    gate = np.array([(NEVER, SIGNAL, ALWAYS)[c % 3] for c in range(n_ch)], np.uint8)
    spool = dict(SPOOL, pool_rows=4 * n_ch, max_records=4 * n_ch)
    if max_batches:
        spool["max_batches"] = max_batches
    return Case(pkg, torch, devices, res.ptr, res.stride, mixers=True, gate=gate, max_rows=max_rows, encoding=fmt, spool=spool, **band)


def _spool_contained(case, takes, end, max_batches):
    """on S: rows past max_rows, a transmission across a batch boundary, and with max_batches both ways to close"""
    assert max(int(t["n_active"]) for t in takes.values()) > case.max_rows, [int(t["n_active"]) for t in takes.values()]
    recs = np.frombuffer(end["records"], REC)
    assert len(recs) > 0 and (recs["n_rows"] >= 2).any() and (recs["peak"] > 0).any(), brief(recs[:8])
    assert IDLE in recs["reason"].tolist(), sorted(set(recs["reason"].tolist()))
    if max_batches:
        assert MAX in recs["reason"].tolist(), sorted(set(recs["reason"].tolist()))
    assert any(np.frombuffer(t["mix_left"], np.float32).any() for t in takes.values())


GATED = [("ulaw", 0), ("s16", 0), ("ulaw", 2), ("s16", 2)]


@pytest.mark.parametrize("fmt,max_batches", GATED, ids=lambda v: v if isinstance(v, str) else "max%d" % v)
def test_gate_encoding_and_spool(pkg, built, monkeypatch, fmt, max_batches):
    """64 dongles of the mixed plan with mixers; gate bytes NEVER / SIGNAL / ALWAYS in turn, 200 rows where up to 170 ALWAYS channels and the SIGNAL channels
    with audio are active."""
    torch = pytest.importorskip("torch")
    case = _gated_case(pkg, torch, 64, fmt, max_batches, 200)
    takes, end = _three_runs(case, monkeypatch, N_GATED)
    _spool_contained(case, takes, end, max_batches)


class _GatedModels:
    """S's gated outputs of one batch against the rule, the encoder's definition, and the spool's model stepped with them"""

    def __init__(self, case, B):
        self.case, self.B, self.hist = case, B, []
        s = case.spool
        self.model = capi.transmission_spool_reference(case.gate == SIGNAL, B, pool_rows=s["pool_rows"], export_rows=max(s["pool_rows"], s.get("max_batches", 480) + 1),
                                                       max_records=s["max_records"], min_batches=s["min_batches"], idle_batches=s["idle_batches"],
                                                       max_batches=s.get("max_batches", 480))

    def __call__(self, k, t):
        case, B = self.case, self.B
        n_ch = len(case.gate)
        self.hist.append(np.frombuffer(t["axc"], np.uint8))
        want = og.expected_active(case.gate, self.hist)[-1]
        kept = np.asarray(want[:case.max_rows], np.intp)
        assert int(t["n_active"]) == len(want), (k, int(t["n_active"]), want)
        assert np.frombuffer(t["channels"], np.int32).tolist() == kept.tolist(), k
        assert t["axc_all"] == t["axc"], k
        wave = np.frombuffer(t["waveout"], np.float32).reshape(n_ch, B)
        assert t["rows"] == wave[kept].tobytes(), (k, "packed rows")
        assert t["iq_rows"] == np.frombuffer(t["iq_out"], np.float32).reshape(n_ch, 2 * B)[kept].tobytes(), (k, "packed raw-I/Q rows")
        audio, info = capi.audio_encode_reference(wave[kept], case.encoding)
        info["channel"] = kept
        assert t["audio"] == audio.tobytes(), (k, "encoded rows")
        assert t["info"] == info.tobytes(), (k, "records")
        self.model.step(len(want), kept, audio, info, selected=want if len(want) > len(kept) else None)


@pytest.mark.parametrize("fmt,max_batches", GATED, ids=lambda v: v if isinstance(v, str) else "max%d" % v)
def test_sequential_gated_outputs_against_the_cpu_models(pkg, built, monkeypatch, fmt, max_batches):
    """The same plan and settings on 8 dongles, 24 rows: S against expected_active, audio_encode_reference and transmission_spool_reference; then A2 against S."""
    torch = pytest.importorskip("torch")
    case = _gated_case(pkg, torch, 8, fmt, max_batches, 24)
    with case.handle(monkeypatch, False) as h:
        B = h.B
    takes, end = _drive(case, monkeypatch, False, N_GATED, model_step=_GatedModels(case, B))
    _spool_contained(case, takes, end, max_batches)
    got, got_end = _drive(case, monkeypatch, True, N_GATED, take_at=(N_GATED - 1,))
    _equal(got[N_GATED - 1], takes[N_GATED - 1], "8 dongles, run ahead, back to back")
    _equal(got_end, end, "8 dongles, run ahead, back to back: the spool's end")


# ---- 2. scope, survey and watch -------------------------------------------------------------------------------------------------------------------------
N_BAND = 8
_BAND = {}


def _band_input(pkg, torch):
    """test_gpu_band_watch._case(): 3 dongles of u8 at WAVE_RATE 8000 and fft 512, a tone on dongle 1 keyed in batches 1 - 4; uploaded once"""
    if not _BAND:
        devices, iq, keyed = bw._case(pkg)
        raw = np.stack([x.view(np.uint8) for x in iq])
        stride = (raw.shape[1] + 255) // 256 * 256
        buf = torch.zeros((len(devices), stride), dtype=torch.uint8, device="cuda")
        buf[:, :raw.shape[1]] = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        with pkg.AirbandHip(devices, wave_rate=8000) as h:
            g = h.geometry
            first, batch = g.first_batch_bytes, g.batch_bytes
            assert first + (N_BAND - 1) * batch + g.lookahead_bytes <= raw.shape[1]
        _BAND.update(devices=devices, iq=iq, keyed=keyed, buf=buf, stride=stride, ptr=lambda k: buf.data_ptr() + (0 if k == 0 else first + (k - 1) * batch))
    return _BAND


def _band_case(pkg, torch, mask=None, flags=0, gate=None):
    b = _band_input(pkg, torch)
    return Case(pkg, torch, b["devices"], b["ptr"], b["stride"], wave_rate=8000, flags=flags, gate=gate, scope=dict(mask=mask, windows=8, mean=True, peak=True),
                survey=dict(max_peaks=bw.MAX_PEAKS, guard_bins=bw.GUARD), watch=dict(bw.WATCH))


class _BandModels:
    """S's band outputs, batch by batch: the scope against float64 of the batch's own bytes, the survey against its definition on S's rows, the watch against
    Reference.advance() on S's survey"""

    def __init__(self, pkg, mask):
        b = _BAND
        self.pkg, self.devices, self.iq = pkg, b["devices"], b["iq"]
        self.sel = [d for d in range(3) if mask is None or mask[d]]
        self.bins = bw._channel_bins(pkg, self.devices, 8000, 9)
        self.win = bs._window(512)
        self.ref = bw.Reference(capi, 3, 512, selected=self.sel, **bw.WATCH)
        self.seen = {}

    def check(self, k, t, off=()):
        """k: the batch whose input the handle looked at"""
        rows = {tr: np.frombuffer(t["scope_" + tr], np.float32).reshape(3, 512) for tr in ("mean", "peak")}
        summary = np.frombuffer(t["summary"], capi.SUMMARY_DTYPE)
        peaks = np.frombuffer(t["peaks"], capi.PEAK_DTYPE).reshape(3, bw.MAX_PEAKS)
        for d in range(3):
            if d not in self.sel:
                assert not rows["mean"][d].any() and not rows["peak"][d].any() and summary[d].tobytes() == bytes(32) and (peaks[d]["bin"] == -1).all(), (k, d)
                continue
            if d not in off:  # a switched-off dongle's rows are an earlier batch's
                wm, wp = bs._want(capi, self.devices[d], self.iq[d], k, 8, 1000, 320, 512, self.win)
                em, ep = bs._rel(rows["mean"][d], wm), bs._rel(rows["peak"][d], wp)
                print("batch %d dongle %d: mean %.3g peak %.3g of the row's RMS" % (k, d, em, ep))
                assert em < bs.POWER_TOL and ep < bs.POWER_TOL, (k, d, em, ep)
            want = capi.band_survey_reference(rows["mean"][d], self.bins[d], bw.MAX_PEAKS, 500, sv.RATIO, bw.GUARD)
            bad = survey_cases.differences(summary[d], peaks[d], want)
            assert not bad, (k, d, bad)
        events = self.ref.advance(dict(summary=summary, peaks=peaks), off=off)
        got = dict(tracks=dict(tracks=np.frombuffer(t["tracks"], capi.TRACK_DTYPE).reshape(3, bw.WATCH["max_tracks"]), rows=np.frombuffer(t["watch_rows"], capi.WATCH_ROW_DTYPE)),
                   events=dict(n_events=int(t["n_events"]), events=np.frombuffer(t["events"], capi.EVENT_DTYPE)))
        bw._check(got, self.ref, events, 4 * len(self.sel), k)
        self.seen[k] = events


def _band_contained(models, takes, n, skipped=()):
    """on S: the keyed tone appears and vanishes where the reference puts it, and consecutive batches' rows differ"""
    keyed, seen = _BAND["keyed"], models.seen
    assert bw._has(seen[2], capi.WATCH_APPEAR, 1, keyed, 512), (keyed, seen[2])
    assert bw._has(seen[6], capi.WATCH_VANISH, 1, keyed, 512), (keyed, seen[6])
    assert not any(bw._has(seen[k], capi.WATCH_VANISH, 1, keyed, 512) for k in seen if k < 6)
    for k in range(1, n):
        for key in ("scope_mean", "scope_peak", "summary"):
            assert (takes[k][key] == takes[k - 1][key]) == (k in skipped), (k, key)


BAND_CASES = [(None, 0), ((1, 1, 0), 0), (None, "FLAG_FORCE_FFT"), ((1, 1, 0), "FLAG_FORCE_FFT")]


@pytest.mark.parametrize("mask,flag", BAND_CASES, ids=["every_dongle", "two_of_three", "fft_wave64-every_dongle", "fft_wave64-two_of_three"])
def test_scope_survey_and_watch(pkg, built, monkeypatch, mask, flag):
    torch = pytest.importorskip("torch")
    case = _band_case(pkg, torch, mask, getattr(capi, flag) if flag else 0)
    with case.handle(monkeypatch, True) as h:
        assert h.channelizer_name() == ("fft_wave64" if flag else "dft_mfma_i8")
    takes, _ = _three_runs(case, monkeypatch, N_BAND)
    models = _BandModels(pkg, mask)
    for k in range(N_BAND):
        models.check(k, takes[k])
    _band_contained(models, takes, N_BAND)


# ---- 3. everything at once, at a size that overlaps -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)  # two seconds on an idle MI355X; the rest is for 10 GB of I/Q to be allocated and generated beside other work
def test_every_output_on_batches_long_enough_to_overlap(pkg, built, monkeypatch):
    """4 096 dongles, the construction of test_gpu_run_ahead.py::test_batches_long_enough_to_overlap, whose argument this size rests on: stage 2 of batch k is still
    running when stage 1 of batch k+1 is enqueued.  Mixers, gate, u-law rows, spool, and scope, survey and watch on every 64th dongle; eight batches back to back on
    either schedule, the last one and the spool's end compared."""
    torch = pytest.importorskip("torch")
    n_dev, n = 4096, 8
    devices, carriers = helpers.plan_devices(n_dev, True, _tweak)
    n_ch = 8 * n_dev
    case = Case(pkg, torch, devices, None, 0, mixers=True, gate=[(NEVER, SIGNAL, ALWAYS)[c % 3] for c in range(n_ch)], max_rows=n_ch // 4, encoding="ulaw",
                spool=dict(SPOOL, pool_rows=n_ch, max_records=n_ch), scope=dict(mask=[d % 64 == 0 for d in range(n_dev)], windows=8, mean=True, peak=True),
                survey=dict(max_peaks=bw.MAX_PEAKS, guard_bins=-1), watch=dict(bw.WATCH))  # every peak: this plan's carriers all sit on configured channels
    with case.handle(monkeypatch, False) as h:
        res = Resident(pkg, torch, h, carriers)
    case.ptr, case.stride = res.ptr, res.stride
    want, want_end = _drive(case, monkeypatch, False, n, take_at=(n - 1,))
    got, end = _drive(case, monkeypatch, True, n, take_at=(n - 1,))
    del res  # 10 GB: hand them back before the next test
    case.ptr = None
    torch.cuda.empty_cache()
    want, got = want[n - 1], got[n - 1]
    assert int(want["n_active"]) > case.max_rows and np.frombuffer(want["axc"], np.uint8).tolist().count(ord(" ")) < n_ch
    recs = np.frombuffer(want_end["records"], REC)
    assert len(recs) > 0 and (recs["n_rows"] >= 2).any() and {IDLE, FLUSH} <= set(recs["reason"].tolist())
    assert np.frombuffer(want["summary"], capi.SUMMARY_DTYPE)["n_over"].sum() > 0 and np.frombuffer(want["watch_rows"], capi.WATCH_ROW_DTYPE)["n_live"].sum() > 0
    _equal(got, want, "4 096 dongles, after batch %d" % (n - 1))
    _equal(end, want_end, "4 096 dongles: the spool's end")


# ---- 4. the sequential detours, with outputs on ---------------------------------------------------------------------------------------------------------
def _detours(case, monkeypatch):
    """batches 2, 3 and 5 on a caller's stream, a process_bins of the sequential handle's own stage-1 output in place of batch 4"""
    return {2: "side", 3: "side", 5: "side", 4: _batch_bins(case, monkeypatch, 4)}


def test_detours_with_gate_encoding_and_spool(pkg, built, monkeypatch):
    torch = pytest.importorskip("torch")
    case = _gated_case(pkg, torch, 64, "ulaw", 2, 200)
    detours = _detours(case, monkeypatch)
    want, want_end = _drive(case, monkeypatch, False, N_GATED, detours=detours)
    got, end = _drive(case, monkeypatch, True, N_GATED, detours=detours)  # (_drive counts the NULL-stream batches alone as run ahead)
    for k in range(N_GATED):
        _equal(got[k], want[k], "batch %d" % k)
    _equal(end, want_end, "the spool's end")
    _spool_contained(case, want, want_end, 2)
    # the detours change nothing the gated outputs are made of: S driven straight gives the same bytes
    straight, straight_end = _drive(case, monkeypatch, False, N_GATED, take_at=(N_GATED - 1,))
    _equal(want[N_GATED - 1], straight[N_GATED - 1], "sequential, with and without the detours")
    _equal(want_end, straight_end, "sequential, with and without the detours: the spool's end")


@pytest.mark.parametrize("flag", [0, "FLAG_FORCE_FFT"], ids=["default", "fft_wave64"])
def test_detours_with_scope_survey_and_watch(pkg, built, monkeypatch, flag):
    torch = pytest.importorskip("torch")
    case = _band_case(pkg, torch, None, getattr(capi, flag) if flag else 0)
    detours = _detours(case, monkeypatch)
    want, _ = _drive(case, monkeypatch, False, N_BAND, detours=detours)
    got, _ = _drive(case, monkeypatch, True, N_BAND, detours=detours)
    for k in range(N_BAND):
        _equal(got[k], want[k], "batch %d" % k)
    # a batch without input leaves the band outputs as batch 3 left them, and the watch's batch number does not advance: the reference is not advanced either
    for key in BAND:
        assert want[4][key] == want[3][key], key
    models = _BandModels(pkg, None)
    for k in range(N_BAND):
        if k != 4:
            models.check(k, want[k])
    _band_contained(models, want, N_BAND, skipped=(4,))


# ---- 5. a dongle switched off and on between batches in flight --------------------------------------------------------------------------------------------
def test_a_dongle_switched_off_and_on_between_batches_in_flight(pkg, built, monkeypatch):
    """Dongle 1 off right behind the enqueue of batch 2 (batches 0 - 2 are enqueued back to back: on the run-ahead handle they are in flight), on again behind batch
    5.  device_enable() takes effect with the next batch."""
    torch = pytest.importorskip("torch")
    gate = np.array([(NEVER, SIGNAL, ALWAYS)[c % 3] for c in range(24)], np.uint8)
    case = _band_case(pkg, torch, None, 0, gate=gate)
    hooks = {2: lambda h: h.device_enable(1, False), 5: lambda h: h.device_enable(1, True)}
    at = tuple(range(2, N_BAND))
    want, _ = _drive(case, monkeypatch, False, N_BAND, take_at=at, hooks=hooks)
    got, _ = _drive(case, monkeypatch, True, N_BAND, take_at=at, hooks=hooks)
    for k in at:
        _equal(got[k], want[k], "batch %d" % k)
    models = _BandModels(pkg, None)
    early, _ = _drive(case, monkeypatch, False, 2)  # batches 0 and 1 were not taken above: the models walk through them on a handle that stops there
    for k in (0, 1):
        models.check(k, early[k])
    hist, on = [np.frombuffer(early[k]["axc"], np.uint8) for k in (0, 1)], [np.ones(24, bool)] * 2
    for k in at:
        off = (1,) if 3 <= k <= 5 else ()
        models.check(k, want[k], off=off)
        hist.append(np.frombuffer(want[k]["axc"], np.uint8))
        on.append(np.array([not (off and 8 <= c < 16) for c in range(24)]))
        active = og.expected_active(gate, hist, on)[-1]
        assert int(want[k]["n_active"]) == len(active) and np.frombuffer(want[k]["channels"], np.int32).tolist() == active, (k, active)
        if off:  # its scope and track rows are batch 2's bytes, no event names it, none of its channels is delivered
            for key, per in (("scope_mean", 2048), ("scope_peak", 2048), ("summary", 32), ("peaks", 8 * bw.MAX_PEAKS), ("tracks", 24 * bw.WATCH["max_tracks"])):
                assert want[k][key][per:2 * per] == want[2][key][per:2 * per], (k, key)
                assert want[k][key][:per] != want[2][key][:per], (k, key)  # dongle 0's move on
            assert not any(int(e["dev"]) == 1 for e in np.frombuffer(want[k]["events"], capi.EVENT_DTYPE))
            assert not any(8 <= c < 16 for c in active) and any(gate[c] == ALWAYS for c in range(8, 16))
    assert bw._has(models.seen[2], capi.WATCH_APPEAR, 1, _BAND["keyed"], 512)
    assert want[6]["scope_mean"][2048:4096] != want[2]["scope_mean"][2048:4096]  # back on


# ---- 6. mixer exchange between two run-ahead handles ------------------------------------------------------------------------------------------------------
def test_add_mixers_between_two_run_ahead_handles(pkg, built, monkeypatch):
    """dst.add_mixers(src) behind every pair of batches: with nothing in between on the host, and with dst's sums collected every time -- the sums of the same pair
    prepared sequentially."""
    torch = pytest.importorskip("torch")
    n = 7
    devices, res = _resident(pkg, torch, 64)
    other = [(d, c, (d + c) % N_MIXERS, 0.5 + 0.05 * c, 0.25 if c == 2 else 0.0) for d, c, *_ in _mix(64)]

    def pair(run_ahead, collect_every):
        sums = {}
        with _handle(pkg, monkeypatch, devices, run_ahead) as dst, _handle(pkg, monkeypatch, devices, run_ahead, mixers=False) as src:
            src.set_mixers(N_MIXERS, other)
            for k in range(n):
                src.process_device(res.ptr(k), res.stride)
                dst.process_device(res.ptr(k), res.stride)
                dst.add_mixers(src)
                if collect_every or k == n - 1:
                    sums[k] = _grab(dst)
            for h in (dst, src):
                info = h.schedule_info()
                assert info["run_ahead"] is run_ahead and info["batches_run_ahead"] == (n if run_ahead else 0), info
            alone = src.collect_mixers()
        return sums, alone

    want, alone = pair(False, True)
    assert any(np.abs(a).max() > 0 for a in alone[:2])
    with _handle(pkg, monkeypatch, devices, False) as h:  # the exchange did add something: dst's own sums are others
        for k in range(n):
            h.process_device(res.ptr(k), res.stride)
        assert not np.array_equal(_grab(h)["mix"][0], want[n - 1]["mix"][0])
    got, _ = pair(True, False)
    _same(got[n - 1], want[n - 1], "add_mixers, %d batch pairs back to back" % n)
    got, _ = pair(True, True)
    for k in range(n):
        _same(got[k], want[k], "add_mixers, collected every time: batch %d" % k)
