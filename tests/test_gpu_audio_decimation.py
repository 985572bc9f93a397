"""Output decimation on the GPU (airband_hip_set_output_decimation / _encoded_row_samples / _decimate_audio, csrc/audio_decimate.hip).

Every comparison is byte for byte: behind the one float32 multiplication the definition is integer arithmetic.  A decimating handle and a twin with the gate
alone are fed the same input; per batch the handle's encoded rows and records must equal capi.audio_decimate_reference() of the float rows the twin's
collect_active() delivers, with the per-channel history carried by the listed rule (tests/decimation_cases.Model), and the count and the list must be the
twin's.  The transmission spool and the RTP stream of a decimating handle are compared with their references fed the reference's decimated rows.
decimate_audio() is how the GPU meets the inputs a demodulator never produces.  (AIRBAND_HIP_EBADSIZE cannot be provoked on a handle: wave_batch is 1000 or
2000, and both halves are multiples of four.)"""
import ctypes as C

import numpy as np
import pytest

import audio_cases as ac
import decimation_cases as dc
import rtp_cases as rc
import test_gpu_audio_encoding as ae
import test_gpu_gate as gg
import test_output_gate as og

pytestmark = pytest.mark.gpu

NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
N_BATCHES = 5
H = dc.H


class Pair:
    """the decimating handle, its twin (the gate alone, a list as long as the fleet) and the model; step() checks the batch that is ready on both"""

    def __init__(self, pkg, hip, twin, fmt, gate, max_rows=None):
        self.pkg, self.hip, self.twin, self.fmt = pkg, hip, twin, fmt
        hip.set_output_gate(gate, max_rows)
        twin.set_output_gate(gate)
        hip.set_output_encoding(fmt)
        assert hip.encoded_row_samples() == hip.B
        hip.set_output_decimation(2)
        assert hip.encoded_row_samples() == hip.B // 2
        self.model = dc.Model(hip.total_channels, fmt)
        self.lists, self.selected, self.infos = [], [], []

    def reference_step(self, what=""):
        """the twin's batch through the model: (the twin's collect_active(), the listed channels, their decimated rows, their records)"""
        ae._same_full(ae._full(self.hip), ae._full(self.twin), what)
        act = self.twin.collect_active()
        rows = self.hip.gate_rows
        listed = act["channels"][:rows]
        audio, info = self.model.step(listed, act["waveout"][:rows])
        self.lists.append(listed.tolist())
        self.selected.append(act["channels"].tolist())
        self.infos.append(info)
        return act, listed, audio, info

    def step(self, what=""):
        what = "%s %s batch %d" % (what, self.fmt, len(self.lists))
        act, listed, audio, info = self.reference_step(what)
        enc = self.hip.collect_active_encoded()
        assert enc["n_active"] == act["n_active"], (what, enc["n_active"], act["n_active"])
        assert enc["channels"].tolist() == listed.tolist(), what
        assert np.array_equal(enc["axcindicate"], act["axcindicate"]), what
        assert enc["audio"].dtype == audio.dtype and enc["audio"].shape == audio.shape == (len(listed), self.hip.B // 2), (what, enc["audio"].dtype, enc["audio"].shape)
        assert enc["audio"].tobytes() == audio.tobytes(), what + ": decimated rows"
        assert enc["info"].tobytes() == info.tobytes(), (what + ": records", enc["info"][:4].tolist(), info[:4].tolist())
        return enc

    def left_and_came_back(self, among=None):
        """channels that were listed, then not, then listed again (among: per batch the channels that count as "not listed" there, default every other one)"""
        out = []
        for c in range(self.hip.total_channels):
            on = [c in l for l in self.lists]
            gone = [not o and (among is None or c in among[b]) for b, o in enumerate(on)]
            if any(on[a] and gone[b] and on[d] for a in range(len(on)) for b in range(a + 1, len(on)) for d in range(b + 1, len(on))):
                out.append(c)
        return out

    def loud(self):
        return int(sum((i["peak"] > 0).sum() for i in self.infos))


def _pattern_pair(pkg, names, gate, fmt, n_batches, max_rows=None):
    devices = gg._devices(len(names))
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        pair = Pair(pkg, hip, twin, fmt, np.asarray(gate, np.uint8), max_rows)
        bins = gg._pattern_inputs(names, hip.B)
        for b in range(n_batches):
            for h in (hip, twin):
                h.process_bins(*bins[b % og.N_BATCHES])
            pair.step("%d channels" % len(names))
    return pair


def _stream(pkg, hip, twin, devices, iq, n_batches, pipelined, step, switch=None):
    """Raw I/Q through the host-ring path of both handles (tests/test_gpu_gate.py's _run_stream, for two handles); switch = {k: (dongle, enabled)}"""
    g = hip.geometry
    off = 0
    for k in range(n_batches):
        take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
        lo = off if k == 0 else off + g.lookahead_bytes
        for h in (hip, twin):
            if switch and k in switch:
                h.device_enable(*switch[k])
            for d in range(len(devices)):
                if switch and k in switch and switch[k] == (d, True):
                    assert h.submit(d, iq[d][off:lo + take]) == lo + take - off
                else:
                    assert h.submit(d, iq[d][lo:lo + take]) == take
            assert h.process()
        off += g.first_batch_bytes if k == 0 else g.batch_bytes
        if pipelined and k == 0:
            assert hip.L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == pkg.capi.EAGAIN  # results lag one batch
        if not pipelined or k > 0:
            step()
    if pipelined:
        for h in (hip, twin):
            h.flush()
        step()


def _stream_pair(pkg, n_dev, n_batches, flags, gate, wave_rate, fmt, switch=None):
    devices, iq = gg._stream_case(pkg, wave_rate, n_dev, n_batches)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags) as twin:
        pair = Pair(pkg, hip, twin, fmt, gate)
        _stream(pkg, hip, twin, devices, iq, n_batches, bool(flags & pkg.capi.FLAG_PIPELINE), lambda: pair.step("wave rate %d, flags %#x" % (wave_rate, flags)), switch)
        assert len(pair.lists) == n_batches
        pair.B = hip.B
    return pair


# ---- 1: twin handles ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave_rate", [16000, 8000])
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_twin_handles_in_the_default_schedule(pkg, built, fmt, wave_rate):
    """Three dongles of the BASELINE plan, 24 channels, submit / process: 2 000 -> 1 000 at WAVE_RATE 16000 (AM, NFM, NFM + CTCSS, NFM + lowpass), 1 000 -> 500 at 8000."""
    pair = _stream_pair(pkg, 3, N_BATCHES, 0, gg._mixed_gate(24), wave_rate, fmt)
    assert pair.B == wave_rate // 8 and pair.loud() > 0
    assert any(c in pair.lists[b] and c in pair.lists[b + 1] for b in range(N_BATCHES - 1) for c in range(24)), "no history was ever carried"


def test_twin_handles_pipelined(pkg, built):
    pair = _stream_pair(pkg, 3, N_BATCHES, pkg.capi.FLAG_PIPELINE, gg._mixed_gate(24), 16000, "ulaw")
    assert pair.B == 2000 and pair.loud() > 0


def test_twin_handles_on_a_caller_stream(pkg, built):
    """process_device on a caller's stream: the collect orders itself behind it."""
    torch = pytest.importorskip("torch")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = 3
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip, pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as twin:
        pair = Pair(pkg, hip, twin, "alaw", gg._mixed_gate(8 * n))
        hip.set_signal_plan(carriers)
        g = hip.geometry
        span = g.first_batch_bytes + (N_BATCHES - 1) * g.batch_bytes + g.lookahead_bytes
        stride = (span + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        hip.generate_iq(buf.data_ptr(), stride, 0, span, stream=s.cuda_stream)
        for b in range(N_BATCHES):
            off = 0 if b == 0 else g.first_batch_bytes + (b - 1) * g.batch_bytes
            for h in (hip, twin):
                h.process_device(buf.data_ptr() + off, stride, stream=s.cuda_stream)
            pair.step("caller stream")
        s.synchronize()
        del buf
    assert pair.loud() > 0


# ---- 2: the history rule --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["s16", "ulaw"])
def test_channels_dropped_past_max_rows_and_keyed_off_restart_from_zeros(pkg, built, fmt):
    """24 AM channels on the squelch patterns, twice over, a list of six: a channel that is selected but dropped past max_rows and listed again later, and a
    channel whose signal is keyed off and on, both restart from a zero history; the channels listed throughout a transmission carry theirs."""
    names = ["k_and_k2", "two_long", "late", "quiet"] * 6
    gate = np.full(24, SIGNAL, np.uint8)
    gate[2] = ALWAYS
    pair = _pattern_pair(pkg, names, gate, fmt, n_batches=12, max_rows=6)
    assert any(len(s) > 6 for s in pair.selected), "the list never overflowed"
    dropped = [[c for c in s if c not in l] for s, l in zip(pair.selected, pair.lists)]
    assert pair.left_and_came_back(among=dropped), "no channel was dropped past max_rows and listed again"
    unselected = [[c for c in range(24) if c not in s] for s in pair.selected]
    assert pair.left_and_came_back(among=unselected), "no channel was keyed off and on"
    assert all(2 in l for l in pair.lists) and pair.loud() > 0  # the ALWAYS channel: one uninterrupted convolution


def test_dongle_switched_off_and_on(pkg, built):
    """The ALWAYS channel of a dongle that is switched off for two batches is not listed meanwhile and comes back from zeros."""
    gate = np.full(16, SIGNAL, np.uint8)
    gate[0] = gate[9] = ALWAYS
    pair = _stream_pair(pkg, 2, 6, 0, gate, 8000, "alaw", switch={2: (0, False), 4: (0, True)})
    assert [0 in l for l in pair.lists] == [True, True, False, False, True, True]
    assert all(9 in l for l in pair.lists) and pair.loud() > 0


# ---- 3: decimate_audio() --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extremes():
    rows = np.concatenate([ac.extremes_rows(1000), dc.saturating_rows(4, 1000)])
    hist = np.random.default_rng(12).integers(-32767, 32768, (len(rows), H)).astype("<i2")
    return rows, hist, {fmt: ac.capi.audio_decimate_reference(rows, fmt, hist) for fmt in ac.FORMATS}


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_decimate_audio_on_extremes(pkg, built, extremes, fmt):
    """Every q, full scale and beyond, the infinities, NaN, denormals, -0.0, the ties and the pattern that drives the filter into its clamp: 71 rows of 1 000
    behind a random history; then 0, 1 and 5 rows, a NULL history, and the calls that are refused."""
    rows, hist, want = extremes
    assert rows.shape == (71, 1000)
    with pkg.AirbandHip(gg._devices(8), wave_rate=8000) as hip:
        audio, info, out = hip.decimate_audio(rows, fmt, hist)
        assert audio.shape == (71, 500) and audio.tobytes() == want[fmt][0].tobytes(), "decimated rows"
        assert info.tobytes() == want[fmt][1].tobytes(), (info[-4:].tolist(), want[fmt][1][-4:].tolist())
        assert out.tobytes() == want[fmt][2].tobytes(), "history"
        assert info["n_clipped"].sum() >= 10 and (info["peak"][-4:] == 32767).all() and info["channel"].tolist() == list(range(71))
        for n in (1, 5):
            a, i, o = hip.decimate_audio(rows[66:66 + n], fmt)  # no history: zeros in
            w = pkg.capi.audio_decimate_reference(rows[66:66 + n], fmt)
            assert a.tobytes() == w[0].tobytes() and i.tobytes() == w[1].tobytes() and o.tobytes() == w[2].tobytes(), n
        L, capi, enc = hip.L, pkg.capi, pkg.capi.AUDIO_ENCODINGS[fmt]
        a = np.full((2, 500), 0x5A, audio.dtype)
        assert L.airband_hip_decimate_audio(hip.h, enc, rows.ctypes.data, 0, None, a.ctypes.data, None) == capi.OK and (a == 0x5A).all()
        assert L.airband_hip_decimate_audio(hip.h, enc, rows[69:].ctypes.data, 2, None, a.ctypes.data, None) == capi.OK  # NULL history, NULL records
        assert a.tobytes() == pkg.capi.audio_decimate_reference(rows[69:], fmt)[0].tobytes()
        assert L.airband_hip_decimate_audio(hip.h, enc, None, 1, None, None, None) == capi.EINVAL
        assert L.airband_hip_decimate_audio(hip.h, enc, rows.ctypes.data, -1, None, None, None) == capi.EINVAL
        assert L.airband_hip_decimate_audio(None, enc, rows.ctypes.data, 1, None, None, None) == capi.EINVAL
        for bad in (capi.AUDIO_F32, 4, -1):
            assert L.airband_hip_decimate_audio(hip.h, bad, rows.ctypes.data, 1, None, None, None) == capi.EINVAL


def test_decimate_audio_chained_through_history_at_2000_samples(pkg, built):
    """Two calls chained through `history` equal one pass over the joined rows."""
    joined = ac.random_rows(9, 4000, seed=16) + (np.sin(np.arange(4000) * 0.05) * 0.3).astype(np.float32)
    chans, _ = pkg.siggen.baseline_plan(mixed=True)
    with pkg.AirbandHip([dict(channels=chans)], wave_rate=16000) as hip:
        assert hip.B == 2000
        for fmt in ac.FORMATS:
            a0, i0, h0 = hip.decimate_audio(joined[:, :2000], fmt)
            a1, i1, h1 = hip.decimate_audio(joined[:, 2000:], fmt, h0)
            want, _, want_hist = pkg.capi.audio_decimate_reference(joined, fmt)
            assert np.concatenate([a0, a1], axis=1).tobytes() == want.tobytes() and h1.tobytes() == want_hist.tobytes(), fmt
            first = pkg.capi.audio_decimate_reference(joined[:, :2000], fmt)
            assert i0.tobytes() == first[1].tobytes() and i1.tobytes() == pkg.capi.audio_decimate_reference(joined[:, 2000:], fmt, first[2])[1].tobytes()


# ---- 4: downstream --------------------------------------------------------------------------------------------------------------------------------------
def test_spool_and_rtp_stream_on_half_length_rows(pkg, built):
    """A transmission spool and an RTP stream on a decimating mu-law handle at WAVE_RATE 16000, F = 160: rows of 1 000, 6.25 packets per row, payload type 0.
    Both references are fed the model's decimated rows; a third handle spools the same run at full rate: twice the audio bytes."""
    capi = pkg.capi
    n_batches = 6
    gate = gg._mixed_gate(24)
    devices, iq = gg._stream_case(pkg, 16000, 3, n_batches)
    spool = dict(pool_rows=160, export_rows=160, max_records=24, min_batches=1, idle_batches=1, max_batches=16)
    with pkg.AirbandHip(devices, wave_rate=16000) as hip, pkg.AirbandHip(devices, wave_rate=16000) as twin:
        pair = Pair(pkg, hip, twin, "ulaw", gate)
        twin.set_output_encoding("ulaw")
        twin.set_transmission_spool(**spool)  # the same run at full rate
        hip.set_transmission_spool(**spool)
        hip.set_rtp_stream(160)
        r = hip.rtp
        assert hip.B == 2000 and r["frame_samples"] == 160 and r["slot_bytes"] == 176 and (r["sources"]["payload_type"] == 0).all()
        spool_model = capi.transmission_spool_reference(gate == SIGNAL, 1000, **spool)
        rtp_model = capi.rtp_stream_reference(r["sources"], "ulaw", 1000, 160, r["max_packets"])
        packets = []

        def step():
            what = "batch %d" % len(pair.lists)
            act, listed, audio, info = pair.reference_step(what)
            spool_model.step(act["n_active"], listed, audio, info)
            want = rtp_model.step(listed, audio, ())
            got = hip.collect_rtp_packets()
            rc.compare_packets(what, got["n_packets"], got["records"], got["packets"], want)
            assert hip.collect_rtp_state().tobytes() == rtp_model.state().tobytes(), what
            packets.append(got)

        _stream(pkg, hip, twin, devices, iq, n_batches, False, step)
        assert hip.rtp_counters() == rtp_model.counters()
        recs = np.concatenate([p["records"] for p in packets])
        per_row = [int((p["records"]["channel"] == 2).sum()) for p in packets]  # the ALWAYS channel: rows of 1 000 in frames of 160
        assert per_row[:4] == [6, 6, 6, 7] and len(recs) > 0
        ts = [int(p["records"]["timestamp"][p["records"]["channel"] == 2][0]) for p in packets]
        assert ts[:3] == [0, 960, 1920]  # ts0 + k * 1000 - carry
        for h in (hip, twin):
            h.spool_flush()
        spool_model.flush()
        g, w, full = hip.collect_transmissions(), spool_model.collect(), twin.collect_transmissions()
        assert len(g["records"]) == len(w["records"]) > 0 and g["n_waiting"] == w["n_waiting"] == 0
        assert g["records"].tobytes() == w["records"].tobytes()
        assert g["audio"].shape == (w["n_rows"], 1000) and g["audio"].tobytes() == w["audio"]
        assert hip.spool_counters() == spool_model.counters()
        assert full["records"]["n_rows"].tolist() == g["records"]["n_rows"].tolist() and full["audio"].shape == (w["n_rows"], 2000)
        assert g["audio"].nbytes * 2 == full["audio"].nbytes > 0


# ---- 5: nothing changed without it ----------------------------------------------------------------------------------------------------------------------
def test_handles_without_a_decimation_return_the_same_bytes(pkg, built):
    """set_output_decimation(None) after set_output_decimation(2), and never calling it: both deliver what the full-rate encoder delivers."""
    names = ["k_and_k2", "two_long", "late"] * 8
    gate = np.full(24, SIGNAL, np.uint8)
    devices = gg._devices(24)
    with pkg.AirbandHip(devices, wave_rate=8000) as removed, pkg.AirbandHip(devices, wave_rate=8000) as never, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        for h in (removed, never, twin):
            h.set_output_gate(gate)
        for h in (removed, never):
            h.set_output_encoding("ulaw")
        removed.set_output_decimation(2)
        assert removed.encoded_row_samples() == 500
        removed.set_output_decimation(None)
        assert removed.encoded_row_samples() == never.encoded_row_samples() == 1000
        bins = gg._pattern_inputs(names, never.B)
        rows = 0
        for b in range(4):
            for h in (removed, never, twin):
                h.process_bins(*bins[b])
            a = removed.collect_active_encoded()
            _, e = ae._check_pair(pkg, never, twin, "ulaw", "batch %d" % b)
            assert a["n_active"] == e["n_active"] and a["channels"].tolist() == e["channels"].tolist()
            assert a["audio"].shape == e["audio"].shape and a["audio"].tobytes() == e["audio"].tobytes() and a["info"].tobytes() == e["info"].tobytes()
            rows += len(e["channels"])
        assert rows > 0


# ---- 6: the validation errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    names = ["k_and_k2", "late"] * 8
    devices = gg._devices(16)
    gate = np.full(16, SIGNAL, np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        L = hip.L
        bins = gg._pattern_inputs(names, hip.B)
        assert L.airband_hip_set_output_decimation(None, 2) == capi.EINVAL and L.airband_hip_encoded_row_samples(None) == capi.EINVAL
        assert L.airband_hip_set_output_decimation(hip.h, 2) == capi.EINVAL  # no gate
        assert L.airband_hip_encoded_row_samples(hip.h) == capi.EINVAL
        for h in (hip, twin):
            h.set_output_gate(gate)
        assert L.airband_hip_set_output_decimation(hip.h, 2) == capi.EINVAL  # a gate, no encoding
        assert L.airband_hip_set_output_decimation(hip.h, 1) == capi.EINVAL
        assert L.airband_hip_encoded_row_samples(hip.h) == capi.EINVAL
        hip.set_output_encoding("s16")
        for bad in (0, 3, 4, -1, -2, 1 << 20):
            assert L.airband_hip_set_output_decimation(hip.h, bad) == capi.EINVAL, bad
            assert hip.encoded_row_samples() == 1000
        hip.set_output_decimation(2)
        hip.set_output_encoding("s16")  # the encoding set again drops the decimation
        assert hip.encoded_row_samples() == 1000
        hip.set_output_decimation(2)
        hip.set_output_gate(gate)  # ... and so does the gate
        assert L.airband_hip_encoded_row_samples(hip.h) == capi.EINVAL
        hip.set_output_encoding("s16")
        hip.set_transmission_spool(32, max_batches=8)
        hip.set_rtp_stream(160)
        hip.set_output_decimation(2)  # setting it drops the spool and the stream
        assert L.airband_hip_collect_transmissions(hip.h, None, None, None, None, None) == capi.EINVAL
        assert L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:  # the frame must fit the half-length row
            hip.set_rtp_stream(504)
        assert e.value.code == capi.EBADSIZE
        hip.set_output_decimation(2)  # again: replaces the setting
        model = dc.Model(16, "s16")
        for b in range(4):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            if b == 0:
                for f in (1, 2):
                    assert L.airband_hip_set_output_decimation(hip.h, f) == capi.EINVAL  # a batch has been enqueued
            act, enc = twin.collect_active(), hip.collect_active_encoded()
            audio, info = model.step(act["channels"], act["waveout"])
            assert enc["channels"].tolist() == act["channels"].tolist() and enc["audio"].tobytes() == audio.tobytes() and enc["info"].tobytes() == info.tobytes(), b
        assert hip.encoded_row_samples() == 500
