"""Encoded audio collect on the GPU (airband_hip_set_output_encoding / _collect_active_encoded / _device_active_encoded / _encode_audio, csrc/audio_pack.hip).

Every comparison is byte for byte: behind the one float32 multiplication the definition is integer arithmetic.  A handle with an encoding and a twin without
one are fed the same input; per batch the encoded rows and records must equal capi.audio_encode_reference() of the float rows the twin's collect_active()
delivers, the count and the list must be the twin's, and everything else the two handles return must be the same bits.  encode_audio() is how the GPU meets
the inputs a demodulator never produces: clipping, NaN, the infinities, ties."""
import os

import ctypes as C
import numpy as np
import pytest

import audio_cases as ac
import helpers
import test_gpu_gate as gg
import test_output_gate as og

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
N_BATCHES = 6


def _full(hip):
    """every channel's row, axcindicate and stats of the batch that is ready, without consuming it"""
    return hip.collect(stats=True, first_channel=0, n_channels=hip.total_channels)


def _same_full(a, b, what):
    assert np.array_equal(gg._bits(a["waveout"]), gg._bits(b["waveout"])), what + ": waveout"
    assert np.array_equal(a["axc"], b["axc"]), what + ": axc"
    assert repr(a["stats"]) == repr(b["stats"]), what + ": stats"


def _check_pair(pkg, hip, twin, fmt, what):
    """The batch that is ready on both handles.  Returns (the twin's collect_active(), the handle's collect_active_encoded())."""
    _same_full(_full(hip), _full(twin), what)
    act = twin.collect_active()
    enc = hip.collect_active_encoded()
    assert enc["n_active"] == act["n_active"], (what, enc["n_active"], act["n_active"])
    assert enc["channels"].tolist() == act["channels"].tolist(), what
    assert np.array_equal(enc["axcindicate"], act["axcindicate"]), what
    audio, info = pkg.capi.audio_encode_reference(act["waveout"], fmt)
    info["channel"] = act["channels"]
    assert enc["audio"].dtype == audio.dtype and enc["audio"].shape == audio.shape, (what, enc["audio"].dtype, enc["audio"].shape)
    assert enc["audio"].tobytes() == audio.tobytes(), what + ": encoded rows"
    assert enc["info"].tobytes() == info.tobytes(), (what + ": records", enc["info"][:4].tolist(), info[:4].tolist())
    return act, enc


def _seen(encs, B):
    """what the run exercised: (rows delivered, rows with audio, rows that are silent or partly silent)"""
    info = np.concatenate([e["info"] for e in encs]) if encs else np.zeros(0, ac.capi.AUDIO_ROW_DTYPE)
    return len(info), int((info["peak"] > 0).sum()), int(((info["first"] > 0) | (info["end"] < B)).sum())


def _run_patterns(pkg, names, gate, fmt, n_batches=N_BATCHES, max_rows=None):
    devices = gg._devices(len(names))
    gate = np.asarray(gate, np.uint8)
    acts, encs = [], []
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        for h in (hip, twin):
            h.set_output_gate(gate, max_rows)
        hip.set_output_encoding(fmt)
        bins = gg._pattern_inputs(names, hip.B)
        for b in range(n_batches):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            act, enc = _check_pair(pkg, hip, twin, fmt, "%s, %d channels, batch %d" % (fmt, len(names), b))
            acts.append(act)
            encs.append(enc)
        B = hip.B
    return acts, encs, B


def _run_stream(pkg, devices, iq, n_batches, flags, gate, wave_rate, fmt, scan=None, sched=None):
    """Raw I/Q through the host-ring path of a handle with an encoding and of its twin (tests/test_gpu_gate.py's _run_stream, for two handles)."""
    capi = pkg.capi
    acts, encs = [], []
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as twin:
        for h in (hip, twin):
            h.set_output_gate(gate)
        hip.set_output_encoding(fmt)
        g = hip.geometry
        pipelined = bool(flags & capi.FLAG_PIPELINE)
        off = 0

        def grab(k):
            act, enc = _check_pair(pkg, hip, twin, fmt, "%s, wave rate %d, flags %#x, batch %d" % (fmt, wave_rate, flags, k))
            acts.append(act)
            encs.append(enc)

        for k in range(n_batches):
            take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
            lo = off if k == 0 else off + g.lookahead_bytes
            for h in (hip, twin):
                for d in range(len(devices)):
                    assert h.submit(d, iq[d][lo:lo + take]) == take
                if sched is not None:
                    h.set_freq_index(0, sched[k])
                assert h.process()
            off += g.first_batch_bytes if k == 0 else g.batch_bytes
            if pipelined and k == 0:
                assert hip.L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EAGAIN  # results lag one batch
            if not pipelined or k > 0:
                grab(k - 1 if pipelined else k)
        if pipelined:
            for h in (hip, twin):
                h.flush()
            grab(n_batches - 1)
        B = hip.B
    assert len(encs) == n_batches
    return acts, encs, B


# ---- agreement with the float rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_squelch_schedule_at_8000(pkg, built, fmt):
    """Three dongles of eight AM channels on the squelch patterns: batches without a row, with every row, and trailing batches whose audio ends inside them."""
    names = ["k_and_k2", "two_long", "late"] * 8
    acts, encs, B = _run_patterns(pkg, names, [SIGNAL] * len(names), fmt)
    assert encs[0]["n_active"] == 0 and encs[0]["audio"].shape == (0, B) and len(encs[0]["info"]) == 0
    assert any(e["n_active"] == len(names) for e in encs)
    rows, loud, partial = _seen(encs, B)
    assert rows > 0 and loud > 0 and partial > 0, (rows, loud, partial)


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_mixed_am_nfm_at_16000(pkg, built, fmt):
    """Three dongles of the BASELINE plan at WAVE_RATE 16000 (AM, NFM, NFM + CTCSS, NFM + lowpass; rows of 2 000 samples), submit / process."""
    devices, iq = gg._stream_case(pkg, 16000, 3, N_BATCHES)
    assert any(c["modulation"] == 1 for c in devices[0]["channels"]) and any(c["modulation"] == 0 for c in devices[0]["channels"])
    acts, encs, B = _run_stream(pkg, devices, iq, N_BATCHES, 0, gg._mixed_gate(24), 16000, fmt)
    rows, loud, partial = _seen(encs, B)
    assert B == 2000 and rows > 0 and loud > 0, (B, rows, loud)


@pytest.mark.parametrize("n_ch", [1, 64, 65])
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_channel_counts_across_a_wavefront_boundary(pkg, built, fmt, n_ch):
    names = [og.PATTERN_NAMES[(c * 7 + c // 64) % 4] for c in range(n_ch)]
    gate = [(NEVER, SIGNAL, ALWAYS, SIGNAL, SIGNAL)[c % 5] for c in range(n_ch)]
    if n_ch == 1:
        names, gate = ["k_and_k2"], [SIGNAL]
    acts, encs, B = _run_patterns(pkg, names, gate, fmt, n_batches=5)
    assert _seen(encs, B)[1] > 0
    if n_ch > 1:
        assert any(len(e["channels"]) and e["channels"][-1] >= n_ch - 2 for e in encs), "the last wavefront's channels never appeared"


@pytest.mark.parametrize("fmt", ["s16", "alaw"])
def test_max_rows_smaller_than_the_active_count(pkg, built, fmt):
    n_ch, rows = 65, 5
    names = ["k_and_k2", "two_long", "late"] * 21 + ["late", "late"]
    gate = np.full(n_ch, SIGNAL, np.uint8)
    gate[2] = NEVER
    devices = gg._devices(n_ch)
    dt = np.dtype("<i2") if fmt == "s16" else np.dtype(np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_output_gate(gate, rows)
        hip.set_output_encoding(fmt)
        B = hip.B
        bins = gg._pattern_inputs(names, B)
        hist = []
        for b in range(4):
            hip.process_bins(*bins[b])
            full = hip.collect(first_channel=0, n_channels=n_ch)
            hist.append(full["axc"].copy())
            want = og.expected_active(gate, hist)[-1]
            kept = want[:rows]
            # the caller's arrays are larger than the capacity and poisoned: nothing past the rows kept may be touched
            idx = np.full(rows + 3, -77, np.int32)
            audio = np.full((rows + 3, B), 0x5A, dt)
            info = np.full(rows + 3, 0x5A5A5A5A, np.uint32).repeat(4).view(pkg.capi.AUDIO_ROW_DTYPE)
            poison = info[0].copy()
            axc = np.zeros(n_ch, np.uint8)
            cnt = C.c_int64(-1)
            assert hip.L.airband_hip_collect_active_encoded(hip.h, C.byref(cnt), idx.ctypes.data, audio.ctypes.data, info.ctypes.data, axc.ctypes.data) == 0
            assert cnt.value == len(want), (b, cnt.value, want)
            assert idx[:len(kept)].tolist() == kept and (idx[len(kept):] == -77).all(), (b, idx)
            ref_audio, ref_info = pkg.capi.audio_encode_reference(full["waveout"][kept].reshape(len(kept), B), fmt)
            ref_info["channel"] = kept
            assert audio[:len(kept)].tobytes() == ref_audio.tobytes() and info[:len(kept)].tobytes() == ref_info.tobytes(), b
            assert (audio[len(kept):] == 0x5A).all() and all(r == poison for r in info[len(kept):]), "memory past the kept rows was written"
            assert np.array_equal(axc, full["axc"])
        assert len(og.expected_active(gate, hist)[3]) == n_ch - 1 > rows  # the overflow did happen


# ---- encode_audio(): the inputs a demodulator never produces -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def extremes():
    rows = ac.extremes_rows(1000)
    return rows, {fmt: ac.capi.audio_encode_reference(rows, fmt) for fmt in ac.FORMATS}


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_encode_audio_on_extremes(pkg, built, extremes, fmt):
    """Every q in -32767 .. 32767, full scale and just beyond it, the infinities, NaN, denormals, -0.0 and exact ties: 67 rows of 1 000."""
    rows, want = extremes
    assert rows.shape == (67, 1000)
    with pkg.AirbandHip(gg._devices(8), wave_rate=8000) as hip:
        audio, info = hip.encode_audio(rows, fmt)
        assert audio.tobytes() == want[fmt][0].tobytes(), "encoded rows"
        assert info.tobytes() == want[fmt][1].tobytes(), (info[-2:].tolist(), want[fmt][1][-2:].tolist())
        assert info["n_clipped"].sum() >= 6 and info["channel"].tolist() == list(range(67))
        # a row count that is no multiple of anything, and the calls that do nothing or are refused
        few, few_info = hip.encode_audio(rows[64:], fmt)
        assert few.tobytes() == want[fmt][0][64:].tobytes() and few_info["channel"].tolist() == [0, 1, 2]
        L, capi, enc = hip.L, pkg.capi, pkg.capi.AUDIO_ENCODINGS[fmt]
        assert L.airband_hip_encode_audio(hip.h, enc, rows.ctypes.data, 0, None, None) == capi.OK
        assert L.airband_hip_encode_audio(hip.h, enc, rows.ctypes.data, 2, None, None) == capi.OK  # either output may be NULL
        assert L.airband_hip_encode_audio(hip.h, enc, None, 1, None, None) == capi.EINVAL
        assert L.airband_hip_encode_audio(hip.h, enc, rows.ctypes.data, -1, None, None) == capi.EINVAL
        for bad in (capi.AUDIO_F32, 4, -1):
            assert L.airband_hip_encode_audio(hip.h, bad, rows.ctypes.data, 1, None, None) == capi.EINVAL


def test_encode_audio_at_2000_samples(pkg, built):
    rows = ac.random_rows(9, 2000, seed=16)
    chans, _ = pkg.siggen.baseline_plan(mixed=True)
    with pkg.AirbandHip([dict(channels=chans)], wave_rate=16000) as hip:
        assert hip.B == 2000
        for fmt in ac.FORMATS:
            audio, info = hip.encode_audio(rows, fmt)
            want_audio, want_info = pkg.capi.audio_encode_reference(rows, fmt)
            assert audio.tobytes() == want_audio.tobytes() and info.tobytes() == want_info.tobytes(), fmt


# ---- device views, schedules, errors -------------------------------------------------------------------------------------------------------------------
def test_device_views_match_the_collect(pkg, built):
    torch = pytest.importorskip("torch")
    names = ["k_and_k2", "two_long", "late", "quiet"] * 5
    n = len(names)
    gate = np.array([SIGNAL, SIGNAL, ALWAYS, SIGNAL] * 5, np.uint8)
    devices = gg._devices(n)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        for h in (hip, twin):
            h.set_output_gate(gate)
        hip.set_output_encoding("ulaw")
        bins = gg._pattern_inputs(names, hip.B)
        for b in range(4):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            act, enc = _check_pair(pkg, hip, twin, "ulaw", "batch %d" % b)
            k = len(enc["channels"])
            v, f = hip.device_active_encoded(), hip.device_active()
            assert v["audio"] and v["info"]
            audio = torch.as_tensor(pkg.DevicePtr(v["audio"], (n, hip.B), "|u1"), device="cuda").cpu().numpy()
            info = torch.as_tensor(pkg.DevicePtr(v["info"], (n, 16), "|u1"), device="cuda").cpu().numpy()
            assert audio[:k].tobytes() == enc["audio"].tobytes() and info[:k].tobytes() == enc["info"].tobytes()
            rows = torch.as_tensor(pkg.DevicePtr(f["rows"], (n, hip.B), "<f4"), device="cuda").cpu().numpy()
            assert np.array_equal(gg._bits(rows[:k]), gg._bits(act["waveout"])), "the float rows are still packed"


def test_pipelined_handle(pkg, built):
    devices, iq = gg._stream_case(pkg, 8000, 2, N_BATCHES)
    acts, encs, B = _run_stream(pkg, devices, iq, N_BATCHES, pkg.capi.FLAG_PIPELINE, gg._mixed_gate(16), 8000, "s16")
    assert _seen(encs, B)[1] > 0


def test_scan_handle_switching_entries(pkg, built):
    devices, iq = gg._stream_case(pkg, 8000, 1, N_BATCHES)
    ch0 = devices[0]["channels"][0]
    rest = {k: v for k, v in devices[0].items() if k != "channels"}
    devs = [dict(rest, channels=[ch0]), devices[0]]
    scan = {0: [ch0, dict(ch0, squelch_snr_threshold_db=14.0, ampfactor=0.5), dict(ch0, notch_freq=1000.0)]}
    gate = np.full(9, SIGNAL, np.uint8)
    gate[0] = gate[4] = ALWAYS
    acts, encs, B = _run_stream(pkg, devs, [iq[0], iq[0]], N_BATCHES, 0, gate, 8000, "alaw", scan=scan, sched=[0, 1, 1, 2, 0, 2])
    assert all(0 in e["channels"].tolist() for e in encs) and _seen(encs, B)[1] > 0


def test_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    n = 16
    names = ["k_and_k2", "late"] * 8
    devices = gg._devices(n)
    ok = np.full(n, SIGNAL, np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        bins = gg._pattern_inputs(names, hip.B)
        L = hip.L
        assert L.airband_hip_set_output_encoding(hip.h, capi.AUDIO_S16) == capi.EINVAL  # no gate
        for h in (hip, twin):
            h.set_output_gate(ok)
        for bad in (4, -1, 255):
            assert L.airband_hip_set_output_encoding(hip.h, bad) == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:  # a gate, no encoding
            hip.collect_active_encoded()
        assert e.value.code == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:
            hip.device_active_encoded()
        assert e.value.code == capi.EINVAL
        hip.set_output_encoding("s16")
        hip.set_output_encoding(None)  # removed again
        assert L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EINVAL
        for b in range(3):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            if b == 0:
                with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
                    hip.set_output_encoding("ulaw")
                assert e.value.code == capi.EINVAL
                assert L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EINVAL
            gg._same_rows(hip.collect(iq=True, first_channel=0, n_channels=n), twin.collect(iq=True, first_channel=0, n_channels=n), "batch %d" % b)
            a, t = hip.collect_active(), twin.collect_active()
            assert a["channels"].tolist() == t["channels"].tolist() and np.array_equal(gg._bits(a["waveout"]), gg._bits(t["waveout"]))
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        for h in (hip, twin):
            h.set_output_gate(ok)
        hip.set_output_encoding("ulaw")
        hip.set_output_encoding("alaw")  # replaced before the first batch
        assert hip.L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EAGAIN  # nothing to collect yet
        for b in range(3):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            _check_pair(pkg, hip, twin, "alaw", "replaced encoding, batch %d" % b)
            assert hip.L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EAGAIN  # the batch is collected
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_output_gate(ok)
        hip.set_output_encoding("s16")
        hip.set_output_gate(ok, 4)  # a new gate drops the encoding
        hip.process_bins(*bins[0])
        assert hip.L.airband_hip_collect_active_encoded(hip.h, None, None, None, None, None) == capi.EINVAL
        with pytest.raises(pkg.AirbandError):
            hip.device_active_encoded()
        assert hip.collect_active()["n_active"] == 0


# ---- a handle without an encoding launches nothing new --------------------------------------------------------------------------------------------------
def _traced_kernels(extra):
    return helpers.traced_kernels("audio_encoding_profile.py", extra, [("demod_kernel", "back_kernel")])


def test_handle_without_an_encoding_launches_no_encode_kernel(pkg, built):
    encoded = _traced_kernels(["--encoding", "ulaw"])
    assert "audio_pack_ulaw_kernel" in encoded and "gate_gather_kernel" in encoded  # the check below is not vacuous
    plain = _traced_kernels(["--encoding", "none"])
    assert "gate_gather_kernel" in plain and "audio_pack" not in plain
