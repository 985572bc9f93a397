"""Gated mixer collect on the GPU (airband_hip_set_mixer_gate / _mixer_gate_step / _collect_active_mixers / _device_active_mixers / _encode_mixer_audio,
csrc/mixer_gate.hip).

Every comparison is byte for byte.  Stage 2 is driven through process_bins with the named squelch patterns of tests/test_output_gate.py, so each channel's signal
history is known; the expectation is always capi.mixer_gate_reference applied to what collect_mixers() of the SAME handle returned per batch, which keeps
these tests apart from stage-2 and mixer-sum parity (other tests' business)."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_cases as ac
import helpers
import test_output_gate as og

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
ENCODINGS = (None, "s16", "ulaw", "alaw")

# ---- the wiring of the rule tests: 72 channels (9 dongles x 8), channel c follows pattern NAMES[c % 4]; 7 mixers ---------------------------------------
N_CH = 72
NAMES = [og.PATTERN_NAMES[c % 4] for c in range(N_CH)]  # k_and_k2, late, quiet, two_long, ...
K2, LATE, QUIET, LONG = 0, 1, 2, 3                      # a channel of each pattern on dongle 0


def _inp(c, mixer, amp=1.0, balance=0.0):
    return (c // 8, c % 8, mixer, amp, balance)


WIRING = ([_inp(K2, 0, 0.8), _inp(QUIET, 0, 0.5)]                                    # 0: mono, two inputs
          + [_inp(LONG, 1, 1.0, 0.5), _inp(LATE, 1, 0.7, -0.5)]                      # 1: stereo by balance +-0.5
          + [_inp(LATE + 4, 2, 0.9)]                                                 # 2: stereo by mixer_set_stereo
          + [_inp(c, 3, 0.05) for c in range(N_CH)]                                  # 3: all 72 channels: two runs of 64 inputs
          + [_inp(QUIET, 5), _inp(QUIET + 4, 5)] + [_inp(QUIET + 8, 6)])             # 4: no inputs; 5, 6: quiet inputs only
N_MIX = 7
GATE = np.array([SIGNAL, SIGNAL, ALWAYS, SIGNAL, ALWAYS, SIGNAL, NEVER], np.uint8)
STEREO_FLAGS = np.array([0, 1, 1, 0, 0, 0, 0], np.uint8)
INPUTS_OF = {0: [K2, QUIET], 1: [LONG, LATE], 2: [LATE + 4], 3: list(range(N_CH)), 4: [], 5: [QUIET, QUIET + 4], 6: [QUIET + 8]}


def _intended_signal():
    """[N_BATCHES][N_MIX] has_signal the patterns are built to produce"""
    axc = og.intended_axc(NAMES)
    return [np.array([any(axc[b][c] != ord(" ") for c in INPUTS_OF[m]) for m in range(N_MIX)], np.uint8) for b in range(og.N_BATCHES)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _devices(n_ch):
    chans = [og.channel(c % 8) for c in range(n_ch)]
    return [dict(channels=chans[c:c + 8]) for c in range(0, n_ch, 8)]


def _pattern_inputs(names, B):
    per = {n: og.pattern_bins(n, B) for n in set(names)}
    return [(np.stack([per[n][b][0] for n in names]), np.stack([per[n][b][1] for n in names])) for b in range(og.N_BATCHES)]


def _wire(hip):
    hip.set_mixers(N_MIX, WIRING)
    hip.mixer_set_stereo(2, True)


def _check_step(hip, gate, max_rows, enc, stereo, hist, flags, where):
    """collect_mixers (appended to hist), then collect_active_mixers, against the reference over the whole history.  Returns (reference of this step, result)."""
    left, right, sig = hip.collect_mixers()
    hist.append((left, right, sig, flags))
    want = ac.capi.mixer_gate_reference(gate, max_rows, enc, stereo, hist)[-1]
    got = hip.collect_active_mixers()
    assert got["n_active"] == want["n_active"], (where, got["n_active"], want["n_active"])
    assert got["mixers"].tolist() == want["mixers"].tolist(), (where, got["mixers"].tolist(), want["mixers"].tolist())
    assert np.array_equal(got["has_signal"], sig), where + ": signal_all"
    if enc is None:
        assert got["rows"].dtype == np.float32 and got["rows"].tobytes() == want["rows"].tobytes(), where + ": float rows"
    else:
        assert got["audio"].dtype == want["rows"].dtype and got["audio"].tobytes() == want["rows"].tobytes(), where + ": encoded rows"
        assert got["info"].tobytes() == want["info"].tobytes(), (where, got["info"].tolist(), want["info"].tolist())
    return want, got


def test_the_run_holds_what_the_rule_distinguishes():
    """Conditions on the INPUTS (no GPU result enters): what tests 1 and 8 rely on, from the intended axcindicate of the patterns and the wiring."""
    sig = _intended_signal()
    batches = [(np.zeros((N_MIX, 4), np.float32),) * 2 + (s, STEREO_FLAGS) for s in sig]
    ref = ac.capi.mixer_gate_reference(GATE, N_MIX, None, False, batches)
    signal_mixers = [m for m in range(N_MIX) if GATE[m] == SIGNAL]
    assert not any(m in ref[0]["mixers"] for m in signal_mixers) and ref[0]["mixers"].tolist() == [2, 4]  # the first batch: no SIGNAL mixer
    assert any(m in ref[b]["mixers"] and not sig[b][m] for b in range(1, og.N_BATCHES) for m in signal_mixers), "no trailing batch"
    assert any(m not in ref[b]["mixers"] for b in range(1, og.N_BATCHES) for m in (0, 1, 3)), "no SIGNAL mixer left out after it had audio"
    assert all(5 not in r["mixers"] and 6 not in r["mixers"] for r in ref)
    assert sig[1][1] and sig[2][1]  # mixer 1 (balance +-0.5) has audio: left = 0.5 x, right = 1.0 x


@pytest.mark.parametrize("enc,stereo,wave_rate", [(e, st, 8000) for e in ENCODINGS for st in (False, True)] + [("ulaw", True, 16000)])
def test_rule_and_rows(pkg, built, enc, stereo, wave_rate):
    """1 and 8: the rule, the rows and the records in every encoding and width (WAVE_RATE 16000 once); an ungated twin returns the same collect() and
    collect_mixers() bits."""
    devices = _devices(N_CH)
    with pkg.AirbandHip(devices, wave_rate=wave_rate) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate) as plain:
        _wire(hip)
        _wire(plain)
        hip.set_mixer_gate(GATE, encoding=enc, stereo=stereo)
        bins = _pattern_inputs(NAMES, hip.B)
        hist, wants = [], []
        intended = _intended_signal()
        for b in range(og.N_BATCHES):
            hip.process_bins(*bins[b])
            plain.process_bins(*bins[b])
            want, got = _check_step(hip, GATE, N_MIX, enc, stereo, hist, STEREO_FLAGS, "batch %d" % b)
            wants.append(want)
            if wave_rate == 8000:
                assert hist[-1][2].tolist() == intended[b].tolist(), (b, hist[-1][2])
            pl, pr, ps = plain.collect_mixers()
            assert np.array_equal(_bits(pl), _bits(hist[-1][0])) and np.array_equal(_bits(pr), _bits(hist[-1][1])) and np.array_equal(ps, hist[-1][2]), "twin: mixers, batch %d" % b
            a, p = hip.collect(iq=True), plain.collect(iq=True)
            assert np.array_equal(_bits(a["waveout"]), _bits(p["waveout"])) and np.array_equal(a["axc"], p["axc"]), "twin: channels, batch %d" % b
        if wave_rate == 8000:
            assert any(m in w["mixers"] and not hist[b][2][m] for b, w in enumerate(wants) for m in (0, 1, 3)), "no trailing row in the run"
            assert wants[0]["mixers"].tolist() == [2, 4] and 0 not in wants[5]["mixers"]
            l, r = hist[1][0][1], hist[1][1][1]
            assert l.any() and r.any() and not np.array_equal(l, r), "mixer 1's right equals its left"
            if stereo:
                row = list(wants[1]["mixers"]).index(1)
                x = wants[1]["rows"][row]
                assert not np.array_equal(x[0::2], x[1::2])
                if enc is not None:
                    assert wants[1]["info"]["reserved"].tolist() == STEREO_FLAGS[wants[1]["mixers"]].tolist()


def test_max_rows_smaller_than_the_count(pkg, built):
    """2: five ALWAYS mixers and max_rows 3: counted 5, the first three listed, nothing written past row 3 of the caller's (larger, poisoned) arrays."""
    devices = _devices(8)
    names = ["k_and_k2", "late", "quiet", "two_long"] * 2
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_mixers(5, [(0, c, c % 5, 1.0, 0.5 if c % 2 else 0.0) for c in range(8)])
        hip.set_mixer_gate(np.full(5, ALWAYS, np.uint8), 3, "s16", stereo=True)
        B = hip.B
        bins = _pattern_inputs(names, B)
        for b in range(3):
            hip.process_bins(*bins[b])
            left, right, sig = hip.collect_mixers()
            want = ac.capi.mixer_gate_reference([ALWAYS] * 5, 3, "s16", True, [(left, right, sig, [1, 1, 1, 1, 0])])[0]  # stereo by balance: channels 1, 3, 5, 7 feed mixers 1, 3, 0, 2
            idx = np.full(6, -77, np.int32)
            audio = np.full((6, 2 * B), 0x5A5A, np.uint16)
            info = np.full(6 * 4, 0xA5A5A5A5, np.uint32)
            sig_all = np.zeros(5, np.uint8)
            cnt = C.c_int64(-1)
            assert hip.L.airband_hip_collect_active_mixers(hip.h, C.byref(cnt), idx.ctypes.data, None, audio.ctypes.data, info.ctypes.data, sig_all.ctypes.data) == 0
            assert cnt.value == 5 and idx[:3].tolist() == [0, 1, 2] and (idx[3:] == -77).all()
            assert audio[:3].tobytes() == want["rows"].tobytes() and info[:12].tobytes() == want["info"].tobytes()
            assert (audio[3:] == 0x5A5A).all() and (info[12:] == 0xA5A5A5A5).all(), "memory past the kept rows was written"
            assert np.array_equal(sig_all, sig)
        assert want["rows"].any()


def test_manual_step_behind_add_mixers(pkg, built):
    """3: two handles on one GPU; dst.add_mixers(src), then dst.mixer_gate_step(): the step sees the node's sums.  In the batches where only src has signal an
    automatic step would have looked at dst's partial sums: the reference on those differs."""
    capi = pkg.capi
    devices = _devices(8)
    src_names, dst_names = ["two_long"] + ["quiet"] * 7, ["late"] + ["quiet"] * 7
    wiring = [(0, 0, 0, 1.0, 0.5), (0, 1, 1, 1.0, 0.0)]
    gate = np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8)
    flags = [1, 0, 0]
    with pkg.AirbandHip(devices, wave_rate=8000) as src, pkg.AirbandHip(devices, wave_rate=8000) as dst:
        for h in (src, dst):
            h.set_mixers(3, wiring)
        dst.set_mixer_gate(gate, encoding="ulaw", stereo=True, manual_step=True)
        assert dst.L.airband_hip_collect_active_mixers(dst.h, None, None, None, None, None, None) == capi.EAGAIN  # no step yet
        sb, db = _pattern_inputs(src_names, src.B), _pattern_inputs(dst_names, dst.B)
        hist, partial, differed = [], [], []
        for b in range(og.N_BATCHES):
            src.process_bins(*sb[b])
            dst.process_bins(*db[b])
            if b == 0:
                assert dst.L.airband_hip_collect_active_mixers(dst.h, None, None, None, None, None, None) == capi.EAGAIN  # nothing is launched with the batch
            partial.append(dst.collect_mixers() + (flags,))
            dst.add_mixers(src)
            dst.mixer_gate_step()
            want, got = _check_step(dst, gate, 3, "ulaw", True, hist, flags, "manual, batch %d" % b)
            alone = capi.mixer_gate_reference(gate, 3, "ulaw", True, partial)[-1]
            if alone["mixers"].tolist() != want["mixers"].tolist() or alone["rows"].tobytes() != want["rows"].tobytes():
                differed.append(b)
            src.collect()
            dst.collect()
        only_src = [b for b in range(og.N_BATCHES) if hist[b][2][0] and not partial[b][2][0]]
        assert only_src and set(only_src) <= set(differed), (only_src, differed)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:  # an automatic gate refuses the manual step
        hip.set_mixers(3, wiring)
        hip.set_mixer_gate(gate)
        with pytest.raises(pkg.AirbandError) as e:
            hip.mixer_gate_step()
        assert e.value.code == capi.EINVAL


def _stream_mixers(hip):
    hip.set_mixers(3, [(0, c, 0, 0.5, 0.5 if c % 2 else -0.25) for c in range(8)] + [(1, c, 1, 0.7, 0.0) for c in range(4)])
    gate = np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8)
    hip.set_mixer_gate(gate, encoding="ulaw", stereo=True)
    return gate, [1, 0, 0]


@pytest.mark.parametrize("flag_names", [(), ("FLAG_PIPELINE",)])
def test_submit_process_schedules(pkg, built, flag_names):
    """4: the default run-ahead schedule and FLAG_PIPELINE (with flush()) through submit / process: W = 2, ulaw."""
    capi = pkg.capi
    flags = 0
    for f in flag_names:
        flags |= getattr(capi, f)
    n_batches = 6
    devices, iq = helpers.format_case(pkg, capi.SFMT_U8, 9, 2_560_000, 8000, 2, n_batches)
    iq = [np.ascontiguousarray(x).view(np.uint8) for x in iq]
    pipelined = bool(flags & capi.FLAG_PIPELINE)
    hist, wants = [], []
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        gate, sflags = _stream_mixers(hip)
        if not pipelined:
            assert hip.schedule_info()["run_ahead"], "the default schedule is not run-ahead here"
        g = hip.geometry
        off = 0
        for k in range(n_batches):
            take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
            lo = off if k == 0 else off + g.lookahead_bytes
            for d in range(2):
                assert hip.submit(d, iq[d][lo:lo + take]) == take
            off += g.first_batch_bytes if k == 0 else g.batch_bytes
            assert hip.process()
            if not pipelined or k > 0:
                wants.append(_check_step(hip, gate, 3, "ulaw", True, hist, sflags, "%s batch %d" % (flag_names, k))[0])
                hip.collect()
        if pipelined:
            hip.flush()
            wants.append(_check_step(hip, gate, 3, "ulaw", True, hist, sflags, "flush")[0])
    assert len(wants) == n_batches
    counts = [w["n_active"] for w in wants]
    assert min(counts) >= 1 and max(counts) >= 2, counts  # the ALWAYS mixer every batch, a SIGNAL mixer in some
    assert any(w["rows"].any() for w in wants)


def test_process_device_on_a_caller_stream(pkg, built):
    """4: batches on a caller's stream: the step runs there, the collect orders itself behind it."""
    torch = pytest.importorskip("torch")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_batches = 2, 5
    hist, wants = [], []
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        gate, sflags = _stream_mixers(hip)
        hip.set_signal_plan(carriers)
        g = hip.geometry
        span = g.first_batch_bytes + (n_batches - 1) * g.batch_bytes + g.lookahead_bytes
        stride = (span + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        hip.generate_iq(buf.data_ptr(), stride, 0, span, stream=s.cuda_stream)
        for b in range(n_batches):
            off = 0 if b == 0 else g.first_batch_bytes + (b - 1) * g.batch_bytes
            hip.process_device(buf.data_ptr() + off, stride, stream=s.cuda_stream)
            wants.append(_check_step(hip, gate, 3, "ulaw", True, hist, sflags, "caller stream, batch %d" % b)[0])
        s.synchronize()
        del buf
    assert any(w["n_active"] >= 2 for w in wants), "no SIGNAL mixer was ever active"


def test_device_views_match_the_collect(pkg, built):
    """5"""
    torch = pytest.importorskip("torch")
    devices = _devices(N_CH)
    for enc in (None, "s16"):
        with pkg.AirbandHip(devices, wave_rate=8000) as hip:
            _wire(hip)
            hip.set_mixer_gate(GATE, encoding=enc, stereo=True)
            bins = _pattern_inputs(NAMES, hip.B)
            hist = []
            for b in range(3):
                hip.process_bins(*bins[b])
                want, got = _check_step(hip, GATE, N_MIX, enc, True, hist, STEREO_FLAGS, "views")
            v = hip.device_active_mixers()
            assert v["index"] and v["count"] and bool(v["rows"]) == (enc is None) and bool(v["audio"]) == (enc is not None) and bool(v["info"]) == (enc is not None)
            k = len(want["mixers"])
            assert k >= 3
            assert torch.as_tensor(pkg.DevicePtr(v["count"], (1,), "<i4"), device="cuda").cpu().numpy()[0] == want["n_active"]
            assert torch.as_tensor(pkg.DevicePtr(v["index"], (N_MIX,), "<i4"), device="cuda").cpu().numpy()[:k].tolist() == want["mixers"].tolist()
            if enc is None:
                rows = torch.as_tensor(pkg.DevicePtr(v["rows"], (N_MIX, 2 * hip.B), "<f4"), device="cuda").cpu().numpy()
                assert rows[:k].tobytes() == got["rows"].tobytes()
            else:
                audio = torch.as_tensor(pkg.DevicePtr(v["audio"], (N_MIX, 2 * hip.B), "<i2"), device="cuda").cpu().numpy()
                info = torch.as_tensor(pkg.DevicePtr(v["info"], (N_MIX, 4), "<i4"), device="cuda").cpu().numpy()
                assert audio[:k].tobytes() == got["audio"].tobytes() and info[:k].tobytes() == got["info"].tobytes()


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_encode_mixer_audio_on_the_edge_rows(pkg, built, fmt):
    """6: mono equals encode_audio; stereo equals the reference; n_rows == 0 is OK."""
    capi = pkg.capi
    with pkg.AirbandHip(_devices(8), wave_rate=8000) as hip:
        x = ac.extremes_rows(hip.B)
        y = x[::-1].copy()
        audio, info = hip.encode_mixer_audio(x, None, fmt)
        a2, i2 = hip.encode_audio(x, fmt)
        assert audio.tobytes() == a2.tobytes() and info.tobytes() == i2.tobytes()
        audio, info = hip.encode_mixer_audio(x, y, fmt)
        want, winfo = capi.mixer_rows_reference(x, y, fmt, True, None, np.ones(len(x), np.uint8))
        assert audio.tobytes() == want.tobytes(), "stereo rows"
        assert info.tobytes() == winfo.tobytes(), (info[:3].tolist(), winfo[:3].tolist())
        assert info["n_clipped"].sum() >= 12 and (info["reserved"] == 1).all()
        L = hip.L
        assert L.airband_hip_encode_mixer_audio(hip.h, capi.AUDIO_ENCODINGS[fmt], x.ctypes.data, None, 0, None, None) == 0
        assert L.airband_hip_encode_mixer_audio(hip.h, capi.AUDIO_F32, x.ctypes.data, None, 1, None, None) == capi.EINVAL
        assert L.airband_hip_encode_mixer_audio(hip.h, capi.AUDIO_ENCODINGS[fmt], None, None, 1, None, None) == capi.EINVAL
        assert L.airband_hip_encode_mixer_audio(hip.h, capi.AUDIO_ENCODINGS[fmt], x.ctypes.data, None, -1, None, None) == capi.EINVAL


def test_errors_leave_a_working_handle(pkg, built):
    """7: every EINVAL of the definition (EBADSIZE needs a WAVE_BATCH that is no multiple of four: no handle has one, it is 1000 or 2000); set_mixers() again drops the gate; the gate can be set after batches have run, with an empty memory."""
    capi = pkg.capi
    devices = _devices(N_CH)
    ok = GATE.copy()
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as plain:
        L = hip.L
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, N_MIX, 0, 0) == capi.EINVAL  # no mixers
        assert L.airband_hip_set_mixer_gate(hip.h, None, 0, 0, 0) == capi.EINVAL
        assert L.airband_hip_mixer_gate_step(hip.h, None) == capi.EINVAL
        _wire(hip)
        _wire(plain)
        bad = ok.copy()
        bad[3] = 3
        assert L.airband_hip_set_mixer_gate(hip.h, bad.ctypes.data, N_MIX, 0, 0) == capi.EINVAL
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, 0, 0, 0) == capi.EINVAL
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, N_MIX + 1, 0, 0) == capi.EINVAL
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, N_MIX, 4, 0) == capi.EINVAL
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, N_MIX, -1, 0) == capi.EINVAL
        assert L.airband_hip_set_mixer_gate(hip.h, ok.ctypes.data, N_MIX, 0, 4) == capi.EINVAL
        for call in (hip.collect_active_mixers, hip.device_active_mixers, hip.mixer_gate_step):  # no gate
            with pytest.raises(pkg.AirbandError) as e:
                call()
            assert e.value.code == capi.EINVAL
        bins = _pattern_inputs(NAMES, hip.B)
        for b in range(2):  # ... and the handle ran on as one that was never asked
            hip.process_bins(*bins[b])
            plain.process_bins(*bins[b])
            for x, y in zip(hip.collect_mixers(), plain.collect_mixers()):
                assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)
            a, p = hip.collect(iq=True), plain.collect(iq=True)
            assert np.array_equal(_bits(a["waveout"]), _bits(p["waveout"])) and np.array_equal(a["axc"], p["axc"])
        # set after batches have run (batch 1 had signal on mixers 0, 1, 3): the memory starts empty, so batch 2 delivers no trailing row of mixer 1
        hip.set_mixer_gate(ok, encoding="alaw", stereo=True)
        assert L.airband_hip_collect_active_mixers(hip.h, None, None, None, None, None, None) == capi.EAGAIN
        rows = np.zeros((N_MIX, 2 * hip.B), np.float32)
        hist = []
        for b in range(2, 5):
            hip.process_bins(*bins[b])
            want, got = _check_step(hip, ok, N_MIX, "alaw", True, hist, STEREO_FLAGS, "late gate, batch %d" % b)
            assert L.airband_hip_collect_active_mixers(hip.h, None, None, rows.ctypes.data, None, None, None) == capi.EINVAL  # float rows of an encoded gate
            hip.collect()
        assert _intended_signal()[1][0] and 0 not in ac.capi.mixer_gate_reference(ok, N_MIX, "alaw", True, hist)[0]["mixers"]
        hip.set_mixer_gate(ok)  # replaced: a float gate refuses audio / info
        hip.process_bins(*bins[5])
        info = np.zeros(N_MIX, capi.AUDIO_ROW_DTYPE)
        assert L.airband_hip_collect_active_mixers(hip.h, None, None, None, rows.ctypes.data, None, None) == capi.EINVAL
        assert L.airband_hip_collect_active_mixers(hip.h, None, None, None, None, info.ctypes.data, None) == capi.EINVAL
        assert hip.collect_active_mixers()["rows"].shape[1] == hip.B
        hip.set_mixer_gate(None)  # removed
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_active_mixers()
        assert e.value.code == capi.EINVAL
        hip.set_mixer_gate(ok)
        _wire(hip)  # set_mixers() again drops the gate
        assert L.airband_hip_collect_active_mixers(hip.h, None, None, None, None, None, None) == capi.EINVAL
        hip.process_bins(*bins[6])
        assert hip.collect_mixers()[0].shape == (N_MIX, hip.B)


# ---- a handle without a mixer gate launches nothing new -------------------------------------------------------------------------------------------------
def _traced_kernels(extra):
    return helpers.traced_kernels("mixer_gate_profile.py", extra, ["mix_final_kernel"])


def test_handle_without_a_mixer_gate_launches_none_of_the_kernels(pkg, built):
    """8"""
    gated = _traced_kernels(["--encoding", "ulaw"])
    for k in ("mixer_gate_select_kernel", "mixer_gate_index_kernel", "mixer_pack_ulaw_stereo_kernel"):
        assert k in gated, k  # the check below is not vacuous
    plain = _traced_kernels(["--encoding", "off"])
    assert "mixer_gate_" not in plain and "mixer_pack_" not in plain
