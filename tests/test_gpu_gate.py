"""Signal-gated collect on the GPU (airband_hip_set_output_gate / _collect_active / _device_active, csrc/gate.hip).

Every comparison is bit for bit: the packed rows are copies.  Per batch, on ONE gated handle, collect_channels (does not consume) gives every row and
axcindicate; collect_active must then return exactly the channels tests/test_output_gate.py::expected_active selects from the axcindicate history, in
ascending order, and their rows.  A twin handle without a gate, fed the same input, must return the same full rows."""
import os

import ctypes as C
import numpy as np
import pytest

import helpers
import test_output_gate as og

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
SPACE = ord(" ")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_batch(hip, gate, hist, en_hist=None, what=""):
    """collect_channels, then collect_active, of the batch that is ready; appends its axcindicate to hist.  Returns (full, active, expected channels)."""
    n = hip.total_channels
    full = hip.collect(iq=True, first_channel=0, n_channels=n)
    act = hip.collect_active(iq=True)
    hist.append(full["axc"].copy())
    want = og.expected_active(gate, hist, en_hist[:len(hist)] if en_hist is not None else None)[-1]
    where = "%s batch %d" % (what, len(hist) - 1)
    assert act["n_active"] == len(want), (where, act["n_active"], want)
    kept = want[:hip.gate_rows]
    assert act["channels"].tolist() == kept, (where, act["channels"].tolist(), kept)
    assert np.array_equal(_bits(act["waveout"]), _bits(full["waveout"][kept])), where + ": waveout rows"
    assert np.array_equal(_bits(act["iq_out"]), _bits(full["iq_out"][kept])), where + ": iq_out rows"
    assert np.array_equal(act["axcindicate"], full["axc"]), where + ": axc_all"
    return full, act, want


def _same_rows(a, b, what):
    assert np.array_equal(_bits(a["waveout"]), _bits(b["waveout"])), what + ": waveout"
    assert np.array_equal(_bits(a["iq_out"]), _bits(b["iq_out"])), what + ": iq_out"
    assert np.array_equal(a["axc"], b["axc"]), what + ": axc"


def _devices(n_ch, iq_every=0):
    chans = [og.channel(c % 8, has_iq_outputs=1 if iq_every and c % iq_every == 0 else 0) for c in range(n_ch)]
    return [dict(channels=chans[c:c + 8]) for c in range(0, n_ch, 8)]


def _pattern_inputs(names, B):
    """per batch (wavein [C][B], iq_in [C][2 B]) for channels following the named patterns"""
    per = {n: og.pattern_bins(n, B) for n in set(names)}
    return [(np.stack([per[n][b][0] for n in names]), np.stack([per[n][b][1] for n in names])) for b in range(og.N_BATCHES)]


def _run_patterns(pkg, names, gate, max_rows=None, iq_every=0, twin=True, flags=0):
    """The patterns through process_bins on a gated handle (and an ungated twin).  Returns (axc history, expected per batch, active results per batch)."""
    n = len(names)
    devices = _devices(n, iq_every)
    gate = np.asarray(gate, np.uint8)
    hist, wants, acts = [], [], []
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip, pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as plain:
        hip.set_output_gate(gate, max_rows)
        bins = _pattern_inputs(names, hip.B)
        for b in range(og.N_BATCHES):
            hip.process_bins(*bins[b])
            full, act, want = _check_batch(hip, gate, hist, what="%d channels" % n)
            wants.append(want)
            acts.append(act)
            if twin:
                plain.process_bins(*bins[b])
                _same_rows(full, plain.collect(iq=True), "ungated twin, batch %d" % b)
    intended = og.intended_axc(names)
    for b in range(og.N_BATCHES):  # the stage-2 inputs did what the CPU oracle said they would (test_output_gate.py)
        assert bytes(hist[b]) == bytes(intended[b]), b
    return hist, wants, acts


def test_squelch_schedule_every_signal_channel(pkg, built):
    """24 SIGNAL channels, every third with a raw-I/Q output, none quiet throughout: the run holds every situation the rule distinguishes."""
    names = ["k_and_k2", "two_long", "late"] * 8
    n = len(names)
    hist, wants, acts = _run_patterns(pkg, names, [SIGNAL] * n, iq_every=3)
    assert any(len(w) == 0 for w in wants), "no batch without an active channel"
    assert wants[0] == [] and acts[0]["n_active"] == 0 and acts[0]["waveout"].shape == (0, 1000)
    assert any(w == list(range(n)) for w in wants), "no batch with every SIGNAL channel active"
    trailing = [(b, c) for b, w in enumerate(wants) for c in w if hist[b][c] == SPACE]
    assert trailing, "no row delivered only because of the batch before"
    assert all(hist[b - 1][c] != SPACE for b, c in trailing)
    c = names.index("k_and_k2")
    k = 1
    assert c in wants[k] and c in wants[k + 2] and hist[k][c] != SPACE and hist[k + 2][c] != SPACE
    assert all(c not in w for w in wants[k + 4:]) and len(wants) > k + 4, "delivered in a later quiet batch"
    assert any(a["iq_out"].any() for a in acts), "no raw-I/Q row with content was packed"


@pytest.mark.parametrize("n_ch", [1, 63, 64, 65, 257])
def test_sizes_across_wavefront_boundaries_with_mixed_gates(pkg, built, n_ch):
    names = [og.PATTERN_NAMES[(c * 7 + c // 64) % 4] for c in range(n_ch)]
    gate = [(NEVER, SIGNAL, ALWAYS, SIGNAL, SIGNAL)[c % 5] for c in range(n_ch)]
    if n_ch == 1:
        names, gate = ["k_and_k2"], [SIGNAL]
    hist, wants, acts = _run_patterns(pkg, names, gate, iq_every=5 if n_ch > 1 else 0)
    assert any(wants), "nothing was ever delivered"
    never = {c for c in range(n_ch) if gate[c] == NEVER}
    always = [c for c in range(n_ch) if gate[c] == ALWAYS]
    for w in wants:
        assert not never & set(w) and set(always) <= set(w)
    if n_ch >= 63:
        assert any(w and w[-1] >= n_ch - 2 for w in wants), "the last wavefront's channels never appeared"


def test_large_handle_active_channels_in_first_middle_and_last_block(pkg, built):
    """5 120 channels = five workgroups of the select pass; most quiet, a few per cent active, gates mixed."""
    n_ch = 5120
    rng = np.random.default_rng(42)
    names = [og.PATTERN_NAMES[i] for i in rng.choice(4, n_ch, p=[0.05, 0.04, 0.87, 0.04])]  # sorted names: k_and_k2, late, quiet, two_long
    gate = rng.choice([NEVER, SIGNAL, ALWAYS], n_ch, p=[0.2, 0.77, 0.03]).astype(np.uint8)
    for c in (0, 1023, 1024, 2600, 4096, 5119):
        names[c], gate[c] = "k_and_k2", SIGNAL
    hist, wants, acts = _run_patterns(pkg, names, gate, twin=False)
    w = wants[3]
    assert {0, 1023, 1024, 2600, 4096, 5119} <= set(w)
    blocks = {c // 1024 for c in w if gate[c] == SIGNAL}
    assert blocks == {0, 1, 2, 3, 4}, blocks
    assert 0 < len(wants[0]) < len(w) < n_ch // 2  # the first batch: the ALWAYS channels alone


def test_max_rows_smaller_than_the_active_count(pkg, built):
    n_ch, rows = 65, 5
    names = ["k_and_k2", "two_long", "late"] * 21 + ["late", "late"]
    gate = np.full(n_ch, SIGNAL, np.uint8)
    gate[2] = NEVER
    devices = _devices(n_ch, iq_every=4)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_output_gate(gate, rows)
        B = hip.B
        bins = _pattern_inputs(names, B)
        hist = []
        for b in range(4):
            hip.process_bins(*bins[b])
            full = hip.collect(iq=True, first_channel=0, n_channels=n_ch)
            hist.append(full["axc"].copy())
            want = og.expected_active(gate, hist)[-1]
            # caller's arrays larger than the capacity and poisoned: nothing past the rows kept may be touched
            idx = np.full(rows + 3, -77, np.int32)
            wave = np.full((rows + 3, B), np.float32(-1234.5))
            iqo = np.full((rows + 3, 2 * B), np.float32(-1234.5))
            axc = np.zeros(n_ch, np.uint8)
            cnt = C.c_int64(-1)
            assert hip.L.airband_hip_collect_active(hip.h, C.byref(cnt), idx.ctypes.data, wave.ctypes.data, iqo.ctypes.data, axc.ctypes.data) == 0
            kept = want[:rows]
            assert cnt.value == len(want), (b, cnt.value, want)
            assert idx[:len(kept)].tolist() == kept and (idx[len(kept):] == -77).all(), (b, idx)
            assert np.array_equal(_bits(wave[:len(kept)]), _bits(full["waveout"][kept]))
            assert np.array_equal(_bits(iqo[:len(kept)]), _bits(full["iq_out"][kept]))
            assert (wave[len(kept):] == np.float32(-1234.5)).all() and (iqo[len(kept):] == np.float32(-1234.5)).all(), "memory past the kept rows was written"
            assert np.array_equal(axc, full["axc"])
        assert len(og.expected_active(gate, hist)[3]) == n_ch - 1 > rows  # the overflow did happen, and NEVER stayed out


def test_device_views_match_collect_active(pkg, built):
    torch = pytest.importorskip("torch")
    names = ["k_and_k2", "two_long", "late", "quiet"] * 5
    n = len(names)
    gate = np.array([SIGNAL, SIGNAL, ALWAYS, SIGNAL] * 5, np.uint8)
    with pkg.AirbandHip(_devices(n, iq_every=2), wave_rate=8000) as hip:
        hip.set_output_gate(gate)
        bins = _pattern_inputs(names, hip.B)
        hist = []
        for b in range(4):
            hip.process_bins(*bins[b])
            _, act, want = _check_batch(hip, gate, hist)
            v = hip.device_active()
            assert v["index"] and v["count"] and v["rows"] and v["iq_rows"]
            k = len(want)
            cnt = torch.as_tensor(pkg.DevicePtr(v["count"], (1,), "<i4"), device="cuda").cpu().numpy()
            assert cnt[0] == k
            idx = torch.as_tensor(pkg.DevicePtr(v["index"], (n,), "<i4"), device="cuda").cpu().numpy()
            rows = torch.as_tensor(pkg.DevicePtr(v["rows"], (n, hip.B), "<f4"), device="cuda").cpu().numpy()
            iqr = torch.as_tensor(pkg.DevicePtr(v["iq_rows"], (n, 2 * hip.B), "<f4"), device="cuda").cpu().numpy()
            assert idx[:k].tolist() == act["channels"].tolist()
            assert np.array_equal(_bits(rows[:k]), _bits(act["waveout"])) and np.array_equal(_bits(iqr[:k]), _bits(act["iq_out"]))
    with pkg.AirbandHip(_devices(8), wave_rate=8000) as hip:  # no raw-I/Q outputs: no packed I/Q rows
        hip.set_output_gate(np.full(8, SIGNAL, np.uint8))
        assert hip.device_active()["iq_rows"] == 0 and hip.device_active()["rows"]


def test_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    n = 16
    names = ["k_and_k2", "late"] * 8
    devices = _devices(n)
    ok = np.full(n, SIGNAL, np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        bins = _pattern_inputs(names, hip.B)
        L = hip.L
        bad = ok.copy()
        bad[7] = 3
        assert L.airband_hip_set_output_gate(hip.h, bad.ctypes.data, n) == capi.EINVAL
        assert L.airband_hip_set_output_gate(hip.h, None, n) == capi.EINVAL
        assert L.airband_hip_set_output_gate(hip.h, ok.ctypes.data, 0) == capi.EINVAL
        assert L.airband_hip_set_output_gate(hip.h, ok.ctypes.data, n + 1) == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:  # no gate
            hip.collect_active()
        assert e.value.code == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:
            hip.device_active()
        assert e.value.code == capi.EINVAL
        hip.process_bins(*bins[0])
        with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
            hip.set_output_gate(ok)
        assert e.value.code == capi.EINVAL
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_active()
        assert e.value.code == capi.EINVAL
        first = hip.collect(iq=True)
        hip.process_bins(*bins[1])
        second = hip.collect(iq=True)
    with pkg.AirbandHip(devices, wave_rate=8000) as plain:  # ... and the handle ran on as one that was never asked
        plain.process_bins(*bins[0])
        _same_rows(first, plain.collect(iq=True), "batch 0")
        plain.process_bins(*bins[1])
        _same_rows(second, plain.collect(iq=True), "batch 1")
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_output_gate(bad.clip(0, 2), 3)
        hip.set_output_gate(ok, n)  # replaced before the first batch
        assert hip.L.airband_hip_collect_active(hip.h, None, None, None, None, None) == capi.EAGAIN  # nothing to collect yet
        hip.process_bins(*bins[0])
        hip.process_bins(*bins[1])
        hist = [np.frombuffer(bytes(og.intended_axc(names)[0]), np.uint8)]
        _check_batch(hip, ok, hist)
        assert hip.L.airband_hip_collect_active(hip.h, None, None, None, None, None) == capi.EAGAIN  # the batch is collected
        assert hip.collect(iq=True, first_channel=0, n_channels=n)["axc"].tolist() == hist[1].tolist()  # collect_channels still serves it


# ---- launch paths: the real front half ----------------------------------------------------------------------------------------------------------------
def _run_stream(pkg, devices, iq, n_batches, flags, gate, wave_rate, scan=None, sched=None, switch=None, what=""):
    """Raw I/Q through the host-ring path of a gated handle.  sched[k]: scan entry of device 0 for batch k; switch = {k: (dongle, enabled)} applied
    before batch k is enqueued.  Returns (axc history, expected per batch, full rows per batch)."""
    capi = pkg.capi
    n_dev = len(devices)
    first = np.cumsum([0] + [len(d["channels"]) for d in devices])
    hist, wants, fulls, en_hist = [], [], [], []
    on = np.ones(first[-1], bool)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as hip:
        if gate is not None:
            hip.set_output_gate(gate)
        g = hip.geometry
        pipelined = bool(flags & capi.FLAG_PIPELINE)
        off = 0

        def grab():
            if gate is None:
                fulls.append(hip.collect(iq=True))
                return
            full, act, want = _check_batch(hip, gate, hist, en_hist if switch else None, what)
            fulls.append(full)
            wants.append(want)

        for k in range(n_batches):
            if switch and k in switch:
                d, enabled = switch[k]
                hip.device_enable(d, enabled)
                on[first[d]:first[d + 1]] = enabled
            en_hist.append(on.copy())
            take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
            lo = off if k == 0 else off + g.lookahead_bytes
            for d in range(n_dev):
                if switch and k in switch and switch[k] == (d, True):  # a dongle that comes back joins at the common stream position with an empty queue
                    assert hip.submit(d, iq[d][off:lo + take]) == lo + take - off
                else:
                    assert hip.submit(d, iq[d][lo:lo + take]) == take
            off += g.first_batch_bytes if k == 0 else g.batch_bytes
            if sched is not None:
                hip.set_freq_index(0, sched[k])
            assert hip.process()
            if gate is not None and pipelined and k == 0:
                assert hip.L.airband_hip_collect_active(hip.h, None, None, None, None, None) == capi.EAGAIN  # results lag one batch
            if not pipelined or k > 0:
                grab()
        if pipelined:
            hip.flush()
            grab()  # flush() delivers the last batch
    assert len(fulls) == n_batches
    return hist, wants, fulls


def _stream_case(pkg, wave_rate, n_dev, n_batches):
    devices, iq = helpers.format_case(pkg, pkg.capi.SFMT_U8, 9, 2_560_000, wave_rate, n_dev, n_batches)
    return devices, [np.ascontiguousarray(x).view(np.uint8) for x in iq]


def _mixed_gate(n):
    gate = np.full(n, SIGNAL, np.uint8)
    gate[1::8] = NEVER
    gate[2::8] = ALWAYS
    return gate


def _has_trailing(gate, hist, wants):
    return any(gate[c] == SIGNAL and hist[b][c] == SPACE for b, w in enumerate(wants) for c in w)


@pytest.mark.parametrize("wave_rate,flag_names", [(8000, ()), (16000, ()), (16000, ("FLAG_REGROUP",)), (16000, ("FLAG_NO_REGROUP",)),
                                                  (16000, ("FLAG_PIPELINE", "FLAG_NO_REGROUP")), (8000, ("FLAG_PIPELINE",))])
def test_submit_process_paths(pkg, built, wave_rate, flag_names):
    """submit / process on the BASELINE plan (WAVE_RATE 16000: AM, NFM, NFM + CTCSS and NFM + lowpass channels), sequential, regrouped and pipelined."""
    flags = 0
    for f in flag_names:
        flags |= getattr(pkg.capi, f)
    n_batches = 9
    devices, iq = _stream_case(pkg, wave_rate, 2, n_batches)
    if wave_rate == 16000:
        assert any(c["ctcss_freq"] for c in devices[0]["channels"]) and any(c["modulation"] == 1 for c in devices[0]["channels"])
    gate = _mixed_gate(16)
    hist, wants, fulls = _run_stream(pkg, devices, iq, n_batches, flags, gate, wave_rate, what=str(flag_names))
    _, _, plain = _run_stream(pkg, devices, iq, n_batches, flags, None, wave_rate)
    for b in range(n_batches):
        _same_rows(fulls[b], plain[b], "ungated twin, batch %d" % b)
    counts = [len(w) for w in wants]
    assert min(counts) < max(counts) and max(counts) <= 14, counts  # the squelches do open and close; NEVER stays out
    assert _has_trailing(gate, hist, wants), "no trailing batch in the run"


def test_process_device_on_a_caller_stream(pkg, built):
    torch = pytest.importorskip("torch")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_batches = 4, 6
    gate = _mixed_gate(8 * n)
    hist, wants = [], []
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        hip.set_output_gate(gate)
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
            _, _, want = _check_batch(hip, gate, hist, what="caller stream")  # collect_active orders itself behind the caller's stream
            wants.append(want)
        s.synchronize()
        del buf
    assert any(gate[c] == SIGNAL for w in wants for c in w), "no SIGNAL channel was ever active"


def test_afc_indicators_count_as_signal(pkg, built):
    devices, carriers = helpers.afc_case(1)
    n_batches = 8
    nbytes = helpers.stream_bytes(n_batches, 8000) + 64
    iq = [pkg.siggen.generate_u8(0, 0, nbytes // 2, carriers)]
    gate = np.full(8, SIGNAL, np.uint8)
    hist, wants, _ = _run_stream(pkg, devices, iq, n_batches, 0, gate, 8000, what="afc")
    moved = [(b, c) for b in range(n_batches) for c in range(8) if hist[b][c] in (ord("<"), ord(">"))]
    assert moved, "no channel reported '<' or '>'"
    for b, c in moved:
        assert c in wants[b]
        if b + 1 < n_batches:
            assert c in wants[b + 1]  # ... and '<' / '>' leaves a trailing batch like '*'


def test_scan_handle_switching_entries(pkg, built):
    n_batches = 9
    devices, iq = _stream_case(pkg, 8000, 1, n_batches)
    ch0 = devices[0]["channels"][0]
    rest = {k: v for k, v in devices[0].items() if k != "channels"}
    devs = [dict(rest, channels=[ch0]), devices[0]]
    scan = {0: [ch0, dict(ch0, squelch_snr_threshold_db=14.0, ampfactor=0.5), dict(ch0, notch_freq=1000.0)]}
    sched = [0, 1, 1, 2, 0, 2, 1, 0, 0]
    gate = np.full(9, SIGNAL, np.uint8)
    gate[4] = ALWAYS
    hist, wants, fulls = _run_stream(pkg, devs, [iq[0], iq[0]], n_batches, 0, gate, 8000, scan=scan, sched=sched, what="scan")
    _, _, plain = _run_stream(pkg, devs, [iq[0], iq[0]], n_batches, 0, None, 8000, scan=scan, sched=sched)
    for b in range(n_batches):
        _same_rows(fulls[b], plain[b], "ungated twin, batch %d" % b)
    assert any(0 in w for w in wants) and any(0 not in w for w in wants), "the scan channel was always / never delivered"


def test_dongle_switched_off_and_back(pkg, built):
    """The switch-off takes effect with the next process call: from that batch on none of the dongle's rows is delivered, whatever the gate."""
    n_batches = 9
    devices, iq = _stream_case(pkg, 8000, 2, n_batches)
    gate = np.full(16, SIGNAL, np.uint8)
    gate[0] = gate[9] = ALWAYS
    hist, wants, _ = _run_stream(pkg, devices, iq, n_batches, 0, gate, 8000, switch={3: (0, False), 6: (0, True)}, what="switch")
    for b in range(n_batches):
        if b in (3, 4, 5):
            assert not [c for c in wants[b] if c < 8], (b, wants[b])  # not even the ALWAYS channel
            assert (hist[b][:8] == SPACE).all()
        else:
            assert 0 in wants[b]
        assert 9 in wants[b]


# ---- a handle without a gate launches nothing new -------------------------------------------------------------------------------------------------------
def _traced_kernels(extra):
    return helpers.traced_kernels("gated_collect_profile.py", extra, [("demod_kernel", "back_kernel")])


def test_ungated_handle_launches_no_gate_kernel(pkg, built):
    gated = _traced_kernels([])
    for k in ("gate_select_kernel", "gate_index_kernel", "gate_gather_kernel"):
        assert k in gated, k  # the check below is not vacuous
    plain = _traced_kernels(["--no-gate"])
    assert "gate_" not in plain
