"""RTP packet stream on the GPU (airband_hip_set_rtp_stream / _collect_rtp_packets / _collect_rtp_state / _rtp_counters_get / _device_rtp_stream,
csrc/rtp_stream.hip).

Every comparison is byte for byte: the definition is integers only.  A handle with a stream runs beside a twin that has gate and encoding only, on the same
input; per batch the handle's count, records, slots[:length], state and counters must equal capi.rtp_stream_reference stepped with the twin's
collect_active_encoded(), and everything else the two handles return must be the same bits.  No packet is excluded from a comparison."""
import ctypes as C

import numpy as np
import pytest

import helpers
import rtp_cases as rc
import test_gpu_audio_encoding as ae
import test_gpu_gate as gg
import test_output_gate as og

pytestmark = pytest.mark.gpu

NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
N_BATCHES = 6
FORMATS = ("ulaw", "alaw", "s16")


class Pair:
    """the handle with a stream, its twin (gate and encoding only, a list as long as the fleet) and the reference; step() checks the batch that is ready on both"""

    def __init__(self, pkg, hip, twin, fmt, gate, F=None, max_rows=None, max_packets=None, sources=None):
        self.pkg, self.hip, self.twin, self.fmt = pkg, hip, twin, fmt
        hip.set_output_gate(gate, max_rows)
        twin.set_output_gate(gate)
        for h in (hip, twin):
            h.set_output_encoding(fmt)
        hip.set_rtp_stream(F, sources, max_packets)
        r = hip.rtp
        self.model = pkg.capi.rtp_stream_reference(r["sources"], fmt, hip.B, r["frame_samples"], r["max_packets"])
        self.seen = []  # per batch (count, records, state)
        self.k = 0

    def reference_step(self):
        """the twin's batch into the reference: (the twin's collect, (count, records, slots))"""
        rows = self.hip.gate_rows
        t = self.twin.collect_active_encoded()
        return t, self.model.step(t["channels"][:rows], t["audio"][:rows], t["channels"][rows:])

    def step(self, what=""):
        what = "%s %s batch %d" % (what, self.fmt, self.k)
        hip, twin = self.hip, self.twin
        ae._same_full(ae._full(hip), ae._full(twin), what)
        t, want = self.reference_step()
        got = hip.collect_rtp_packets()
        assert np.array_equal(got["axcindicate"], t["axcindicate"]), what
        rc.compare_packets(what, got["n_packets"], got["records"], got["packets"], want)
        state = hip.collect_rtp_state()
        assert state.tobytes() == self.model.state().tobytes(), "%s: state differs at channels %r" % (what, np.flatnonzero(state != self.model.state())[:8])
        assert hip.rtp_counters() == self.model.counters(), (what, hip.rtp_counters(), self.model.counters())
        self.seen.append((got["n_packets"], got["records"].copy(), state))
        self.k += 1
        return got

    def flags(self):
        return np.concatenate([s[1]["flags"] for s in self.seen])

    def carries(self, c):
        return [int(s[2]["carry"][c]) for s in self.seen]


def _pattern_pair(pkg, names, gate, fmt, n_batches=N_BATCHES, **kw):
    devices = gg._devices(len(names))
    gate = np.asarray(gate, np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        pair = Pair(pkg, hip, twin, fmt, gate, **kw)
        bins = gg._pattern_inputs(names, hip.B)
        for b in range(n_batches):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            pair.step("%d channels" % len(names))
    return pair


def _stream_pair(pkg, devices, iq, n_batches, flags, gate, wave_rate, fmt, switch=None, **kw):
    """Raw I/Q through the host-ring path of both handles (tests/test_gpu_gate.py's _run_stream, for two handles); switch = {k: (dongle, enabled)}"""
    capi = pkg.capi
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags) as twin:
        pair = Pair(pkg, hip, twin, fmt, gate, **kw)
        g = hip.geometry
        pipelined = bool(flags & capi.FLAG_PIPELINE)
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
                assert hip.L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EAGAIN  # results lag one batch
            if not pipelined or k > 0:
                pair.step("wave rate %d, flags %#x" % (wave_rate, flags))
        if pipelined:
            for h in (hip, twin):
                h.flush()
            pair.step("flushed")
    assert len(pair.seen) == n_batches
    return pair


# ---- agreement with the reference -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_squelch_schedule_with_signal_and_always_gates(pkg, built, fmt):
    """Three dongles of eight AM channels on the squelch patterns and a quiet one, gates mixing SIGNAL and ALWAYS, F = 160, process_bins."""
    names = (["k_and_k2", "two_long", "late"] * 8)[:23] + ["quiet"]
    gate = [ALWAYS if c % 5 == 2 else SIGNAL for c in range(24)]
    pair = _pattern_pair(pkg, names, gate, fmt)
    flags = pair.flags()
    assert (flags & pkg.capi.RTP_MARKER).any(), "no marker packet"
    assert (flags & pkg.capi.RTP_FLUSH).any(), "no flush packet"
    assert pair.carries(2)[:4] == [40, 80, 120, 0], "no full carry cycle"
    assert all(int(s[2]["packets"][23]) == 0 for s in pair.seen)  # the quiet channel never sent


@pytest.mark.parametrize("n_ch", [1, 64, 65])
def test_channel_counts_across_a_wavefront_boundary(pkg, built, n_ch):
    names = [og.PATTERN_NAMES[(c * 7 + c // 64) % 4] for c in range(n_ch)]
    gate = [(NEVER, SIGNAL, ALWAYS, SIGNAL, SIGNAL)[c % 5] for c in range(n_ch)]
    if n_ch == 1:
        names, gate = ["two_long"], [SIGNAL]  # delivered in batches 1, 2, 3: a carry of 120 samples is left for batch 4 to flush
    pair = _pattern_pair(pkg, names, gate, "ulaw", n_batches=6)
    assert sum(s[0] for s in pair.seen) > 0
    if n_ch == 1:
        assert pair.seen[0][0] == 0, "a batch with zero packets"  # nothing is selected before the first signal
        assert (pair.flags() & pkg.capi.RTP_FLUSH).any()
    else:
        assert any(len(s[1]) and s[1]["channel"][-1] >= n_ch - 2 for s in pair.seen), "the last wavefront's channels never appeared"
        assert not pair.hip.rtp["sources"]["stream"][0] and pair.hip.rtp["sources"]["stream"][1]  # the default sources leave the NEVER channels out


def test_mixed_am_nfm_at_16000(pkg, built):
    """Three dongles of the BASELINE plan at WAVE_RATE 16000 (rows of 2 000 samples), the default frame of 320 samples, S16, submit / process."""
    devices, iq = gg._stream_case(pkg, 16000, 3, N_BATCHES)
    pair = _stream_pair(pkg, devices, iq, N_BATCHES, 0, gg._mixed_gate(24), 16000, "s16")
    assert pair.hip.B == 2000 and pair.hip.rtp["frame_samples"] == 320 and pair.hip.rtp["slot_bytes"] == 656
    assert pair.carries(2)[:4] == [80, 160, 240, 0]
    assert sum(s[0] for s in pair.seen) > 0


def test_pipelined_handle(pkg, built):
    devices, iq = gg._stream_case(pkg, 8000, 2, N_BATCHES)
    pair = _stream_pair(pkg, devices, iq, N_BATCHES, pkg.capi.FLAG_PIPELINE, gg._mixed_gate(16), 8000, "alaw")
    assert pair.carries(2)[:4] == [40, 80, 120, 0]


def test_dongle_switched_off_flushes_in_that_batch(pkg, built):
    """The switch-off applies with the next process call: the ALWAYS channel's carry of 120 samples goes out as a flush packet in that very batch."""
    devices, iq = gg._stream_case(pkg, 8000, 2, 7)
    gate = np.full(16, SIGNAL, np.uint8)
    gate[0] = gate[9] = ALWAYS
    pair = _stream_pair(pkg, devices, iq, 7, 0, gate, 8000, "ulaw", switch={3: (0, False), 5: (0, True)})
    recs = pair.seen[3][1]
    mine = recs[recs["channel"] == 0]
    assert len(mine) == 1 and mine[0]["flags"] == pkg.capi.RTP_FLUSH and mine[0]["length"] == 12 + 120
    assert pair.carries(0)[:5] == [40, 80, 120, 0, 0]
    back = pair.seen[5][1]
    assert back[back["channel"] == 0][0]["flags"] == pkg.capi.RTP_MARKER  # back on: a new talkspurt


def test_max_rows_smaller_than_the_active_count(pkg, built):
    n_ch, rows = 65, 5
    names = ["k_and_k2", "two_long", "late"] * 21 + ["late", "late"]
    gate = np.full(n_ch, SIGNAL, np.uint8)
    gate[2] = NEVER
    gate[0] = ALWAYS
    pair = _pattern_pair(pkg, names, gate, "ulaw", n_batches=5, max_rows=rows)
    assert pair.model.counters()["lost_rows"] > 0
    assert (pair.flags() & pkg.capi.RTP_FLUSH).any()  # a channel listed in one batch and dropped past max_rows in the next is flushed


def test_max_packets_smaller_than_the_packet_count(pkg, built):
    """The caller's arrays are larger than the capacity and poisoned: nothing past the packets kept may be touched; seq advances for the dropped ones."""
    n_ch, cap = 24, 10
    names = ["k_and_k2", "two_long", "late"] * 8
    gate = np.full(n_ch, SIGNAL, np.uint8)
    gate[3] = ALWAYS
    devices = gg._devices(n_ch)
    capi = pkg.capi
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        pair = Pair(pkg, hip, twin, "s16", gate, F=160, max_packets=cap)
        slot = hip.rtp["slot_bytes"]
        assert slot == 336
        bins = gg._pattern_inputs(names, hip.B)
        over = 0
        for b in range(5):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            t, (count, w_records, w_slots) = pair.reference_step()
            records = np.full((cap + 3) * 4, 0x5A5A5A5A, np.uint32).view(capi.RTP_PACKET_DTYPE)
            packets = np.full((cap + 3, slot), 0x5A, np.uint8)
            cnt = C.c_int64(-1)
            assert hip.L.airband_hip_collect_rtp_packets(hip.h, C.byref(cnt), records.ctypes.data, packets.ctypes.data, None) == 0
            n = min(count, cap)
            over += count > cap
            rc.compare_packets("batch %d" % b, int(cnt.value), records[:n], packets[:n], (count, w_records, w_slots))
            assert (records[n:].view(np.uint32) == 0x5A5A5A5A).all() and (packets[n:] == 0x5A).all(), "memory past the kept packets was written"
            assert hip.collect_rtp_state().tobytes() == pair.model.state().tobytes(), b
            assert hip.rtp_counters() == pair.model.counters(), b
        assert over >= 2 and pair.model.counters()["dropped_packets"] > 0  # the overflow did happen


def test_device_views_match_the_collect(pkg, built):
    torch = pytest.importorskip("torch")
    names = ["k_and_k2", "two_long", "late", "quiet"] * 5
    n = len(names)
    gate = np.array([SIGNAL, SIGNAL, ALWAYS, SIGNAL] * 5, np.uint8)
    devices = gg._devices(n)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        pair = Pair(pkg, hip, twin, "ulaw", gate)
        cap, slot = hip.rtp["max_packets"], hip.rtp["slot_bytes"]
        bins = gg._pattern_inputs(names, hip.B)
        for b in range(4):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            got = pair.step("views")
            k = len(got["records"])
            v = hip.device_rtp_stream()
            assert all(v.values())
            count = torch.as_tensor(pkg.DevicePtr(v["n_packets"], (1,), "<i4"), device="cuda").cpu().numpy()
            records = torch.as_tensor(pkg.DevicePtr(v["records"], (cap, 16), "|u1"), device="cuda").cpu().numpy()
            packets = torch.as_tensor(pkg.DevicePtr(v["packets"], (cap, slot), "|u1"), device="cuda").cpu().numpy()
            state = torch.as_tensor(pkg.DevicePtr(v["state"], (n, 16), "|u1"), device="cuda").cpu().numpy()
            assert int(count[0]) == got["n_packets"]
            assert records[:k].tobytes() == got["records"].tobytes() and packets[:k].tobytes() == got["packets"].tobytes()
            assert state.tobytes() == pair.seen[-1][2].tobytes()


def test_errors_leave_a_working_handle(pkg, built):
    capi = pkg.capi
    n = 16
    names = ["k_and_k2", "late"] * 8
    devices = gg._devices(n)
    ok = np.full(n, SIGNAL, np.uint8)
    ok[5] = NEVER
    src = np.zeros(n, capi.RTP_SOURCE_DTYPE)
    src["stream"] = 1
    src["stream"][5] = 0
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        L = hip.L
        bins = gg._pattern_inputs(names, hip.B)
        assert L.airband_hip_set_rtp_stream(hip.h, src.ctypes.data, 160, 100) == capi.EINVAL  # no gate
        for h in (hip, twin):
            h.set_output_gate(ok)
        assert L.airband_hip_set_rtp_stream(hip.h, src.ctypes.data, 160, 100) == capi.EINVAL  # no encoding
        for h in (hip, twin):
            h.set_output_encoding("s16")
        for F in (36, 162, 1004, 732):  # below 40, no multiple of 4, above wave_batch, 12 + 2 F above 1472
            assert L.airband_hip_set_rtp_stream(hip.h, src.ctypes.data, F, 100) == capi.EBADSIZE, F
        assert L.airband_hip_set_rtp_stream(hip.h, src.ctypes.data, 160, 0) == capi.EINVAL
        bad = src.copy()
        bad["payload_type"][1] = 128
        assert L.airband_hip_set_rtp_stream(hip.h, bad.ctypes.data, 160, 100) == capi.EINVAL
        bad = src.copy()
        bad["stream"][5] = 1  # gate NEVER
        assert L.airband_hip_set_rtp_stream(hip.h, bad.ctypes.data, 160, 100) == capi.EINVAL
        for call in (hip.collect_rtp_packets, hip.collect_rtp_state, hip.rtp_counters, hip.device_rtp_stream):
            with pytest.raises(pkg.AirbandError) as e:  # nothing of that set a stream
                call()
            assert e.value.code == capi.EINVAL
        hip.set_rtp_stream(160, src, 100)
        hip.set_rtp_stream(remove=True)
        assert L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EINVAL
        for b in range(3):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            if b == 0:
                assert L.airband_hip_set_rtp_stream(hip.h, src.ctypes.data, 160, 100) == capi.EINVAL  # a batch has been enqueued
            ae._same_full(ae._full(hip), ae._full(twin), "batch %d" % b)
            a, t = hip.collect_active_encoded(), twin.collect_active_encoded()
            assert a["channels"].tolist() == t["channels"].tolist() and a["audio"].tobytes() == t["audio"].tobytes() and a["info"].tobytes() == t["info"].tobytes()
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        pair = Pair(pkg, hip, twin, "ulaw", ok, F=40)
        hip.set_rtp_stream(160, src, 100)  # replaced before the first batch
        pair.model = capi.rtp_stream_reference(src, "ulaw", hip.B, 160, 100)
        assert hip.L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EAGAIN  # nothing to collect yet
        for b in range(4):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            if b % 2:
                # the gate and the encoding of a handle with a stream still agree with the twin's; the stream's step ran all the same
                ae._same_full(ae._full(hip), ae._full(twin), "batch %d" % b)
                a = hip.collect_active_encoded()
                t, _ = pair.reference_step()
                assert a["n_active"] == t["n_active"] and a["channels"].tolist() == t["channels"].tolist()
                assert a["audio"].tobytes() == t["audio"].tobytes() and a["info"].tobytes() == t["info"].tobytes()
                assert hip.collect_rtp_state().tobytes() == pair.model.state().tobytes()
                pair.k += 1
            else:
                pair.step("replaced stream")
            assert hip.L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EAGAIN  # the batch is collected
    with pkg.AirbandHip(devices, wave_rate=8000) as hip:
        hip.set_output_gate(ok)
        hip.set_output_encoding("ulaw")
        hip.set_rtp_stream()
        hip.set_output_encoding("alaw")  # a new encoding drops the stream
        hip.process_bins(*bins[0])
        assert hip.L.airband_hip_collect_rtp_packets(hip.h, None, None, None, None) == capi.EINVAL
        assert hip.collect_active_encoded()["n_active"] == 0


# ---- a handle without a stream launches nothing new ------------------------------------------------------------------------------------------------------
def test_handle_without_a_stream_launches_no_rtp_kernel(pkg, built):
    streamed = helpers.traced_kernels("rtp_stream_profile.py", ["--rtp", "160"], [("demod_kernel", "back_kernel")])
    for k in ("rtp_count_kernel", "rtp_scan_kernel", "rtp_write_kernel", "audio_pack_ulaw_kernel"):
        assert k in streamed, k  # the check below is not vacuous
    plain = helpers.traced_kernels("rtp_stream_profile.py", ["--rtp", "none"], [("demod_kernel", "back_kernel")])
    assert "audio_pack_ulaw_kernel" in plain and "rtp_" not in plain
