"""Transmission spool on the GPU (airband_hip_set_transmission_spool / _collect_transmissions / _spool_flush / _spool_counters_get /
_device_transmission_spool, csrc/tx_spool.hip).

Every comparison is byte for byte: the definition is integer arithmetic on the encoder's rows and records.  A handle with a spool and a twin without one are
fed the same input; capi.transmission_spool_reference() is fed the twin's collect_active_encoded() per batch; the spooled handle's collect_transmissions() --
called only after the last batch and a flush unless a case says otherwise -- must give the model's records and audio, and its counters; everything else the
two handles return must be the same bits.  Each case asserts, from the model's output, that its run contained what the case is for."""
import os

import numpy as np
import pytest

import helpers
import spool_cases as sc
import test_gpu_audio_encoding as ae
import test_gpu_gate as gg
import test_output_gate as og

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
capi = sc.capi
IDLE, MAX, FLUSH = capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH
RULE = dict(min_batches=2, idle_batches=1)
THREE = ["k_and_k2", "two_long", "late"]


class Pair:
    """a spooled handle, its twin and the model"""

    def __init__(self, pkg, hip, twin, gate, fmt, max_rows=None, mask=None, **params):
        self.pkg, self.hip, self.twin, self.fmt = pkg, hip, twin, fmt
        self.gate = np.asarray(gate, np.uint8)
        for h in (hip, twin):
            h.set_output_gate(self.gate, max_rows)
            h.set_output_encoding(fmt)
        hip.set_transmission_spool(mask=mask, **params)
        resolved = (self.gate == SIGNAL) if mask is None else np.asarray(mask, bool)
        params.setdefault("export_rows", max(params["pool_rows"], params.get("max_batches", 480) + 1))
        params.setdefault("max_records", hip.total_channels)
        self.model = capi.transmission_spool_reference(resolved, hip.B, **params)
        self.hist, self.got, self.want = [], [], []

    def batch(self, what):
        """the batch that is ready on both handles: the same bits from both, and the model's step"""
        hip, twin = self.hip, self.twin
        full = ae._full(twin)
        ae._same_full(ae._full(hip), full, what)
        self.hist.append(full["axc"].copy())
        a, b = hip.collect_active_encoded(), twin.collect_active_encoded()
        assert a["n_active"] == b["n_active"] and a["channels"].tolist() == b["channels"].tolist(), what
        assert a["audio"].tobytes() == b["audio"].tobytes() and a["info"].tobytes() == b["info"].tobytes(), what + ": encoded rows"
        selected = None
        if b["n_active"] > len(b["channels"]):  # rows past max_rows: the model needs the gate's whole selection
            selected = og.expected_active(self.gate, self.hist)[-1]
            assert len(selected) == b["n_active"]
        self.model.step(b["n_active"], b["channels"], b["audio"], b["info"], selected=selected)

    def collect(self, what, until_empty=True):
        """collect on both until nothing waits; every call must agree"""
        calls = 0
        while True:
            g, w = self.hip.collect_transmissions(), self.model.collect()
            calls += 1
            where = "%s, collect %d" % (what, len(self.got))
            assert len(g["records"]) == len(w["records"]) and g["n_waiting"] == w["n_waiting"], (where, len(g["records"]), len(w["records"]), g["n_waiting"], w["n_waiting"])
            assert g["records"].tobytes() == w["records"].tobytes(), (where, sc.brief(g["records"][:4]), sc.brief(w["records"][:4]))
            assert g["audio"].shape[0] == w["n_rows"] and g["audio"].tobytes() == w["audio"], where + ": audio"
            self.got.append(g)
            self.want.append(w)
            if not until_empty or not w["n_waiting"]:
                return calls

    def finish(self, what):
        self.hip.spool_flush()
        self.model.flush()
        calls = self.collect(what)
        assert self.hip.spool_counters() == self.model.counters(), (what, self.hip.spool_counters(), self.model.counters())
        return calls

    def records(self):
        return np.concatenate([w["records"] for w in self.want]) if self.want else np.zeros(0, sc.REC)


def _run_patterns(pkg, names, gate, fmt, n_batches=og.N_BATCHES, max_rows=None, mask=None, collect_every=0, repeat=1, **params):
    devices = gg._devices(len(names))
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        p = Pair(pkg, hip, twin, gate, fmt, max_rows=max_rows, mask=mask, **params)
        bins = gg._pattern_inputs(names, hip.B)
        mid_calls = 0
        for b in range(n_batches * repeat):
            for h in (hip, twin):
                h.process_bins(*bins[b % og.N_BATCHES])
            p.batch("%s, %d channels, batch %d" % (fmt, len(names), b))
            if collect_every and b % collect_every == collect_every - 1:
                mid_calls += p.collect("mid-run after batch %d" % b)
        calls = p.finish("%s, %d channels" % (fmt, len(names)))
    return p, mid_calls + calls


# ---- 1: the three patterns, both closing rules ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batches", [16, 2])
@pytest.mark.parametrize("fmt", ["ulaw", "s16"])
def test_patterns_close_by_idle_and_by_length(pkg, built, fmt, max_batches):
    names = THREE * 8
    p, _ = _run_patterns(pkg, names, [SIGNAL] * 24, fmt, pool_rows=100, max_records=64, max_batches=max_batches, **RULE)
    recs = p.records()
    if max_batches == 16:  # (step 5, two_long, 3 rows), (6, k_and_k2, 4 rows), (6, late, 2 rows), eight times each
        assert [(int(r["close_batch"]), int(r["channel"]) % 3, int(r["n_rows"]), int(r["reason"])) for r in recs] == \
            [(5, 1, 3, IDLE)] * 8 + [(6, 0, 4, IDLE), (6, 2, 2, IDLE)] * 8
    else:
        assert set(recs["reason"].tolist()) == {IDLE, MAX} and len(recs) == 32
        first = [(int(r["channel"]), int(r["close_batch"]), int(r["n_rows"]), int(r["reason"])) for r in recs if r["channel"] < 3]
        assert first == [(0, 4, 3, MAX), (1, 4, 3, MAX), (2, 6, 2, IDLE), (0, 7, 1, IDLE)]
    assert (recs["n_lost"] == 0).all() and (recs["peak"] > 0).any()


def test_flush_finishes_open_transmissions(pkg, built):
    p, _ = _run_patterns(pkg, THREE * 8, [SIGNAL] * 24, "alaw", n_batches=5, pool_rows=100, max_records=64, max_batches=16, **RULE)
    recs = p.records()
    assert len(recs) == 24 and (recs["reason"] == FLUSH).all() and (recs["close_batch"] == 5).all()
    assert recs["channel"].tolist() == list(range(24)) and recs["n_rows"].tolist() == [4, 3, 2] * 8


# ---- 2: channel counts across a wavefront boundary, mixed gates, a mask --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ch", [63, 64, 65])
def test_mixed_gates_and_a_mask(pkg, built, n_ch):
    names = [og.PATTERN_NAMES[(c * 7 + c // 64) % 4] for c in range(n_ch)]
    gate = np.array([(NEVER, SIGNAL, ALWAYS, SIGNAL, SIGNAL)[c % 5] for c in range(n_ch)], np.uint8)
    mask = np.zeros(n_ch, np.uint8)
    mask[np.flatnonzero(gate == SIGNAL)[::2]] = 1  # every other SIGNAL channel
    p, _ = _run_patterns(pkg, names, gate, "ulaw", mask=mask, pool_rows=200, max_records=80, max_batches=16, **RULE)
    recs = p.records()
    assert len(recs) > 0 and all(mask[c] for c in recs["channel"]) and recs["n_rows"].sum() == p.model.counters()["rows_stored_total"] > 0
    assert recs["channel"].max() >= n_ch - 6, "the last wavefront's channels never finished a transmission"


# ---- 3, 4, 5: a dry pool, a full list, a short gate ------------------------------------------------------------------------------------------------------
def test_pool_exhaustion(pkg, built):
    p, _ = _run_patterns(pkg, THREE, [SIGNAL] * 3, "ulaw", pool_rows=4, export_rows=4, max_records=8, max_batches=3, **RULE)
    recs = p.records()
    assert (recs["n_lost"] > 0).any() and (recs["n_rows"] == 0).any(), sc.brief(recs)
    assert [(int(r["channel"]), int(r["n_rows"]), int(r["n_lost"])) for r in recs] == [(0, 2, 2), (1, 2, 1), (2, 0, 2)]


def test_full_list_drops_transmissions(pkg, built):
    p, _ = _run_patterns(pkg, THREE * 8, [SIGNAL] * 24, "s16", pool_rows=100, max_records=1, max_batches=16, **RULE)
    cn = p.model.counters()
    assert cn["dropped_transmissions"] >= 1 and cn["finished_total"] >= 1 and cn["free_rows_now"] == 100
    assert len(p.records()) == cn["finished_total"]


def test_rows_past_the_gates_max_rows_are_lost(pkg, built):
    n_ch = 65
    names = THREE * 21 + ["late", "late"]
    p, _ = _run_patterns(pkg, names, [SIGNAL] * n_ch, "alaw", max_rows=5, pool_rows=100, max_records=80, max_batches=16, **RULE)
    recs = p.records()
    assert (recs["n_lost"] > 0).any() and (recs["n_rows"] > 0).any() and ((recs["n_rows"] == 0) & (recs["channel"] > 5)).any(), sc.brief(recs[:8])
    assert p.model.counters()["rows_lost_total"] > 0


# ---- 6: the smallest export buffer, collects in mid-run, freed rows used again ------------------------------------------------------------------------------
def test_smallest_export_buffer_and_collects_in_mid_run(pkg, built):
    p, calls = _run_patterns(pkg, THREE * 8, [SIGNAL] * 24, "ulaw", collect_every=3, repeat=2, pool_rows=80, export_rows=3, max_records=64, max_batches=2, **RULE)
    cn = p.model.counters()
    assert calls >= 2 and max(len(w["records"]) for w in p.want) >= 1 and all(w["n_rows"] <= 3 for w in p.want)
    assert cn["rows_lost_total"] == 0 and cn["rows_stored_total"] > 80, cn  # more rows than the pool has: the collects' rows were used again
    assert sum(1 for w in p.want if len(w["records"])) >= 2


# ---- 7, 8: raw I/Q through the host ring, sequential and pipelined; a scan handle -------------------------------------------------------------------------
def _run_stream(pkg, devices, iq, n_batches, flags, gate, wave_rate, fmt, scan=None, sched=None, **params):
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as twin:
        p = Pair(pkg, hip, twin, gate, fmt, **params)
        g = hip.geometry
        pipelined = bool(flags & capi.FLAG_PIPELINE)
        off = 0
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
            if not pipelined or k > 0:
                p.batch("wave rate %d, flags %#x, batch %d" % (wave_rate, flags, k - 1 if pipelined else k))
        if pipelined:
            for h in (hip, twin):
                h.flush()  # the last batch's results and its step, before the spool's flush
            p.batch("wave rate %d, flags %#x, last batch" % (wave_rate, flags))
        p.finish("wave rate %d, flags %#x" % (wave_rate, flags))
        assert p.model.counters()["steps"] == n_batches and hip.B == (2000 if wave_rate == 16000 else 1000)
    return p


@pytest.mark.parametrize("flag_names", [(), ("FLAG_PIPELINE",)])
def test_stream_at_16000(pkg, built, flag_names):
    flags = 0
    for f in flag_names:
        flags |= getattr(capi, f)
    devices, iq = gg._stream_case(pkg, 16000, 3, ae.N_BATCHES)
    p = _run_stream(pkg, devices, iq, ae.N_BATCHES, flags, gg._mixed_gate(24), 16000, "s16", pool_rows=200, max_records=64, max_batches=3, **RULE)
    recs = p.records()
    assert len(recs) > 0 and recs["n_rows"].sum() > 0 and (recs["peak"] > 0).any()


def test_scan_handle_switching_entries(pkg, built):
    devices, iq = gg._stream_case(pkg, 8000, 1, ae.N_BATCHES)
    ch0 = devices[0]["channels"][0]
    rest = {k: v for k, v in devices[0].items() if k != "channels"}
    devs = [dict(rest, channels=[ch0]), devices[0]]
    scan = {0: [ch0, dict(ch0, squelch_snr_threshold_db=14.0, ampfactor=0.5), dict(ch0, notch_freq=1000.0)]}
    gate = np.full(9, SIGNAL, np.uint8)
    gate[4] = ALWAYS
    p = _run_stream(pkg, devs, [iq[0], iq[0]], ae.N_BATCHES, 0, gate, 8000, "alaw", scan=scan, sched=[0, 1, 1, 2, 0, 2], pool_rows=100, max_records=32, max_batches=2, **RULE)
    recs = p.records()
    assert len(recs) > 0 and recs["n_rows"].sum() > 0 and 4 not in recs["channel"].tolist()


# ---- 9: errors leave a working handle -----------------------------------------------------------------------------------------------------------------------
def test_errors_leave_a_working_handle(pkg, built):
    n = 16
    names = ["k_and_k2", "late"] * 8
    devices = gg._devices(n)
    ok = np.full(n, SIGNAL, np.uint8)
    mixed = ok.copy()
    mixed[3] = ALWAYS
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        L = hip.L
        bins = gg._pattern_inputs(names, hip.B)
        good = (64, 64, 16, 2, 1, 16)
        assert L.airband_hip_set_transmission_spool(hip.h, None, *good) == capi.EINVAL  # no gate
        hip.set_output_gate(mixed)
        assert L.airband_hip_set_transmission_spool(hip.h, None, *good) == capi.EINVAL  # no encoding
        for call in (hip.collect_transmissions, hip.spool_flush, hip.spool_counters, hip.device_transmission_spool):
            with pytest.raises(pkg.AirbandError) as e:  # no spool
                call()
            assert e.value.code == capi.EINVAL
        hip.set_output_encoding("ulaw")
        for bad in ((-1, 64, 16, 2, 1, 16), (64, -1, 16, 2, 1, 16), (64, 64, -1, 2, 1, 16), (64, 64, 16, -1, 1, 16), (64, 64, 16, 2, -1, 16), (64, 64, 16, 2, 1, 0),
                    (64, 16, 16, 2, 1, 16), (64, 64, 0, 2, 1, 16)):
            assert L.airband_hip_set_transmission_spool(hip.h, None, *bad) == capi.EINVAL, bad
        everyone = np.ones(n, np.uint8)
        assert L.airband_hip_set_transmission_spool(hip.h, everyone.ctypes.data, *good) == capi.EINVAL  # channel 3's gate is ALWAYS
        hip.set_transmission_spool(64, max_batches=16)  # NULL mask: the SIGNAL channels
        hip.set_transmission_spool(0)                   # removed again
        assert L.airband_hip_collect_transmissions(hip.h, None, None, None, None, None) == capi.EINVAL
        hip.set_transmission_spool(64, max_batches=16)
        hip.set_output_encoding("alaw")                 # an encoding set again drops the spool
        assert L.airband_hip_spool_flush(hip.h) == capi.EINVAL
        hip.set_output_gate(ok)                         # ... and so does a gate
        twin.set_output_gate(ok)
        for h in (hip, twin):
            h.set_output_encoding("alaw")
        for b in range(3):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            if b == 0:
                assert L.airband_hip_set_transmission_spool(hip.h, None, *good) == capi.EINVAL  # a batch has been enqueued
                assert L.airband_hip_collect_transmissions(hip.h, None, None, None, None, None) == capi.EINVAL
            ae._same_full(ae._full(hip), ae._full(twin), "batch %d" % b)
            a, t = hip.collect_active_encoded(), twin.collect_active_encoded()
            assert a["channels"].tolist() == t["channels"].tolist() and a["audio"].tobytes() == t["audio"].tobytes()
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        p = Pair(pkg, hip, twin, ok, "ulaw", pool_rows=8, max_records=4, max_batches=16, **RULE)
        hip.set_transmission_spool(64, max_records=32, max_batches=16, **RULE)  # replaced before the first batch
        p.model = capi.transmission_spool_reference(ok, hip.B, pool_rows=64, export_rows=64, max_records=32, max_batches=16, **RULE)
        got = hip.collect_transmissions()  # before any batch: nothing, and no EAGAIN
        assert len(got["records"]) == 0 and got["audio"].shape == (0, hip.B) and got["n_waiting"] == 0
        for b in range(og.N_BATCHES):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            p.batch("replaced spool, batch %d" % b)
        # any out-pointer may be NULL: the transmissions are taken all the same
        assert hip.L.airband_hip_collect_transmissions(hip.h, None, None, None, None, None) == capi.OK
        assert len(p.model.collect()["records"]) == 16
        p.finish("replaced spool")
        v = hip.device_transmission_spool()
        assert v["audio"] and v["records"] and v["n_export"]


# ---- 10: a handle without a spool launches nothing new ----------------------------------------------------------------------------------------------------
def _traced_kernels(extra):
    return helpers.traced_kernels("transmission_spool_profile.py", extra, [("demod_kernel", "back_kernel")])


def test_handle_without_a_spool_launches_no_spool_kernel(pkg, built):
    spooled = _traced_kernels(["--handles", "spool"])
    for k in ("spool_scan_kernel", "spool_close_kernel", "spool_append_kernel", "spool_copy_kernel", "audio_pack_ulaw_kernel"):
        assert k in spooled, k  # the check below is not vacuous
    plain = _traced_kernels(["--handles", "host"])
    assert "audio_pack_ulaw_kernel" in plain and "spool_" not in plain.replace("transmission_spool_profile", "")
