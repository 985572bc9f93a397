"""Mixer transmission spool on the GPU (airband_hip_set_mixer_spool / _collect_mixer_transmissions / _mixer_spool_flush / _mixer_spool_counters_get /
_device_mixer_spool; csrc/tx_spool.hip behind the mixer gate's pack).

Every comparison is byte for byte.  The expectation throughout is the definition in plain Python (capi.transmission_spool_reference) fed, step by step, what
collect_active_mixers() of the SAME handle returned -- which keeps these tests apart from the mixer gate's own (tests/test_gpu_mixer_gate.py) and from mixer-sum
parity; `selected` comes from has_signal by the gate's rule (capi.mixer_gate_selection) and must agree with the gate's count and list.  Records, audio and
counters are compared as bytes.  Each case asserts, from the model's output, that its run contained what the case is for."""
import importlib
import os
import sys

import numpy as np
import pytest

import helpers
import spool_cases as sc
import test_gpu_mixer_gate as mg
import test_output_gate as og

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")
NEVER, SIGNAL, ALWAYS = og.NEVER, og.SIGNAL, og.ALWAYS
capi = sc.capi
IDLE, MAX, FLUSH = capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH
RULE = dict(min_batches=2, idle_batches=1)


class Spooled:
    """a handle with an encoded mixer gate and a mixer spool, and the model"""

    def __init__(self, hip, gate, enc, stereo, max_rows=None, mask=None, manual=False, **params):
        self.hip, self.gate = hip, np.asarray(gate, np.uint8)
        hip.set_mixer_gate(self.gate, max_rows, enc, stereo=stereo, manual_step=manual)
        self.set_spool(mask, **params)

    def set_spool(self, mask=None, **params):
        """(again: replaces the spool, and the model with it; the gate's memory stays)"""
        self.hip.set_mixer_spool(mask=mask, **params)
        resolved = (self.gate == SIGNAL) if mask is None else np.asarray(mask, bool)
        params.setdefault("export_rows", max(params["pool_rows"], params.get("max_batches", 480) + 1))
        params.setdefault("max_records", len(self.gate))
        self.model = capi.transmission_spool_reference(resolved, self.hip.B, **params)
        if not hasattr(self, "sel"):
            self.sel = capi.mixer_gate_selection(self.gate)
        self.got, self.want, self.fed = [], [], []

    def step(self, what):
        """behind a mixer gate step: what the handle's own collect_active_mixers() returns is the model's step"""
        a = self.hip.collect_active_mixers()
        selected = self.sel.step(a["has_signal"])
        assert len(selected) == a["n_active"] and selected[:len(a["mixers"])].tolist() == a["mixers"].tolist(), (what, a["n_active"], selected.tolist(), a["mixers"].tolist())
        self.model.step(a["n_active"], a["mixers"], a["audio"], a["info"], selected=selected)
        self.fed.append(a)
        return a

    def collect(self, what, until_empty=True):
        calls = 0
        while True:
            g, w = self.hip.collect_mixer_transmissions(), self.model.collect()
            calls += 1
            where = "%s, collect %d" % (what, len(self.got))
            assert len(g["records"]) == len(w["records"]) and g["n_waiting"] == w["n_waiting"], (where, len(g["records"]), len(w["records"]), g["n_waiting"], w["n_waiting"])
            assert g["records"].tobytes() == w["records"].tobytes(), (where, sc.brief(g["records"][:4]), g["records"]["reserved"][:4].tolist(), sc.brief(w["records"][:4]), w["records"]["reserved"][:4].tolist())
            assert g["audio"].shape[0] == w["n_rows"] and g["audio"].tobytes() == w["audio"], where + ": audio"
            self.got.append(g)
            self.want.append(w)
            if not until_empty or not w["n_waiting"]:
                return calls

    def finish(self, what):
        self.hip.mixer_spool_flush()
        self.model.flush()
        calls = self.collect(what)
        assert self.hip.mixer_spool_counters() == self.model.counters(), (what, self.hip.mixer_spool_counters(), self.model.counters())
        return calls

    def records(self):
        return np.concatenate([w["records"] for w in self.want]) if self.want else np.zeros(0, sc.REC)


def _brief(recs):
    """(mixer, open, last, close, n_rows, n_lost, reason, reserved[1])"""
    return [(int(r["channel"]), int(r["open_batch"]), int(r["last_batch"]), int(r["close_batch"]), int(r["n_rows"]), int(r["n_lost"]), int(r["reason"]), int(r["reserved"][1]))
            for r in recs]


def _many_mixers(n):
    """n mixers over the 72 pattern channels: mixer m sums channel m % 72 (pattern mg.NAMES[...]) and is stereo by balance where m % 3 == 0"""
    return [((m % mg.N_CH) // 8, (m % mg.N_CH) % 8, m, 0.6, 0.5 if m % 3 == 0 else 0.0) for m in range(n)]


def _run_patterns(pkg, gate, enc, stereo, wave_rate=8000, wiring=None, n_batches=og.N_BATCHES, repeat=1, collect_every=0, stereo_at=None, **kw):
    """the named squelch patterns through process_bins on one handle; stereo_at = (batch, mixer): airband_hip_mixer_set_stereo(mixer, True) in front of that batch"""
    with pkg.AirbandHip(mg._devices(mg.N_CH), wave_rate=wave_rate) as hip:
        if wiring is None:
            mg._wire(hip)
        else:
            hip.set_mixers(len(gate), wiring)
        p = Spooled(hip, gate, enc, stereo, **kw)
        bins = mg._pattern_inputs(mg.NAMES, hip.B)
        mid = 0
        for b in range(n_batches * repeat):
            if stereo_at and stereo_at[0] == b:
                hip.mixer_set_stereo(stereo_at[1], True)
            hip.process_bins(*bins[b % og.N_BATCHES])
            p.step("batch %d" % b)
            hip.collect()
            if collect_every and b % collect_every == collect_every - 1:
                mid += p.collect("mid-run after batch %d" % b)
        calls = p.finish("%s, stereo %s" % (enc, stereo))
        assert p.model.counters()["steps"] == n_batches * repeat
        assert hip.B == (2000 if wave_rate == 16000 else 1000)
        row = hip.B * (2 if stereo else 1) * (2 if enc == "s16" else 1)
        assert all(len(w["audio"]) == w["n_rows"] * row for w in p.want)
    return p, mid + calls


# ---- 1: both closing rules, every width and encoding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("enc,stereo,wave_rate,max_batches", [("ulaw", False, 8000, 16), ("ulaw", True, 8000, 2), ("s16", False, 8000, 2), ("s16", True, 8000, 16),
                                                               ("alaw", True, 16000, 16)])
def test_idle_and_max_closing(pkg, built, enc, stereo, wave_rate, max_batches):
    """The wiring of tests/test_gpu_mixer_gate.py: mixers 0, 1, 3, 5 are SIGNAL (spooled by the NULL mask), 2 and 4 ALWAYS, 6 NEVER; mixers 1 and 2 are stereo.
    Mixer 0 turns stereo in front of batch 3, in the middle of its transmission."""
    p, _ = _run_patterns(pkg, mg.GATE, enc, stereo, wave_rate, stereo_at=(3, 0), pool_rows=64, max_batches=max_batches, **RULE)
    recs = p.records()
    assert len(recs) > 0 and set(recs["channel"].tolist()) <= {0, 1, 3, 5} and (recs["n_lost"] == 0).all() and (recs["peak"] > 0).any()
    if wave_rate == 8000:
        assert {0, 1, 3} <= set(recs["channel"].tolist()) and 5 not in recs["channel"].tolist()  # mixer 5's inputs are quiet
        assert set(recs["reason"].tolist()) == ({IDLE} if max_batches == 16 else {IDLE, MAX}), _brief(recs)
        by_mixer = {m: [int(r["reserved"][1]) for r in recs if r["channel"] == m] for m in (0, 1, 3)}
        assert set(by_mixer[1]) == {1} and set(by_mixer[3]) == {0} and 1 in by_mixer[0], by_mixer  # stereo, mono, mono-then-stereo
    assert (recs["reserved"][:, 0] == 0).all() and (recs["first"] <= p.hip.B).all() and (recs["end"] <= p.hip.B).all()  # frames, not samples


def test_flush_finishes_open_transmissions(pkg, built):
    p, _ = _run_patterns(pkg, mg.GATE, "alaw", True, n_batches=3, pool_rows=64, max_batches=16, **RULE)
    recs = p.records()
    assert len(recs) >= 2 and (recs["reason"] == FLUSH).all() and (recs["close_batch"] == 3).all() and recs["channel"].tolist() == sorted(recs["channel"].tolist())


# ---- 2: mixer counts across a wavefront boundary, mixed gates, a mask ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65])
def test_mixed_gates_and_a_mask(pkg, built, n):
    gate = np.array([(NEVER, SIGNAL, ALWAYS, SIGNAL, SIGNAL)[m % 5] for m in range(n)], np.uint8)
    mask = np.zeros(n, np.uint8)
    mask[np.flatnonzero(gate == SIGNAL)[::2]] = 1  # every other SIGNAL mixer
    p, _ = _run_patterns(pkg, gate, "ulaw", True, wiring=_many_mixers(n), mask=mask, pool_rows=300, max_records=100, max_batches=16, **RULE)
    recs = p.records()
    assert len(recs) > 0 and all(mask[m] for m in recs["channel"]) and recs["n_rows"].sum() == p.model.counters()["rows_stored_total"] > 0
    assert recs["channel"].max() >= n - 6, "the last wavefront's mixers never finished a transmission"
    assert set(recs["reserved"][:, 1].tolist()) == {0, 1}


# ---- 3, 4, 5: a dry pool, a full list, a short gate --------------------------------------------------------------------------------------------------------
def test_pool_exhaustion(pkg, built):
    p, _ = _run_patterns(pkg, mg.GATE, "ulaw", True, pool_rows=4, export_rows=4, max_records=8, max_batches=3, **RULE)
    recs = p.records()
    assert (recs["n_lost"] > 0).any() and p.model.counters()["rows_lost_total"] > 0, _brief(recs)
    lost = [int(r["channel"]) for r in recs if r["n_lost"]]
    assert max(lost) == max(recs["channel"]) or len(set(lost)) > 1, _brief(recs)  # who loses is decided by rank: the higher mixers first


def test_full_list_drops_transmissions(pkg, built):
    gate = np.full(24, SIGNAL, np.uint8)
    p, _ = _run_patterns(pkg, gate, "s16", False, wiring=_many_mixers(24), pool_rows=200, max_records=1, max_batches=16, **RULE)
    cn = p.model.counters()
    assert cn["dropped_transmissions"] >= 1 and cn["finished_total"] >= 1 and cn["free_rows_now"] == 200
    assert len(p.records()) == cn["finished_total"]


def test_rows_past_the_gates_max_rows_are_lost(pkg, built):
    n = 65
    gate = np.full(n, SIGNAL, np.uint8)
    p, _ = _run_patterns(pkg, gate, "alaw", True, wiring=_many_mixers(n), max_rows=5, pool_rows=200, max_records=80, max_batches=16, **RULE)
    recs = p.records()
    assert any(a["n_active"] > 5 for a in p.fed), "the gate never selected more than it lists"
    assert (recs["n_lost"] > 0).any() and (recs["n_rows"] > 0).any() and ((recs["n_rows"] == 0) & (recs["channel"] > 5)).any(), _brief(recs[:8])
    assert p.model.counters()["rows_lost_total"] > 0


# ---- 6: the smallest export buffer, collects in mid-run, freed rows used again -----------------------------------------------------------------------------
def test_smallest_export_buffer_and_collects_in_mid_run(pkg, built):
    gate = np.full(24, SIGNAL, np.uint8)
    p, calls = _run_patterns(pkg, gate, "ulaw", True, wiring=_many_mixers(24), collect_every=3, repeat=2, pool_rows=60, export_rows=3, max_records=64, max_batches=2, **RULE)
    cn = p.model.counters()
    assert calls >= 2 and all(w["n_rows"] <= 3 for w in p.want) and sum(1 for w in p.want if len(w["records"])) >= 2
    assert cn["rows_lost_total"] == 0 and cn["rows_stored_total"] > 60, cn  # more rows than the pool has: the collects' rows were used again


# ---- 7: a manual gate stepped behind add_mixers() on two handles: k follows the steps, not the batches ------------------------------------------------------
def test_manual_steps_behind_add_mixers_count_k(pkg, built):
    devices = mg._devices(8)
    src_names, dst_names = ["two_long"] + ["quiet"] * 7, ["late"] + ["quiet"] * 7
    wiring = [(0, 0, 0, 1.0, 0.5), (0, 1, 1, 1.0, 0.0)]
    gate = np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as src, pkg.AirbandHip(devices, wave_rate=8000) as dst:
        for h in (src, dst):
            h.set_mixers(3, wiring)
        p = Spooled(dst, gate, "ulaw", True, manual=True, pool_rows=64, max_batches=16, **RULE)
        sb, db = mg._pattern_inputs(src_names, src.B), mg._pattern_inputs(dst_names, dst.B)
        alone, steps = [], 0  # alone: per step, mixer 0's signal flag in dst's own sums
        for b in range(og.N_BATCHES):
            src.process_bins(*sb[b])
            dst.process_bins(*db[b])
            assert dst.mixer_spool_counters()["steps"] == steps  # nothing steps with the batch
            own = int(dst.collect_mixers()[2][0])
            dst.add_mixers(src)
            for _ in range(2 if b % 2 else 1):  # two steps behind an odd batch: k runs ahead of the batch number
                dst.mixer_gate_step()
                p.step("manual, batch %d" % b)
                alone.append(own)
                steps += 1
            src.collect()
            dst.collect()
        p.finish("manual")
        recs = p.records()
        assert steps == 12 == p.model.counters()["steps"] and len(recs) >= 1 and recs["channel"].tolist()[0] == 0
        listed = [0 in a["mixers"].tolist() for a in p.fed]  # per step; a second step behind one batch sees the same sums, and by `prev` lists mixer 0 again
        batch_of = [b for b in range(og.N_BATCHES) for _ in range(2 if b % 2 else 1)]
        assert sum(listed) > len({b for b, l in zip(batch_of, listed) if l}) and int(recs["n_rows"][recs["channel"] == 0].sum()) == sum(listed), (_brief(recs), listed)
        first = recs[0]
        assert int(first["open_batch"]) == listed.index(True) and int(first["last_batch"]) - int(first["open_batch"]) + 1 == int(first["n_rows"]), _brief(recs)  # step numbers
        assert any(a["has_signal"][0] and not own for a, own in zip(p.fed, alone)), "mixer 0 never had signal from src alone: the steps saw nothing a batch-time step would not"


# ---- 8: FLAG_PIPELINE through submit / process, and process_device on a caller's stream ---------------------------------------------------------------------
def test_pipelined_submit_process(pkg, built):
    n_batches = 6
    devices, iq = helpers.format_case(pkg, capi.SFMT_U8, 9, 2_560_000, 8000, 2, n_batches)
    iq = [np.ascontiguousarray(x).view(np.uint8) for x in iq]
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE) as hip:
        hip.set_mixers(3, [(0, c, 0, 0.5, 0.5 if c % 2 else -0.25) for c in range(8)] + [(1, c, 1, 0.7, 0.0) for c in range(4)])
        p = Spooled(hip, np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8), "ulaw", True, pool_rows=32, max_batches=2, min_batches=1, idle_batches=0)
        g = hip.geometry
        off = 0
        for k in range(n_batches):
            take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
            lo = off if k == 0 else off + g.lookahead_bytes
            for d in range(2):
                assert hip.submit(d, iq[d][lo:lo + take]) == take
            off += g.first_batch_bytes if k == 0 else g.batch_bytes
            assert hip.process()
            if k > 0:
                p.step("pipelined, batch %d" % (k - 1))
                hip.collect()
        hip.flush()  # the last batch's results and its step, before the spool's flush
        p.step("pipelined, last batch")
        p.finish("pipelined")
    assert p.model.counters()["steps"] == n_batches and len(p.records()) > 0 and p.records()["n_rows"].sum() > 0


def test_process_device_on_a_caller_stream(pkg, built):
    torch = pytest.importorskip("torch")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_batches = 2, 5
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        hip.set_mixers(3, [(0, c, 0, 0.5, 0.5 if c % 2 else -0.25) for c in range(8)] + [(1, c, 1, 0.7, 0.0) for c in range(4)])
        p = Spooled(hip, np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8), "s16", True, pool_rows=32, max_batches=2, min_batches=1, idle_batches=0)
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
            p.step("caller stream, batch %d" % b)
            if b == 2:
                p.collect("caller stream, mid-run", until_empty=False)
        p.finish("caller stream")
        s.synchronize()
        del buf
    assert p.model.counters()["steps"] == n_batches and len(p.records()) > 0 and p.records()["n_rows"].sum() > 0


# ---- 9: the gate set again drops the spool; the spool set again restarts k ---------------------------------------------------------------------------------
def test_gate_again_drops_the_spool_and_spool_again_restarts_k(pkg, built):
    with pkg.AirbandHip(mg._devices(mg.N_CH), wave_rate=8000) as hip:
        mg._wire(hip)
        p = Spooled(hip, mg.GATE, "ulaw", True, pool_rows=64, max_batches=16, **RULE)
        bins = mg._pattern_inputs(mg.NAMES, hip.B)
        for b in range(3):
            hip.process_bins(*bins[b])
            p.step("first spool, batch %d" % b)
            hip.collect()
        assert p.model.counters()["open_now"] >= 2 and hip.mixer_spool_counters() == p.model.counters()
        p.set_spool(pool_rows=48, max_batches=16, **RULE)  # after batches have run: replaced, k = 0 again, the open transmissions are gone
        assert hip.mixer_spool_counters() == p.model.counters() and p.model.counters()["steps"] == 0
        for b in range(3, og.N_BATCHES):
            hip.process_bins(*bins[b])
            p.step("second spool, batch %d" % b)
            hip.collect()
        p.finish("second spool")
        recs = p.records()
        assert len(recs) > 0 and int(recs["open_batch"].min()) == 0 and int(recs["close_batch"].max()) <= og.N_BATCHES - 3, _brief(recs)
        hip.set_mixer_spool(0)  # removed
        assert hip.L.airband_hip_mixer_spool_flush(hip.h) == capi.EINVAL
        hip.set_mixer_spool(16, max_batches=8)
        hip.set_mixer_gate(mg.GATE, encoding="ulaw", stereo=True)  # the gate set again drops it
        assert hip.L.airband_hip_collect_mixer_transmissions(hip.h, None, None, None, None, None) == capi.EINVAL
        hip.set_mixer_spool(16, max_batches=8)
        mg._wire(hip)  # ... and so does the wiring
        assert hip.L.airband_hip_mixer_spool_counters_get(hip.h, capi.SpoolCounters()) == capi.EINVAL


# ---- 10: a channel spool and a mixer spool on one handle ----------------------------------------------------------------------------------------------------
def test_channel_spool_and_mixer_spool_on_one_handle(pkg, built):
    devices = mg._devices(mg.N_CH)
    ch_gate = np.full(mg.N_CH, SIGNAL, np.uint8)
    with pkg.AirbandHip(devices, wave_rate=8000) as hip, pkg.AirbandHip(devices, wave_rate=8000) as twin:
        for h in (hip, twin):
            h.set_output_gate(ch_gate)
            h.set_output_encoding("ulaw")
            h.set_transmission_spool(300, max_records=100, max_batches=16, **RULE)
            mg._wire(h)
        ch_model = capi.transmission_spool_reference(ch_gate == SIGNAL, hip.B, pool_rows=300, export_rows=300, max_records=100, max_batches=16, **RULE)
        p = Spooled(hip, mg.GATE, "s16", True, pool_rows=64, max_batches=16, **RULE)
        twin.set_mixer_gate(mg.GATE, encoding="s16", stereo=True)  # the twin: the same gate, no mixer spool
        bins = mg._pattern_inputs(mg.NAMES, hip.B)
        for b in range(og.N_BATCHES):
            for h in (hip, twin):
                h.process_bins(*bins[b])
            p.step("both spools, batch %d" % b)
            a, t = hip.collect_active_encoded(), twin.collect_active_encoded()
            assert a["n_active"] == t["n_active"] and a["audio"].tobytes() == t["audio"].tobytes() and a["info"].tobytes() == t["info"].tobytes()
            ch_model.step(t["n_active"], t["channels"], t["audio"], t["info"])
            if b == 5:
                hip.collect_mixer_transmissions()  # a mixer collect in mid-run leaves the channel spool alone
                p.model.collect()
        p.finish("both spools: the mixers'")
        for h in (hip, twin):
            h.spool_flush()
        ch_model.flush()
        a, t, w = hip.collect_transmissions(), twin.collect_transmissions(), ch_model.collect()
        assert len(w["records"]) > 0 and a["records"].tobytes() == t["records"].tobytes() == w["records"].tobytes()
        assert a["audio"].tobytes() == t["audio"].tobytes() == w["audio"] and a["n_waiting"] == t["n_waiting"] == w["n_waiting"] == 0
        assert (a["records"]["reserved"] == 0).all()
        assert hip.spool_counters() == twin.spool_counters() == ch_model.counters()
        assert len(p.records()) > 0


# ---- 11: every error leaves a working handle ---------------------------------------------------------------------------------------------------------------
def test_errors_leave_a_working_handle(pkg, built):
    good = (64, 64, 16, 2, 1, 16)
    with pkg.AirbandHip(mg._devices(mg.N_CH), wave_rate=8000) as hip:
        L = hip.L
        assert L.airband_hip_set_mixer_spool(hip.h, None, *good) == capi.EINVAL  # no mixers
        mg._wire(hip)
        assert L.airband_hip_set_mixer_spool(hip.h, None, *good) == capi.EINVAL  # no mixer gate
        hip.set_mixer_gate(mg.GATE, stereo=True)
        assert L.airband_hip_set_mixer_spool(hip.h, None, *good) == capi.EINVAL  # a float gate
        assert "AIRBAND_AUDIO_F32" in hip.L.airband_hip_last_error(hip.h).decode()
        hip.set_mixer_gate(mg.GATE, encoding="ulaw", stereo=True)
        for call in (hip.collect_mixer_transmissions, hip.mixer_spool_flush, hip.mixer_spool_counters, hip.device_mixer_spool):
            with pytest.raises(pkg.AirbandError) as e:  # no spool
                call()
            assert e.value.code == capi.EINVAL
        for bad in ((-1, 64, 16, 2, 1, 16), (64, -1, 16, 2, 1, 16), (64, 64, -1, 2, 1, 16), (64, 64, 16, -1, 1, 16), (64, 64, 16, 2, -1, 16), (64, 64, 16, 2, 1, 0),
                    (64, 16, 16, 2, 1, 16), (64, 64, 0, 2, 1, 16)):
            assert L.airband_hip_set_mixer_spool(hip.h, None, *bad) == capi.EINVAL, bad
        everyone = np.ones(mg.N_MIX, np.uint8)
        assert L.airband_hip_set_mixer_spool(hip.h, everyone.ctypes.data, *good) == capi.EINVAL  # mixer 2's gate is ALWAYS
        assert L.airband_hip_mixer_spool_flush(hip.h) == capi.EINVAL  # none of them left a spool behind
        # ... and the handle runs on: a spool set after batches have run, against the model
        bins = mg._pattern_inputs(mg.NAMES, hip.B)
        hist = []
        for b in range(2):
            hip.process_bins(*bins[b])
            mg._check_step(hip, mg.GATE, mg.N_MIX, "ulaw", True, hist, mg.STEREO_FLAGS, "before the spool, batch %d" % b)
            hip.collect()
        p = Spooled.__new__(Spooled)
        p.hip, p.gate = hip, mg.GATE
        p.sel = capi.mixer_gate_selection(mg.GATE)
        for _, _, sig, _ in hist:
            p.sel.step(sig)  # the gate's memory is two steps old
        p.set_spool(pool_rows=64, max_batches=16, **RULE)
        got = hip.collect_mixer_transmissions()  # before any step: nothing, and no EAGAIN
        assert len(got["records"]) == 0 and got["audio"].shape == (0, 2 * hip.B) and got["n_waiting"] == 0
        for b in range(2, og.N_BATCHES):
            hip.process_bins(*bins[b])
            p.step("late spool, batch %d" % b)
            hip.collect()
        assert hip.L.airband_hip_collect_mixer_transmissions(hip.h, None, None, None, None, None) == capi.OK  # any out-pointer may be NULL: taken all the same
        assert len(p.model.collect()["records"]) >= 1
        p.finish("late spool")
        assert p.model.counters()["steps"] == og.N_BATCHES - 2 and p.model.counters()["finished_total"] >= 2


# ---- 12: the device views match the collect -----------------------------------------------------------------------------------------------------------------
def test_device_views_match_the_collect(pkg, built):
    torch = pytest.importorskip("torch")
    with pkg.AirbandHip(mg._devices(mg.N_CH), wave_rate=8000) as hip:
        mg._wire(hip)
        p = Spooled(hip, mg.GATE, "s16", True, pool_rows=64, export_rows=40, max_records=12, max_batches=16, **RULE)
        bins = mg._pattern_inputs(mg.NAMES, hip.B)
        for b in range(og.N_BATCHES):
            hip.process_bins(*bins[b])
            p.step("views, batch %d" % b)
            hip.collect()
        hip.mixer_spool_flush()
        p.model.flush()
        p.collect("views", until_empty=False)
        got = p.got[0]
        n, rows = len(got["records"]), got["audio"].shape[0]
        v = hip.device_mixer_spool()
        assert torch.as_tensor(pkg.DevicePtr(v["n_export"], (3,), "<i4"), device="cuda").cpu().numpy().tolist() == [n, rows, got["n_waiting"]] and n >= 2
        recs = torch.as_tensor(pkg.DevicePtr(v["records"], (12, 12), "<i4"), device="cuda").cpu().numpy()
        audio = torch.as_tensor(pkg.DevicePtr(v["audio"], (40, 2 * hip.B), "<i2"), device="cuda").cpu().numpy()
        assert recs[:n].tobytes() == got["records"].tobytes() and audio[:rows].tobytes() == got["audio"].tobytes()


# ---- 13: a handle with a mixer gate and no spool launches no spool kernel -----------------------------------------------------------------------------------
def _traced_kernels(extra):
    return helpers.traced_kernels("mixer_spool_profile.py", extra, ["mix_final_kernel", "mixer_pack_ulaw_stereo_kernel"])


def test_mixer_gate_without_a_spool_launches_no_spool_kernel(pkg, built):
    spooled = _traced_kernels(["--handles", "spool"])
    for k in ("spool_scan_kernel", "spool_close_kernel", "spool_append_kernel", "spool_copy_kernel"):
        assert k in spooled, k  # the check below is not vacuous
    plain = _traced_kernels(["--handles", "host"])
    assert "spool_" not in plain.replace("mixer_spool_profile", "")


# ---- 14: two ranks through tests/fake_rccl/: each spools a disjoint half of the mixers, behind the exchange ---------------------------------------------------
N_FABRIC_MIXERS, N_FABRIC_BATCHES, PER_RANK = 64, 5, 6


def _fabric_main(log, q):
    try:
        os.environ["AIRBAND_HIP_RCCL_LIB"] = FAKE_RCCL
        os.environ["FAKE_RCCL_LOG"] = log
        for path in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            if path not in sys.path:
                sys.path.insert(0, path)
        import torch

        pkg = importlib.import_module("rtlsdr-airband_amd")
        multi = importlib.import_module("rtlsdr-airband_amd.multigpu")
        chans, carriers = pkg.siggen.baseline_plan(mixed=True)
        gate = np.full(N_FABRIC_MIXERS, SIGNAL, np.uint8)
        params = dict(pool_rows=400, max_records=N_FABRIC_MIXERS, max_batches=2, min_batches=1, idle_batches=0)
        hs, streams, halves = [], [], []
        for r in range(2):
            h = pkg.AirbandHip([dict(channels=chans)] * PER_RANK, wave_rate=16000, hip_device=0)
            h.set_mixers(N_FABRIC_MIXERS, multi.baseline_mixer_inputs(r * PER_RANK, (r + 1) * PER_RANK, 8, N_FABRIC_MIXERS))
            h.set_signal_plan(carriers)
            half = (np.arange(N_FABRIC_MIXERS) % 2 == r).astype(np.uint8)
            h.set_mixer_gate(gate, encoding="ulaw", stereo=True, manual_step=True)
            h.set_mixer_spool(mask=half, **params)
            g = h.geometry
            span = g.first_batch_bytes + (N_FABRIC_BATCHES - 1) * g.batch_bytes + g.lookahead_bytes
            stride = (span + 255) // 256 * 256
            iq = torch.empty((PER_RANK, stride), dtype=torch.uint8, device="cuda:0")
            h.generate_iq(iq.data_ptr(), stride, 0, span, seed=0x5EED, device_index_offset=r * PER_RANK)
            h.synchronize()
            hs.append(h)
            streams.append((iq, stride))
            halves.append(half)
        pkg.AirbandHip.comm_init_all(hs)
        steps, partial = [], []
        for b in range(N_FABRIC_BATCHES):
            for h, (iq, stride) in zip(hs, streams):
                g = h.geometry
                h.process_device(iq.data_ptr() + (0 if b == 0 else g.first_batch_bytes + (b - 1) * g.batch_bytes), stride)
            partial.append([h.collect_mixers()[2].copy() for h in hs])
            pkg.AirbandHip.allreduce_mixers_group(hs)
            for h in hs:
                h.mixer_gate_step()  # behind the exchange: the spool sees the node's sums
            steps.append([h.collect_active_mixers() for h in hs])
        clips = []
        for h in hs:
            h.mixer_spool_flush()
            mine = []
            while True:
                mine.append(h.collect_mixer_transmissions())
                if not mine[-1]["n_waiting"]:
                    break
            clips.append((mine, h.mixer_spool_counters()))
        B = hs[0].B
        for h in hs:
            h.close()
        q.put(("ok", dict(steps=steps, clips=clips, partial=partial, halves=halves, params=params, B=B)))
    except Exception:  # noqa: BLE001
        import traceback

        q.put(("error", traceback.format_exc()))


@pytest.mark.skipif(not os.path.exists(FAKE_RCCL), reason="tests/fake_rccl/libfake_rccl.so not built")
def test_two_ranks_spool_disjoint_halves_behind_the_exchange(pkg, built, tmp_path):
    """One thread, two handles on one GPU, comm_init_all; per batch one grouped all-reduce, then a manual gate step on each rank.  Every rank holds every sum, so
    both ranks' steps are the same bytes; each spools its half.  The union of the clips is the model's (every mixer spooled) on the exchanged sums."""
    pytest.importorskip("torch")
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_fabric_main, args=(str(tmp_path / "fake_rccl.log"), q))
    p.start()
    status, out = q.get(timeout=500)
    p.join(timeout=120)
    assert status == "ok", out
    assert p.exitcode == 0
    whole = capi.transmission_spool_reference(np.ones(N_FABRIC_MIXERS, bool), out["B"], export_rows=400, **out["params"])
    per_rank = [capi.transmission_spool_reference(h, out["B"], export_rows=400, **out["params"]) for h in out["halves"]]
    for b, (a0, a1) in enumerate(out["steps"]):
        assert a0["n_active"] == a1["n_active"] and a0["mixers"].tolist() == a1["mixers"].tolist() and a0["audio"].tobytes() == a1["audio"].tobytes() and \
            a0["info"].tobytes() == a1["info"].tobytes(), "batch %d: the ranks disagree about the node's rows" % b
        for m in [whole] + per_rank:
            m.step(a0["n_active"], a0["mixers"], a0["audio"], a0["info"])
    assert any(a0["has_signal"][m] and not part[0][m] for (a0, _), part in zip(out["steps"], out["partial"]) for m in range(N_FABRIC_MIXERS)), \
        "no mixer had signal from the other rank alone: a step in front of the exchange would have seen the same"
    whole.flush()
    want = whole.collect()
    assert want["n_waiting"] == 0 and len(want["records"]) >= 4
    union = []
    for r, (mine, counters) in enumerate(out["clips"]):
        per_rank[r].flush()
        for got in mine:
            w = per_rank[r].collect()
            assert got["records"].tobytes() == w["records"].tobytes() and got["audio"].tobytes() == w["audio"], "rank %d" % r
            row = got["audio"].shape[1] if len(got["audio"]) else 0
            for rec in got["records"]:
                assert int(rec["channel"]) % 2 == r
                union.append((int(rec["close_batch"]), int(rec["channel"]), rec, got["audio"][int(rec["row_offset"]):int(rec["row_offset"] + rec["n_rows"])].tobytes()))
        assert counters == per_rank[r].counters()
    union.sort(key=lambda t: t[:2])
    assert len(union) == len(want["records"])
    at = 0
    for (_, _, rec, audio), w in zip(union, want["records"]):
        for f in sc.RECORD_FIELDS[:-1]:
            assert int(rec[f]) == int(w[f]), (f, _brief([rec]), _brief([w]))
        assert rec["reserved"].tolist() == w["reserved"].tolist()
        n = int(w["n_rows"]) * 2 * out["B"]
        assert audio == want["audio"][at:at + n]
        at += n
    assert {int(t[1]) % 2 for t in union} == {0, 1}, "one rank finished nothing"
