"""CTCSS tone detection at every standard tone, every tone-bank shape and both wave rates, on the CPU: the conditions the sweep generator
(helpers.ctcss_sweep_case) has to meet, checked with the oracle alone; the bank shapes params.cpp::build_plan derives for the sweep's targets; the sweep through
the host wavefront emulation of csrc/demod.hip (front kernel -> tone_kernel -> back_kernel), bit for bit against the oracle; and the oracle's CTCSS pinned to the
compiled reference at the off-list targets and at WAVE_RATE 16000.  tests/test_gpu_ctcss.py runs the same streams on the GPU.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import helpers
import pyoracle
import pyref
from test_host_demod import HostDemod, pkg
from test_host_wave64 import wave64  # noqa: F401  (the fixture)
from test_oracle_vs_reference import _reference_run, need_ref
from test_reference_unit_cases import _ctcss_run, _tone

STATS = ("noise_level", "signal_level", "squelch_level", "agcavgfast", "open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "squelch_state")


def _oracle_sweep(wave_rate):
    """The sweep through the oracle alone: (metas flat, traces [C][n], stats per channel)."""
    devices, B, n_batches, streams, metas = helpers.ctcss_sweep_case(wave_rate, meta=True)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate)
    try:
        traces = []
        for d in range(len(devices)):
            w, q = streams[d]
            traces.append(np.concatenate([orc.run_bins(d, w[:, b * B:(b + 1) * B], q[:, 2 * b * B:2 * (b + 1) * B])["trace"] for b in range(n_batches)], axis=1))
        stats = [orc.stats(d, j) for d in range(len(devices)) for j in range(len(devices[d]["channels"]))]
    finally:
        orc.close()
    return [m for part in metas for m in part], np.concatenate(traces), stats


def _tone_drops_with_the_squelch_open(trace):
    """bit 5 (has_tone) 1 -> 0 between two samples at both of which the squelch's state is OPEN (4)."""
    tone, st = (trace >> 5) & 1, trace & 7
    return bool(((tone[:-1] == 1) & (tone[1:] == 0) & (st[:-1] == 4) & (st[1:] == 4)).any())


@pytest.mark.parametrize("wave_rate", [16000, 8000])
def test_the_sweep_meets_its_conditions(built, wave_rate):
    """Conditions on the generator's streams, with the oracle as the only judge: every target has a channel on which the right tone was found in two or more
    windows, one with a window in which it was not, and one on which the fast detector says yes and the slow one overrules it while the squelch is open; no
    channel without a tone ever finds one.  NO TARGET IS EXEMPT from the third condition: where no standard tone shares the target's fast bin from 5 Hz or more
    away (67.0, 69.3, 250.3, 254.1 and the targets far from the list) the `switch` transmission of helpers.ctcss_sweep_plan stands in for the neighbour."""
    meta, trace, stats = _oracle_sweep(wave_rate)
    assert len(meta) > 200
    found, missed, dropped = set(), set(), set()
    for m, tr, st in zip(meta, trace, stats):
        assert st["open_count"] >= m["keys"], (m, st)  # the squelch did open for every transmission
        if m["what"] == "target" and st["ctcss_count"] >= 2:
            found.add(m["target"])
        if st["no_ctcss_count"] >= 1:
            missed.add(m["target"])
        if _tone_drops_with_the_squelch_open(tr):
            dropped.add(m["target"])
        if m["what"] == "none":
            assert st["ctcss_count"] == 0, (m, st)
        if m["what"] in ("decoy", "switch"):
            assert _tone_drops_with_the_squelch_open(tr), m
    every = set(helpers.CTCSS_SWEEP_TARGETS)
    assert found == every, sorted(every - found)
    assert missed == every, sorted(every - missed)
    assert dropped == every, sorted(every - dropped)
    assert sum(m["keys"] == 2 for m in meta) >= 20
    if wave_rate == 16000:  # more than one 64-slot block of the packed kind and of the generic kind, and a partly filled one of each
        packed = sum(m["kind"] == "nfm" for m in meta)
        generic = len(meta) - packed
        assert packed > 64 and packed % 64 and generic > 64 and generic % 64 and {m["kind"] for m in meta} == {"nfm", "nfm_lp", "am"}
    else:
        assert {m["kind"] for m in meta} == {"am"}


def test_bank_shapes_of_the_sweep(built):
    """The tone-bank sizes (fast, slow) that params.cpp::build_plan derives for the sweep's targets, read from the library: every shape the issue names occurs --
    (12, 52) far from the list on either side, (10, 48) for 71.9, (11, k) for k = 48 ... 52 -- n0 + n1 never exceeds 64 and reaches it, and the two wave rates
    agree (both windows scale with the rate).  tone_kernel's side-by-side lane layout (`merged`) is therefore the only one build_plan leads to, and (12, 52)
    fills the wavefront to its last lane."""
    L = pyoracle.lib()

    def restated(t, rate, win):
        """CTCSS's bank (src/ctcss.cpp:105-122) from the reference's tone list and the oracle's coefficient function: the target, then every standard tone 5 Hz or more away,
        a coefficient once.  A wrong entry in the library's own copy of the list changes a count somewhere."""
        coeff = [L.orc_tone_coeff(t, float(rate), win)]
        for s in helpers.CTCSS_STANDARD_TONES:
            c = L.orc_tone_coeff(s, float(rate), win)
            if abs(np.float32(t) - np.float32(s)) >= 5 and c not in coeff:
                coeff.append(c)
        return len(coeff)

    shapes = {}
    for rate in (16000, 8000):
        for t in helpers.CTCSS_SWEEP_TARGETS:
            s = helpers.ctcss_bank_shape(pkg, t, rate)
            assert s == (restated(t, rate, int(rate * 0.05)), restated(t, rate, int(rate * 0.4))), (t, rate, s)
            assert s == shapes.setdefault(t, s), (t, rate, s, shapes[t])
            assert s[0] + s[1] <= 64, (t, s)
    have = set(shapes.values())
    assert {(12, 52), (10, 48)} | {(11, k) for k in range(48, 53)} <= have, sorted(have)
    assert max(a + b for a, b in have) == 64
    assert shapes[33.0] == shapes[300.0] == (12, 52) and shapes[71.9] == (10, 48) and shapes[60.0] == (11, 52) and shapes[98.7] == (11, 48)
    # any target at all: at most 12 distinct fast bins and 52 distinct slow ones (the target's and one per standard tone, fewer where tones share a bin)
    rng = np.random.default_rng(64)
    for t in [1.0, 10.0, 45.0, 64.9, 500.0, 1000.0, 3999.0] + [float(x) for x in rng.uniform(20.0, 400.0, 60)]:
        s = helpers.ctcss_bank_shape(pkg, t, 16000)
        assert s[0] <= 12 and s[1] <= 52, (t, s)


@pytest.mark.parametrize("mode", [0, 1], ids=["slot_order", "regrouped"])
@pytest.mark.parametrize("wave_rate", [16000, 8000])
def test_sweep_with_wavefront_semantics(wave64, monkeypatch, wave_rate, mode):  # noqa: F811
    """The sweep through csrc/demod.hip compiled for the host with wavefront semantics (tests/test_host_wave64.py): squelch trace (tone bit included), axcindicate,
    audio after every batch and every statistic at the end equal the oracle's bit for bit."""
    if mode:
        monkeypatch.setenv("AB_HOST_REGROUP", str(mode))
    else:
        monkeypatch.delenv("AB_HOST_REGROUP", raising=False)
    devices, B, n_batches, streams, metas = helpers.ctcss_sweep_case(wave_rate, meta=True)
    meta = [m for part in metas for m in part]
    n_dev = len(devices)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate)
    hd = HostDemod(wave64, devices, wave_rate)
    try:
        assert hd.B == B
        for b in range(n_batches):
            w = np.concatenate([s[0][:, b * B:(b + 1) * B] for s in streams])
            q = np.concatenate([s[1][:, 2 * b * B:2 * (b + 1) * B] for s in streams])
            want = [orc.run_bins(d, streams[d][0][:, b * B:(b + 1) * B], streams[d][1][:, 2 * b * B:2 * (b + 1) * B]) for d in range(n_dev)]
            hd.process_bins(w, q)
            got_w, got_a, got_t = hd.collect()
            for name, got, ref in (("trace", got_t, np.concatenate([x["trace"] for x in want])), ("axc", got_a, np.concatenate([x["axc"] for x in want])),
                                   ("waveout", got_w.view(np.uint32), np.concatenate([x["waveout"] for x in want]).view(np.uint32))):
                bad = np.nonzero((got != ref).reshape(len(meta), -1).any(axis=1))[0]
                assert len(bad) == 0, "batch %d: %s differs on %d channels, first %d: %s" % (b, name, len(bad), bad[0], meta[bad[0]])
        st = hd.stats()
        k = 0
        for d in range(n_dev):
            for j in range(len(devices[d]["channels"])):
                o = orc.stats(d, j)
                for f in STATS:
                    assert o[f] == st[k][f], (meta[k], f, o[f], st[k][f])
                k += 1
    finally:
        hd.close()
        orc.close()


IMPLS_REF = pytest.mark.skipif(not pyref.have_ref(False), reason="oracle/_ref not built")


@IMPLS_REF
@pytest.mark.parametrize("rate,window", [(16000.0, 800), (16000.0, 6400), (8000.0, 400), (8000.0, 3200)])
def test_oracle_ctcss_is_the_reference_at_every_bank_shape(built, rate, window):
    """orc_ctcss_run against the reference's CTCSS class (refh_ctcss_run), sample by sample: has_tone and enough_samples after every sample of three windows, for the
    off-list targets (banks of 12 / 52 tones, nothing left out) and a spread of standard ones, fed the target, a near tone, a far tone and noise.  WAVE_RATE 16000
    with both of its windows was not pinned before (only 8 kHz with the 0.4 s window)."""
    rng = np.random.default_rng(int(rate) + window)
    n = 3 * window + 17
    verdicts = set()
    for target in helpers.CTCSS_OFFLIST_TARGETS + [1000.0, 71.9, 218.1, 241.8] + helpers.CTCSS_STANDARD_TONES[::6]:
        for sent in (target, target + 3.1, target * 1.2 + 9.0, 0.0):
            x = (_tone(sent, n, rate=rate) if sent else np.zeros(n, np.float32)) + (0.02 * rng.standard_normal(n)).astype(np.float32)
            a, b = _ctcss_run("oracle", target, rate, window, x), _ctcss_run("reference", target, rate, window, x)
            assert np.array_equal(a, b), (target, sent, int(np.argmax(a != b)))
            assert a[-1] & 2
            verdicts.add(int(a[-1] & 1))
    assert verdicts == {0, 1}


def sweep_plan_case(pkg, seed):
    """test_oracle_vs_reference.random_plan_case with the CTCSS targets drawn from the whole sweep list -- every bank shape -- and the sub-tone sent on most FM
    channels: right, the next standard tone, or a standard tone further away."""
    sg = pkg.siggen
    rng = np.random.default_rng(62_000 + seed)
    nfm_build = bool(seed % 4)
    wave_rate = 16000 if nfm_build else 8000
    fm_demod = int(rng.integers(0, 2)) if nfm_build else 0
    chans, carriers = [], []
    for k, off in enumerate(sg.PLAN_OFFSETS_HZ):
        c = dict(frequency=sg.CENTERFREQ + off, modulation=0, afc=0, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0, ctcss_freq=0.0,
                 bandwidth_hz=0, ampfactor=1.0, tau_us=-1, has_iq_outputs=0)
        if nfm_build and rng.random() < 0.75:
            c["modulation"] = 1
            c["tau_us"] = int(rng.choice([-1, 0, 50, 200]))
        if rng.random() < 0.3:
            c["bandwidth_hz"] = int(rng.choice([6250, 12500]))
        if rng.random() < 0.8:
            c["ctcss_freq"] = float(rng.choice(helpers.CTCSS_SWEEP_TARGETS))
        if rng.random() < 0.3:
            c["notch_freq"], c["notch_q"] = float(c["ctcss_freq"] or 100.0), 10.0
        chans.append(c)
        tone = rng.random()
        ct = c["ctcss_freq"] if tone < 0.5 else (float(rng.choice(helpers.CTCSS_STANDARD_TONES)) if tone < 0.85 else 0.0)
        period, on = [(2.0, 1.7), (1.5, 0.75), (0.5, 0.3)][int(rng.integers(0, 3))]
        carriers.append(sg.make_carrier(off, sg.SAMPLE_RATE, amplitude=float(rng.choice([0.08, 0.05, 0.03])), kind=c["modulation"], ctcss_hz=ct if c["modulation"] == 1 else 0.0,
                                        key_slot=k, key_period_s=period, key_on_s=on, key_slot_s=0.04))
    return dict(channels=chans), carriers, wave_rate, fm_demod, 8


@need_ref
@pytest.mark.parametrize("seed", range(int(os.environ.get("AIRBAND_FUZZ_SEEDS_ORACLE_CTCSS", "4"))))
def test_oracle_is_the_reference_on_plans_over_the_sweep_targets(built, seed):
    """The twin of test_oracle_vs_reference.py::test_oracle_is_the_reference_on_random_plans with targets from the whole sweep list: whole streams through the
    reference's demodulate() and through the oracle, audio, axcindicate and every statistic (CTCSS counters included) bit for bit."""
    device, carriers, wave_rate, fm_demod, n_batches = sweep_plan_case(pkg, seed)
    iq = pkg.siggen.generate_u8(seed, 0, helpers.stream_bytes(n_batches, wave_rate) // 2, carriers)
    ref = _reference_run([device], [iq], n_batches, nfm=wave_rate == 16000, fm_demod=fm_demod)[0]
    orc = pyoracle.Oracle([device], wave_rate=wave_rate, fm_demod=fm_demod)
    try:
        got = orc.run_device(0, iq, n_batches)
        assert ref["n_batches"] == got["n_batches"] == n_batches
        assert np.array_equal(ref["axc"], got["axc"]), "seed %d: axcindicate" % seed
        assert np.array_equal(ref["waveout"].view(np.uint32), got["waveout"].view(np.uint32)), "seed %d: waveout" % seed
        for j in range(8):
            a, b = ref["stats"][j], orc.stats(0, j)
            for k in a:
                if k != "squelch_state":
                    assert a[k] == b[k], (seed, j, k, a[k], b[k])
    finally:
        orc.close()
