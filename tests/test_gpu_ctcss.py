"""The CTCSS chain of csrc/demod.hip on the GPU -- the front kernel's hand-off (packed and generic), tone_kernel, the verdict masks, back_kernel -- at every
standard tone, every tone-bank shape (the (12, 52) banks that fill the wavefront to lane 63 included) and both wave rates: the sweep of helpers.ctcss_sweep_case
(tests/test_ctcss_sweep.py checks its conditions on the CPU) through process_bins against Oracle.run_bins after every batch, bit for bit; the same under the
other launch paths; one case through stage 1; a fuzz over random plans whose targets come from the sweep list."""
import os

import numpy as np
import pytest

import helpers
import pyoracle

pytestmark = pytest.mark.gpu

STATS = ("noise_level", "signal_level", "squelch_level", "agcavgfast", "open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "bin", "squelch_state",
         "signal_outside_filter")


def _what(pkg, m, wave_rate):
    return "target %.1f Hz, sent %.1f Hz (%s), %s%s, bank %s" % (m["target"], m["sent"], m["what"], m["kind"], " + notch" if m["notch"] else "",
                                                                helpers.ctcss_bank_shape(pkg, m["target"], wave_rate))


def _run_sweep(pkg, wave_rate, flags, against_oracle=True):
    """The sweep through one handle; per batch dict(trace, axc, waveout, stats), compared with the oracle on the way."""
    devices, B, n_batches, streams, metas = helpers.ctcss_sweep_case(wave_rate, meta=True)
    meta = [m for part in metas for m in part]
    n_dev = len(devices)
    res = []
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate)
    try:
        with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags | pkg.capi.FLAG_TRACE_SQUELCH) as hip:
            for b in range(n_batches):
                w = np.concatenate([s[0][:, b * B:(b + 1) * B] for s in streams])
                q = np.concatenate([s[1][:, 2 * b * B:2 * (b + 1) * B] for s in streams])
                hip.process_bins(np.ascontiguousarray(w), np.ascontiguousarray(q))
                out = hip.collect(stats=True)
                r = dict(trace=hip.read_trace(), axc=out["axc"], waveout=out["waveout"].view(np.uint32), stats=out["stats"])
                res.append(r)
                if not against_oracle:
                    continue
                want = [orc.run_bins(d, streams[d][0][:, b * B:(b + 1) * B], streams[d][1][:, 2 * b * B:2 * (b + 1) * B]) for d in range(n_dev)]
                for name, ref in (("trace", np.concatenate([x["trace"] for x in want])), ("axc", np.concatenate([x["axc"] for x in want])),
                                  ("waveout", np.concatenate([x["waveout"] for x in want]).view(np.uint32))):
                    bad = np.nonzero((r[name] != ref).reshape(len(meta), -1).any(axis=1))[0]
                    assert len(bad) == 0, "flags 0x%x batch %d: %s differs on %d channels; first, channel %d: %s" % (flags, b, name, len(bad), bad[0], _what(pkg, meta[bad[0]], wave_rate))
                k = 0
                for d in range(n_dev):
                    for j in range(len(devices[d]["channels"])):
                        o = orc.stats(d, j)
                        for f in STATS:
                            assert o[f] == r["stats"][k][f], "flags 0x%x batch %d: %s is %r, the oracle's %r: %s" % (flags, b, f, r["stats"][k][f], o[f], _what(pkg, meta[k], wave_rate))
                        k += 1
    finally:
        orc.close()
    assert sum(s["ctcss_count"] for s in res[-1]["stats"]) > 2 * len(helpers.CTCSS_SWEEP_TARGETS)
    return res, meta


@pytest.mark.parametrize("wave_rate", [16000, 8000])
def test_sweep_equals_the_oracle(pkg, built, wave_rate):
    """Every target of the sweep in ONE handle: squelch trace (tone bit included), axcindicate, audio and every statistic after every batch, bit for bit."""
    _run_sweep(pkg, wave_rate, 0)


def test_sweep_on_the_other_launch_paths(pkg, built):
    """The 16 kHz sweep under FLAG_REGROUP and under FLAG_NO_REGROUP | FLAG_SERIAL_DEMOD -- tone_kernel launched over sub-ranges of the blocks -- equals the plain
    run and the oracle bit for bit.  (process_bins is refused on a FLAG_PIPELINE handle: the pipelined path is covered by the case through stage 1 below.)"""
    capi = pkg.capi
    plain, meta = _run_sweep(pkg, 16000, 0, against_oracle=False)
    for flags in (capi.FLAG_REGROUP, capi.FLAG_NO_REGROUP | capi.FLAG_SERIAL_DEMOD):
        got, _ = _run_sweep(pkg, 16000, flags)
        for b, (x, y) in enumerate(zip(plain, got)):
            for name in ("trace", "axc", "waveout"):
                bad = np.nonzero((x[name] != y[name]).reshape(len(meta), -1).any(axis=1))[0]
                assert len(bad) == 0, "flags 0x%x batch %d: %s differs from the plain run; first, channel %d: %s" % (flags, b, name, bad[0], _what(pkg, meta[bad[0]], 16000))
            assert x["stats"] == y["stats"], (flags, b)


E2E_TARGETS = [33.0, 67.0, 71.9, 98.7, 100.0, 123.0, 150.0, 203.5, 218.1, 241.8, 254.1, 300.0]  # (12, 52) on either side of the list, (10, 48), (11, 48 ... 51)


def test_end_to_end_through_stage_1(pkg, built):
    """Raw u8 I/Q (siggen.make_carrier(kind=1, ctcss_hz=...)) through submit / process at twelve targets, each with a transmitter that sends its tone and one that
    sends the next standard tone: decisions bit-exact, audio within the project's 1e-4 RMS, the bars of test_gpu_parity.py::test_end_to_end_stream.  The same
    stream through a FLAG_PIPELINE handle: bit-identical to the sequential handle's results, one process call later."""
    sg, capi = pkg.siggen, pkg.capi
    wave_rate, n_batches = 16000, 12
    chans, carriers = [], []
    for i, t in enumerate(E2E_TARGETS):
        above = [s for s in helpers.CTCSS_STANDARD_TONES if s > t]
        for sent in (t, min(above) if above else max(helpers.CTCSS_STANDARD_TONES)):
            k = len(chans) % 8
            chans.append(dict(frequency=sg.CENTERFREQ + sg.PLAN_OFFSETS_HZ[k], modulation=1, afc=0, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0,
                              notch_freq=t if i % 3 == 0 else 0.0, notch_q=10.0 if i % 3 == 0 else 0.0, ctcss_freq=t, bandwidth_hz=12500 if i % 2 else 0, ampfactor=1.0,
                              tau_us=-1, has_iq_outputs=0))
            carriers.append(sg.make_carrier(sg.PLAN_OFFSETS_HZ[k], sg.SAMPLE_RATE, kind=1, ctcss_hz=sent, key_slot=k, key_period_s=1.5, key_on_s=1.1, key_slot_s=0.04))
    n_dev = len(chans) // 8
    devices = [dict(channels=chans[8 * d:8 * d + 8]) for d in range(n_dev)]
    nbytes = helpers.stream_bytes(n_batches, wave_rate)
    iq = [sg.generate_u8(d, 0, nbytes // 2, carriers[8 * d:8 * d + 8]) for d in range(n_dev)]
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate)
    ref = [orc.run_device(d, iq[d], n_batches) for d in range(n_dev)]
    assert all(r["n_batches"] == n_batches for r in ref)
    found = [orc.stats(d, j)["ctcss_count"] for d in range(n_dev) for j in range(8)]
    assert sum(c >= 1 for c in found[0::2]) >= 8, found  # the right tone was found at eight targets or more (the oracle counts no window at 33 and 300 Hz on this signal: the sweep covers those)

    def run(flags):
        res = []
        with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags | capi.FLAG_TRACE_SQUELCH) as hip:
            g = hip.geometry
            off = 0
            for k in range(n_batches):
                take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
                lo = off if k == 0 else off + g.lookahead_bytes
                for d in range(n_dev):
                    assert hip.submit(d, iq[d][lo:lo + take]) == take
                off += g.first_batch_bytes if k == 0 else g.batch_bytes
                assert hip.process()
                if not (flags & capi.FLAG_PIPELINE) or k > 0:
                    r = hip.collect(stats=True)
                    r["trace"] = hip.read_trace()
                    res.append(r)
            if flags & capi.FLAG_PIPELINE:
                hip.flush()
                r = hip.collect(stats=True)
                r["trace"] = hip.read_trace()
                res.append(r)
        return res

    seq = run(0)
    for b, r in enumerate(seq):
        assert np.array_equal(r["axc"], np.concatenate([x["axc"][b] for x in ref])), "batch %d: axc" % b
        want_t = np.concatenate([x["trace"][b] for x in ref])
        assert np.array_equal(r["trace"], want_t), "batch %d: squelch trace (channels %s)" % (b, np.nonzero((r["trace"] != want_t).any(axis=1))[0])
        err = helpers.rms(r["waveout"] - np.concatenate([x["waveout"][b] for x in ref]))
        assert err <= 1e-4, "batch %d: audio rms %g" % (b, err)
    k = 0
    for d in range(n_dev):
        for j in range(8):
            o = orc.stats(d, j)
            for f in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "squelch_state"):
                assert o[f] == seq[-1]["stats"][k][f], (d, j, f)
            k += 1
    pip = run(capi.FLAG_PIPELINE | capi.FLAG_NO_REGROUP)
    assert len(pip) == len(seq)
    for b, (x, y) in enumerate(zip(seq, pip)):
        assert np.array_equal(x["trace"], y["trace"]) and np.array_equal(x["axc"], y["axc"]), "pipelined, batch %d" % b
        assert np.array_equal(x["waveout"].view(np.uint32), y["waveout"].view(np.uint32)), "pipelined, batch %d: waveout" % b
        assert x["stats"] == y["stats"], "pipelined, batch %d: statistics" % b
    orc.close()


@pytest.mark.parametrize("seed", range(int(os.environ.get("AIRBAND_FUZZ_SEEDS_CTCSS", "4"))))
def test_random_plans_over_the_sweep_targets(pkg, built, seed):
    """test_gpu_parity.py::test_random_plans_on_the_gpu with the CTCSS targets drawn from the whole sweep list (test_host_wave64.random_scenario(tones=...)):
    squelch trace, axcindicate and audio bit for bit, NaN where the oracle has NaN (AIRBAND_FUZZ_SEEDS_CTCSS=N for more seeds)."""
    from test_host_wave64 import random_scenario
    devices, wave_rate, fm_demod, B, n_batches, streams = random_scenario(seed, max_dev=12, tones=helpers.CTCSS_SWEEP_TARGETS)
    n_dev = len(devices)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fm_demod=fm_demod)
    try:
        with pkg.AirbandHip(devices, wave_rate=wave_rate, fm_demod=fm_demod, flags=pkg.capi.FLAG_TRACE_SQUELCH) as hip:
            for b in range(n_batches):
                w = np.concatenate([s[0][:, b * B:(b + 1) * B] for s in streams])
                q = np.concatenate([s[1][:, 2 * b * B:2 * (b + 1) * B] for s in streams])
                want = [orc.run_bins(d, streams[d][0][:, b * B:(b + 1) * B], streams[d][1][:, 2 * b * B:2 * (b + 1) * B]) for d in range(n_dev)]
                hip.process_bins(np.ascontiguousarray(w), np.ascontiguousarray(q))
                out = hip.collect(iq=True, stats=True)
                tr = hip.read_trace()
                wt = np.concatenate([x["trace"] for x in want])
                assert np.array_equal(tr, wt), "seed %d batch %d: squelch trace (channels %s)" % (seed, b, np.nonzero((tr != wt).any(axis=1))[0])
                assert np.array_equal(out["axc"], np.concatenate([x["axc"] for x in want])), "seed %d batch %d: axc" % (seed, b)
                for key in ("waveout", "iq_out"):
                    ww = np.concatenate([x[key] for x in want])
                    same = (out[key].view(np.uint32) == ww.view(np.uint32)) | (np.isnan(out[key]) & np.isnan(ww))
                    assert same.all(), "seed %d batch %d: %s (channels %s)" % (seed, b, key, np.nonzero((~same).any(axis=1))[0])
            k = 0
            for d in range(n_dev):
                for j in range(len(devices[d]["channels"])):
                    o = orc.stats(d, j)
                    for f in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "squelch_state"):
                        assert o[f] == out["stats"][k][f], (seed, d, j, f, o[f], out["stats"][k][f])
                    k += 1
    finally:
        orc.close()
