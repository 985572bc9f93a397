"""Scan-mode devices on the GPU (airband_hip_prepare_scan / set_freq_index / freq_stats).

Ground truth is a composition of per-entry oracles: one pyoracle.Oracle per list entry, configured as that entry at entry 0's frequency, and batch b
goes through the oracle of the entry that is active in b.  That equals the reference wherever the channel's shared state (wavein / waveout carry)
cannot differ, which the bins fed here make hold: every batch ends on one fixed quiet tail, and every entry is CLOSED at the end of every batch
(asserted from the oracle traces)."""
import numpy as np
import pytest

import helpers
import pyoracle

pytestmark = pytest.mark.gpu

F0 = 120_100_000


def _entry(**kw):
    e = dict(frequency=F0, modulation=0)
    e.update(kw)
    return e


def _bins(B, n_batches, seed, keyed):
    """Synthetic stage-1 output of one channel: complex noise, a carrier keyed on in [on0, on1) of the batches listed in `keyed` (batch -> (on0, on1)),
    and one fixed quiet tail over the last AGC_EXTRA rows of every batch.  |bin| in float32 as the reference computes it from the two floats."""
    rng = np.random.default_rng(seed)
    tail = (rng.standard_normal(200) * 0.7).astype(np.float32).reshape(100, 2)
    out = []
    for b in range(n_batches):
        z = (rng.standard_normal((B, 2)) * 0.7).astype(np.float32)
        if b in keyed:
            on0, on1, amp = keyed[b]
            ph = rng.uniform(0, 2 * np.pi) + 0.3 * np.arange(on1 - on0)
            z[on0:on1, 0] += (amp * np.cos(ph)).astype(np.float32)
            z[on0:on1, 1] += (amp * np.sin(ph)).astype(np.float32)
        z[-100:] = tail
        re, im = z[:, 0], z[:, 1]
        mag = np.sqrt(re * re + im * im).astype(np.float32)
        out.append((mag[None, :], np.ascontiguousarray(z.reshape(1, 2 * B))))
    return out


def _warm(hip, orcs, B):
    """One quiet batch through every entry, on the GPU (switching through the list) and in every entry's oracle: from then on the waveout carry an
    oracle holds is what the channel holds, the zeros of a closed squelch -- not the config-time prefill of an oracle that has not run yet."""
    quiet = _bins(B, 1, 99, {})[0]
    for f, o in enumerate(orcs):
        hip.set_freq_index(0, f)
        w = o.run_bins(0, *quiet)
        assert not (w["trace"][0] & 7).any()
        hip.process_bins(*quiet)
        hip.collect()


def _compare_batch(b, got, trace, want, st_got, st_want):
    assert np.array_equal(trace[0], want["trace"][0]), "batch %d: squelch trace" % b
    assert got["axc"][0] == want["axc"][0], "batch %d: axc" % b
    assert np.array_equal(got["waveout"][0].view(np.uint32), want["waveout"][0].view(np.uint32)), "batch %d: waveout" % b
    assert np.array_equal(got["iq_out"][0].view(np.uint32), want["iq_out"][0].view(np.uint32)), "batch %d: iq_out" % b
    assert st_got == st_want, "batch %d: stats %s != %s" % (b, st_got, st_want)


AM_LISTS = {
    "am": [_entry(), _entry(frequency=F0 + 25_000, squelch_snr_threshold_db=12.0, ampfactor=0.7),
           _entry(frequency=F0 + 50_000, notch_freq=1000.0, ampfactor=1.8), _entry(frequency=F0 + 75_000, squelch_snr_threshold_db=6.0)],
    "generic": [_entry(), _entry(frequency=F0 + 25_000, ctcss_freq=88.5), _entry(frequency=F0 + 50_000, squelch_snr_threshold_db=8.0, notch_freq=800.0),
                _entry(frequency=F0 + 62_500, squelch_threshold_dbfs=-5)],  # a manual squelch level of about 10 (AB_F_MANUAL, sq_manual_level)
}


@pytest.mark.parametrize("kind", sorted(AM_LISTS))
def test_am_lists_match_the_composition_of_per_entry_oracles(pkg, built, kind):
    capi = pkg.capi
    entries = AM_LISTS[kind]
    n = len(entries)
    wave_rate = 8000
    n_batches = 14
    rng = np.random.default_rng(7)
    sched = [0, 0, 1, 1, 0, 2] + [int(x) for x in rng.integers(0, n, n_batches - 6)]
    sched[9] = sched[7]  # away and back
    keyed = {b: (150, 450, 25.0) for b in range(n_batches) if b % 3 != 2}
    bins = _bins(1000, n_batches, 11, keyed)
    dev = [dict(channels=[entries[0]])]
    orcs = [pyoracle.Oracle([dict(channels=[dict(e, frequency=entries[0]["frequency"])])], wave_rate=wave_rate) for e in entries]  # at entry 0's frequency
    with pkg.AirbandHip(dev, wave_rate=wave_rate, flags=capi.FLAG_TRACE_SQUELCH, scan={0: entries}) as hip:
        _warm(hip, orcs, 1000)
        for b in range(n_batches):
            f = sched[b]
            hip.set_freq_index(0, f)
            want = orcs[f].run_bins(0, *bins[b])
            assert want["trace"][0][-1] & 7 == 0, "precondition: entry %d CLOSED at the end of batch %d" % (f, b)
            hip.process_bins(*bins[b])
            got = hip.collect(iq=True, stats=True)
            _compare_batch(b, got, hip.read_trace(), want, got["stats"][0], orcs[f].stats(0, 0))
            for g in range(n):  # every entry, the inactive ones frozen
                assert hip.freq_stats(0, g) == orcs[g].stats(0, 0), "batch %d: freq_stats of entry %d" % (b, g)
        opened = [orcs[g].stats(0, 0)["open_count"] for g in range(n)]
        assert sum(1 for o in opened if o > 0) >= 2, opened


def test_nfm_and_mixed_lists_one_opener(pkg, built):
    """NFM entries with lowpass, CTCSS, notch and tau beside AM entries: the kinds merge to the generic one, the channel needs raw I/Q.  Only entry 1
    (plain NFM) ever sees a carrier; every other entry stays CLOSED throughout."""
    wave_rate = 16000
    entries = [_entry(modulation=0, squelch_snr_threshold_db=9.0), _entry(frequency=F0 + 12_500, modulation=1),
               _entry(frequency=F0 + 25_000, modulation=1, bandwidth_hz=8000, ctcss_freq=100.0),
               _entry(frequency=F0 + 37_500, modulation=1, notch_freq=900.0), _entry(frequency=F0 + 50_000, modulation=0, notch_freq=1200.0)]
    n = len(entries)
    n_batches = 10
    sched = [1, 0, 1, 2, 3, 1, 4, 2, 1, 0]
    keyed = {b: (300, 900, 30.0) for b in range(n_batches) if sched[b] == 1}
    bins = _bins(2000, n_batches, 5, keyed)
    # the reference's NFM channels have needs_raw_iq, so every entry's oracle does (and so does the scan channel): the AM entries see the same derotated input
    orcs = [pyoracle.Oracle([dict(channels=[dict(e, frequency=entries[0]["frequency"])])], wave_rate=wave_rate) for e in entries]  # at entry 0's frequency
    with pkg.AirbandHip([dict(channels=[entries[0]])], wave_rate=wave_rate, flags=pkg.capi.FLAG_TRACE_SQUELCH, scan={0: entries}) as hip:
        _warm(hip, orcs, 2000)
        for b in range(n_batches):
            f = sched[b]
            hip.set_freq_index(0, f)
            want = orcs[f].run_bins(0, *bins[b])
            assert want["trace"][0][-1] & 7 == 0
            if f != 1:
                assert not (want["trace"][0] & 7).any(), "entry %d must stay CLOSED" % f
            hip.process_bins(*bins[b])
            got = hip.collect(iq=True, stats=True)
            tr = hip.read_trace()
            assert np.array_equal(tr[0], want["trace"][0]), b
            assert got["axc"][0] == want["axc"][0], b
            assert np.array_equal(got["waveout"][0].view(np.uint32), want["waveout"][0].view(np.uint32)), b
            assert np.array_equal(got["iq_out"][0].view(np.uint32), want["iq_out"][0].view(np.uint32)), b
            assert got["stats"][0] == orcs[f].stats(0, 0), b
            for g in range(n):
                assert hip.freq_stats(0, g) == orcs[g].stats(0, 0), (b, g)
        assert orcs[1].stats(0, 0)["open_count"] > 0


def _run_process(pkg, devices, iq, n_batches, scan, flags, sched=None, dev=None, wave_rate=8000):
    """Raw I/Q through the host-ring path; sched[b] is set for scan device `dev` before batch b is enqueued.  Returns per-batch results."""
    capi = pkg.capi
    res = []
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags | capi.FLAG_TRACE_SQUELCH, scan=scan) as hip:
        g = hip.geometry
        pipelined = bool(flags & capi.FLAG_PIPELINE)
        off = 0

        def grab():
            r = hip.collect(iq=True, stats=True)
            r["trace"] = hip.read_trace()
            r["fs"] = [[hip.freq_stats(d, f) for f in range(len(scan[d]))] for d in sorted(scan)] if scan else []
            res.append(r)

        for k in range(n_batches):
            take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
            lo = off if k == 0 else off + g.lookahead_bytes
            for d in range(len(devices)):
                assert hip.submit(d, iq[d][lo:lo + take]) == take
            off += g.first_batch_bytes if k == 0 else g.batch_bytes
            if sched is not None:
                hip.set_freq_index(dev, sched[k])
            assert hip.process()
            if not pipelined:
                grab()
            elif k > 0:  # the batch before, whose stage 2 this call enqueued
                grab()
        if pipelined:
            hip.flush()
            grab()
    return res


def _plan_case(pkg, wave_rate, n_batches, sfmt=None):
    """The BASELINE channel plan on one dongle (helpers.format_case): its channels, the device's other settings, the stream as bytes."""
    devices, iq = helpers.format_case(pkg, pkg.capi.SFMT_U8 if sfmt is None else sfmt, 9, 2_560_000, wave_rate, 1, n_batches)
    dev = {k: v for k, v in devices[0].items() if k != "channels"}
    return devices[0]["channels"], np.ascontiguousarray(iq[0]).view(np.uint8), dev


def _same(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x["waveout"].view(np.uint32), y["waveout"].view(np.uint32)), (what, k, "waveout")
        assert np.array_equal(x["iq_out"].view(np.uint32), y["iq_out"].view(np.uint32)), (what, k, "iq_out")
        assert np.array_equal(x["axc"], y["axc"]), (what, k, "axc")
        assert np.array_equal(x["trace"], y["trace"]), (what, k, "trace")
        assert x["stats"] == y["stats"], (what, k, "stats")
        assert x["fs"] == y["fs"], (what, k, "freq_stats")


@pytest.mark.parametrize("wave_rate,fmt", [(8000, "u8"), (16000, "u8"), (16000, "cs16")])
def test_lists_that_never_switch_equal_the_handle_without_them(pkg, built, wave_rate, fmt):
    """A multichannel dongle plus two one-channel dongles on the same stream; scan lists of 1 and 3 entries whose index stays 0 are bit-identical to
    the same handle without scan lists.  The entries that never ran report their initial state (a fresh oracle of the entry)."""
    n_batches = 4
    chans, iq, dev = _plan_case(pkg, wave_rate, n_batches, pkg.capi.SFMT_S16 if fmt == "cs16" else None)
    c1, c2 = dict(chans[1]), dict(chans[3])
    devices = [dict(dev, channels=chans), dict(dev, channels=[c1]), dict(dev, channels=[c2])]
    extra = [dict(c2, squelch_snr_threshold_db=15.0), dict(c2, ampfactor=0.25, frequency=c2["frequency"] + 25_000)]
    scan = {1: [c1], 2: [c2] + extra}
    plain = _run_process(pkg, devices, [iq] * 3, n_batches, None, pkg.capi.FLAG_NO_REGROUP, wave_rate=wave_rate)
    with_lists = _run_process(pkg, devices, [iq] * 3, n_batches, scan, pkg.capi.FLAG_NO_REGROUP, wave_rate=wave_rate)
    for x in plain:
        x["fs"] = None
    fs = [x.pop("fs") for x in with_lists]
    for x in with_lists:
        x["fs"] = None
    _same(plain, with_lists, "no scan lists vs lists at index 0")
    assert sum(s["open_count"] for s in plain[-1]["stats"]) > 0
    fresh = [pyoracle.Oracle([dict(dev, channels=[dict(e, frequency=c2["frequency"])])], wave_rate=wave_rate).stats(0, 0) for e in extra]
    for k, x in enumerate(with_lists):  # the active entry's freq_stats is its collect row, the others never ran
        assert fs[k][0][0] == x["stats"][8]
        assert fs[k][1][0] == x["stats"][9]
        assert fs[k][1][1:] == fresh


@pytest.mark.parametrize("mixed", [False, True])
def test_every_schedule_equals_the_sequential_run(pkg, built, mixed):
    """The same seeded schedule (switching away and back) under REGROUP, NO_REGROUP + SERIAL_DEMOD and PIPELINE is bit-identical to the sequential
    NO_REGROUP run.  Under PIPELINE the index is set between the process() calls: stage 2 of a batch must use the index latched when it was enqueued."""
    capi = pkg.capi
    wave_rate = 16000 if mixed else 8000
    n_batches = 8
    chans, iq, dev = _plan_case(pkg, wave_rate, n_batches)
    base = dict(chans[0])
    if mixed:
        entries = [base, dict(base, modulation=1, frequency=base["frequency"] + 12_500), dict(base, modulation=1, bandwidth_hz=6000),
                   dict(base, squelch_snr_threshold_db=6.0, notch_freq=1000.0)]
    else:
        entries = [base, dict(base, squelch_snr_threshold_db=12.0, ampfactor=0.6), dict(base, notch_freq=1000.0), dict(base, ctcss_freq=100.0)]
    devices = [dict(channels=chans), dict(channels=[base]), dict(channels=[dict(chans[2])])]
    scan = {1: entries}
    rng = np.random.default_rng(3)
    sched = [0, 1, 1, 0] + [int(x) for x in rng.integers(0, len(entries), n_batches - 4)]
    ref = _run_process(pkg, devices, [iq] * 3, n_batches, scan, capi.FLAG_NO_REGROUP, sched, 1, wave_rate)
    assert any(r["axc"][8] != ord(" ") for r in ref)
    for flags in (capi.FLAG_REGROUP, capi.FLAG_NO_REGROUP | capi.FLAG_SERIAL_DEMOD, capi.FLAG_PIPELINE | capi.FLAG_NO_REGROUP):
        got = _run_process(pkg, devices, [iq] * 3, n_batches, scan, flags, sched, 1, wave_rate)
        _same(ref, got, "flags 0x%x" % flags)


def test_set_freq_index_errors_on_a_live_handle(pkg, built):
    capi = pkg.capi
    e0 = _entry()
    devs = [dict(channels=[e0, _entry(frequency=F0 + 25_000)]), dict(channels=[e0])]
    with pkg.AirbandHip(devs, wave_rate=8000, scan={1: [e0, _entry(frequency=F0 + 50_000, ampfactor=2.0)]}) as hip:
        for dev, f in ((0, 0), (1, 2), (1, -1), (5, 0)):
            with pytest.raises(pkg.AirbandError) as e:
                hip.set_freq_index(dev, f)
            assert e.value.code == capi.EINVAL
            with pytest.raises(pkg.AirbandError) as e:
                hip.freq_stats(dev, f)
            assert e.value.code == capi.EINVAL
        # nothing changed: the list still runs entry 0, bit-identical to a handle whose list was never touched
        B = hip.B
        z = np.zeros((3, B), np.float32) + 1.0
        q = np.zeros((3, 2 * B), np.float32)
        hip.process_bins(z, q)
        a = hip.collect(stats=True)
        with pkg.AirbandHip(devs, wave_rate=8000, scan={1: [e0, _entry(frequency=F0 + 50_000, ampfactor=2.0)]}) as fresh:
            fresh.process_bins(z, q)
            b = fresh.collect(stats=True)
        assert a["stats"] == b["stats"] and np.array_equal(a["waveout"], b["waveout"])
        assert hip.freq_stats(1, 0) == a["stats"][2]


def test_shared_channel_state_two_nfm_openers(pkg, built):
    """Two NFM entries (no lowpass, no CTCSS) that both open, one after the other.  The FM discriminator's history (pr, pj) and the de-emphasis'
    prev_waveout belong to the channel (src/rtl_airband.cpp:565-579): when the second entry opens it carries on from what the first one left, where
    a private-state composition starts from its own.  So trace, axc and the squelch statistics stay bit-exact with the composition throughout, waveout
    up to the second opener's first audio sample, and that sample DIFFERS; over the opening the difference decays with the de-emphasis."""
    wave_rate = 16000
    entries = [_entry(modulation=1), _entry(frequency=F0 + 12_500, modulation=1, squelch_snr_threshold_db=6.0)]
    sched = [0, 0, 1, 1]
    keyed = {1: (300, 900, 30.0), 3: (400, 1000, 30.0)}
    bins = _bins(2000, len(sched), 21, keyed)
    orcs = [pyoracle.Oracle([dict(channels=[dict(e, frequency=F0)])], wave_rate=wave_rate) for e in entries]
    squelch_keys = [k for k in orcs[0].stats(0, 0) if k != "agcavgfast"]  # agcavgfast is the NFM DC blocker: it is fed the discriminator output
    with pkg.AirbandHip([dict(channels=[entries[0]])], wave_rate=wave_rate, flags=pkg.capi.FLAG_TRACE_SQUELCH, scan={0: entries}) as hip:
        _warm(hip, orcs, 2000)
        for b, f in enumerate(sched):
            hip.set_freq_index(0, f)
            want = orcs[f].run_bins(0, *bins[b])
            assert want["trace"][0][-1] & 7 == 0
            hip.process_bins(*bins[b])
            got = hip.collect(iq=True, stats=True)
            assert np.array_equal(hip.read_trace()[0], want["trace"][0]), b
            assert got["axc"][0] == want["axc"][0], b
            st, so = got["stats"][0], orcs[f].stats(0, 0)
            assert {k: st[k] for k in squelch_keys} == {k: so[k] for k in squelch_keys}, b
            gw, ww = got["waveout"][0], want["waveout"][0]
            if b < 3:
                assert np.array_equal(gw.view(np.uint32), ww.view(np.uint32)), b
                assert st == so
                continue
            # batch 3: the second opener.  Audio of batch sample t sits at waveout[AGC_EXTRA + t] (the row starts with the previous batch's tail)
            audio = np.nonzero(want["trace"][0] & 0x10)[0]
            assert audio.size > 0
            first = 100 + int(audio[0])
            assert np.array_equal(gw[:first].view(np.uint32), ww[:first].view(np.uint32))
            assert gw[first] != ww[first], "the second opener must carry on from the channel's discriminator history, not its own"
            d = (gw[first:] - ww[first:]).astype(np.float64)
            rms = float(np.sqrt(np.mean(d * d)))
            print("second NFM opener: first-sample difference %.3e, RMS difference over the opening %.3e" % (abs(d[0]), rms))
            assert rms <= RMS_SHARED_STATE, rms
        assert orcs[0].stats(0, 0)["open_count"] > 0 and orcs[1].stats(0, 0)["open_count"] > 0


RMS_SHARED_STATE = 2e-2  # measured on an MI355X: 1.85e-2 (first sample 0.45 apart, then the de-emphasis lets it decay)


_FLEET_LISTS = [
    [dict(), dict(squelch_snr_threshold_db=12.0, ampfactor=0.7), dict(notch_freq=1000.0, ampfactor=1.8), dict(squelch_snr_threshold_db=6.0)],
    [dict(), dict(ctcss_freq=88.5), dict(squelch_threshold_dbfs=-5), dict(squelch_snr_threshold_db=8.0, notch_freq=800.0)],
]


def _fleet_bins(rng, n_ch, B, key, tail):
    """Stage-1 rows of n_ch channels for one batch (as _bins, vectorised): a carrier on rows [150, 450) where key is set, one fixed quiet tail."""
    z = rng.standard_normal((n_ch, B, 2), dtype=np.float32) * np.float32(0.7)
    idx = np.nonzero(key)[0]
    if idx.size:
        ph = rng.uniform(0, 2 * np.pi, (idx.size, 1)) + 0.3 * np.arange(300)
        z[idx, 150:450, 0] += (25.0 * np.cos(ph)).astype(np.float32)
        z[idx, 150:450, 1] += (25.0 * np.sin(ph)).astype(np.float32)
    z[:, -100:] = tail
    re, im = z[..., 0], z[..., 1]
    return np.sqrt(re * re + im * im).astype(np.float32), np.ascontiguousarray(z.reshape(n_ch, 2 * B))


def _fleet(pkg, n_multi, lengths, n_sample, n_batches=8, seed=1):
    """n_multi multichannel dongles of 8 AM channels, then len(lengths) scan dongles with lists of those lengths, in ONE handle.  Per-dongle seeded
    schedules, and one batch in which every scan dongle switches.  Sampled scan dongles against per-entry oracles (every entry's freq_stats after every
    batch), the multichannel dongles against the same handle without scan lists."""
    capi = pkg.capi
    B, wave_rate = 1000, 8000
    n_scan = len(lengths)
    lists = []
    for s, n in enumerate(lengths):
        f0 = F0 + 12_500 * (s % 8)
        lists.append([_entry(frequency=f0 + 25_000 * k, **_FLEET_LISTS[s % 2][k % 4]) if k else _entry(frequency=f0) for k in range(n)])
    multi = [dict(channels=[_entry(frequency=F0 + 12_500 * j) for j in range(8)]) for _ in range(n_multi)]
    devices = multi + [dict(channels=[lst[0]]) for lst in lists]
    scan = {n_multi + s: lists[s] for s in range(n_scan)}
    n_ch = 8 * n_multi + n_scan
    ext0 = 8 * n_multi
    rng = np.random.default_rng(seed)
    sched = np.zeros((n_scan, n_batches), np.int64)
    for s, n in enumerate(lengths):
        r = np.random.default_rng(1000 + s)
        sched[s] = r.integers(0, n, n_batches)
    k_all = n_batches // 2
    switching = [s for s, n in enumerate(lengths) if n > 1]
    for s in switching:
        sched[s, k_all] = (sched[s, k_all - 1] + 1 + rng.integers(0, lengths[s] - 1)) % lengths[s]
    sample = sorted(set(np.linspace(0, n_scan - 1, n_sample).astype(int).tolist()))
    orcs = {s: [pyoracle.Oracle([dict(channels=[dict(e, frequency=lists[s][0]["frequency"])])], wave_rate=wave_rate) for e in lists[s]] for s in sample}
    tail = (rng.standard_normal((100, 2)) * 0.7).astype(np.float32)
    flags = capi.FLAG_TRACE_SQUELCH
    opened = 0
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as hip, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags) as plain:
        # warm-up: every entry of every list sees one quiet batch (entry 0 of shorter lists several), in the oracles too
        quiet = _fleet_bins(np.random.default_rng(99), 1, B, np.zeros(1, bool), tail)
        qw, qi = np.repeat(quiet[0], n_ch, 0), np.repeat(quiet[1], n_ch, 0)
        for w in range(max(lengths)):
            for s, n in enumerate(lengths):
                hip.set_freq_index(n_multi + s, w if w < n else 0)
            for s in sample:
                orcs[s][w if w < lengths[s] else 0].run_bins(0, quiet[0], quiet[1])
            hip.process_bins(qw, qi)
            plain.process_bins(qw, qi)
            hip.collect()
            plain.collect()
        for b in range(n_batches):
            key = rng.random(n_ch) < 0.6
            wavein, iqin = _fleet_bins(rng, n_ch, B, key, tail)
            for s in range(n_scan):
                hip.set_freq_index(n_multi + s, int(sched[s, b]))
            hip.process_bins(wavein, iqin)
            plain.process_bins(wavein, iqin)
            got, ref = hip.collect(iq=True, stats=True), plain.collect(iq=True, stats=True)
            tr, tr_ref = hip.read_trace(), plain.read_trace()
            m = slice(0, ext0)
            assert np.array_equal(got["waveout"][m].view(np.uint32), ref["waveout"][m].view(np.uint32)), b
            assert np.array_equal(got["axc"][m], ref["axc"][m]) and np.array_equal(tr[m], tr_ref[m]), b
            assert got["stats"][:ext0] == ref["stats"][:ext0], b
            for s in sample:
                c, f = ext0 + s, int(sched[s, b])
                want = orcs[s][f].run_bins(0, wavein[c][None], iqin[c][None])
                assert want["trace"][0][-1] & 7 == 0, (s, b)
                _compare_batch(b, {"axc": got["axc"][c:c + 1], "waveout": got["waveout"][c:c + 1], "iq_out": got["iq_out"][c:c + 1]}, tr[c:c + 1], want,
                               got["stats"][c], orcs[s][f].stats(0, 0))
                for g in range(lengths[s]):
                    assert hip.freq_stats(n_multi + s, g) == orcs[s][g].stats(0, 0), (b, s, g)
        for s in sample:
            opened += sum(1 for o in orcs[s] if o.stats(0, 0)["open_count"] > 0)
    assert opened >= 2 * len(sample)
    return sched, k_all


def test_several_lists_of_different_lengths(pkg, built):
    """Lists of 2, 3, 5, 1 and 4 entries beside two multichannel dongles: bank indices past the first list, several switches per batch."""
    sched, k_all = _fleet(pkg, 2, [2, 3, 5, 1, 4], 5, n_batches=10)
    assert (sched[[0, 1, 2, 4], k_all] != sched[[0, 1, 2, 4], k_all - 1]).all()


def test_fleet_of_scan_dongles_beside_multichannel_dongles(pkg, built):
    """4 096 scan dongles with 4 entries each and 4 096 multichannel dongles of 8 channels in one handle; one batch where every scan dongle switches;
    32 sampled scan dongles against the composition."""
    sched, k_all = _fleet(pkg, 4096, [4] * 4096, 32, n_batches=6)
    assert (sched[:, k_all] != sched[:, k_all - 1]).all()
