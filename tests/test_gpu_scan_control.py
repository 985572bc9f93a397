"""Scan control on the GPU (airband_hip_set_scan_control / _scan_hold / _collect_scan_events / _collect_scan_state, csrc/scan_control.hip).

Ground truth is a TWIN: a second handle with the same configuration and the same input and no controller, whose set_freq_index() is driven by
capi.scan_control_reference() applied to the twin's own axcindicate -- the host method this feature replaces, which tests/test_gpu_scan.py pins to the oracle.
The controlled handle must give the reference's records and states and the twin's results, bit for bit, batch after batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F0 = 120_100_000
IDLE, DWELL = 2, 1


def _entry(**kw):
    e = dict(frequency=F0, modulation=0)
    e.update(kw)
    return e


# entries that differ in notch, CTCSS, manual squelch and ampfactor: ChanConst.flags differs between the entries of a list
LIST4 = [_entry(), _entry(frequency=F0 + 25_000, ctcss_freq=88.5), _entry(frequency=F0 + 50_000, squelch_snr_threshold_db=8.0, notch_freq=800.0, ampfactor=1.8),
         _entry(frequency=F0 + 62_500, squelch_threshold_dbfs=-5)]  # (a manual squelch level of about 10)
LIST1 = [_entry(frequency=F0 + 12_500)]
LIST3 = [_entry(frequency=F0 + 37_500), _entry(frequency=F0 + 75_000, notch_freq=1000.0, ampfactor=0.7), _entry(frequency=F0 + 87_500, squelch_threshold_dbfs=-5, ampfactor=1.5)]
MULTI = [_entry(frequency=F0 + 12_500 * j) for j in range(8)]
# the lists in an order that is not the dongles': records and states come in DONGLE order all the same
SCAN = {2: LIST3, 0: LIST4, 1: LIST1}
DEVICES = [dict(channels=[LIST4[0]]), dict(channels=[LIST1[0]]), dict(channels=[LIST3[0]]), dict(channels=MULTI)]
EXT = {0: 0, 1: 1, 2: 2}  # scan dongle -> its channel
N_CH = 11


def _bins(rng, n_ch, B, key):
    """Stage-1 rows of n_ch channels for one batch: complex noise, and a carrier on rows [100, B) of the channels where key is set."""
    z = rng.standard_normal((n_ch, B, 2), dtype=np.float32) * np.float32(0.7)
    idx = np.nonzero(key)[0]
    if idx.size:
        ph = rng.uniform(0, 2 * np.pi, (idx.size, 1)) + 0.3 * np.arange(B - 100)
        z[idx, 100:, 0] += (25.0 * np.cos(ph)).astype(np.float32)
        z[idx, 100:, 1] += (25.0 * np.sin(ph)).astype(np.float32)
    re, im = z[..., 0], z[..., 1]
    return np.sqrt(re * re + im * im).astype(np.float32), np.ascontiguousarray(z.reshape(n_ch, 2 * B))


# which batches the scan channels (and two of the ordinary ones) hear a carrier in: quiet spells long enough to saturate and wrap, openings after them
KEYED = {0: {9, 10, 17}, 1: {5, 6}, 2: {6, 7, 14, 21}, 5: {3, 4, 5, 12}, 9: {8, 20}}
N_BATCHES = 24


def _keys(n_batches=N_BATCHES, n_ch=N_CH):
    key = np.zeros((n_batches, n_ch), bool)
    for c, bs in KEYED.items():
        for b in bs:
            if b < n_batches and c < n_ch:
                key[b, c] = True
    return key


class Twin:
    """The reference's state per list, and the twin handle it steers with set_freq_index()."""

    def __init__(self, capi, hip, scan, ext, idle=IDLE, dwell=DWELL, start=None):
        self.capi, self.hip, self.scan, self.ext, self.idle, self.dwell = capi, hip, scan, ext, idle, dwell
        self.state = {d: capi.scan_control_blank((start or {}).get(d, 0)) for d in scan}
        self.batch = 0
        self.enabled = {d: True for d in scan}

    def advance(self, axc):
        """One batch: every list's state from the twin's axcindicate; the new entries go to the twin for its next batch.  Returns the batch's records."""
        recs = []
        for d in sorted(self.scan):
            st, rec = self.capi.scan_control_reference(self.state[d], axc[self.ext[d]], len(self.scan[d]), self.batch, idle_batches=self.idle, dwell_batches=self.dwell,
                                                       dev=d, enabled=self.enabled[d])
            self.state[d] = st
            recs.append(rec)
            self.hip.set_freq_index(d, int(st["idx"]))
        self.batch += 1
        return np.concatenate(recs)

    def states(self, n_dev):
        out = np.zeros(n_dev, self.capi.SCAN_STATE_DTYPE)
        for d, st in self.state.items():
            out[d] = st
        return out


def _same_results(b, got, want, what=""):
    for k in ("waveout", "iq_out"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "batch %d: %s %s" % (b, k, what)
    assert np.array_equal(got["axc"], want["axc"]), "batch %d: axc %s: %r != %r" % (b, what, bytes(got["axc"]), bytes(want["axc"]))
    assert got["stats"] == want["stats"], "batch %d: stats %s" % (b, what)


def _check_batch(b, ctl, tw, n_dev, max_records=None):
    """The controlled handle's batch against the twin's and the reference's; returns the batch's records."""
    got, ref = ctl.collect(iq=True, stats=True), tw.hip.collect(iq=True, stats=True)
    _same_results(b, got, ref)
    for d in sorted(tw.scan):
        for f in range(len(tw.scan[d])):
            assert ctl.freq_stats(d, f) == tw.hip.freq_stats(d, f), "batch %d: freq_stats of dongle %d entry %d" % (b, d, f)
    recs = tw.advance(ref["axc"])
    ev = ctl.collect_scan_events()
    cap = len(tw.scan) if max_records is None else max_records
    assert ev["n_records"] == len(recs), "batch %d: %d records, the reference has %d" % (b, ev["n_records"], len(recs))
    assert ev["records"].tobytes() == recs[:cap].tobytes(), "batch %d: records %r != %r" % (b, ev["records"].tolist(), recs[:cap].tolist())
    st = ctl.collect_scan_state()
    assert st.tobytes() == tw.states(n_dev).tobytes(), "batch %d: states %r != %r" % (b, st.tolist(), tw.states(n_dev).tolist())
    return recs


def _run_bins(pkg, devices, scan, ext, wave_rate, n_batches, keys, *, seed=3, events=None, max_records=None, flags=0):
    """process_bins batches on a controlled handle and its twin; events: {batch: callable(ctl, twin)} run before that batch.  Returns all records per batch."""
    capi = pkg.capi
    n_ch = sum(len(d["channels"]) for d in devices)
    rng = np.random.default_rng(seed)
    out = []
    with pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as ctl, pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags, scan=scan) as plain:
        ctl.set_scan_control(IDLE, DWELL, max_records)
        tw = Twin(capi, plain, scan, ext)
        assert ctl.collect_scan_state().tobytes() == tw.states(len(devices)).tobytes()  # valid from the start
        for b in range(n_batches):
            if events and b in events:
                events[b](ctl, tw)
            wavein, iqin = _bins(rng, n_ch, ctl.B, keys[b])
            ctl.process_bins(wavein, iqin)
            plain.process_bins(wavein, iqin)
            out.append(_check_batch(b, ctl, tw, len(devices), max_records))
    return out


def _summary(per_batch, capi):
    allr = np.concatenate(per_batch)
    hops = allr[allr["kind"] == capi.SCAN_HOP]
    act = allr[allr["kind"] == capi.SCAN_ACTIVITY]
    wrapped = sorted(set(hops["dev"][(hops["freq_idx"] == 0) & (hops["prev_idx"] > 0)].tolist()))
    opened = sorted(set(zip(act["dev"].tolist(), act["freq_idx"].tolist())))
    return hops, act, wrapped, opened


def test_every_batch_equals_the_twin_and_the_reference(pkg, built):
    """Three lists of 4, 1 and 3 entries and an ordinary 8-channel dongle, 24 batches: records, count, states, waveout, iq_out, axc, stats and every entry's
    freq_stats."""
    capi = pkg.capi
    per_batch = _run_bins(pkg, DEVICES, SCAN, EXT, 8000, N_BATCHES, _keys())
    hops, act, wrapped, opened = _summary(per_batch, capi)
    print("%d HOP, %d ACTIVITY (%d RETAG); lists that wrapped: %r; entries that opened: %r" % (len(hops), len(act), int((act["flags"] == capi.SCAN_RETAG).sum()), wrapped, opened))
    assert len(opened) >= 2 and len(wrapped) >= 2, (opened, wrapped)
    assert (act["flags"] == capi.SCAN_RETAG).any() and 1 not in set(hops["dev"].tolist())  # the list of one entry never hops
    assert max(len(r) for r in per_batch) >= 2  # two lists in one batch: dongle order was put to the test
    for r in per_batch:
        assert np.all(np.diff(r["dev"]) > 0)


def test_a_list_mixing_am_and_nfm_at_16000(pkg, built):
    """wave rate 16 000, a list of AM and NFM entries (with lowpass, notch): scan_mag_kernel keeps rewriting |bin| under the GPU's hops."""
    capi = pkg.capi
    mixed = [_entry(squelch_snr_threshold_db=9.0), _entry(frequency=F0 + 12_500, modulation=1), _entry(frequency=F0 + 25_000, modulation=1, bandwidth_hz=8000),
             _entry(frequency=F0 + 50_000, notch_freq=1200.0)]
    plain3 = [_entry(frequency=F0 + 37_500), _entry(frequency=F0 + 75_000, ampfactor=0.7), _entry(frequency=F0 + 87_500, squelch_snr_threshold_db=6.0)]
    devices = [dict(channels=[mixed[0]]), dict(channels=[plain3[0]]), dict(channels=MULTI[:4])]
    keys = np.zeros((16, 6), bool)
    for c, bs in {0: {3, 8, 9, 14}, 1: {5, 11}, 3: {2, 7}}.items():
        for b in bs:
            keys[b, c] = True
    per_batch = _run_bins(pkg, devices, {0: mixed, 1: plain3}, {0: 0, 1: 1}, 16000, 16, keys, seed=5)
    hops, act, wrapped, opened = _summary(per_batch, capi)
    print("mixed list: %d HOP, %d ACTIVITY; wrapped %r; opened %r" % (len(hops), len(act), wrapped, opened))
    assert len(hops) >= 4 and len(act) >= 2 and len(opened) >= 2, (hops.tolist(), act.tolist())


def _iq_case(pkg, n_batches, wave_rate=8000, sample_rate=2_560_000, fft_log=9):
    """One u8 stream with two transmitters keyed a quarter of every second, half a second apart, on the bins of two channels; three dongles hear it: an ordinary
    one with both channels and six more, a scan dongle on the first transmitter's channel (4 entries) and one on the second's (3 entries)."""
    sg = pkg.siggen
    chans, _ = sg.baseline_plan(mixed=False)
    probe = [dict(channels=[dict(c) for c in chans], sample_rate=sample_rate)]
    n_fft = 1 << fft_log
    carriers = []
    for slot, k in enumerate((0, 2)):
        b = int(pkg.derive_constants(probe, k, wave_rate=wave_rate, fft_log=fft_log)[0])
        off = (b if b < n_fft // 2 else b - n_fft) * sample_rate / n_fft
        carriers.append(sg.make_carrier(off, sample_rate, kind=0, key_slot=slot, key_period_s=1.0, key_on_s=0.25, key_slot_s=0.5))
    hop = round(sample_rate / wave_rate)
    n_samples = (n_batches * (wave_rate // 8) + 100) * hop + n_fft + 8
    iq = sg.generate_u8(0, 0, n_samples, carriers)
    a, c = dict(chans[0]), dict(chans[2])
    la = [a, dict(a, squelch_snr_threshold_db=12.0, ampfactor=0.6), dict(a, notch_freq=1000.0), dict(a, ctcss_freq=100.0)]
    lc = [c, dict(c, ampfactor=1.7), dict(c, squelch_snr_threshold_db=6.0, notch_freq=800.0)]
    devices = [dict(channels=chans), dict(channels=[a]), dict(channels=[c])]
    return devices, {1: la, 2: lc}, {1: 8, 2: 9}, iq


def _feed(hip, iq, k, n_dev):
    g = hip.geometry
    off = 0 if k == 0 else g.first_batch_bytes + (k - 1) * g.batch_bytes
    take = (g.first_batch_bytes + g.lookahead_bytes) if k == 0 else g.batch_bytes
    lo = off if k == 0 else off + g.lookahead_bytes
    for d in range(n_dev):
        assert hip.submit(d, iq[lo:lo + take]) == take
    assert hip.process()


@pytest.mark.parametrize("pipelined", [False, True], ids=["default", "pipeline"])
def test_through_stage_one_in_both_schedules(pkg, built, pipelined):
    """process() on u8 I/Q at fft 512.  The twin runs the sequential schedule and learns batch k's axcindicate before it enqueues batch k + 1; the controlled handle
    -- pipelined or not -- must have the hop decided behind batch k in force for batch k + 1 to give the same bits."""
    capi = pkg.capi
    n_batches = 14
    devices, scan, ext, iq = _iq_case(pkg, n_batches)
    flags = capi.FLAG_NO_REGROUP | (capi.FLAG_PIPELINE if pipelined else 0)
    grabbed, per_batch = [], []
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags, scan=scan) as ctl, pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_NO_REGROUP, scan=scan) as plain:
        ctl.set_scan_control(IDLE, DWELL)
        tw = Twin(capi, plain, scan, ext)

        def grab():
            r = ctl.collect(iq=True, stats=True)
            r["fs"] = [[ctl.freq_stats(d, f) for f in range(len(scan[d]))] for d in sorted(scan)]
            r["ev"], r["st"] = ctl.collect_scan_events(), ctl.collect_scan_state()
            grabbed.append(r)

        for k in range(n_batches):
            _feed(ctl, iq, k, 3)
            if not pipelined or k > 0:
                grab()
        if pipelined:
            ctl.flush()
            grab()
        for k in range(n_batches):
            _feed(plain, iq, k, 3)
            ref = plain.collect(iq=True, stats=True)
            got = grabbed[k]
            _same_results(k, got, ref)
            assert got["fs"] == [[plain.freq_stats(d, f) for f in range(len(scan[d]))] for d in sorted(scan)], k
            recs = tw.advance(ref["axc"])
            per_batch.append(recs)
            assert got["ev"]["n_records"] == len(recs) and got["ev"]["records"].tobytes() == recs.tobytes(), (k, got["ev"]["records"].tolist(), recs.tolist())
            assert got["st"].tobytes() == tw.states(3).tobytes(), (k, got["st"].tolist())
    hops, act, wrapped, opened = _summary(per_batch, capi)
    print("stage 1, %s: %d HOP, %d ACTIVITY; wrapped %r; opened %r" % ("pipelined" if pipelined else "default", len(hops), len(act), wrapped, opened))
    assert len(hops) >= 4 and len(act) >= 1, (hops.tolist(), act.tolist())


def test_hold_and_release(pkg, built):
    """Dongle 0 pinned to entry 0 before batch 4 (it is on entry 2 by then: a HOP behind batch 4) and released before batch 9; dongle 2 pinned to the entry it is on
    (no record, and none for the carrier it hears while it is pinned)."""
    capi = pkg.capi

    def pin(d, f):
        def go(ctl, tw):
            ctl.scan_hold(d, f)
            tw.state[d]["hold"] = f
        return go

    def both(*fs):
        return lambda ctl, tw: [f(ctl, tw) for f in fs]

    events = {4: both(pin(0, 0), pin(2, 2)), 9: pin(0, -1), 11: pin(2, -1)}
    per_batch = _run_bins(pkg, DEVICES, SCAN, EXT, 8000, 16, _keys(16), events=events)
    r4 = per_batch[4]
    assert r4[r4["dev"] == 0].tolist() == [(0, 0, 2, capi.SCAN_HOP, 0, 0, 4)], r4.tolist()
    assert all(len(r[r["dev"] == 0]) == 0 for r in per_batch[5:9])  # pinned: no hop, no activity record
    assert not any((r["dev"] == 2).any() for r in per_batch[4:11])


def test_a_dongle_switched_off_and_on_again(pkg, built):
    """Dongle 0 hops on the GPU, is switched off before batch 7 (frozen: no record, its state stays) and on again before batch 12: it comes back with the flags word
    of the entry the GPU had put in force (its results equal the twin's, whose host copy of the flags followed its own hops)."""
    off = lambda ctl, tw: (ctl.device_enable(0, False), tw.hip.device_enable(0, False), tw.enabled.__setitem__(0, False))
    on = lambda ctl, tw: (ctl.device_enable(0, True), tw.hip.device_enable(0, True), tw.enabled.__setitem__(0, True))
    per_batch = _run_bins(pkg, DEVICES, SCAN, EXT, 8000, 20, _keys(20), events={7: off, 12: on})
    assert sum((r["dev"] == 0).sum() for r in per_batch[:7]) >= 3  # it had hopped
    assert all(not (r["dev"] == 0).any() for r in per_batch[7:12])
    assert sum((r["dev"] == 0).sum() for r in per_batch[12:]) >= 1


def test_fewer_records_than_there_are(pkg, built):
    """max_records = 1 and batches with two records: the count says 2, the one record kept is the first in dongle order."""
    per_batch = _run_bins(pkg, DEVICES, SCAN, EXT, 8000, 8, _keys(8), max_records=1)
    assert max(len(r) for r in per_batch) >= 2


def test_switched_off_the_host_continues_from_the_gpus_index(pkg, built):
    capi = pkg.capi
    rng = np.random.default_rng(11)
    keys = _keys(12)
    with pkg.AirbandHip(DEVICES, wave_rate=8000, scan=SCAN) as ctl, pkg.AirbandHip(DEVICES, wave_rate=8000, scan=SCAN) as plain:
        plain.set_freq_index(0, 3)
        ctl.set_freq_index(0, 3)  # control switched on later starts from what set_freq_index last set
        ctl.set_scan_control(IDLE, DWELL)
        tw = Twin(capi, plain, SCAN, EXT, start={0: 3})
        for b in range(4):
            wavein, iqin = _bins(rng, N_CH, ctl.B, keys[b])
            ctl.process_bins(wavein, iqin)
            plain.process_bins(wavein, iqin)
            _check_batch(b, ctl, tw, 4)
        assert int(tw.state[0]["idx"]) != 3 and int(tw.state[2]["idx"]) != 0  # the GPU has moved both lists
        ctl.set_scan_control(0)
        with pytest.raises(pkg.AirbandError) as e:
            ctl.collect_scan_events()
        assert e.value.code == capi.EINVAL
        # the host hops again: dongle 2 goes on by hand, dongle 0 is left where the GPU put it
        nxt = (int(tw.state[2]["idx"]) + 1) % 3
        for b in range(4, 9):  # (the hop decided behind batch 3 had not been exchanged in yet when control went off: the host's first batch brings it in)
            if b == 6:
                ctl.set_freq_index(2, nxt)
                plain.set_freq_index(2, nxt)
            wavein, iqin = _bins(rng, N_CH, ctl.B, keys[b])
            ctl.process_bins(wavein, iqin)
            plain.process_bins(wavein, iqin)
            _same_results(b, ctl.collect(iq=True, stats=True), plain.collect(iq=True, stats=True), "after control was switched off")
            for d in sorted(SCAN):
                for f in range(len(SCAN[d])):
                    assert ctl.freq_stats(d, f) == plain.freq_stats(d, f), (b, d, f)
        # and on again: the lists keep their entries
        ctl.set_scan_control(IDLE, DWELL)
        st = ctl.collect_scan_state()
        assert st["idx"].tolist() == [int(tw.state[0]["idx"]), 0, nxt, 0] and st["hold"].tolist() == [-1, -1, -1, 0] and st["has_list"].tolist() == [1, 1, 1, 0]


def test_refusals(pkg, built):
    capi = pkg.capi
    EINVAL = capi.EINVAL

    def refused(fn, *a):
        with pytest.raises(pkg.AirbandError) as e:
            fn(*a)
        assert e.value.code == EINVAL, (fn, a, e.value.code)

    with pkg.AirbandHip([dict(channels=MULTI)], wave_rate=8000) as hip:  # a handle without scan lists
        refused(hip.set_scan_control, 16, 2)
        refused(hip.scan_hold, 0, 0)
        refused(hip.collect_scan_state)
    with pkg.AirbandHip(DEVICES, wave_rate=8000, scan=SCAN) as hip:
        refused(hip.set_scan_control, -1, 2)
        refused(hip.set_scan_control, 16, -1)
        refused(hip.scan_hold, 0, 1)  # control is off
        refused(hip.collect_scan_events)
        refused(hip.collect_scan_state)
        refused(hip.device_scan_control)
        hip.set_scan_control(0)  # off while off: nothing happens
        hip.set_freq_index(0, 1)
        hip.set_scan_control(16, 2, -5)  # max_records <= 0: one per list
        refused(hip.set_freq_index, 0, 2)  # the GPU sets the index now ...
        assert hip.collect_scan_state()["idx"].tolist() == [1, 0, 0, 0]  # ... and nothing changed
        refused(hip.scan_hold, 3, 0)  # no list
        refused(hip.scan_hold, 7, 0)
        refused(hip.scan_hold, 0, 4)
        refused(hip.scan_hold, 0, -2)
        refused(hip.collect_scan_state, 2, 3)
        with pytest.raises(pkg.AirbandError) as e:
            hip.collect_scan_events()
        assert e.value.code == capi.EAGAIN  # no batch yet
        ptrs = hip.device_scan_control()
        assert ptrs["n_records"] and ptrs["records"] and ptrs["state"]
        hip.scan_hold(0, 3)
        hip.scan_hold(1, 0)
        assert hip.collect_scan_state()["hold"].tolist() == [3, 0, -1, 0]


def test_a_list_too_long_for_the_int16_fields_is_refused(pkg, built):
    """idx, hold and last are int16: switching control on for a list of 32 768 entries is EINVAL, the host goes on hopping it."""
    big = [_entry()] + [_entry(frequency=F0 + 25 * k, ampfactor=1.0 + (k % 7) / 8) for k in range(1, 32768)]
    with pkg.AirbandHip([dict(channels=[big[0]])], wave_rate=8000, scan={0: big}) as hip:
        with pytest.raises(pkg.AirbandError) as e:
            hip.set_scan_control(16, 2)
        assert e.value.code == pkg.capi.EINVAL and "32 767" in str(e.value)
        hip.set_scan_control(0)  # switching off is no error
        hip.set_freq_index(0, 32767)
        with pytest.raises(pkg.AirbandError):
            hip.scan_hold(0, 1)  # control is off


def test_switched_on_while_a_pipelined_batch_is_pending(pkg, built):
    """AIRBAND_HIP_FLAG_PIPELINE: stage 1 of batch 0 is enqueued with entry 1 of dongle 1, then set_freq_index() names entry 3 and control is switched on.  The
    pending batch keeps the entry it was enqueued with and the list starts from it; the index no batch had latched is dropped."""
    capi = pkg.capi
    devices, scan, ext, iq = _iq_case(pkg, 3)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_PIPELINE | capi.FLAG_NO_REGROUP, scan=scan) as ctl, \
            pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_NO_REGROUP, scan=scan) as plain:
        ctl.set_freq_index(1, 1)
        plain.set_freq_index(1, 1)
        _feed(ctl, iq, 0, 3)  # stage 1 of batch 0; its stage 2 waits for the next call
        ctl.set_freq_index(1, 3)
        ctl.set_scan_control(IDLE, DWELL)
        assert ctl.collect_scan_state()["idx"].tolist() == [0, 1, 0]
        tw = Twin(capi, plain, scan, ext, start={1: 1})
        for k in range(3):
            if k < 2:
                _feed(ctl, iq, k + 1, 3)
            else:
                ctl.flush()
            _feed(plain, iq, k, 3)
            ref = plain.collect(iq=True, stats=True)
            _same_results(k, ctl.collect(iq=True, stats=True), ref)
            recs = tw.advance(ref["axc"])
            assert ctl.collect_scan_events()["records"].tobytes() == recs.tobytes(), k
            assert ctl.collect_scan_state().tobytes() == tw.states(3).tobytes(), k
