"""The default schedule of NULL-stream airband_hip_process_device() batches (run-ahead: stage 1 of batch k on a stream of its own, stage 2 of batch k on the handle's
stream behind it, both enqueued by the same call) against the single-stream schedule a handle prepared under AIRBAND_HIP_RUN_AHEAD=0 has.  Same library, same
resident I/Q: every comparison is BIT-IDENTICAL -- waveout, axcindicate, every channel_stats field, iq_out and the mixer outputs -- and no tolerance is involved.

The I/Q is generated on the GPU (airband_hip_generate_iq) into a ring of three resident batches behind the first one, as bench.py does, starting four batches into the
keying period so that squelches are open."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

WAVE_RATE, RING, START_BATCH, N_MIXERS = 16000, 3, 4, 4
SEQ_INFO = dict(run_ahead=False, ring_batches=1, channelizer_waves_per_cu=0)
AHEAD_INFO = dict(run_ahead=True, ring_batches=2, channelizer_waves_per_cu=5)


def _tweak(d, ch):
    ch[3]["has_iq_outputs"] = 1  # iq_out is not all zeros


def _afc(d, ch):
    _tweak(d, ch)
    ch[0]["afc"] = 2


def _mix(n_dev):
    return [(d, c, (d * 8 + c) % N_MIXERS, 1.0 + 0.1 * c, 0.25 if c == 5 else 0.0) for d in range(n_dev) for c in range(8)]


def _handle(pkg, monkeypatch, devices, run_ahead, flags=0, mixers=True, wave_rate=WAVE_RATE):
    """A handle prepared with the run-ahead schedule switched on (the default: variable unset) or off (AIRBAND_HIP_RUN_AHEAD=0); the variable is read at prepare."""
    with monkeypatch.context() as m:
        if run_ahead:
            m.delenv("AIRBAND_HIP_RUN_AHEAD", raising=False)
        else:
            m.setenv("AIRBAND_HIP_RUN_AHEAD", "0")
        h = pkg.AirbandHip(devices, wave_rate=wave_rate, flags=flags)
    if mixers:
        h.set_mixers(N_MIXERS, _mix(len(devices)))
    return h


def _info(h):
    i = h.schedule_info()
    return {k: i[k] for k in SEQ_INFO}


class Resident:
    """n_dev dongles' I/Q in HBM: the first batch (with its lead-in), RING more, the look-ahead."""

    def __init__(self, pkg, torch, h, carriers):
        g = h.geometry
        self.first, self.batch = g.first_batch_bytes, g.batch_bytes
        self.span = self.first + RING * self.batch + g.lookahead_bytes
        self.stride = (self.span + 255) // 256 * 256
        self.buf = torch.zeros((g.device_count, self.stride), dtype=torch.uint8, device="cuda")
        self.fill(h, carriers)
        h.synchronize()

    def fill(self, h, carriers):
        """(enqueued on h's own stream; the caller decides whether to wait)"""
        h.set_signal_plan(carriers)
        h.generate_iq(self.buf.data_ptr(), self.stride, START_BATCH * self.batch, self.span)

    def ptr(self, k):
        return self.buf.data_ptr() + (0 if k == 0 else self.first + ((k - 1) % RING) * self.batch)


def _grab(h, mixers=True):
    r = h.collect(iq=True, stats=True)
    r["mix"] = h.collect_mixers() if mixers else ()
    return r


def _same(got, want, what):
    assert np.array_equal(got["axc"], want["axc"]), what + ": axcindicate"
    assert np.array_equal(got["waveout"].view(np.uint32), want["waveout"].view(np.uint32)), what + ": waveout"
    assert np.array_equal(got["iq_out"].view(np.uint32), want["iq_out"].view(np.uint32)), what + ": iq_out"
    assert len(got["mix"]) == len(want["mix"])
    for a, b in zip(got["mix"], want["mix"]):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), what + ": mixer outputs"
    assert len(got["stats"]) == len(want["stats"])
    for c, (x, y) in enumerate(zip(got["stats"], want["stats"])):
        assert x == y, "%s: channel_stats of channel %d: %r != %r" % (what, c, x, y)


N_DEV, N_BATCHES = 64, 7  # the `tiny` plan; seven batches: the lead-in batch, and the two-deep ring wraps three times


@pytest.fixture(scope="module")
def tiny(pkg, built):
    """The resident I/Q of the 64-dongle plan and what the single-stream schedule makes of it, batch by batch -- computed once, read by every test below."""
    torch = pytest.importorskip("torch")
    mp = pytest.MonkeyPatch()
    devices, carriers = helpers.plan_devices(N_DEV, True, _tweak)
    ref = _handle(pkg, mp, devices, run_ahead=False)
    try:
        assert _info(ref) == SEQ_INFO
        res = Resident(pkg, torch, ref, carriers)
        want, bins = [], None
        for k in range(N_BATCHES):
            ref.process_device(res.ptr(k), res.stride)
            want.append(_grab(ref))
            if k == 2:
                bins = ref.read_bins()
        assert ref.schedule_info()["batches_run_ahead"] == 0
    finally:
        ref.close()
        mp.undo()
    assert sum(int((w["axc"] != ord(" ")).sum()) for w in want) > 0 and any(np.abs(w["iq_out"]).max() > 0 for w in want)
    assert any(np.abs(w["mix"][0]).max() > 0 for w in want) and any(np.abs(w["mix"][1]).max() > 0 for w in want)
    return dict(devices=devices, carriers=carriers, res=res, want=want, bins=bins, torch=torch)


def test_back_to_back_batches(pkg, tiny, monkeypatch):
    """Seven batches enqueued with no synchronisation in between (stage 1 of batch k+1 beside stage 2 of batch k), compared after the last; then again on a fresh
    handle with every batch collected, compared after each."""
    res, want = tiny["res"], tiny["want"]
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        assert _info(h) == AHEAD_INFO
        for k in range(N_BATCHES):
            h.process_device(res.ptr(k), res.stride)
        _same(_grab(h), want[-1], "unsynchronised, after batch %d" % (N_BATCHES - 1))
        assert h.schedule_info()["batches_run_ahead"] == N_BATCHES
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        for k in range(N_BATCHES):
            h.process_device(res.ptr(k), res.stride)
            h.synchronize()
            _same(_grab(h), want[k], "synchronised, batch %d" % k)


def test_batches_long_enough_to_overlap(pkg, built, monkeypatch):
    """4 096 dongles, about a millisecond per step: stage 2 of batch k is still running when stage 1 of batch k+1 is enqueued, so a missing wait for the ring rows
    stage 1 overwrites (those stage 2 of batch k-1 read) would show.  Eight batches back to back, the last one compared."""
    torch = pytest.importorskip("torch")
    n_dev, n_batches = 4096, 8
    devices, carriers = helpers.plan_devices(n_dev, True, _tweak)
    got = []
    res = None
    for run_ahead in (False, True):
        with _handle(pkg, monkeypatch, devices, run_ahead=run_ahead) as h:
            assert _info(h) == (AHEAD_INFO if run_ahead else SEQ_INFO)
            if res is None:
                res = Resident(pkg, torch, h, carriers)
            for k in range(n_batches):
                h.process_device(res.ptr(k), res.stride)
            got.append(_grab(h))
    del res  # 10 GB: hand them back before the next test
    torch.cuda.empty_cache()
    assert int((got[0]["axc"] != ord(" ")).sum()) > 0
    _same(got[1], got[0], "4 096 dongles, after batch %d" % (n_batches - 1))


def test_input_generated_on_the_handle_is_waited_for(pkg, tiny, monkeypatch):
    """airband_hip_generate_iq on the handle's stream, then process_device with no synchronisation in between: stage 1, on its own stream, reads what the generator
    wrote.  The buffer holds zeros until the generator has run."""
    torch = tiny["torch"]
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        res = Resident.__new__(Resident)
        src = tiny["res"]
        res.first, res.batch, res.span, res.stride = src.first, src.batch, src.span, src.stride
        res.buf = torch.zeros_like(src.buf)
        torch.cuda.synchronize()
        res.fill(h, tiny["carriers"])
        for k in range(3):
            h.process_device(res.ptr(k), res.stride)
        _same(_grab(h), tiny["want"][2], "generate_iq then three batches")
        assert torch.equal(res.buf, src.buf)
        # and again in the middle of a run: batch 3's bytes are wiped and regenerated right in front of the call that reads them
        res.buf.zero_()
        torch.cuda.synchronize()
        res.fill(h, tiny["carriers"])
        h.process_device(res.ptr(3), res.stride)
        _same(_grab(h), tiny["want"][3], "generate_iq in front of batch 3")
        assert h.schedule_info()["batches_run_ahead"] == 4


def test_mixers_cleared_and_rewired_between_batches(pkg, tiny, monkeypatch):
    """clear_mixers() in front of every batch and set_mixers() (the same wiring, new buffers) in the middle of the run, nothing else in between."""
    res, want = tiny["res"], tiny["want"]
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        for k in range(N_BATCHES):
            if k == 3:
                h.set_mixers(N_MIXERS, _mix(N_DEV))
            if k > 0:
                h.clear_mixers()
            h.process_device(res.ptr(k), res.stride)
            if k in (2, 3):
                _same(_grab(h), want[k], "batch %d" % k)
        _same(_grab(h), want[-1], "after batch %d" % (N_BATCHES - 1))
        h.clear_mixers()
        left, right, sig = h.collect_mixers()
        assert not left.any() and not right.any() and not sig.any()


def test_a_callers_stream_takes_the_sequential_path(pkg, tiny, monkeypatch):
    """Batches on a caller's stream between batches on the handle's own: the former run whole on that stream (and are not counted as run ahead)."""
    torch = tiny["torch"]
    res, want = tiny["res"], tiny["want"]
    side = torch.cuda.Stream()
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        ahead = 0
        for k in range(N_BATCHES):
            if k in (2, 3, 5):
                h.process_device(res.ptr(k), res.stride, side.cuda_stream)
            else:
                h.process_device(res.ptr(k), res.stride)
                ahead += 1
            _same(_grab(h), want[k], "batch %d" % k)
            assert h.schedule_info()["batches_run_ahead"] == ahead
        assert _info(h) == AHEAD_INFO


def test_afc_handles_stay_sequential(pkg, tiny, monkeypatch):
    res = tiny["res"]
    devices, _ = helpers.plan_devices(N_DEV, True, _afc)
    got = []
    for run_ahead in (False, True):
        with _handle(pkg, monkeypatch, devices, run_ahead=run_ahead) as h:
            assert _info(h) == SEQ_INFO
            for k in range(4):
                h.process_device(res.ptr(k), res.stride)
            got.append(_grab(h))
            assert h.schedule_info()["batches_run_ahead"] == 0
    _same(got[1], got[0], "afc on channel 0")


def test_pipelined_handles_keep_their_lag(pkg, tiny, monkeypatch):
    res, want = tiny["res"], tiny["want"]
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True, flags=pkg.capi.FLAG_PIPELINE) as h:
        assert _info(h) == dict(run_ahead=False, ring_batches=2, channelizer_waves_per_cu=5)
        for k in range(4):
            h.process_device(res.ptr(k), res.stride)
            if k == 0:
                with pytest.raises(pkg.AirbandError) as e:
                    h.collect()
                assert e.value.code == pkg.capi.EAGAIN
            else:
                _same(_grab(h), want[k - 1], "pipelined, call %d" % k)
        h.flush()
        _same(_grab(h), want[3], "pipelined, flush")
        assert h.schedule_info()["batches_run_ahead"] == 0


def test_process_bins_between_run_ahead_batches(pkg, tiny, monkeypatch):
    """Stage 2 alone on the single-stream handle's own stage-1 output of batch 2, after two batches that ran ahead and in front of one more."""
    res, want = tiny["res"], tiny["want"]
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        for k in range(2):
            h.process_device(res.ptr(k), res.stride)
        h.process_bins(*tiny["bins"])
        _same(_grab(h), want[2], "process_bins as batch 2")
        assert h.schedule_info()["batches_run_ahead"] == 2
        h.process_device(res.ptr(3), res.stride)
        h.process_device(res.ptr(4), res.stride)
        _same(_grab(h), want[4], "batch 4, two batches behind process_bins")


def test_release_with_batches_in_flight(pkg, tiny, monkeypatch):
    res, want = tiny["res"], tiny["want"]
    h = _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True)
    for k in range(3):
        h.process_device(res.ptr(k), res.stride)
    h.close()
    tiny["torch"].cuda.synchronize()
    with _handle(pkg, monkeypatch, tiny["devices"], run_ahead=True) as h:
        for k in range(3):
            h.process_device(res.ptr(k), res.stride)
        _same(_grab(h), want[2], "a fresh handle after the release")
