"""AIRBAND_HIP_FLAG_WIDE_HOPS for CF32 dongles on the GPU (csrc/channelizer_f32_wide.hip): devices above ~3 MS/s on the float32 matrix-core channelizer -- parity
with the oracle at every shape of tests/test_wide_hops_f32.py's table (20 MS/s included, which prepare() refuses without the flag), against the wavefront FFT on the
same stream, the flag inert inside the ordinary limits, zero-copy spans sized to the byte at hops of an odd number of samples, pipelined and run-ahead handles,
AFC, and the golden tests/golden/cf32_8000k.npz."""
import json

import numpy as np
import pytest

import helpers
import pyoracle
import test_gpu_wide_hops as gw
import test_wide_hops_f32 as tf

pytestmark = pytest.mark.gpu

_feed_all = gw._feed_all


@pytest.mark.parametrize("fft_log,sample_rate,wave_rate,n_batches", tf.GPU_CASES)
def test_wide_hop_parity(pkg, built, fft_log, sample_rate, wave_rate, n_batches):
    """Two dongles x 8 channels: squelch trace, axcindicate and counters exact, audio <= 1e-4 RMS, stage-1 bins within 1e-5 relative RMS of the oracle's (the bars
    of tests/test_gpu_parity.py), on the float matrix-core channelizer by the flag."""
    capi = pkg.capi
    n_dev = 2
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, fft_log, sample_rate, wave_rate, n_dev, n_batches)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    ref = [orc.run_device(d, iq[d], n_batches) for d in range(n_dev)]
    assert all(r["n_batches"] == n_batches for r in ref)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == "dft_mfma_f32"
        assert hip.channelizer_reason() == ""
        got = _feed_all(hip, iq, n_batches, bins=True)
    opened = 0
    worst_audio = worst_bins = 0.0
    for b, g in enumerate(got):
        want_t = np.concatenate([r["trace"][b] for r in ref])
        ww = np.concatenate([r["waveout"][b] for r in ref])
        e_w = helpers.rel_rms(g["w"], np.concatenate([r["raw_wavein"][b] for r in ref]))
        e_q = helpers.rel_rms(g["q"], np.concatenate([r["raw_iq"][b] for r in ref]))
        e_a = helpers.rms(g["waveout"] - ww)
        worst_audio, worst_bins = max(worst_audio, e_a), max(worst_bins, e_w, e_q)
        print("batch %d: |bin| %.3g, bin I/Q %.3g, audio RMS %.3g, trace mismatches %d" % (b, e_w, e_q, e_a, int((g["trace"] != want_t).sum())))
        assert e_w <= 1e-5 and e_q <= 1e-5, "batch %d bins" % b
        assert np.array_equal(g["axc"], np.concatenate([r["axc"][b] for r in ref])), "batch %d axc" % b
        assert np.array_equal(g["trace"], want_t), "batch %d: %d squelch-state mismatches" % (b, int((g["trace"] != want_t).sum()))
        assert e_a <= 1e-4
        opened += int((g["axc"] == ord("*")).sum())
    k = 0
    for d in range(n_dev):
        for j in range(len(devices[d]["channels"])):
            have, want = got[-1]["stats"][k], orc.stats(d, j)
            for key in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "bin"):
                assert have[key] == want[key], (d, j, key)
            k += 1
    assert opened > 0
    print("worst: bins %.3g, audio %.3g" % (worst_bins, worst_audio))


def test_same_stream_with_and_without_the_flag(pkg, built):
    """CF32 at 8 MS/s: the flagged handle (matrix cores) and the unflagged one (wavefront FFT, which says that the flag is what is missing) decide identically, audio
    within 1e-4 RMS of each other.  At 20 MS/s the unflagged prepare() is refused with a message that names the flag."""
    capi = pkg.capi
    n_dev, n_batches = 2, 5
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, 9, 8_000_000, 8000, n_dev, n_batches)
    runs = {}
    for flag in (0, capi.FLAG_WIDE_HOPS):
        with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == ("dft_mfma_f32" if flag else "fft_wave64")
            assert hip.channelizer_reason() == ("" if flag else "hop 8000 bytes: beyond the float channelizer's tile; AIRBAND_HIP_FLAG_WIDE_HOPS not set")
            runs[flag] = _feed_all(hip, iq, n_batches)
    for b, (x, y) in enumerate(zip(runs[0], runs[capi.FLAG_WIDE_HOPS])):
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]), b
        assert helpers.rms(x["waveout"] - y["waveout"]) <= 1e-4
        for sx, sy in zip(x["stats"], y["stats"]):
            for key in ("open_count", "flappy_count", "active_counter", "bin"):
                assert sx[key] == sy[key]
    devices, _ = helpers.format_case(pkg, capi.SFMT_F32, 9, 20_000_000, 8000, 1, 1)
    with pytest.raises(pkg.AirbandError) as e:
        pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH)
    assert e.value.code == capi.EBADSIZE and "AIRBAND_HIP_FLAG_WIDE_HOPS" in str(e.value)


@pytest.mark.parametrize("sample_rate", [2_560_000, 2_000_000])
def test_flag_is_inert_inside_the_ordinary_limits(pkg, built, sample_rate):
    """CF32 at 2.56 MS/s and 2.0 MS/s (hops of an odd number of samples), WAVE_RATE 16000: the ordinary float kernel with and without the flag, every output bit."""
    capi = pkg.capi
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, 9, sample_rate, 16000, n_dev, n_batches)
    for d in devices:
        d["channels"][3]["has_iq_outputs"] = 1
    with pytest.raises(pkg.AirbandError):
        pkg.wide_hop_plan_f32(512, sample_rate // 16000)
    runs = []
    for flag in (0, capi.FLAG_WIDE_HOPS):
        with pkg.AirbandHip(devices, wave_rate=16000, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == "dft_mfma_f32" and hip.channelizer_reason() == ""
            runs.append(_feed_all(hip, iq, n_batches, bins=True, iq_out=True))
    for b, (x, y) in enumerate(zip(*runs)):
        for key in ("waveout", "iq_out", "w", "q"):
            assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (b, key)
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"])
        assert x["stats"] == y["stats"]


def test_zero_copy_spans_sized_to_the_byte(pkg, built):
    """process_device on CF32 fft 256 at 10 MS/s, WAVE_RATE 16000 (hops of 625 samples = 5 000 bytes: 8-byte alignment): dongle 0 at the allocation's first byte,
    dongle 1 at an address that is 8 and not 16 bytes aligned, its span ending where the allocation ends -- batch_bytes + lookahead_bytes and not a byte more, so a
    read past the span is a read past the allocation (tests/test_gpu_wide_hops.py's construction).  Results equal the host path's bit for bit."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    n_dev, n_batches = 2, 3
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, 8, 10_000_000, 16000, n_dev, n_batches)
    flags = capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS
    with pkg.AirbandHip(devices, wave_rate=16000, fft_log=8, flags=flags) as hip:
        assert hip.channelizer_name() == "dft_mfma_f32"
        want = _feed_all(hip, iq, n_batches, bins=True)
    with pkg.AirbandHip(devices, wave_rate=16000, fft_log=8, flags=flags) as hip:
        g = hip.geometry
        pos = 0
        for b in range(n_batches):
            nb = g.first_batch_bytes if b == 0 else g.batch_bytes
            span = nb + g.lookahead_bytes
            stride = (span + 7) // 8 * 8 + 8
            if stride % 16 == 0:
                stride += 8
            buf = torch.empty((stride + span,), dtype=torch.uint8, device="cuda")   # dongle 0 at the allocation's first byte, dongle 1's span ends at its last
            assert buf.data_ptr() % 16 == 0 and stride % 16 == 8
            for d in range(n_dev):
                raw = iq[d].view(np.uint8)[pos:pos + span]
                assert len(raw) == span
                buf[d * stride:d * stride + span] = torch.from_numpy(raw.copy()).cuda()
            torch.cuda.synchronize()
            hip.process_device(buf.data_ptr(), stride)
            out = hip.collect(stats=True)
            w, q = hip.read_bins()
            tr = hip.read_trace()
            assert np.array_equal(out["waveout"].view(np.uint32), want[b]["waveout"].view(np.uint32)), b
            assert np.array_equal(out["axc"], want[b]["axc"]) and np.array_equal(tr, want[b]["trace"])
            assert np.array_equal(w.view(np.uint32), want[b]["w"].view(np.uint32)) and np.array_equal(q.view(np.uint32), want[b]["q"].view(np.uint32))
            assert out["stats"] == want[b]["stats"]
            pos += nb
            del buf


def test_pipelined_handle_is_the_sequential_one(pkg, built):
    """FLAG_PIPELINE | FLAG_WIDE_HOPS at CF32 8 MS/s: results one process() late, bit-identical."""
    capi = pkg.capi
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, 9, 8_000_000, 8000, n_dev, n_batches)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
        want = _feed_all(hip, iq, n_batches)
    got = []
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS | capi.FLAG_PIPELINE) as hip:
        assert hip.channelizer_name() == "dft_mfma_f32"
        pos = [0] * n_dev

        def take():
            out = hip.collect(stats=True)
            got.append(dict(axc=out["axc"].copy(), waveout=out["waveout"].copy(), stats=out["stats"], trace=hip.read_trace().copy()))

        for b in range(n_batches):
            for d in range(n_dev):
                pos[d] += hip.submit(d, iq[d].view(np.uint8)[pos[d]:])
            assert hip.process()
            if b >= 1:
                take()
        hip.flush()
        take()
    assert len(got) == n_batches
    for b, (x, y) in enumerate(zip(want, got)):
        assert np.array_equal(x["waveout"].view(np.uint32), y["waveout"].view(np.uint32)), b
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]) and x["stats"] == y["stats"], b


def test_process_device_runs_ahead(pkg, built):
    """A wide CF32 handle qualifies for run-ahead like any other: NULL-stream process_device batches take that path and equal the host path's bit for bit."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    n_dev, n_batches = 2, 3
    devices, iq = helpers.format_case(pkg, capi.SFMT_F32, 9, 8_000_000, 8000, n_dev, n_batches)
    flags = capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        want = _feed_all(hip, iq, n_batches)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        info = hip.schedule_info()
        assert info["run_ahead"] == 1 and info["ring_batches"] == 2
        g = hip.geometry
        pos = 0
        for b in range(n_batches):
            nb = g.first_batch_bytes if b == 0 else g.batch_bytes
            span = nb + g.lookahead_bytes
            stride = (span + 255) // 256 * 256
            buf = torch.zeros((n_dev * stride,), dtype=torch.uint8, device="cuda")
            for d in range(n_dev):
                buf[d * stride:d * stride + span] = torch.from_numpy(iq[d].view(np.uint8)[pos:pos + span].copy()).cuda()
            torch.cuda.synchronize()
            hip.process_device(buf.data_ptr(), stride)
            out = hip.collect(stats=True)
            assert np.array_equal(out["waveout"].view(np.uint32), want[b]["waveout"].view(np.uint32)), b
            assert np.array_equal(out["axc"], want[b]["axc"]) and np.array_equal(hip.read_trace(), want[b]["trace"]) and out["stats"] == want[b]["stats"]
            pos += nb
        assert hip.schedule_info()["batches_run_ahead"] == n_batches


def test_afc_on_wide_hops(pkg, built):
    """CF32 at 8 MS/s with channels that AFC moves, flag set: the batches run on the float matrix-core channelizer (private tables re-tuned on the device, the last
    hop's spectrum from a one-window launch of the wavefront FFT), oracle parity as tests/test_gpu_afc.py defines it."""
    import test_gpu_afc as ta

    capi = pkg.capi
    case = helpers.afc_format_case(pkg, capi.SFMT_F32, 9, 8_000_000, 8000, [helpers.afc_plan(8)] * 2, ta.N_BATCHES)
    _, moved = ta.run_against_oracle(pkg, case, 9, 8000, flags=capi.FLAG_WIDE_HOPS, name="dft_mfma_f32", what="SFMT_F32, fft 512, 8 MS/s, WAVE_RATE 8000, wide hops")
    assert moved > 0 and case["ups"] > 0 and case["downs"] > 0


def test_hip_matches_wide_golden(pkg, built):
    """tests/golden/cf32_8000k.npz (the reference's outputs) against the flagged handle: decisions exact, audio <= 1e-4 RMS."""
    z, c, devices, iq = tf.load_golden()
    with pkg.AirbandHip(devices, wave_rate=c["wave_rate"], fft_log=c["fft_log"], flags=pkg.capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == "dft_mfma_f32" and hip.channelizer_reason() == ""
        raw, pos = iq.view(np.uint8), 0
        for b in range(c["n_batches"]):
            pos += hip.submit(0, raw[pos:])
            assert hip.process()
            out = hip.collect(stats=True)
            assert np.array_equal(out["axc"], z["axc"][b]), "batch %d" % b
            assert helpers.rms(out["waveout"] - z["waveout"][b]) <= 1e-4
        for j, want in enumerate(json.loads(str(z["stats"]))):
            for k in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "bin"):
                assert out["stats"][j][k] == want[k], (j, k)
