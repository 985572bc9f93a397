"""AIRBAND_HIP_FLAG_WIDE_HOPS at CS16 fft 2048, u8 / s8 fft 4096 and CS16 fft 4096 on the GPU: the k-segmented row staging of csrc/channelizer_dft_wide.hip --
parity with the oracle at every shape, flagged against unflagged on one stream, zero-copy spans sized to the byte, one-segment shapes untouched, pipelined
handles, AFC, and the golden tests/golden/cs16_10000k_fft2048.npz.  (u8 / s8 fft 4096 at hops of an odd number of samples is not on the kernel -- its variant
spills registers, tests/test_wide_windows.py -- and the handle says so: test_odd_hops_at_fft_4096_stay_on_the_wavefront_fft.)"""
import json

import numpy as np
import pytest

import helpers
import pyoracle
import test_gpu_wide_hops as gw
import test_wide_windows as ww

pytestmark = pytest.mark.gpu


def _hop_bytes(capi, sfmt_name, sample_rate, wave_rate):
    return 2 * round(sample_rate / wave_rate) * capi.BYTES_PER_SAMPLE[getattr(capi, sfmt_name)]


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", ww.GPU_CASES)
def test_wide_window_parity(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """Two dongles, seven batches (the first with its lead-in) through the host path with FLAG_TRACE_SQUELCH | FLAG_WIDE_HOPS: on the matrix cores by the plan, squelch
    trace, axcindicate and counters exact, audio <= 1e-4 RMS, stage-1 bins within 1e-5 relative RMS of the oracle's."""
    seg, lds = pkg.wide_hop_plan(1 << fft_log, _hop_bytes(pkg.capi, sfmt_name, sample_rate, wave_rate), getattr(pkg.capi, sfmt_name))
    assert seg in (2, 4) and lds <= 160 * 1024
    gw.test_wide_hop_parity(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate)


def test_odd_hops_at_fft_4096_stay_on_the_wavefront_fft(pkg, built):
    """s8 10 MS/s, WAVE_RATE 16000, fft 4096 (hops of 1 250 bytes): the segmented AL = 2 variant spills registers and is not built; the flagged handle says why and
    computes what the unflagged one computes, bit for bit."""
    capi = pkg.capi
    sfmt_name, fft_log, sample_rate, wave_rate = ww.ODD_HOP_CASE
    devices, iq = helpers.format_case(pkg, getattr(capi, sfmt_name), fft_log, sample_rate, wave_rate, 2, 2)
    runs = []
    for flag in (capi.FLAG_WIDE_HOPS, 0):
        with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == "fft_wave64"
            if flag:
                assert hip.channelizer_reason() == "wide hops: fft 4096 at hops of an odd number of samples: the segmented kernel spills registers and is not built"
            runs.append(gw._feed_all(hip, iq, 2, bins=True))
    for x, y in zip(*runs):
        for key in ("waveout", "w", "q"):
            assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), key
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"])


def test_same_stream_with_and_without_the_flag(pkg, built):
    """CS16 fft 2048 at 10 MS/s: the flagged handle (matrix cores) and the unflagged one (wavefront FFT) decide identically, audio within 1e-4 RMS of each other."""
    capi = pkg.capi
    n_dev, n_batches = 2, 5
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 11, 10_000_000, 8000, n_dev, n_batches)
    runs = {}
    for flag in (0, capi.FLAG_WIDE_HOPS):
        with pkg.AirbandHip(devices, wave_rate=8000, fft_log=11, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == ("dft_mfma_i8" if flag else "fft_wave64")
            assert hip.channelizer_reason() == ("" if flag else "hop 5000 bytes > 1280: AIRBAND_HIP_FLAG_WIDE_HOPS not set")
            runs[flag] = gw._feed_all(hip, iq, n_batches)
    opened = 0
    for b, (x, y) in enumerate(zip(runs[0], runs[capi.FLAG_WIDE_HOPS])):
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]), b
        assert helpers.rms(x["waveout"] - y["waveout"]) <= 1e-4
        opened += int((x["axc"] == ord("*")).sum())
        for sx, sy in zip(x["stats"], y["stats"]):
            for key in ("open_count", "flappy_count", "active_counter", "bin"):
                assert sx[key] == sy[key]
    assert opened > 0


def test_zero_copy_spans_sized_to_the_byte(pkg, built):
    """tests/test_gpu_wide_hops.py's construction at CS16 fft 2048, 10 MS/s: dongle 1's span starts 8 bytes off a 16-byte boundary and ends where the allocation
    ends -- batch_bytes + lookahead_bytes and not a byte more, so a transfer past the span is a read past the allocation.  Bit-identical to the host path."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    n_dev, n_batches = 2, 3
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 11, 10_000_000, 8000, n_dev, n_batches)
    flags = capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=11, flags=flags) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8"
        want = gw._feed_all(hip, iq, n_batches, bins=True)
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=11, flags=flags) as hip:
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


def test_one_segment_shapes_are_untouched(pkg, built):
    """CS16 fft 1024 at 10 MS/s, a shape the wide kernel took before: the plan says one segment with the LDS of wide_hop_lds_bytes(), and a second handle's bins and
    audio equal the first's bit for bit (within this build; across commits the benchmark's dumped outputs are compared)."""
    capi = pkg.capi
    assert pkg.wide_hop_plan(1024, 5000, capi.SFMT_S16) == (1, pkg.wide_hop_lds_bytes(1024, 5000, capi.SFMT_S16))
    n_dev, n_batches = 2, 3
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 10, 10_000_000, 8000, n_dev, n_batches)
    runs = []
    for _ in range(2):
        with pkg.AirbandHip(devices, wave_rate=8000, fft_log=10, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
            assert hip.channelizer_name() == "dft_mfma_i8" and hip.channelizer_reason() == ""
            runs.append(gw._feed_all(hip, iq, n_batches, bins=True))
    orc = pyoracle.Oracle(devices, wave_rate=8000, fft_log=10)
    ref = [orc.run_device(d, iq[d], n_batches) for d in range(n_dev)]
    for b, (x, y) in enumerate(zip(*runs)):
        for key in ("waveout", "w", "q"):
            assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (b, key)
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]) and x["stats"] == y["stats"]
        assert helpers.rel_rms(x["w"], np.concatenate([r["raw_wavein"][b] for r in ref])) <= 1e-5
        assert np.array_equal(x["axc"], np.concatenate([r["axc"][b] for r in ref]))


def test_pipelined_handle_is_the_sequential_one(pkg, built):
    """FLAG_PIPELINE | FLAG_WIDE_HOPS at CS16 fft 2048, 10 MS/s: results one process() late, bit-identical."""
    capi = pkg.capi
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 11, 10_000_000, 8000, n_dev, n_batches)
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=11, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
        want = gw._feed_all(hip, iq, n_batches)
    got = []
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=11, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS | capi.FLAG_PIPELINE) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8"
        pos = [0] * n_dev

        def take():
            out = hip.collect(stats=True)
            got.append(dict(axc=out["axc"].copy(), waveout=out["waveout"].copy(), stats=out["stats"], trace=hip.read_trace().copy()))

        for b in range(n_batches):
            for d in range(n_dev):
                raw = iq[d].view(np.uint8)
                pos[d] += hip.submit(d, raw[pos[d]:])
            assert hip.process()
            if b > 0:
                take()
        hip.flush()
        take()
    assert len(got) == n_batches
    for b, (x, y) in enumerate(zip(want, got)):
        assert np.array_equal(x["waveout"].view(np.uint32), y["waveout"].view(np.uint32)), b
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]) and x["stats"] == y["stats"], b


def test_afc_on_wide_windows(pkg, built):
    """CS16 fft 2048 at 6 MS/s (hops of 3 000 bytes) with channels that AFC moves: private tables re-tuned on the device, oracle parity as tests/test_gpu_afc.py
    defines it."""
    import test_gpu_afc as ta

    capi = pkg.capi
    case = helpers.afc_format_case(pkg, capi.SFMT_S16, 11, 6_000_000, 8000, [helpers.afc_plan(8)] * 2, ta.N_BATCHES)
    _, moved = ta.run_against_oracle(pkg, case, 11, 8000, flags=capi.FLAG_WIDE_HOPS, name="dft_mfma_i8", what="SFMT_S16, fft 2048, 6 MS/s, WAVE_RATE 8000, wide hops")
    assert moved > 0 and case["ups"] > 0 and case["downs"] > 0


def test_hip_matches_the_golden(pkg, built):
    z, c, devices, iq = ww.load_golden()
    with pkg.AirbandHip(devices, wave_rate=c["wave_rate"], fft_log=c["fft_log"], flags=pkg.capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8"
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
