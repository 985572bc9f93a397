"""AIRBAND_HIP_FLAG_WIDE_HOPS on the GPU (csrc/channelizer_dft_wide.hip): devices above ~4 MS/s on the int8 matrix-core channelizer -- parity with the oracle at
every shape of the issue's table, against the wavefront FFT on the same stream, the flag inert inside the ordinary limits, zero-copy spans sized to the byte,
the reasons a handle gives for its channelizer, pipelined handles, and the golden tests/golden/cs16_10000k.npz."""
import numpy as np
import pytest

import helpers
import pyoracle
import test_wide_hops as tw

pytestmark = pytest.mark.gpu


def _feed_all(hip, iq, n_batches, *, trace=True, bins=False, iq_out=False):
    """Every batch of the streams through the host path: [dict(axc, waveout, trace, stats[, w, q, iq_out])] per batch."""
    got, pos = [], [0] * len(iq)
    for b in range(n_batches):
        for d in range(len(iq)):
            raw = iq[d].view(np.uint8)
            pos[d] += hip.submit(d, raw[pos[d]:])
        assert hip.process(), "batch %d: not enough input queued" % b
        out = hip.collect(iq=iq_out, stats=True)
        r = dict(axc=out["axc"].copy(), waveout=out["waveout"].copy(), stats=out["stats"])
        if iq_out:
            r["iq_out"] = out["iq_out"].copy()
        if trace:
            r["trace"] = hip.read_trace().copy()
        if bins:
            w, q = hip.read_bins()
            r["w"], r["q"] = w.copy(), q.copy()
        got.append(r)
    return got


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", tw.GPU_CASES)
def test_wide_hop_parity(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """Two dongles, seven batches: squelch trace, axcindicate and counters exact, audio <= 1e-4 RMS, stage-1 bins within 1e-5 relative RMS of the oracle's
    (the bars of tests/test_gpu_parity.py), on the matrix-core channelizer by the flag."""
    capi = pkg.capi
    sfmt = getattr(capi, sfmt_name)
    n_dev, n_batches = 2, 7
    devices, iq = helpers.format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, n_dev, n_batches)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    ref = [orc.run_device(d, iq[d], n_batches) for d in range(n_dev)]
    assert all(r["n_batches"] == n_batches for r in ref)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8"
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
    """CS16 at 10 MS/s: the flagged handle (matrix cores) and the unflagged one (wavefront FFT) decide identically, audio within 1e-4 RMS of each other."""
    capi = pkg.capi
    n_dev, n_batches = 2, 5
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 9, 10_000_000, 8000, n_dev, n_batches)
    runs = {}
    for flag in (0, capi.FLAG_WIDE_HOPS):
        with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == ("dft_mfma_i8" if flag else "fft_wave64")
            if not flag:
                assert hip.channelizer_reason() == "hop 5000 bytes > 1280: AIRBAND_HIP_FLAG_WIDE_HOPS not set"
            runs[flag] = _feed_all(hip, iq, n_batches)
    for b, (x, y) in enumerate(zip(runs[0], runs[capi.FLAG_WIDE_HOPS])):
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"]), b
        assert helpers.rms(x["waveout"] - y["waveout"]) <= 1e-4
        for sx, sy in zip(x["stats"], y["stats"]):
            for key in ("open_count", "flappy_count", "active_counter", "bin"):
                assert sx[key] == sy[key]


@pytest.mark.parametrize("sfmt_name,sample_rate", [("SFMT_U8", 2_560_000), ("SFMT_S16", 2_400_000)])
def test_flag_is_inert_inside_the_ordinary_limits(pkg, built, sfmt_name, sample_rate):
    capi = pkg.capi
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, getattr(capi, sfmt_name), 9, sample_rate, 16000, n_dev, n_batches)
    for d in devices:
        d["channels"][3]["has_iq_outputs"] = 1
    runs = []
    for flag in (0, capi.FLAG_WIDE_HOPS):
        with pkg.AirbandHip(devices, wave_rate=16000, flags=capi.FLAG_TRACE_SQUELCH | flag) as hip:
            assert hip.channelizer_name() == "dft_mfma_i8" and hip.channelizer_reason() == ""
            runs.append(_feed_all(hip, iq, n_batches, bins=True, iq_out=True))
    for b, (x, y) in enumerate(zip(*runs)):
        for key in ("waveout", "iq_out", "w", "q"):
            assert np.array_equal(x[key].view(np.uint32), y[key].view(np.uint32)), (b, key)
        assert np.array_equal(x["axc"], y["axc"]) and np.array_equal(x["trace"], y["trace"])
        assert x["stats"] == y["stats"]


def test_zero_copy_spans_sized_to_the_byte(pkg, built):
    """process_device on CS16 at 10 MS/s (hops of 5 000 bytes: 8-byte alignment): one span at the very start of its allocation at an address that is 8 and not 16
    bytes aligned... the allocation of the last dongle ends where its span ends -- batch_bytes + lookahead_bytes and not a byte more -- so a read past the span is a
    read past the allocation.  Results equal the host path's bit for bit."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    n_dev, n_batches = 2, 3
    devices, iq = helpers.format_case(pkg, capi.SFMT_S16, 9, 10_000_000, 8000, n_dev, n_batches)
    flags = capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        want = _feed_all(hip, iq, n_batches, bins=True)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=flags) as hip:
        g = hip.geometry
        assert g.batch_bytes % 16 == 0 or True
        pos = 0
        for b in range(n_batches):
            nb = g.first_batch_bytes if b == 0 else g.batch_bytes
            span = nb + g.lookahead_bytes
            stride = (span + 7) // 8 * 8 + 8          # multiples of 8, not of 16, where the span's length allows: dongle 1 starts 8 bytes off a 16-byte boundary
            if stride % 16 == 0:
                stride += 8
            buf = torch.empty((stride + span,), dtype=torch.uint8, device="cuda")   # dongle 0 at the allocation's first byte, dongle 1's span ends at its last
            assert buf.data_ptr() % 16 == 0
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


def test_fallback_says_why(pkg, built):
    capi = pkg.capi
    # the geometry function rejects u8 at fft 8192: 16 rows of 16 KiB, twice
    assert pkg.wide_hop_lds_bytes(8192, 1500, capi.SFMT_U8) > 160 * 1024
    devices, _ = helpers.format_case(pkg, capi.SFMT_U8, 13, 6_000_000, 8000, 1, 1)
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=13, flags=capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == "fft_wave64"
        assert hip.channelizer_reason().startswith("wide hops: fft 8192 staging does not fit LDS")
    with pkg.AirbandHip(devices, wave_rate=8000, fft_log=13) as hip:
        assert hip.channelizer_name() == "fft_wave64"
        assert hip.channelizer_reason() == "hop 1500 bytes > 1024: AIRBAND_HIP_FLAG_WIDE_HOPS not set"
    devices, _ = helpers.format_case(pkg, capi.SFMT_S8, 9, 10_000_000, 8000, 1, 1)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_WIDE_HOPS | capi.FLAG_FORCE_FFT) as hip:
        assert hip.channelizer_name() == "fft_wave64" and hip.channelizer_reason() == "FORCE_FFT"


def test_pipelined_handle_is_the_sequential_one(pkg, built):
    """FLAG_PIPELINE | FLAG_WIDE_HOPS at s8 10 MS/s: results one process() late, bit-identical."""
    capi = pkg.capi
    n_dev, n_batches = 2, 5
    devices, iq = helpers.format_case(pkg, capi.SFMT_S8, 9, 10_000_000, 8000, n_dev, n_batches)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS) as hip:
        want = _feed_all(hip, iq, n_batches)
    got = []
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS | capi.FLAG_PIPELINE) as hip:
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


def test_hip_matches_wide_golden(pkg, built):
    import json

    z, c, devices, iq = tw.load_golden()
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


def test_afc_on_wide_hops(pkg, built):
    """CS16 at 6 MS/s (hops of 3 000 bytes) with channels that AFC moves, flag set: the batches run on the matrix-core channelizer (private tables re-tuned on the
    device, the last hop's spectrum from the wavefront FFT as on every matrix-core handle), oracle parity as tests/test_gpu_afc.py defines it."""
    import test_gpu_afc as ta

    capi = pkg.capi
    case = helpers.afc_format_case(pkg, capi.SFMT_S16, 9, 6_000_000, 8000, [helpers.afc_plan(8)] * 2, ta.N_BATCHES)
    _, moved = ta.run_against_oracle(pkg, case, 9, 8000, flags=capi.FLAG_WIDE_HOPS, name="dft_mfma_i8", what="SFMT_S16, fft 512, 6 MS/s, WAVE_RATE 8000, wide hops")
    assert moved > 0 and case["ups"] > 0 and case["downs"] > 0


@pytest.mark.timeout(900)
def test_sampled_dongles_of_a_large_wide_hop_handle(pkg, built):
    """CS16 at 10 MS/s in the WAVE_RATE 8000 build, 1 024 dongles x 8 channels, HBM-resident I/Q cycled the way tests/test_gpu_scale.py cycles it (first batch with
    its lead-in, then a ring of resident batches): eight distinct streams repeated over the fleet (odd dongles with their own CS16 full scale), sampled dongles --
    first, last, around the 16 / 128 placement groups, pseudo-random ones -- against oracle twins fed exactly those bytes."""
    torch = pytest.importorskip("torch")
    import pyverify

    capi = pkg.capi
    n_dev, n_batches, ring, distinct = 1024, 7, 3, 8
    devs8, iq8 = helpers.format_case(pkg, capi.SFMT_S16, 9, 10_000_000, 8000, distinct, ring + 1)
    devices = [devs8[d % distinct] for d in range(n_dev)]
    dongles = pyverify.sample_dongles(n_dev, 32)
    hip = pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_TRACE_SQUELCH | capi.FLAG_WIDE_HOPS)
    iq = spot = None
    try:
        assert hip.channelizer_name() == "dft_mfma_i8" and hip.channelizer_reason() == ""
        g = hip.geometry
        lead = g.first_batch_bytes - g.batch_bytes
        span = lead + (ring + 1) * g.batch_bytes + g.lookahead_bytes
        stride = (span + 255) // 256 * 256
        helpers.wait_for_gpu_memory(n_dev * stride + (1 << 30))
        iq = torch.empty((n_dev, stride), dtype=torch.uint8, device="cuda")
        for k in range(distinct):
            raw = iq8[k].view(np.uint8)
            assert len(raw) >= span
            iq[k::distinct, :span] = torch.from_numpy(raw[:span].copy()).cuda()
        torch.cuda.synchronize()
        host = {d: iq8[d % distinct].view(np.uint8)[:span] for d in dongles}
        assert np.array_equal(iq[n_dev - 1, :span].cpu().numpy(), host[n_dev - 1])
        spot = pyverify.SpotCheck(lambda d: devices[d], dongles, wave_rate=8000)

        def offset(i):
            return 0 if i == 0 else g.first_batch_bytes + ((i - 1) % ring) * g.batch_bytes

        opened, worst = 0, 0.0
        for i in range(n_batches):
            hip.process_device(iq.data_ptr() + offset(i), stride)
            spot.feed([host[d][offset(i):] for d in dongles])
            w = spot.compare(hip, trace=True, what="%d wide-hop dongles" % n_dev)
            worst = max(worst, w["audio_rms"])
            opened += sum(int((r["axc"] == ord("*")).sum()) for r in spot.last)
        assert opened > 0
        for d in (n_dev // 3, (2 * n_dev) // 3):
            r = hip.collect(first_channel=8 * d, n_channels=8)
            assert np.isfinite(r["waveout"]).all() and set(np.unique(r["axc"])) <= {ord(" "), ord("*")}
    finally:
        if spot is not None:
            spot.close()
        hip.close()
        del iq
    print("%d dongles, %d sampled: worst audio RMS error %.3g" % (n_dev, len(dongles), worst))
