"""Every wide-hop kernel variant on the GPU (AIRBAND_HIP_FLAG_WIDE_HOPS: csrc/channelizer_dft_wide.hip, csrc/channelizer_f32_wide.hip): the sweep of
tests/test_wide_variants.py -- one configuration per variant a flagged handle can select, on the first wide hop of its class, with two different channel plans on the
handle (helpers.wide_case) -- and a fuzz of random wide configurations, both against the float64 oracle's stage-1 bins with three bars:

  (a) relative RMS <= 1e-5 over a dongle's whole batch, magnitudes and raw I/Q (the bar of every channelizer);
  (b) the same 1e-5 on slices, each normalised by the dongle's whole-batch RMS: every channel's row, the hops of the batch's first 16-hop tile, the hops of its
      last one.  A correct kernel's error does not depend on the hop or the channel, so a slice meets what the whole meets; one misplaced row of a staged image, or
      a partial sum dropped on one tile, is a slice that is wrong by its own size and disappears in (a) among 8 000 values;
  (c) the worst element: max |got - oracle| over all (channel, hop) <= 1e-5 of the dongle's RMS.  DESIGN.md sections 2 and 4 measured 1e-7 ... 1e-6 relative RMS
      for these kernels; five deviations over at most 11 x 1 100 values are about 5e-6.

Tiles are 16 rows of the rings: read_bins() column t of batch b is ring row b x B + 100 + t (the first batch's 100 lead-in hops are not in it), so the first tile
of a batch's columns are those up to the next multiple of 16 of that row number and the last tile those from the last multiple on.  In the second batch the first
tile is the one the kernels stage with hops in front of the span (negative hops); both batches end inside a tile."""
import os

import numpy as np
import pytest

import helpers
import pyoracle
import test_wide_variants as tv

pytestmark = pytest.mark.gpu

BAR = 1e-5
KERNEL = {"8bit": "dft_mfma_i8", "cs16": "dft_mfma_i8", "cf32": "dft_mfma_f32"}
AGC_EXTRA = 100


def tile_columns(b, B):
    """(columns of read_bins() in the first ring tile of batch b, columns in its last)"""
    first_row, end_row = b * B + AGC_EXTRA, (b + 1) * B + AGC_EXTRA
    return np.arange(0, 16 - first_row % 16), np.arange(B - (end_row % 16 or 16), B)


def check_dongle(got, want, cols, what, pairs, rewritten=(), elem_bar=BAR):
    """Bars (a) - (c) for one dongle's [channels][B x pairs] array of one batch.  Returns (whole, worst slice, worst element), all relative to the dongle's RMS.
    rewritten: rows that are no longer stage 1's output (rewritten_rows) and are left out.  elem_bar: bar (c) where a caller has its own (tests/test_gpu_ordinary_variants.py)."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    for c in rewritten:
        got[c] = want[c]
    norm = helpers.rms(want)
    if norm == 0.0:   # a dongle without raw-I/Q channels: nothing is stored, nothing is read
        assert not got.any(), what
        return 0.0, 0.0, 0.0
    err = got - want
    whole = helpers.rms(err) / norm
    slices = {"channel %d" % c: helpers.rms(err[c]) / norm for c in range(err.shape[0])}
    for name, t in zip(("first tile", "last tile"), cols):
        idx = t if pairs == 1 else np.concatenate([2 * t, 2 * t + 1])
        slices[name] = helpers.rms(err[:, idx]) / norm
    worst_slice = max(slices, key=slices.get)
    at = np.unravel_index(np.argmax(np.abs(err)), err.shape)
    elem = float(np.abs(err[at])) / norm
    print("%s: whole %.3g, worst slice %.3g (%s), worst element %.3g (channel %d, column %d)" % (what, whole, slices[worst_slice], worst_slice, elem, at[0], at[1] // pairs))
    assert whole <= BAR, "%s: relative RMS %g" % (what, whole)
    assert slices[worst_slice] <= BAR, "%s: %s is off by %g of the dongle's RMS" % (what, worst_slice, slices[worst_slice])
    assert elem <= elem_bar, "%s: channel %d, column %d is off by %g of the dongle's RMS" % (what, at[0], at[1] // pairs, elem)
    return whole, slices[worst_slice], elem


def rewritten_rows(orc, d, device, ref):
    """The channels of a dongle whose MAGNITUDES read_bins() does not return as stage 1 wrote them: an AM channel that stores raw I/Q has them rewritten in place
    by stage 2 as soon as its squelch sees a signal (helpers.WIDE_SHUT_DBFS).  Stage 1's they stay where the channel has a manual squelch level and its magnitudes
    never come near it; the channel's raw I/Q is compared either way."""
    rows = []
    for c, ch in enumerate(device["channels"]):
        v = orc.constants(d, c)
        if ch["modulation"] == 0 and v[13] and not (v[10] > 0 and float(ref["raw_wavein"][:, c].max()) < 0.9 * v[10] and not (ref["trace"][:, c] & 7).any()):
            rows.append(c)
    return rows


def run_against_oracle(pkg, devices, iq, fft_log, wave_rate, n_batches, kernel, what, may_rewrite=False, flags=None, elem_bar=BAR, on_handle=None):
    """The streams through the host path of a handle (flags: AIRBAND_HIP_FLAG_WIDE_HOPS unless given), every batch's read_bins() against the oracle's raw_wavein /
    raw_iq dongle by dongle.  on_handle(hip, what): the caller's own look at the handle in front of the first batch.
    Returns (kernel name, worst whole-batch RMS, worst slice, worst element)."""
    capi = pkg.capi
    flags = capi.FLAG_WIDE_HOPS if flags is None else flags
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    try:
        ref = [orc.run_device(d, iq[d], n_batches) for d in range(len(devices))]
        rewritten = [rewritten_rows(orc, d, devices[d], ref[d]) for d in range(len(devices))]
    finally:
        orc.close()
    if any(rewritten):
        print("%s: magnitudes rewritten by stage 2, left out: %s" % (what, rewritten))
    assert may_rewrite or not any(rewritten), "%s: the squelch of an AM channel with raw I/Q saw a signal: %s" % (what, rewritten)
    assert all(r["n_batches"] == n_batches for r in ref), what
    for d, r in enumerate(ref):
        for c in range(r["raw_wavein"].shape[1]):
            assert helpers.rms(r["raw_wavein"][:, c]) > 0.0, "%s: dongle %d channel %d: the oracle's row is empty" % (what, d, c)
    worst = [0.0, 0.0, 0.0]
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=flags) as hip:
        name = hip.channelizer_name()
        what = "%s, %s" % (what, name)
        assert name == kernel, what
        assert hip.channelizer_reason() == "", what
        if on_handle is not None:
            on_handle(hip, what)
        B = hip.B
        pos = [0] * len(devices)
        for b in range(n_batches):
            for d in range(len(devices)):
                raw = iq[d].view(np.uint8)
                pos[d] += hip.submit(d, raw[pos[d]:])
            assert hip.process(), "%s: batch %d: not enough input queued" % (what, b)
            hip.collect()
            w, q = hip.read_bins()
            cols = tile_columns(b, B)
            k = 0
            for d, r in enumerate(ref):
                nc = len(devices[d]["channels"])
                for got, want, pairs, kind in ((w[k:k + nc], r["raw_wavein"][b], 1, "|bin|"), (q[k:k + nc], r["raw_iq"][b], 2, "bin I/Q")):
                    fig = check_dongle(got, want, cols, "%s; batch %d dongle %d %s" % (what, b, d, kind), pairs, rewritten[d] if pairs == 1 else (), elem_bar)
                    worst = [max(x, y) for x, y in zip(worst, fig)]
                k += nc
    return (name,) + tuple(worst)


@pytest.mark.parametrize("case", tv.SWEEP_CASES, ids=tv.SWEEP_IDS)
def test_wide_variant_sweep(pkg, built, case):
    """One configuration per kernel variant: 2 dongles (8 and 11 channels), 2 batches, host path, bars (a) - (c)."""
    sfmt_name, fft_log, sample_rate, wave_rate = case
    key = tv.case_key(case)
    devices, iq = helpers.wide_case(pkg, getattr(pkg.capi, sfmt_name), fft_log, sample_rate, wave_rate, 2, 2)
    what = "%s fft %d, hops of %d samples, WAVE_RATE %d, variant %s" % (sfmt_name, 1 << fft_log, sample_rate // wave_rate, wave_rate, key)
    name, whole, part, elem = run_against_oracle(pkg, devices, iq, fft_log, wave_rate, 2, KERNEL[key[0]], what)
    print("VARIANT | %s | %d | %d | %s | %s | %.2g | %.2g | %.2g |" % (sfmt_name[5:].lower(), 1 << fft_log, sample_rate // wave_rate,
                                                                     ("AL %d" % key[2]) if key[0] != "cf32" else key[2], key[3], whole, part, elem))


def feed_host(hip, iq, n_batches):
    got, pos = [], [0] * len(iq)
    for b in range(n_batches):
        for d in range(len(iq)):
            pos[d] += hip.submit(d, iq[d].view(np.uint8)[pos[d]:])
        assert hip.process()
        out = hip.collect()
        w, q = hip.read_bins()
        got.append(dict(waveout=out["waveout"].copy(), axc=out["axc"].copy(), w=w.copy(), q=q.copy()))
    return got


@pytest.mark.parametrize("case", tv.ZERO_COPY_CASES, ids=[tv.SWEEP_IDS[tv.SWEEP_CASES.index(c)] for c in tv.ZERO_COPY_CASES])
def test_zero_copy_spans_sized_to_the_byte(pkg, built, case):
    """process_device at hops whose alignment is 2 bytes (8-bit, an odd number of samples) and 8 bytes (CF32, an odd number of samples): dongle 1's span starts that
    far behind a 16-byte boundary and ends on the allocation's last byte (helpers.feed_zero_copy).  Bit-identical to the host path."""
    pytest.importorskip("torch")
    capi = pkg.capi
    sfmt_name, fft_log, sample_rate, wave_rate = case
    sfmt, key = getattr(capi, sfmt_name), tv.case_key(case)
    hop_bytes = 2 * (sample_rate // wave_rate) * capi.BYTES_PER_SAMPLE[sfmt]
    al = tv.hop_alignment(hop_bytes)
    assert al == (8 if key[0] == "cf32" else 2)
    n_batches = 2
    devices, iq = helpers.wide_case(pkg, sfmt, fft_log, sample_rate, wave_rate, 2, n_batches)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == KERNEL[key[0]] and hip.channelizer_reason() == ""
        want = feed_host(hip, iq, n_batches)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS) as hip:
        assert hip.channelizer_name() == KERNEL[key[0]]
        for b, out in enumerate(helpers.feed_zero_copy(hip, iq, n_batches, al)):
            for k in ("waveout", "w", "q"):
                assert np.array_equal(out[k].view(np.uint32), want[b][k].view(np.uint32)), (b, k)
            assert np.array_equal(out["axc"], want[b]["axc"]), b


# ---- fuzz ----

def first_wide_hop(sfmt_name, fft):
    return next(h for h in range(8, 2501) if tv.variant_key(sfmt_name, fft, h) is not None)


def random_wide_case(pkg, seed, n_batches=2):
    """(devices, iq, fft_log, wave_rate, n_batches, variant key): a random configuration with a wide-hop plan -- sample format, an fft size that has a plan for it, a
    hop between the first wide one and 2 500 samples (half of the draws within 64 samples of that edge; even and odd; any alignment), 1 ... 4 dongles with 1 ... 8
    channels each (about one in five: 9 ... 24) at random frequencies, every dongle with its own plan and its own CS16 full scale -- and I/Q for it: noise plus a
    tone near every channel's bin at a random level, into the rails now and then.  Dongles are dropped from the draw where the streams would exceed 12 M samples."""
    capi = pkg.capi
    rng = np.random.default_rng(31_000 + seed)
    sfmt_name = ["SFMT_U8", "SFMT_S8", "SFMT_S16", "SFMT_F32"][int(rng.integers(0, 4))]
    sfmt = getattr(capi, sfmt_name)
    fft_log = int(rng.choice([8, 9, 10, 11, 12, 13] if sfmt == capi.SFMT_F32 else [8, 9, 10, 11, 12]))
    wave_rate = int(rng.choice([8000, 16000]))
    first = first_wide_hop(sfmt_name, 1 << fft_log)
    key = None
    for _ in range(100):   # (CF32 fft 1024 ... 8192: a few hops behind the first wide one are the ordinary kernel's; u8 / s8 fft 4096: odd hops have no plan)
        hop = int(rng.integers(first, first + 65)) if rng.random() < 0.5 else int(rng.integers(first, 2501))
        key = tv.variant_key(sfmt_name, 1 << fft_log, hop)
        if key is not None:
            break
    assert key is not None, "seed %d: no hop with a wide plan drawn for %s fft %d" % (seed, sfmt_name, 1 << fft_log)
    sample_rate = hop * wave_rate
    n = (n_batches * (wave_rate // 8) + 100) * hop + (1 << fft_log) + 8
    n_dev = max(1, min(int(rng.integers(1, 5)), 12_000_000 // n))
    devices, iq = [], []
    for d in range(n_dev):
        n_ch = int(rng.integers(9, 25)) if rng.random() < 0.2 else int(rng.integers(1, 9))
        chans = [helpers.wide_channel(120_000_000 + int(rng.uniform(-0.42, 0.42) * sample_rate / 1000) * 1000, modulation=int(rng.integers(0, 2)) if wave_rate == 16000 else 0,
                                      has_iq_outputs=int(rng.random() < 0.15)) for _ in range(n_ch)]
        gain = float(rng.choice([8.0, 50.0, 200.0])) if sfmt == capi.SFMT_S16 else 1.0
        devices.append(dict(channels=chans, sample_rate=sample_rate, sfmt=sfmt, fullscale=127.5 * gain if sfmt == capi.SFMT_S16 else 0.0))
        # (an AM channel with raw I/Q: squelch held shut and a tone under its level, helpers.WIDE_SHUT_DBFS; a strong neighbour may still open it: rewritten_rows)
        levels = [helpers.shut_squelch_tone(1 << fft_log) if c["squelch_threshold_dbfs"] == helpers.WIDE_SHUT_DBFS else float(10.0 ** rng.uniform(0.0, 1.9)) for c in chans]
        x, _ = helpers.tone_stream(pkg, devices[d], fft_log, wave_rate, n, rng, noise=float(rng.uniform(1.0, 25.0)), levels=levels, gain=gain)
        iq.append(x)
    return devices, iq, fft_log, wave_rate, n_batches, key


@pytest.mark.parametrize("seed", range(int(os.environ.get("AIRBAND_FUZZ_SEEDS_WIDE", "8"))))
def test_random_wide_configurations(pkg, built, seed):
    """Random wide configurations, always on a matrix-core kernel (the generator draws only shapes with a plan): bars (a) - (c), seed, kernel and shape in every message."""
    devices, iq, fft_log, wave_rate, n_batches, key = random_wide_case(pkg, seed)
    what = "seed %d: sfmt %d, fft %d, %d S/s, WAVE_RATE %d, variant %s, channels %s" % (seed, devices[0]["sfmt"], 1 << fft_log, devices[0]["sample_rate"], wave_rate, key,
                                                                                     [len(d["channels"]) for d in devices])
    name, whole, part, elem = run_against_oracle(pkg, devices, iq, fft_log, wave_rate, n_batches, KERNEL[key[0]], what, may_rewrite=True)
    print("FUZZ %s, %s: whole %.2g, slice %.2g, element %.2g" % (what, name, whole, part, elem))
