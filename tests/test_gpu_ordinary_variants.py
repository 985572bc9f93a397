"""Every variant of the ordinary matrix-core channelizers on the GPU (csrc/channelizer_dft.hip, csrc/channelizer_f32.hip: what an unflagged handle and bench.py
run): the sweep of tests/test_ordinary_variants.py -- one configuration per variant an unflagged handle can select, on the smallest hop of the variant, plus the
largest hops of the range, with two different channel plans on the handle (helpers.wide_case) --, zero-copy spans at the alignments nothing ran zero-copy, the
splits == 1 launch shape (one workgroup walks a whole batch) at the large windows, and a fuzz over the whole hop range.  Everything against the float64 oracle's
stage-1 bins with the three bars of tests/test_gpu_wide_variants.py (check_dongle there):

  (a) relative RMS <= 1e-5 over a dongle's whole batch, magnitudes and raw I/Q (the bar of every channelizer);
  (b) the same 1e-5 on slices, each normalised by the dongle's whole-batch RMS: every channel's row, the hops of the batch's first 16-hop ring tile, those of its last;
  (c) the worst element, max |got - oracle| as a share of the dongle's RMS: ELEM_BAR per channelizer, from MEASURED below.

MEASURED: the largest worst-element figure of the sweep per channelizer, against the oracle, with the case that produced it (one run of test_ordinary_variant_sweep
with (c) printed and not asserted).  Bar (c) is twice the figure -- the margin AWAY_BAR takes in tests/test_gpu_afc.py -- and 1e-5 wherever that is below 1e-5, so
that this file and the wide one read alike."""
import os

import numpy as np
import pytest

import helpers
import pyoracle
import test_ordinary_variants as tv
from test_gpu_wide_variants import BAR, check_dongle, feed_host, rewritten_rows, run_against_oracle, tile_columns

pytestmark = pytest.mark.gpu

KERNEL = {"8bit": "dft_mfma_i8", "cs16": "dft_mfma_i8", "cf32": "dft_mfma_f32"}
# channelizer: (worst element of the sweep as a share of the dongle's RMS, the case)
MEASURED = {
    "dft_mfma_i8": (1.7e-6, "u8-fft4096-hop34-w8000"),    # (its whole-batch RMS 1.2e-7, its worst slice 4.0e-7: the largest of the int8 cases too)
    "dft_mfma_f32": (2.9e-6, "f32-fft4096-hop10-w8000"),  # (2.2e-7 and 7.4e-7: the largest of the CF32 cases too)
}
ELEM_BAR = {name: max(BAR, 2.0 * fig) for name, (fig, _) in MEASURED.items()}   # 3.4e-6 and 5.8e-6 are below 1e-5: both families are held to 1e-5


def confirm_edge_hi_zero(key):
    """The one restated element of the key a handle reports (airband_hip_read_tables): asserted in front of the first batch."""
    def look(hip, what):
        info = hip.table_info()
        assert info["channelizer"] == KERNEL[key[0]], what
        if key[0] != "cf32":
            assert info["edge_hi_zero"] == key[4], "%s: the handle reports edge_hi_zero %s" % (what, info["edge_hi_zero"])
    return look


@pytest.mark.parametrize("case", tv.SWEEP_CASES, ids=tv.SWEEP_IDS)
def test_ordinary_variant_sweep(pkg, built, case):
    """One configuration per kernel variant (and the largest hops): 2 dongles (8 and 11 channels), 2 batches, host path, bars (a) - (c).  The second batch's first
    tile is the one staged with hops in front of the span; both batches end inside a tile (tile_columns)."""
    sfmt_name, fft_log, sample_rate, wave_rate = case
    key = tv.case_key(case)
    B = wave_rate // 8
    assert all((b * B + 100) % 16 for b in (1, 2))
    devices, iq = helpers.wide_case(pkg, getattr(pkg.capi, sfmt_name), fft_log, sample_rate, wave_rate, 2, 2)
    what = "%s fft %d, hops of %d samples, WAVE_RATE %d, variant %s" % (sfmt_name, 1 << fft_log, sample_rate // wave_rate, wave_rate, key)
    name, whole, part, elem = run_against_oracle(pkg, devices, iq, fft_log, wave_rate, 2, KERNEL[key[0]], what, flags=0, elem_bar=ELEM_BAR[KERNEL[key[0]]],
                                                 on_handle=confirm_edge_hi_zero(key))
    print("VARIANT | %s | %s | %d | %d | %s | %.2g | %.2g | %.2g |" % (name, sfmt_name[5:].lower(), 1 << fft_log, sample_rate // wave_rate, key[2:], whole, part, elem))


@pytest.mark.parametrize("case", tv.ZERO_COPY_CASES, ids=[tv.SWEEP_IDS[tv.SWEEP_CASES.index(c)] for c in tv.ZERO_COPY_CASES])
def test_ordinary_variants_zero_copy(pkg, built, case):
    """process_device at hops whose alignment is 2 bytes (8-bit, an odd number of samples) and 4 bytes (CS16, an odd number of samples): dongle 1's span starts
    that far behind a 16-byte boundary and ends on the allocation's last byte (helpers.feed_zero_copy).  CF32 layout 1 (an odd number of samples, hops of 8 mod 16
    bytes): channelizer_f32.hip fetches whole 16-byte pieces, the interface asks for spans and strides on 16 bytes whatever the hop and refuses others -- that refusal
    is asserted, and the spans start on 16 bytes and end on the allocation's last byte.  Bit-identical to the host path of the same case, which
    test_ordinary_variant_sweep holds to the oracle."""
    pytest.importorskip("torch")
    capi = pkg.capi
    sfmt_name, fft_log, sample_rate, wave_rate = case
    sfmt, key = getattr(capi, sfmt_name), tv.case_key(case)
    al = tv.hop_alignment(2 * (sample_rate // wave_rate) * capi.BYTES_PER_SAMPLE[sfmt])
    assert al == {"8bit": 2, "cs16": 4, "cf32": 8}[key[0]]
    misalign = 0 if key[0] == "cf32" else al
    n_batches = 2
    devices, iq = helpers.wide_case(pkg, sfmt, fft_log, sample_rate, wave_rate, 2, n_batches)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log) as hip:
        assert hip.channelizer_name() == KERNEL[key[0]] and hip.channelizer_reason() == ""
        want = feed_host(hip, iq, n_batches)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log) as hip:
        assert hip.channelizer_name() == KERNEL[key[0]]
        if key[0] == "cf32":   # (the pointer is refused for its value; the allocation covers both spans from there all the same)
            import torch
            stride = (int(hip.geometry.first_batch_bytes) + int(hip.geometry.lookahead_bytes) + 15) // 16 * 16
            spare = torch.zeros((2 * stride + 16,), dtype=torch.uint8, device="cuda")
            with pytest.raises(pkg.AirbandError) as e:
                hip.process_device(spare.data_ptr() + 8, stride)
            assert e.value.code == capi.EINVAL and "multiples of 16" in str(e.value)
        for b, out in enumerate(helpers.feed_zero_copy(hip, iq, n_batches, misalign)):
            for k in ("waveout", "w", "q"):
                assert np.array_equal(out[k].view(np.uint32), want[b][k].view(np.uint32)), (b, k)
            assert np.array_equal(out["axc"], want[b]["axc"]), b


# ---- the whole-batch walk: splits == 1 ----
# The launch cuts a work item's tiles into `splits` workgroups (csrc/airband_hip.cpp):
#   dft_args(), lines 212-216:  `int splits = (8192 + a.n_items - 1) / a.n_items;`  (then capped at a quarter of the staging steps)  -> 1 exactly from 8 192 work items on
#   f32_args(), lines 163-167:  `int splits = (2048 + a.n_items - 1) / a.n_items;`  (capped at a quarter of the tiles)              -> 1 exactly from 2 048 work items on
# A work item is a group of up to eight channels of one dongle, so dongles of 64 channels are eight items each.
ITEMS_FOR_ONE_SPLIT = {"dft_mfma_i8": 8192, "dft_mfma_f32": 2048}
WALK_CHANNELS = 64
WALK_CASES = [   # (sample format, fft_log, hop in samples, WAVE_RATE): the smallest hop of a variant each
    pytest.param("SFMT_U8", 10, 36, 8000, id="u8-fft1024"),
    pytest.param("SFMT_S8", 12, 33, 8000, id="s8-fft4096"),
    pytest.param("SFMT_U8", 13, 32, 8000, id="u8-fft8192-two-passes"),
    pytest.param("SFMT_S16", 11, 33, 8000, id="s16-fft2048"),
    pytest.param("SFMT_F32", 11, 9, 16000, id="f32-fft2048"),
    pytest.param("SFMT_F32", 13, 10, 16000, id="f32-fft8192-four-segments"),
]


def walk_device(capi, sfmt, sample_rate, wave_rate):
    """One dongle of 64 channels spread over the passband: AM, WAVE_RATE 16000: odd channels NFM (raw I/Q stored), channel 2 an AM channel with raw-I/Q outputs
    and its squelch held shut (helpers.wide_channel)."""
    chans = [helpers.wide_channel(120_000_000 + int((-0.42 + 0.84 * k / (WALK_CHANNELS - 1)) * sample_rate), modulation=1 if wave_rate == 16000 and k % 2 == 1 else 0,
                                  has_iq_outputs=1 if k == helpers.WIDE_PLAN_B_IQ_CHANNEL else 0) for k in range(WALK_CHANNELS)]
    return dict(channels=chans, sample_rate=sample_rate, sfmt=sfmt, fullscale=127.5 * 50.0 if sfmt == capi.SFMT_S16 else 0.0)


@pytest.mark.parametrize("sfmt_name,fft_log,hop,wave_rate", WALK_CASES)
def test_whole_batch_walk(pkg, built, sfmt_name, fft_log, hop, wave_rate):
    """The launch shape of a production fleet at the large windows: so many work items that splits == 1 and ONE workgroup walks a work item's whole batch through
    its staging buffers.  Every dongle carries the same 64-channel plan and the same stream (made once on the host, replicated on the GPU, process_device), two
    batches; dongle 0, a middle one and the last against the oracle (one 64-channel dongle) with bars (a) - (c), every other dongle's bins bit-identical to dongle 0's
    (CF32: to one of at most eight results, each of which is held to the oracle -- see max_kinds below).
    The handle does not report `splits`: what this test relies on is n_items (airband_hip_read_tables) against the formulas above."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    sfmt, n_fft, sample_rate, n_batches = getattr(capi, sfmt_name), 1 << fft_log, hop * wave_rate, 2
    key = tv.variant_key(sfmt_name, n_fft, hop)
    assert key is not None and tv.scan_variants()[key] == hop
    kernel = KERNEL[key[0]]
    need = ITEMS_FOR_ONE_SPLIT[kernel]
    n_dev = need // (WALK_CHANNELS // 8)
    assert (need + n_dev * 8 - 1) // (n_dev * 8) == 1 and (need + (n_dev - 1) * 8 - 1) // ((n_dev - 1) * 8) == 2   # the smallest such fleet
    dev = walk_device(capi, sfmt, sample_rate, wave_rate)
    rng = np.random.default_rng([7200, int(sfmt), fft_log, hop, wave_rate])
    n_samples = (n_batches * (wave_rate // 8) + 100) * hop + n_fft + 8
    levels = [helpers.shut_squelch_tone(n_fft) if c["squelch_threshold_dbfs"] == helpers.WIDE_SHUT_DBFS else 4.0 for c in dev["channels"]]   # 64 tones of 4 counts and the noise: 23.4 per rail
    x, _ = helpers.tone_stream(pkg, dev, fft_log, wave_rate, n_samples, rng, noise=6.0, levels=levels, gain=50.0 if sfmt == capi.SFMT_S16 else 1.0)
    raw = x.view(np.uint8)
    what = "walk: %s fft %d, hops of %d samples, %d dongles, variant %s" % (sfmt_name, n_fft, hop, n_dev, key)
    orc = pyoracle.Oracle([dev], wave_rate=wave_rate, fft_log=fft_log)
    try:
        ref = orc.run_device(0, x, n_batches)
        rewritten = rewritten_rows(orc, 0, dev, ref)
    finally:
        orc.close()
    assert ref["n_batches"] == n_batches and all(helpers.rms(ref["raw_wavein"][:, c]) > 0.0 for c in range(WALK_CHANNELS)), what
    chunk = 128   # dongles per read_bins
    # int8: integer digit sums, one order of recombination -- every dongle's bins are dongle 0's, bit for bit.  CF32: the wave that adds the NW = 8 pieces' float sums
    # starts from its own and takes the others in turn, and which wave that is rotates with the workgroup (csrc/channelizer_f32.hip, `fin = wg & (NW - 1)`), so
    # dongles differ in the last bit by the order of seven float additions: at most NW distinct results, and EVERY distinct one is held to the oracle
    max_kinds = 1 if key[0] != "cf32" else 8

    def held(w_d, q_d, b, d):
        for got, want, pairs, kind in ((w_d, ref["raw_wavein"][b], 1, "|bin|"), (q_d, ref["raw_iq"][b], 2, "bin I/Q")):
            check_dongle(got, want, tile_columns(b, B), "%s; batch %d dongle %d %s" % (what, b, d, kind), pairs, rewritten if pairs == 1 else (), ELEM_BAR[kernel])
    with pkg.AirbandHip([dev] * n_dev, wave_rate=wave_rate, fft_log=fft_log) as hip:
        assert hip.channelizer_name() == kernel and hip.channelizer_reason() == "", what
        info = hip.table_info()
        assert info["n_items"] == n_dev * (WALK_CHANNELS // 8) >= need, (what, info)
        if key[0] != "cf32":
            assert info["edge_hi_zero"] == key[4], (what, info)
        g, B, pos = hip.geometry, hip.B, 0
        for b in range(n_batches):
            nb = int(g.first_batch_bytes if b == 0 else g.batch_bytes)
            span = nb + int(g.lookahead_bytes)
            stride = (span + 15) // 16 * 16
            row = np.zeros(stride, np.uint8)
            row[:span] = raw[pos:pos + span]
            buf = torch.from_numpy(row).cuda().unsqueeze(0).repeat(n_dev, 1)
            assert buf.is_contiguous() and buf.data_ptr() % 16 == 0
            torch.cuda.synchronize()
            hip.process_device(buf.data_ptr(), stride)
            hip.collect(first_channel=0, n_channels=WALK_CHANNELS)
            kinds = []   # the distinct results among the dongles, bit for bit: (|bin|, bin I/Q, first dongle that has it)
            for d0 in range(0, n_dev, chunk):
                n = min(chunk, n_dev - d0)
                w, q = hip.read_bins(d0 * WALK_CHANNELS, n * WALK_CHANNELS)
                w, q = w.reshape(n, WALK_CHANNELS, B), q.reshape(n, WALK_CHANNELS, 2 * B)
                for d in (0, n_dev // 2, n_dev - 1):
                    if d0 <= d < d0 + n:
                        held(w[d - d0], q[d - d0], b, d)
                known = np.zeros(n, bool)
                for kw, kq, _ in kinds:
                    known |= (w.view(np.uint32) == kw.view(np.uint32)[None]).all(axis=(1, 2)) & (q.view(np.uint32) == kq.view(np.uint32)[None]).all(axis=(1, 2))
                for i in np.flatnonzero(~known):
                    if not any(np.array_equal(w[i].view(np.uint32), kw.view(np.uint32)) and np.array_equal(q[i].view(np.uint32), kq.view(np.uint32)) for kw, kq, _ in kinds):
                        assert len(kinds) < max_kinds, "%s; batch %d: dongle %d differs from the dongles %s" % (what, b, d0 + i, [k[2] for k in kinds])
                        held(w[i], q[i], b, d0 + i)
                        kinds.append((w[i].copy(), q[i].copy(), d0 + i))
            print("%s; batch %d: %d distinct result(s), first on dongles %s" % (what, b, len(kinds), [k[2] for k in kinds]))
            pos += nb
            del buf


# ---- fuzz ----

def random_ordinary_case(pkg, seed, n_batches=2):
    """(devices, iq, fft_log, wave_rate, n_batches, variant key): a random unflagged configuration -- sample format, fft size 256 ... 8192, a hop drawn UNIFORMLY from
    the whole range the ordinary kernel of that format supports at that fft size (tests/test_ordinary_variants.py's scan range: every alignment, hops next to both
    limits; CF32 hops f32_supported() refuses inside the range are drawn again), 1 ... 3 dongles with 1 ... 24 channels at random frequencies, every dongle with
    its own plan and its own CS16 full scale -- and I/Q for it: noise plus a tone near every channel's bin at a random level, into the rails now and then."""
    capi = pkg.capi
    rng = np.random.default_rng(47_000 + seed)
    sfmt_name = ["SFMT_U8", "SFMT_S8", "SFMT_S16", "SFMT_F32"][int(rng.integers(0, 4))]
    sfmt = getattr(capi, sfmt_name)
    fft_log = int(rng.integers(8, 14))
    n_fft = 1 << fft_log
    wave_rate = int(rng.choice([8000, 16000]))
    if sfmt == capi.SFMT_F32:
        lo, hi = tv.F32_FIRST_HOP, tv.f32_last_hop(n_fft)
    else:
        first, last, _ = tv.INT8_HOP_BYTES["cs16" if sfmt == capi.SFMT_S16 else "8bit"]
        per = 2 * capi.BYTES_PER_SAMPLE[sfmt]
        lo, hi = first // per, min(last // per, n_fft - 1)
    key = None
    for _ in range(100):
        hop = int(rng.integers(lo, hi + 1))
        key = tv.variant_key(sfmt_name, n_fft, hop)
        if key is not None:
            break
    assert key is not None, "seed %d: no supported hop drawn for %s fft %d" % (seed, sfmt_name, n_fft)
    sample_rate = hop * wave_rate
    n = (n_batches * (wave_rate // 8) + 100) * hop + n_fft + 8
    devices, iq = [], []
    for d in range(int(rng.integers(1, 4))):
        n_ch = int(rng.integers(1, 25))
        chans = [helpers.wide_channel(120_000_000 + int(rng.uniform(-0.42, 0.42) * sample_rate), modulation=int(rng.integers(0, 2)) if wave_rate == 16000 else 0,
                                      has_iq_outputs=int(rng.random() < 0.15)) for _ in range(n_ch)]
        gain = float(rng.choice([8.0, 50.0, 200.0])) if sfmt == capi.SFMT_S16 else 1.0
        devices.append(dict(channels=chans, sample_rate=sample_rate, sfmt=sfmt, fullscale=127.5 * gain if sfmt == capi.SFMT_S16 else 0.0))
        levels = [helpers.shut_squelch_tone(n_fft) if c["squelch_threshold_dbfs"] == helpers.WIDE_SHUT_DBFS else float(10.0 ** rng.uniform(0.0, 1.9)) for c in chans]
        x, _ = helpers.tone_stream(pkg, devices[d], fft_log, wave_rate, n, rng, noise=float(rng.uniform(1.0, 25.0)), levels=levels, gain=gain)
        iq.append(x)
    return devices, iq, fft_log, wave_rate, n_batches, key


@pytest.mark.parametrize("seed", range(int(os.environ.get("AIRBAND_FUZZ_SEEDS_ORDINARY", "8"))))
def test_random_ordinary_configurations(pkg, built, seed):
    """Random unflagged configurations, always on a matrix-core kernel: bars (a) - (c), seed, kernel and shape in every message."""
    devices, iq, fft_log, wave_rate, n_batches, key = random_ordinary_case(pkg, seed)
    what = "seed %d: sfmt %d, fft %d, %d S/s, WAVE_RATE %d, variant %s, channels %s" % (seed, devices[0]["sfmt"], 1 << fft_log, devices[0]["sample_rate"], wave_rate, key,
                                                                                     [len(d["channels"]) for d in devices])
    name, whole, part, elem = run_against_oracle(pkg, devices, iq, fft_log, wave_rate, n_batches, KERNEL[key[0]], what, may_rewrite=True, flags=0,
                                                 elem_bar=ELEM_BAR[KERNEL[key[0]]], on_handle=confirm_edge_hi_zero(key))
    print("FUZZ %s, %s: whole %.2g, slice %.2g, element %.2g" % (what, name, whole, part, elem))
