"""Every wide-hop kernel variant (AIRBAND_HIP_FLAG_WIDE_HOPS: csrc/channelizer_dft_wide.hip, csrc/channelizer_f32_wide.hip) without a GPU: the table of sweep cases
tests/test_gpu_wide_variants.py runs -- one configuration per variant a flagged handle can select, found by scanning the public plan functions and not by reading
kernel source --, that the table is complete and sits on the edges of the selection, the coefficient tables at every case, and the C restatement pinned against the
reference at every case, on the eleven-channel plan of helpers.wide_case().

A VARIANT is what the launch code instantiates a kernel for:
  int8 family   (8-bit or CS16, fft size, AL = the largest of 16 / 8 / 4 / 2 that divides the hop's bytes, k-segments of the staging plan)
  CF32 family   (fft size, hop of an even or odd number of samples, segment launches of the staging plan)"""
import importlib

import numpy as np
import pytest

import helpers
import pyoracle
import test_wide_hops as tw

need_ref = tw.need_ref

FFT_SIZES = (256, 512, 1024, 2048, 4096, 8192)
MAX_HOP_BYTES_INT8, MAX_HOP_SAMPLES_F32 = 5000, 2500   # the required range: 20 MS/s of CS8 / CF32, 10 MS/s of CS16 at WAVE_RATE 8000

# (sample format, fft_log, hop in samples, WAVE_RATE); the sample rate is hop x WAVE_RATE.  Unless noted the hop is the FIRST wide hop of its class:
# u8 / s8 1 026 / 1 028 / 1 032 / 1 040 bytes = 513 / 514 / 516 / 520 samples (AL = 2 / 4 / 8 / 16); CS16 1 284 / 1 288 / 1 296 bytes = 321 / 322 / 324 samples
# (AL = 4 / 8 / 16); CF32 the first hop of each parity wide_hop_plan_f32() accepts.  u8 and s8 are one variant (a runtime XOR mask): they alternate.
_SWEEP_HOPS = [
    ("SFMT_U8", 8, 520, 8000), ("SFMT_S8", 8, 516, 16000), ("SFMT_U8", 8, 514, 8000), ("SFMT_S8", 8, 513, 16000),
    ("SFMT_S8", 9, 520, 16000), ("SFMT_U8", 9, 516, 8000), ("SFMT_S8", 9, 514, 8000), ("SFMT_U8", 9, 513, 16000),
    ("SFMT_U8", 10, 520, 16000), ("SFMT_S8", 10, 516, 8000), ("SFMT_U8", 10, 514, 16000), ("SFMT_S8", 10, 513, 8000),
    ("SFMT_S8", 11, 520, 8000), ("SFMT_U8", 11, 2500, 8000), ("SFMT_S8", 11, 514, 16000), ("SFMT_U8", 11, 513, 8000),   # (2 500 samples = 5 000 bytes: the large hop, AL = 8)
    ("SFMT_U8", 12, 520, 8000), ("SFMT_S8", 12, 516, 16000), ("SFMT_U8", 12, 514, 8000),                                # (fft 4096 at AL = 2 has no plan)
    ("SFMT_S16", 8, 324, 8000), ("SFMT_S16", 8, 322, 16000), ("SFMT_S16", 8, 321, 8000),
    ("SFMT_S16", 9, 324, 16000), ("SFMT_S16", 9, 322, 8000), ("SFMT_S16", 9, 321, 16000),
    ("SFMT_S16", 10, 324, 8000), ("SFMT_S16", 10, 1250, 8000), ("SFMT_S16", 10, 321, 16000),                            # (1 250 samples = 5 000 bytes: the large hop, AL = 8)
    ("SFMT_S16", 11, 324, 16000), ("SFMT_S16", 11, 322, 8000), ("SFMT_S16", 11, 321, 8000),
    ("SFMT_S16", 12, 324, 8000), ("SFMT_S16", 12, 322, 16000), ("SFMT_S16", 12, 321, 16000),
    ("SFMT_F32", 8, 394, 8000), ("SFMT_F32", 8, 393, 16000),
    ("SFMT_F32", 9, 376, 8000), ("SFMT_F32", 9, 377, 16000),
    ("SFMT_F32", 10, 512, 8000), ("SFMT_F32", 10, 529, 16000),   # (hops of 513 - 527 samples stay with the ordinary kernel)
    ("SFMT_F32", 11, 448, 16000), ("SFMT_F32", 11, 461, 8000),
    ("SFMT_F32", 12, 448, 8000), ("SFMT_F32", 12, 461, 16000),
    ("SFMT_F32", 13, 2500, 16000), ("SFMT_F32", 13, 461, 8000),  # (2 500 samples = 20 000 bytes, 2 100 hops in the first batch: the largest input)
]
SWEEP_CASES = [(f, n, h * w, w) for f, n, h, w in _SWEEP_HOPS]
SWEEP_IDS = ["%s-fft%d-hop%d-w%d" % (f[5:].lower(), 1 << n, h, w) for f, n, h, w in _SWEEP_HOPS]
# the process_device cases of the GPU file: none of them had run on a GPU -- 8-bit AL = 2 at fft 256 and fft 2048, CF32 odd hops at fft 512 and fft 4096
ZERO_COPY_CASES = [SWEEP_CASES[3], SWEEP_CASES[15], SWEEP_CASES[37], SWEEP_CASES[43]]


def _pkg():
    return importlib.import_module("rtlsdr-airband_amd")


def hop_alignment(hop_bytes):
    return next(a for a in (16, 8, 4, 2, 1) if hop_bytes % a == 0)


def variant_key(sfmt, fft, hop_samples):
    """The kernel variant a flagged handle runs at this shape, from the public plan functions and the hop's byte alignment alone; None where it has no wide plan
    (the ordinary kernels' shapes, shapes that stay on the wavefront FFT).  sfmt: a capi.SFMT_* name."""
    pkg = _pkg()
    capi = pkg.capi
    code = getattr(capi, sfmt)
    if code == capi.SFMT_F32:
        try:
            seg, _ = pkg.wide_hop_plan_f32(fft, hop_samples)
        except pkg.AirbandError:
            return None
        return ("cf32", fft, "odd" if hop_samples & 1 else "even", seg)
    hop_bytes = 2 * hop_samples * capi.BYTES_PER_SAMPLE[code]
    if pkg.wide_hop_lds_bytes(fft, hop_bytes, code) < 0:   # not a wide shape
        return None
    try:
        seg, _ = pkg.wide_hop_plan(fft, hop_bytes, code)
    except pkg.AirbandError:
        return None
    return ("cs16" if code == capi.SFMT_S16 else "8bit", fft, hop_alignment(hop_bytes), seg)


def case_key(case):
    sfmt, fft_log, sample_rate, wave_rate = case
    assert sample_rate % wave_rate == 0
    return variant_key(sfmt, 1 << fft_log, sample_rate // wave_rate)


_scan_cache = {}


def scan_variants():
    """{variant key: the first hop (in samples) that selects it} over the required range: every even hop length in bytes (CS16: multiples of 4) up to 5 000 bytes for
    the int formats, every hop up to 2 500 samples for CF32, fft 256 ... 8192.  u8 and s8 are scanned both and must agree."""
    if not _scan_cache:
        for fft in FFT_SIZES:
            for hop in range(1, MAX_HOP_BYTES_INT8 // 2 + 1):
                a, b = variant_key("SFMT_U8", fft, hop), variant_key("SFMT_S8", fft, hop)
                assert a == b, (fft, hop, a, b)
                if a is not None:
                    _scan_cache.setdefault(a, hop)
            for hop in range(1, MAX_HOP_BYTES_INT8 // 4 + 1):
                a = variant_key("SFMT_S16", fft, hop)
                if a is not None:
                    _scan_cache.setdefault(a, hop)
            for hop in range(1, MAX_HOP_SAMPLES_F32 + 1):
                a = variant_key("SFMT_F32", fft, hop)
                if a is not None:
                    _scan_cache.setdefault(a, hop)
    return _scan_cache


def test_sweep_covers_every_variant_once(built):
    """The table's keys are exactly the keys of the scan, one case each."""
    found = scan_variants()
    keys = [case_key(c) for c in SWEEP_CASES]
    assert None not in keys
    assert len(set(keys)) == len(keys), "two sweep cases on one variant"
    assert set(keys) == set(found), (sorted(set(found) - set(keys)), sorted(set(keys) - set(found)))
    per_family = {fam: sorted(k for k in found if k[0] == fam) for fam in ("8bit", "cs16", "cf32")}
    print({fam: len(v) for fam, v in per_family.items()})
    # what the dispatch code says, confirmed from the scan: every (fft 256 ... 4096) x (AL 16 / 8 / 4 / 2) for the 8-bit formats but fft 4096 at AL = 2, every
    # (fft 256 ... 4096) x (AL 16 / 8 / 4) for CS16 (a CS16 hop is whole samples: no AL = 2), nothing for the int formats at fft 8192, and every fft x parity for CF32
    int_ffts = [f for f in FFT_SIZES if f != 8192]
    assert {k[1:3] for k in per_family["8bit"]} == {(f, al) for f in int_ffts for al in (16, 8, 4, 2)} - {(4096, 2)}
    assert {k[1:3] for k in per_family["cs16"]} == {(f, al) for f in int_ffts for al in (16, 8, 4)}
    assert {k[1:3] for k in per_family["cf32"]} == {(f, p) for f in FFT_SIZES for p in ("even", "odd")}
    assert {k[3] for k in found if k[0] != "cf32"} == {1, 2, 4} and {k[3] for k in found if k[0] == "cf32"} == {1, 2, 4, 8}
    assert len(ZERO_COPY_CASES) == 4 and [case_key(c) for c in ZERO_COPY_CASES] == [("8bit", 256, 2, 1), ("8bit", 2048, 2, 1), ("cf32", 512, "odd", 1), ("cf32", 4096, "odd", 4)]


def test_sweep_hops_are_on_the_edges(pkg, built):
    """Every case sits on the first hop of its class -- the edge of the selection, where the plan and the map change -- except one large hop per family:
    5 000 bytes for the int formats, 2 500 samples for CF32."""
    capi = pkg.capi
    found = scan_variants()
    large = {"8bit": 0, "cs16": 0, "cf32": 0}
    for (sfmt, fft_log, sample_rate, wave_rate) in SWEEP_CASES:
        hop = sample_rate // wave_rate
        key = variant_key(sfmt, 1 << fft_log, hop)
        hop_bytes = 2 * hop * capi.BYTES_PER_SAMPLE[getattr(capi, sfmt)]
        if (hop_bytes == MAX_HOP_BYTES_INT8 and key[0] != "cf32") or (hop == MAX_HOP_SAMPLES_F32 and key[0] == "cf32"):
            large[key[0]] += 1
        else:
            assert hop == found[key], (sfmt, fft_log, hop, found[key])
    assert all(n >= 1 for n in large.values()), large
    # the edges themselves, as the dispatch code states them
    for fft in (256, 512, 1024, 2048):
        assert [2 * found[("8bit", fft, al, 1)] for al in (2, 4, 8, 16)] == [1026, 1028, 1032, 1040]
    for fft in (256, 512, 1024):
        assert [4 * found[("cs16", fft, al, 1)] for al in (4, 8, 16)] == [1284, 1288, 1296]
    assert (found[("cf32", 512, "even", 1)], found[("cf32", 512, "odd", 1)]) == (376, 377)
    assert (found[("cf32", 256, "odd", 1)], found[("cf32", 256, "even", 1)]) == (393, 394)
    assert found[("cf32", 1024, "even", 1)] == 512 and found[("cf32", 1024, "odd", 1)] >= 528
    assert all(variant_key("SFMT_F32", 1024, h) is None for h in range(513, 528))   # the ordinary kernel's own


def test_wide_case_plan(pkg, built):
    """helpers.wide_case(): dongle 0 is format_case's, dongle 1 has what no wide-hop GPU test had -- two column sets with the second partly filled, bins in the upper
    half, two channels on one bin, magnitude and raw I/Q from one lane, NFM lanes at WAVE_RATE 16000 -- at every sweep shape (the bins are the library's own)."""
    capi = pkg.capi
    for sfmt_name, fft_log, sample_rate, wave_rate in SWEEP_CASES:
        sfmt, n_fft = getattr(capi, sfmt_name), 1 << fft_log
        devices = helpers.wide_devices(capi, sfmt, sample_rate, wave_rate, 2)
        if (sfmt_name, fft_log, sample_rate, wave_rate) in (SWEEP_CASES[0], SWEEP_CASES[20]):   # (one case per WAVE_RATE: format_case also makes streams)
            assert devices[0] == helpers.format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, 1, 0)[0][0]
        assert len(devices[0]["channels"]) == 8 and len(devices[1]["channels"]) == 11
        consts = [pkg.derive_constants(devices, 8 + k, wave_rate=wave_rate, fft_log=fft_log) for k in range(11)]
        bins = [int(v[0]) for v in consts]
        assert sum(b >= n_fft // 2 for b in bins) >= 3, bins
        assert bins[4] == bins[5] and len(set(bins)) == 10, bins
        chans = devices[1]["channels"]
        assert [c["has_iq_outputs"] for c in chans] == [1 if k == 2 else 0 for k in range(11)] and chans[2]["modulation"] == 0
        assert [c["modulation"] for c in chans] == [1 if wave_rate == 16000 and k % 2 else 0 for k in range(11)]
        assert [bool(v[13]) for v in consts] == [k == 2 or (wave_rate == 16000 and k % 2 == 1) for k in range(11)]   # who stores raw I/Q
        if sfmt == capi.SFMT_S16:
            assert devices[0]["fullscale"] != devices[1]["fullscale"] and min(devices[0]["fullscale"], devices[1]["fullscale"]) > 0


@pytest.mark.parametrize("case", SWEEP_CASES, ids=SWEEP_IDS)
def test_tables_selftest_at_every_variant(pkg, built, case):
    """The coefficient tables of both plans of a sweep case, in the order the case's kernel contracts them: 1e-6 (tests/test_dft_tables.py's bar)."""
    sfmt_name, fft_log, sample_rate, wave_rate = case
    devices = helpers.wide_devices(pkg.capi, getattr(pkg.capi, sfmt_name), sample_rate, wave_rate, 2)
    err = pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2, flags=pkg.capi.FLAG_WIDE_HOPS)
    print("table error", case, err)
    assert err <= 1e-6


@need_ref
@pytest.mark.parametrize("case", SWEEP_CASES, ids=SWEEP_IDS)
def test_oracle_is_the_reference_at_every_variant(pkg, built, case):
    """The C restatement against the reference itself on the eleven-channel dongle of every sweep case, two batches: audio, axcindicate and the bin / dm_dphi constants
    bit for bit (tests/test_wide_hops.py's comparison).  The stream is the one the GPU sweep feeds its dongle 1: about 1 % of its samples are on a rail."""
    sfmt_name, fft_log, sample_rate, wave_rate = case
    n_batches, info = 2, {}
    devices, iq = helpers.wide_case(pkg, getattr(pkg.capi, sfmt_name), fft_log, sample_rate, wave_rate, 2, n_batches, only=(1,), info=info)
    assert 0.003 <= info["railed"][1] <= 0.03, info
    dev, x = [devices[1]], iq[1]
    ref = tw._reference_run(dev, [x], n_batches, nfm=wave_rate == 16000, fft_log=fft_log)[0]
    orc = pyoracle.Oracle(dev, wave_rate=wave_rate, fft_log=fft_log)
    try:
        got = orc.run_device(0, x, n_batches)
        assert ref["n_batches"] == got["n_batches"] == n_batches
        assert np.array_equal(ref["axc"], got["axc"])
        assert np.array_equal(ref["waveout"].view(np.uint32), got["waveout"].view(np.uint32))
        for j in range(len(dev[0]["channels"])):
            assert ref["consts"][j][0] == orc.constants(0, j)[0], j   # bin
            assert ref["consts"][j][1] == orc.constants(0, j)[1], j   # dm_dphi
            assert helpers.rms(got["raw_wavein"][:, j]) > 0.0           # the tone is on the channel's bin: no comparison of the GPU sweep is empty
    finally:
        orc.close()
