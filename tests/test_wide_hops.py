"""AIRBAND_HIP_FLAG_WIDE_HOPS without a GPU: the coefficient tables at wide-hop configurations (flag set: checked; not set: refused), the interface, the staging
geometry over the whole required range, the C restatement pinned against the reference at every configuration tests/test_gpu_wide_hops.py runs, and the
golden tests/golden/cs16_10000k.npz (tests/golden/make_golden_wide.py)."""
import ctypes as C
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

import helpers
import pyoracle
import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
import make_golden_wide  # noqa: E402

# (sample format, sample rate, WAVE_RATE) -> hop bytes: the devices the flag is about
WIDE_ROWS = [("SFMT_S16", 10_000_000, 8000), ("SFMT_S16", 10_000_000, 16000), ("SFMT_S16", 8_000_000, 8000), ("SFMT_S16", 6_000_000, 8000), ("SFMT_S16", 6_000_000, 16000),
             ("SFMT_S8", 10_000_000, 8000), ("SFMT_S8", 10_000_000, 16000), ("SFMT_S8", 8_000_000, 8000), ("SFMT_U8", 6_000_000, 8000)]
HOP_BYTES = [5000, 2500, 4000, 3000, 1500, 2500, 1250, 2000, 1500]
# what the GPU file runs: every row at fft 512, CS16 and s8 at 10 MS/s (WAVE_RATE 8000) also at fft 256 and 1024
GPU_CASES = [(f, 9, r, w) for f, r, w in WIDE_ROWS] + [(f, n, 10_000_000, 8000) for f in ("SFMT_S16", "SFMT_S8") for n in (8, 10)]
LDS_CU = 160 * 1024


def _devices(pkg, sfmt_name, sample_rate, n_ch=8):
    capi = pkg.capi
    sfmt = getattr(capi, sfmt_name)
    chans = [dict(frequency=120_000_000 + int((k - 3.5) * 0.09 * sample_rate), modulation=0) for k in range(n_ch)]
    return [dict(channels=chans, sample_rate=sample_rate, sfmt=sfmt, fullscale=0.0 if sfmt != capi.SFMT_S16 else 32768.0)]


def test_rows_are_the_hops_the_issue_names(pkg):
    for (f, r, w), hb in zip(WIDE_ROWS, HOP_BYTES):
        assert 2 * round(r / w) * pkg.capi.BYTES_PER_SAMPLE[getattr(pkg.capi, f)] == hb


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", [(f, 9, r, w) for f, r, w in WIDE_ROWS] + [("SFMT_S16", 10, 10_000_000, 8000)])
def test_tables_selftest_honours_the_flag(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """The coefficient tables do not depend on the hop: with the flag a wide-hop configuration is checked like any other (1e-6: tests/test_dft_tables.py's bar);
    without it the configuration is refused as before."""
    devices = _devices(pkg, sfmt_name, sample_rate)
    err = pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2, flags=pkg.capi.FLAG_WIDE_HOPS)
    print("table error", sfmt_name, 1 << fft_log, sample_rate, wave_rate, err)
    assert err <= 1e-6
    with pytest.raises(pkg.AirbandError) as e:
        pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2)
    assert e.value.code == pkg.capi.EBADSIZE


def test_flag_changes_nothing_for_the_selftest_inside_the_limits(pkg, built):
    devices = _devices(pkg, "SFMT_S16", 2_400_000)
    assert pkg.dft_selftest(devices, wave_rate=16000, flags=pkg.capi.FLAG_WIDE_HOPS) == pkg.dft_selftest(devices, wave_rate=16000)


def test_header_and_exports(pkg, built):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert re.search(r"#define AIRBAND_HIP_FLAG_WIDE_HOPS 0x80u", text)
    assert re.search(r"const char\* airband_hip_channelizer_reason\(const airband_hip_handle\* h\);", text)
    assert re.search(r"#define AIRBAND_HIP_ABI_VERSION 2u", text)
    assert pkg.capi.FLAG_WIDE_HOPS == 0x80 and pkg.capi.ABI_VERSION == 2
    L = pkg.load_library()
    for name in ("airband_hip_channelizer_reason", "airband_hip_wide_hop_lds_bytes"):
        assert name in pkg.EXPORTS
        getattr(L, name)
    assert L.airband_hip_channelizer_reason(None) == b""


def test_staging_fits_lds_over_the_required_range(pkg, built):
    """u8 / s8 / CS16 at fft 256, 512, 1024 and every even hop (CS16: multiples of 4 bytes) beyond the ordinary limits up to 5 000 bytes: two buffers and the
    exchange area fit a CU's 160 KiB.  The rows' LDS is 16 x (window + 16) per buffer whatever the hop."""
    capi = pkg.capi
    for sfmt in (capi.SFMT_U8, capi.SFMT_S8, capi.SFMT_S16):
        bps, limit, step = capi.BYTES_PER_SAMPLE[sfmt], (1280 if sfmt == capi.SFMT_S16 else 1024), (4 if sfmt == capi.SFMT_S16 else 2)
        for fft in (256, 512, 1024):
            np_ = max(1, fft // 512)
            win = 2 * fft * bps
            want = 2 * ((16 * (win + 16) + 1023) // 1024 * 1024) + (2 * (np_ - 1) * 64 * 16 if np_ > 1 else 0)
            for hop in range(limit + step, 5000 + 1, step):
                got = pkg.wide_hop_lds_bytes(fft, hop, sfmt)
                assert got == want and 0 < got <= LDS_CU, (sfmt, fft, hop, got)
            assert pkg.wide_hop_lds_bytes(fft, limit, sfmt) == -1                  # inside the ordinary limits: not a wide shape
            assert pkg.wide_hop_lds_bytes(fft, limit + step + 1, sfmt) == -1       # an odd number of bytes
    assert pkg.wide_hop_lds_bytes(512, 3002, capi.SFMT_S16) == -1                  # not whole CS16 samples
    assert pkg.wide_hop_lds_bytes(512, 5000, capi.SFMT_F32) == -1
    # beyond the required range: u8 / s8 fft 2048 fit, CS16 fft 2048 and everything from 4096 up do not (the handle then stays on the wavefront FFT and says so)
    assert 0 < pkg.wide_hop_lds_bytes(2048, 1500, capi.SFMT_U8) <= LDS_CU
    for sfmt, fft in ((capi.SFMT_S16, 2048), (capi.SFMT_U8, 4096), (capi.SFMT_U8, 8192), (capi.SFMT_S16, 8192)):
        assert pkg.wide_hop_lds_bytes(fft, 3000 if sfmt == capi.SFMT_S16 else 1500, sfmt) > LDS_CU


need_ref = pytest.mark.skipif(not (pyref.have_ref(True) and pyref.have_ref(False)), reason="oracle/_ref not built")


def _reference_run(devices, iq_list, n_batches, **kw):
    for _ in range(4):  # (the harness may come back a batch short: tests/test_oracle_vs_reference.py)
        ref = pyref.run_reference(devices, iq_list, n_batches, **kw)
        if all(r["n_batches"] == n_batches for r in ref):
            break
    return ref


@need_ref
@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", GPU_CASES)
def test_oracle_is_the_reference_at_wide_hops(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """The C restatement against the reference itself on whole streams at every configuration the GPU cases measure against it: audio, axcindicate, statistics and
    the bin / dm_dphi constants bit for bit (the comparison of tests/test_oracle_vs_reference.py::test_stream_bit_exact_other_formats)."""
    sfmt = getattr(pkg.capi, sfmt_name)
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, n_dev, n_batches, first_dongle=5)
    ref = [_reference_run([devices[d]], [iq[d]], n_batches, nfm=wave_rate == 16000, fft_log=fft_log)[0] for d in range(n_dev)]
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    opened = 0
    for d in range(n_dev):
        got = orc.run_device(d, iq[d], n_batches)
        assert ref[d]["n_batches"] == got["n_batches"] == n_batches
        assert np.array_equal(ref[d]["axc"], got["axc"])
        assert np.array_equal(ref[d]["waveout"].view(np.uint32), got["waveout"].view(np.uint32))
        opened += int((ref[d]["axc"] == ord("*")).sum())
        for j in range(8):
            a, b = ref[d]["stats"][j], orc.stats(d, j)
            for k in a:
                if k != "squelch_state":
                    assert a[k] == b[k], (d, j, k, a[k], b[k])
            assert ref[d]["consts"][j][0] == orc.constants(d, j)[0]
            assert ref[d]["consts"][j][1] == orc.constants(d, j)[1]
    assert opened > 0


def load_golden():
    z = np.load(os.path.join(GOLDEN, make_golden_wide.NAME + ".npz"))
    c, devices, iq = make_golden_wide.build_case()
    assert hashlib.sha256(iq.tobytes()).digest() == z["iq_sha256"].tobytes(), "synthetic I/Q generator no longer reproduces the fixture's input"
    assert json.loads(str(z["channels"])) == devices[0]["channels"]
    return z, c, devices, iq


def test_golden_is_small_and_shows_an_open_and_a_close():
    path = os.path.join(GOLDEN, make_golden_wide.NAME + ".npz")
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != make_golden_wide.NAME + ".npz")
    assert os.path.getsize(path) <= largest
    axc = np.load(path)["axc"]
    assert (axc == ord("*")).any() and (axc == ord(" ")).any()


def test_oracle_reproduces_wide_golden(built):
    z, c, devices, iq = load_golden()
    orc = pyoracle.Oracle(devices, wave_rate=c["wave_rate"], fft_log=c["fft_log"])
    got = orc.run_device(0, iq, c["n_batches"])
    assert got["n_batches"] == c["n_batches"]
    assert np.array_equal(got["axc"], z["axc"])
    assert np.array_equal(got["waveout"].view(np.uint32), z["waveout"].view(np.uint32))
    for j, want in enumerate(json.loads(str(z["stats"]))):
        have = orc.stats(0, j)
        for k in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "bin"):
            assert have[k] == want[k], (j, k)
        for k in ("noise_level", "signal_level", "squelch_level", "agcavgfast"):
            assert np.float32(have[k]) == np.float32(want[k]), (j, k)
