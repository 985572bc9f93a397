"""AIRBAND_HIP_FLAG_WIDE_HOPS for CF32 dongles without a GPU (csrc/channelizer_f32_wide.hip, csrc/f32_wide_map.h): the staging plan over the whole required range,
the kernel's address map compiled for the host (tests/host_f32_wide_map.cpp), the float tables in the wide kernel's order (flag set: checked; not set: refused),
the interface, the C restatement pinned against the reference at every configuration tests/test_gpu_wide_hops_f32.py runs, and the golden
tests/golden/cf32_8000k.npz (tests/golden/make_golden_wide_f32.py)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers
import pyoracle
import pyref
import test_wide_variants

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "rtlsdr-airband_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_golden_wide_f32  # noqa: E402

LDS_CU = 160 * 1024
# (fft_log, sample rate, WAVE_RATE, batches) of the GPU parity cases: disjoint windows; hops of an odd number of samples (625); overlapping rows (hops of 750 samples
# under a window of 1 024); the shape prepare() refuses without the flag (2 500 samples); and fft 2048, whose window is staged in two segments (two launches)
GPU_CASES = [(9, 8_000_000, 8000, 7), (8, 10_000_000, 16000, 7), (10, 6_000_000, 8000, 7), (9, 20_000_000, 8000, 5), (11, 8_000_000, 8000, 5)]
HOPS = [1000, 625, 750, 2500, 1000]


def _devices(pkg, sample_rate, n_ch=8):
    chans = [dict(frequency=120_000_000 + int((k - 3.5) * 0.09 * sample_rate), modulation=0) for k in range(n_ch)]
    return [dict(channels=chans, sample_rate=sample_rate, sfmt=pkg.capi.SFMT_F32, fullscale=0.0)]


def test_cases_are_the_hops_named(pkg):
    for (f, r, w, _), hop in zip(GPU_CASES, HOPS):
        assert round(r / w) == hop


def _first_refused(pkg, fft):
    """the first hop f32_supported() refuses = the first one with a wide plan (the plan function answers EBADSIZE inside the ordinary limits)"""
    for hop in range(8, 2501):
        try:
            pkg.wide_hop_plan_f32(fft, hop)
            return hop
        except pkg.AirbandError as e:
            assert e.code == pkg.capi.EBADSIZE
    return None


def test_plan_over_the_required_range(pkg, built):
    """fft 256 / 512 / 1024, every hop (even and odd) from the first one the ordinary kernel refuses up to 2 500 samples (20 MS/s at WAVE_RATE 8000): one segment, one
    image of 16 x (window + 16) bytes + the exchange area of the waves, within a CU's 163 840 bytes whatever the hop.  The last supported hop has no plan."""
    for fft in (256, 512, 1024):
        first = _first_refused(pkg, fft)
        assert first is not None and first <= 760, (fft, first)
        nw = 4 if fft <= 512 else 8
        want = 16 * (8 * fft + 16) + 2 * (nw - 1) * 64 * 16
        ordinary = []
        for hop in range(first, 2501):
            try:
                seg, lds = pkg.wide_hop_plan_f32(fft, hop)
            except pkg.AirbandError as e:
                assert e.code == pkg.capi.EBADSIZE
                ordinary.append(hop)
                continue
            assert seg == 1 and lds == want and lds <= LDS_CU, (fft, hop, seg, lds)
        # The ordinary kernel's limit is not monotonic in the hop near its edge (its staged image is padded differently for hops that are multiples of 32 samples, odd
        # hops carry 16 bytes more): a few hops beyond the first refused one are still its own.  Those -- and only those -- have no wide plan: an unflagged
        # configuration at such a hop is on the ordinary float kernel, which is what the table self-test accepts without the flag.
        assert len(ordinary) <= 16 and all(h < first + 64 for h in ordinary), (fft, ordinary)
        for hop in ordinary:
            assert pkg.dft_selftest(_devices(pkg, hop * 8000), wave_rate=8000, fft_log=fft.bit_length() - 1, windows=1) <= 1e-6
        with pytest.raises(pkg.AirbandError) as e:
            pkg.wide_hop_plan_f32(fft, first - 1)
        assert e.value.code == pkg.capi.EBADSIZE
        print("fft %d: wide from hops of %d samples, %d bytes of LDS; hops beyond that the ordinary kernel still takes: %s" % (fft, first, want, ordinary))
    # at the rates the issue names the ordinary kernel's cap is what the issue says: fft 512 takes 375 samples and not 376
    assert _first_refused(pkg, 512) == 376
    # beyond the required sizes: segments of 1 024 samples, one launch each
    for fft, want_seg in ((2048, 2), (4096, 4), (8192, 8)):
        try:
            seg, lds = pkg.wide_hop_plan_f32(fft, 1000)
            print("fft %d: planned, %d segments, %d bytes" % (fft, seg, lds))
            assert seg == want_seg and lds == 16 * (8 * 1024 + 16) + 2 * 7 * 64 * 16 <= LDS_CU
        except pkg.AirbandError as e:
            print("fft %d: refused" % fft)
            assert e.code == pkg.capi.EBADSIZE
    # the int-format helpers keep refusing CF32
    assert pkg.wide_hop_lds_bytes(512, 8000, pkg.capi.SFMT_F32) == -1
    with pytest.raises(pkg.AirbandError):
        pkg.wide_hop_plan(512, 8000, pkg.capi.SFMT_F32)
    with pytest.raises(pkg.AirbandError):
        pkg.wide_hop_plan_f32(500, 1000)


# ---- the address map (csrc/f32_wide_map.h), compiled for the host ----

@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("f32widemap") / "libf32widemap.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-I" + CSRC, "-o", out, os.path.join(HERE, "host_f32_wide_map.cpp")], check=True)
    lib = C.CDLL(out)
    lp = C.POINTER(C.c_long)
    lib.f32wm_geometry.argtypes = [C.c_int, C.POINTER(C.c_int)]
    lib.f32wm_walk.argtypes = [C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, lp, lp]
    return lib


def test_map_geometry(pkg, built, wm):
    for fft in (256, 512, 1024, 2048, 4096, 8192):
        g = (C.c_int * 7)()
        assert wm.f32wm_geometry(fft, g) == 0
        pitch, image, total, nw, seg, even, odd = g
        s = fft // seg
        assert pitch == 8 * s + 16 and (pitch // 16) % 2 == 1 and image == 16 * pitch and total == image + 2 * (nw - 1) * 64 * 16 <= LDS_CU
        assert (even, odd) == (s // 2, s // 2 + 1) and 16 * odd <= pitch
        assert pkg.wide_hop_plan_f32(fft, 2000) == (seg, total)   # the kernel's header and the library's plan are one


# the GPU shapes, one even and one odd hop more per fft size (the first refused hops among them), the segmented sizes, and every CF32 shape of the variant sweep
# (tests/test_wide_variants.py: the first wide hop of each parity at every fft size, 8192 and its eight segment launches included)
MAP_SHAPES = sorted(set([(1 << f, h) for (f, _, _, _), h in zip(GPU_CASES, HOPS)] + [(256, 393), (256, 700), (512, 376), (512, 625), (1024, 751), (1024, 1250), (2048, 625), (4096, 1250)]
                        + [(1 << n, r // w) for f, n, r, w in test_wide_variants.SWEEP_CASES if f == "SFMT_F32"]))


@pytest.mark.parametrize("fft,hop", MAP_SHAPES)
def test_address_map_exhaustively(wm, fft, hop):
    """Every (segment, tile, row, 16-byte piece) staged into a model of the image, then every fragment read of every wave, lane group and step: (a) every window byte
    of every hop inside [0, n_hops) is delivered from exactly the stream byte it is -- staged once, read once; (b) the 16 rows of one fragment read fall in 16
    different bank groups, aligned to 16 bytes (8 with odd hops); (c) no source lies more than 15 bytes in front of the span or past the last hop's window (which
    batch_bytes + lookahead_bytes covers).  Odd hops: spans that start on and 8 bytes behind a 16-byte boundary.  Batches: a first tile with negative hops, a whole
    batch of 1 000 hops, a batch shorter than a tile, one hop."""
    for mis in ((0, 8) if hop & 1 else (0,)):
        for n_hops, shift in ((40, 5), (1000, 0), (1016, 8), (3, 15), (1, 0)):
            counts, where = (C.c_long * 4)(), (C.c_long * 4)()
            rc = wm.f32wm_walk(fft, hop, mis, n_hops, shift, counts, where)
            assert rc == 0, (fft, hop, mis, n_hops, shift, rc, list(where))
            assert counts[1] == n_hops * 8 * fft and counts[0] > 0 and counts[2] > 0
    if not hop & 1:
        counts, where = (C.c_long * 4)(), (C.c_long * 4)()
        assert wm.f32wm_walk(fft, hop, 8, 40, 5, counts, where) == 2   # even hops: the span starts on 16 bytes (the alignment rule of airband_hip_process_device)


@pytest.mark.parametrize("fft_log,sample_rate,wave_rate", [c[:3] for c in GPU_CASES] + [(9, 10_000_000, 16000), (10, 10_000_000, 8000), (12, 8_000_000, 8000)])
def test_tables_selftest_honours_the_flag(pkg, built, fft_log, sample_rate, wave_rate):
    """The float tables, contracted in float32 in the order the wide kernel contracts them: 1e-6 (tests/test_dft_tables.py's bar).  Without the flag the configuration
    is refused as before."""
    devices = _devices(pkg, sample_rate)
    err = pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2, flags=pkg.capi.FLAG_WIDE_HOPS)
    print("table error", 1 << fft_log, sample_rate, wave_rate, err)
    assert err <= 1e-6
    with pytest.raises(pkg.AirbandError) as e:
        pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2)
    assert e.value.code == pkg.capi.EBADSIZE


def test_flag_changes_nothing_for_the_selftest_inside_the_limits(pkg, built):
    devices = _devices(pkg, 2_560_000)
    assert pkg.dft_selftest(devices, wave_rate=16000, flags=pkg.capi.FLAG_WIDE_HOPS) == pkg.dft_selftest(devices, wave_rate=16000)


def test_header_and_exports(pkg, built):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert re.search(r"int airband_hip_wide_hop_plan_f32\(int32_t fft_size, int32_t hop_samples, int32_t\* segments, int64_t\* lds_bytes\);", text)
    assert re.search(r"#define AIRBAND_HIP_ABI_VERSION 2u", text) and pkg.capi.ABI_VERSION == 2
    assert "channelizer_f32_wide.hip" in text
    # (EXPORTS itself is pinned by tests/test_abi.py to the header's names of letters and underscores; names with digits are listed in EXPORTS_F32)
    assert "airband_hip_wide_hop_plan_f32" in pkg.EXPORTS_F32 and not set(pkg.EXPORTS_F32) & set(pkg.EXPORTS)
    assert all(hasattr(pkg.load_library(), n) and re.search(r"\b%s\(" % n, text) for n in pkg.EXPORTS_F32)
    L = pkg.load_library()   # no GPU is touched
    seg, lds = C.c_int32(0), C.c_int64(0)
    assert L.airband_hip_wide_hop_plan_f32(512, 1000, C.byref(seg), C.byref(lds)) == 0 and (seg.value, lds.value) == (1, 71936)
    assert L.airband_hip_wide_hop_plan_f32(512, 1000, None, None) == 0
    assert L.airband_hip_wide_hop_plan_f32(512, 160, None, None) == pkg.capi.EBADSIZE


need_ref = pytest.mark.skipif(not (pyref.have_ref(True) and pyref.have_ref(False)), reason="oracle/_ref not built")


def _reference_run(devices, iq_list, n_batches, **kw):
    for _ in range(4):  # (the harness may come back a batch short: tests/test_oracle_vs_reference.py)
        ref = pyref.run_reference(devices, iq_list, n_batches, **kw)
        if all(r["n_batches"] == n_batches for r in ref):
            break
    return ref


@need_ref
@pytest.mark.parametrize("fft_log,sample_rate,wave_rate,n_batches", GPU_CASES)
def test_oracle_is_the_reference_at_wide_hops(pkg, built, fft_log, sample_rate, wave_rate, n_batches):
    """The C restatement against the reference itself on whole CF32 streams at every configuration the GPU cases measure against it: audio, axcindicate, statistics
    and the bin / dm_dphi constants bit for bit (tests/test_wide_hops.py's comparison)."""
    n_dev, n_batches = 2, 4
    devices, iq = helpers.format_case(pkg, pkg.capi.SFMT_F32, fft_log, sample_rate, wave_rate, n_dev, n_batches, first_dongle=5)
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
    z = np.load(os.path.join(GOLDEN, make_golden_wide_f32.NAME + ".npz"))
    c, devices, iq = make_golden_wide_f32.build_case()
    assert hashlib.sha256(iq.tobytes()).digest() == z["iq_sha256"].tobytes(), "synthetic I/Q generator no longer reproduces the fixture's input"
    assert json.loads(str(z["channels"])) == devices[0]["channels"]
    return z, c, devices, iq


def test_golden_is_small_and_shows_an_open_and_a_close():
    path = os.path.join(GOLDEN, make_golden_wide_f32.NAME + ".npz")
    assert os.path.getsize(path) <= 1 << 20
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
