"""Wide hops at the window sizes whose two staging buffers do not fit a CU's LDS whole -- CS16 fft 2048, u8 / s8 fft 4096, CS16 fft 4096: k-segmented row staging
(csrc/channelizer_dft_wide.hip, csrc/dft_wide_map.h) -- without a GPU: the plan a flagged handle follows, the coefficient tables, the kernel's address map compiled
for the host and checked exhaustively, the C restatement pinned against the reference at every configuration tests/test_gpu_wide_windows.py runs, and the golden
tests/golden/cs16_10000k_fft2048.npz (tests/golden/make_golden_wide2048.py).

One shape of the issue's list is NOT on the kernel: u8 / s8 fft 4096 at hops of an odd number of samples (s8 10 MS/s, WAVE_RATE 16000: 1 250 bytes).  Its variant --
the five-dword fragment reader beside sums that live across the segments' staging -- spills 29 registers (13 with the two-ahead prefetch that was tried), and a
spilling variant is not shipped: the handle stays on the wavefront FFT and says so (tests/test_gpu_wide_windows.py::test_odd_hops_at_fft_4096_stay_on_the_wavefront_fft)."""
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
import test_wide_hops as tw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "rtlsdr-airband_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
import make_golden_wide2048  # noqa: E402

LDS_CU = 160 * 1024
# (sample format, fft_log, sample rate, WAVE_RATE): what tests/test_gpu_wide_windows.py runs against the oracle
GPU_CASES = [("SFMT_S16", 11, 10_000_000, 8000), ("SFMT_S16", 11, 10_000_000, 16000), ("SFMT_S16", 11, 6_000_000, 8000),
             ("SFMT_S8", 12, 10_000_000, 8000), ("SFMT_U8", 12, 6_000_000, 8000),
             ("SFMT_S16", 12, 10_000_000, 8000), ("SFMT_S16", 12, 8_000_000, 8000)]
ODD_HOP_CASE = ("SFMT_S8", 12, 10_000_000, 16000)  # hops of 1 250 bytes: not on the kernel (module docstring)


def _plan_rc(pkg, fft, hop, sfmt):
    try:
        return pkg.wide_hop_plan(fft, hop, sfmt)
    except pkg.AirbandError as e:
        return e.code


def test_plan_of_the_new_shapes(pkg, built):
    capi = pkg.capi
    # image = roundup(16 NP (S + 16), 1 KiB), total = 2 image + 2 (NP - 1) KiB
    assert pkg.wide_hop_plan(2048, 5000, capi.SFMT_S16) == (2, 2 * 66560 + 2 * 3 * 1024) == (2, 139264)
    for sfmt in (capi.SFMT_U8, capi.SFMT_S8):
        assert pkg.wide_hop_plan(4096, 2500, sfmt) == (2, 2 * 67584 + 2 * 7 * 1024) == (2, 149504)
    assert pkg.wide_hop_plan(4096, 5000, capi.SFMT_S16) == (4, 149504)
    for hop in (1500, 2500, 3000, 4000, 5000):
        assert pkg.wide_hop_plan(2048, hop, capi.SFMT_S16)[0] == 2 and pkg.wide_hop_plan(4096, hop, capi.SFMT_S16)[0] == 4
    for hop in (1500, 2000, 2500, 1252):
        assert pkg.wide_hop_plan(4096, hop, capi.SFMT_S8)[0] == 2


def test_plan_keeps_one_segment_wherever_whole_windows_fit(pkg, built):
    """Every shape of tests/test_wide_hops.py's required range (and u8 / s8 fft 2048): one segment, the LDS of airband_hip_wide_hop_lds_bytes()."""
    capi = pkg.capi
    for sfmt in (capi.SFMT_U8, capi.SFMT_S8, capi.SFMT_S16):
        limit, step = (1280 if sfmt == capi.SFMT_S16 else 1024), (4 if sfmt == capi.SFMT_S16 else 2)
        for fft in (256, 512, 1024) + ((2048,) if sfmt != capi.SFMT_S16 else ()):
            for hop in range(limit + step, 5000 + 1, step):
                seg, lds = pkg.wide_hop_plan(fft, hop, sfmt)
                assert seg == 1 and lds == pkg.wide_hop_lds_bytes(fft, hop, sfmt) and 0 < lds <= LDS_CU, (sfmt, fft, hop, seg, lds)


def test_plan_fits_lds_wherever_there_is_one(pkg, built):
    capi = pkg.capi
    for sfmt in (capi.SFMT_U8, capi.SFMT_S8, capi.SFMT_S16):
        for fft in (256, 512, 1024, 2048, 4096, 8192):
            for hop in (1284, 1500, 2000, 2500, 3000, 4000, 5000, 1250, 1026):
                r = _plan_rc(pkg, fft, hop, sfmt)
                if isinstance(r, tuple):
                    assert r[0] in (1, 2, 4) and 0 < r[1] <= LDS_CU, (sfmt, fft, hop, r)
                else:
                    assert r == capi.EBADSIZE


def test_no_plan(pkg, built):
    capi = pkg.capi
    for sfmt, hop in ((capi.SFMT_U8, 1500), (capi.SFMT_S8, 2500), (capi.SFMT_S16, 5000)):
        assert _plan_rc(pkg, 8192, hop, sfmt) == capi.EBADSIZE           # the two-pass partial sums are not in this kernel
    assert _plan_rc(pkg, 2048, 5000, capi.SFMT_F32) == capi.EBADSIZE
    assert _plan_rc(pkg, 2048, 5001, capi.SFMT_S8) == capi.EBADSIZE      # an odd number of bytes
    assert _plan_rc(pkg, 2048, 3002, capi.SFMT_S16) == capi.EBADSIZE     # not whole CS16 samples
    assert _plan_rc(pkg, 2048, 1280, capi.SFMT_S16) == capi.EBADSIZE     # inside the ordinary limits
    assert _plan_rc(pkg, 4096, 1024, capi.SFMT_U8) == capi.EBADSIZE
    assert _plan_rc(pkg, 4096, 320, capi.SFMT_U8) == capi.EBADSIZE


def test_odd_hops_at_fft_4096_have_no_plan(pkg, built):
    """u8 / s8 fft 4096 at hops of an odd number of samples: the segmented kernel's AL = 2 variant spills registers and is not built (module docstring); the same hops
    with whole windows (one segment) keep their plan."""
    capi = pkg.capi
    for sfmt in (capi.SFMT_U8, capi.SFMT_S8):
        assert _plan_rc(pkg, 4096, 1250, sfmt) == capi.EBADSIZE
        assert _plan_rc(pkg, 4096, 1254, sfmt) == capi.EBADSIZE
        assert pkg.wide_hop_plan(2048, 1250, sfmt)[0] == 1
        assert pkg.wide_hop_lds_bytes(4096, 1250, sfmt) > LDS_CU


def test_header_and_exports(pkg, built):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert re.search(r"int airband_hip_wide_hop_plan\(int32_t fft_size, int32_t hop_bytes, int32_t sample_format, int32_t\* segments, int64_t\* lds_bytes\);", text)
    assert re.search(r"#define AIRBAND_HIP_ABI_VERSION 2u", text)
    assert "airband_hip_wide_hop_plan" in pkg.EXPORTS
    L = pkg.load_library()
    assert L.airband_hip_wide_hop_plan(2048, 5000, pkg.capi.SFMT_S16, None, None) == 0    # either out-pointer may be NULL


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", [GPU_CASES[0], GPU_CASES[3], GPU_CASES[5]])
def test_tables_selftest_at_the_new_shapes(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    devices = tw._devices(pkg, sfmt_name, sample_rate)
    err = pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2, flags=pkg.capi.FLAG_WIDE_HOPS)
    print("table error", sfmt_name, 1 << fft_log, sample_rate, wave_rate, err)
    assert err <= 1e-6
    with pytest.raises(pkg.AirbandError) as e:
        pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2)
    assert e.value.code == pkg.capi.EBADSIZE


def test_tables_selftest_follows_the_plan(pkg, built):
    """The selftest admits what prep_channelizer() admits: no plan (fft 8192; odd hops at fft 4096), no selftest, flag or no flag."""
    for sfmt_name, fft_log, sample_rate, wave_rate in (("SFMT_S16", 13, 10_000_000, 8000), ODD_HOP_CASE):
        with pytest.raises(pkg.AirbandError) as e:
            pkg.dft_selftest(tw._devices(pkg, sfmt_name, sample_rate), wave_rate=wave_rate, fft_log=fft_log, windows=1, flags=pkg.capi.FLAG_WIDE_HOPS)
        assert e.value.code == pkg.capi.EBADSIZE


# ---- the address map (csrc/dft_wide_map.h), compiled for the host ----

# shape id of tests/host_wide_map.cpp -> (bytes per window piece, pieces, segments, the alignment-class hops of the format: AL = 16 / 8 / 4 [/ 2])
MAP_SHAPES = {0: (2048, 4, 2, (4000, 5000, 2500)), 1: (1024, 8, 2, (2000, 1500, 1250)), 2: (2048, 8, 4, (4000, 5000, 2500)), 3: (2048, 1, 1, (4000, 5000, 2500))}
# ... and the one-segment shapes of every other (format, fft size) launch_channelizer_dft_wide() selects, each at the FIRST wide hop of every alignment class
# (tests/test_wide_variants.py: the edge of the selection) -- u8 / s8: 1 040 / 1 032 / 1 028 / 1 026 bytes (AL = 16 / 8 / 4 / 2), CS16: 1 296 / 1 288 / 1 284
WIDE_HOPS_8BIT, WIDE_HOPS_CS16 = (1040, 1032, 1028, 1026), (1296, 1288, 1284)
MAP_SHAPES.update({4: (512, 1, 1, WIDE_HOPS_8BIT),      # u8 / s8 fft 256
                   5: (1024, 1, 1, WIDE_HOPS_8BIT),     # u8 / s8 fft 512
                   6: (1024, 1, 1, WIDE_HOPS_CS16),     # CS16 fft 256
                   7: (1024, 2, 1, WIDE_HOPS_8BIT),     # u8 / s8 fft 1024
                   8: (2048, 2, 1, WIDE_HOPS_CS16),     # CS16 fft 1024
                   9: (1024, 4, 1, WIDE_HOPS_8BIT)})    # u8 / s8 fft 2048


@pytest.fixture(scope="module")
def wm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("widemap") / "libwidemap.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-I" + CSRC, "-o", out, os.path.join(HERE, "host_wide_map.cpp")], check=True)
    lib = C.CDLL(out)
    lp, ip = C.POINTER(C.c_long), C.POINTER(C.c_int)
    lib.wm_geometry.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip]
    lib.wm_span_end.argtypes = [C.c_int, C.c_long, C.c_int, C.c_int]
    lib.wm_span_end.restype = C.c_long
    lib.wm_delta.argtypes = [C.c_long, C.c_long, C.c_int]
    lib.wm_sources.argtypes = [C.c_int, C.c_long, C.c_long, C.c_int, C.c_int, C.c_long, lp]
    lib.wm_frags.argtypes = [C.c_int, C.c_int, C.c_int, ip]
    return lib


def _geometry(wm, shape):
    win, np_, seg, _ = MAP_SHAPES[shape]
    g = (C.c_int * 7)()
    assert wm.wm_geometry(shape, win, np_, seg, g) == 0
    return dict(zip(("n_sub", "s", "pitch", "image", "n_dma", "total", "plan"), g))


def test_map_geometry_is_the_issues_table(wm):
    want = {0: (1024, 66560, 139264, 2), 1: (512, 67584, 149504, 2), 2: (512, 67584, 149504, 4), 3: (2048, 33792, 67584, 1)}
    for shape, (s, image, total, plan) in want.items():
        win, np_, seg, _ = MAP_SHAPES[shape]
        g = _geometry(wm, shape)
        assert (g["s"], g["image"], g["total"], g["plan"]) == (s, image, total, plan), (shape, g)
        sub_len = win * np_ if seg == 1 else s
        assert g["pitch"] == sub_len + 16 and (g["pitch"] // 16) % 2 == 1 and g["n_sub"] == (1 if seg == 1 else np_)
        assert g["image"] == (16 * g["n_sub"] * g["pitch"] + 1023) // 1024 * 1024 and g["n_dma"] * 1024 == g["image"] and g["total"] <= LDS_CU


@pytest.mark.parametrize("shape", sorted(MAP_SHAPES))
def test_address_map_exhaustively(wm, shape):
    """Every alignment-class hop, every span misalignment the hop's alignment allows (the span starts on a sample of a stream whose hops keep the alignment: multiples
    of AL below 16), the first tile of a batch with its negative hops, a middle tile and the last one, every segment:
    (a) every byte a fragment read delivers for (row, piece, segment, k) is stream byte hop x hop_bytes + piece x WIN_BYTES + k of that row, for the hops inside
        [0, n_hops); (b) every transfer's source lies in [0, span_end - 16]; (c) every fragment read -- with the AL = 2 reader's five dwords -- lies inside its image;
    (d) the 16 rows of one k-chunk fall on 16 different 16-byte bank columns; and the reads are aligned to AL."""
    win, np_, seg, hops = MAP_SHAPES[shape]
    g = _geometry(wm, shape)
    image, s, n16 = g["image"], g["s"], g["s"] // 16
    n_hops, shift = 40, 5
    tiles = (shift + n_hops + 15) // 16
    assert tiles == 3
    src = (C.c_long * (g["n_dma"] * 64))()
    frag = (C.c_int * (16 * np_ * n16))()
    byte16 = np.arange(16)
    checked = 0
    for sg in range(seg):
        assert wm.wm_frags(shape, np_, sg, frag) == 0
        f = np.frombuffer(frag, dtype=np.int32).reshape(16, np_, n16).copy()
        # (d) 16 rows of a k-chunk of a piece -> 16 different bank columns (256 bytes = 16 columns of 16 bytes)
        cols = np.sort((f // 16) % 16, axis=0)
        assert (f % 16 == 0).all() and (cols == np.arange(16)[:, None, None]).all()
        k = sg * s + 16 * np.arange(n16)
        for hop_bytes in hops:
            al = 16 if hop_bytes % 16 == 0 else 8 if hop_bytes % 8 == 0 else 4 if hop_bytes % 4 == 0 else 2
            for mis in range(0, 16, al):
                span_end = wm.wm_span_end(n_hops, hop_bytes, win * np_, mis)
                assert span_end % 16 == 0 and span_end - 16 < mis + (n_hops - 1) * hop_bytes + win * np_ <= span_end
                for t in range(tiles):
                    hop0 = t * 16 - shift
                    assert wm.wm_sources(shape, hop0, hop_bytes, mis, sg, span_end, src) == 0
                    so = np.frombuffer(src, dtype=np.int64)
                    assert so.min() >= 0 and so.max() <= span_end - 16 and (so % 16 == 0).all()                     # (b)
                    pos = (so[:, None] + byte16[None, :]).reshape(-1)                                               # image byte -> offset from the aligned origin
                    assert len(pos) == image
                    for row in range(16):
                        hop = hop0 + row
                        delta = wm.wm_delta(hop, hop_bytes, mis)
                        assert delta % al == 0 and delta == (hop * hop_bytes + mis) % 16
                        first = f[row] + delta                                                                      # [piece][k-chunk]
                        last = (first - first % 4 + 20) if al == 2 else first + 16                                 # AL = 2: five aligned dwords from the one at or in front
                        assert first.min() >= 0 and last.max() <= 16 * g["n_sub"] * g["pitch"] <= image              # (c)
                        if not 0 <= hop < n_hops:
                            continue
                        got = pos[(first[:, :, None] + byte16[None, None, :])]
                        want = mis + hop * hop_bytes + (np.arange(np_) * win)[:, None, None] + k[None, :, None] + byte16[None, None, :]
                        assert np.array_equal(got, want), (hop_bytes, mis, t, row, sg)                              # (a)
                        checked += got.size
    assert checked == sum(16 // (16 if h % 16 == 0 else 8 if h % 8 == 0 else 4 if h % 4 == 0 else 2) for h in hops) * n_hops * np_ * win


# ---- the oracle pinned to the reference, and the golden ----

need_ref = tw.need_ref


@need_ref
@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", GPU_CASES + [ODD_HOP_CASE])
def test_oracle_is_the_reference_at_wide_windows(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """tests/test_wide_hops.py::test_oracle_is_the_reference_at_wide_hops at the configurations of the GPU file: bit for bit, and channels open."""
    tw.test_oracle_is_the_reference_at_wide_hops(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate)


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", GPU_CASES + [ODD_HOP_CASE])
def test_streams_open_channels_at_these_shapes(pkg, built, sfmt_name, fft_log, sample_rate, wave_rate):
    """helpers.format_case makes streams whose channels open at these shapes (the oracle alone: needs no reference build), over the GPU file's seven batches."""
    devices, iq = helpers.format_case(pkg, getattr(pkg.capi, sfmt_name), fft_log, sample_rate, wave_rate, 1, 7)
    got = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log).run_device(0, iq[0], 7)
    assert got["n_batches"] == 7 and (got["axc"] == ord("*")).any() and (got["axc"] == ord(" ")).any()


def load_golden():
    z = np.load(os.path.join(GOLDEN, make_golden_wide2048.NAME + ".npz"))
    c, devices, iq = make_golden_wide2048.build_case()
    assert hashlib.sha256(iq.tobytes()).digest() == z["iq_sha256"].tobytes(), "synthetic I/Q generator no longer reproduces the fixture's input"
    assert json.loads(str(z["channels"])) == devices[0]["channels"]
    return z, c, devices, iq


def test_golden_is_small_and_shows_an_open_and_a_close():
    name = make_golden_wide2048.NAME + ".npz"
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != name)
    assert os.path.getsize(os.path.join(GOLDEN, name)) <= largest
    c = json.loads(str(np.load(os.path.join(GOLDEN, name))["case"]))
    assert (c["sfmt"], c["fft_log"], c["sample_rate"]) == ("SFMT_S16", 11, 10_000_000)
    axc = np.load(os.path.join(GOLDEN, name))["axc"]
    assert axc.shape[1] == 8                                        # one dongle
    opened, closed = axc == ord("*"), axc == ord(" ")
    assert (closed[:-1] & opened[1:]).any() and (opened[:-1] & closed[1:]).any()   # some channel opens, some channel closes, from one batch to the next


def test_oracle_reproduces_the_golden(built):
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
