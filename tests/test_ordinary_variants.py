"""Every variant of the ordinary matrix-core channelizers (csrc/channelizer_dft.hip, csrc/channelizer_f32.hip: what an unflagged handle and bench.py run) without a
GPU: the table of sweep cases tests/test_gpu_ordinary_variants.py runs -- one configuration per kernel variant an unflagged handle can select, found by scanning the
library's own selection rules (tests/host_ordinary_select.cpp) and not by reading kernel source --, that the table is complete and sits on the edges of the selection,
and the coefficient tables at every case, on the two plans of helpers.wide_case() (which does not depend on the hop being wide).

A VARIANT is what the launch code instantiates a kernel for:
  int8 family   ("8bit" | "cs16", fft size, AL = the largest of 16 / 8 / 4 / 2 that divides the hop's bytes, hop-specialised 0 / 320 / 640, edge_hi_zero)
  CF32 family   ("cf32", fft size, layout 0 ... 3 of the staged image, "small" | "large" tile)
The fft size stands for the window pieces / segments: fft 1024 / 2048 / 4096 are NP = 2 / 4 / 8 wavefronts of the fft 512 int8 kernel and 8192 two passes of eight
(DftArgs::partial); CF32 fft 4096 / 8192 are 2 / 4 segment launches of the fft 2048 kernel (F32Args::partial).

Two elements of the int8 key have no callable rule and are RESTATED here, each with the line it restates; the GPU file confirms what a handle reports:
  hop-specialised   csrc/channelizer_dft.hip launch_one_piece(): u8 / s8 at fft 512, a hop of 320 or 640 bytes whose nbuf / sub / lds_per_buf -- dft_args() derives them
                    from (hop, window bytes, pieces) -- equal c_nbuf(hop) / c_sub(hop) / c_lds_per_buf(hop), which are the same functions at their default arguments
                    (1 024 window bytes, one piece).  The handle does not report which of the two launches it took.
  edge_hi_zero      csrc/params.cpp build_dft_tables(): `p.b_edge_hi_zero = NP == 1`, then cleared where a table's top digit is not zero in the outer k-steps.  With
                    the project's window it is never cleared, so the value is fft size <= 512; airband_hip_read_tables() reports it and the GPU sweep asserts it."""
import atexit
import ctypes as C
import importlib
import os
import shutil
import subprocess
import tempfile

import pytest

import helpers

HERE = os.path.dirname(os.path.abspath(__file__))
FFT_SIZES = (256, 512, 1024, 2048, 4096, 8192)
INT8_HOP_BYTES = {"8bit": (64, 1024, 2), "cs16": (128, 1280, 4)}   # the scan range: (first, last, step) in bytes
F32_FIRST_HOP = 8

# (sample format, fft_log, hop in samples, WAVE_RATE); the sample rate is hop x WAVE_RATE.  Unless noted the hop is the SMALLEST of its variant in the scan range.
# u8 and s8 are one variant (a runtime XOR mask): they alternate.  8-bit AL = 16 / 8 / 4 / 2 start at 64 / 72 / 68 / 66 bytes = 32 / 36 / 34 / 33 samples; CS16
# AL = 16 / 8 / 4 at 128 / 136 / 132 bytes = 32 / 34 / 33 samples.
_SWEEP_HOPS = [
    ("SFMT_U8", 8, 32, 8000), ("SFMT_S8", 8, 36, 8000), ("SFMT_U8", 8, 34, 16000), ("SFMT_S8", 8, 33, 16000),
    ("SFMT_U8", 9, 32, 8000), ("SFMT_S8", 9, 36, 8000), ("SFMT_U8", 9, 34, 16000), ("SFMT_S8", 9, 33, 16000), ("SFMT_U8", 9, 160, 8000), ("SFMT_S8", 9, 320, 8000),   # (320 / 640 bytes: the hop-specialised kernels)
    ("SFMT_U8", 10, 32, 16000), ("SFMT_S8", 10, 36, 16000), ("SFMT_U8", 10, 34, 8000), ("SFMT_S8", 10, 33, 8000), ("SFMT_S8", 10, 512, 8000),   # (512 samples = 1 024 bytes: the largest hop, AL = 16)
    ("SFMT_U8", 11, 32, 16000), ("SFMT_S8", 11, 36, 16000), ("SFMT_U8", 11, 34, 8000), ("SFMT_S8", 11, 33, 8000),
    ("SFMT_U8", 12, 32, 16000), ("SFMT_S8", 12, 36, 16000), ("SFMT_U8", 12, 34, 8000), ("SFMT_S8", 12, 33, 8000),
    ("SFMT_U8", 13, 32, 16000), ("SFMT_S8", 13, 36, 16000), ("SFMT_U8", 13, 34, 8000), ("SFMT_S8", 13, 33, 8000),
    ("SFMT_S16", 8, 32, 8000), ("SFMT_S16", 8, 34, 16000), ("SFMT_S16", 8, 33, 8000),
    ("SFMT_S16", 9, 32, 16000), ("SFMT_S16", 9, 34, 8000), ("SFMT_S16", 9, 33, 16000),
    ("SFMT_S16", 10, 32, 8000), ("SFMT_S16", 10, 34, 16000), ("SFMT_S16", 10, 33, 8000),
    ("SFMT_S16", 11, 32, 16000), ("SFMT_S16", 11, 34, 8000), ("SFMT_S16", 11, 33, 16000), ("SFMT_S16", 11, 320, 8000),   # (320 samples = 1 280 bytes: the largest hop, AL = 16)
    ("SFMT_S16", 12, 32, 8000), ("SFMT_S16", 12, 34, 16000), ("SFMT_S16", 12, 33, 8000),
    ("SFMT_S16", 13, 32, 16000), ("SFMT_S16", 13, 34, 8000), ("SFMT_S16", 13, 33, 16000),
    ("SFMT_F32", 8, 8, 8000), ("SFMT_F32", 8, 9, 16000), ("SFMT_F32", 8, 32, 8000), ("SFMT_F32", 8, 10, 16000),   # (small tiles, layouts 0, 1, 2, 3)
    ("SFMT_F32", 8, 188, 8000), ("SFMT_F32", 8, 189, 16000), ("SFMT_F32", 8, 192, 8000), ("SFMT_F32", 8, 190, 16000), ("SFMT_F32", 8, 392, 8000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
    ("SFMT_F32", 9, 8, 8000), ("SFMT_F32", 9, 9, 16000), ("SFMT_F32", 9, 10, 8000),   # (small tiles, layouts 0, 1, 3)
    ("SFMT_F32", 9, 172, 16000), ("SFMT_F32", 9, 171, 8000), ("SFMT_F32", 9, 192, 16000), ("SFMT_F32", 9, 174, 8000), ("SFMT_F32", 9, 375, 16000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
    ("SFMT_F32", 10, 8, 16000), ("SFMT_F32", 10, 9, 8000), ("SFMT_F32", 10, 32, 16000), ("SFMT_F32", 10, 10, 8000),   # (small tiles, layouts 0, 1, 2, 3)
    ("SFMT_F32", 10, 344, 16000), ("SFMT_F32", 10, 343, 8000), ("SFMT_F32", 10, 352, 16000), ("SFMT_F32", 10, 342, 8000), ("SFMT_F32", 10, 527, 8000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
    ("SFMT_F32", 11, 8, 16000), ("SFMT_F32", 11, 9, 8000), ("SFMT_F32", 11, 32, 16000), ("SFMT_F32", 11, 10, 8000),   # (small tiles, layouts 0, 1, 2, 3)
    ("SFMT_F32", 11, 276, 16000), ("SFMT_F32", 11, 273, 8000), ("SFMT_F32", 11, 288, 16000), ("SFMT_F32", 11, 274, 8000), ("SFMT_F32", 11, 459, 16000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
    ("SFMT_F32", 12, 8, 16000), ("SFMT_F32", 12, 9, 8000), ("SFMT_F32", 12, 32, 16000), ("SFMT_F32", 12, 10, 8000),   # (small tiles, layouts 0, 1, 2, 3)
    ("SFMT_F32", 12, 276, 16000), ("SFMT_F32", 12, 273, 8000), ("SFMT_F32", 12, 288, 16000), ("SFMT_F32", 12, 274, 8000), ("SFMT_F32", 12, 459, 8000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
    ("SFMT_F32", 13, 8, 16000), ("SFMT_F32", 13, 9, 8000), ("SFMT_F32", 13, 32, 16000), ("SFMT_F32", 13, 10, 8000),   # (small tiles, layouts 0, 1, 2, 3)
    ("SFMT_F32", 13, 276, 16000), ("SFMT_F32", 13, 273, 8000), ("SFMT_F32", 13, 288, 16000), ("SFMT_F32", 13, 274, 8000), ("SFMT_F32", 13, 459, 16000),   # (large tiles, layouts 0 - 3; the last hop f32_supported() accepts)
]
SWEEP_CASES = [(f, n, h * w, w) for f, n, h, w in _SWEEP_HOPS]
SWEEP_IDS = ["%s-fft%d-hop%d-w%d" % (f[5:].lower(), 1 << n, h, w) for f, n, h, w in _SWEEP_HOPS]
# the process_device cases of the GPU file (only fft-512 u8 had run zero-copy against anything): 8-bit AL = 2 at fft 256 and at fft 2048, CS16 AL = 4 at fft 4096,
# CF32 layout 1 (an odd hop) at fft 512 and at fft 8192
ZERO_COPY_CASES = [("SFMT_S8", 8, 33 * 16000, 16000), ("SFMT_S8", 11, 33 * 8000, 8000), ("SFMT_S16", 12, 33 * 8000, 8000), ("SFMT_F32", 9, 9 * 16000, 16000), ("SFMT_F32", 13, 9 * 8000, 8000)]
assert all(c in SWEEP_CASES for c in ZERO_COPY_CASES)


def _pkg():
    return importlib.import_module("rtlsdr-airband_amd")


_sel_cache = {}


def selection_library():
    """tests/host_ordinary_select.cpp built with g++ against the built libairband_hip.so: dft_supported, f32_supported, f32_layout, f32_small_tile and
    dft_nbuf / dft_sub / dft_lds_per_buf as the library has them."""
    if "lib" not in _sel_cache:
        pkg = _pkg()
        product = pkg._build.build()
        rocm = os.path.dirname(os.path.dirname(os.path.abspath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))))
        d = tempfile.mkdtemp(prefix="ordsel_")
        atexit.register(shutil.rmtree, d, True)
        out = os.path.join(d, "libordsel.so")
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-I" + pkg._build.CSRC, "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                        "-o", out, os.path.join(HERE, "host_ordinary_select.cpp"), os.path.abspath(product)], check=True)
        lib = C.CDLL(out)
        for name in ("dft_supported", "dft_nbuf", "dft_sub", "dft_lds_per_buf", "f32_supported", "f32_layout", "f32_small_tile", "f32_n_seg"):
            getattr(lib, "ordsel_" + name).restype = C.c_int
        _sel_cache["lib"] = lib
    return _sel_cache["lib"]


def hop_alignment(hop_bytes):
    return next(a for a in (16, 8, 4, 2, 1) if hop_bytes % a == 0)


def hop_specialised(fft, hop_bytes, bytes_per_sample):
    """RESTATES csrc/channelizer_dft.hip launch_one_piece(), `if (a.hop_bytes == 320 && a.nbuf == c_nbuf(320) && ...` and the same for 640, which u8 / s8 reach at
    fft 512 only (CS16 and fft 256 return above it, larger windows never call it); the geometry on the left is dft_args()'s (csrc/airband_hip.cpp): whole-window
    bytes of up to eight pieces."""
    L = selection_library()
    if fft != 512 or bytes_per_sample != 1 or hop_bytes not in (320, 640):
        return 0
    np_total = fft // 512 if fft > 512 else 1
    np_ = min(np_total, 8)
    win_bytes = 2 * fft * bytes_per_sample // np_total * np_
    same = all(f(hop_bytes, win_bytes, np_) == f(hop_bytes, 1024, 1) for f in (L.ordsel_dft_nbuf, L.ordsel_dft_sub, L.ordsel_dft_lds_per_buf))
    return hop_bytes if same else 0


def edge_hi_zero(fft):
    """RESTATES csrc/params.cpp build_dft_tables(), `p.b_edge_hi_zero = NP == 1;` with NP = the window's pieces of 512 samples (see the module's docstring)."""
    return fft <= 512


def variant_key(sfmt, fft, hop_samples):
    """The kernel variant an unflagged handle runs at this shape, or None where neither ordinary matrix-core channelizer takes it.  sfmt: a capi.SFMT_* name."""
    capi, L = _pkg().capi, selection_library()
    code = getattr(capi, sfmt)
    if code == capi.SFMT_F32:
        if not L.ordsel_f32_supported(fft, hop_samples, code):
            return None
        return ("cf32", fft, L.ordsel_f32_layout(fft, 8 * hop_samples), "small" if L.ordsel_f32_small_tile(fft, 8 * hop_samples) else "large")
    bps = capi.BYTES_PER_SAMPLE[code]
    hop_bytes = 2 * hop_samples * bps
    if not L.ordsel_dft_supported(fft, hop_bytes, code, 8):
        return None
    return ("cs16" if code == capi.SFMT_S16 else "8bit", fft, hop_alignment(hop_bytes), hop_specialised(fft, hop_bytes, bps), edge_hi_zero(fft))   # (AL: launch_generic())


def case_key(case):
    sfmt, fft_log, sample_rate, wave_rate = case
    assert sample_rate % wave_rate == 0
    return variant_key(sfmt, 1 << fft_log, sample_rate // wave_rate)


_last_hop_cache = {}


def f32_last_hop(fft):
    """The last hop f32_supported() accepts at this fft size (beyond it the layouts' LDS needs differ, so a few hops in front of it are refused too)."""
    if fft not in _last_hop_cache:
        L, code = selection_library(), _pkg().capi.SFMT_F32
        _last_hop_cache[fft] = max(h for h in range(F32_FIRST_HOP, 4096) if L.ordsel_f32_supported(fft, h, code))
    return _last_hop_cache[fft]


_scan_cache = {}


def scan_variants():
    """{variant key: the smallest hop (in samples) that selects it} over the unflagged range: fft 256 ... 8192; u8 / s8 every even hop length from 64 to 1 024
    bytes and CS16 every multiple of 4 from 128 to 1 280 bytes, both at hops shorter than the window; CF32 every hop from 8 samples to the last one f32_supported()
    accepts at that fft size.  u8 and s8 are scanned both and must agree."""
    if not _scan_cache:
        for fft in FFT_SIZES:
            for fam, fmts, bps in (("8bit", ("SFMT_U8", "SFMT_S8"), 1), ("cs16", ("SFMT_S16",), 2)):
                first, last, step = INT8_HOP_BYTES[fam]
                for hop_bytes in range(first, last + 1, step):
                    hop = hop_bytes // (2 * bps)
                    if hop >= fft:
                        break
                    keys = {variant_key(f, fft, hop) for f in fmts}
                    assert len(keys) == 1 and None not in keys, (fft, hop, keys)   # the whole range is the int8 kernel's
                    _scan_cache.setdefault(keys.pop(), hop)
            for hop in range(F32_FIRST_HOP, f32_last_hop(fft) + 1):
                a = variant_key("SFMT_F32", fft, hop)
                if a is not None:
                    _scan_cache.setdefault(a, hop)
    return _scan_cache


LARGEST_INT8 = {"8bit": 1024, "cs16": 1280}   # bytes


def is_largest_hop(key, hop_samples, capi):
    if key[0] == "cf32":
        return hop_samples == f32_last_hop(key[1])
    return 2 * hop_samples * (2 if key[0] == "cs16" else 1) == LARGEST_INT8[key[0]]


def variant_cases():
    """The sweep without its largest-hop extras: [(case, key)] of the cases that sit on the smallest hop of their variant."""
    found = scan_variants()
    return [(c, case_key(c)) for c in SWEEP_CASES if found.get(case_key(c)) == c[2] // c[3]]


def test_sweep_covers_every_variant_once(built):
    """The table's keys are exactly the keys of the scan, one case each (the largest-hop extras aside), and the structure the dispatch code implies."""
    found = scan_variants()
    keys = [k for _, k in variant_cases()]
    assert None not in keys
    assert len(set(keys)) == len(keys), "two sweep cases on one variant: %s" % sorted(k for k in set(keys) if keys.count(k) > 1)
    missing, unknown = sorted(set(found) - set(keys), key=str), sorted(set(keys) - set(found), key=str)
    assert not missing and not unknown, "variants without a sweep case: %s; sweep cases on no variant of the scan: %s" % (missing, unknown)
    per_family = {fam: sorted(k for k in found if k[0] == fam) for fam in ("8bit", "cs16", "cf32")}
    print("variants per family:", {fam: len(v) for fam, v in per_family.items()}, "sweep cases:", len(SWEEP_CASES))
    # int8, as launch_channelizer_dft() / launch_generic() say: every fft size with every AL -- 16 / 8 / 4 / 2 for the 8-bit formats, 16 / 8 / 4 for CS16 (a CS16 hop
    # is whole samples of 4 bytes: no AL = 2) --, counted separately, plus the two hop-specialised kernels of u8 / s8 at fft 512
    generic8 = [k for k in per_family["8bit"] if k[3] == 0]
    assert sorted(k[1:3] for k in generic8) == sorted((f, al) for f in FFT_SIZES for al in (16, 8, 4, 2)) and len(generic8) == 24
    assert sorted(k[1:3] for k in per_family["cs16"]) == sorted((f, al) for f in FFT_SIZES for al in (16, 8, 4)) and len(per_family["cs16"]) == 18
    assert sorted(k for k in per_family["8bit"] if k[3]) == [("8bit", 512, 16, 320, True), ("8bit", 512, 16, 640, True)]
    assert not any(k[3] for k in per_family["cs16"])
    # UNREACHABLE template combinations of channelizer_dft_kernel<FFT_N, EDGE_HI_ZERO, ...> (the library builds both EDGE_HI_ZERO values of every instantiation):
    #   EDGE_HI_ZERO = false at NP = 1 (fft 256, 512): build_dft_tables() clears the flag only where a table's top digit is not zero in the outer k-steps, and the
    #     7-term cosine window is below 2^-8 there at every bin: no plan of the suite's (the project's one) window gives it;
    #   EDGE_HI_ZERO = true at NP > 1 (fft 1024 ... 8192): `p.b_edge_hi_zero = NP == 1` -- a window piece has its small coefficients at one end only.
    assert all(k[4] == (k[1] <= 512) for k in per_family["8bit"] + per_family["cs16"])
    # CF32, as launch_channelizer_f32() / f32_layout() say: which (fft, layout, tile) exist.  Every one of 6 x 4 x 2 but
    #   UNREACHABLE (512, layout 2, small): f32_layout() keeps fft 512's small tiles on layout 0 (layout 2's LDS would cost the third workgroup per CU), so
    #     channelizer_f32_kernel<512, 6, 4, 2> is built and never launched.
    # (fft 4096 / 8192 are the fft 2048 kernels once per segment: their triples are fft 2048's, at the same hops.)
    assert sorted(k[1:] for k in per_family["cf32"]) == sorted((f, lay, t) for f in FFT_SIZES for lay in (0, 1, 2, 3) for t in ("small", "large") if (f, lay, t) != (512, 2, "small"))
    assert len(per_family["cf32"]) == 47
    for t in ("small", "large"):
        for lay in (0, 1, 2, 3):
            assert found[("cf32", 2048, lay, t)] == found[("cf32", 4096, lay, t)] == found[("cf32", 8192, lay, t)]
    L = selection_library()
    assert [L.ordsel_f32_n_seg(f) for f in FFT_SIZES] == [1, 1, 1, 1, 2, 4]
    assert [case_key(c) for c in ZERO_COPY_CASES] == [("8bit", 256, 2, 0, True), ("8bit", 2048, 2, 0, False), ("cs16", 4096, 4, 0, False), ("cf32", 512, 1, "small"), ("cf32", 8192, 1, "small")]


def test_sweep_hops_are_on_the_edges(pkg, built):
    """Every case sits on the smallest hop of its variant -- the edge of the selection -- except the largest hops of the range: one per int family (8-bit 1 024
    bytes, CS16 1 280 bytes) and, per fft size, the last hop f32_supported() accepts."""
    capi = pkg.capi
    found = scan_variants()
    large = {"8bit": [], "cs16": [], "cf32": []}
    for case in SWEEP_CASES:
        hop = case[2] // case[3]
        key = case_key(case)
        if hop == found[key]:
            continue
        assert is_largest_hop(key, hop, capi), (case, key, found[key])
        large[key[0]].append(key[1])
    assert len(large["8bit"]) >= 1 and len(large["cs16"]) >= 1 and sorted(large["cf32"]) == list(FFT_SIZES), large
    # the edges themselves, as the dispatch code states them
    for fft in FFT_SIZES:
        assert [2 * found[("8bit", fft, al, 0, fft <= 512)] for al in (16, 2, 4, 8)] == [64, 66, 68, 72]
        assert [4 * found[("cs16", fft, al, 0, fft <= 512)] for al in (16, 4, 8)] == [128, 132, 136]
        assert [found[("cf32", fft, lay, "small")] for lay in (0, 1, 3)] == [8, 9, 10]
        assert fft == 512 or found[("cf32", fft, 2, "small")] == 32                       # the first multiple of 256 bytes
        assert found[("cf32", fft, 2, "large")] % 32 == 0
    assert [f32_last_hop(f) for f in FFT_SIZES] == [392, 375, 527, 459, 459, 459]
    # the small-tile rule at its edge: the last small hop and the first large one are neighbours, whatever the layout
    L = selection_library()
    for fft in FFT_SIZES:
        first_large = min(h for k, h in found.items() if k[0] == "cf32" and k[1] == fft and k[3] == "large")
        assert all(L.ordsel_f32_small_tile(fft, 8 * h) for h in range(8, first_large)) and not any(L.ordsel_f32_small_tile(fft, 8 * h) for h in range(first_large, f32_last_hop(fft) + 1))


def test_ordinary_case_plan(pkg, built):
    """helpers.wide_case()'s plans at every sweep shape: 8 and 11 channels; dongle 1 has another plan -- a short last group of three, bins in the upper half, one AM
    channel with raw-I/Q outputs (its squelch held shut) -- and, CS16, another full scale."""
    capi = pkg.capi
    for sfmt_name, fft_log, sample_rate, wave_rate in SWEEP_CASES:
        sfmt, n_fft = getattr(capi, sfmt_name), 1 << fft_log
        devices = helpers.wide_devices(capi, sfmt, sample_rate, wave_rate, 2)
        assert len(devices[0]["channels"]) == 8 and len(devices[1]["channels"]) == 11 and 11 % 8 == 3
        assert [c["frequency"] for c in devices[0]["channels"]] != [c["frequency"] for c in devices[1]["channels"]][:8]
        bins = [int(pkg.derive_constants(devices[1:], k, wave_rate=wave_rate, fft_log=fft_log)[0]) for k in range(3)]   # (the first three lie below the centre frequency)
        assert all(n_fft // 2 <= b < n_fft for b in bins) and len(set(bins)) == 3, bins
        chans = devices[1]["channels"]
        assert [c["has_iq_outputs"] for c in chans] == [1 if k == helpers.WIDE_PLAN_B_IQ_CHANNEL else 0 for k in range(11)]
        assert chans[helpers.WIDE_PLAN_B_IQ_CHANNEL]["modulation"] == 0 and chans[helpers.WIDE_PLAN_B_IQ_CHANNEL]["squelch_threshold_dbfs"] == helpers.WIDE_SHUT_DBFS
        if sfmt == capi.SFMT_S16:
            assert devices[0]["fullscale"] != devices[1]["fullscale"] and min(devices[0]["fullscale"], devices[1]["fullscale"]) > 0


@pytest.mark.parametrize("case", SWEEP_CASES, ids=SWEEP_IDS)
def test_tables_selftest_at_every_variant(pkg, built, case):
    """The coefficient tables of both plans of a sweep case, in the order the case's kernel contracts them, under tests/test_dft_tables.py's bar for
    airband_hip_dft_selftest: the worst value within 2e-6 of the RMS (24-bit coefficients; CF32: float sums of up to 4 096 products per segment)."""
    sfmt_name, fft_log, sample_rate, wave_rate = case
    devices = helpers.wide_devices(pkg.capi, getattr(pkg.capi, sfmt_name), sample_rate, wave_rate, 2)
    err = pkg.dft_selftest(devices, wave_rate=wave_rate, fft_log=fft_log, windows=2)
    print("table error", case, err)
    assert err < 2e-6
