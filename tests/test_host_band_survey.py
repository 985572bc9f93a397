"""The band survey's kernel (csrc/band_survey.hip) with its wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles and barriers are rendezvous points; the LDS integer add is a plain one) by tests/host_survey_harness.cpp, launched by the file's own launch_band_survey(), compared field by field and bit for bit with the definition in numpy
(capi.band_survey_reference).  It checks the LOGIC of the code the GPU runs -- the radix select, the flags pass, the repeated workgroup maximum, the index
masks (the shim aborts on a write past the launch's LDS) -- tests/test_gpu_band_survey.py is what a GPU says."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hostbed
import survey_cases

pkg = importlib.import_module("rtlsdr-airband_amd")
capi = pkg.capi


@pytest.fixture(scope="module")
def hostsurvey(tmp_path_factory):
    lib = C.CDLL(hostbed.build("host_survey_harness.cpp", tmp_path_factory.mktemp("hostsurvey") / "libhostsurvey.so", shared=True))
    vp, i = C.c_void_p, C.c_int
    lib.hostsurvey_run.argtypes = [vp, i, i, vp, vp, i, i, C.c_float, i, vp, vp]
    lib.hostsurvey_lds_bytes.restype = C.c_long
    return lib


def _run(lib, rows, bins_per_row, max_peaks, floor_permille, ratio, guard_bins):
    rows = np.ascontiguousarray(rows, np.float32)
    n_rows, n = rows.shape
    first = np.zeros(n_rows + 1, np.int32)
    first[1:] = np.cumsum([len(b) for b in bins_per_row])
    flat = np.array([b for bl in bins_per_row for b in bl] + [0], np.int32)
    # poisoned: every entry must be written
    summary = np.frombuffer(bytearray(b"\xEE" * (32 * n_rows)), capi.SUMMARY_DTYPE).copy()
    peaks = np.frombuffer(bytearray(b"\xEE" * (8 * n_rows * max_peaks)), capi.PEAK_DTYPE).copy().reshape(n_rows, max_peaks)
    rc = lib.hostsurvey_run(rows.ctypes.data, n_rows, int(np.log2(n)), first.ctypes.data, flat.ctypes.data, max_peaks, floor_permille, float(ratio), guard_bins,
                            summary.ctypes.data, peaks.ctypes.data)
    assert rc == 0
    return summary, peaks


def _check(lib, rows, bins_per_row, max_peaks, floor_permille, ratio, guard_bins, what):
    summary, peaks = _run(lib, rows, bins_per_row, max_peaks, floor_permille, ratio, guard_bins)
    for r in range(len(rows)):
        want = capi.band_survey_reference(rows[r], bins_per_row[r], max_peaks, floor_permille, ratio, guard_bins)
        bad = survey_cases.differences(summary[r], peaks[r], want)
        assert not bad, (what, r, bad)
        listed = peaks[r]["bin"]
        assert ((listed >= -1) & (listed < rows.shape[1])).all()
    return summary, peaks


CASES = survey_cases.hand_made()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_made_rows(hostsurvey, case):
    name, row, bins, kw, _ = case
    _check(hostsurvey, row[None, :], [bins], kw["max_peaks"], kw["floor_permille"], kw["ratio"], kw["guard_bins"], name)


def test_lds_budget(hostsurvey):
    assert hostsurvey.hostsurvey_lds_bytes(13) <= 64 * 1024  # no opt-in to large LDS needed at any size
    assert hostsurvey.hostsurvey_lds_bytes(8) >= 4 * 256 + 4 * 256


def _bins(rng, n, count):
    return sorted(int(b) for b in rng.choice(n, count, replace=False))


@pytest.mark.parametrize("fft_log", [8, 9, 10, 13])
def test_uniform_random_bits(hostsurvey, fft_log):
    """Any bit pattern: negative values, infinities, NaNs, denormals.  The result equals the reference, nothing is written outside the LDS the launch asked for
    (the shim's guard zone), every listed bin is a bin of the row."""
    n = 1 << fft_log
    rng = np.random.default_rng(900 + fft_log)
    rows = rng.integers(0, 1 << 32, (3, n), dtype=np.uint64).astype(np.uint32)
    rows[1, : n // 2] = rows[1, : n // 2] & 0x7FFFFFFF | 0x7F800000  # half the row infinities and NaNs
    rows[2, ::3] = 0xFFFFFFFF
    rows = rows.view(np.float32)
    bins = [_bins(rng, n, 8), [], _bins(rng, n, 64)]
    for max_peaks, permille, ratio, guard in ((4, 500, 10.0, 8), (64, 0, 1.0, 0), (1, 1000, 0.5, -1), (7, 333, 1e-30, n // 2)):
        _check(hostsurvey, rows, bins, max_peaks, permille, np.float32(ratio), guard, (fft_log, max_peaks, permille))


@pytest.mark.parametrize("fft_log", [8, 9, 10, 13])
def test_heavy_ties(hostsurvey, fft_log):
    """Values drawn from four distinct floats: plateaus everywhere, equal keys but for the bin, histogram entries that take a whole row."""
    n = 1 << fft_log
    rng = np.random.default_rng(700 + fft_log)
    values = np.array([0.0, 1.0, 10.5, 200.0], np.float32)
    rows = values[rng.integers(0, 4, (3, n))]
    rows[2] = values[rng.choice(4, n, p=[0.9, 0.07, 0.02, 0.01])]
    bins = [_bins(rng, n, 8), _bins(rng, n, 1), _bins(rng, n, 16)]
    for max_peaks, permille, ratio, guard in ((4, 500, 10.0, 8), (64, 250, 2.0, 1), (16, 100, 1.0, -1)):
        summary, _ = _check(hostsurvey, rows, bins, max_peaks, permille, np.float32(ratio), guard, (fft_log, max_peaks, permille))
    assert (summary["n_peaks"] > 16).any()  # (the last setting) more peaks than entries: the list is the strongest, lowest bins first


@pytest.mark.parametrize("fft_log", [8, 9, 10, 13])
def test_noise_and_carriers(hostsurvey, fft_log):
    """What a scope row looks like: exponentially distributed noise powers and a few carriers, some of them on channels."""
    n = 1 << fft_log
    rng = np.random.default_rng(500 + fft_log)
    rows = rng.exponential(3.0e4, (2, n)).astype(np.float32)
    bins = [_bins(rng, n, 8), _bins(rng, n, 8)]
    for r in range(2):
        at = rng.choice(n, 9, replace=False)
        rows[r, at] *= 300.0
        rows[r, bins[r][0]] *= 1000.0
        rows[r, 1] *= 500.0
    summary, peaks = _check(hostsurvey, rows, bins, 4, 500, np.float32(10.0), 2, fft_log)
    assert (summary["n_peaks"] > 4).all() and (peaks["bin"] >= 0).all()
