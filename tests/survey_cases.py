"""Rows for the band survey's tests (tests/test_band_survey_abi.py: the numpy definition against expectations written out by hand;
tests/test_host_band_survey.py: the kernel source on the CPU against the numpy definition) and the bit-for-bit comparison both the CPU and the GPU tests use."""
import numpy as np

N = 256  # the smallest fft size: one bin per thread of the kernel's workgroup


def hand_made():
    """[(name, row, channel bins, dict(max_peaks, floor_permille, ratio, guard_bins), expectations)]: expectations are the fields of
    capi.band_survey_reference()'s result that the case is about ("peaks" = the list of reported bins)."""
    base = dict(max_peaks=4, floor_permille=500, ratio=np.float32(10.0), guard_bins=3)
    cases = []

    row = np.full(N, 1.0, np.float32)
    cases.append(("all_equal", row, [17], base, dict(floor=1.0, threshold=10.0, n_over=0, n_peaks=0, max_bin=0, max_power=1.0, peaks=[])))

    row = np.full(N, 1.0, np.float32)
    row[100:103] = 50.0
    cases.append(("plateau", row, [17], base, dict(n_over=3, n_peaks=1, max_bin=100, peaks=[102])))

    row = np.full(N, 1.0, np.float32)
    row[0] = 50.0
    cases.append(("peak_at_bin_0", row, [17], base, dict(n_over=1, n_peaks=1, max_bin=0, peaks=[0])))

    row = np.full(N, 1.0, np.float32)
    row[N - 1] = row[0] = 50.0  # a plateau through the wrap: once, at its last bin
    cases.append(("plateau_through_the_wrap", row, [17], base, dict(n_over=2, n_peaks=1, max_bin=0, peaks=[0])))

    row = np.full(N, 1.0, np.float32)
    row[N - 2] = 50.0  # 3 from b = 1 through the wrap: covered
    row[N - 4] = 60.0  # 5 from it: not
    cases.append(("covered_through_the_wrap", row, [1], base, dict(n_over=2, n_peaks=1, max_bin=N - 4, peaks=[N - 4])))

    row = np.full(N, 1.0, np.float32)
    row[200] = row[40] = 30.0
    row[120] = 20.0
    cases.append(("equal_powers_by_bin", row, [17], base, dict(n_peaks=3, max_bin=40, peaks=[40, 200, 120])))

    row = np.full(N, 1.0, np.float32)
    at = [30, 60, 90, 150, 180, 210]
    row[at] = [20.0, 70.0, 40.0, 60.0, 30.0, 50.0]
    cases.append(("more_peaks_than_max_peaks", row, [17], base, dict(n_over=6, n_peaks=6, max_bin=60, peaks=[60, 150, 210, 90])))

    ramp = ((np.arange(N) * 37) % N + 1).astype(np.float32)  # a permutation of 1 .. N
    for permille, want in ((0, 1.0), (500, float(N // 2 + 1)), (1000, float(N))):
        cases.append(("floor_permille_%d" % permille, ramp, [17], dict(base, floor_permille=permille, ratio=np.float32(1.0)),
                      dict(floor=want, threshold=want, n_over=N - int(want))))

    row = np.full(N, 1.0, np.float32)
    row[17] = 50.0
    cases.append(("on_a_channel", row, [17], base, dict(n_over=1, n_peaks=0, max_bin=17, peaks=[])))
    cases.append(("guard_bins_minus_1", row, [17], dict(base, guard_bins=-1), dict(n_over=1, n_peaks=1, max_bin=17, peaks=[17])))
    return cases


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differences(summary, peaks, want):
    """Fields of one dongle's collected survey (an element of SUMMARY_DTYPE, a [max_peaks] array of PEAK_DTYPE) that are not bit for bit
    capi.band_survey_reference()'s: [] when all agree."""
    bad = []
    for f in ("floor", "threshold", "max_power"):
        if bits(np.float32(summary[f]).reshape(1))[0] != bits(np.float32(want[f]).reshape(1))[0]:
            bad.append((f, summary[f], want[f]))
    for f in ("max_bin", "n_over", "n_peaks"):
        if int(summary[f]) != int(want[f]):
            bad.append((f, int(summary[f]), int(want[f])))
    if np.any(np.asarray(summary["reserved"]) != 0):
        bad.append(("reserved", summary["reserved"], 0))
    if not np.array_equal(peaks["bin"], want["peaks"]["bin"]) or not np.array_equal(bits(peaks["power"]), bits(want["peaks"]["power"])):
        bad.append(("peaks", peaks.tolist(), want["peaks"].tolist()))
    return bad
