"""The band survey's public interface without a GPU: the three entry points in the built library and in the header, the two structs, the validation in front of
the device, and the definition in numpy (capi.band_survey_reference) on rows whose answers are written out by hand."""
import ctypes as C
import os

import numpy as np
import pytest

import survey_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_band_survey", "airband_hip_collect_band_survey", "airband_hip_device_band_survey")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.BAND_SURVEY_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # no existing struct changed


def test_struct_sizes(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.BandPeak) == 8 and C.sizeof(capi.BandSummary) == 32
    assert np.dtype(capi.PEAK_DTYPE).itemsize == 8 and np.dtype(capi.SUMMARY_DTYPE).itemsize == 32
    for struct, dtype in ((capi.BandPeak, capi.PEAK_DTYPE), (capi.BandSummary, capi.SUMMARY_DTYPE)):
        dt = np.dtype(dtype)
        assert [(f[0], getattr(struct, f[0]).offset) for f in struct._fields_] == [(n, dt.fields[n][1]) for n in dt.names]


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert "#define AIRBAND_HIP_ABI_VERSION 2" in text
    for decl in ("int airband_hip_set_band_survey(airband_hip_handle* h, uint32_t trace, int32_t max_peaks, int32_t floor_permille, float threshold_ratio, int32_t guard_bins);",
                 "int airband_hip_collect_band_survey(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_band_summary* summary, airband_hip_band_peak* peaks);",
                 "int airband_hip_device_band_survey(airband_hip_handle* h, airband_hip_band_summary** d_summary, airband_hip_band_peak** d_peaks);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("} airband_hip_band_peak; /* 8 bytes */", "} airband_hip_band_summary; /* 32 bytes */", "BY ITS BIT PATTERN", "PREPARE-TIME bin",
                   "does not follow it", "(N * floor_permille) / 1000", "AIRBAND_HIP_EAGAIN before any batch"):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    p = [C.c_void_p() for _ in range(2)]
    assert L.airband_hip_set_band_survey(None, capi.SCOPE_MEAN, 8, 500, 10.0, 8) == capi.EINVAL
    assert L.airband_hip_collect_band_survey(None, 0, 1, None, None) == capi.EINVAL
    assert L.airband_hip_device_band_survey(None, *[C.byref(x) for x in p]) == capi.EINVAL


CASES = survey_cases.hand_made()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_on_hand_made_rows(pkg, case):
    name, row, bins, kw, expect = case
    got = pkg.capi.band_survey_reference(row, bins, **kw)
    assert got["peaks"].dtype == np.dtype(pkg.capi.PEAK_DTYPE) and got["peaks"].shape == (kw["max_peaks"],)
    for key, want in expect.items():
        if key == "peaks":
            listed = got["peaks"]["bin"][got["peaks"]["bin"] >= 0].tolist()
            assert listed == want, (name, listed)
            m = len(want)
            assert np.array_equal(got["peaks"]["power"][:m], row[want]) and (got["peaks"]["bin"][m:] == -1).all() and (got["peaks"]["power"][m:] == 0).all()
            assert got["n_peaks"] >= m and (got["n_peaks"] == m or m == kw["max_peaks"])
        else:
            assert got[key] == want, (name, key, got[key])


def test_reference_orders_by_bit_pattern(pkg):
    """Negative floats and NaNs sort ABOVE every non-negative float (unsigned bit patterns): a total order, whatever the row holds."""
    row = np.full(survey_cases.N, 1.0, np.float32)
    row[10] = -2.0
    row[20] = np.nan
    got = pkg.capi.band_survey_reference(row, [], 4, 500, np.float32(10.0), -1)
    assert got["max_bin"] == (10 if row[10:11].view(np.uint32)[0] > row[20:21].view(np.uint32)[0] else 20)
    assert got["n_over"] == 2 and got["peaks"]["bin"][:2].tolist() == sorted([10, 20], key=lambda k: -int(row[k:k + 1].view(np.uint32)[0]))
