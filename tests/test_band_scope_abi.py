"""The band scope's public interface without a GPU: the three entry points in the built library and in the header, their validation in front of the device,
and the window-selection rule restated in Python."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_band_scope", "airband_hip_collect_band_scope", "airband_hip_device_band_scope")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.BAND_SCOPE_PROTOTYPES[name]
    assert (pkg.capi.SCOPE_MEAN, pkg.capi.SCOPE_PEAK) == (1, 2)
    assert pkg.capi.ABI_VERSION == 2  # no struct changed


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert "#define AIRBAND_HIP_ABI_VERSION 2" in text
    assert re.search(r"#define AIRBAND_SCOPE_MEAN 0x1u", text) and re.search(r"#define AIRBAND_SCOPE_PEAK 0x2u", text)
    for decl in ("int airband_hip_set_band_scope(airband_hip_handle* h, const uint8_t* dev_mask, int32_t windows_per_batch, uint32_t traces);",
                 "int airband_hip_collect_band_scope(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, float* mean, float* peak);",
                 "int airband_hip_device_band_scope(airband_hip_handle* h, float** d_mean, float** d_peak, int32_t** d_row_of_dev);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("(j * WAVE_BATCH) / K", "AGC_EXTRA lead-in hops are never selected", "natural bin order", "AIRBAND_HIP_EAGAIN before any batch"):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    p = [C.c_void_p() for _ in range(3)]
    assert L.airband_hip_set_band_scope(None, None, 8, capi.SCOPE_MEAN) == capi.EINVAL
    assert L.airband_hip_collect_band_scope(None, 0, 1, None, None) == capi.EINVAL
    assert L.airband_hip_device_band_scope(None, *[C.byref(x) for x in p]) == capi.EINVAL


@pytest.mark.parametrize("wave_rate", [8000, 16000])
def test_window_selection_rule(pkg, wave_rate):
    B = wave_rate // 8  # WAVE_BATCH, src/rtl_airband.h:73
    for K in (1, 3, 7, 8, B):
        rows = pkg.capi.scope_window_hops(K, B)
        assert rows == [(j * B) // K for j in range(K)]
        assert len(rows) == K and rows[0] == 0  # row 0 is the first row read_bins() returns
        assert all(0 <= r < B for r in rows)
        assert all(a < b for a, b in zip(rows, rows[1:]))  # strictly ascending, so all distinct
        assert len(set(rows)) == K
    assert pkg.capi.scope_window_hops(B, B) == list(range(B))
