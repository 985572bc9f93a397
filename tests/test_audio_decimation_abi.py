"""The output decimation's public interface without a GPU: the three entry points in the built library with their prototypes, the build flags of the kernel,
and the refusal of a NULL handle before any device is touched."""
import ctypes as C

import numpy as np

NAMES = ("airband_hip_set_output_decimation", "airband_hip_encoded_row_samples", "airband_hip_decimate_audio")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.AUDIO_DECIMATION_PROTOTYPES[name]
    assert set(pkg.capi.AUDIO_DECIMATION_PROTOTYPES) == set(NAMES)
    assert pkg.capi.ABI_VERSION == 2  # additions only


def test_kernel_is_built_like_the_encoder(pkg):
    flags = pkg._build.HIP_SOURCES["audio_decimate.hip"]
    assert flags == pkg._build.HIP_SOURCES["audio_pack.hip"] and "-ffp-contract=off" in flags  # the two share audio_sample.h's float step


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    rows = np.zeros((1, 1000), np.float32)
    hist = np.full((1, 46), 7, "<i2")
    for factor in (1, 2, 3):
        assert L.airband_hip_set_output_decimation(None, factor) == capi.EINVAL
    assert L.airband_hip_encoded_row_samples(None) == capi.EINVAL
    assert L.airband_hip_decimate_audio(None, capi.AUDIO_S16, rows.ctypes.data, 1, hist.ctypes.data, None, None) == capi.EINVAL
    assert (hist == 7).all()
    assert C.sizeof(capi.AudioRow) == 16  # the record's layout is unchanged
