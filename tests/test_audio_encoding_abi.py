"""The encoded audio collect's public interface without a GPU: the four entry points in the built library and in the header, the constants and the 16-byte
record, and the definition in numpy (capi.audio_encode_reference / audio_decode_reference): against Python's audioop over every int16 value, the facts the header
states about the two laws, and the float step at full scale, beyond it, at the infinities, NaN, denormals, -0.0 and at exact ties."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_output_encoding", "airband_hip_collect_active_encoded", "airband_hip_device_active_encoded", "airband_hip_encode_audio")
LAWS = ("ulaw", "alaw")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.AUDIO_ENCODING_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # additions only


def test_constants_and_struct(pkg):
    capi = pkg.capi
    assert (capi.AUDIO_F32, capi.AUDIO_S16, capi.AUDIO_ULAW, capi.AUDIO_ALAW) == (0, 1, 2, 3)
    assert C.sizeof(capi.AudioRow) == 16
    want = dict(channel=0, peak=4, n_clipped=6, first=8, end=10, reserved=12)
    dt = np.dtype(capi.AUDIO_ROW_DTYPE)
    assert dt.itemsize == 16
    assert {f[0]: getattr(capi.AudioRow, f[0]).offset for f in capi.AudioRow._fields_} == want == {n: dt.fields[n][1] for n in dt.names}


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_set_output_encoding(airband_hip_handle* h, int32_t encoding);",
                 "int airband_hip_collect_active_encoded(airband_hip_handle* h, int64_t* n_active, int32_t* channel_index, void* audio, airband_hip_audio_row* info, char* axc_all);",
                 "int airband_hip_device_active_encoded(airband_hip_handle* h, void** d_audio, airband_hip_audio_row** d_info);",
                 "int airband_hip_encode_audio(airband_hip_handle* h, int32_t encoding, const float* rows, int64_t n_rows, void* audio, airband_hip_audio_row* info);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("#define AIRBAND_AUDIO_F32 0\n", "#define AIRBAND_AUDIO_S16 1\n", "#define AIRBAND_AUDIO_ULAW 2\n", "#define AIRBAND_AUDIO_ALAW 3\n",
                   "} airband_hip_audio_row; /* 16 bytes */", "v = x * 32767.0f", "ties to even", "m = min(|p|, 8159) + 33", "mask 0xD5", "multiple of four",
                   "#define AIRBAND_HIP_ABI_VERSION 2u"):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    n = C.c_int64(7)
    p = [C.c_void_p() for _ in range(2)]
    rows = np.zeros((1, 1000), np.float32)
    for enc in (capi.AUDIO_F32, capi.AUDIO_S16, 99):
        assert L.airband_hip_set_output_encoding(None, enc) == capi.EINVAL
    assert L.airband_hip_collect_active_encoded(None, C.byref(n), None, None, None, None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_device_active_encoded(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)
    assert L.airband_hip_encode_audio(None, capi.AUDIO_S16, rows.ctypes.data, 1, None, None) == capi.EINVAL


# ---- the two laws -------------------------------------------------------------------------------------------------------------------------------------
def test_laws_equal_audioop_over_every_int16(pkg):
    capi = pkg.capi
    try:
        import audioop
    except ImportError:
        pytest.skip("this Python has no audioop module")
    q = np.arange(-32768, 32768, dtype=np.int32)
    raw = q.astype("<i2").tobytes()
    assert capi.audio_law_reference(q, capi.AUDIO_ULAW).tobytes() == audioop.lin2ulaw(raw, 2)
    assert capi.audio_law_reference(q, capi.AUDIO_ALAW).tobytes() == audioop.lin2alaw(raw, 2)
    codes = np.arange(256, dtype=np.uint8)
    assert capi.audio_decode_reference(codes, "ulaw").astype("<i2").tobytes() == audioop.ulaw2lin(codes.tobytes(), 2)
    assert capi.audio_decode_reference(codes, "alaw").astype("<i2").tobytes() == audioop.alaw2lin(codes.tobytes(), 2)


def test_facts_the_header_states(pkg):
    capi = pkg.capi
    q = np.arange(-32767, 32768, dtype=np.int32)
    codes = np.arange(256, dtype=np.uint8)
    u, a = capi.audio_law_reference(q, capi.AUDIO_ULAW), capi.audio_law_reference(q, capi.AUDIO_ALAW)
    assert sorted(set(u.tolist())) == [c for c in range(256) if c != 0x7F]  # 255 distinct codes, never 0x7F
    assert sorted(set(a.tolist())) == list(range(256))
    again = capi.audio_law_reference(capi.audio_decode_reference(codes, "alaw"), capi.AUDIO_ALAW)
    assert np.array_equal(again, codes)
    again = capi.audio_law_reference(capi.audio_decode_reference(codes, "ulaw"), capi.AUDIO_ULAW)
    assert np.flatnonzero(again != codes).tolist() == [0x7F]
    for law, got in (("ulaw", u), ("alaw", a)):
        err = np.abs(capi.audio_decode_reference(got, law) - q)
        assert (err <= (np.abs(q) >> 5) + 8).all(), (law, int(err.max()))
    assert np.array_equal(capi.audio_decode_reference(q.astype("<i2"), "s16"), q)  # the identity


def test_every_q_comes_back_from_the_float_step(pkg):
    x, q = ac.every_q()
    got, clipped = pkg.capi.audio_quantize_reference(x)
    assert np.array_equal(got, q) and not clipped.any()


def test_float_step_at_the_specials(pkg):
    capi = pkg.capi
    f = np.float32
    x = np.array([1.0, -1.0, np.nextafter(f(1), f(2)), np.nextafter(f(-1), f(-2)), np.inf, -np.inf, np.nan, 1e-40, -1e-40, -0.0], np.float32)
    assert x[7] != 0 and abs(x[7]) < np.finfo(np.float32).tiny  # a denormal
    q, clipped = capi.audio_quantize_reference(x)
    assert q.tolist() == [32767, -32767, 32767, -32767, 32767, -32767, 0, 0, 0, 0]
    assert clipped.tolist() == [False, False, True, True, True, True, False, False, False, False]
    row = np.zeros((1, 12), np.float32)
    row[0, 1:11] = x
    for fmt in ac.FORMATS:
        audio, info = capi.audio_encode_reference(row, fmt)
        assert info.tolist() == [(0, 32767, 4, 1, 7, 0)], (fmt, info)
        assert audio.dtype == (np.dtype("<i2") if fmt == "s16" else np.uint8) and audio.shape == (1, 12)
    s16 = capi.audio_encode_reference(row, "s16")[0][0]
    assert s16.tolist() == [0] + q.tolist() + [0]
    audio, info = capi.audio_encode_reference(np.zeros((2, 8), np.float32), "ulaw")  # silence: first = B, end = 0
    assert info.tolist() == [(0, 0, 0, 8, 0, 0), (1, 0, 0, 8, 0, 0)] and (audio == 0xFF).all()
    assert (capi.audio_encode_reference(np.zeros((1, 8), np.float32), "alaw")[0] == 0xD5).all()


def test_float_step_at_exact_ties(pkg):
    """float32 x whose float32 product with 32767 is exactly k + 0.5: the result is the EVEN neighbour, for either sign."""
    capi = pkg.capi
    found = ac.ties()
    assert any(k % 2 == 0 for k, _ in found) and any(k % 2 == 1 for k, _ in found), found
    assert {0, 1, 2} <= {k for k, _ in found}
    for k, x in found:
        assert np.float32(x * np.float32(32767.0)) == np.float32(k + 0.5)
        want = k if k % 2 == 0 else k + 1
        q, clipped = capi.audio_quantize_reference(np.array([x, -x], np.float32))
        assert q.tolist() == [want, -want] and not clipped.any(), (k, x, q)
