"""The output decimation's definition without a GPU (include/airband_hip.h, "output decimation"; capi.AUDIO_DECIMATE_TAPS / audio_decimate_reference): the tap
table and what the header states about it, the response computed from the table, the reference against a plain int64 numpy.convolve of the q stream, batches with a
carried history against one shot, a constant input, the output clamp, and the record on the constructed rows of tests/audio_cases.py.  Pure numpy."""
import os
import re

import numpy as np
import pytest

import audio_cases as ac
import decimation_cases as dc

capi = ac.capi
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = capi.AUDIO_DECIMATE_TAPS
SIDE = [10383, -3332, 1853, -1178, 781, -520, 339, -213, 126, -68, 32, -11]


def _plain(stream):
    """y of a whole q stream that starts from a zero history: the full int64 convolution, every second value from index 46 on, shifted and clamped"""
    S = np.concatenate([np.zeros(46, np.int64), np.asarray(stream, np.int64)])
    full = np.convolve(S, TAPS.astype(np.int64))  # full[m] = sum_j h[j] S[m - j]; h is symmetric, so sum_j h[j] S[2 n + j] = full[2 n + 46]
    r = (full[46:46 + len(stream):2] + 16384) >> 15
    return np.clip(r, -32767, 32767), r


def test_tap_table():
    assert TAPS.dtype == np.int64 and TAPS.shape == (47,) and not TAPS.flags.writeable
    assert int(TAPS.sum()) == 32768 and int(np.abs(TAPS).sum()) == 54056
    assert 54056 * 32767 + 16384 < 2 ** 31
    assert np.array_equal(TAPS, TAPS[::-1]) and TAPS[23] == 16384
    assert [int(TAPS[23 + d]) for d in range(1, 24, 2)] == SIDE == [int(TAPS[23 - d]) for d in range(1, 24, 2)]
    zero = [j for j in range(47) if j != 23 and (j - 23) % 2 == 0]
    assert len(zero) == 22 and not TAPS[zero].any() and np.count_nonzero(TAPS) == 25
    assert capi.AUDIO_DECIMATE_HISTORY == 46


def test_the_table_is_the_one_the_kernel_and_the_header_hold():
    src = open(os.path.join(ROOT, "rtlsdr-airband_amd", "csrc", "audio_decimate.h")).read()
    m = re.search(r"AUDIO_DECIMATE_SIDE\[12\] = \{([^}]*)\}", src)
    assert [int(x) for x in m.group(1).split(",")] == SIDE
    assert "AUDIO_DECIMATE_CENTRE = 16384" in src and "AUDIO_DECIMATE_TAPS = 47" in src and "AUDIO_DECIMATE_HIST = 46" in src
    header = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert "#define AIRBAND_AUDIO_DECIMATE_TAPS 47\n" in header
    assert ", ".join(str(t) for t in SIDE) in header and "h[23] = 16384" in header
    for decl in ("int airband_hip_set_output_decimation(airband_hip_handle* h, int32_t factor);",
                 "int airband_hip_encoded_row_samples(const airband_hip_handle* h);",
                 "int airband_hip_decimate_audio(airband_hip_handle* h, int32_t encoding, const float* rows, int64_t n_rows, int16_t* history, void* audio, airband_hip_audio_row* info);"):
        at = header.index(decl)
        assert header[:at].rstrip().endswith("*/"), decl  # a comment right above
    assert header.index("---- encoded audio collect") < header.index("---- output decimation") < header.index("---- RTP packet stream")


def test_response_computed_from_the_table():
    """+-0.05 dB up to 3.4 kHz and <= -50 dB from 4.6 kHz at 16 kHz input (on this 1 Hz grid the table gives -0.019 .. +0.011 dB and -53.0 dB)."""
    f = np.arange(0, 8001, dtype=np.float64)
    resp = np.abs(np.exp(-2j * np.pi * np.outer(f, np.arange(47)) / 16000.0) @ (TAPS / 32768.0))
    db = 20 * np.log10(np.maximum(resp, 1e-12))
    passband, stopband = db[f <= 3400], db[f >= 4600]
    print("passband %.4f .. %.4f dB, stopband max %.2f dB" % (passband.min(), passband.max(), stopband.max()))
    assert passband.min() >= -0.05 and passband.max() <= 0.05
    assert stopband.max() <= -50.0
    assert abs(resp[0] - 1.0) < 1e-12  # the DC gain is exact


@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_reference_is_a_plain_convolution(fmt):
    rows = np.concatenate([ac.random_rows(9, 1000, seed=21), dc.saturating_rows(3, 1000)])
    q, clipped = capi.audio_quantize_reference(rows)
    audio, info, hist = capi.audio_decimate_reference(rows, fmt)
    assert audio.shape == (12, 500) and audio.dtype == (np.dtype("<i2") if fmt == "s16" else np.uint8) and hist.shape == (12, 46) and hist.dtype == np.dtype("<i2")
    for r in range(12):
        y, raw = _plain(q[r])
        want = y.astype("<i2") if fmt == "s16" else capi.audio_law_reference(y.astype(np.int32), capi.AUDIO_ENCODINGS[fmt])
        assert np.array_equal(audio[r], want), r
        assert int(info["n_clipped"][r]) == int(clipped[r].sum()) + int((y != raw).sum())
        assert np.array_equal(hist[r], q[r, -46:])
    assert info["channel"].tolist() == list(range(12)) and not info["reserved"].any()


@pytest.mark.parametrize("B", [1000, 2000])
def test_batches_with_carried_history_equal_one_shot(B):
    rows = ac.random_rows(5, 4 * B, seed=B + 1)
    rows[:, :] += (np.sin(np.arange(4 * B) * 0.07) * 0.4).astype(np.float32)  # no silent rows: the history matters
    whole, _, hist_whole = capi.audio_decimate_reference(rows, "s16")
    hist, parts = None, []
    for k in range(4):
        a, _, hist = capi.audio_decimate_reference(rows[:, k * B:(k + 1) * B], "s16", hist)
        parts.append(a)
    assert np.array_equal(np.concatenate(parts, axis=1), whole) and np.array_equal(hist, hist_whole)
    dropped, _, _ = capi.audio_decimate_reference(rows[:, B:2 * B], "s16")  # without the history the batch's first 23 outputs differ
    assert not np.array_equal(dropped[:, :23], parts[1][:, :23]) and np.array_equal(dropped[:, 23:], parts[1][:, 23:])


def test_a_constant_reproduces_itself_once_the_history_is_full():
    x = np.array([[0.3], [-0.71], [1.0], [-1.0], [1e-4]], np.float32) * np.ones((1, 1000), np.float32)
    q, _ = capi.audio_quantize_reference(x)
    first, _, hist = capi.audio_decimate_reference(x, "s16")
    assert np.array_equal(first[:, 23:], q[:, :477])  # from output 23 on every tap sees the constant: sum h = 32768
    assert not np.array_equal(first[:, :23], q[:, :23])
    second, info, _ = capi.audio_decimate_reference(x, "s16", hist)
    assert np.array_equal(second, q[:, :500])
    assert info["peak"].tolist() == np.abs(q[:, 0]).tolist() and info["first"].tolist() == [0] * 5 and info["end"].tolist() == [500] * 5 and not info["n_clipped"].any()


def test_a_saturating_input_clamps_and_is_counted():
    rows = dc.saturating_rows(4, 1000)
    q, clipped = capi.audio_quantize_reference(rows)
    assert not clipped.any()  # +-1.0 is full scale, not beyond it
    audio, info, _ = capi.audio_decimate_reference(rows, "s16")
    for r in range(4):
        n0 = 30 + (r * 37) % 440
        _, raw = _plain(q[r])
        assert abs(int(raw[n0])) == (54056 * 32767 + 16384) >> 15 and abs(int(raw[n0])) > 32767
        assert int(audio[r, n0]) == (32767 if r % 2 == 0 else -32767)
        assert int(info["n_clipped"][r]) == int((np.abs(raw) > 32767).sum()) >= 1 and int(info["peak"][r]) == 32767
    law = capi.audio_decimate_reference(rows, "ulaw")[0]
    assert law[0, 30] == capi.audio_law_reference(np.array([32767]), capi.AUDIO_ULAW)[0]


@pytest.mark.parametrize("B", [1000, 2000])
def test_record_on_the_constructed_rows(B):
    rows = np.concatenate([ac.extremes_rows(B), ac.random_rows(40, B, seed=B + 3), np.zeros((1, B), np.float32)])
    hist = (np.random.default_rng(8).integers(-3000, 3000, (len(rows), 46))).astype("<i2")
    hist[-1] = 0
    infos = []
    for fmt in ac.FORMATS:
        audio, info, _ = capi.audio_decimate_reference(rows, fmt, hist)
        infos.append(info)
        if fmt == "s16":
            y = audio.astype(np.int64)
    assert infos[0].tobytes() == infos[1].tobytes() == infos[2].tobytes()  # computed on y, whatever the format
    info = infos[0]
    for r in range(len(rows)):
        nz = np.flatnonzero(y[r])
        want = (int(nz[0]), int(nz[-1]) + 1) if len(nz) else (B // 2, 0)
        assert (int(info["first"][r]), int(info["end"][r])) == want, r
        assert int(info["peak"][r]) == int(np.abs(y[r]).max())
    assert (int(info["first"][-1]), int(info["end"][-1]), int(info["peak"][-1])) == (B // 2, 0, 0)
    assert (info["first"] > 0).any() and (info["end"] < B // 2).any() and (info["n_clipped"] > 0).any()
