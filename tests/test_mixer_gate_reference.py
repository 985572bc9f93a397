"""capi.mixer_gate_reference -- the gated mixer collect's definition in numpy (include/airband_hip.h) -- against cases written out by hand."""
import numpy as np
import pytest

import audio_cases as ac

capi = ac.capi
NEVER, SIGNAL, ALWAYS = capi.GATE_NEVER, capi.GATE_SIGNAL, capi.GATE_ALWAYS
B = 16


def _batches(history, stereo_flags=None, seed=0):
    """history: per batch a string with one character per mixer, '*' = has signal; a mixer with signal holds random audio, one without holds zeros"""
    rng = np.random.default_rng(seed)
    out = []
    for row in history:
        sig = np.array([c == "*" for c in row], np.uint8)
        left = (rng.standard_normal((len(row), B)) * 0.3).astype(np.float32) * sig[:, None]
        right = (rng.standard_normal((len(row), B)) * 0.3).astype(np.float32) * sig[:, None]
        out.append((left, right, sig, np.zeros(len(row), np.uint8) if stereo_flags is None else np.asarray(stereo_flags, np.uint8)))
    return out


def _lists(res):
    return [r["mixers"].tolist() for r in res]


def test_one_trailing_batch_and_never_two():
    res = capi.mixer_gate_reference([SIGNAL], 1, None, False, _batches(["*", "*", " ", " ", " ", "*", " ", " "]))
    assert _lists(res) == [[0], [0], [0], [], [], [0], [0], []]
    assert [r["n_active"] for r in res] == [1, 1, 1, 0, 0, 1, 1, 0]
    assert res[2]["rows"].shape == (1, B) and not res[2]["rows"].any()  # the trailing batch's row is the zeros of the sums
    assert res[3]["rows"].shape == (0, B)


def test_first_batch_counts_nothing_before_it():
    assert _lists(capi.mixer_gate_reference([SIGNAL, SIGNAL], 2, None, False, _batches([" *", "  "]))) == [[1], [1]]


def test_always_with_a_silent_mixer_gives_zeros_and_an_empty_extent():
    for stereo in (False, True):
        W = 2 if stereo else 1
        for enc, silence in (("s16", 0), ("ulaw", 0xFF), ("alaw", 0xD5)):
            r = capi.mixer_gate_reference([ALWAYS], 1, enc, stereo, _batches([" "]))[0]
            assert r["n_active"] == 1 and r["mixers"].tolist() == [0]
            assert r["rows"].shape == (1, W * B) and (r["rows"] == silence).all()
            assert r["info"].tolist() == [(0, 0, 0, B, 0, 0)]  # first == B, end == 0
        r = capi.mixer_gate_reference([ALWAYS], 1, None, stereo, _batches([" "]))[0]
        assert r["info"] is None and r["rows"].dtype == np.float32 and r["rows"].shape == (1, W * B) and not r["rows"].any()


def test_never_and_mixed_gates():
    res = capi.mixer_gate_reference([NEVER, ALWAYS, SIGNAL, NEVER], 4, "ulaw", False, _batches(["****", "    ", "    "]))
    assert _lists(res) == [[1, 2], [1, 2], [1]]
    assert [r["info"]["channel"].tolist() for r in res] == [[1, 2], [1, 2], [1]]


def test_overflow_past_max_rows_is_counted_not_listed():
    res = capi.mixer_gate_reference([ALWAYS] * 5, 3, "s16", True, _batches(["* * *"]))
    assert res[0]["n_active"] == 5 and res[0]["mixers"].tolist() == [0, 1, 2]
    assert res[0]["rows"].shape == (3, 2 * B) and len(res[0]["info"]) == 3


@pytest.mark.parametrize("enc", ac.FORMATS)
def test_mono_equals_the_channel_encoder_row_for_row(enc):
    rows = ac.random_rows(9, 1000, seed=21)
    rows[3, :4] = [np.nan, np.inf, -2.0, 1.0]
    sig = np.ones(9, np.uint8)
    r = capi.mixer_gate_reference([ALWAYS] * 9, 9, enc, False, [(rows, np.zeros_like(rows), sig, np.zeros(9, np.uint8))])[0]
    audio, info = capi.audio_encode_reference(rows, enc)
    assert r["rows"].tobytes() == audio.tobytes() and r["info"].tobytes() == info.tobytes()


def test_stereo_rows_interleave_and_the_extent_is_in_frames():
    left, right = np.zeros((2, B), np.float32), np.zeros((2, B), np.float32)
    right[0, 5], right[0, 6] = 0.5, -0.25      # audio in right alone: samples 11 and 13 of the interleaved row, frames 5 and 6
    left[1, 3], right[1, 9] = 1.0, 2.0         # left frame 3 (full scale, not clipped), right frame 9 (clipped)
    batch = [(left, right, np.ones(2, np.uint8), np.zeros(2, np.uint8))]
    r = capi.mixer_gate_reference([ALWAYS, ALWAYS], 2, "s16", True, batch)[0]
    row = r["rows"][0]
    assert row.shape == (2 * B,) and row[11] == 16384 and row[13] == -8192 and np.count_nonzero(row) == 2 and not row[0::2].any()
    assert (int(r["info"][0]["first"]), int(r["info"][0]["end"])) == (5, 7)  # frames, not samples 11 .. 14
    assert r["rows"][1][6] == 32767 and r["rows"][1][19] == 32767
    assert r["info"][1].tolist() == (1, 32767, 1, 3, 10, 0)
    f = capi.mixer_gate_reference([ALWAYS, ALWAYS], 2, None, True, batch)[0]["rows"]
    assert np.array_equal(f[:, 0::2], left) and np.array_equal(f[:, 1::2], right)
    m = capi.mixer_gate_reference([ALWAYS, ALWAYS], 2, "s16", False, batch)[0]   # W = 1: right is not delivered
    assert not m["rows"][0].any() and m["info"][0].tolist() == (0, 0, 0, B, 0, 0)


def test_reserved_is_the_mixers_stereo_flag():
    res = capi.mixer_gate_reference([ALWAYS] * 3, 3, "alaw", True, _batches(["***"], stereo_flags=[0, 1, 7]))
    assert res[0]["info"]["reserved"].tolist() == [0, 1, 1]
    res = capi.mixer_gate_reference([NEVER, ALWAYS, ALWAYS], 3, "alaw", False, _batches(["***"], stereo_flags=[1, 0, 1]))
    assert res[0]["info"]["channel"].tolist() == [1, 2] and res[0]["info"]["reserved"].tolist() == [0, 1]
