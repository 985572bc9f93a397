"""tests/table_reference.py against the DEFINITION of the pruned DFT (no GPU, and nothing of the project's builders): contracting (byte - 127.5) with the exact
coefficients is the windowed DFT sum of the levels; the unpackers invert the documented layouts."""
import numpy as np
import pytest

import table_reference as tr

FFT_LOGS = [8, 9, 10, 11, 12, 13]


@pytest.mark.parametrize("fft_log", FFT_LOGS)
def test_exact_coefficients_are_the_windowed_dft(built, fft_log):
    """Random bytes, eight bins (0, 1, N / 2, N - 1 and random ones): sum_k (b_k - 127.5) x[k][col] / S against
    X[bin] = sum_n w[n] ((I_n - 127.5) + j (Q_n - 127.5)) exp(-2 pi j bin n / N) summed in float64 with the phase reduced in integers, and against numpy's FFT of the
    windowed samples: both within 1e-12 of the RMS of the exact values (float64 sums of 2 N terms: ~1e-16 x sqrt(2 N) x the terms' size, some 1e-14 relative)."""
    N = 1 << fft_log
    rng = np.random.default_rng(4100 + fft_log)
    bins = [0, 1, N // 2, N - 1] + [int(b) for b in rng.integers(2, N - 1, 4)]
    raw = rng.integers(0, 256, 2 * N).astype(np.float64) - 127.5
    x = tr.exact_table(N, bins).astype(np.float64) / tr.COEF_SCALE
    got = raw @ x                                                 # [16]: re, im per bin
    z = (raw[0::2] + 1j * raw[1::2]) * tr.window(N).astype(np.float64)
    n = np.arange(N)
    want = np.array([np.sum(z * np.exp(-2j * np.pi * ((b * n) % N) / N)) for b in bins])
    spec = np.fft.fft(z)[bins]
    rms = np.sqrt(np.mean(np.abs(want) ** 2))
    assert rms > 0
    got_c = got[0::2] + 1j * got[1::2]
    assert np.abs(got_c - want).max() <= 1e-12 * rms, np.abs(got_c - want).max() / rms
    assert np.abs(got_c - spec).max() <= 1e-12 * rms, np.abs(got_c - spec).max() / rms


def test_signs_on_a_single_tone(built):
    """I + jQ = exp(+2 pi j b n / N) puts the window's sum, real and positive, into bin b and next to nothing into bin N - b: byte 2n is I, 2n + 1 is Q; column 2c is re, 2c + 1 im."""
    N, b = 256, 5
    x = tr.exact_table(N, [b, N - b], scale=1.0).astype(np.float64)
    n = np.arange(N)
    raw = np.empty(2 * N)
    raw[0::2], raw[1::2] = np.cos(2 * np.pi * b * n / N), np.sin(2 * np.pi * b * n / N)
    got = raw @ x
    total = float(tr.window(N).astype(np.float64).sum())
    assert abs(got[0] - total) <= 1e-9 * total and abs(got[1]) <= 1e-9 * total
    assert abs(got[2]) <= 0.1 * total and abs(got[3]) <= 0.1 * total      # the mirror bin sees the window's leakage from ten bins away and no more
    q_only = np.zeros(2 * N)
    q_only[1::2] = 1.0                                                      # Q = 1 at DC: X[0] = j sum w
    dc = q_only @ tr.exact_table(N, [0], scale=1.0).astype(np.float64)
    assert abs(dc[0]) <= 1e-9 * total and abs(dc[1] - total) <= 1e-9 * total


def test_twiddles_are_exact_on_the_axes_and_symmetric():
    for N in (256, 8192):
        c, s = tr.twiddles(N)
        assert (c[0], s[0], c[N // 4], s[N // 4], c[N // 2], s[N // 2]) == (1, 0, 0, 1, -1, 0)
        ulp = 1.1e-19 if tr.WIDE else 2.3e-16   # cos(-a) = cos a, sin(-a) = -sin a: value for value but at the odd eighths, where cos and sin of pi / 4 meet an ulp apart
        assert float(np.abs(c[1:] - c[:0:-1]).max()) <= ulp and float(np.abs(s[1:] + s[:0:-1]).max()) <= ulp
        assert float(np.abs(c.astype(np.float64) - np.cos(2 * np.pi * np.arange(N) / N)).max()) <= 1e-15   # (the double side's rounded angle, up to 2 pi x 1.1e-16)
        assert float(np.abs(c * c + s * s - 1).max()) <= (3e-19 if tr.WIDE else 5e-16)


@pytest.mark.parametrize("fft_log", FFT_LOGS)
def test_int8_layout_round_trip(fft_log):
    """pack_int8 / unpack_int8 invert each other, a coefficient lands on the byte the layout names, and balanced digits recompose."""
    N = 1 << fft_log
    pieces, K, KS, nbytes = tr.int8_geometry(N)
    assert (pieces, K, nbytes) == (max(N // 512, 1), 2 * min(N, 512), 96 * N)
    rng = np.random.default_rng(fft_log)
    top = 127 * (1 + 256 + 65536)   # 8 355 711: what three balanced digits reach, and why the scale is 8 355 000
    v = rng.integers(-top, top + 1, (pieces, K, 16))
    raw = tr.pack_int8(v, N)
    assert np.array_equal(tr.unpack_int8(raw, N), v)
    d = tr.balanced_digits(v)
    assert d.min() >= -128 and d.max() <= 127 and np.array_equal(d[..., 0] + 256 * d[..., 1] + 65536 * d[..., 2], v)
    for _ in range(50):   # [piece][t][s = k / 64][lane = ((k % 64) / 16) * 16 + col][byte = k % 16]
        p, t, k, col = int(rng.integers(pieces)), int(rng.integers(3)), int(rng.integers(K)), int(rng.integers(16))
        at = (((p * 3 + t) * KS + k // 64) * 64 + ((k % 64) // 16) * 16 + col) * 16 + k % 16
        assert raw[at] == d[p, k, col, t]


@pytest.mark.parametrize("fft_log", FFT_LOGS)
def test_f32_layout(fft_log):
    """unpack_f32 reads entry [segment][piece][s][lane] as coefficient k = segment * 2 SEG + piece * VPP + 16 (s / 4) + 4 (lane >> 4) + s % 4, column lane & 15."""
    N = 1 << fft_log
    nseg, nw, vpp, n = tr.f32_geometry(N)
    assert n * 4 == 128 * N and nseg * nw * vpp == 2 * N
    raw = np.arange(n, dtype=np.float32)
    f = tr.unpack_f32(raw, N)
    rng = np.random.default_rng(fft_log)
    kw = vpp // 4
    for _ in range(50):
        seg, piece, s, lane = int(rng.integers(nseg)), int(rng.integers(nw)), int(rng.integers(kw)), int(rng.integers(64))
        k = seg * 2 * min(N, 2048) + piece * vpp + 16 * (s // 4) + 4 * (lane >> 4) + s % 4
        assert f[k, lane & 15] == (((seg * nw + piece) * kw + s) * 64 + lane)
