"""An exact-by-construction reference for the coefficient tables of the matrix-core channelizers (test infrastructure, plain numpy).

Written from the definitions (csrc/kernels.h, csrc/common.h), not from the builders in csrc/params.cpp or csrc/misc_kernels.hip:

  A table holds, for the window byte k = 2n + {0: I, 1: Q} and the column 2c + {0: re, 1: im} of channel c on bin b,
      (I + jQ) w[n] exp(-j theta) = (I w cos + Q w sin) + j (Q w cos - I w sin),   theta = 2 pi (b n mod N) / N
  i.e. column re holds (w cos, w sin) for (I, Q) and column im holds (-w sin, w cos).  w[n] is the oracle's window (orc_window_coeff) as float32.
  int8 tables: the value times AB_DFT_COEF_SCALE = 8 355 000, rounded to an integer v = d0 + 256 d1 + 65 536 d2 of balanced digits in [-128, 127], laid out
  [piece][digit t][k-step s = k / 64][lane = ((k % 64) / 16) * 16 + col][byte = k % 16], K = 2 min(N, 512) window bytes per piece; plus, per piece and column,
  corr = half the column sum of v (the u8 path contracts (b - 128) and adds it: (b - 127.5) = (b - 128) + 0.5).
  float tables: the value itself as float32, entry [segment][piece][s][lane] = coefficient (k, column lane & 15) with
  k = segment * 2 SEG + piece * VPP + 16 (s / 4) + 4 (lane >> 4) + s % 4, SEG = min(N, 2048), 4 pieces up to fft 512 and 8 beyond, VPP = 2 SEG / pieces.

PRECISION.  The phase b n mod N is reduced in Python integers and then folded into the first octant by the exact symmetries of sine and cosine, so the axis
values are exactly 0 and +-1.  The octant value is evaluated in numpy.longdouble where that type has a 64-bit mantissa (x86: error ~1e-19, 1e-12 table units after
the scale); where long double is only a double (np.finfo(np.longdouble).nmant < 63) the octant's sine and cosine come from Taylor series in `decimal` at 40 digits
and are rounded once to double (error 1.1e-16 relative, 1e-9 table units).  Either is far inside the 1e-6 the table tests allow on top of the rounding's 0.5.
"""
from __future__ import annotations

import decimal
import functools

import numpy as np

import pyoracle

COEF_SCALE = 8355000.0   # AB_DFT_COEF_SCALE (csrc/common.h)
WIDE = np.finfo(np.longdouble).nmant >= 63
REAL = np.longdouble if WIDE else np.float64


@functools.lru_cache(maxsize=None)
def window(n_fft: int) -> np.ndarray:
    """w[n], n < n_fft: the oracle's window, float32."""
    L = pyoracle.lib()
    w = np.array([L.orc_window_coeff(n_fft, i) for i in range(n_fft)], np.float32)
    w.setflags(write=False)
    return w


def _octant_decimal(j: int, n_fft: int):
    """(cos, sin) of 2 pi j / n_fft for 0 <= 8 j <= n_fft, Taylor series at 40 digits, rounded once to double."""
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        pi = decimal.Decimal("3.141592653589793238462643383279502884197169399375")
        x = 2 * pi * j / n_fft
        c = s = decimal.Decimal(0)
        term = decimal.Decimal(1)
        for i in range(40):   # x <= pi / 4: term 40 is below 1e-52
            if i % 2 == 0:
                c += term if i % 4 == 0 else -term
            else:
                s += term if i % 4 == 1 else -term
            term = term * x / (i + 1)
        return float(c), float(s)


@functools.lru_cache(maxsize=None)
def twiddles(n_fft: int):
    """(cos, sin) of 2 pi p / n_fft for every phase p < n_fft, in REAL."""
    eighth = n_fft // 8
    if WIDE:
        pi = 4 * np.arctan(np.longdouble(1))
        a = 2 * pi * np.arange(eighth + 1, dtype=np.longdouble) / np.longdouble(n_fft)
        oc, os_ = np.cos(a), np.sin(a)
    else:
        pairs = [_octant_decimal(j, n_fft) for j in range(eighth + 1)]
        oc, os_ = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    oc[0], os_[0] = 1, 0
    cos, sin = np.zeros(n_fft, REAL), np.zeros(n_fft, REAL)
    for p in range(n_fft):
        q, r = divmod(p, n_fft // 4)                 # quadrant, position inside it
        c, s = (oc[r], os_[r]) if r <= eighth else (os_[n_fft // 4 - r], oc[n_fft // 4 - r])
        cos[p], sin[p] = [(c, s), (-s, c), (-c, -s), (s, -c)][q]
    cos.setflags(write=False)
    sin.setflags(write=False)
    return cos, sin


def exact_column_pair(n_fft: int, bin_: int, scale: float = COEF_SCALE) -> np.ndarray:
    """x[k][half], k < 2 n_fft, half 0 = re, 1 = im: the unrounded coefficients of one channel on `bin_`, in REAL, times `scale`."""
    cos, sin = twiddles(n_fft)
    phase = np.array([(int(bin_) * n) % n_fft for n in range(n_fft)])   # Python integers
    w = window(n_fft).astype(REAL) * REAL(scale)
    wc, ws = w * cos[phase], w * sin[phase]
    x = np.zeros((2 * n_fft, 2), REAL)
    x[0::2, 0], x[1::2, 0] = wc, ws      # re = I w cos + Q w sin
    x[0::2, 1], x[1::2, 1] = -ws, wc     # im = Q w cos - I w sin
    return x


def exact_table(n_fft: int, bins, scale: float = COEF_SCALE) -> np.ndarray:
    """x[k][col], col < 16: the table of up to eight bins (-1 or missing: the column pair stays zero)."""
    x = np.zeros((2 * n_fft, 16), REAL)
    for c, b in enumerate(bins):
        if b >= 0:
            x[:, 2 * c:2 * c + 2] = exact_column_pair(n_fft, b, scale)
    return x


# ---- int8 tables ------------------------------------------------------------------------------------------------------------------------------------------
def int8_geometry(n_fft: int):
    """(pieces, K window bytes per piece, k-steps per piece, bytes per table)"""
    pieces = n_fft // 512 if n_fft > 512 else 1
    K = 2 * min(n_fft, 512)
    return pieces, K, K // 64, pieces * 3 * K * 16


def unpack_int8_digits(raw, n_fft: int) -> np.ndarray:
    """digits[piece][t][k][col] (int64) of one raw table."""
    pieces, K, KS, nbytes = int8_geometry(n_fft)
    raw = np.asarray(raw).view(np.int8)
    assert raw.shape == (nbytes,), raw.shape
    d = raw.reshape(pieces, 3, KS, 4, 16, 16)            # [piece][t][s][k % 64 / 16][col][k % 16]
    return d.transpose(0, 1, 2, 3, 5, 4).reshape(pieces, 3, K, 16).astype(np.int64)


def unpack_int8(raw, n_fft: int) -> np.ndarray:
    """v[piece][k][col] = d0 + 256 d1 + 65 536 d2 (int64) of one raw table."""
    d = unpack_int8_digits(raw, n_fft)
    return d[:, 0] + 256 * d[:, 1] + 65536 * d[:, 2]


def balanced_digits(v: np.ndarray) -> np.ndarray:
    """digits[..., t] of the integers v: three balanced base-256 digits, each in [-128, 127] (three of them reach +-8 355 711, which is why the scale is 8 355 000)."""
    out, rest = [], np.asarray(v, np.int64)
    for _ in range(3):
        lo = ((rest + 128) & 255) - 128
        out.append(lo)
        rest = (rest - lo) // 256
    assert not rest.any(), "a coefficient does not fit three balanced digits"
    return np.stack(out, axis=-1)


def pack_int8(v: np.ndarray, n_fft: int) -> np.ndarray:
    """The raw table (int8 bytes) of v[piece][k][col]: the inverse of unpack_int8."""
    pieces, K, KS, nbytes = int8_geometry(n_fft)
    d = np.moveaxis(balanced_digits(v), -1, 1)           # [piece][t][k][col]
    d = d.reshape(pieces, 3, KS, 4, 16, 16).transpose(0, 1, 2, 3, 5, 4)   # k = 64 s + 16 g + j -> [s][g][col][j]
    return np.ascontiguousarray(d).astype(np.int8).reshape(nbytes)


def by_piece(x: np.ndarray, n_fft: int) -> np.ndarray:
    """x[k][col] over the whole window -> [piece][k in piece][col]"""
    pieces, K, _, _ = int8_geometry(n_fft)
    return x.reshape(pieces, K, x.shape[-1])


# ---- float tables -----------------------------------------------------------------------------------------------------------------------------------------
def f32_geometry(n_fft: int):
    """(segments, pieces per segment, values per piece, floats per table)"""
    seg = min(n_fft, 2048)
    nw = 4 if n_fft <= 512 else 8
    return n_fft // seg, nw, 2 * seg // nw, 32 * n_fft


def unpack_f32(raw, n_fft: int) -> np.ndarray:
    """f[k][col] (float32), k < 2 n_fft, of one raw float table."""
    nseg, nw, vpp, n = f32_geometry(n_fft)
    raw = np.asarray(raw).view(np.float32)
    assert raw.shape == (n,), raw.shape
    t = raw.reshape(nseg, nw, vpp // 16, 4, 4, 16)       # [segment][piece][s / 4][s % 4][lane >> 4][col]; k in piece = 16 (s / 4) + 4 (lane >> 4) + s % 4
    return t.transpose(0, 1, 2, 4, 3, 5).reshape(2 * n_fft, 16)
