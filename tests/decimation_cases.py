"""Shared by the output decimation's tests: the model of a decimating handle -- capi.audio_decimate_reference() with the per-channel history carried by the
listed rule of include/airband_hip.h ("output decimation") -- and the input that drives the filter into its output clamp."""
import numpy as np

import audio_cases as ac

capi = ac.capi
H = capi.AUDIO_DECIMATE_HISTORY
TAPS = capi.AUDIO_DECIMATE_TAPS


class Model:
    """n_ch channels' histories, all zero at the start.  step(channels, rows): the listed channels (ascending, already cut to max_rows) and their float rows
    [n][B] -> (audio, info with channel = the listed channel); a channel not listed in a step restarts from zeros."""

    def __init__(self, n_ch, fmt):
        self.fmt = fmt
        self.hist = np.zeros((n_ch, H), "<i2")

    def step(self, channels, rows):
        channels = np.asarray(channels, np.int64)
        rows = np.ascontiguousarray(rows, np.float32)
        audio, info, hist = capi.audio_decimate_reference(rows, self.fmt, self.hist[channels])
        info["channel"] = channels
        self.hist = np.zeros_like(self.hist)
        self.hist[channels] = hist
        return audio, info


def saturating_rows(n, B, seed=0):
    """Rows whose samples are +-full scale with the sign of the tap that meets them at output n0: |acc| = 54056 * 32767 there, far beyond the clamp.  The pattern
    sits at a different place in every row; the rest is a seeded quiet signal.  Row r alternates the overall sign."""
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n, B)) * 0.02).astype(np.float32)
    sign = np.where(TAPS >= 0, 1.0, -1.0).astype(np.float32)
    for r in range(n):
        n0 = 30 + (r * 37) % (B // 2 - 60)  # output index; S[2 n0 + j] = row[2 n0 + j - 46]
        t0 = 2 * n0 - H
        rows[r, t0:t0 + 47] = sign * (1.0 if r % 2 == 0 else -1.0)
    return rows
