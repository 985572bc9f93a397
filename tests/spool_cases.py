"""Shared by the transmission spool's tests: random selection schedules with rows and records a gate and an encoder could have left, a driver that feeds
capi.transmission_spool_reference() with them, and the comparison of records."""
import importlib

import numpy as np

capi = importlib.import_module("rtlsdr-airband_amd").capi

REC = np.dtype(capi.TRANSMISSION_DTYPE)
RECORD_FIELDS = ("channel", "open_batch", "last_batch", "close_batch", "n_rows", "n_lost", "n_clipped", "peak", "first", "end", "reason", "row_offset")


def schedule(n_ch, n_steps, seed, max_rows=None, row_bytes=16, wave_batch=16, p_start=0.12, p_stop=0.35, every_other=True):
    """A run of n_steps batches over n_ch channels: transmissions start and stop at random, so channels are selected in bursts with gaps.  Returns
    (mask [n_ch] bytes, steps) with steps[k] = dict(selected: ascending channels, channels: the first max_rows of them, audio [n][row_bytes] uint8,
    info [n] of AUDIO_ROW_DTYPE).  Every row's bytes are its own (step, channel), so a row in the wrong clip shows."""
    rng = np.random.default_rng(seed)
    max_rows = n_ch if max_rows is None else max_rows
    mask = np.ones(n_ch, np.uint8)
    if every_other and n_ch > 1:
        mask[1::3] = 0  # channels the gate selects and the spool ignores
    on = np.zeros(n_ch, bool)
    steps = []
    for k in range(n_steps):
        flip = rng.random(n_ch)
        on = np.where(on, flip >= p_stop, flip < p_start)
        if k >= n_steps - 3:
            on[:] = False  # a quiet tail: the idle rule gets its turn
        selected = np.flatnonzero(on).astype(np.int32)
        channels = selected[:max_rows]
        n = len(channels)
        audio = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
        if n:
            audio[:, 0] = k & 0xFF
            audio[:, 1] = channels & 0xFF
        info = np.zeros(n, capi.AUDIO_ROW_DTYPE)
        info["channel"] = channels
        info["peak"] = rng.integers(0, 32768, n)
        info["n_clipped"] = rng.integers(0, 3, n) * rng.integers(0, wave_batch + 1, n)
        info["first"] = rng.integers(0, wave_batch + 1, n)
        info["end"] = rng.integers(0, wave_batch + 1, n)
        steps.append(dict(selected=selected, channels=channels, audio=audio, info=info))
    return mask, steps


def run_model(mask, steps, wave_batch, ops=None, **params):
    """ops: per step index, what follows the step: a string of "f" (flush) and "c" (collect).  A flush and collects until nothing waits end the run.
    Returns (model, collects: the collect() results in order)."""
    model = capi.transmission_spool_reference(mask, wave_batch, **params)
    collects = []
    for k, s in enumerate(steps):
        model.step(len(s["selected"]), s["channels"], s["audio"], s["info"], selected=s["selected"])
        for op in (ops or {}).get(k, ""):
            if op == "f":
                model.flush()
            else:
                collects.append(model.collect())
    model.flush()
    while True:
        collects.append(model.collect())
        if collects[-1]["n_waiting"] == 0:
            break
    return model, collects


def brief(records):
    """records as tuples of RECORD_FIELDS, for messages and hand-written expectations"""
    return [tuple(int(r[f]) for f in RECORD_FIELDS) for r in records]
