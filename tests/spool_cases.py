"""Shared by the transmission spool's tests: random selection schedules with rows and records a gate and an encoder could have left, a driver that feeds
capi.transmission_spool_reference() with them, the comparison of records, and for the CPU tests of both spools (channels and mixers) the script that
tests/host_spool_harness.cpp runs, the model's answer to it and the comparison of the two."""
import importlib
import struct

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


# ---- tests/host_spool_harness.cpp: its script, its results ----------------------------------------------------------------------------------------------------
def script(mask, steps, ops, max_rows, row_bytes, wave_batch, gate=None, **p):
    """The harness's script and the model's answer to it: (blob, expected results, model).  gate None: a channel spool, steps[k] as schedule() makes them (the
    selection bytes go into the script).  gate [n] bytes: a mixer spool, steps[k] = dict(signal, selected, mixers, audio, info) (the has_signal bytes go into
    the script, the harness derives the selection).  ops as run_model()'s; a flush and collects until nothing waits end the run."""
    n = len(mask)
    blob = struct.pack("<11i", 0 if gate is None else 1, n, max_rows, row_bytes, wave_batch, p["pool_rows"], p["export_rows"], p["max_records"], p["min_batches"],
                       p["idle_batches"], p["max_batches"])
    if gate is not None:
        blob += np.asarray(gate, np.uint8).tobytes()
    blob += np.asarray(mask, np.uint8).tobytes()
    model = capi.transmission_spool_reference(mask, wave_batch, **p)
    want = b""

    def collect():
        got = model.collect()
        return struct.pack("<3i", len(got["records"]), got["n_rows"], got["n_waiting"]) + got["records"].tobytes() + got["audio"], got["n_waiting"]

    for k, s in enumerate(steps):
        listed = s["channels"] if gate is None else s["mixers"]
        if gate is None:
            sel = np.zeros(n, np.uint8)
            sel[s["selected"]] = 1
        else:
            sel = s["signal"]
        blob += struct.pack("<i", 0) + sel.tobytes()
        for r in range(len(listed)):
            blob += s["audio"][r].tobytes() + s["info"][r].tobytes()
        model.step(len(s["selected"]), listed, s["audio"], s["info"], selected=s["selected"])
        for op in ops.get(k, ""):
            blob += struct.pack("<i", 1 if op == "f" else 2)
            if op == "f":
                model.flush()
            else:
                want += collect()[0]
    blob += struct.pack("<i", 1)
    model.flush()
    while True:
        blob += struct.pack("<i", 2)
        w, waiting = collect()
        want += w
        if not waiting:
            break
    cn = model.counters()
    want += struct.pack("<8Q", *[cn[k] for k in capi.SPOOL_COUNTER_NAMES])
    return blob, want, model


def collects(blob, row_bytes):
    """the results file taken apart: ([(records, audio bytes, n_waiting)], counters)"""
    out, at = [], 0
    while at + 12 <= len(blob) - 64:
        n, rows, waiting = struct.unpack("<3i", blob[at:at + 12])
        recs = np.frombuffer(blob[at + 12:at + 12 + 48 * n], REC)
        out.append((recs, blob[at + 12 + 48 * n:at + 12 + 48 * n + row_bytes * rows], waiting))
        at += 12 + 48 * n + row_bytes * rows
    return out, struct.unpack("<8Q", blob[-64:])


def compare(got, want, row_bytes, what):
    """walk both results collect by collect, so that a difference is named"""
    if got == want:
        return
    g, w = collects(got, row_bytes), collects(want, row_bytes)
    for i, ((gr, ga, gw), (wr, wa, ww)) in enumerate(zip(g[0], w[0])):
        assert (len(gr), len(ga), gw) == (len(wr), len(wa), ww), "%s: collect %d: counts got %r want %r" % (what, i, (len(gr), len(ga) // row_bytes, gw), (len(wr), len(wa) // row_bytes, ww))
        bad = [j for j in range(len(wr)) if gr[j].tobytes() != wr[j].tobytes()]
        assert not bad, "%s: collect %d: records %r: got %r %r want %r %r" % (what, i, bad[:3], brief(gr[bad[:3]]), gr[bad[:3]]["reserved"].tolist(), brief(wr[bad[:3]]), wr[bad[:3]]["reserved"].tolist())
        assert ga == wa, "%s: collect %d: audio bytes" % (what, i)
    raise AssertionError("%s: counters got %r want %r (%d collects, %d wanted)" % (what, g[1], w[1], len(g[0]), len(w[0])))
