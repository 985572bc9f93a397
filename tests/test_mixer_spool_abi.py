"""The mixer transmission spool's public interface without a GPU: the five entry points in the built library and in the header, the stereo OR that the shared
definition (capi.transmission_spool_reference) gained, and the model fed by capi.mixer_gate_reference() on a schedule worked by hand."""
import ctypes as C
import os

import numpy as np

import spool_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_mixer_spool", "airband_hip_collect_mixer_transmissions", "airband_hip_mixer_spool_flush", "airband_hip_mixer_spool_counters_get",
         "airband_hip_device_mixer_spool")
capi = sc.capi
IDLE, MAX, FLUSH = capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH
NEVER, SIGNAL, ALWAYS = capi.GATE_NEVER, capi.GATE_SIGNAL, capi.GATE_ALWAYS


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    assert tuple(capi.MIXER_SPOOL_PROTOTYPES) == NAMES
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == capi.MIXER_SPOOL_PROTOTYPES[name]
    twins = dict(zip(NAMES, capi.TRANSMISSION_SPOOL_PROTOTYPES.values()))
    assert all(capi.MIXER_SPOOL_PROTOTYPES[n] == twins[n] for n in NAMES)  # the channel twins' prototypes
    assert capi.ABI_VERSION == 2  # additions only
    for m in ("set_mixer_spool", "collect_mixer_transmissions", "mixer_spool_flush", "mixer_spool_counters", "device_mixer_spool"):
        assert callable(getattr(pkg.AirbandHip, m)), m


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_set_mixer_spool(airband_hip_handle* h, const uint8_t* spool, int64_t pool_rows, int64_t export_rows, int64_t max_records, "
                 "int32_t min_batches, int32_t idle_batches, int32_t max_batches);",
                 "int airband_hip_collect_mixer_transmissions(airband_hip_handle* h, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting);",
                 "int airband_hip_mixer_spool_flush(airband_hip_handle* h);",
                 "int airband_hip_mixer_spool_counters_get(airband_hip_handle* h, airband_hip_spool_counters* out);",
                 "int airband_hip_device_mixer_spool(airband_hip_handle* h, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    section = text.index("---- mixer transmission spool")
    assert section > text.index("---- transmission spool") and all(text.index(n + "(") > section for n in NAMES)
    pinned = "Out of scope: a transmission spool over mixer rows, raw-I/Q, MP3, and per-mixer encodings."
    assert "mixer transmission spool" in text[text.index(pinned) + len(pinned):section]  # the old sentence stays, and points here
    for phrase in ("reserved[1] of a finished record is the OR of the stored rows' airband_hip_audio_row.reserved", "One spool step per MIXER GATE STEP",
                   "#define AIRBAND_HIP_ABI_VERSION 2u"):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L = pkg.load_library()
    n, rows, waiting = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    p = [C.c_void_p() for _ in range(3)]
    out = capi.SpoolCounters()
    assert L.airband_hip_set_mixer_spool(None, None, 8, 8, 8, 8, 4, 4) == capi.EINVAL
    assert L.airband_hip_set_mixer_spool(None, None, 0, 0, 0, 0, 0, 0) == capi.EINVAL
    assert L.airband_hip_collect_mixer_transmissions(None, C.byref(n), None, None, C.byref(rows), C.byref(waiting)) == capi.EINVAL
    assert (n.value, rows.value, waiting.value) == (7, 7, 7)
    assert L.airband_hip_mixer_spool_flush(None) == capi.EINVAL
    assert L.airband_hip_mixer_spool_counters_get(None, C.byref(out)) == capi.EINVAL
    assert L.airband_hip_device_mixer_spool(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)


# ---- reserved[1]: the OR of the stored records' `reserved` ------------------------------------------------------------------------------------------------
def _rows(items, k, B, reserved):
    """what a gate and a pack leave for the listed items at step k: rows whose bytes name (step, item), records with the given `reserved`"""
    items = np.asarray(items, np.int32)
    audio = np.zeros((len(items), B), np.uint8)
    audio[:, 0], audio[:, 1] = k, items
    info = np.zeros(len(items), capi.AUDIO_ROW_DTYPE)
    info["channel"], info["peak"], info["first"], info["end"], info["reserved"] = items, 10 * k + items, k, B - items, reserved
    return audio, info


def test_reserved_of_a_mono_then_stereo_mixer_is_one_and_of_channels_zero():
    """Mixer 0 is mono in steps 0 and 1 and stereo in step 2 (airband_hip_mixer_set_stereo between the steps); mixer 1 stays mono; mixer 2 is stereo in its only
    step, whose row finds no pool row (pool of 5): a flag that was never STORED is not in the OR."""
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=5, export_rows=9, max_records=8, min_batches=2, idle_batches=1, max_batches=8)
    m.step(2, [0, 1], *_rows([0, 1], 0, 8, [0, 0]))
    m.step(2, [0, 1], *_rows([0, 1], 1, 8, [0, 0]))
    m.step(3, [0, 1, 2], *_rows([0, 1, 2], 2, 8, [1, 0, 1]))  # rows held: 4 -> F = 1: mixer 0 stores (j = 0), mixers 1 and 2 lose
    m.flush()
    got = m.collect()
    assert [(int(r["channel"]), int(r["n_rows"]), int(r["n_lost"]), r["reserved"].tolist()) for r in got["records"]] == [(0, 3, 0, [0, 1]), (1, 2, 1, [0, 0]), (2, 0, 1, [0, 0])]
    # channel-shaped records (reserved 0 throughout): reserved[1] stays 0, so the channel spool's bytes are what they were
    m = capi.transmission_spool_reference([1, 1], 8, pool_rows=8, export_rows=9, max_records=8, min_batches=2, idle_batches=1, max_batches=8)
    for k in range(3):
        m.step(2, [0, 1], *_rows([0, 1], k, 8, 0))
    m.flush()
    assert (m.collect()["records"]["reserved"] == 0).all()
    # flags OR bit by bit
    m = capi.transmission_spool_reference([1], 8, pool_rows=8, export_rows=9, max_records=8, min_batches=2, idle_batches=1, max_batches=8)
    for k, f in enumerate((4, 0, 1)):
        m.step(1, [0], *_rows([0], k, 8, [f]))
    m.flush()
    assert m.collect()["records"]["reserved"].tolist() == [[0, 5]]


# ---- the model fed by the mixer gate's reference, on a schedule worked by hand -----------------------------------------------------------------------------
# Three mixers, gates SIGNAL, SIGNAL, ALWAYS; B = 4 frames, stereo rows (W = 2), ulaw; min_batches 2, idle_batches 1, max_batches 3.
#   has_signal of mixer 0: steps 1 .. 6     -> the gate lists it in steps 1 .. 7 (one trailing step)
#   has_signal of mixer 1: steps 2, 3 and 9 -> listed in 2, 3, 4 and in 9, 10
#   mixer 2 is ALWAYS: listed every step, never spooled.
# Spool steps (k = the step), by the rule:
#   mixer 0 opens at 1; at k = 5: age 4 > max_batches 3 -> MAX, rows 1 .. 4; it is selected in 5 again and opens at 5; last 7; at k = 9: age 4 > 2 and quiet
#     2 > 1 -> IDLE (and age 4 > 3 too: idle names the reason), rows 5, 6, 7;
#   mixer 1 opens at 2, last 4; at k = 6: age 4 > 2, quiet 2 > 1 -> IDLE, rows 2, 3, 4; opens at 9, last 10; the run ends after step 10 -> FLUSH at 11, rows 9, 10.
# Mixer 1 turns stereo between steps 9 and 10: its second clip has reserved[1] = 1, its first 0; mixer 0 is stereo throughout: 1 and 1.
def test_model_fed_by_the_mixer_gate_reference_on_a_hand_schedule():
    B, n_steps = 4, 11
    gate = np.array([SIGNAL, SIGNAL, ALWAYS], np.uint8)
    sig = np.zeros((n_steps, 3), np.uint8)
    sig[1:7, 0] = 1
    sig[[2, 3, 9], 1] = 1
    rng = np.random.default_rng(11)
    batches = []
    for k in range(n_steps):
        left = (rng.random((3, B), np.float32) - 0.5) * sig[k][:, None].clip(0, 1)
        right = (rng.random((3, B), np.float32) - 0.5) * sig[k][:, None].clip(0, 1)
        batches.append((left.astype(np.float32), right.astype(np.float32), sig[k], [1, 1 if k >= 10 else 0, 0]))
    ref = capi.mixer_gate_reference(gate, 3, "ulaw", True, batches)
    assert [r["mixers"].tolist() for r in ref] == [[2], [0, 2], [0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 2], [0, 2], [0, 2], [2], [1, 2], [1, 2]]
    model = capi.transmission_spool_reference(gate == SIGNAL, B, pool_rows=16, export_rows=4, max_records=8, min_batches=2, idle_batches=1, max_batches=3)
    sel = capi.mixer_gate_selection(gate)
    for k, r in enumerate(ref):
        assert sel.step(sig[k]).tolist() == r["mixers"].tolist()  # the gate's rule from has_signal: what `selected` is made of when the list is short
        model.step(r["n_active"], r["mixers"], r["rows"], r["info"])
    model.flush()
    recs, audio = [], b""
    while True:
        got = model.collect()
        assert got["n_rows"] <= 4
        recs += list(got["records"])
        audio += got["audio"]
        if not got["n_waiting"]:
            break
    # (mixer, open, last, close, n_rows, reason, reserved[1])
    assert [(int(r["channel"]), int(r["open_batch"]), int(r["last_batch"]), int(r["close_batch"]), int(r["n_rows"]), int(r["reason"]), int(r["reserved"][1])) for r in recs] == \
        [(0, 1, 4, 5, 4, MAX, 1), (1, 2, 4, 6, 3, IDLE, 0), (0, 5, 7, 9, 3, IDLE, 1), (1, 9, 10, 11, 2, FLUSH, 1)]
    assert all(int(r["reserved"][0]) == 0 and int(r["n_lost"]) == 0 for r in recs)

    def row(k, m):
        return ref[k]["rows"][ref[k]["mixers"].tolist().index(m)].tobytes()

    want = b"".join(row(k, 0) for k in (1, 2, 3, 4)) + b"".join(row(k, 1) for k in (2, 3, 4)) + b"".join(row(k, 0) for k in (5, 6, 7)) + b"".join(row(k, 1) for k in (9, 10))
    assert audio == want and len(audio) == 12 * 2 * B
    # frames: the trailing rows (step 7 for mixer 0, step 4 for mixer 1) are silence, so `end` of those clips is 0; `first` is the first stored row's
    assert [int(r["end"]) for r in recs[:3]] == [int(ref[4]["info"][0]["end"]), 0, 0] and int(recs[1]["first"]) == int(ref[2]["info"][1]["first"])
    assert model.counters() == dict(steps=11, open_now=0, waiting_now=0, free_rows_now=16, finished_total=4, dropped_transmissions=0, rows_stored_total=12, rows_lost_total=0)
