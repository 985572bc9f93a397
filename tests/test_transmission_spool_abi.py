"""The transmission spool's public interface without a GPU: the five entry points in the built library and in the header, the constants, the 48-byte record and
the 64-byte counters, and the definition in plain Python (capi.transmission_spool_reference) against cases worked by hand from the rule and against the
invariants every schedule must keep."""
import ctypes as C
import os

import numpy as np
import pytest

import spool_cases as sc
import test_output_gate as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_transmission_spool", "airband_hip_collect_transmissions", "airband_hip_spool_flush", "airband_hip_spool_counters_get",
         "airband_hip_device_transmission_spool")
capi = sc.capi
IDLE, MAX, FLUSH = capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.TRANSMISSION_SPOOL_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # additions only
    for m in ("set_transmission_spool", "collect_transmissions", "spool_flush", "spool_counters", "device_transmission_spool"):
        assert callable(getattr(pkg.AirbandHip, m)), m


def test_constants_and_structs(pkg):
    assert (IDLE, MAX, FLUSH) == (1, 2, 3)
    assert C.sizeof(capi.Transmission) == 48 and C.sizeof(capi.SpoolCounters) == 64
    want = dict(channel=0, open_batch=4, last_batch=8, close_batch=12, n_rows=16, n_lost=20, n_clipped=24, peak=28, first=30, end=32, reason=34, row_offset=36,
                reserved=40)
    dt = np.dtype(capi.TRANSMISSION_DTYPE)
    assert dt.itemsize == 48
    assert {f[0]: getattr(capi.Transmission, f[0]).offset for f in capi.Transmission._fields_} == want == {n: dt.fields[n][1] for n in dt.names}
    assert capi.SPOOL_COUNTER_NAMES == ("steps", "open_now", "waiting_now", "free_rows_now", "finished_total", "dropped_transmissions", "rows_stored_total",
                                        "rows_lost_total")
    assert [getattr(capi.SpoolCounters, n).offset for n in capi.SPOOL_COUNTER_NAMES] == list(range(0, 64, 8))


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_set_transmission_spool(airband_hip_handle* h, const uint8_t* spool, int64_t pool_rows, int64_t export_rows, int64_t max_records, "
                 "int32_t min_batches, int32_t idle_batches, int32_t max_batches);",
                 "int airband_hip_collect_transmissions(airband_hip_handle* h, int64_t* n, airband_hip_transmission* records, void* audio, int64_t* n_rows, int64_t* n_waiting);",
                 "int airband_hip_spool_flush(airband_hip_handle* h);",
                 "int airband_hip_spool_counters_get(airband_hip_handle* h, airband_hip_spool_counters* out);",
                 "int airband_hip_device_transmission_spool(airband_hip_handle* h, void** d_export_audio, airband_hip_transmission** d_export_records, int32_t** d_n_export);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("#define AIRBAND_SPOOL_IDLE 1\n", "#define AIRBAND_SPOOL_MAX 2\n", "#define AIRBAND_SPOOL_FLUSH 3\n", "} airband_hip_transmission; /* 48 bytes */",
                   "} airband_hip_spool_counters; /* 64 bytes */", "k - open_batch > min_batches", "k - last_batch > idle_batches", "k - open_batch > max_batches",
                   "STORED iff j < F", "export_rows >= max_batches + 1", "#define AIRBAND_HIP_ABI_VERSION 2u"):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L = pkg.load_library()
    n, rows, waiting = C.c_int64(7), C.c_int64(7), C.c_int64(7)
    p = [C.c_void_p() for _ in range(3)]
    out = capi.SpoolCounters()
    assert L.airband_hip_set_transmission_spool(None, None, 8, 8, 8, 8, 4, 4) == capi.EINVAL
    assert L.airband_hip_set_transmission_spool(None, None, 0, 0, 0, 0, 0, 0) == capi.EINVAL
    assert L.airband_hip_collect_transmissions(None, C.byref(n), None, None, C.byref(rows), C.byref(waiting)) == capi.EINVAL
    assert (n.value, rows.value, waiting.value) == (7, 7, 7)
    assert L.airband_hip_spool_flush(None) == capi.EINVAL
    assert L.airband_hip_spool_counters_get(None, C.byref(out)) == capi.EINVAL
    assert L.airband_hip_device_transmission_spool(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)


# ---- the model against cases worked by hand --------------------------------------------------------------------------------------------------------------
# The gate delivers the patterns of tests/test_output_gate.py in these batches (test_the_patterns_open_and_close_where_intended verifies them against the
# oracle): k_and_k2 1-4, two_long 1-3, late 3-4.  Channels 0, 1, 2; min_batches 2, idle_batches 1.
PATTERN_CHANNELS = ["k_and_k2", "two_long", "late"]


def _pattern_steps(n_steps=8, B=8):
    act = og.expected_active([og.SIGNAL] * 3, og.intended_axc(PATTERN_CHANNELS))
    assert act[:8] == [[], [0, 1], [0, 1], [0, 1, 2], [0, 2], [], [], []]
    steps = []
    for k in range(n_steps):
        ch = np.array(act[k], np.int32)
        audio = np.zeros((len(ch), B), np.uint8)
        audio[:, 0], audio[:, 1] = k, ch
        info = np.zeros(len(ch), capi.AUDIO_ROW_DTYPE)
        info["channel"], info["peak"], info["n_clipped"], info["first"], info["end"] = ch, 100 * k + ch, 1, k, B - ch
        steps.append(dict(selected=ch, channels=ch, audio=audio, info=info))
    return steps


def _feed(model, steps):
    for s in steps:
        model.step(len(s["selected"]), s["channels"], s["audio"], s["info"])


def _clip(c, batches, B=8):
    return b"".join(bytes([k, c] + [0] * (B - 2)) for k in batches)


def test_hand_case_idle_closes():
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=16, export_rows=17, max_records=8, min_batches=2, idle_batches=1, max_batches=16)
    _feed(m, _pattern_steps())
    got = m.collect()
    # (channel, open, last, close, n_rows, n_lost, n_clipped, peak, first, end, reason, row_offset)
    assert sc.brief(got["records"]) == [(1, 1, 3, 5, 3, 0, 3, 301, 1, 7, IDLE, 0), (0, 1, 4, 6, 4, 0, 4, 400, 1, 8, IDLE, 3), (2, 3, 4, 6, 2, 0, 2, 402, 3, 6, IDLE, 7)]
    assert got["audio"] == _clip(1, [1, 2, 3]) + _clip(0, [1, 2, 3, 4]) + _clip(2, [3, 4])
    assert got["n_rows"] == 9 and got["n_waiting"] == 0
    assert m.counters() == dict(steps=8, open_now=0, waiting_now=0, free_rows_now=16, finished_total=3, dropped_transmissions=0, rows_stored_total=9, rows_lost_total=0)
    assert m.collect()["records"].shape == (0,)  # an empty list gives n = 0


def test_hand_case_max_closes_and_reopens():
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=16, export_rows=3, max_records=8, min_batches=2, idle_batches=1, max_batches=2)
    _feed(m, _pattern_steps())
    recs, audio = [], b""
    while True:
        got = m.collect()
        assert got["n_rows"] <= 3
        recs += [r[:11] for r in sc.brief(got["records"])]
        audio += got["audio"]
        if not got["n_waiting"]:
            break
    assert recs == [(0, 1, 3, 4, 3, 0, 3, 300, 1, 8, MAX), (1, 1, 3, 4, 3, 0, 3, 301, 1, 7, MAX), (2, 3, 4, 6, 2, 0, 2, 402, 3, 6, IDLE), (0, 4, 4, 7, 1, 0, 1, 400, 4, 8, IDLE)]
    assert audio == _clip(0, [1, 2, 3]) + _clip(1, [1, 2, 3]) + _clip(2, [3, 4]) + _clip(0, [4])


def test_hand_case_flush():
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=16, export_rows=17, max_records=8, min_batches=2, idle_batches=1, max_batches=16)
    _feed(m, _pattern_steps(5))
    m.flush()
    got = sc.brief(m.collect()["records"])
    assert [(r[0], r[3], r[4], r[10]) for r in got] == [(0, 5, 4, FLUSH), (1, 5, 3, FLUSH), (2, 5, 2, FLUSH)]
    assert m.counters()["steps"] == 5 and m.counters()["open_now"] == 0


def test_hand_case_pool_exhaustion_and_drops():
    """pool_rows 4: steps 1 and 2 store channels 0 and 1, steps 3 and 4 find no row for anybody -- channel 2's transmission has n_rows 0."""
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=4, export_rows=4, max_records=8, min_batches=2, idle_batches=1, max_batches=3)
    _feed(m, _pattern_steps())
    m.flush()
    got = sc.brief(m.collect()["records"])
    assert [(r[0], r[3], r[4], r[5], r[10]) for r in got] == [(0, 5, 2, 2, MAX), (1, 5, 2, 1, IDLE), (2, 6, 0, 2, IDLE)]
    assert any(r[4] == 0 and r[5] > 0 for r in got), got
    # max_records 1: the second transmission to finish while one waits is dropped, its rows come back
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=16, export_rows=17, max_records=1, min_batches=2, idle_batches=1, max_batches=16)
    _feed(m, _pattern_steps())
    assert m.counters()["dropped_transmissions"] == 2 and m.counters()["waiting_now"] == 1 and m.counters()["free_rows_now"] == 16 - 3
    assert sc.brief(m.collect()["records"])[0][:5] == (1, 1, 3, 5, 3)


def test_rows_past_max_rows_are_lost_and_need_the_selection():
    m = capi.transmission_spool_reference([1, 1, 1], 8, pool_rows=16, export_rows=17, max_records=8, min_batches=2, idle_batches=1, max_batches=16)
    s = _pattern_steps()[3]
    with pytest.raises(ValueError):
        m.step(3, s["channels"][:2], s["audio"][:2], s["info"][:2])
    m.step(3, s["channels"][:2], s["audio"][:2], s["info"][:2], selected=[0, 1, 2])
    m.flush()
    assert [(r[0], r[4], r[5]) for r in sc.brief(m.collect()["records"])] == [(0, 1, 0), (1, 1, 0), (2, 0, 1)]


# ---- invariants over random schedules -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_ch,pool_rows,max_records,max_batches,max_rows", [(1, 40, 1000, 1000, 50, None), (2, 40, 9, 1000, 4, None), (3, 70, 30, 2, 3, None),
                                                                                    (4, 70, 25, 5, 6, 7), (5, 1, 3, 1, 2, None)])
def test_invariants_over_random_schedules(seed, n_ch, pool_rows, max_records, max_batches, max_rows):
    """Every selected row of a spooled channel is in exactly one clip, or counted in n_lost, or went with a dropped transmission; free + held rows == pool_rows
    after every step."""
    mask, steps = sc.schedule(n_ch, 40, seed, max_rows=max_rows)
    model = capi.transmission_spool_reference(mask, 16, pool_rows=pool_rows, export_rows=max_batches + 1, max_records=max_records, min_batches=3, idle_batches=1,
                                              max_batches=max_batches)
    clips, lost, selected_rows = [], 0, 0
    sent = {}
    for k, s in enumerate(steps):
        model.step(len(s["selected"]), s["channels"], s["audio"], s["info"], selected=s["selected"])
        selected_rows += sum(1 for c in s["selected"] if mask[c])
        for r, c in enumerate(s["channels"]):
            sent[(k, int(c))] = s["audio"][r].tobytes()
        cn = model.counters()
        held = sum(t["n_rows"] for t in model.open.values()) + sum(t["n_rows"] for t in model.finished)
        assert cn["free_rows_now"] + held == pool_rows and cn["free_rows_now"] >= 0
        assert cn["waiting_now"] <= max_records
        if k % 5 == 4:
            clips.append(model.collect())
    model.flush()
    while True:
        clips.append(model.collect())
        if not clips[-1]["n_waiting"]:
            break
    cn = model.counters()
    assert cn["open_now"] == 0 and cn["waiting_now"] == 0 and cn["free_rows_now"] == pool_rows
    seen = set()
    n_rec = 0
    for got in clips:
        assert got["n_rows"] <= max_batches + 1
        for r in got["records"]:
            n_rec += 1
            assert r["n_rows"] <= max_batches + 1
            rows = got["audio"][16 * int(r["row_offset"]):16 * int(r["row_offset"] + r["n_rows"])]
            lost += int(r["n_lost"])
            for i in range(int(r["n_rows"])):
                row = rows[16 * i:16 * i + 16]
                key = (row[0], int(r["channel"]))
                assert row[1] == key[1] & 0xFF and sent[key] == row and key not in seen, key  # the right channel's row, once
                assert int(r["open_batch"]) <= key[0] <= int(r["last_batch"])
                seen.add(key)
    assert n_rec == cn["finished_total"]
    in_dropped = selected_rows - len(seen) - lost  # what dropped transmissions took with them: their records are gone, the counters know their rows
    assert in_dropped >= 0
    if cn["dropped_transmissions"] == 0:
        assert in_dropped == 0 and len(seen) == cn["rows_stored_total"] and lost == cn["rows_lost_total"]
    assert cn["rows_stored_total"] + cn["rows_lost_total"] == selected_rows
    assert len(seen) <= cn["rows_stored_total"] and lost <= cn["rows_lost_total"]
    if seed == 3:
        assert cn["dropped_transmissions"] > 0
    if seed in (2, 4):
        assert cn["rows_lost_total"] > 0
