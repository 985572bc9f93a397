"""The band watch's public interface without a GPU: the four entry points in the built library and in the header, the three structs, the validation in front of
the device, and the definition in plain Python (capi.band_watch_reference) on sequences whose answers are written out by hand (tests/watch_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import watch_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_band_watch", "airband_hip_collect_band_events", "airband_hip_collect_band_tracks", "airband_hip_device_band_watch")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.BAND_WATCH_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # no existing struct changed


def test_struct_sizes_and_offsets(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.BandTrack) == 24 and C.sizeof(capi.BandEvent) == 16 and C.sizeof(capi.BandWatchRow) == 16
    want = {capi.BandTrack: dict(bin=0, power=4, max_power=8, first_batch=12, last_batch=16, hits=20, misses=22, state=23),
            capi.BandEvent: dict(dev=0, bin=4, power=8, kind=12, track=13, batches=14),
            capi.BandWatchRow: dict(n_live=0, n_confirmed=4, n_events=8, dropped=12)}
    for struct, dtype in ((capi.BandTrack, capi.TRACK_DTYPE), (capi.BandEvent, capi.EVENT_DTYPE), (capi.BandWatchRow, capi.WATCH_ROW_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct)
        assert {f[0]: getattr(struct, f[0]).offset for f in struct._fields_} == want[struct] == {n: dt.fields[n][1] for n in dt.names}
    assert (capi.WATCH_APPEAR, capi.WATCH_VANISH) == (1, 2) and (capi.WATCH_FREE, capi.WATCH_TENTATIVE, capi.WATCH_CONFIRMED) == (0, 1, 2)


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    assert "#define AIRBAND_HIP_ABI_VERSION 2" in text
    for decl in ("int airband_hip_set_band_watch(airband_hip_handle* h, int32_t max_tracks, int32_t match_bins, int32_t confirm_hits, int32_t release_misses, int64_t max_events);",
                 "int airband_hip_collect_band_events(airband_hip_handle* h, int64_t* n_events, airband_hip_band_event* events);",
                 "int airband_hip_collect_band_tracks(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_band_watch_row* rows, airband_hip_band_track* tracks);",
                 "int airband_hip_device_band_watch(airband_hip_handle* h, int32_t** d_n_events, airband_hip_band_event** d_events, airband_hip_band_watch_row** d_rows, airband_hip_band_track** d_tracks);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    for phrase in ("} airband_hip_band_track; /* 24 bytes */", "} airband_hip_band_event; /* 16 bytes */", "} airband_hip_band_watch_row; /* 16 bytes */",
                   "#define AIRBAND_WATCH_APPEAR 1", "#define AIRBAND_WATCH_VANISH 2", "BY BIT PATTERN", "is NOT advanced", "not reused", "AIRBAND_HIP_EAGAIN before any batch"):
        assert phrase in text, phrase
    # the prototypes of the header and of capi agree: one ctypes type per parameter
    kinds = {"airband_hip_handle*": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "int64_t*": C.POINTER(C.c_int64), "airband_hip_band_event*": C.c_void_p,
             "airband_hip_band_watch_row*": C.c_void_p, "airband_hip_band_track*": C.c_void_p, "int32_t**": C.POINTER(C.c_void_p),
             "airband_hip_band_event**": C.POINTER(C.c_void_p), "airband_hip_band_watch_row**": C.POINTER(C.c_void_p), "airband_hip_band_track**": C.POINTER(C.c_void_p)}
    for name in NAMES:
        at = text.index("int " + name + "(")
        args = text[at:text.index(");", at)].split("(", 1)[1].split(",")
        assert [kinds[a.strip().rsplit(" ", 1)[0]] for a in args] == pkg.capi.BAND_WATCH_PROTOTYPES[name], name


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    p = [C.c_void_p() for _ in range(4)]
    n = C.c_int64(7)
    assert L.airband_hip_set_band_watch(None, 8, 2, 2, 4, 16) == capi.EINVAL
    assert L.airband_hip_collect_band_events(None, C.byref(n), None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_collect_band_tracks(None, 0, 1, None, None) == capi.EINVAL
    assert L.airband_hip_device_band_watch(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)


CASES = watch_cases.constructed()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_reference_on_constructed_sequences(pkg, case):
    name, p, batches, check = case
    sim = watch_cases.simulate(p, batches)
    check(sim)
    for s in sim:
        assert s["tracks"].dtype == np.dtype(pkg.capi.TRACK_DTYPE) and s["events"].dtype == np.dtype(pkg.capi.EVENT_DTYPE)
        for r in range(p["n_rows"]):
            free = s["tracks"][r]["state"] == 0
            blank = pkg.capi.band_watch_blank(1)[0][0].tobytes()
            assert all(t.tobytes() == blank for t in s["tracks"][r][free])  # a free slot: bin -1, everything else 0
            assert int(s["rows"][r]["n_live"]) == int((~free).sum()) and int(s["rows"][r]["n_events"]) == len(s["row_events"][r]) <= p["max_peaks"] + p["T"]


def test_reference_leaves_its_arguments_alone(pkg):
    capi = pkg.capi
    tracks, row = capi.band_watch_blank(4)
    before = tracks.tobytes(), row.tobytes()
    t, r, ev = capi.band_watch_reference(tracks, row, watch_cases.peak_array([(10, 3.0)], 4), 1, 0, 4, 2, 1, 2, 512, dev=5)
    assert (tracks.tobytes(), row.tobytes()) == before and int(t[0]["bin"]) == 10 and int(r["n_confirmed"]) == 1
    assert ev.tobytes() == np.array([(5, 10, np.float32(3.0), 1, 0, 1)], capi.EVENT_DTYPE).tobytes()
