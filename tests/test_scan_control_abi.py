"""Scan control's public interface without a GPU: the five entry points in the built library and in the header, the two structs, and the definition in plain
Python (capi.scan_control_reference) on a sequence whose answers are written out by hand."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_scan_control", "airband_hip_scan_hold", "airband_hip_collect_scan_events", "airband_hip_collect_scan_state",
         "airband_hip_device_scan_control")


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    assert sorted(pkg.capi.SCAN_CONTROL_PROTOTYPES) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.SCAN_CONTROL_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # no existing struct changed
    for method in ("set_scan_control", "scan_hold", "collect_scan_events", "collect_scan_state", "device_scan_control"):
        assert callable(getattr(pkg.AirbandHip, method))


def test_struct_sizes_and_offsets(pkg):
    capi = pkg.capi
    assert C.sizeof(capi.ScanEvent) == 16 and C.sizeof(capi.ScanState) == 16
    want = {capi.ScanEvent: dict(dev=0, freq_idx=4, prev_idx=6, kind=8, flags=9, reserved=10, batch=12),
            capi.ScanState: dict(idx=0, hold=2, idle=4, since=8, last=12, has_list=14)}
    for struct, dtype in ((capi.ScanEvent, capi.SCAN_EVENT_DTYPE), (capi.ScanState, capi.SCAN_STATE_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct)
        assert {f[0]: getattr(struct, f[0]).offset for f in struct._fields_} == want[struct] == {n: dt.fields[n][1] for n in dt.names}
    assert (capi.SCAN_HOP, capi.SCAN_ACTIVITY, capi.SCAN_RETAG) == (1, 2, 1)


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_set_scan_control(airband_hip_handle* h, int32_t idle_batches, int32_t dwell_batches, int64_t max_records);",
                 "int airband_hip_scan_hold(airband_hip_handle* h, int32_t dev, int32_t freq_idx);",
                 "int airband_hip_collect_scan_events(airband_hip_handle* h, int64_t* n_records, airband_hip_scan_event* records);",
                 "int airband_hip_collect_scan_state(airband_hip_handle* h, int32_t first_dev, int32_t n_dev, airband_hip_scan_state* state);",
                 "int airband_hip_device_scan_control(airband_hip_handle* h, int32_t** d_n_records, airband_hip_scan_event** d_records, airband_hip_scan_state** d_state);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above ...
        comment = text[text[:at].rindex("/*"):at]
        assert "src/rtl_airband.cpp:1" in comment, decl  # ... that cites the reference lines it replaces
    for phrase in ("} airband_hip_scan_event; /* 16 bytes */", "} airband_hip_scan_state; /* 16 bytes */", "#define AIRBAND_SCAN_HOP 1", "#define AIRBAND_SCAN_ACTIVITY 2",
                   "#define AIRBAND_SCAN_RETAG 1", "#define AIRBAND_HIP_ABI_VERSION 2", "A handle without scan control does exactly the work it did."):
        assert phrase in text, phrase


def test_null_handle_is_refused_without_a_device(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    p = [C.c_void_p() for _ in range(3)]
    n = C.c_int64(7)
    assert L.airband_hip_set_scan_control(None, 16, 2, 0) == capi.EINVAL
    assert L.airband_hip_scan_hold(None, 0, 0) == capi.EINVAL
    assert L.airband_hip_collect_scan_events(None, C.byref(n), None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_collect_scan_state(None, 0, 1, None) == capi.EINVAL
    assert L.airband_hip_device_scan_control(None, *[C.byref(x) for x in p]) == capi.EINVAL and not any(x.value for x in p)


def test_reference_by_hand(pkg):
    """One list of three entries on dongle 5, idle_batches = 2.  Columns of a state: (idx, hold, idle, since, last, has_list); of a record:
    (dev, freq_idx, prev_idx, kind, flags, reserved, batch)."""
    capi = pkg.capi
    HOP, ACT, RETAG = capi.SCAN_HOP, capi.SCAN_ACTIVITY, capi.SCAN_RETAG
    quiet, signal = ord(" "), ord("*")
    st = capi.scan_control_blank()
    assert st.tolist() == (0, -1, 0, 0, 0, 1) and st.dtype == np.dtype(capi.SCAN_STATE_DTYPE)

    def step(k, axc, dwell, want_state, want_rec, **kw):
        nonlocal st
        before = st.tobytes()
        new, rec = capi.scan_control_reference(st, axc, kw.pop("n", 3), k, idle_batches=2, dwell_batches=dwell, dev=5, **kw)
        assert st.tobytes() == before  # its arguments are left alone
        assert rec.dtype == np.dtype(capi.SCAN_EVENT_DTYPE) and new.dtype == np.dtype(capi.SCAN_STATE_DTYPE)
        assert new.tolist() == want_state and rec.tolist() == ([want_rec] if want_rec else []), (k, new.tolist(), rec.tolist())
        st = new

    # dwell 1: the reference's thread.  Idle saturates at 2, the first hop comes one batch later, then one per batch, wrapping at the end of the list
    step(0, quiet, 1, (0, -1, 1, 0, 0, 1), None)
    step(1, quiet, 1, (0, -1, 2, 0, 0, 1), None)
    step(2, quiet, 1, (1, -1, 2, 0, 0, 1), (5, 1, 0, HOP, 0, 0, 2))
    step(3, quiet, 1, (2, -1, 2, 0, 0, 1), (5, 2, 1, HOP, 0, 0, 3))
    step(4, quiet, 1, (0, -1, 2, 0, 0, 1), (5, 0, 2, HOP, 0, 0, 4))
    # the squelch opens after a saturated spell on the entry of the last activity (0): ACTIVITY without RETAG; the batch after is no news
    step(5, signal, 1, (0, -1, 0, 0, 0, 1), (5, 0, 0, ACT, 0, 0, 5))
    step(6, signal, 1, (0, -1, 0, 0, 0, 1), None)
    step(7, quiet, 1, (0, -1, 1, 0, 0, 1), None)
    step(8, ord("<"), 1, (0, -1, 0, 0, 0, 1), None)  # a signal before saturation (any byte but ' '): idle starts again, no record
    step(9, quiet, 1, (0, -1, 1, 0, 0, 1), None)
    step(10, quiet, 1, (0, -1, 2, 0, 0, 1), None)
    step(11, quiet, 1, (1, -1, 2, 0, 0, 1), (5, 1, 0, HOP, 0, 0, 11))
    step(12, signal, 1, (1, -1, 0, 0, 1, 1), (5, 1, 0, ACT, RETAG, 0, 12))  # on another entry than the last activity's: RETAG, last = 1
    # dwell 2: every other batch once saturated
    step(13, quiet, 2, (1, -1, 1, 0, 1, 1), None)
    step(14, quiet, 2, (1, -1, 2, 0, 1, 1), None)
    step(15, quiet, 2, (1, -1, 2, 1, 1, 1), None)
    step(16, quiet, 2, (2, -1, 2, 0, 1, 1), (5, 2, 1, HOP, 0, 0, 16))
    step(17, quiet, 2, (2, -1, 2, 1, 1, 1), None)
    # a frozen dongle and a list of one entry: nothing moves, whatever the byte
    step(18, quiet, 2, (2, -1, 2, 1, 1, 1), None, enabled=False)
    step(19, signal, 2, (2, -1, 2, 1, 1, 1), None, enabled=False)
    step(20, quiet, 2, (2, -1, 2, 1, 1, 1), None, n=1)
    # hold: a HOP to the pinned entry behind the next batch whatever the byte says, counters cleared; then nothing while it is pinned
    st["hold"] = 0
    step(21, signal, 2, (0, 0, 0, 0, 1, 1), (5, 0, 2, HOP, 0, 0, 21))
    step(22, quiet, 2, (0, 0, 0, 0, 1, 1), None)
    step(23, quiet, 2, (0, 0, 0, 0, 1, 1), None)
    # release: the count starts from nothing
    st["hold"] = -1
    step(24, quiet, 2, (0, -1, 1, 0, 1, 1), None)
    step(25, quiet, 2, (0, -1, 2, 0, 1, 1), None)
    step(26, signal, 2, (0, -1, 0, 0, 0, 1), (5, 0, 1, ACT, RETAG, 0, 26))
    # the batch number is a uint32
    _, rec = capi.scan_control_reference(dict_state(capi, idx=1, idle=2), quiet, 2, (1 << 32) + 3, idle_batches=2, dwell_batches=1, dev=9)
    assert rec.tolist() == [(9, 0, 1, HOP, 0, 0, 3)]


def dict_state(capi, **kw):
    st = capi.scan_control_blank()
    for k, v in kw.items():
        st[k] = v
    return st
