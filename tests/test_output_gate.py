"""Signal-gated collect (airband_hip_set_output_gate / _collect_active / _device_active), the parts that need no GPU: the exports, the rule stated in
plain Python and checked on hand-written cases, and -- with the CPU oracle -- that the stage-2 inputs tests/test_gpu_gate.py feeds open and close the
squelch in the batches they are meant to."""
import ctypes as C

import numpy as np
import pytest

import pyoracle

NEVER, SIGNAL, ALWAYS = 0, 1, 2


def expected_active(gate, axc_history, enabled_history=None):
    """The rule of include/airband_hip.h, "signal-gated collect".  gate [C] bytes; axc_history [K][C] axcindicate bytes of K consecutive batches;
    enabled_history [K][C] truth values (the channel's dongle was switched on for the batch; default: always).  Returns, per batch, the ascending list
    of delivered channels.
    SIGNAL: delivered iff the batch's axcindicate is not ' ' or the batch before's was not (the reference's file-output rule, src/output.cpp:501,531);
    ALWAYS: every batch; NEVER: never.  A channel of a dongle that is off is not delivered and forgets the batch before."""
    gate = np.asarray(gate)
    prev = np.zeros(len(gate), bool)
    out = []
    for k, axc in enumerate(axc_history):
        on = np.ones(len(gate), bool) if enabled_history is None else np.asarray(enabled_history[k], bool)
        signal = on & (np.asarray(axc) != ord(" "))
        active = on & ((gate == ALWAYS) | ((gate == SIGNAL) & (signal | prev)))
        out.append([int(c) for c in np.flatnonzero(active)])
        prev = signal
    return out


def _axc(rows):
    return [np.frombuffer(r.encode(), np.uint8) for r in rows]


# ---- the rule itself, on cases written out by hand -------------------------------------------------------------------------------------------------
def test_rule_first_batch_counts_nothing_before_it():
    assert expected_active([SIGNAL, SIGNAL], _axc([" *", "  "])) == [[1], [1]]
    assert expected_active([SIGNAL], _axc([" "])) == [[]]


def test_rule_one_trailing_batch_and_never_two():
    got = expected_active([SIGNAL], _axc(["*", "*", " ", " ", " ", "*", " ", " "]))
    assert got == [[0], [0], [0], [], [], [0], [0], []]


def test_rule_afc_indicators_are_signal():
    assert expected_active([SIGNAL, SIGNAL, SIGNAL], _axc(["<> ", "   ", "   "])) == [[0, 1], [0, 1], []]


def test_rule_never_and_always():
    gate = [NEVER, ALWAYS, SIGNAL, NEVER]
    got = expected_active(gate, _axc(["****", "    ", "    "]))
    assert got == [[1, 2], [1, 2], [1]]


def test_rule_dongle_switched_off_and_on_again():
    gate = [SIGNAL, ALWAYS, SIGNAL]  # channels 0, 1: dongle A; channel 2: dongle B
    axc = _axc(["* *", "  *", "  *", "* *", "   "])
    on = [[1, 1, 1], [0, 0, 1], [0, 0, 1], [1, 1, 1], [1, 1, 1]]
    got = expected_active(gate, axc, on)
    # batch 1: A is off from this batch on -- not even the trailing batch of channel 0, not the ALWAYS channel; batch 3: back, with signal;
    # batch 4: the trailing batch of batch 3's signal
    assert got == [[0, 1, 2], [2], [2], [0, 1, 2], [0, 1, 2]]
    # the memory of the batch before is cleared by the switch-off: signal in batch 0, off in batch 1, back and quiet in batch 2 -> no trailing batch
    assert expected_active([SIGNAL], _axc(["*", " ", " "]), [[1], [0], [1]]) == [[0], [], []]
    # ... and a channel that reports signal while its dongle is off (it cannot, but the rule does not depend on that) leaves no memory either
    assert expected_active([SIGNAL], _axc(["*", "*", " "]), [[1], [0], [1]]) == [[0], [], []]


def test_rule_order_is_ascending():
    rng = np.random.default_rng(3)
    gate = rng.integers(0, 3, 300)
    axc = [np.where(rng.random(300) < 0.3, ord("*"), ord(" ")).astype(np.uint8) for _ in range(6)]
    for row in expected_active(gate, axc):
        assert row == sorted(row)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_three_entry_points_are_exported_with_their_signatures(pkg, built):
    L = pkg.load_library()
    for name in ("airband_hip_set_output_gate", "airband_hip_collect_active", "airband_hip_device_active"):
        assert name in pkg.EXPORTS
        assert hasattr(L, name), name
    vp, i64 = C.c_void_p, C.c_int64
    assert L.airband_hip_set_output_gate.argtypes == [vp, vp, i64]
    assert L.airband_hip_collect_active.argtypes == [vp, C.POINTER(i64), vp, vp, vp, vp]
    assert L.airband_hip_device_active.argtypes == [vp] + [C.POINTER(vp)] * 4
    header = open(pkg.HERE + "/../include/airband_hip.h").read()
    for decl in ("int airband_hip_set_output_gate(airband_hip_handle* h, const uint8_t* gate, int64_t max_rows);",
                 "int airband_hip_collect_active(airband_hip_handle* h, int64_t* n_active, int32_t* channel_index, float* waveout, float* iq_out, char* axc_all);",
                 "int airband_hip_device_active(airband_hip_handle* h, int32_t** d_index, int32_t** d_count, float** d_rows, float** d_iq_rows);"):
        assert decl in header, decl
    for k, name in enumerate(("AIRBAND_GATE_NEVER", "AIRBAND_GATE_SIGNAL", "AIRBAND_GATE_ALWAYS")):
        assert "#define %s %d\n" % (name, k) in header
    assert (pkg.capi.GATE_NEVER, pkg.capi.GATE_SIGNAL, pkg.capi.GATE_ALWAYS) == (NEVER, SIGNAL, ALWAYS)
    assert "#define AIRBAND_HIP_ABI_VERSION 2u" in header and pkg.capi.ABI_VERSION == 2  # additions only


def test_null_handles_are_refused(pkg, built):
    L, capi = pkg.load_library(), pkg.capi
    gate = (C.c_uint8 * 4)(1, 1, 1, 1)
    n = C.c_int64(-7)
    assert L.airband_hip_set_output_gate(None, gate, 4) == capi.EINVAL
    assert L.airband_hip_set_output_gate(None, None, 0) == capi.EINVAL
    assert L.airband_hip_collect_active(None, C.byref(n), None, None, None, None) == capi.EINVAL
    assert n.value == -7
    p = [C.c_void_p() for _ in range(4)]
    assert L.airband_hip_device_active(None, *[C.byref(x) for x in p]) == capi.EINVAL
    assert L.airband_hip_device_active(None, None, None, None, None) == capi.EINVAL
    assert not any(x.value for x in p)


# ---- the stage-2 inputs of the GPU tests ---------------------------------------------------------------------------------------------------------------
# A pattern says, per batch, whether the channel's squelch is to open in the batch: axcindicate starts every batch as ' ' and becomes '*' with the first
# sample that has audio (the oracle's stage2_channel), so a batch in which a transmission ends still reports '*' and the batch after it is the trailing one.
N_BATCHES = 8
PATTERNS = {
    "quiet": [0, 0, 0, 0, 0, 0, 0, 0],
    "k_and_k2": [0, 1, 0, 1, 0, 0, 0, 0],  # signal in batches 1 and 3: delivered in 1, 2, 3, 4 and in no later batch
    "two_long": [0, 1, 1, 0, 0, 0, 0, 0],  # delivered in 1, 2, 3
    "late": [0, 0, 0, 1, 0, 0, 0, 0],      # delivered in 3, 4
}
PATTERN_NAMES = sorted(PATTERNS)
KEY_ON, KEY_OFF, KEY_AMP = 200, 500, 25.0  # the carrier is up over samples [200, 500) of a batch, and from one batch into the next where both have signal


def pattern_bins(name, B):
    """Stage-1 output of one AM channel for the N_BATCHES batches of pattern `name`: [(wavein [B], iq_in [2 B])] -- complex noise of 0.7 per component
    and a carrier of KEY_AMP while the pattern's transmission lasts; |bin| in float32 as the reference computes it from the two floats."""
    rng = np.random.default_rng(1000 + PATTERN_NAMES.index(name))
    want = PATTERNS[name]
    z = (rng.standard_normal((N_BATCHES * B, 2)) * 0.7).astype(np.float32)
    on = np.zeros(N_BATCHES * B, bool)
    for b in range(N_BATCHES):
        if want[b]:
            on[b * B + KEY_ON:b * B + KEY_OFF] = True
            if b + 1 < N_BATCHES and want[b + 1]:
                on[b * B + KEY_OFF:(b + 1) * B + KEY_ON] = True
    ph = 0.3 * np.arange(N_BATCHES * B)
    z[on, 0] += (KEY_AMP * np.cos(ph[on])).astype(np.float32)
    z[on, 1] += (KEY_AMP * np.sin(ph[on])).astype(np.float32)
    re, im = z[:, 0], z[:, 1]
    mag = np.sqrt(re * re + im * im).astype(np.float32)
    return [(mag[b * B:(b + 1) * B].copy(), np.ascontiguousarray(z[b * B:(b + 1) * B]).reshape(2 * B).copy()) for b in range(N_BATCHES)]


def channel(k, **kw):
    c = dict(frequency=118_850_000 + 300_000 * k, modulation=0)
    c.update(kw)
    return c


def intended_axc(names):
    """[N_BATCHES][len(names)] axcindicate bytes the patterns are built to produce"""
    return [np.array([ord("*") if PATTERNS[n][b] else ord(" ") for n in names], np.uint8) for b in range(N_BATCHES)]


@pytest.mark.parametrize("iq_outputs", [0, 1])
def test_the_patterns_open_and_close_where_intended(pkg, built, iq_outputs):
    """Each pattern through the CPU oracle's stage 2, as a plain AM channel and as one with a raw-I/Q output (the generic demod kind on the GPU)."""
    names = PATTERN_NAMES * 2
    devices = [dict(channels=[channel(k, has_iq_outputs=iq_outputs) for k in range(len(names))])]
    orc = pyoracle.Oracle(devices, wave_rate=8000)
    try:
        bins = [pattern_bins(n, orc.B) for n in names]
        want = intended_axc(names)
        for b in range(N_BATCHES):
            r = orc.run_bins(0, np.stack([x[b][0] for x in bins]), np.stack([x[b][1] for x in bins]))
            assert bytes(r["axc"]) == bytes(want[b]), (b, bytes(r["axc"]), bytes(want[b]))
            for k, n in enumerate(names):  # a closed squelch writes zeros: what makes a quiet channel's row not worth copying
                if not PATTERNS[n][b] and not (b > 0 and PATTERNS[n][b - 1]):
                    assert not r["waveout"][k][100:].any(), (b, n)
    finally:
        orc.close()
    # what the GPU test relies on, from the rule alone
    act = expected_active([SIGNAL] * 3, intended_axc(["k_and_k2", "two_long", "late"]))
    assert act[0] == [] and act[7] == [] and act[3] == [0, 1, 2]            # nothing at all / every SIGNAL channel
    assert 1 in act[3] and not PATTERNS["two_long"][3]                        # delivered only because of the batch before
    assert 0 in act[1] and 0 in act[3] and all(0 not in a for a in act[5:])   # active in k and k + 2, not delivered in a later quiet batch
