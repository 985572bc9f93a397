"""The mixer RTP stream's public interface without a GPU: the seven entry points in the built library and in the header, the pure function
airband_hip_mixer_rtp_slot_bytes(), and the definition in plain Python (capi.rtp_stream_reference with a width, and its flush()) against values worked by hand
and against a recorded run of the width-less reference (tests/golden/rtp_reference_widthless.bin)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import rtp_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_mixer_rtp_stream", "airband_hip_collect_mixer_rtp_packets", "airband_hip_collect_mixer_rtp_state", "airband_hip_mixer_rtp_counters_get",
         "airband_hip_mixer_rtp_flush", "airband_hip_device_mixer_rtp_stream", "airband_hip_mixer_rtp_slot_bytes")
capi = rc.capi


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.MIXER_RTP_PROTOTYPES[name]
    assert set(NAMES) == set(pkg.capi.MIXER_RTP_PROTOTYPES)
    assert pkg.capi.ABI_VERSION == 2  # additions only
    for m in ("set_mixer_rtp_stream", "collect_mixer_rtp_packets", "collect_mixer_rtp_state", "mixer_rtp_counters", "mixer_rtp_flush", "device_mixer_rtp_stream"):
        assert callable(getattr(pkg.AirbandHip, m)), m


def test_structs_are_the_channel_streams(pkg):
    """no new struct: the mixer stream's sources, records, state and counters are the channel stream's"""
    assert (C.sizeof(capi.RtpSource), C.sizeof(capi.RtpPacket), C.sizeof(capi.RtpState), C.sizeof(capi.RtpCounters)) == (12, 16, 16, 40)
    assert capi.MIXER_RTP_PROTOTYPES["airband_hip_mixer_rtp_counters_get"][1] == C.POINTER(capi.RtpCounters)


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_mixer_rtp_slot_bytes(int32_t encoding, int32_t frame_samples, int32_t width);",
                 "int airband_hip_set_mixer_rtp_stream(airband_hip_handle* h, const airband_hip_rtp_source* sources, int32_t frame_samples, int64_t max_packets);",
                 "int airband_hip_collect_mixer_rtp_packets(airband_hip_handle* h, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets, uint8_t* signal_all);",
                 "int airband_hip_collect_mixer_rtp_state(airband_hip_handle* h, int64_t first_mixer, int64_t n_mixers, airband_hip_rtp_state* state);",
                 "int airband_hip_mixer_rtp_counters_get(airband_hip_handle* h, airband_hip_rtp_counters* out);",
                 "int airband_hip_mixer_rtp_flush(airband_hip_handle* h);",
                 "int airband_hip_device_mixer_rtp_stream(airband_hip_handle* h, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    assert text.index("---- mixer transmission spool") < text.index("---- mixer RTP stream") < text.index("---- band scope")
    section = text[text.index("---- mixer RTP stream"):text.index("---- band scope")]
    for phrase in ("12 + F * W * sample_bytes <= 1472", "count frames", "COLLECT FIRST", "k does not advance", "stream == 0 is how each rank", "F <= 364"):
        assert phrase in section, phrase


LEGAL_F = range(40, 1464, 4)


def test_slot_bytes_needs_no_gpu(pkg, built):
    L = pkg.load_library()
    f = L.airband_hip_mixer_rtp_slot_bytes
    for enc in (capi.AUDIO_ULAW, capi.AUDIO_ALAW, capi.AUDIO_S16):  # width 1 is the channel function, over every legal F and the refused ones beside them
        for F in list(LEGAL_F) + [36, 38, 162, 1464, 1468, 2000]:
            assert f(enc, F, 1) == L.airband_hip_rtp_slot_bytes(enc, F), (enc, F)
    assert f(capi.AUDIO_S16, 364, 2) == 16 * ((12 + 364 * 4 + 15) // 16) == 1472 == capi.mixer_rtp_slot_bytes("s16", 364, 2)
    assert f(capi.AUDIO_S16, 368, 2) == capi.EBADSIZE
    assert f(capi.AUDIO_ULAW, 728, 2) == 1472 == capi.mixer_rtp_slot_bytes("ulaw", 728, 2) and f(capi.AUDIO_ALAW, 728, 2) == 1472
    assert f(capi.AUDIO_ULAW, 732, 2) == capi.EBADSIZE and f(capi.AUDIO_ALAW, 732, 2) == capi.EBADSIZE
    assert f(capi.AUDIO_ULAW, 160, 2) == 336 == capi.mixer_rtp_slot_bytes("ulaw", 160, 2) and f(capi.AUDIO_S16, 160, 2) == 656
    for F in LEGAL_F:  # the formula, and the Python twin, wherever the packet fits
        for enc, sb in ((capi.AUDIO_ULAW, 1), (capi.AUDIO_S16, 2)):
            if 12 + F * 2 * sb <= 1472:
                assert f(enc, F, 2) == (12 + F * 2 * sb + 15) // 16 * 16 == capi.mixer_rtp_slot_bytes(enc, F, 2)
            else:
                assert f(enc, F, 2) == capi.EBADSIZE
    for F in (36, 162):
        assert f(capi.AUDIO_ULAW, F, 2) == capi.EBADSIZE
    for enc in (capi.AUDIO_F32, 4, -1):
        assert f(enc, 160, 2) == capi.EINVAL
    for width in (0, 3, -1):
        assert f(capi.AUDIO_ULAW, 160, width) == capi.EINVAL
    for bad in (("s16", 368, 2), ("ulaw", 732, 2), ("ulaw", 160, 3)):
        with pytest.raises(ValueError):
            capi.mixer_rtp_slot_bytes(*bad)
    assert capi.mixer_rtp_slot_bytes("alaw", 160) == capi.rtp_slot_bytes("alaw", 160) == 176


def test_null_handle_is_refused_without_a_device(pkg, built):
    L = pkg.load_library()
    n = C.c_int64(7)
    src = np.zeros(4, capi.RTP_SOURCE_DTYPE)
    out = capi.RtpCounters()
    p = [C.c_void_p() for _ in range(4)]
    assert L.airband_hip_set_mixer_rtp_stream(None, src.ctypes.data, 160, 8) == capi.EINVAL
    assert L.airband_hip_collect_mixer_rtp_packets(None, C.byref(n), None, None, None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_collect_mixer_rtp_state(None, 0, 1, src.ctypes.data) == capi.EINVAL
    assert L.airband_hip_mixer_rtp_counters_get(None, C.byref(out)) == capi.EINVAL
    assert L.airband_hip_mixer_rtp_flush(None) == capi.EINVAL
    assert L.airband_hip_device_mixer_rtp_stream(None, *[C.byref(x) for x in p]) == capi.EINVAL


# ---- the reference with a width, worked by hand: W = 2, B = 1000, F = 160, mu-law ----------------------------------------------------------------------------
def _stereo_model(max_packets=100):
    src = np.zeros(2, capi.RTP_SOURCE_DTYPE)
    src[0] = (0xAABBCCDD, 5000, 10, 0, 1)
    src[1] = (0x11223344, 0, 0, 0, 1)
    return capi.rtp_stream_reference(src, "ulaw", 1000, 160, max_packets, width=2)


def test_stereo_carry_cycle_lengths_and_timestamps_worked_by_hand():
    """1000 frames = 6 * 160 + 40: the carry runs 40, 80, 120, 0 FRAMES; a packet is 12 + 160 * 2 = 332 bytes; timestamps step by 160 (frames, not samples);
    the marker sits on the first packet of the talkspurt only."""
    model = _stereo_model()
    assert model.slot_bytes == 336
    rows = (np.arange(8 * 2000) % 251).astype(np.uint8).reshape(8, 2000)  # [step][L0 R0 L1 R1 ...]
    carries, counts, ts = [], [], []
    for k in range(8):
        count, records, slots = model.step([0], rows[k:k + 1])
        counts.append(count)
        carries.append(int(model.state()["carry"][0]))
        ts += records["timestamp"].tolist()
        assert (records["length"] == 332).all() and (records["channel"] == 0).all()
        assert records["flags"].tolist() == [capi.RTP_MARKER if (k == 0 and j == 0) else 0 for j in range(count)]
        assert (slots[:, 1] >> 7).tolist() == [1 if (k == 0 and j == 0) else 0 for j in range(count)]
    assert carries == [40, 80, 120, 0] * 2 and counts == [6, 6, 6, 7] * 2
    assert ts == [5000 + 160 * j for j in range(50)]  # 8000 frames sent as 50 packets, no gap and no overlap across the steps
    # step 1's first packet: the 40 carried frames (80 bytes) of row 0 in front of the first 120 frames (240 bytes) of row 1
    model = _stereo_model()
    model.step([0], rows[0:1])
    _, records, slots = model.step([0], rows[1:2])
    assert bytes(slots[0, 12:92]) == rows[0, 1920:].tobytes() and bytes(slots[0, 92:332]) == rows[1, :240].tobytes()
    assert records["timestamp"][0] == 5000 + 1000 - 40 and records["seq"].tolist() == list(range(16, 22))
    st = model.state()[0]
    assert st.tolist() == (12, 12 * 320, 22, 80, 1)  # octets count bytes, carry counts frames


def test_stereo_flush_packet_and_flush_call_worked_by_hand():
    """A mixer that is no longer listed emits ONE packet of 12 + 2 * carry bytes; flush() does the same for every carrying mixer without advancing k."""
    model = _stereo_model()
    rows = (np.arange(2 * 2000) % 241).astype(np.uint8).reshape(2, 2000)
    model.step([0, 1], rows)
    count, records, slots = model.step([1], rows[1:2])  # mixer 0 dropped out with 40 frames carried, mixer 1 goes on to 80
    assert count == 1 + 6 and records["channel"].tolist() == [0] + [1] * 6
    assert (int(records[0]["length"]), int(records[0]["flags"]), int(records[0]["timestamp"])) == (12 + 2 * 40, capi.RTP_FLUSH, 5000 + 1000 - 40)
    assert bytes(slots[0, 12:92]) == rows[0, 1920:].tobytes() and not slots[0, 92:].any()
    assert model.state()["carry"].tolist() == [0, 80] and model.state()["flags"].tolist() == [0, 1]
    before = model.counters()
    count, records, slots = model.flush()
    assert count == 1 and records["channel"].tolist() == [1]
    assert (int(records[0]["length"]), int(records[0]["flags"]), int(records[0]["timestamp"])) == (12 + 2 * 80, capi.RTP_FLUSH, 2 * 1000 - 80)  # k = 2 steps so far
    assert bytes(slots[0, 12:172]) == rows[1, 1840:].tobytes()
    after = model.counters()
    assert after["steps"] == before["steps"] == 2 and after["packets"] == before["packets"] + 1 and after["octets"] == before["octets"] + 160
    assert after["lost_rows"] == before["lost_rows"] == 0
    assert model.state()["carry"].tolist() == [0, 0] and model.state()["flags"].tolist() == [0, 0]
    assert model.flush()[0] == 0 and model.counters() == after  # nothing carried: nothing emitted
    count, records, _ = model.step([1], rows[1:2])  # the next step is step 2, and starts a talkspurt
    assert records["timestamp"][0] == 2 * 1000 and records["flags"][0] == capi.RTP_MARKER and model.counters()["steps"] == 3


def test_s16_stereo_is_left_right_big_endian():
    src = np.zeros(1, capi.RTP_SOURCE_DTYPE)
    src["stream"] = 1
    model = capi.rtp_stream_reference(src, "s16", 1000, 200, 10, width=2)
    row = np.arange(2000, dtype="<i2").reshape(1, 2000) - 1000
    count, records, slots = model.step([0], row)
    assert count == 5 and (records["length"] == 12 + 200 * 4).all() and model.state()["carry"][0] == 0
    assert list(struct.unpack(">400h", bytes(slots[1, 12:812]))) == row[0, 400:800].tolist()


def test_default_width_reproduces_a_recorded_widthless_run():
    """tests/golden/rtp_reference_widthless.bin: two runs of the reference as it was before it had a width (4 channels, 6 steps, a list of 3 rows, 14 slots),
    per step the count, the records, the slots and the state, then the counters."""
    want = open(os.path.join(ROOT, "tests", "golden", "rtp_reference_widthless.bin"), "rb").read()
    got = []
    for enc, B, F, seed in (("ulaw", 1000, 160, 31), ("s16", 2000, 320, 32)):
        src = rc.sources(4, enc, seed, unstreamed=(2,))
        steps = rc.schedule(4, 6, seed + 100, B, enc, max_rows=3, always=(0,), quiet_steps=(4,))
        model = capi.rtp_stream_reference(src, enc, B, F, 14)
        for s in steps:
            count, records, slots = model.step(s["channels"], s["audio"], s["dropped"])
            got += [struct.pack("<i", count), records.tobytes(), slots.tobytes(), model.state().tobytes()]
        c = model.counters()
        got.append(struct.pack("<5q", *[c[k] for k in capi.RTP_COUNTER_NAMES]))
    assert b"".join(got) == want
