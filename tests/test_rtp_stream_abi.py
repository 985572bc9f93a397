"""The RTP packet stream's public interface without a GPU: the six entry points in the built library and in the header, the three structs, the pure function
airband_hip_rtp_slot_bytes(), and the definition in plain Python (capi.rtp_stream_reference) against an independent parser of the packets it writes, against
wrapping fields and against values worked by hand."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import rtp_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("airband_hip_set_rtp_stream", "airband_hip_collect_rtp_packets", "airband_hip_collect_rtp_state", "airband_hip_rtp_counters_get",
         "airband_hip_device_rtp_stream", "airband_hip_rtp_slot_bytes")
capi = rc.capi


def test_symbols_in_the_built_library(pkg, built):
    L = pkg.load_library()
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in pkg.EXPORTS
        assert getattr(L, name).argtypes == pkg.capi.RTP_STREAM_PROTOTYPES[name]
    assert pkg.capi.ABI_VERSION == 2  # additions only
    for m in ("set_rtp_stream", "collect_rtp_packets", "collect_rtp_state", "rtp_counters", "device_rtp_stream"):
        assert callable(getattr(pkg.AirbandHip, m)), m


def test_struct_sizes_and_layouts(pkg):
    assert (C.sizeof(capi.RtpSource), C.sizeof(capi.RtpPacket), C.sizeof(capi.RtpState)) == (12, 16, 16)
    assert C.sizeof(capi.RtpCounters) == 40 and capi.RTP_COUNTER_NAMES == ("steps", "packets", "dropped_packets", "octets", "lost_rows")
    for struct_, dtype in ((capi.RtpSource, capi.RTP_SOURCE_DTYPE), (capi.RtpPacket, capi.RTP_PACKET_DTYPE), (capi.RtpState, capi.RTP_STATE_DTYPE)):
        dt = np.dtype(dtype)
        assert dt.itemsize == C.sizeof(struct_)
        assert {f[0]: getattr(struct_, f[0]).offset for f in struct_._fields_} == {n: dt.fields[n][1] for n in dt.names}
    assert (capi.RTP_MARKER, capi.RTP_FLUSH) == (1, 2)


def test_header_documents_them(pkg):
    text = open(os.path.join(ROOT, "include", "airband_hip.h")).read()
    for decl in ("int airband_hip_set_rtp_stream(airband_hip_handle* h, const airband_hip_rtp_source* sources, int32_t frame_samples, int64_t max_packets);",
                 "int airband_hip_collect_rtp_packets(airband_hip_handle* h, int64_t* n_packets, airband_hip_rtp_packet* records, void* packets, char* axc_all);",
                 "int airband_hip_collect_rtp_state(airband_hip_handle* h, int64_t first_channel, int64_t n_channels, airband_hip_rtp_state* state);",
                 "int airband_hip_rtp_counters_get(airband_hip_handle* h, airband_hip_rtp_counters* out);",
                 "int airband_hip_device_rtp_stream(airband_hip_handle* h, int32_t** d_n_packets, airband_hip_rtp_packet** d_records, void** d_packets, airband_hip_rtp_state** d_state);",
                 "int airband_hip_rtp_slot_bytes(int32_t encoding, int32_t frame_samples);"):
        at = text.index(decl)
        assert text[:at].rstrip().endswith("*/"), decl  # a comment right above
    assert text.index("---- encoded audio collect") < text.index("---- RTP packet stream") < text.index("---- gated mixer collect")
    for phrase in ("} airband_hip_rtp_source;   /* 12 bytes */", "} airband_hip_rtp_packet; /* 16 bytes */", "} airband_hip_rtp_state; /* 16 bytes */",
                   "12 + F * sample_bytes <= 1472", "ts_start = ts0 + k * B - carry_n", "all moves are whole dwords", "Out of scope: mixer rows"):
        assert phrase in text, phrase


def test_slot_bytes_needs_no_gpu(pkg, built):
    L = pkg.load_library()
    assert L.airband_hip_rtp_slot_bytes(capi.AUDIO_ULAW, 160) == 176 == capi.rtp_slot_bytes("ulaw", 160)
    assert L.airband_hip_rtp_slot_bytes(capi.AUDIO_S16, 160) == 336 == capi.rtp_slot_bytes("s16", 160)
    assert L.airband_hip_rtp_slot_bytes(capi.AUDIO_S16, 800) == capi.EBADSIZE
    assert L.airband_hip_rtp_slot_bytes(capi.AUDIO_ALAW, 1460) == 1472 and L.airband_hip_rtp_slot_bytes(capi.AUDIO_ALAW, 1464) == capi.EBADSIZE
    for F in (36, 162):
        assert L.airband_hip_rtp_slot_bytes(capi.AUDIO_ULAW, F) == capi.EBADSIZE
    for enc in (capi.AUDIO_F32, 4, -1):
        assert L.airband_hip_rtp_slot_bytes(enc, 160) == capi.EINVAL
    with pytest.raises(ValueError):
        capi.rtp_slot_bytes("s16", 800)


def test_null_handle_is_refused_without_a_device(pkg, built):
    L = pkg.load_library()
    n = C.c_int64(7)
    src = np.zeros(4, capi.RTP_SOURCE_DTYPE)
    out = capi.RtpCounters()
    p = [C.c_void_p() for _ in range(4)]
    assert L.airband_hip_set_rtp_stream(None, src.ctypes.data, 160, 8) == capi.EINVAL
    assert L.airband_hip_collect_rtp_packets(None, C.byref(n), None, None, None) == capi.EINVAL and n.value == 7
    assert L.airband_hip_collect_rtp_state(None, 0, 1, src.ctypes.data) == capi.EINVAL
    assert L.airband_hip_rtp_counters_get(None, C.byref(out)) == capi.EINVAL
    assert L.airband_hip_device_rtp_stream(None, *[C.byref(x) for x in p]) == capi.EINVAL


# ---- the reference against an independent parser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,B,F", [("ulaw", 1000, 160), ("s16", 2000, 320), ("alaw", 1000, 40), ("s16", 1000, 728)])
def test_random_schedule_against_an_independent_parser(encoding, B, F):
    """6 channels, a random schedule of listed / unlisted batches.  Writing every packet's payload at position timestamp - ts0 reproduces exactly the encoded rows
    of the listed batches and nothing else; seq is consecutive per channel; markers sit exactly on the talkspurt starts; flush packets are exactly the short ones."""
    n_ch, n_steps, sb = 6, 40, rc.sample_bytes(encoding)
    src = rc.sources(n_ch, encoding, 77, unstreamed=(4,))
    steps = rc.schedule(n_ch, n_steps, 78, B, encoding, always=(1,), p_start=0.3, p_stop=0.4)
    wants, counters, model = rc.run_reference(src, encoding, B, F, 10_000, steps)
    timeline = {c: {} for c in range(n_ch)}  # channel -> sample position -> wire bytes of that sample
    next_seq = {c: int(src["seq0"][c]) for c in range(n_ch)}
    markers = {c: [] for c in range(n_ch)}
    n_flush = 0
    for k, (count, records, slots, _) in enumerate(wants):
        assert count == len(records)
        assert records["channel"].tolist() == sorted(records["channel"].tolist())  # channel ascending ...
        for i, r in enumerate(records):
            c = int(r["channel"])
            marker, pt, seq, ts, ssrc, payload = rc.parse_packet(slots[i, :r["length"]])
            assert (pt, ssrc) == (int(src["payload_type"][c]), int(src["ssrc"][c])) and src["stream"][c]
            assert (seq, ts) == (int(r["seq"]), int(r["timestamp"])) and marker == (int(r["flags"]) & 1) and r["reserved"] == 0
            assert seq == next_seq[c]
            next_seq[c] = (seq + 1) & 0xFFFF
            flush = bool(r["flags"] & capi.RTP_FLUSH)
            assert flush == (len(payload) < F * sb) and len(payload) % sb == 0 and (flush or len(payload) == F * sb)  # flush packets are exactly the short ones
            assert not (flush and marker)
            n_flush += flush
            pos = (ts - int(src["ts0"][c])) & 0xFFFFFFFF
            if marker:
                markers[c].append(pos)
            for s in range(len(payload) // sb):
                assert pos + s not in timeline[c]  # ... time ascending, nothing twice
                timeline[c][pos + s] = payload[s * sb:(s + 1) * sb]
    assert (n_flush > 0) == (B % F != 0)  # where F divides B nothing is ever carried
    for c in range(n_ch):
        listed = [k for k, s in enumerate(steps) if c in s["channels"].tolist()] if src["stream"][c] else []
        want = {}
        for k in listed:
            row = steps[k]["audio"][steps[k]["channels"].tolist().index(c)]
            wire = row.astype(">i2").tobytes() if sb == 2 else row.tobytes()
            for s in range(B):
                want[k * B + s] = wire[s * sb:(s + 1) * sb]
        sent = dict(timeline[c])
        # what the last step still carries has not been sent yet
        carried = int(wants[-1][3]["carry"][c])
        for s in range(carried):
            del want[listed[-1] * B + B - carried + s]
        assert sent == want, "channel %d" % c
        starts = [k * B for k in listed if k - 1 not in listed]
        assert markers[c] == starts, "channel %d: markers at %r, talkspurts start at %r" % (c, markers[c], starts)
    assert counters["packets"] == sum(w[0] for w in wants) and counters["dropped_packets"] == 0 and counters["steps"] == n_steps


def test_timestamp_and_seq_wrap_in_the_first_two_steps():
    src = np.zeros(1, capi.RTP_SOURCE_DTYPE)
    src[0] = (0xDEADBEEF, 0xFFFFFF00, 0xFFFE, 0, 1)
    model = capi.rtp_stream_reference(src, "ulaw", 1000, 160, 100)
    rows = np.arange(2000, dtype=np.uint8).reshape(2, 1000)
    _, r0, s0 = model.step([0], rows[:1])
    _, r1, s1 = model.step([0], rows[1:])
    assert r0["seq"].tolist() == [0xFFFE, 0xFFFF, 0, 1, 2, 3] and r1["seq"].tolist() == [4, 5, 6, 7, 8, 9]
    assert r0["timestamp"].tolist() == [(0xFFFFFF00 + 160 * j) & 0xFFFFFFFF for j in range(6)]
    assert r0["timestamp"][1] == 0xFFFFFFA0 and r0["timestamp"][2] == 0x40  # wrapped inside the first step
    assert r1["timestamp"].tolist() == [(0xFFFFFF00 + 960 + 160 * j) & 0xFFFFFFFF for j in range(6)]
    assert [rc.parse_packet(s0[j, :172])[2:5] for j in (1, 2)] == [(0xFFFF, 0xFFFFFFA0, 0xDEADBEEF), (0, 0x40, 0xDEADBEEF)]
    assert bytes(s0[0, :12]) == bytes([0x80, 0x80, 0xFF, 0xFE, 0xFF, 0xFF, 0xFF, 0x00, 0xDE, 0xAD, 0xBE, 0xEF])  # marker on the talkspurt's first packet
    assert bytes(s1[0, 12:52]) == rows[0, 960:].tobytes() and bytes(s1[0, 52:172]) == rows[1, :120].tobytes()  # the carry in front of the new row
    assert model.state()[0].tolist() == (12, 1920, 10, 80, 1)


@pytest.mark.parametrize("B,F,carries", [(1000, 160, [40, 80, 120, 0]), (2000, 320, [80, 160, 240, 0])])
def test_carry_cycle_worked_by_hand(B, F, carries):
    """1000 = 6 * 160 + 40: an ALWAYS channel's carry runs 40, 80, 120, 0 and it emits 6, 6, 6, 7 packets; the same cycle at 2000 / 320."""
    src = np.zeros(1, capi.RTP_SOURCE_DTYPE)
    src["stream"] = 1
    model = capi.rtp_stream_reference(src, "s16", B, F, 100)
    rows = np.arange(8 * B, dtype="<i2").reshape(8, B)
    seen, counts = [], []
    for k in range(8):
        count, records, slots = model.step([0], rows[k:k + 1])
        counts.append(count)
        seen.append(int(model.state()["carry"][0]))
        assert (records["flags"] == (np.arange(count) == 0) * (k == 0)).all() and (records["length"] == 12 + 2 * F).all()
    assert seen == carries * 2 and counts == [6, 6, 6, 7] * 2
    # L16 is network order; the last step's first packet is the carry of the row before followed by the head of its own
    first = struct.unpack(">%dh" % F, bytes(slots[0, 12:12 + 2 * F]))
    assert list(first) == rows[6, B - carries[2]:].tolist() + rows[7, :F - carries[2]].tolist()
    count, records, slots = model.step([], rows[:0])
    assert count == 0 and model.state()["flags"][0] == 0  # not listed, nothing carried: the talkspurt ends, nothing is emitted
