"""Shared by the RTP packet stream's tests: random schedules of listed / unlisted batches with rows an encoder could have left, a driver that steps
capi.rtp_stream_reference() through them, an independent parser of packets (struct.unpack(">BBHII")), and for the CPU test the script that
tests/host_rtp_harness.cpp runs and the comparison of what it wrote with the reference."""
import importlib
import struct

import numpy as np

capi = importlib.import_module("rtlsdr-airband_amd").capi

REC = np.dtype(capi.RTP_PACKET_DTYPE)
STATE = np.dtype(capi.RTP_STATE_DTYPE)


def sample_bytes(encoding):
    return 2 if capi.audio_encoding_value(encoding) == capi.AUDIO_S16 else 1


def sources(n_ch, encoding, seed, unstreamed=()):
    """[n_ch] of RTP_SOURCE_DTYPE: random ssrc, ts0 and seq0, the encoding's payload type, every channel streamed but `unstreamed`."""
    rng = np.random.default_rng(seed)
    src = np.zeros(n_ch, capi.RTP_SOURCE_DTYPE)
    src["ssrc"] = rng.integers(0, 2**32, n_ch, dtype=np.uint64)
    src["ts0"] = rng.integers(0, 2**32, n_ch, dtype=np.uint64)
    src["seq0"] = rng.integers(0, 2**16, n_ch)
    src["payload_type"] = capi.RTP_PAYLOAD_TYPES[capi.audio_encoding_value(encoding)]
    src["stream"] = 1
    src["stream"][list(unstreamed)] = 0
    return src


def schedule(n_ch, n_steps, seed, wave_batch, encoding, max_rows=None, p_start=0.25, p_stop=0.35, always=(), quiet_steps=()):
    """n_steps batches over n_ch channels: transmissions start and stop at random, the channels in `always` are selected in every batch, nobody in
    `quiet_steps`.  steps[k] = dict(selected: ascending channels, channels: the first max_rows of them, dropped: the rest, audio [n][wave_batch] int16 or
    uint8, random)."""
    rng = np.random.default_rng(seed)
    max_rows = n_ch if max_rows is None else max_rows
    on = np.zeros(n_ch, bool)
    steps = []
    for k in range(n_steps):
        flip = rng.random(n_ch)
        on = np.where(on, flip >= p_stop, flip < p_start)
        sel = on.copy()
        sel[list(always)] = True
        if k in quiet_steps:
            sel[:] = False
        selected = np.flatnonzero(sel).astype(np.int32)
        channels = selected[:max_rows]
        if sample_bytes(encoding) == 2:
            audio = rng.integers(-32767, 32768, (len(channels), wave_batch)).astype("<i2")
        else:
            audio = rng.integers(0, 256, (len(channels), wave_batch), dtype=np.uint8)
        steps.append(dict(selected=selected, channels=channels, dropped=selected[max_rows:], audio=audio))
    return steps


def run_reference(src, encoding, wave_batch, frame_samples, max_packets, steps):
    """the reference stepped through `steps`: ([(count, records, slots, state)], counters, the model)"""
    model = capi.rtp_stream_reference(src, encoding, wave_batch, frame_samples, max_packets)
    out = []
    for s in steps:
        count, records, slots = model.step(s["channels"], s["audio"], s["dropped"])
        out.append((count, records, slots, model.state()))
    return out, model.counters(), model


def parse_packet(data):
    """The independent parser: (marker, payload_type, seq, timestamp, ssrc, payload) of one packet's bytes."""
    b0, b1, seq, ts, ssrc = struct.unpack(">BBHII", bytes(data[:12]))
    assert b0 == 0x80  # version 2, no padding, no extension, no CSRC
    return b1 >> 7, b1 & 0x7F, seq, ts, ssrc, bytes(data[12:])


def script(src, encoding, wave_batch, frame_samples, max_packets, steps, max_rows=None, grid=2, damaged_last=False):
    """the harness's input for the same run; damaged_last: the last step runs with a damaged work list (and writes no results)"""
    n_ch = len(src)
    blob = [struct.pack("<7i", n_ch, n_ch if max_rows is None else max_rows, wave_batch, sample_bytes(encoding), frame_samples, max_packets, grid),
            np.ascontiguousarray(src, capi.RTP_SOURCE_DTYPE).tobytes()]
    for i, s in enumerate(steps):
        sel = np.zeros(n_ch, np.uint8)
        sel[s["selected"]] = 1
        blob += [struct.pack("<i", 1 if damaged_last and i == len(steps) - 1 else 0), sel.tobytes(), np.ascontiguousarray(s["audio"]).tobytes()]
    return b"".join(blob)


def compare_packets(label, count, records, slots, want, poison=None):
    """one step's count, records and slots against the reference's (count, records, slots, ...): every packet, every defined byte; poison: the byte the caller
    filled the slots with, which the bytes behind `length` must still hold"""
    w_count, w_records, w_slots = want[0], want[1], want[2]
    assert count == w_count, "%s: %d packets, the reference has %d" % (label, count, w_count)
    assert len(records) == len(w_records), label
    assert records.tobytes() == w_records.tobytes(), "%s: records differ, first at %r" % (label, next(i for i in range(len(records)) if records[i] != w_records[i]))
    for i in range(len(records)):
        n = int(records[i]["length"])
        assert slots[i, :n].tobytes() == w_slots[i, :n].tobytes(), "%s: packet %d (channel %d) differs" % (label, i, records[i]["channel"])
        if poison is not None:
            assert (slots[i, n:] == poison).all(), "%s: packet %d: bytes behind its length were written" % (label, i)


def compare_host(got, wants, counters, n_ch, slot_bytes, max_packets, label):
    """the harness's results file against run_reference()'s"""
    at = 0
    for k, want in enumerate(wants):
        (count,) = struct.unpack("<i", got[at:at + 4])
        at += 4
        n = min(count, max_packets)
        records = np.frombuffer(got[at:at + 16 * n], REC)
        at += 16 * n
        slots = np.frombuffer(got[at:at + slot_bytes * n], np.uint8).reshape(n, slot_bytes)
        at += slot_bytes * n
        state = np.frombuffer(got[at:at + 16 * n_ch], STATE)
        at += 16 * n_ch
        compare_packets("%s, step %d" % (label, k), count, records, slots, want, poison=0xEE)
        assert state.tobytes() == want[3].tobytes(), "%s, step %d: state differs at channels %r" % (label, k, np.flatnonzero(state != want[3])[:8])
    got_counters = struct.unpack("<4Q", got[at:at + 32])
    assert at + 32 == len(got), label
    assert got_counters == (counters["packets"], counters["dropped_packets"], counters["octets"], counters["lost_rows"]), label
