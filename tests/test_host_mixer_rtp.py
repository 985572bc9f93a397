"""The RTP stream's kernels (csrc/rtp_stream.hip) as the MIXER stream runs them, with their wavefront semantics on the CPU: the kernel source compiled for the
host through tests/hostshim_wave64/ into a stand-alone program (tests/host_mixer_rtp_harness.cpp) that runs a script of consecutive steps and flushes over rows
of wave_batch frames of W samples, with the state kept in the harness, and writes, per operation, the count, the records, the slots and every mixer's state;
compared byte for byte with the definition in plain Python (capi.rtp_stream_reference(width=W) and its flush()).  It checks the LOGIC of the code the GPU runs
-- frames against bytes in every pass, the ranks across wavefronts and workgroups, the flush step without a mask, the clamps -- tests/test_gpu_mixer_rtp.py is
what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes and the step with a damaged work list."""
import struct

import numpy as np
import pytest

import hostbed
import rtp_cases as rc

capi = rc.capi
FLUSH = dict(flush=True)


@pytest.fixture(scope="module")
def hostrtp(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_mixer_rtp", "host_mixer_rtp_harness.cpp")


def _script(src, encoding, W, B, F, max_packets, ops, max_rows=None, grid=2, damaged_last=False):
    n = len(src)
    blob = [struct.pack("<8i", n, n if max_rows is None else max_rows, B, rc.sample_bytes(encoding), W, F, max_packets, grid),
            np.ascontiguousarray(src, capi.RTP_SOURCE_DTYPE).tobytes()]
    for i, s in enumerate(ops):
        if s.get("flush"):
            blob.append(struct.pack("<i", 2))
            continue
        sel = np.zeros(n, np.uint8)
        sel[s["selected"]] = 1
        blob += [struct.pack("<i", 1 if damaged_last and i == len(ops) - 1 else 0), sel.tobytes(), np.ascontiguousarray(s["audio"]).tobytes()]
    return b"".join(blob)


def _reference(src, encoding, W, B, F, max_packets, ops):
    """([(count, records, slots, state)] per operation, counters, the model)"""
    model = capi.rtp_stream_reference(src, encoding, B, F, max_packets, width=W)
    out = []
    for s in ops:
        count, records, slots = model.flush() if s.get("flush") else model.step(s["channels"], s["audio"], s["dropped"])
        out.append((count, records, slots, model.state()))
    return out, model.counters(), model


def _ops(n, n_steps, seed, B, W, encoding, flush_after=(), **kw):
    """rc.schedule() with rows of W * B samples, and a flush behind each step in flush_after"""
    ops = []
    for k, s in enumerate(rc.schedule(n, n_steps, seed, B * W, encoding, **kw)):
        ops.append(s)
        if k in flush_after:
            ops.append(FLUSH)
    return ops


def _run(program, name, n, encoding, W, B, F, n_steps=9, max_rows=None, max_packets=None, unstreamed=(), seed=0, always=(0,), quiet_steps=(5,), flush_after=()):
    src = rc.sources(n, encoding, seed + 1, unstreamed)
    ops = _ops(n, n_steps, seed, B, W, encoding, flush_after, max_rows=max_rows, always=always, quiet_steps=quiet_steps)
    max_packets = n * ((F - 4 + B) // F) if max_packets is None else max_packets
    wants, counters, model = _reference(src, encoding, W, B, F, max_packets, ops)
    got, _ = program.run(_script(src, encoding, W, B, F, max_packets, ops, max_rows=max_rows), name)
    rc.compare_host(got, wants, counters, n, model.slot_bytes, max_packets, name)
    assert counters["steps"] == n_steps
    return wants, counters, ops


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("encoding", ["ulaw", "alaw", "s16"])
def test_mixer_counts_widths_and_encodings(hostrtp, n, W, encoding):
    """1 / 64 / 65 mixers (the write pass on a grid of two workgroups), mono and stereo, all three encodings, B = 1000, F = 160: an always-listed mixer walks
    the carry cycle in FRAMES, the others start and stop, step 5 lists nobody (every carry is flushed there)."""
    wants, counters, _ = _run(hostrtp, "enc_%d_%d_%s" % (n, W, encoding), n, encoding, W, 1000, 160, seed=n + W)
    flags = np.concatenate([w[1]["flags"] for w in wants])
    lengths = np.concatenate([w[1]["length"] for w in wants])
    assert (flags & capi.RTP_MARKER).any() and (flags & capi.RTP_FLUSH).any()
    assert [int(w[3]["carry"][0]) for w in wants[:4]] == [40, 80, 120, 0]
    assert set(lengths[flags & capi.RTP_FLUSH == 0].tolist()) == {12 + 160 * W * rc.sample_bytes(encoding)}
    assert counters["dropped_packets"] == 0 and counters["lost_rows"] == 0


@pytest.mark.parametrize("W,encoding,B,F", [(2, "ulaw", 1000, 40), (1, "alaw", 1000, 40), (2, "s16", 1000, 160), (2, "alaw", 2000, 320), (1, "s16", 2000, 320),
                                             (2, "s16", 2000, 364), (2, "ulaw", 2000, 728)])
def test_batch_and_frame_lengths(hostrtp, W, encoding, B, F):
    """(B, F) = (1000, 40): never a carry; (1000, 160) and (2000, 320): the four-step cycle; (2000, 364): the longest S16 stereo frame, 12 + 1456 bytes, whose
    carry runs through multiples of gcd = 4 frames; (2000, 728): the longest G.711 stereo frame."""
    wants, _, _ = _run(hostrtp, "bf_%d_%s_%d_%d" % (W, encoding, B, F), 65, encoding, W, B, F, n_steps=6, seed=B + F + W, quiet_steps=(3,))
    if B % F == 0:
        assert all((w[3]["carry"] == 0).all() for w in wants)
    else:
        assert any((w[3]["carry"] != 0).any() for w in wants)
    if F == 364:
        assert [int(w[3]["carry"][0]) for w in wants[:3]] == [180, 360, 176] and wants[0][1]["length"].max() == 1468


def test_stereo_limits_are_refused_past_the_packet():
    for enc, F in (("s16", 368), ("ulaw", 732)):
        with pytest.raises(ValueError):
            capi.rtp_stream_reference(rc.sources(1, enc, 0), enc, 2000, F, 1, width=2)


def test_rows_beyond_max_rows_are_lost_and_flushed(hostrtp):
    """130 stereo mixers and a list of 20 rows: mixers selected but dropped past max_rows count as lost_rows, and a dropped mixer's carry is flushed."""
    wants, counters, _ = _run(hostrtp, "max_rows", 130, "alaw", 2, 1000, 160, n_steps=10, max_rows=20, seed=11, always=(0, 129), quiet_steps=())
    assert counters["lost_rows"] > 0
    flags = np.concatenate([w[1]["flags"] for w in wants])
    assert (flags & capi.RTP_FLUSH).any()
    assert all(w[3]["packets"][129] == 0 for w in wants)  # always selected, never listed


def test_packets_beyond_max_packets(hostrtp):
    """fewer slots than packets: the guard slots behind the buffers stay untouched (the harness checks them after every operation) and seq still advances."""
    wants, counters, _ = _run(hostrtp, "max_packets", 65, "s16", 2, 1000, 160, max_packets=17, seed=5)
    assert counters["dropped_packets"] > 0
    assert any(w[0] > 17 for w in wants)
    last = wants[-1][3]
    assert int(last["packets"].sum()) == counters["packets"] > sum(len(w[1]) for w in wants)


def test_unstreamed_mixers_inside_the_list(hostrtp):
    wants, _, _ = _run(hostrtp, "unstreamed", 70, "ulaw", 2, 1000, 160, unstreamed=(0, 3, 64, 65), seed=9, always=(0, 1, 64))
    for w in wants:
        assert not np.isin(w[1]["channel"], (0, 3, 64, 65)).any()
        assert w[3][[0, 3, 64, 65]].tobytes() == bytes(64)


def test_more_than_one_workgroup(hostrtp):
    """2 100 mixers are three workgroups of the per-mixer passes: ranks and prefix sums cross workgroup boundaries; a flush behind step 1 crosses them too."""
    wants, _, ops = _run(hostrtp, "blocks", 2100, "ulaw", 2, 1000, 160, n_steps=4, seed=2, always=(0, 1023, 1024, 2099), quiet_steps=(), flush_after=(1,))
    at = next(i for i, s in enumerate(ops) if s.get("flush"))
    flushed = wants[at][1]["channel"]
    assert {0, 1023, 1024, 2099} <= set(flushed.tolist()) and flushed.max() > 2048 and flushed.min() < 1024


def test_flush_after_a_step_with_carries_and_flush_with_none(hostrtp):
    """A flush behind step 0 (every listed mixer carries 40 frames): one short packet each with timestamp ts0 + 1 * B - 40, length 12 + 40 * FB, no step counted,
    every mixer silent and empty afterwards; a second flush right behind it emits nothing; the step after starts new talkspurts at k = 1.  And a flush behind a
    step that left no carry (step 3 of the cycle for the always-listed mixer, everyone else quiet)."""
    n, enc, W, B, F = 65, "s16", 2, 1000, 160
    src = rc.sources(n, enc, 41)
    steps = rc.schedule(n, 5, 40, B * W, enc, always=(0,), quiet_steps=())
    ops = [steps[0], FLUSH, FLUSH] + steps[1:]
    wants, counters, model = _reference(src, enc, W, B, F, 1000, ops)
    got, _ = hostrtp.run(_script(src, enc, W, B, F, 1000, ops), "flushes")
    rc.compare_host(got, wants, counters, n, model.slot_bytes, 1000, "flushes")
    listed0 = steps[0]["channels"]
    count, records, _, state = wants[1]
    assert count == len(listed0) > 1 and records["channel"].tolist() == listed0.tolist()
    assert (records["length"] == 12 + 40 * 4).all() and (records["flags"] == capi.RTP_FLUSH).all()
    assert records["timestamp"].tolist() == [(int(src["ts0"][m]) + B - 40) & 0xFFFFFFFF for m in listed0]
    assert not state["carry"].any() and not state["flags"].any()
    assert wants[2][0] == 0 and wants[2][3].tobytes() == state.tobytes()
    first = wants[3][1][wants[3][1]["channel"] == 0][0]
    assert first["flags"] == capi.RTP_MARKER and first["timestamp"] == (int(src["ts0"][0]) + B) & 0xFFFFFFFF
    assert counters["steps"] == 5
    # no carry anywhere: four steps of one always-listed mixer, then the flush
    one = rc.sources(3, "ulaw", 43)
    steps = rc.schedule(3, 4, 44, B * W, "ulaw", p_start=0.0, always=(1,), quiet_steps=())
    ops = steps + [FLUSH]
    wants, counters, model = _reference(one, "ulaw", W, B, F, 50, ops)
    got, _ = hostrtp.run(_script(one, "ulaw", W, B, F, 50, ops), "flush_none")
    rc.compare_host(got, wants, counters, 3, model.slot_bytes, 50, "flush_none")
    assert wants[3][3]["carry"].tolist() == [0, 0, 0] and wants[4][0] == 0 and wants[4][3]["flags"].tolist() == [0, 0, 0] and wants[3][3]["flags"][1] == 1


def test_two_shapes_and_a_damaged_work_list_under_host_sanitizers(hostrtp):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report; then a step whose work list names mixers, rows and slots far out of range
    (and a carry length beyond the buffer): they are clamped, not followed."""
    san = hostrtp.sanitized()
    _run(san, "san_ulaw", 65, "ulaw", 2, 1000, 160, max_packets=40, seed=21, flush_after=(2,))
    _run(san, "san_s16", 130, "s16", 2, 2000, 364, n_steps=6, max_rows=50, seed=22, quiet_steps=(3,), flush_after=(5,))
    src = rc.sources(65, "s16", 5)
    ops = rc.schedule(65, 3, 5, 2000, "s16", always=(0, 64), quiet_steps=())
    got, _ = san.run(_script(src, "s16", 2, 1000, 160, 30, ops, damaged_last=True), "san_damaged")
    wants, _, model = _reference(src, "s16", 2, 1000, 160, 30, ops[:2])
    at = 0
    for want in wants:  # the steps in front of the damaged one are whole
        kept = min(want[0], 30)
        at += 4 + 16 * kept + model.slot_bytes * kept + 16 * 65
    assert len(got) == at + 32
