"""The RTP packet stream's kernels (csrc/rtp_stream.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; ballots, shuffles and barriers are rendezvous points) into a stand-alone program (tests/host_rtp_harness.cpp) that runs
a script of consecutive steps with the state kept in the harness and writes, per step, the count, the records, the slots and every channel's state; compared byte
for byte with the definition in plain Python (capi.rtp_stream_reference).  It checks the LOGIC of the code the GPU runs -- the ranks across wavefronts and
workgroups, the prefix sums, the carry, the headers, the clamps -- tests/test_gpu_rtp_stream.py is what a GPU says.  The same program built under ASan + UBSan
(tests/hostbed.py) runs two of the shapes and the step with a damaged work list."""
import numpy as np
import pytest

import hostbed
import rtp_cases as rc

capi = rc.capi


@pytest.fixture(scope="module")
def hostrtp(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_rtp", "host_rtp_harness.cpp")


def _run(program, name, n_ch, encoding, B, F, n_steps=9, max_rows=None, max_packets=None, unstreamed=(), seed=0, always=(0,), quiet_steps=(5,)):
    src = rc.sources(n_ch, encoding, seed + 1, unstreamed)
    steps = rc.schedule(n_ch, n_steps, seed, B, encoding, max_rows=max_rows, always=always, quiet_steps=quiet_steps)
    max_packets = n_ch * ((F - 4 + B) // F) if max_packets is None else max_packets
    wants, counters, model = rc.run_reference(src, encoding, B, F, max_packets, steps)
    blob = rc.script(src, encoding, B, F, max_packets, steps, max_rows=max_rows)
    got, _ = program.run(blob, name)
    rc.compare_host(got, wants, counters, n_ch, model.slot_bytes, max_packets, name)
    return wants, counters


@pytest.mark.parametrize("n_ch", [1, 64, 65])
@pytest.mark.parametrize("encoding", ["ulaw", "alaw", "s16"])
def test_channel_counts_and_encodings(hostrtp, n_ch, encoding):
    """1 / 64 / 65 channels (the write pass on a grid of two workgroups), all three encodings, B = 1000, F = 160: an always-listed channel walks the carry cycle,
    the others start and stop, step 5 lists nobody (every carry is flushed there)."""
    wants, counters = _run(hostrtp, "enc_%d_%s" % (n_ch, encoding), n_ch, encoding, 1000, 160, seed=n_ch)
    flags = np.concatenate([w[1]["flags"] for w in wants])
    assert (flags & capi.RTP_MARKER).any() and (flags & capi.RTP_FLUSH).any()
    assert [int(w[3]["carry"][0]) for w in wants[:4]] == [40, 80, 120, 0]
    assert counters["dropped_packets"] == 0 and counters["lost_rows"] == 0


@pytest.mark.parametrize("B,F", [(1000, 40), (1000, 1000), (2000, 40), (2000, 160), (2000, 320), (2000, 2000)])
def test_batch_and_frame_lengths(hostrtp, B, F):
    """B in 1000 and 2000, F = 40, 160 and B (mu-law: 12 + 2000 bytes exceed a packet for nothing else).  With F = B, and with F = 40, there is never a carry."""
    enc = "ulaw" if 12 + F <= 1472 else None
    if enc is None:
        # F = B = 2000 does not fit a packet in any encoding: the frame check refuses it, for the reference as for the handle
        with pytest.raises(ValueError):
            capi.rtp_stream_reference(rc.sources(1, "ulaw", 0), "ulaw", B, F, 1)
        return
    wants, _ = _run(hostrtp, "bf_%d_%d" % (B, F), 65, enc, B, F, n_steps=6, seed=B + F, quiet_steps=(3,))
    if B % F == 0:
        assert all((w[3]["carry"] == 0).all() for w in wants)
    else:
        assert any((w[3]["carry"] != 0).any() for w in wants)


def test_s16_frames_up_to_the_packet_limit(hostrtp):
    """S16 at F = 728, the longest frame of two-byte samples (12 + 1456 <= 1472), B = 2000"""
    _run(hostrtp, "s16_728", 65, "s16", 2000, 728, n_steps=6, seed=3, quiet_steps=(3,))


def test_rows_beyond_max_rows_are_lost_and_flushed(hostrtp):
    """130 channels and a list of 20 rows: channels selected but dropped past max_rows count as lost_rows, and a dropped channel's carry is flushed."""
    wants, counters = _run(hostrtp, "max_rows", 130, "alaw", 1000, 160, n_steps=10, max_rows=20, seed=11, always=(0, 129), quiet_steps=())
    assert counters["lost_rows"] > 0
    flags = np.concatenate([w[1]["flags"] for w in wants])
    assert (flags & capi.RTP_FLUSH).any()
    assert all(w[3]["packets"][129] == 0 for w in wants)  # always selected, never listed


def test_packets_beyond_max_packets(hostrtp):
    """fewer slots than packets: the guard slots behind the buffers stay untouched (the harness checks them after every step) and seq still advances."""
    wants, counters = _run(hostrtp, "max_packets", 65, "ulaw", 1000, 160, max_packets=17, seed=5)
    assert counters["dropped_packets"] > 0
    assert any(w[0] > 17 for w in wants)
    last = wants[-1][3]
    assert int(last["packets"].sum()) == counters["packets"] > sum(len(w[1]) for w in wants)


def test_unstreamed_channels_inside_the_list(hostrtp):
    wants, _ = _run(hostrtp, "unstreamed", 70, "ulaw", 1000, 160, unstreamed=(0, 3, 64, 65), seed=9, always=(0, 1, 64))
    for w in wants:
        assert not np.isin(w[1]["channel"], (0, 3, 64, 65)).any()
        assert w[3][[0, 3, 64, 65]].tobytes() == bytes(64)


def test_more_than_one_workgroup(hostrtp):
    """2 100 channels are three workgroups of the per-channel passes: ranks and prefix sums cross workgroup boundaries."""
    _run(hostrtp, "blocks", 2100, "ulaw", 1000, 160, n_steps=5, seed=2, always=(0, 1023, 1024, 2099), quiet_steps=(3,))


def test_two_shapes_and_a_damaged_work_list_under_host_sanitizers(hostrtp):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report; then a step whose work list names channels, rows and slots far out of range
    (and a carry length beyond the buffer): they are clamped, not followed."""
    san = hostrtp.sanitized()
    _run(san, "san_ulaw", 65, "ulaw", 1000, 160, max_packets=40, seed=21)
    _run(san, "san_s16", 130, "s16", 2000, 320, n_steps=6, max_rows=50, seed=22, quiet_steps=(3,))
    src = rc.sources(65, "s16", 5)
    steps = rc.schedule(65, 3, 5, 1000, "s16", always=(0, 64), quiet_steps=())
    blob = rc.script(src, "s16", 1000, 160, 30, steps, damaged_last=True)
    got, _ = san.run(blob, "san_damaged")
    wants, _, model = rc.run_reference(src, "s16", 1000, 160, 30, steps[:2])
    at = 0
    for want in wants:  # the steps in front of the damaged one are whole
        n = min(want[0], 30)
        at += 4 + 16 * n + model.slot_bytes * n + 16 * 65
    assert len(got) == at + 32
