"""The transmission spool's kernels (csrc/tx_spool.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; ballots, shuffles and barriers are rendezvous points) into a stand-alone program (tests/host_spool_harness.cpp, in its channel mode) that
reads a script of steps, flushes and collects from a file and writes what the collects returned; compared byte for byte, records and audio and the counters,
with the definition in plain Python (capi.transmission_spool_reference) on random selection schedules.  It checks the LOGIC of the code the GPU runs -- the
verdicts, the ranks across wavefronts and workgroups, the chains and the free stack, the ring of finished records, the prefix of the collect, the clamps --
tests/test_gpu_transmission_spool.py is what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import struct

import numpy as np
import pytest

import hostbed
import spool_cases as sc

capi = sc.capi
ROW_BYTES, B = 16, 16


@pytest.fixture(scope="module")
def hostspool(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_spool", "host_spool_harness.cpp")


def _script(mask, steps, ops, max_rows, row_bytes, **p):
    return sc.script(mask, steps, ops, max_rows, row_bytes, B, **p)


SHAPES = [
    # n_ch, pool_rows, max_records, max_batches, max_rows, row_bytes: room for everything ...
    (1, 40, 8, 6, None, 16), (63, 400, 200, 6, None, 16), (64, 400, 200, 6, None, 12), (65, 400, 200, 6, None, 16), (130, 900, 400, 6, None, 16),
    # ... a pool of three rows, a list of one record, both, and a gate that lists fewer rows than it selects
    (63, 3, 200, 6, None, 16), (65, 3, 200, 4, None, 12), (130, 3, 400, 6, None, 16),
    (64, 400, 1, 6, None, 16), (130, 900, 1, 6, None, 16), (65, 3, 1, 6, None, 16),
    (65, 60, 200, 6, 5, 16), (130, 50, 7, 3, 40, 12),
]


@pytest.mark.parametrize("n_ch,pool_rows,max_records,max_batches,max_rows,row_bytes", SHAPES)
def test_random_schedules_equal_the_model(hostspool, n_ch, pool_rows, max_records, max_batches, max_rows, row_bytes):
    """export_rows == max_batches + 1 throughout: a collect takes few transmissions, so every run collects many times; collects and a flush in mid-run too."""
    mask, steps = sc.schedule(n_ch, 36, seed=n_ch * 7 + pool_rows + max_records, max_rows=max_rows, row_bytes=row_bytes, wave_batch=B)
    ops = {9: "c", 14: "cc", 20: "fc", 27: "c"}
    blob, want, model = _script(mask, steps, ops, max_rows or n_ch, row_bytes, pool_rows=pool_rows, export_rows=max_batches + 1, max_records=max_records,
                                min_batches=3, idle_batches=1, max_batches=max_batches)
    cn = model.counters()
    # the run contained what its shape is for
    assert cn["finished_total"] > 0 and cn["rows_stored_total"] > 0
    if pool_rows == 3 or max_rows:
        assert cn["rows_lost_total"] > 0
    if max_records == 1 and n_ch > 1:
        assert cn["dropped_transmissions"] > 0
    got, _ = hostspool.run(blob, "random_%d_%d_%d_%d" % (n_ch, pool_rows, max_records, max_batches))
    sc.compare(got, want, row_bytes, "%d channels, pool %d, list %d" % (n_ch, pool_rows, max_records))


def test_every_reason_and_more_than_one_workgroup(hostspool):
    """2 100 channels are three workgroups of the per-channel passes: ranks cross workgroup boundaries; the schedule ends transmissions by IDLE, MAX and FLUSH."""
    mask, steps = sc.schedule(2100, 14, seed=5, p_start=0.05, p_stop=0.2, wave_batch=B)
    steps = steps[:11]  # no quiet tail: the final flush finds open transmissions
    blob, want, model = _script(mask, steps, {6: "c"}, 2100, ROW_BYTES, pool_rows=3000, export_rows=4000, max_records=3000, min_batches=2, idle_batches=1, max_batches=3)
    reasons = set()
    at = 0
    while at + 12 <= len(want) - 64:
        n, rows, _ = struct.unpack("<3i", want[at:at + 12])
        reasons |= set(np.frombuffer(want[at + 12:at + 12 + 48 * n], sc.REC)["reason"].tolist())
        at += 12 + 48 * n + ROW_BYTES * rows
    assert reasons == {capi.SPOOL_IDLE, capi.SPOOL_MAX, capi.SPOOL_FLUSH}
    got, _ = hostspool.run(blob, "blocks")
    sc.compare(got, want, ROW_BYTES, "2100 channels")


def test_two_shapes_under_host_sanitizers(hostspool):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    for n_ch, pool_rows, max_records, max_batches, max_rows, row_bytes in (SHAPES[7], SHAPES[12]):
        mask, steps = sc.schedule(n_ch, 24, seed=n_ch + pool_rows, max_rows=max_rows, row_bytes=row_bytes, wave_batch=B)
        blob, want, _ = _script(mask, steps, {8: "c", 15: "fc"}, max_rows or n_ch, row_bytes, pool_rows=pool_rows, export_rows=max_batches + 1, max_records=max_records,
                                min_batches=3, idle_batches=1, max_batches=max_batches)
        got, _ = hostspool.sanitized().run(blob, "san_%d" % n_ch)
        sc.compare(got, want, row_bytes, "sanitized, %d channels" % n_ch)
