"""The spool kernels (csrc/tx_spool.hip) on MIXER-shaped input, with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ into a stand-alone program (tests/host_spool_harness.cpp, in its mixer mode) that fills SpoolArgs the way the driver does for a mixer spool -- the
mixer count, the mixer gate's verdicts from gate bytes and has_signal flags, rows of W * B samples (1 000 .. 8 000 bytes), records whose stereo flags change from
step to step, wave_batch = B frames -- and runs a script of steps, flushes and collects.  What the collects returned is compared byte for byte, records and
audio and the counters, with capi.transmission_spool_reference() fed the same steps (`selected` from has_signal by the gate's rule: capi.mixer_gate_selection).
tests/test_gpu_mixer_spool.py is what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes, directly."""
import numpy as np
import pytest

import hostbed
import spool_cases as sc

capi = sc.capi
NEVER, SIGNAL, ALWAYS = capi.GATE_NEVER, capi.GATE_SIGNAL, capi.GATE_ALWAYS
FRAMES = {1000: 1000, 2000: 2000, 4000: 2000, 8000: 2000}  # row bytes -> B: (W 1, ulaw, 8000), (W 1, ulaw, 16000), (W 2, ulaw, 16000), (W 2, s16, 16000)


@pytest.fixture(scope="module")
def hostspool(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_mixer_spool", "host_spool_harness.cpp")


def schedule(n_mix, n_steps, seed, max_rows, row_bytes, p_start=0.12, p_stop=0.35):
    """gate bytes (mostly SIGNAL, some ALWAYS and NEVER), the spool mask (two of three SIGNAL mixers), and per step has_signal, the gate's whole selection, its
    list, the listed rows (bytes that name step and mixer) and records with a stereo flag that changes from step to step"""
    rng = np.random.default_rng(seed)
    frames = FRAMES[row_bytes]
    gate = np.full(n_mix, SIGNAL, np.uint8)
    if n_mix > 2:
        gate[2::7] = ALWAYS
        gate[5::11] = NEVER
    mask = (gate == SIGNAL).astype(np.uint8)
    if n_mix > 1:
        mask[1::3] = 0  # mixers the gate selects and the spool ignores
    gate[-1], mask[-1] = SIGNAL, 1  # the last mixer is spooled and talks early (of 1 025 it is the second workgroup's only one)
    sel =capi.mixer_gate_selection(gate)
    on = np.zeros(n_mix, bool)
    steps = []
    for k in range(n_steps):
        flip = rng.random(n_mix)
        on = np.where(on, flip >= p_stop, flip < p_start)
        if k in (1, 2):
            on[-1] = True
        if k >= n_steps - 4:
            on[:] = False  # a quiet tail: the idle rule gets its turn
        selected = sel.step(on)
        mixers = selected[:max_rows]
        n = len(mixers)
        audio = rng.integers(0, 256, (n, row_bytes), dtype=np.uint8)
        info = np.zeros(n, capi.AUDIO_ROW_DTYPE)
        if n:
            audio[:, 0], audio[:, 1], audio[:, -1] = k & 0xFF, mixers & 0xFF, (mixers >> 8) & 0xFF
            info["channel"] = mixers
            info["peak"] = rng.integers(0, 32768, n)
            info["n_clipped"] = rng.integers(0, 3, n) * rng.integers(0, 2001, n)
            info["first"] = rng.integers(0, frames + 1, n)
            info["end"] = rng.integers(0, frames + 1, n)
            info["reserved"] = rng.integers(0, 2, n)  # the stereo flag at this step
        steps.append(dict(signal=on.astype(np.uint8), selected=selected, mixers=mixers, audio=audio, info=info))
    return gate, mask, steps


def _script(gate, mask, steps, ops, max_rows, row_bytes, **p):
    return sc.script(mask, steps, ops, max_rows, row_bytes, FRAMES[row_bytes], gate=gate, **p)


SHAPES = [
    # n_mixers, row_bytes, pool_rows, max_records, max_batches, max_rows, steps: room for everything, at the wavefront edge and in a second workgroup ...
    (1, 1000, 40, 8, 6, None, 36), (63, 2000, 400, 200, 6, None, 36), (64, 4000, 400, 200, 6, None, 36), (65, 8000, 400, 200, 6, None, 36),
    (1025, 1000, 3000, 1200, 4, None, 16),
    # ... a pool that runs dry, a full finished list, both, and a gate whose max_rows is below its count
    (65, 1000, 3, 200, 6, None, 36), (64, 2000, 400, 1, 6, None, 36), (63, 8000, 3, 1, 4, None, 36),
    (65, 4000, 60, 200, 6, 5, 36), (1025, 8000, 50, 7, 3, 40, 14),
]


@pytest.mark.parametrize("n_mix,row_bytes,pool_rows,max_records,max_batches,max_rows,n_steps", SHAPES)
def test_random_mixer_schedules_equal_the_model(hostspool, n_mix, row_bytes, pool_rows, max_records, max_batches, max_rows, n_steps):
    """export_rows == max_batches + 1 throughout, collects and a flush in mid-run; every run must contain what its shape is for"""
    big = n_mix > 1000
    gate, mask, steps = schedule(n_mix, n_steps, seed=n_mix * 7 + pool_rows + max_records + row_bytes, max_rows=max_rows or n_mix, row_bytes=row_bytes,
                                 p_start=0.05 if big else 0.12, p_stop=0.3 if big else 0.35)
    ops = {4: "c", 7: "cc", 10: "fc"} if big else {9: "c", 14: "cc", 20: "fc", 27: "c"}
    blob, want, model = _script(gate, mask, steps, ops, max_rows or n_mix, row_bytes, pool_rows=pool_rows, export_rows=max_batches + 1, max_records=max_records,
                                min_batches=3 if not big else 2, idle_batches=1, max_batches=max_batches)
    cn = model.counters()
    collects, _ = sc.collects(want, row_bytes)
    recs = np.concatenate([c[0] for c in collects])
    assert cn["finished_total"] > 0 and cn["rows_stored_total"] > 0 and len(recs) == cn["finished_total"]
    assert all(mask[m] for m in recs["channel"]) and (recs["reserved"][:, 0] == 0).all()
    if n_mix > 1 and pool_rows > 3:
        assert set(recs["reserved"][:, 1].tolist()) == {0, 1}, "the run holds no clip with and no clip without a stereo flag"
    seen = {}
    for s in steps:
        for m, f in zip(s["mixers"].tolist(), s["info"]["reserved"].tolist()):
            seen.setdefault(m, set()).add(f)
    assert any(len(v) == 2 for v in seen.values()), "no mixer's flag changes from step to step"
    if pool_rows == 3 or max_rows:
        assert cn["rows_lost_total"] > 0
    if max_records == 1 and n_mix > 1:
        assert cn["dropped_transmissions"] > 0
    if max_rows:
        assert any(len(s["selected"]) > max_rows for s in steps)
    if big and not max_rows:  # (with a list of seven records and 40 rows its clip is among the dropped ones)
        assert recs["channel"].max() >= 1024, "no clip of the second workgroup's mixer"
    got, _ = hostspool.run(blob, "random_%d_%d_%d_%d" % (n_mix, row_bytes, pool_rows, max_records))
    sc.compare(got, want, row_bytes, "%d mixers, rows of %d bytes, pool %d, list %d" % (n_mix, row_bytes, pool_rows, max_records))


def test_two_shapes_under_host_sanitizers(hostspool):
    """The stand-alone program built under ASan + UBSan and run directly: the same bytes, no report."""
    for n_mix, row_bytes, pool_rows, max_records, max_batches, max_rows, n_steps in (SHAPES[7], SHAPES[8]):
        gate, mask, steps = schedule(n_mix, 24, seed=n_mix + pool_rows, max_rows=max_rows or n_mix, row_bytes=row_bytes)
        blob, want, _ = _script(gate, mask, steps, {8: "c", 15: "fc"}, max_rows or n_mix, row_bytes, pool_rows=pool_rows, export_rows=max_batches + 1,
                                max_records=max_records, min_batches=3, idle_batches=1, max_batches=max_batches)
        got, _ = hostspool.sanitized().run(blob, "san_%d" % n_mix)
        sc.compare(got, want, row_bytes, "sanitized, %d mixers" % n_mix)
