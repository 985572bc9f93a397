"""The band watch's kernels (csrc/band_watch.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles, ballots and barriers are rendezvous points) into a stand-alone program (tests/host_watch_harness.cpp) that
reads sequences of batches from a file and writes what the kernels left; compared byte for byte with the definition in plain Python
(capi.band_watch_reference).  It checks the LOGIC of the code the GPU runs -- the key minimum, the ballots, the event indices, the carried prefix sum of the
pack kernel -- tests/test_gpu_band_watch.py is what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs the fuzz's first seeds."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostbed
import watch_cases

capi = watch_cases.capi


@pytest.fixture(scope="module")
def hostwatch(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_watch", "host_watch_harness.cpp")


def _run_split(hostwatch, cases, name, pieces=8):
    """The cases in `pieces` files, one process each, side by side (the emulation switches fibers at every cross-lane operation: it is slow, and rows are independent)."""
    step = (len(cases) + pieces - 1) // pieces
    procs = []
    for i in range(0, len(cases), step):
        src, dst = os.path.join(hostwatch.dir, "%s%d.cases" % (name, i)), os.path.join(hostwatch.dir, "%s%d.results" % (name, i))
        open(src, "wb").write(watch_cases.encode(cases[i:i + step]))
        procs.append((subprocess.Popen([hostwatch.exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), dst))
    got = b""
    for proc, dst in procs:
        log, _ = proc.communicate()
        assert proc.returncode == 0, log[-4000:]
        got += open(dst, "rb").read()
    return got


def _compare(got, cases, sims):
    """The results file against the reference, case by case and batch by batch."""
    at = 0
    for n, ((p, batches), sim) in enumerate(zip(cases, sims)):
        for k, want in enumerate(watch_cases.expected_bytes(p, sim)):
            have = got[at:at + len(want)]
            if have != want:
                T, rows = p["T"], p["n_rows"]
                nt = 24 * T * rows
                what = "tracks" if have[:nt] != want[:nt] else "rows" if have[nt:nt + 16 * rows] != want[nt:nt + 16 * rows] else "events"
                raise AssertionError("case %d batch %d: %s differ (parameters %r)" % (n, k, what, {a: b for a, b in p.items() if a != "init"}))
            at += len(want)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


CONSTRUCTED = watch_cases.constructed()


@pytest.mark.parametrize("case", CONSTRUCTED, ids=[c[0] for c in CONSTRUCTED])
def test_constructed_sequences(hostwatch, case):
    name, p, batches, check = case
    sim = watch_cases.simulate(p, batches)
    check(sim)  # the property, on the reference's output
    got, _ = hostwatch.run(watch_cases.encode([(p, batches)]), name)
    _compare(got, [(p, batches)], [sim])


def test_constructed_sequences_with_two_sets(hostwatch):
    """The same sequences where the tables a batch starts from are the other set's, as on a pipelined handle: every entry of the set written to is written."""
    cases = [(dict(p, two_sets=1), batches) for _, p, batches, _ in CONSTRUCTED if p["C"] != 255]
    got, _ = hostwatch.run(watch_cases.encode(cases), "two_sets")
    _compare(got, cases, [watch_cases.simulate(p, b) for p, b in cases])


@pytest.fixture(scope="module")
def fuzz():
    cases = [watch_cases.wandering(seed) for seed in range(200)]
    return cases, [watch_cases.simulate(p, b) for p, b in cases]


def test_seeded_fuzz(hostwatch, fuzz):
    """200 seeds, 40 batches, 3 rows: random parameters, wandering carriers and strays, rows switched off now and then."""
    cases, sims = fuzz
    got = _run_split(hostwatch, cases, "fuzz")
    _compare(got, cases, sims)
    events = sum(s["n_events"] for sim in sims for s in sim)
    vanish = sum(int((s["events"]["kind"] == watch_cases.VANISH).sum()) for sim in sims for s in sim)
    dropped = sum(int(sim[-1]["rows"]["dropped"].sum()) for sim in sims)
    print("fuzz: %d events, %d of them VANISH, %d peaks dropped" % (events, vanish, dropped))
    assert events > 2000 and vanish > 500 and dropped > 100  # no rule went unexercised


def _pack_case(n_rows, counts, E, T=8, max_peaks=8):
    """The pack kernel alone: rows with `counts` staged events, every record distinct."""
    p = watch_cases.params(n_rows=n_rows, T=T, max_peaks=max_peaks, E=E, pack=2)
    staged = []
    for r, n in enumerate(counts):
        ev = np.zeros(n, capi.EVENT_DTYPE)
        ev["dev"], ev["bin"], ev["track"], ev["kind"], ev["batches"] = r, np.arange(n), np.arange(n), 1 + (r & 1), r % 65536
        ev["power"] = np.float32(r) + np.arange(n, dtype=np.float32) / 64
        staged.append(ev)
    blob = struct.pack("<13i", n_rows, 9, max_peaks, T, 2, 2, 2, E, 1, 0, 2, 0, 0) + np.arange(n_rows, dtype="<i4").tobytes()
    blob += np.array(counts, "<i4").tobytes() + b"".join(e.tobytes() for e in staged)
    return p, blob, np.concatenate(staged) if staged else np.zeros(0, capi.EVENT_DTYPE)


def _pack_shapes():
    rng = np.random.default_rng(4)
    shapes = []
    for n_rows in (1, 5, 1000, 1024, 1025, 2500):
        sparse = np.zeros(n_rows, int)
        sparse[rng.choice(n_rows, max(1, n_rows // 7), replace=False)] = rng.integers(1, 17, max(1, n_rows // 7))  # rows with none between rows with many
        total = int(sparse.sum())
        for E in sorted({1, max(1, total - 1), total, total + 1, 16 * n_rows} - {0}):
            if E <= 16 * n_rows:
                shapes.append((n_rows, sparse.tolist(), E))
        shapes.append((n_rows, [0] * n_rows, 3 if n_rows > 1 else 1))
        shapes.append((n_rows, [16] * n_rows, 16 * n_rows))
    return shapes


def test_pack_kernel(hostwatch):
    """Rows with no event between rows with many; n_events == E, E + 1, E - 1 and 0; 1 row, 1 000 rows, and counts on both sides of the chunk of 1 024 rows.
    The records arrive in row order, the count is exact, and nothing is written behind the records kept (the harness's guard zone)."""
    shapes = _pack_shapes()
    made = [_pack_case(*s) for s in shapes]
    blob = struct.pack("<i", len(made)) + b"".join(m[1] for m in made)
    got, _ = hostwatch.run(blob, "pack")
    at = 0
    for (n_rows, counts, E), (p, _, events) in zip(shapes, made):
        at += 24 * p["T"] * n_rows + 16 * n_rows  # tables and records: not the pack kernel's
        n = struct.unpack_from("<i", got, at)[0]
        at += 4
        assert n == sum(counts), (n_rows, E, n)
        kept = min(n, E)
        assert got[at:at + 16 * kept] == events[:kept].tobytes(), (n_rows, E)
        at += 16 * kept
    assert at == len(got)


def test_first_seeds_under_host_sanitizers(hostwatch, fuzz):
    """The stand-alone program built under ASan + UBSan on the fuzz's first seeds and a pack case: the same bytes, no report."""
    cases, sims = fuzz
    cases, sims = cases[:2], sims[:2]  # (seed 0 runs the pack kernel too)
    got, _ = hostwatch.sanitized().run(watch_cases.encode(cases), "san")
    _compare(got, cases, sims)
    p, blob, events = _pack_case(1025, [3] * 1025, 2000)
    got, _ = hostwatch.sanitized().run(struct.pack("<i", 1) + blob, "san_pack")
    assert got[-16 * 2000:] == events[:2000].tobytes()
