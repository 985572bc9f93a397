"""The transmission spool's kernels (csrc/tx_spool.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; ballots, shuffles and barriers are rendezvous points) into a stand-alone program (tests/host_spool_harness.cpp) that
reads a script of steps, flushes and collects from a file and writes what the collects returned; compared byte for byte, records and audio and the counters,
with the definition in plain Python (capi.transmission_spool_reference) on random selection schedules.  It checks the LOGIC of the code the GPU runs -- the
verdicts, the ranks across wavefronts and workgroups, the chains and the free stack, the ring of finished records, the prefix of the collect, the clamps --
tests/test_gpu_transmission_spool.py is what a GPU says.  The same program built with -fsanitize=address,undefined runs two of the shapes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import spool_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
capi = sc.capi
ROW_BYTES, B = 16, 16


def _build(out, extra):
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O1", "-DAB_WAVE64_EMU", "-I" + os.path.join(HERE, "hostshim_wave64"), "-I" + os.path.join(REPO, "include")] + extra + \
          ["-o", out, os.path.join(HERE, "host_spool_harness.cpp")]
    subprocess.run(cmd, check=True)
    return out


@pytest.fixture(scope="module")
def hostspool(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ in this image")
    d = tmp_path_factory.mktemp("hostspool")
    return dict(dir=str(d), exe=_build(str(d / "host_spool"), []))


def _script(mask, steps, ops, max_rows, row_bytes, **p):
    """the harness's script and the model's answer to it: (blob, expected results)"""
    n_ch = len(mask)
    blob = struct.pack("<10i", n_ch, max_rows, row_bytes, B, p["pool_rows"], p["export_rows"], p["max_records"], p["min_batches"], p["idle_batches"], p["max_batches"])
    blob += np.asarray(mask, np.uint8).tobytes()
    model = capi.transmission_spool_reference(mask, B, **p)
    want = b""

    def collect():
        got = model.collect()
        return struct.pack("<3i", len(got["records"]), got["n_rows"], got["n_waiting"]) + got["records"].tobytes() + got["audio"], got["n_waiting"]

    for k, s in enumerate(steps):
        sel = np.zeros(n_ch, np.uint8)
        sel[s["selected"]] = 1
        blob += struct.pack("<i", 0) + sel.tobytes()
        for r in range(len(s["channels"])):
            blob += s["audio"][r].tobytes() + s["info"][r].tobytes()
        model.step(len(s["selected"]), s["channels"], s["audio"], s["info"], selected=s["selected"])
        for op in ops.get(k, ""):
            blob += struct.pack("<i", 1 if op == "f" else 2)
            if op == "f":
                model.flush()
            else:
                want += collect()[0]
    blob += struct.pack("<i", 1)
    model.flush()
    while True:
        blob += struct.pack("<i", 2)
        w, waiting = collect()
        want += w
        if not waiting:
            break
    cn = model.counters()
    want += struct.pack("<8Q", *[cn[k] for k in capi.SPOOL_COUNTER_NAMES])
    return blob, want, model


def _run(hostspool, blob, name, exe=None, env=None):
    src, dst = os.path.join(hostspool["dir"], name + ".script"), os.path.join(hostspool["dir"], name + ".results")
    open(src, "wb").write(blob)
    r = subprocess.run([exe or hostspool["exe"], src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    return open(dst, "rb").read(), r.stdout


def _compare(got, want, row_bytes, what):
    """walk both results collect by collect, so that a difference is named"""
    if got == want:
        return
    at = 0
    n_collect = 0
    while at + 12 <= len(want) - 64:
        n, rows, waiting = struct.unpack("<3i", want[at:at + 12])
        size = 12 + 48 * n + row_bytes * rows
        g, w = got[at:at + size], want[at:at + size]
        if g != w:
            gh = struct.unpack("<3i", g[:12]) if len(g) >= 12 else None
            detail = "counts got %r want %r" % (gh, (n, rows, waiting))
            if gh == (n, rows, waiting):
                gr, wr = np.frombuffer(g[12:12 + 48 * n], sc.REC), np.frombuffer(w[12:12 + 48 * n], sc.REC)
                bad = [i for i in range(n) if gr[i].tobytes() != wr[i].tobytes()]
                detail = "records %r: got %r want %r" % (bad[:3], sc.brief(gr[bad[:3]]), sc.brief(wr[bad[:3]])) if bad else "audio bytes"
            raise AssertionError("%s: collect %d differs: %s" % (what, n_collect, detail))
        at += size
        n_collect += 1
    raise AssertionError("%s: counters got %r want %r" % (what, struct.unpack("<8Q", got[-64:]) if len(got) >= 64 else None, struct.unpack("<8Q", want[-64:])))


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
    got, _ = _run(hostspool, blob, "random_%d_%d_%d_%d" % (n_ch, pool_rows, max_records, max_batches))
    _compare(got, want, row_bytes, "%d channels, pool %d, list %d" % (n_ch, pool_rows, max_records))


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
    got, _ = _run(hostspool, blob, "blocks")
    _compare(got, want, ROW_BYTES, "2100 channels")


def test_two_shapes_under_host_sanitizers(hostspool):
    """The stand-alone program built with -fsanitize=address,undefined: the same bytes, no report."""
    exe = _build(os.path.join(hostspool["dir"], "host_spool_san"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    env = dict(os.environ, ASAN_OPTIONS="detect_stack_use_after_return=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for n_ch, pool_rows, max_records, max_batches, max_rows, row_bytes in (SHAPES[7], SHAPES[12]):
        mask, steps = sc.schedule(n_ch, 24, seed=n_ch + pool_rows, max_rows=max_rows, row_bytes=row_bytes, wave_batch=B)
        blob, want, _ = _script(mask, steps, {8: "c", 15: "fc"}, max_rows or n_ch, row_bytes, pool_rows=pool_rows, export_rows=max_batches + 1, max_records=max_records,
                                min_batches=3, idle_batches=1, max_batches=max_batches)
        got, log = _run(hostspool, blob, "san_%d" % n_ch, exe=exe, env=env)
        assert "ERROR: AddressSanitizer" not in log and "runtime error" not in log, log[-4000:]
        _compare(got, want, row_bytes, "sanitized, %d channels" % n_ch)
