"""The band follow's kernels (csrc/band_follow.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles, ballots and barriers are rendezvous points) into a stand-alone program (tests/host_follow_harness.cpp) that
reads sequences of batches from a file and writes what the kernels left; compared byte for byte with the definition in plain Python
(capi.band_follow_reference) on seeded random track tables.  It checks the LOGIC of the code the GPU runs -- the cross-lane reads of step A, the ballots and
their lowest bits in step B, the staging indices, the bins written to ChanState, the packed list -- tests/test_gpu_band_follow.py is what a GPU says.  The same
program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import struct

import numpy as np
import pytest

import hostbed
import watch_cases

capi = watch_cases.capi
N_BATCHES, N_FFT = 12, 512


@pytest.fixture(scope="module")
def hostfollow(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_follow", "host_follow_harness.cpp")


def _tables(rng, n_rows, T, n_batches, busy, script=None):
    """n_batches track tables [n_rows][T] as a watch could leave them: slots appear tentative, are confirmed, drift by a bin, vanish (a free slot) and are filled
    again.  busy: how many slots per row are kept alive on average.  script: {(batch, row, slot): (state, bin)} entries written over the random ones."""
    tracks = np.zeros((n_rows, T), capi.TRACK_DTYPE)
    tracks["bin"] = -1
    out = []
    for k in range(n_batches):
        for r in range(n_rows):
            for s in range(T):
                t = tracks[r, s]
                state, u = int(t["state"]), rng.random()
                if state == capi.WATCH_FREE:
                    if u < busy / T:
                        t["bin"], t["state"], t["hits"], t["first_batch"], t["last_batch"] = int(rng.integers(0, N_FFT)), capi.WATCH_TENTATIVE, 1, k, k
                elif state == capi.WATCH_TENTATIVE:
                    if u < 0.8:
                        t["state"], t["hits"], t["last_batch"] = capi.WATCH_CONFIRMED, 2, k
                    else:
                        tracks[r, s] = np.zeros((), capi.TRACK_DTYPE)
                        tracks[r, s]["bin"] = -1
                else:
                    if u < 0.2:  # gone: the slot is free in this batch and may be filled in the next
                        tracks[r, s] = np.zeros((), capi.TRACK_DTYPE)
                        tracks[r, s]["bin"] = -1
                    elif u < 0.5:  # drift
                        t["bin"] = (int(t["bin"]) + int(rng.choice([-1, 1]))) % N_FFT
                        t["hits"] = min(int(t["hits"]) + 1, 65535)
                        t["last_batch"] = k
            for (kk, rr, ss), (state, b) in (script or {}).items():
                if kk == k and rr == r:
                    tracks[r, ss] = np.zeros((), capi.TRACK_DTYPE)
                    tracks[r, ss]["bin"], tracks[r, ss]["state"], tracks[r, ss]["hits"] = b, state, 2 if state else 0
        out.append(tracks.copy())
    return out


def _case(seed, T, per_row, E=None, first_batch=0, off=None, busy=None, script=None):
    """Three rows on dongles 1, 2, 4 (dongles 0 and 3 have no row; dongle 0 has a follower nobody tunes), per_row[r] followers on row r."""
    rng = np.random.default_rng([seed, T] + list(per_row))
    n_rows, dev_of_row = len(per_row), [1, 2, 4][:len(per_row)]
    n_follow = 1 + sum(per_row)
    ranges, at = [], 1
    for n in per_row:
        ranges.append((at, n))
        at += n
    channel = np.sort(rng.choice(4 * n_follow, n_follow, replace=False)).astype("<i4")
    home = rng.integers(0, N_FFT, n_follow).astype("<i4")
    busy = max(per_row) + 1.5 if busy is None else busy  # more confirmed tracks than followers now and then
    tables = _tables(rng, n_rows, T, N_BATCHES, min(busy, T), script)
    disabled = np.zeros((N_BATCHES, n_rows), "<i4")
    for k, r in (off or []):
        disabled[k, r] = 1
    most = n_follow + n_rows * T
    p = dict(n_rows=n_rows, T=T, E=most if E is None else E, first_batch=first_batch, n_follow=n_follow, dev_of_row=dev_of_row, ranges=ranges, channel=channel,
             home=home, tables=tables, disabled=disabled)
    return p


def _encode(cases):
    blob = struct.pack("<i", len(cases))
    for p in cases:
        blob += struct.pack("<7i", p["n_rows"], 9, p["T"], p["E"], N_BATCHES, p["first_batch"], p["n_follow"])
        blob += np.array(p["dev_of_row"], "<i4").tobytes() + np.array(p["ranges"], "<i4").tobytes() + p["home"].tobytes() + p["channel"].tobytes()
        for k in range(N_BATCHES):
            blob += p["disabled"][k].tobytes() + p["tables"][k].tobytes()
    return blob


def _simulate(p):
    """capi.band_follow_reference() over the case's batches: per batch the bytes the harness writes, and what happened (for the non-vacuity checks)."""
    fol = capi.band_follow_blank(p["channel"], p["home"])
    rows = np.zeros(p["n_rows"], capi.FOLLOW_ROW_DTYPE)
    stamp, out, seen = 0, [], dict(kinds=[], unserved=0, frozen=0, clipped=0, changes=[])
    for k in range(N_BATCHES):
        changes = []
        for r, (first, n) in enumerate(p["ranges"]):
            if p["disabled"][k, r]:
                rows[r]["n_changes"] = 0
                seen["frozen"] += 1
                continue
            f, row, ch = capi.band_follow_reference(fol[first:first + n], p["tables"][k][r], p["home"][first:first + n], p["first_batch"] + k, dev=p["dev_of_row"][r])
            fol[first:first + n], rows[r] = f, row
            changes.append(ch)
            seen["unserved"] += int(row["n_unserved"])
        changes = np.concatenate(changes) if changes else np.zeros(0, capi.FOLLOW_CHANGE_DTYPE)
        if len(changes):
            stamp = k + 1
        seen["kinds"] += changes["kind"].tolist()
        seen["clipped"] += len(changes) > p["E"]
        seen["changes"].append(changes)
        out.append(fol.tobytes() + rows.tobytes() + fol["bin"].astype("<i4").tobytes() + struct.pack("<2i", stamp, len(changes)) + changes[:p["E"]].tobytes())
    return out, seen


def _compare(got, cases, sims):
    at = 0
    for n, (p, (want, _)) in enumerate(zip(cases, sims)):
        for k, w in enumerate(want):
            have = got[at:at + len(w)]
            if have != w:
                nf, nr = 16 * p["n_follow"], 16 * p["n_rows"]
                what = "followers" if have[:nf] != w[:nf] else "rows" if have[nf:nf + nr] != w[nf:nf + nr] else "bins, stamp or changes"
                raise AssertionError("case %d batch %d: %s differ (T %d, followers per row %r, E %d)" % (n, k, what, p["T"], [c for _, c in p["ranges"]], p["E"]))
            at += len(w)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


SHAPES = [(T, F) for T in (1, 8, 64) for F in (1, 2, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=["T%d-F%d" % s for s in SHAPES])
def test_seeded_tables_equal_the_reference(hostfollow, shape):
    """max_tracks in {1, 8, 64} x followers per row in {1, 2, 64}, 12 batches of random tables on three rows, one row frozen for three batches."""
    T, F = shape
    cases = [_case(seed, T, [F, F, max(1, F // 2)], off=[(4, 1), (5, 1), (6, 1)], first_batch=7 * seed) for seed in range(2)]
    sims = [_simulate(p) for p in cases]
    got, _ = hostfollow.run(_encode(cases), "t%df%d" % shape)
    _compare(got, cases, sims)
    kinds = sum((s[1]["kinds"] for s in sims), [])
    print("T %d F %d: %d TUNE %d MOVE %d HOME, %d unserved" % (T, F, kinds.count(1), kinds.count(2), kinds.count(3), sum(s[1]["unserved"] for s in sims)))
    assert kinds.count(capi.FOLLOW_TUNE) > 0 and kinds.count(capi.FOLLOW_HOME) > 0 and all(s[1]["frozen"] == 3 for s in sims)
    if T > 1:
        assert kinds.count(capi.FOLLOW_MOVE) > 0
    if T > F:
        assert sum(s[1]["unserved"] for s in sims) > 0  # more confirmed tracks than followers: the case arose


def test_a_slot_that_vanishes_and_is_refilled_the_batch_after(hostfollow):
    """Slot 2 of row 0 confirmed at batch 1 on bin 100, free at batch 4, confirmed again at batch 5 on bin 300: TUNE, HOME, TUNE -- and while row 0 is frozen
    (batches 7 - 8) a track that ends does not send its follower home until the row is back."""
    C, Fr = capi.WATCH_CONFIRMED, capi.WATCH_FREE
    script = {(k, 0, 2): (C, 100) for k in (1, 2, 3)}
    script[(4, 0, 2)] = (Fr, -1)
    script.update({(k, 0, 2): (C, 300) for k in (5, 6)})
    script.update({(k, 0, 2): (Fr, -1) for k in range(7, N_BATCHES)})
    script.update({(k, 0, s): (Fr, -1) for k in range(N_BATCHES) for s in range(8) if s != 2})
    p = _case(3, 8, [1], busy=0.0, off=[(7, 0), (8, 0)], script=script)
    want, seen = _simulate(p)
    got, _ = hostfollow.run(_encode([p]), "refill")
    _compare(got, [p], [(want, seen)])
    ch = [(k, int(c["kind"]), int(c["bin"]), int(c["track"])) for k, cs in enumerate(seen["changes"]) for c in cs]
    home = int(p["home"][1])
    assert ch == [(1, capi.FOLLOW_TUNE, 100, 2), (4, capi.FOLLOW_HOME, home, 2), (5, capi.FOLLOW_TUNE, 300, 2), (9, capi.FOLLOW_HOME, home, 2)], ch


def test_fewer_records_than_changes(hostfollow):
    """max_changes = 2 with three busy rows: n_changes is exact, the first two records are the reference's first two, nothing behind them is written (the
    harness's guard zone), followers and rows are complete."""
    cases = [_case(11, 8, [2, 2, 2], E=2), _case(12, 64, [64, 64, 64], E=1)]
    sims = [_simulate(p) for p in cases]
    got, _ = hostfollow.run(_encode(cases), "clipped")
    _compare(got, cases, sims)
    assert all(s[1]["clipped"] > 0 for s in sims)


def test_two_shapes_under_host_sanitizers(hostfollow):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    cases = [_case(21, 8, [2, 1, 2], E=3, off=[(2, 0)]), _case(22, 64, [64, 3, 1])]
    sims = [_simulate(p) for p in cases]
    got, _ = hostfollow.sanitized().run(_encode(cases), "san")
    _compare(got, cases, sims)
