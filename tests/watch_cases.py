"""Shared by the band watch's tests: sequences of batches as the host harness (tests/host_watch_harness.cpp, run through tests/hostbed.py) reads them, what capi.band_watch_reference() makes
of them as the bytes the harness writes, and the constructed sequences with the properties the definition promises for each (asserted on the reference's own
output, so that a byte-for-byte comparison against it proves them of the kernel)."""
import importlib
import struct

import numpy as np

capi = importlib.import_module("rtlsdr-airband_amd").capi

APPEAR, VANISH = capi.WATCH_APPEAR, capi.WATCH_VANISH


def params(**kw):
    p = dict(n_rows=1, fft_log=9, max_peaks=8, T=8, M=2, C=2, R=2, E=None, two_sets=0, pack=1, first_batch=0, init=None, dev_of_row=None)
    p.update(kw)
    if p["E"] is None:
        p["E"] = p["n_rows"] * (p["T"] + p["max_peaks"])
    if p["dev_of_row"] is None:
        p["dev_of_row"] = list(range(p["n_rows"]))
    return p


def peak_array(listed, max_peaks):
    """[(bin, power)] -> [max_peaks] of PEAK_DTYPE as the survey leaves it: {-1, 0} behind the listed ones."""
    a = np.zeros(max_peaks, capi.PEAK_DTYPE)
    a["bin"] = -1
    for i, (b, p) in enumerate(listed[:max_peaks]):
        a[i] = (b, np.float32(p))
    return a


def _row_input(entry, max_peaks):
    """A row of a batch: None (switched off), a list [(bin, power)], or (list, n_peaks) where the survey counted more peaks than it lists."""
    if entry is None:
        return None
    listed, n_peaks = entry if isinstance(entry, tuple) else (entry, len(entry))
    return peak_array(listed, max_peaks), int(n_peaks)


def encode(cases):
    """The harness's cases file."""
    out = [struct.pack("<i", len(cases))]
    for p, batches in cases:
        out.append(struct.pack("<13i", p["n_rows"], p["fft_log"], p["max_peaks"], p["T"], p["M"], p["C"], p["R"], p["E"], len(batches), p["two_sets"], p["pack"],
                               p["first_batch"], 1 if p["init"] is not None else 0))
        out.append(np.array(p["dev_of_row"], "<i4").tobytes())
        if p["init"] is not None:
            out.append(np.ascontiguousarray(p["init"][0], capi.TRACK_DTYPE).tobytes() + np.ascontiguousarray(p["init"][1], capi.WATCH_ROW_DTYPE).tobytes())
        for batch in batches:
            rows = [_row_input(e, p["max_peaks"]) for e in batch]
            out.append(np.array([1 if r is None else 0 for r in rows], "<i4").tobytes())
            out.append(np.array([0 if r is None else r[1] for r in rows], "<i4").tobytes())
            out.append(b"".join((peak_array([], p["max_peaks"]) if r is None else r[0]).tobytes() for r in rows))
    return b"".join(out)


def simulate(p, batches):
    """capi.band_watch_reference() over the sequence: per batch dict(tracks [n_rows][T], rows [n_rows], row_events [per row], n_events, events (all of them))."""
    n_rows, T = p["n_rows"], p["T"]
    if p["init"] is not None:
        tracks = np.array(p["init"][0], capi.TRACK_DTYPE).reshape(n_rows, T).copy()
        rows = np.array(p["init"][1], capi.WATCH_ROW_DTYPE).reshape(n_rows).copy()
    else:
        tracks = np.stack([capi.band_watch_blank(T)[0] for _ in range(n_rows)])
        rows = np.zeros(n_rows, capi.WATCH_ROW_DTYPE)
    out = []
    for k, batch in enumerate(batches):
        row_events = []
        for r in range(n_rows):
            given = _row_input(batch[r], p["max_peaks"])
            if given is None:  # switched off: frozen, no events
                rows[r]["n_events"] = 0
                row_events.append(np.zeros(0, capi.EVENT_DTYPE))
                continue
            t, rr, ev = capi.band_watch_reference(tracks[r], rows[r], given[0], given[1], p["first_batch"] + k, T, p["M"], p["C"], p["R"], 1 << p["fft_log"],
                                                  dev=p["dev_of_row"][r])
            tracks[r], rows[r] = t, rr
            row_events.append(ev)
        events = np.concatenate(row_events)
        out.append(dict(tracks=tracks.copy(), rows=rows.copy(), row_events=row_events, n_events=len(events), events=events))
    return out


def expected_bytes(p, sim):
    """What the harness writes for the sequence, batch by batch."""
    out = []
    for s in sim:
        b = s["tracks"].tobytes() + s["rows"].tobytes()
        if p["pack"]:
            b += struct.pack("<i", s["n_events"]) + s["events"][:p["E"]].tobytes()
        else:
            b += s["events"].tobytes()
        out.append(b)
    return out


def kinds(s, row=0):
    """[(kind, bin, track, batches)] of a row's events in a simulated batch."""
    return [(int(e["kind"]), int(e["bin"]), int(e["track"]), int(e["batches"])) for e in s["row_events"][row]]


# ---- constructed sequences: (name, params, batches, check(sim)) ----------------------------------------------------------------------------------------------
def constructed():
    N = 512
    cases = []

    def add(name, p, batches, check):
        cases.append((name, p, batches, check))

    def confirm(C):
        def check(sim):
            for k, s in enumerate(sim):
                want = [(APPEAR, 100, 0, C)] if k == C - 1 else []
                assert kinds(s) == want, (C, k, kinds(s))
                t = s["tracks"][0][0]
                assert int(t["hits"]) == k + 1 and int(t["state"]) == (2 if k >= C - 1 else 1) and int(t["first_batch"]) == 0 and int(t["last_batch"]) == k
        return check

    for C in (1, 2, 255):
        add("confirm_after_%d" % C, params(C=C, pack=0 if C == 255 else 1), [[[(100, 5.0)]]] * (C + 1), confirm(C))

    def tentative(sim):
        assert all(kinds(s) == [] for s in sim)
        assert [int(s["rows"][0]["n_live"]) for s in sim] == [1, 1, 0, 1, 1]
        assert int(sim[4]["tracks"][0][0]["hits"]) == 2 and int(sim[4]["tracks"][0][0]["first_batch"]) == 3 and int(sim[4]["tracks"][0][0]["state"]) == 1
    add("tentative_freed_by_one_miss", params(C=3), [[[(100, 5.0)]], [[(100, 5.0)]], [[]], [[(100, 5.0)]], [[(100, 5.0)]]], tentative)

    def release(sim):
        assert kinds(sim[1]) == [(APPEAR, 100, 0, 2)]
        assert kinds(sim[2]) == [] and kinds(sim[3]) == [] and int(sim[3]["tracks"][0][0]["misses"]) == 2 and int(sim[3]["rows"][0]["n_confirmed"]) == 1
        assert kinds(sim[4]) == [(VANISH, 100, 0, 2)] and int(sim[4]["rows"][0]["n_live"]) == 0
        assert sim[4]["row_events"][0]["power"][0] == np.float32(7.0)  # the largest power it was seen with
        assert sim[4]["tracks"][0][0].tobytes() == capi.band_watch_blank(1)[0][0].tobytes()
    add("release_after_exactly_R", params(C=2, R=3), [[[(100, 5.0)]], [[(100, 7.0)]], [[]], [[]], [[]], [[]]], release)

    def drift(sim):
        assert [int(s["tracks"][0][0]["bin"]) for s in sim[:3]] == [100, 102, 104] and kinds(sim[1]) == [(APPEAR, 102, 0, 2)]
        assert int(sim[3]["tracks"][0][1]["bin"]) == 107 and int(sim[3]["tracks"][0][1]["hits"]) == 1  # M + 1 away: a new track
        assert int(sim[3]["tracks"][0][0]["bin"]) == 104 and int(sim[3]["tracks"][0][0]["misses"]) == 1
    add("drift_of_M_followed_M_plus_1_not", params(M=2, R=5), [[[(100, 5.0)]], [[(102, 5.0)]], [[(104, 5.0)]], [[(107, 5.0)]]], drift)

    def circular(sim):
        assert kinds(sim[1]) == [(APPEAR, N - 1, 0, 2)] and int(sim[1]["rows"][0]["n_live"]) == 1
        assert kinds(sim[2]) == [] and int(sim[2]["tracks"][0][0]["bin"]) == 1 and int(sim[2]["tracks"][0][0]["hits"]) == 3
    add("circular_distance", params(M=2), [[[(1, 5.0)]], [[(N - 1, 5.0)]], [[(1, 5.0)]]], circular)

    def equal_distance(sim):
        t = sim[1]["tracks"][0]
        assert int(t[0]["bin"]) == 102 and int(t[0]["hits"]) == 2 and int(sim[0]["tracks"][0][0]["bin"]) == 104  # slot 0 held the HIGHER bin: the slot decides
        assert int(t[1]["state"]) == 0  # the other one was tentative and missed
        assert kinds(sim[1]) == [(APPEAR, 102, 0, 2)]
    add("equal_distance_lower_slot_wins", params(M=2), [[[(104, 9.0), (100, 8.0)]], [[(102, 9.0)]]], equal_distance)

    def two_peaks(sim):
        t = sim[1]["tracks"][0]
        assert int(t[0]["bin"]) == 101 and int(t[0]["hits"]) == 2 and int(t[1]["bin"]) == 99 and int(t[1]["hits"]) == 1 and int(t[1]["state"]) == 1
    add("two_peaks_near_one_track", params(M=2), [[[(100, 5.0)]], [[(101, 9.0), (99, 8.0)]]], two_peaks)

    def freed(sim):
        assert kinds(sim[0]) == [(APPEAR, 100, 0, 1)]
        assert kinds(sim[1]) == [(VANISH, 100, 0, 1)] and int(sim[1]["rows"][0]["dropped"]) == 1 and int(sim[1]["rows"][0]["n_live"]) == 0
        assert kinds(sim[2]) == [(APPEAR, 200, 0, 1)] and int(sim[2]["rows"][0]["dropped"]) == 1
    add("freed_slot_reused_next_batch", params(T=1, C=1, R=1), [[[(100, 5.0)]], [[(200, 5.0)]], [[(200, 5.0)]]], freed)

    def full(sim):
        for k, s in enumerate(sim):
            assert int(s["rows"][0]["dropped"]) == k + 1 and int(s["rows"][0]["n_live"]) == 2
            assert [int(b) for b in s["tracks"][0]["bin"]] == [50, 150]
        assert kinds(sim[1]) == [(APPEAR, 50, 0, 2), (APPEAR, 150, 1, 2)]
    add("table_full_counts_dropped", params(T=2), [[[(50, 9.0), (150, 8.0), (250, 7.0)]]] * 3, full)

    many = [(8 * i + 3, 100.0 - i) for i in range(64)]

    def t1(sim):
        assert int(sim[0]["rows"][0]["dropped"]) == 63 and int(sim[1]["rows"][0]["dropped"]) == 126 and kinds(sim[1]) == [(APPEAR, 3, 0, 2)]
    add("T1_with_64_peaks", params(T=1, max_peaks=64), [[many], [many]], t1)

    def t64(sim):
        assert int(sim[0]["rows"][0]["n_live"]) == 64 and int(sim[0]["rows"][0]["dropped"]) == 0
        assert kinds(sim[1]) == [(APPEAR, 8 * i + 3, i, 2) for i in range(64)]
        assert kinds(sim[2]) == [] and kinds(sim[3]) == [(VANISH, 8 * i + 3, i, 2) for i in range(64)]
    add("T64_with_64_peaks", params(T=64, max_peaks=64, R=2), [[many], [many], [[]], [[]]], t64)

    def more(sim):
        assert int(sim[0]["rows"][0]["n_live"]) == 4 and int(sim[0]["rows"][0]["dropped"]) == 0
    add("n_peaks_above_max_peaks", params(max_peaks=4), [[([(10 + 20 * i, 9.0 - i) for i in range(4)], 20)]], more)

    def empty(sim):
        assert all(s["tracks"].tobytes() == sim[0]["tracks"].tobytes() and s["rows"].tobytes() == bytes(16) for s in sim)
    add("empty_list", params(), [[[]], [[]]], empty)

    init_t, init_r = capi.band_watch_blank(8)
    init_t[2] = (300, np.float32(4.0), np.float32(6.0), 0, 70000, 65534, 0, 2)
    init_r = np.array((1, 1, 0, 5), capi.WATCH_ROW_DTYPE)

    def saturate(sim):
        assert [int(s["tracks"][0][2]["hits"]) for s in sim[:3]] == [65535, 65535, 65535]
        assert kinds(sim[4]) == [(VANISH, 300, 2, 65535)] and int(sim[4]["rows"][0]["dropped"]) == 5
    add("hits_and_batches_saturate", params(first_batch=70001, init=(init_t[None, :], np.array([init_r]))),
        [[[(300, 5.0)]], [[(300, 5.0)]], [[(300, 5.0)]], [[]], [[]]], saturate)

    def order(sim):
        # batch 2: peaks in power order 300 (new, tentative), 100 (confirmed earlier, no event); 400 and 200 miss once; batch 3 (R = 2): they vanish in SLOT order
        assert kinds(sim[1]) == [(APPEAR, 200, 0, 2), (APPEAR, 100, 1, 2), (APPEAR, 400, 2, 2)]
        assert kinds(sim[3]) == [(APPEAR, 300, 3, 2), (VANISH, 200, 0, 2), (VANISH, 400, 2, 2)]
    first = [(200, 9.0), (100, 8.0), (400, 7.0)]
    add("event_order_within_a_row", params(R=2), [[first], [first], [[(300, 9.5), (100, 8.0)]], [[(300, 9.5), (100, 8.0)]]], order)

    def frozen(sim):
        assert sim[2]["tracks"][1].tobytes() == sim[1]["tracks"][1].tobytes() and int(sim[2]["rows"][1]["n_events"]) == 0
        assert sim[3]["tracks"][1].tobytes() == sim[1]["tracks"][1].tobytes()
        assert [kinds(s, 1) for s in sim] == [[], [(APPEAR, 100, 0, 2)], [], [], []] and int(sim[4]["tracks"][1][0]["hits"]) == 3
        assert [e["dev"] for e in sim[1]["events"]] == [4, 7, 9]
    one = [(100, 5.0)]
    for two_sets in (0, 1):
        add("switched_off_row_is_frozen_%d_sets" % (two_sets + 1), params(n_rows=3, dev_of_row=[4, 7, 9], two_sets=two_sets),
            [[one, one, one], [one, one, one], [one, None, one], [one, None, []], [one, one, one]], frozen)
    return cases


def wandering(seed, n_batches=40, n_rows=3):
    """The fuzz: random parameters, a handful of wandering carriers per row plus strays, lists in the survey's order."""
    rng = np.random.default_rng(seed)
    fft_log = int(rng.choice([8, 9, 13]))
    N = 1 << fft_log
    max_peaks = int(rng.choice([1, 3, 8, 16]))
    T = int(rng.choice([1, 2, 4, 8, 64]))
    p = params(n_rows=n_rows, fft_log=fft_log, max_peaks=max_peaks, T=T, M=int(rng.choice([0, 1, 2, 5, N // 2])), C=int(rng.choice([1, 2, 3])), R=int(rng.choice([1, 2, 4])),
               two_sets=int(seed & 1), pack=1 if seed % 8 == 0 else 0, first_batch=int(rng.choice([0, 7, 0xFFFFFFF0 - (1 << 32)])),
               dev_of_row=sorted(int(d) for d in rng.choice(10, n_rows, replace=False)))
    p["E"] = int(rng.integers(1, n_rows * (T + max_peaks) + 1))
    carriers = [[int(b) for b in rng.integers(0, N, int(rng.integers(1, 6)))] for _ in range(n_rows)]
    batches = []
    for _ in range(n_batches):
        batch = []
        for r in range(n_rows):
            if rng.random() < 0.08:
                batch.append(None)
                continue
            found = {}
            for i, b in enumerate(carriers[r]):
                carriers[r][i] = b = (b + int(rng.integers(-2, 3))) % N
                if rng.random() < 0.7:
                    found[b] = np.float32(rng.choice([4.0, 8.0, 16.0]) * (1 + (rng.random() < 0.5) * rng.random()))
            for _ in range(int(rng.integers(0, 3))):
                found[int(rng.integers(0, N))] = np.float32(2.0 + rng.random())
            listed = sorted(found.items(), key=lambda bp: (-int(np.float32(bp[1]).view(np.uint32)), bp[0]))
            batch.append((listed, len(listed) + int(rng.integers(0, 2)) * (len(listed) >= max_peaks)))
        batches.append(batch)
    return p, batches
