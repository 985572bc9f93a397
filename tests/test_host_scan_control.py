"""Scan control's kernels (csrc/scan_control.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ into a stand-alone program (tests/host_scan_control_harness.cpp) that reads sequences of batches from a file and writes what the kernels
left; compared byte for byte with the definition in plain Python (capi.scan_control_reference) on seeded random axcindicate bytes, enable masks and holds.  It
checks the LOGIC of the code the GPU runs -- the decision, the switch list the exchange kernel is fed, the packed record list across a pack chunk --
tests/test_gpu_scan_control.py is what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import importlib
import struct

import numpy as np
import pytest

import hostbed

capi = importlib.import_module("rtlsdr-airband_amd").capi
N_BATCHES = 14
LEAVE = -2  # the harness's "leave the list's hold as it is"


@pytest.fixture(scope="module")
def hostscan(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_scan_control", "host_scan_control_harness.cpp")


def _case(seed, n_lists, idle=2, dwell=1, E=None, first_batch=0, p_signal=0.25, n_batches=N_BATCHES):
    """n_lists lists of 1 .. 5 entries on every other dongle (the dongles between have eight channels and no list), started on random entries; per batch random
    axcindicate bytes, now and then a dongle switched off for a few batches, now and then a hold set or released."""
    rng = np.random.default_rng([seed, n_lists, idle, dwell])
    n_dev = 2 * n_lists + 1
    sizes = (np.arange(n_lists) + int(rng.integers(0, 5))) % 5 + 1  # every size from 1 to 5 wherever there are five lists
    lists, first, ext = [], 0, 0
    for i in range(n_lists):
        ext += 8  # the multichannel dongle in front
        lists.append((2 * i + 1, ext, 64 * i + 3, first, int(sizes[i])))
        first += int(sizes[i])
        ext += 1
    n_ch = ext + 8
    state = np.zeros(n_lists, capi.SCAN_STATE_DTYPE)
    state["idx"] = rng.integers(0, sizes)
    state["hold"], state["has_list"] = -1, 1
    state["last"] = rng.integers(0, sizes)
    disabled = np.zeros((n_batches, n_dev), "<i4")
    for i in rng.choice(n_lists, max(1, n_lists // 6), replace=False):
        k0 = int(rng.integers(1, n_batches - 3))
        disabled[k0:k0 + int(rng.integers(1, 4)), 2 * i + 1] = 1
    axc = np.where(rng.random((n_batches, n_ch)) < p_signal, rng.choice(np.frombuffer(b"*<>", np.uint8), (n_batches, n_ch)), ord(" ")).astype(np.uint8)
    hold = np.full((n_batches, n_lists), LEAVE, "<i4")
    for i in rng.choice(n_lists, max(1, n_lists // 5), replace=False):
        k0 = int(rng.integers(0, n_batches - 4))
        hold[k0, i] = int(rng.integers(0, sizes[i]))
        hold[k0 + int(rng.integers(2, 5)), i] = -1
    return dict(n_lists=n_lists, n_dev=n_dev, n_ch=n_ch, idle=idle, dwell=dwell, E=n_lists if E is None else E, first_batch=first_batch, lists=lists, state=state,
                disabled=disabled, axc=axc, hold=hold, n_batches=n_batches)


def _encode(cases):
    blob = struct.pack("<i", len(cases))
    for p in cases:
        blob += struct.pack("<8i", p["n_lists"], p["n_dev"], p["n_ch"], p["idle"], p["dwell"], p["E"], p["n_batches"], p["first_batch"])
        blob += np.array(p["lists"], "<i4").tobytes() + p["state"].tobytes()
        pad = b"\0" * (-p["n_ch"] % 4)
        for k in range(p["n_batches"]):
            blob += p["disabled"][k].tobytes() + p["axc"][k].tobytes() + pad + p["hold"][k].tobytes()
    return blob


def _simulate(p):
    """capi.scan_control_reference() over the case's batches: per batch the bytes the harness writes, and what happened (for the non-vacuity checks)."""
    state = p["state"].copy()
    out, seen = [], dict(kinds=[], retag=0, frozen=0, clipped=0, wraps=0, held_hops=0, records=[])
    for k in range(p["n_batches"]):
        records, sw = [], np.zeros((p["n_lists"], 3), "<i4")
        sw[:, 0] = -1
        for i, (dev, ext, slot, first, n) in enumerate(p["lists"]):
            if p["hold"][k, i] != LEAVE:
                state[i]["hold"] = p["hold"][k, i]
            on = not p["disabled"][k, dev]
            seen["frozen"] += (not on) and n >= 2
            before = int(state[i]["idx"])
            st, rec = capi.scan_control_reference(state[i], p["axc"][k, ext], n, p["first_batch"] + k, idle_batches=p["idle"], dwell_batches=p["dwell"], dev=dev, enabled=on)
            state[i] = st
            records.append(rec)
            if int(st["idx"]) != before:
                sw[i] = (slot, first + before, first + int(st["idx"]))
                seen["wraps"] += int(st["idx"]) == 0 and int(st["hold"]) < 0
                seen["held_hops"] += int(st["hold"]) >= 0
        records = np.concatenate(records)
        seen["kinds"] += records["kind"].tolist()
        seen["retag"] += int((records["flags"] == capi.SCAN_RETAG).sum())
        seen["clipped"] += len(records) > p["E"]
        seen["records"].append(records)
        out.append(state.tobytes() + sw.tobytes() + struct.pack("<i", len(records)) + records[:p["E"]].tobytes())
    return out, seen


def _compare(got, cases, sims):
    at = 0
    for n, (p, (want, _)) in enumerate(zip(cases, sims)):
        for k, w in enumerate(want):
            have = got[at:at + len(w)]
            if have != w:
                ns, nw = 16 * p["n_lists"], 12 * p["n_lists"]
                what = "states" if have[:ns] != w[:ns] else "switch lists" if have[ns:ns + nw] != w[ns:ns + nw] else "count or records"
                raise AssertionError("case %d batch %d: %s differ (%d lists, idle %d, dwell %d, E %d)" % (n, k, what, p["n_lists"], p["idle"], p["dwell"], p["E"]))
            at += len(w)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


SIZES = [1, 63, 64, 65, 1025]  # one list; either side of a wavefront; 1 025 crosses a chunk of the pack kernel


@pytest.mark.parametrize("n_lists", SIZES)
def test_seeded_sequences_equal_the_reference(hostscan, n_lists):
    """Lists of 1 to 5 entries, random bytes, enable masks and holds, at dwell 1 and 2: records, counts, states and switch lists."""
    cases = [_case(1, n_lists, idle=2, dwell=1, first_batch=5), _case(2, n_lists, idle=3, dwell=2, p_signal=0.15)]
    if n_lists == 1:  # the one list has one entry in one of them and several in the others
        cases += [_case(s, 1, idle=1, dwell=1) for s in range(3, 8)]
        assert {p["lists"][0][4] for p in cases} >= {1, 2}
    sims = [_simulate(p) for p in cases]
    got, _ = hostscan.run(_encode(cases), "n%d" % n_lists)
    _compare(got, cases, sims)
    kinds = sum((s[1]["kinds"] for s in sims), [])
    print("%d lists: %d HOP %d ACTIVITY (%d RETAG), %d wraps, %d hops to a hold, %d frozen list-batches" % (
        n_lists, kinds.count(capi.SCAN_HOP), kinds.count(capi.SCAN_ACTIVITY), sum(s[1]["retag"] for s in sims), sum(s[1]["wraps"] for s in sims),
        sum(s[1]["held_hops"] for s in sims), sum(s[1]["frozen"] for s in sims)))
    assert kinds.count(capi.SCAN_HOP) > 0
    if n_lists >= 63:  # the fleet's cases all arose
        assert kinds.count(capi.SCAN_ACTIVITY) > 0 and sum(s[1]["retag"] for s in sims) > 0 and sum(s[1]["wraps"] for s in sims) > 0
        assert sum(s[1]["held_hops"] for s in sims) > 0 and sum(s[1]["frozen"] for s in sims) > 0
        assert 0 < kinds.count(capi.SCAN_ACTIVITY) - sum(s[1]["retag"] for s in sims)  # ACTIVITY without RETAG too


def test_fewer_records_than_there_are(hostscan):
    """max_records below the record count: the count is exact, the records kept are the reference's first, nothing behind them is written (the harness's guard
    zone), states and switch lists are complete."""
    cases = [_case(11, 65, E=3), _case(12, 1025, E=1), _case(13, 1025, E=500, idle=1, p_signal=0.05)]
    sims = [_simulate(p) for p in cases]
    got, _ = hostscan.run(_encode(cases), "clipped")
    _compare(got, cases, sims)
    assert all(s[1]["clipped"] > 0 for s in sims)
    assert max(len(r) for r in sims[2][1]["records"]) > 500  # hundreds of records kept, and the cut falls inside the pack kernel's first chunk of lists


def test_two_shapes_under_host_sanitizers(hostscan):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    cases = [_case(21, 65, E=4), _case(22, 1025, n_batches=6)]
    sims = [_simulate(p) for p in cases]
    got, _ = hostscan.sanitized().run(_encode(cases), "san")
    _compare(got, cases, sims)
