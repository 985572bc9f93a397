"""The mixer gate's kernels (csrc/mixer_gate.hip, with the passes of csrc/gate_passes.h and the samples of csrc/audio_sample.h) with their wavefront semantics on
the CPU: the kernel source compiled for the host through tests/hostshim_wave64/ (lanes as fibers; ballots, shuffles and barriers are rendezvous points) into a
stand-alone program (tests/host_mixer_gate_harness.cpp) that reads steps from a file and writes what the kernels left; compared byte for byte with the definition
in numpy (capi.mixer_gate_reference).  It checks the LOGIC of the code the GPU runs -- the rule and its memory, the ascending list across wavefronts and
workgroups, the interleaving of left and right, the frame-indexed record, the row stride of the grid, the clamps -- tests/test_gpu_mixer_gate.py is what a GPU
says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import struct

import numpy as np
import pytest

import audio_cases as ac
import hostbed

capi = ac.capi
ENCODINGS = (None, "s16", "ulaw", "alaw")
NEVER, SIGNAL, ALWAYS = capi.GATE_NEVER, capi.GATE_SIGNAL, capi.GATE_ALWAYS


def _enc(e):
    return capi.AUDIO_F32 if e is None else capi.AUDIO_ENCODINGS[e]


@pytest.fixture(scope="module")
def hostmix(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_mixer_gate", "host_mixer_gate_harness.cpp", extra=["-ffp-contract=off"])


def _case(enc, stereo, gate, steps, max_rows=None, grid=2, stereo_flags=None, listed=None):
    """steps: [(left [M][B], right [M][B], has_signal [M])].  listed = (count, index): the pack alone on a given list, padded to max_rows with mixers out of range
    the kernel must never follow."""
    gate = np.asarray(gate, np.uint8)
    M = len(gate)
    B = steps[0][0].shape[1]
    flags = np.zeros(M, np.uint8) if stereo_flags is None else np.asarray(stereo_flags, np.uint8)
    steps = [(np.ascontiguousarray(l, np.float32), np.ascontiguousarray(r, np.float32), np.asarray(s, np.uint8)) for l, r, s in steps]
    if listed is not None:
        count, index = listed
        max_rows = max(len(index), 1) if max_rows is None else max_rows
        listed = (count, (list(index) + [M + 1000, -9, 2 ** 31 - 1] * max_rows)[:max_rows])
    return dict(enc=enc, W=2 if stereo else 1, gate=gate, flags=flags, steps=steps, B=B, M=M, max_rows=M if max_rows is None else max_rows, grid=grid, listed=listed)


def _encode(cases):
    blob = struct.pack("<i", len(cases))
    for p in cases:
        blob += struct.pack("<8i", _enc(p["enc"]), p["W"], p["B"], p["M"], p["max_rows"], p["grid"], len(p["steps"]), 0 if p["listed"] is None else 1)
        blob += p["gate"].tobytes() + p["flags"].tobytes()
        if p["listed"] is not None:
            blob += struct.pack("<i", p["listed"][0]) + np.array(p["listed"][1], "<i4").tobytes()
        for l, r, s in p["steps"]:
            blob += s.tobytes() + l.tobytes() + r.tobytes()
    return blob


def _want(p):
    """per step: the bytes the harness writes"""
    out = []
    if p["listed"] is None:
        ref = capi.mixer_gate_reference(p["gate"], p["max_rows"], p["enc"], p["W"] == 2, [(l, r, s, p["flags"]) for l, r, s in p["steps"]])
        for w in ref:
            b = struct.pack("<ii", w["n_active"], len(w["mixers"])) + w["mixers"].astype("<i4").tobytes() + w["rows"].tobytes()
            out.append(b + (w["info"].tobytes() if w["info"] is not None else b""))
    else:
        count, index = p["listed"]
        kept = min(max(count, 0), p["max_rows"])
        for l, r, s in p["steps"]:
            rows, info = capi.mixer_rows_reference(l, r, p["enc"], p["W"] == 2, index[:kept], p["flags"])
            b = struct.pack("<ii", count, kept) + np.array(index[:kept], "<i4").tobytes() + rows.tobytes()
            out.append(b + (info.tobytes() if info is not None else b""))
    return out


def _compare(got, cases):
    at = 0
    for n, p in enumerate(cases):
        for k, w in enumerate(_want(p)):
            have = got[at:at + len(w)]
            if have != w:
                kept = struct.unpack("<i", w[4:8])[0]
                a, b = 8 + 4 * kept, len(w) - (16 * kept if p["enc"] is not None else 0)
                what = "count" if have[:8] != w[:8] else "list" if have[8:a] != w[8:a] else "row bytes" if have[a:b] != w[a:b] else "records"
                detail = ""
                if what == "records":
                    detail = " got %r want %r" % (np.frombuffer(have[b:], capi.AUDIO_ROW_DTYPE)[:4].tolist(), np.frombuffer(w[b:], capi.AUDIO_ROW_DTYPE)[:4].tolist())
                if what == "count":
                    detail = " got %r want %r" % (struct.unpack("<ii", have[:8]), struct.unpack("<ii", w[:8]))
                raise AssertionError("case %d step %d (%s, W %d, B %d, %d mixers, max_rows %d, grid %d): %s differ%s"
                                     % (n, k, p["enc"], p["W"], p["B"], p["M"], p["max_rows"], p["grid"], what, detail))
            at += len(w)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


def _signal_steps(M, B, n_steps, seed, p_signal=0.3):
    """random sums with a signal history: a mixer without signal holds zeros, as the sums of a closed squelch do"""
    rng = np.random.default_rng(seed)
    steps = []
    for k in range(n_steps):
        sig = (rng.random(M) < p_signal).astype(np.uint8)
        if k == 0:
            sig[:] = 0
            sig[M // 2] = 1
        left = ac.random_rows(M, B, seed=seed + 10 * k) * sig[:, None]
        right = ac.random_rows(M, B, seed=seed + 10 * k + 5) * sig[:, None]
        steps.append((left, right, sig))
    return steps


def _mixed_gate(M, seed=1):
    gate = np.random.default_rng(seed).choice([NEVER, SIGNAL, SIGNAL, ALWAYS], M).astype(np.uint8)
    gate[M // 2] = SIGNAL
    if M > 1:
        gate[M - 1] = ALWAYS
    return gate


@pytest.mark.parametrize("M", [1, 63, 64, 65, 1025])
def test_list_across_wavefronts_and_workgroups(hostmix, M):
    """The rule with its memory over four steps, mixed gates, max_rows below, equal to and above the count; the list crosses a wavefront (65), a workgroup and two
    workgroups (1025).  Small rows keep the fibers quick: the pack is ulaw, W = 2, B = 8 here; the full-size rows are the other tests'."""
    steps = _signal_steps(M, 8, 4, seed=M)
    gate = _mixed_gate(M)
    flags = (np.arange(M) % 3 == 0).astype(np.uint8)
    ref = capi.mixer_gate_reference(gate, M, "ulaw", True, [(l, r, s, flags) for l, r, s in steps])
    counts = [w["n_active"] for w in ref]
    cases = [_case("ulaw", True, gate, steps, stereo_flags=flags)]                                       # above (or equal to) every count
    if max(counts) > 1:
        cases.append(_case("ulaw", True, gate, steps, max_rows=max(counts) - 1, stereo_flags=flags))    # below
        cases.append(_case("ulaw", True, gate, steps, max_rows=max(counts), stereo_flags=flags))        # equal
    cases.append(_case(None, False, gate, steps, max_rows=1, grid=1))
    got, _ = hostmix.run(_encode(cases), "list_%d" % M)
    _compare(got, cases)
    if M >= 63:
        trailing = [m for k in range(1, 4) for m in ref[k]["mixers"] if gate[m] == SIGNAL and not steps[k][2][m]]
        assert trailing, "no mixer delivered only because of the step before"
        assert any(gate[m] == SIGNAL and m not in w["mixers"] for w in ref for m in range(M)), "no SIGNAL mixer ever left out"
    if M == 1025:
        assert any(w["mixers"][-1] == 1024 for w in ref if len(w["mixers"])), "the second workgroup's mixer never listed"


@pytest.mark.parametrize("B", [1000, 2000])
@pytest.mark.parametrize("stereo", [False, True])
@pytest.mark.parametrize("enc", ENCODINGS)
def test_rows_of_every_encoding_and_width(hostmix, enc, stereo, B):
    """Seven mixers of mixed scale over two steps, grid 1, 2 and larger than the row count; ALWAYS gates so that silent rows are packed too."""
    steps = _signal_steps(7, B, 2, seed=B + (3 if stereo else 0), p_signal=0.7)
    gate = np.array([ALWAYS, SIGNAL, ALWAYS, NEVER, SIGNAL, ALWAYS, SIGNAL], np.uint8)
    flags = np.array([1, 0, 1, 0, 1, 0, 0], np.uint8)
    cases = [_case(enc, stereo, gate, steps, grid=g, stereo_flags=flags) for g in (1, 2, 16)]
    got, _ = hostmix.run(_encode(cases), "rows_%s_%d_%d" % (enc, stereo, B))
    _compare(got, cases)


@pytest.mark.parametrize("where", ["left", "right", "both"])
def test_edge_samples_in_left_right_and_both(hostmix, where):
    """NaN, the infinities, full scale and just beyond, denormals, -0.0, the rounding ties and every q of every segment (tests/audio_cases.py), placed in left only,
    in right only and in both (different rows in each, so that L and R of a frame differ)."""
    B = 1000
    x = ac.extremes_rows(B)
    zero = np.zeros_like(x)
    left = x if where in ("left", "both") else zero
    right = x[::-1].copy() if where == "both" else (x if where == "right" else zero)
    M = len(x)
    steps = [(left, right, np.ones(M, np.uint8))]
    gate = np.full(M, SIGNAL, np.uint8)
    cases = [_case(enc, True, gate, steps) for enc in ENCODINGS] + [_case(enc, False, gate, steps) for enc in ("s16", "alaw")]
    ref = capi.mixer_gate_reference(gate, M, "s16", True, [(left, right, steps[0][2], np.zeros(M))])[0]
    assert ref["info"]["n_clipped"].sum() >= 6
    got, _ = hostmix.run(_encode(cases), "edges_" + where)
    _compare(got, cases)


def test_first_and_end_are_frames(hostmix):
    """Audio only in right, only in left, in the last frame, too small to leave a q, and nowhere."""
    B = 1000
    left, right = np.zeros((6, B), np.float32), np.zeros((6, B), np.float32)
    right[0, 300], right[0, 301] = 0.25, -0.5      # right alone: frames 300 .. 301
    left[1, 0] = 0.1                               # frame 0
    right[2, B - 1] = 2.0                          # the last frame, clipped
    left[3, 10], right[3, 700] = 1e-6, 0.5         # q = 0 in left: the first frame is right's
    left[4, 255], left[4, 256], right[4, 900] = 0.1, np.nan, -np.inf
    steps = [(left, right, np.ones(6, np.uint8))]
    gate = np.full(6, ALWAYS, np.uint8)
    ref = capi.mixer_gate_reference(gate, 6, "s16", True, [(left, right, steps[0][2], np.zeros(6))])[0]
    assert [(int(r["first"]), int(r["end"])) for r in ref["info"]] == [(300, 302), (0, 1), (B - 1, B), (700, 701), (255, 901), (B, 0)]
    assert ref["info"]["n_clipped"].tolist() == [0, 0, 1, 0, 1, 0]
    cases = [_case(enc, True, gate, steps) for enc in ENCODINGS] + [_case("ulaw", False, gate, steps)]
    got, _ = hostmix.run(_encode(cases), "extent")
    _compare(got, cases)


def test_padded_list_and_counts_out_of_range(hostmix):
    """The pack on a given list: a count beyond max_rows writes max_rows rows, a negative count none; the list's tail holds mixers out of range the kernel must
    never follow (the harness checks the guard rows), and an entry out of range inside the count is clamped, not followed."""
    B = 1000
    left, right = ac.random_rows(9, B, seed=77), ac.random_rows(9, B, seed=78)
    steps = [(left, right, np.ones(9, np.uint8))]
    gate = np.full(9, ALWAYS, np.uint8)
    flags = np.arange(9) % 2
    cases = []
    for enc in ENCODINGS:
        cases.append(_case(enc, True, gate, steps, listed=(9, [0, 2, 4, 8]), max_rows=4, stereo_flags=flags))
        cases.append(_case(enc, True, gate, steps, listed=(2 ** 31 - 1, [1, 7]), max_rows=2, stereo_flags=flags))
        cases.append(_case(enc, False, gate, steps, listed=(-5, [1, 7]), max_rows=2, stereo_flags=flags))
        cases.append(_case(enc, False, gate, steps, listed=(2, [6, 3]), max_rows=6, grid=1, stereo_flags=flags))
    got, _ = hostmix.run(_encode(cases), "listed")
    _compare(got, cases)
    p = _case("s16", True, gate, steps, listed=(2, [0, 8]), max_rows=2, stereo_flags=flags)
    p["listed"] = (2, [12, -3])  # out of range either way: rows 8 and 0 are read, the record keeps what the list said
    got, _ = hostmix.run(_encode([p]), "clamp")
    rows, info = capi.mixer_rows_reference(left, right, "s16", True, [8, 0], flags)
    info["channel"] = [12, -3]
    assert got == struct.pack("<ii", 2, 2) + np.array([12, -3], "<i4").tobytes() + rows.tobytes() + info.tobytes()


def test_two_shapes_under_host_sanitizers(hostmix):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    gate = _mixed_gate(65)
    cases = [_case("alaw", True, gate, _signal_steps(65, 8, 3, seed=5), max_rows=9),
             _case("s16", True, np.full(5, ALWAYS, np.uint8), _signal_steps(5, 2000, 1, seed=8, p_signal=1.0), grid=3, stereo_flags=[1, 0, 0, 1, 1]),
             _case(None, False, np.full(3, ALWAYS, np.uint8), [(ac.extremes_rows(1000)[-3:], ac.extremes_rows(1000)[:3], np.ones(3, np.uint8))], listed=(11, [2, 1]), max_rows=2)]
    got, _ = hostmix.sanitized().run(_encode(cases), "san")
    _compare(got, cases)
