"""The output decimation's kernels (csrc/audio_decimate.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles and the wavefront's LDS exchanges are rendezvous points) into a stand-alone program
(tests/host_decimate_harness.cpp) that reads rows from a file and writes what the kernel left; compared byte for byte with the definition in numpy
(capi.audio_decimate_reference, the history carried by tests/decimation_cases.Model).  It checks the LOGIC of the code the GPU runs -- the deinterleaved row in
LDS, the tap pairs against whole and straddling dwords, the history's load, write-back and stamp, the row stride of the grid, the record's reduction, the clamps
-- with the plain-integer form of the pair product (the GPU build takes v_dot2_i32_i16 for it); tests/test_gpu_audio_decimation.py is what a GPU says.  The same
program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import struct

import numpy as np
import pytest

import audio_cases as ac
import decimation_cases as dc
import hostbed

capi = ac.capi
H = dc.H


@pytest.fixture(scope="module")
def hostdec(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_decimate", "host_decimate_harness.cpp", extra=["-ffp-contract=off"])


def _dense(fmt, rows, count=None, max_rows=None, grid=2, history=None):
    """airband_hip_decimate_audio()'s form, one step: row r is source row r"""
    rows = np.ascontiguousarray(rows, np.float32)
    n_ch, B = rows.shape
    count = n_ch if count is None else count
    return dict(fmt=fmt, B=B, n_ch=n_ch, max_rows=max(n_ch, 1) if max_rows is None else max_rows, grid=grid, mode=0 if history is None else 1, history=history,
                steps=[dict(count=count, index=None, rows=rows)])


def _listed(fmt, steps, max_rows, grid=2):
    """the gate's form: steps = [(rows [n_ch][B], index, count or None)]; the list is padded to max_rows with a channel out of range, which the kernel must
    never follow"""
    n_ch, B = steps[0][0].shape
    out = []
    for rows, index, count in steps:
        count = len(index) if count is None else count
        out.append(dict(count=count, index=(list(index) + [n_ch + 1000] * max_rows)[:max_rows], rows=np.ascontiguousarray(rows, np.float32)))
    return dict(fmt=fmt, B=B, n_ch=n_ch, max_rows=max_rows, grid=grid, mode=2, history=None, steps=out)


def _encode(cases):
    blob = struct.pack("<i", len(cases))
    for p in cases:
        blob += struct.pack("<7i", capi.AUDIO_ENCODINGS[p["fmt"]], p["B"], p["n_ch"], p["max_rows"], p["grid"], p["mode"], len(p["steps"]))
        if p["mode"] == 1:
            blob += np.ascontiguousarray(p["history"], "<i2").tobytes()
        for s in p["steps"]:
            blob += struct.pack("<i", s["count"])
            if p["mode"] == 2:
                blob += np.array(s["index"], "<i4").tobytes()
            blob += s["rows"].tobytes()
    return blob


def _want(p):
    """[(what, bytes)] in the order of the results file"""
    out = []
    n_ch = p["n_ch"]
    model = dc.Model(n_ch, p["fmt"])
    hist = None if p["mode"] != 1 else np.array(p["history"], "<i2")
    stamp = np.zeros(n_ch, "<u4")
    for k, s in enumerate(p["steps"]):
        kept = min(max(s["count"], 0), p["max_rows"])
        if p["mode"] == 2:
            said = np.array(s["index"][:kept], np.int64)
            src = np.clip(said, 0, n_ch - 1)
            audio, info = model.step(src, s["rows"][src].reshape(kept, p["B"]))
            info["channel"] = said
            stamp[src] = k + 1
        else:
            audio, info, new = capi.audio_decimate_reference(s["rows"][:kept].reshape(kept, p["B"]), p["fmt"], None if hist is None else hist[:kept])
            if hist is not None:
                hist[:kept] = new
        out += [("row count of step %d" % k, struct.pack("<i", kept)), ("audio bytes of step %d" % k, audio.tobytes()), ("records of step %d" % k, info.tobytes())]
    if p["mode"] == 1:
        out.append(("histories", hist.tobytes()))
    if p["mode"] == 2:
        out += [("histories", model.hist.tobytes()), ("stamps", stamp.tobytes())]
    return out


def _compare(got, cases):
    at = 0
    for n, p in enumerate(cases):
        want = _want(p)
        last = len(p["steps"])
        for i, (what, w) in enumerate(want):
            have = got[at:at + len(w)]
            if what == "histories" and p["mode"] == 2:
                # a history counts only if its stamp is the last step's: what the next step would read
                stamps = np.frombuffer(got[at + len(w):at + len(w) + 4 * p["n_ch"]], "<u4")
                raw = np.frombuffer(have, "<i2").reshape(p["n_ch"], H)
                have = np.where((stamps == last)[:, None], raw, 0).astype("<i2").tobytes()
            if have != w:
                detail = ""
                if what.startswith("records"):
                    detail = " got %r want %r" % (np.frombuffer(have, capi.AUDIO_ROW_DTYPE)[:4].tolist(), np.frombuffer(w, capi.AUDIO_ROW_DTYPE)[:4].tolist())
                raise AssertionError("case %d (%s, B %d, mode %d, %d rows at most, grid %d): %s differ%s" % (n, p["fmt"], p["B"], p["mode"], p["max_rows"], p["grid"], what, detail))
            at += len(w)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


@pytest.mark.parametrize("B", [1000, 2000])
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_every_q_specials_ties_and_the_output_clamp(hostdec, fmt, B):
    """audio_cases.extremes_rows -- every q, clipping, NaN, the infinities, denormals, -0.0, the ties -- and the saturating pattern, as dense rows with a random
    history; two workgroups stride over the rows."""
    rows = np.concatenate([ac.extremes_rows(B), dc.saturating_rows(4, B)])
    hist = np.random.default_rng(B).integers(-32767, 32768, (len(rows), H)).astype("<i2")
    _, info, _ = capi.audio_decimate_reference(rows, fmt, hist)
    assert info["n_clipped"].sum() >= 10 and (info["peak"] == 32767).any()
    cases = [_dense(fmt, rows, history=hist), _dense(fmt, rows[-6:])]
    got, _ = hostdec.run(_encode(cases), "extremes_%s_%d" % (fmt, B))
    _compare(got, cases)


@pytest.mark.parametrize("B", [1000, 2000])
def test_row_counts_the_empty_case_and_the_stride(hostdec, B):
    """0, 1 and 5 rows on a grid of two workgroups, dense and through a shuffled list."""
    rows = ac.random_rows(7, B, seed=B)
    cases = []
    for fmt in ac.FORMATS:
        for n in (0, 1, 5):
            cases.append(_dense(fmt, rows, count=n, max_rows=7))
            cases.append(_listed(fmt, [(rows, [6, 0, 3, 2, 5][:n], None)], max_rows=6))
    got, _ = hostdec.run(_encode(cases), "counts_%d" % B)
    _compare(got, cases)


@pytest.mark.parametrize("B", [1000, 2000])
def test_count_beyond_max_rows_writes_nothing_behind_them(hostdec, B):
    """The gate counts more channels than it lists: max_rows rows are written, the guard zones behind the rows, records, histories and stamps stay as they were
    (the harness checks them), and a channel out of range in the list is clamped, not followed."""
    rows = ac.random_rows(9, B, seed=77)
    cases = []
    for fmt in ac.FORMATS:
        cases.append(_listed(fmt, [(rows, [0, 2, 4, 8], 9)], max_rows=4))
        cases.append(_listed(fmt, [(rows, [1, 7], 2 ** 31 - 1)], max_rows=2))
        cases.append(_listed(fmt, [(rows, [1, 7], -5)], max_rows=2))
        cases.append(_dense(fmt, rows, count=9, max_rows=3, grid=1))
        p = _listed(fmt, [(rows, [0, 8], None), (rows[::-1], [0, 8], None)], max_rows=2)
        p["steps"][0]["index"] = p["steps"][1]["index"] = [12, -3]  # out of range either way: rows 8 and 0 are read, the record keeps what the list said
        cases.append(p)
    got, _ = hostdec.run(_encode(cases), "overflow_%d" % B)
    _compare(got, cases)


@pytest.mark.parametrize("B", [1000, 2000])
def test_channels_leave_and_rejoin_the_list(hostdec, B):
    """Consecutive steps: channels 1 and 4 stay listed throughout (one uninterrupted convolution), 0 and 6 leave and come back (from zeros), 3 joins late, 5 is
    never listed.  No row is silent, so a history that was carried where it should have been zeroed -- or the reverse -- shows in the first 23 outputs."""
    rng = np.random.default_rng(B)
    steps = []
    for index in ([0, 1, 4, 6], [1, 2, 4], [0, 1, 3, 4, 6], [1, 3, 4, 6]):
        rows = (rng.standard_normal((7, B)) * 0.3 + 0.2).astype(np.float32)
        steps.append((rows, index, None))
    cases = [_listed(fmt, steps, max_rows=5, grid=g) for fmt in ac.FORMATS for g in (1, 3)]
    a = dc.Model(7, "s16")
    outs = [a.step(idx, rows[idx])[0] for rows, idx, _ in steps]
    fresh = capi.audio_decimate_reference(steps[2][0][[0]], "s16")[0]
    assert np.array_equal(outs[2][0], fresh[0])  # channel 0 came back from zeros
    carried = capi.audio_decimate_reference(steps[2][0][[1]], "s16")[0]
    assert not np.array_equal(outs[2][1], carried[0])  # channel 1 did not
    got, _ = hostdec.run(_encode(cases), "rejoin_%d" % B)
    _compare(got, cases)


def test_two_shapes_under_host_sanitizers(hostdec):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    rows = ac.random_rows(6, 2000, seed=3)
    small = np.concatenate([ac.extremes_rows(1000)[-2:], dc.saturating_rows(2, 1000)])
    hist = np.random.default_rng(1).integers(-32767, 32768, (4, H)).astype("<i2")
    cases = [_dense("ulaw", small, history=hist), _listed("s16", [(rows, [1, 4, 5], 11), (rows[::-1], [0, 1, 5], None)], max_rows=3), _dense("alaw", rows, count=5, max_rows=6)]
    got, _ = hostdec.sanitized().run(_encode(cases), "san")
    _compare(got, cases)
