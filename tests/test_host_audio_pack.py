"""The encoder's kernels (csrc/audio_pack.hip) with their wavefront semantics on the CPU: the kernel source compiled for the host through
tests/hostshim_wave64/ (lanes as fibers; shuffles are rendezvous points) into a stand-alone program (tests/host_audio_harness.cpp) that reads rows from a file
and writes what the kernel left; compared byte for byte with the definition in numpy (capi.audio_encode_reference).  It checks the LOGIC of the code the GPU
runs -- the float step, the segment search by leading zeros, the packing of four samples per lane, the row stride of the grid, the record's reduction, the
clamps -- tests/test_gpu_audio_encoding.py is what a GPU says.  The same program built under ASan + UBSan (tests/hostbed.py) runs two of the shapes."""
import struct

import numpy as np
import pytest

import audio_cases as ac
import hostbed

capi = ac.capi


@pytest.fixture(scope="module")
def hostaudio(tmp_path_factory):
    return hostbed.program(tmp_path_factory, "host_audio", "host_audio_harness.cpp", extra=["-ffp-contract=off"])


def _case(fmt, rows, count=None, max_rows=None, grid=2, index=None):
    """index: the gate's form (row r = channel index[r], padded to max_rows with a channel out of range, which the kernel must never follow)."""
    rows = np.ascontiguousarray(rows, np.float32)
    n_ch, B = rows.shape
    if index is None:
        count = n_ch if count is None else count
        max_rows = max(n_ch, 1) if max_rows is None else max_rows
    else:
        count = len(index) if count is None else count
        max_rows = max(len(index), 1) if max_rows is None else max_rows
        index = (list(index) + [n_ch + 1000] * max_rows)[:max_rows]
    return dict(fmt=fmt, rows=rows, B=B, n_ch=n_ch, count=count, max_rows=max_rows, grid=grid, index=index)


def _encode(cases):
    blob = struct.pack("<i", len(cases))
    for p in cases:
        blob += struct.pack("<7i", capi.AUDIO_ENCODINGS[p["fmt"]], p["B"], p["n_ch"], p["max_rows"], p["count"], p["grid"], 0 if p["index"] is None else 1)
        if p["index"] is not None:
            blob += np.array(p["index"], "<i4").tobytes()
        blob += p["rows"].tobytes()
    return blob


def _want(p):
    kept = min(max(p["count"], 0), p["max_rows"])
    src = p["rows"][:kept] if p["index"] is None else p["rows"][p["index"][:kept]]
    audio, info = capi.audio_encode_reference(src.reshape(kept, p["B"]), p["fmt"])
    if p["index"] is not None:
        info["channel"] = p["index"][:kept]
    return struct.pack("<i", kept) + audio.tobytes() + info.tobytes()


def _compare(got, cases):
    at = 0
    for n, p in enumerate(cases):
        w = _want(p)
        have = got[at:at + len(w)]
        if have != w:
            kept = struct.unpack("<i", w[:4])[0]
            a = len(w) - 16 * kept
            what = "row count" if have[:4] != w[:4] else "audio bytes" if have[4:a] != w[4:a] else "records"
            detail = ""
            if what == "records":
                detail = " got %r want %r" % (np.frombuffer(have[a:], capi.AUDIO_ROW_DTYPE)[:4].tolist(), np.frombuffer(w[a:], capi.AUDIO_ROW_DTYPE)[:4].tolist())
            raise AssertionError("case %d (%s, B %d, %d rows of %d, grid %d): %s differ%s" % (n, p["fmt"], p["B"], p["count"], p["max_rows"], p["grid"], what, detail))
        at += len(w)
    assert at == len(got), "the harness wrote %d bytes more than the reference accounts for" % (len(got) - at)


@pytest.mark.parametrize("B", [1000, 2000])
@pytest.mark.parametrize("fmt", ac.FORMATS)
def test_every_q_specials_and_ties(hostaudio, fmt, B):
    """Every code of every segment, clipping, NaN, the infinities, denormals, -0.0 and the ties, as dense rows; two workgroups stride over the 34 or 67 rows."""
    rows = ac.extremes_rows(B)
    audio, info = capi.audio_encode_reference(rows, fmt)
    assert info["n_clipped"].sum() >= 6 and len(np.unique(audio)) >= (255 if fmt != "s16" else 65535)
    cases = [_case(fmt, rows)]
    got, _ = hostaudio.run(_encode(cases), "extremes_%s_%d" % (fmt, B))
    _compare(got, cases)


@pytest.mark.parametrize("B", [1000, 2000])
def test_row_counts_the_empty_case_and_the_stride(hostaudio, B):
    """0, 1 and 5 rows on a grid of two workgroups, dense and through a list; the list's channels are out of order and repeat."""
    rows = ac.random_rows(7, B, seed=B)
    cases = []
    for fmt in ac.FORMATS:
        for n in (0, 1, 5):
            cases.append(_case(fmt, rows, count=n, max_rows=7))
            cases.append(_case(fmt, rows, index=[6, 0, 3, 3, 5][:n], max_rows=6))
    got, _ = hostaudio.run(_encode(cases), "counts_%d" % B)
    _compare(got, cases)


def test_count_beyond_max_rows_writes_nothing_behind_them(hostaudio):
    """The gate counts more channels than it lists: max_rows rows are written, the guard rows behind the buffers stay as they were (the harness checks them),
    and a channel out of range in the list is clamped, not followed."""
    rows = ac.random_rows(9, 1000, seed=77)
    cases = []
    for fmt in ac.FORMATS:
        cases.append(_case(fmt, rows, index=[0, 2, 4, 8], count=9, max_rows=4))
        cases.append(_case(fmt, rows, index=[1, 7], count=2 ** 31 - 1, max_rows=2))
        cases.append(_case(fmt, rows, index=[1, 7], count=-5, max_rows=2))
        cases.append(_case(fmt, rows, count=9, max_rows=3, grid=1))
    got, _ = hostaudio.run(_encode(cases), "overflow")
    _compare(got, cases)
    p = _case("s16", rows, index=[0, 8], max_rows=2)
    p["index"] = [12, -3]  # out of range either way: rows 8 and 0 are read, the record keeps what the list said
    q = dict(p, index=[8, 0])
    got, _ = hostaudio.run(_encode([p]), "clamp")
    want = _want(q)
    kept_audio = len(want) - 32
    assert got[:kept_audio] == want[:kept_audio]
    assert np.frombuffer(got[kept_audio:], capi.AUDIO_ROW_DTYPE)["channel"].tolist() == [12, -3]


@pytest.mark.parametrize("B", [1000, 2000])
def test_first_and_end(hostaudio, B):
    """All zero; one sample at index 0; one at B - 1; both; one in the last lane's last pass; a sample too small to leave a non-zero q."""
    rows = np.zeros((7, B), np.float32)
    rows[1, 0] = 0.25
    rows[2, B - 1] = -0.25
    rows[3, 0], rows[3, B - 1] = 1e-3, 2.0
    rows[4, B - 4] = 0.5
    rows[5, 300] = 1e-6  # q = 0
    rows[6, 255], rows[6, 256], rows[6, 700] = 0.1, np.nan, -np.inf
    _, info = capi.audio_encode_reference(rows, "s16")
    assert [(int(r["first"]), int(r["end"])) for r in info] == [(B, 0), (0, 1), (B - 1, B), (0, B), (B - 4, B - 3), (B, 0), (255, 701)]
    assert info["n_clipped"].tolist() == [0, 0, 0, 1, 0, 0, 1]
    cases = [_case(fmt, rows) for fmt in ac.FORMATS]
    got, _ = hostaudio.run(_encode(cases), "extent_%d" % B)
    _compare(got, cases)


def test_seeded_random_rows(hostaudio):
    """200 rows of mixed scale through a shuffled list, two workgroups."""
    rows = ac.random_rows(200, 1000, seed=9)
    index = np.random.default_rng(4).permutation(200).tolist()
    cases = [_case(fmt, rows, index=index) for fmt in ac.FORMATS]
    _, info = capi.audio_encode_reference(rows, "s16")
    assert (info["n_clipped"] > 0).any() and (info["peak"] == 0).any() and (info["first"] > 0).any()
    got, _ = hostaudio.run(_encode(cases), "random")
    _compare(got, cases)


def test_two_shapes_under_host_sanitizers(hostaudio):
    """The stand-alone program built under ASan + UBSan: the same bytes, no report."""
    rows = ac.random_rows(6, 2000, seed=3)
    cases = [_case("ulaw", ac.extremes_rows(1000)[-3:]), _case("s16", rows, index=[5, 1, 1, 0], count=11, max_rows=4), _case("alaw", rows, count=5, max_rows=6)]
    got, _ = hostaudio.sanitized().run(_encode(cases), "san")
    _compare(got, cases)
