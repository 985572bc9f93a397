"""The coefficient tables the DEVICE builds, read back (airband_hip_read_tables) and held against an exact reference (tests/table_reference.py).

The matrix-core channelizers contract the samples with tables that have each channel's bin baked in.  Three builders make them: the host (csrc/params.cpp; pinned on
the CPU by tests/test_dft_tables.py), build_tables_kernel (csrc/misc_kernels.hip: every shared table past the host's first AIRBAND_HIP_HOST_TABLES_MAX = 4 096) and
retune_kernel (same file: private tables, at start-up by copying column pairs from the home table, later by rebuilding the pair of a channel AFC has moved).  With the
environment variable at 0 ... 3 a fleet of nine dongles goes through the device builder.

THE FLEET (fleet()): seven dongles of eight channels on pairwise distinct plans (channel c of dongle d sits ((d >> 2c) & 3) bins above the BASELINE plan's), one of
five channels (a short group: columns 5 ... 7 unused), one of eleven (two groups, the second short): ten shared tables.

What maps to which test (builder; window pieces; formats; launch shape of build_tables_kernel = tables in [first, first + n), four to a workgroup):
  test_device_built_tables ............ build_tables_kernel; 1 (fft 256, 512), 2, 4, 8, 16 pieces; u8, s8, CS16 and one wide-hop CS16 handle (fft 1024 at 10 MS/s);
                                        first = 2, n = 8: two whole workgroups.  Digits, rounding, offset correction, unused columns, the skipped top digit
  test_partial_last_workgroup ......... build_tables_kernel; 2 pieces; u8; first = 0 / 1 / 3, n = 10 / 9 / 7: a last workgroup of 2 / 1 / 3 tables (first = 0: no
                                        host image at all)
  test_device_against_host ............ both shared builders; 1 and 4 pieces; u8; the same invariants on the host's tables, at most one unit between the two
  test_private_tables_over_device_built_homes ... retune_kernel's start-up copy behind build_tables_kernel on one stream; 1 piece; u8 (int8 tables) and CF32 (float
                                        tables, host-built homes); three AFC dongles and two plain ones
  test_moved_column ................... retune_kernel's build_column_pair (u8: 1 and 4 pieces) and build_column_pair_f32 (CF32, fft 1024), its copies of the unmoved
                                        columns, and the work item's switch to the private table and back
  test_end_to_end_through_device_built_tables ... build_tables_kernel -> channelizer -> stage 2: u8 at fft 512, 1024, 8192 (two-pass partial sums), CS16 at fft 2048,
                                        u8 wide hops (6 MS/s); every channel's stage-1 bins, audio, axcindicate, squelch trace and counters against the oracle
  test_error_paths .................... airband_hip_read_tables on a wavefront-FFT handle, past the last table, with a NULL buffer, after release

Bars.  Rounding: |v - x| <= 0.5 + 1e-6 table units (|x| < 2^23, a double's ulp there is 2^-29 = 1.9e-9 units; sincospi and two multiplications stay far below
1e-6).  Offset correction: equality (integer sums below 2^53).  CF32: half a float32 ulp of the exact value plus 1e-12 relative (a double product rounded once).
Derived, not measured.  Stage-1 bins: tests/test_gpu_afc.py's AWAY_BAR (every column here is device-built).

Measured, for information (test_device_against_host prints it; no bar): the share of coefficients on which the device's tables differ from the host's by one
unit.  MI355X, 2026-10-20: 0 of 147 456 at fft 512 and 0 of 589 824 at fft 2048 -- the device's sincospi and the host's libm rounded every coefficient of the fleet
alike (a difference needs an exact value within ~1e-9 of a half, a few in a billion).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import pyoracle
import table_reference as tr
from test_gpu_afc import AWAY_BAR, HOME_BAR

pytestmark = pytest.mark.gpu

ENV = "AIRBAND_HIP_HOST_TABLES_MAX"
EXTRA_OFFSETS_HZ = [125_000, -125_000, 625_000]   # channels 8 ... 10 of the eleven-channel dongle


def fleet(pkg, sfmt, fft_log, sample_rate):
    """The nine dongles (see the module docstring) and bins[d] = the bin of every channel by the reference's rule (src/config.cpp:666-667)."""
    capi, n_fft = pkg.capi, 1 << fft_log
    bin_hz = sample_rate // n_fft

    def tweak(d, ch):
        if d == 7:
            del ch[5:]
        if d == 8:
            ch.extend(dict(ch[0], frequency=helpers.sg.CENTERFREQ + off) for off in EXTRA_OFFSETS_HZ)
        for c, sh in zip(ch, pkg.siggen.plan_shift_bins(d, 16, len(ch))):
            c["frequency"] += sh * bin_hz

    devices, _ = helpers.plan_devices(9, False, tweak)
    for d, dev in enumerate(devices):
        dev.update(sample_rate=sample_rate, sfmt=sfmt, fullscale=127.5 * (200.0 if d % 2 == 0 else 50.0) if sfmt == capi.SFMT_S16 else 0.0)
    bins = [[helpers.afc_reference_bin(c["frequency"], helpers.sg.CENTERFREQ, sample_rate, n_fft) for c in dev["channels"]] for dev in devices]
    return devices, bins


def expected_sets(bins):
    """The sharing rule (csrc/params.cpp): one table per distinct group of up to eight bins, numbered as first met, dongle-major.  Returns (keys, home table per item)."""
    keys, home = [], []
    for b in bins:
        for g in range(0, len(b), 8):
            key = tuple(b[g:g + 8])
            if key not in keys:
                keys.append(key)
            home.append(keys.index(key))
    return keys, home


@functools.lru_cache(maxsize=None)
def exact_pair(n_fft, bin_, scale=tr.COEF_SCALE):
    x = tr.exact_column_pair(n_fft, bin_, scale)
    x.setflags(write=False)
    return x


def check_int8_column_pair(n_fft, raw, corr, c, bin_, what):
    """Column pair c of one raw table against the exact coefficients of `bin_` (-1: unused): digits, rounding, offset correction."""
    d = tr.unpack_int8_digits(raw, n_fft)[..., 2 * c:2 * c + 2]   # [piece][t][k][half]
    v = d[:, 0] + 256 * d[:, 1] + 65536 * d[:, 2]
    if bin_ < 0:
        assert not d.any(), "%s column pair %d is unused and not zero" % (what, c)
        assert not corr[:, 2 * c:2 * c + 2].any(), "%s column pair %d is unused, its correction is not zero" % (what, c)
        return v
    assert d.min() >= -128 and d.max() <= 127
    assert np.array_equal(np.moveaxis(tr.balanced_digits(v), -1, 1), d), "%s column pair %d: the bytes are not the balanced digits of their value" % (what, c)
    x = tr.by_piece(exact_pair(n_fft, bin_), n_fft)
    err = np.abs(v.astype(tr.REAL) - x)
    assert float(err.max()) <= 0.5 + 1e-6, "%s column pair %d (bin %d): a coefficient is %.9f units from the exact value" % (what, c, bin_, float(err.max()))
    want = 0.5 * v.sum(axis=1).astype(np.float64)                  # [piece][half]; integer sums below 2^53: exact
    assert np.array_equal(corr[:, 2 * c:2 * c + 2], want), "%s column pair %d (bin %d): correction %r, half the column sums are %r" % (what, c, bin_, corr[:, 2 * c:2 * c + 2].tolist(), want.tolist())
    return v


def check_int8_table(n_fft, raw, corr, bins8, what):
    assert np.array_equal(tr.pack_int8(tr.unpack_int8(raw, n_fft), n_fft), np.asarray(raw).view(np.int8)), "%s: recomposed and decomposed again, the bytes differ" % what
    return np.concatenate([check_int8_column_pair(n_fft, raw, corr, c, int(bins8[c]), what) for c in range(8)], axis=-1)


def check_top_digit(n_fft, got):
    """info says the kernel skips the top digit in the outer k-steps (KS / 8 at either end: 0, 1, 14, 15 of 16): then it is zero there in EVERY table."""
    if not got["info"]["edge_hi_zero"]:
        return False
    _, K, KS, _ = tr.int8_geometry(n_fft)
    edge = KS // 8
    for t, raw in enumerate(got["tables"]):
        top = tr.unpack_int8_digits(raw, n_fft)[:, 2].reshape(-1, KS, 64, 16)
        assert not top[:, :edge].any() and not top[:, KS - edge:].any(), "table %d: the top digit the kernel skips is not zero" % t
    return True


def check_structure(got, bins, n_host):
    """Counts, bset_bin and the work items of a handle on the fleet's `bins` without private tables."""
    keys, home = expected_sets(bins)
    info = got["info"]
    assert (info["n_shared_bsets"], info["n_bsets"], info["n_items"]) == (len(keys), len(keys), len(home)), info
    assert info["n_host_bsets"] == n_host, "the handle was meant to have %d host-built tables: %r" % (n_host, info)
    want = np.full((len(keys), 8), -1, np.int32)
    for t, key in enumerate(keys):
        want[t, :len(key)] = key
    assert np.array_equal(got["bset_bin"], want)
    assert np.array_equal(got["item_home"], home) and np.array_equal(got["item_bset"], home) and np.array_equal(got["item_private"], home)
    return keys


def read_fleet_tables(pkg, monkeypatch, sfmt_name, fft_log, sample_rate, wave_rate, host_max, flags=0):
    capi = pkg.capi
    if host_max is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(host_max))
    devices, bins = fleet(pkg, getattr(capi, sfmt_name), fft_log, sample_rate)
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=flags) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8", hip.channelizer_reason()
        got = hip.read_tables()
    assert got["info"]["channelizer"] == "dft_mfma_i8"
    pieces, _, _, nbytes = tr.int8_geometry(1 << fft_log)
    assert (got["info"]["pieces_per_table"], got["info"]["bytes_per_table"]) == (pieces, nbytes)
    keys = check_structure(got, bins, 10 if host_max is None else host_max)
    assert len(keys) == 10
    return got, keys


def check_fleet_tables(n_fft, got, keys, first, last, what):
    v = {}
    for t in range(first, last):
        v[t] = check_int8_table(n_fft, got["tables"][t], got["corr"][t], got["bset_bin"][t], "%s table %d" % (what, t))
    check_top_digit(n_fft, got)
    return v


# ---- (a) every device-built shared table --------------------------------------------------------------------------------------------------------------
TABLE_CASES = [(f, n, 2_560_000, 8000, 0) for n in (8, 9, 10, 11, 12, 13) for f in ("SFMT_U8", "SFMT_S8", "SFMT_S16")] + [("SFMT_S16", 10, 10_000_000, 8000, "wide")]


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate,wide", TABLE_CASES, ids=lambda v: str(v))
def test_device_built_tables(pkg, built, monkeypatch, sfmt_name, fft_log, sample_rate, wave_rate, wide):
    """AIRBAND_HIP_HOST_TABLES_MAX=2: tables 2 ... 9 of the fleet come from build_tables_kernel (first = 2).  Every one of them, every piece, every column: the bytes
    are the balanced digits of their value, the value is within 0.5 + 1e-6 of the exact coefficient, corr is half the column sum exactly, unused columns (the five-
    and eleven-channel dongles) are zero with zero corr, bset_bin is the plan's bins; and where the handle says the kernel skips the top digit, it is zero in the
    outer k-steps of every table."""
    flags = pkg.capi.FLAG_WIDE_HOPS if wide else 0
    got, keys = read_fleet_tables(pkg, monkeypatch, sfmt_name, fft_log, sample_rate, wave_rate, 2, flags)
    assert any(len(k) < 8 for k in keys[2:]), "no short group among the device-built tables"
    check_fleet_tables(1 << fft_log, got, keys, 2, 10, "%s fft %d" % (sfmt_name, 1 << fft_log))
    print("fft %d %s: edge_hi_zero %s" % (1 << fft_log, sfmt_name, got["info"]["edge_hi_zero"]))


@pytest.mark.parametrize("host_max", [0, 1, 3])
def test_partial_last_workgroup(pkg, built, monkeypatch, host_max):
    """Ten shared tables, 0 / 1 / 3 of them the host's: the builder's last workgroup holds 2 / 1 / 3 tables, `first` is 0 / 1 / 3; at 0 the host image is empty.  fft 1024.
    The host's tables pass the same checks, and the tables next to the last one are exactly as large as the geometry says (a wavefront past `n` writes nothing)."""
    got, keys = read_fleet_tables(pkg, monkeypatch, "SFMT_U8", 10, 2_560_000, 8000, host_max)
    check_fleet_tables(1024, got, keys, 0, 10, "host_max %d" % host_max)


# ---- (b) device against host ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_log", [9, 11])
def test_device_against_host(pkg, built, monkeypatch, fft_log):
    """The fleet once with every table from the host (variable unset) and once with every table from the device (0): the host's tables satisfy the same invariants, and no
    coefficient differs by more than one unit between the two.  Prints the share that differs (information, no bar)."""
    n_fft = 1 << fft_log
    host, keys = read_fleet_tables(pkg, monkeypatch, "SFMT_U8", fft_log, 2_560_000, 8000, None)
    dev, _ = read_fleet_tables(pkg, monkeypatch, "SFMT_U8", fft_log, 2_560_000, 8000, 0)
    vh = check_fleet_tables(n_fft, host, keys, 0, 10, "host-built")
    vd = check_fleet_tables(n_fft, dev, keys, 0, 10, "device-built")
    assert host["info"]["edge_hi_zero"] == dev["info"]["edge_hi_zero"] or not dev["info"]["edge_hi_zero"]   # the device side decides on the window alone: never bolder than the host
    differ = total = 0
    for t in range(10):
        used = np.repeat(np.asarray(keys[t] + (-1,) * (8 - len(keys[t]))) >= 0, 2)
        diff = np.abs(vh[t] - vd[t])[..., used]
        assert diff.max() <= 1, "table %d: host and device differ by %d units" % (t, diff.max())
        differ += int((diff != 0).sum())
        total += diff.size
    print("device-versus-host fft %d: %d of %d coefficients differ by one unit (share %.3g)" % (n_fft, differ, total, differ / total))


# ---- (c) private tables over device-built homes -----------------------------------------------------------------------------------------------------------
def private_case(pkg, sfmt):
    """helpers.afc_case(3) plus two plain dongles on plans of their own: homes 0 (the AFC dongles share it), 1, 2; private tables 3, 4, 5."""
    devices, _ = helpers.afc_case(3)

    def tweak(d, ch):
        for c, sh in zip(ch, pkg.siggen.plan_shift_bins(d + 1, 16, len(ch))):
            c["frequency"] += sh * (helpers.sg.SAMPLE_RATE // 512)

    devices += helpers.plan_devices(2, False, tweak)[0]
    for dev in devices:
        dev.update(sfmt=sfmt)
    bins = [[helpers.afc_reference_bin(c["frequency"], helpers.sg.CENTERFREQ, helpers.sg.SAMPLE_RATE, 512) for c in dev["channels"]] for dev in devices]
    return devices, bins


def check_f32_column_pair(n_fft, tab, c, bin_, what):
    """Each float of column pair c is the exact value rounded: within half a float32 ulp of it plus 1e-12 relative (a double product rounded once to float)."""
    f = tr.unpack_f32(tab, n_fft)[:, 2 * c:2 * c + 2].astype(tr.REAL)
    x = exact_pair(n_fft, bin_, 1.0)
    ax = np.abs(x).astype(np.float64)
    _, e = np.frexp(ax)
    half_ulp = np.ldexp(0.5, np.maximum(e - 24, -149))
    miss = np.abs(f - x) - (half_ulp + 1e-12 * ax)
    assert float(miss.max()) <= 0, "%s column pair %d (bin %d): a float is %.3g beyond half an ulp of the exact value" % (what, c, bin_, float(miss.max()))


@pytest.mark.parametrize("sfmt_name", ["SFMT_U8", "SFMT_F32"])
def test_private_tables_over_device_built_homes(pkg, built, monkeypatch, sfmt_name):
    """AIRBAND_HIP_HOST_TABLES_MAX=0: every home table comes from build_tables_kernel and retune_kernel copies the private tables from them right behind it, on the same
    stream.  After prepare(): each private table equals its home table byte for byte (corr included), bset_bin is filled with the base bins, every work item reads its
    home table.  CF32: the same for the float tables (whose homes the host builds), and the home tables themselves are the exact values rounded to float."""
    capi = pkg.capi
    monkeypatch.setenv(ENV, "0")
    f32 = sfmt_name == "SFMT_F32"
    devices, bins = private_case(pkg, getattr(capi, sfmt_name))
    with pkg.AirbandHip(devices, wave_rate=16000) as hip:
        assert hip.channelizer_name() == ("dft_mfma_f32" if f32 else "dft_mfma_i8")
        got = hip.read_tables()
    info = got["info"]
    assert (info["n_shared_bsets"], info["n_bsets"], info["n_items"]) == (3, 6, 5), info
    assert info["n_host_bsets"] == (3 if f32 else 0), info
    assert got["item_home"].tolist() == [0, 0, 0, 1, 2] and got["item_private"].tolist() == [3, 4, 5, 1, 2]
    assert got["item_bset"].tolist() == [0, 0, 0, 1, 2], "every channel starts on its base bin: every work item reads its home table"
    assert np.array_equal(got["bset_bin"][:3], [bins[0], bins[3], bins[4]])
    for t in range(3):
        for c in range(8):
            if f32:
                check_f32_column_pair(512, got["tables"][t], c, bins[[0, 3, 4][t]][c], "home table %d" % t)
        if not f32:
            check_int8_table(512, got["tables"][t], got["corr"][t], got["bset_bin"][t], "home table %d" % t)
    assert np.abs(got["tables"][0]).max() > 0
    for t in (3, 4, 5):
        assert np.array_equal(got["bset_bin"][t], bins[0]), "private table %d: bset_bin %r" % (t, got["bset_bin"][t].tolist())
        assert np.array_equal(got["tables"][t].view(np.uint8), got["tables"][0].view(np.uint8)), "private table %d is not its home table" % t
        assert np.array_equal(got["corr"][t], got["corr"][0])


# ---- (d) a moved column ---------------------------------------------------------------------------------------------------------------------------------------
MOVED = [("SFMT_U8", 9, 2_000_000, 16000), ("SFMT_U8", 11, 2_400_000, 16000), ("SFMT_F32", 10, 2_560_000, 16000)]   # points of tests/test_gpu_afc.py's MATRIX
MOVED_BATCHES = 7   # the transmitters key for two batches out of five: a move and the return


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate", MOVED, ids=lambda v: str(v))
def test_moved_column(pkg, built, monkeypatch, sfmt_name, fft_log, sample_rate, wave_rate):
    """Two dongles of tests/test_gpu_afc.py's matrix plan (they share one home table, device-built on the int8 path).  After every batch the handle's bins are the
    oracle's, and each dongle's private table holds: for a channel away from its base bin the column pair of the NEW bin (the checks of test_device_built_tables;
    CF32: half a float32 ulp), for every other channel the home table's bytes; the work item reads the private table while a channel is away and the home table
    again once the whole group is back (the fft 512 streams bring single channels home within these batches, never all eight of a dongle at once: there the copy
    home of the returned channel's column pair is what is checked, the switch back at fft 2048 and on CF32)."""
    capi, n_fft = pkg.capi, 1 << fft_log
    f32 = sfmt_name == "SFMT_F32"
    monkeypatch.setenv(ENV, "0")
    case = helpers.afc_format_case(pkg, getattr(capi, sfmt_name), fft_log, sample_rate, wave_rate, [helpers.afc_plan(8)] * 2, MOVED_BATCHES)
    base = np.array(case["base"])
    assert case["ups"] + case["downs"] > 0 and case["returns"] > 0, "the streams were meant to move channels and bring them home"
    away_seen = back_seen = moved_pairs = returned_pairs = 0
    was_away = [False, False]
    been_away = np.zeros((2, 8), bool)
    with pkg.AirbandHip(case["devices"], wave_rate=wave_rate, fft_log=fft_log) as hip:
        assert hip.channelizer_name() == ("dft_mfma_f32" if f32 else "dft_mfma_i8")
        pos = [0, 0]
        for b in range(MOVED_BATCHES):
            for d, iq in enumerate(case["iq"]):
                pos[d] += hip.submit(d, iq.view(np.uint8)[pos[d]:])
            assert hip.process()
            stats = hip.collect(stats=True)["stats"]
            got = hip.read_tables()
            assert got["info"]["n_shared_bsets"] == 1 and got["info"]["n_bsets"] == 3 and got["item_private"].tolist() == [1, 2] and got["item_home"].tolist() == [0, 0]
            for d in range(2):
                now = np.array([s["bin"] for s in stats[8 * d:8 * d + 8]])
                assert np.array_equal(now, case["ref"][d]["bin"][b]), "batch %d dongle %d: bins %r, oracle %r" % (b, d, now.tolist(), case["ref"][d]["bin"][b].tolist())
                t = 1 + d
                what = "batch %d private table %d" % (b, t)
                assert np.array_equal(got["bset_bin"][t], now), "%s: bset_bin %r, the channels are on %r" % (what, got["bset_bin"][t].tolist(), now.tolist())
                for c in range(8):
                    returned_pairs += int(now[c] == base[d][c] and been_away[d][c])
                    been_away[d][c] |= now[c] != base[d][c]
                    if now[c] != base[d][c]:
                        moved_pairs += 1
                        if f32:
                            check_f32_column_pair(n_fft, got["tables"][t], c, int(now[c]), what)
                        else:
                            check_int8_column_pair(n_fft, got["tables"][t], got["corr"][t], c, int(now[c]), what)
                    elif f32:
                        assert np.array_equal(tr.unpack_f32(got["tables"][t], n_fft)[:, 2 * c:2 * c + 2].view(np.uint32), tr.unpack_f32(got["tables"][0], n_fft)[:, 2 * c:2 * c + 2].view(np.uint32)), "%s column pair %d is not the home table's" % (what, c)
                    else:
                        assert np.array_equal(tr.unpack_int8_digits(got["tables"][t], n_fft)[..., 2 * c:2 * c + 2], tr.unpack_int8_digits(got["tables"][0], n_fft)[..., 2 * c:2 * c + 2]), "%s column pair %d is not the home table's" % (what, c)
                        assert np.array_equal(got["corr"][t][:, 2 * c:2 * c + 2], got["corr"][0][:, 2 * c:2 * c + 2])
                away = bool((now != base[d]).any())
                assert got["item_bset"][d] == (t if away else 0), "%s: the work item reads table %d with the group %s" % (what, got["item_bset"][d], "away" if away else "at home")
                away_seen += int(away)
                back_seen += int(was_away[d] and not away)
                was_away[d] = away
            if not f32:
                check_int8_table(n_fft, got["tables"][0], got["corr"][0], got["bset_bin"][0], "batch %d home table" % b)
                check_top_digit(n_fft, got)
    assert moved_pairs > 0 and away_seen > 0 and returned_pairs > 0, (moved_pairs, away_seen, returned_pairs)
    assert back_seen > 0 or fft_log == 9, "no group came home: the switch back to the home table was not seen"


# ---- (e) end to end through the device-built tables -------------------------------------------------------------------------------------------------------------
E2E = [("SFMT_U8", 9, 2_560_000, 8000, 0), ("SFMT_U8", 10, 2_560_000, 8000, 0), ("SFMT_U8", 13, 2_560_000, 8000, 0), ("SFMT_S16", 11, 2_560_000, 8000, 0),
       ("SFMT_U8", 9, 6_000_000, 8000, "wide")]
E2E_BATCHES = 3


def fleet_streams(pkg, devices, bins, fft_log, sample_rate, wave_rate, n_batches):
    """A transmitter on every channel's bin (where the reference LOOKS: helpers.format_case), keyed as format_case keys them."""
    capi, n_fft = pkg.capi, 1 << fft_log
    hop = round(sample_rate / wave_rate)
    n_samples = (n_batches * (wave_rate // 8) + capi.AGC_EXTRA) * hop + n_fft + 8
    iq = []
    for d, dev in enumerate(devices):
        carriers = [helpers.sg.make_carrier((b if b < n_fft // 2 else b - n_fft) * sample_rate / n_fft, sample_rate, key_slot=k, key_period_s=0.5, key_on_s=0.3, key_slot_s=0.04)
                    for k, b in enumerate(bins[d])]
        gain = dev["fullscale"] / 127.5 if dev["sfmt"] == capi.SFMT_S16 else 1.0
        iq.append(helpers.convert_format(helpers.sg.generate_u8(d, 0, n_samples, carriers), dev["sfmt"], capi, gain))
    return iq


@pytest.mark.parametrize("sfmt_name,fft_log,sample_rate,wave_rate,wide", E2E, ids=lambda v: str(v))
def test_end_to_end_through_device_built_tables(pkg, built, monkeypatch, sfmt_name, fft_log, sample_rate, wave_rate, wide):
    """The fleet with AIRBAND_HIP_HOST_TABLES_MAX=0, three batches, against the oracle: EVERY channel's stage-1 bins within tests/test_gpu_afc.py's AWAY_BAR (the bar of
    device-built columns; the five- and eleven-channel dongles channel by channel like the rest: a stale value in an unused column would show in a neighbour's bin),
    squelch trace, axcindicate and counters equal, audio within 1e-4 RMS (the bars of tests/test_gpu_parity.py); at least one squelch opens."""
    capi = pkg.capi
    monkeypatch.setenv(ENV, "0")
    devices, bins = fleet(pkg, getattr(capi, sfmt_name), fft_log, sample_rate)
    iq = fleet_streams(pkg, devices, bins, fft_log, sample_rate, wave_rate, E2E_BATCHES)
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    try:
        ref = [orc.run_device(d, iq[d], E2E_BATCHES) for d in range(len(devices))]
        assert all(r["n_batches"] == E2E_BATCHES for r in ref)
        want_stats = [[orc.stats(d, j) for j in range(len(dev["channels"]))] for d, dev in enumerate(devices)]
    finally:
        orc.close()
    bar = AWAY_BAR["dft_mfma_i8"]
    assert bar <= HOME_BAR
    first = np.cumsum([0] + [len(dev["channels"]) for dev in devices])
    misses, opened, worst = [], 0, 0.0
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH | (capi.FLAG_WIDE_HOPS if wide else 0)) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8", hip.channelizer_reason()
        info = hip.table_info()
        assert info["n_host_bsets"] == 0 and info["n_shared_bsets"] == 10, info
        pos = [0] * len(devices)
        for b in range(E2E_BATCHES):
            for d in range(len(devices)):
                pos[d] += hip.submit(d, iq[d].view(np.uint8)[pos[d]:])
            assert hip.process(), "batch %d: not enough input queued" % b
            out = hip.collect(stats=True)
            trace = hip.read_trace()
            w, _ = hip.read_bins()
            for d, r in enumerate(ref):
                sl = slice(first[d], first[d + 1])
                for j in range(first[d + 1] - first[d]):
                    e = helpers.rel_rms(w[first[d] + j], r["raw_wavein"][b][j])
                    worst = max(worst, e)
                    if not e <= bar:
                        misses.append("batch %d dongle %d channel %d (bin %d): |bin| %.3g > %g" % (b, d, j, bins[d][j], e, bar))
                if not np.array_equal(out["axc"][sl], r["axc"][b]):
                    misses.append("batch %d dongle %d axc %r, oracle %r" % (b, d, bytes(out["axc"][sl]), bytes(r["axc"][b])))
                if not np.array_equal(trace[sl], r["trace"][b]):
                    misses.append("batch %d dongle %d: %d squelch-state mismatches" % (b, d, int((trace[sl] != r["trace"][b]).sum())))
                e = helpers.rms(out["waveout"][sl] - r["waveout"][b])
                if not e <= 1e-4:
                    misses.append("batch %d dongle %d audio %g" % (b, d, e))
            opened += int((out["axc"] == ord("*")).sum())
        for d in range(len(devices)):
            for j, want in enumerate(want_stats[d]):
                have = out["stats"][first[d] + j]
                for key in ("open_count", "flappy_count", "ctcss_count", "no_ctcss_count", "active_counter", "bin"):
                    if have[key] != want[key]:
                        misses.append("dongle %d channel %d %s %r, oracle %r" % (d, j, key, have[key], want[key]))
    print("end to end %s fft %d: worst per-channel |bin| error %.3g (bar %g), %d channel-batches open" % (sfmt_name, 1 << fft_log, worst, bar, opened))
    assert not misses, "%d misses, first: %s" % (len(misses), "; ".join(misses[:6]))
    assert opened > 0, "no squelch opened: not a meaningful parity run"


# ---- (f) the entry point's error paths ----------------------------------------------------------------------------------------------------------------------------
def test_error_paths(pkg, built):
    """airband_hip_read_tables refuses a handle on the wavefront FFT, a range outside [0, n_bsets) and a NULL buffer with AIRBAND_HIP_EINVAL, and touches nothing once the
    handle is released."""
    capi = pkg.capi
    devices, _ = helpers.plan_devices(2, False)
    with pkg.AirbandHip(devices, wave_rate=8000, flags=capi.FLAG_FORCE_FFT) as hip:
        assert hip.channelizer_name() == "fft_wave64"
        with pytest.raises(pkg.AirbandError) as e:
            hip.table_info()
        assert e.value.code == capi.EINVAL and "no coefficient tables" in str(e.value)
    hip = pkg.AirbandHip(devices, wave_rate=8000)
    try:
        info = hip.table_info()
        assert info["n_bsets"] == 1 and info["channelizer"] == "dft_mfma_i8"
        for first, n in ((1, 1), (0, 2), (-1, 1), (0, -1), (2, 0)):
            with pytest.raises(pkg.AirbandError) as e:
                hip.read_tables(first, n)
            assert e.value.code == capi.EINVAL, (first, n)
        assert hip.read_tables(1, 0)["tables"].shape[0] == 0   # the empty range at the end is a range
        raw = capi.TableInfo()
        tab = np.full(info["bytes_per_table"], 0x55, np.int8)
        corr = np.full(16 * info["pieces_per_table"], 7.0)
        bins = np.full(8, 77, np.int32)
        items = np.full(3 * info["n_items"], 77, np.int32)
        args = [tab.ctypes.data, corr.ctypes.data, bins.ctypes.data, items.ctypes.data]
        for k in range(4):
            assert hip.L.airband_hip_read_tables(hip.h, 0, 1, C.byref(raw), *[None if i == k else a for i, a in enumerate(args)]) == capi.EINVAL
        assert hip.L.airband_hip_read_tables(hip.h, 0, 1, None, *args) == capi.EINVAL
        assert (tab == 0x55).all() and (corr == 7.0).all() and (bins == 77).all() and (items == 77).all(), "a refused call wrote to its buffers"
        assert hip.L.airband_hip_read_tables(hip.h, 0, 1, C.byref(raw), *args) == capi.OK and bins[0] >= 0 and items.tolist() == [0, 0, 0, 0, 0, 0]
    finally:
        hip.close()
    tab[:], corr[:], bins[:], items[:] = 0x55, 7.0, 77, 77
    assert hip.L.airband_hip_read_tables(None, 0, 1, C.byref(raw), *args) == capi.EINVAL
    with pytest.raises(pkg.AirbandError):
        hip.read_tables()
    assert (tab == 0x55).all() and (corr == 7.0).all() and (bins == 77).all() and (items == 77).all()
