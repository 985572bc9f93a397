"""AFC re-tuning on the GPU at every sample format, fft size, hop alignment, WAVE_RATE, group structure and launch path, against the CPU oracle.

AFC (class AFC, src/rtl_airband.cpp:180-251) is the one feature that rewrites stage-1 state while a handle runs: afc_kernel walks the spectrum of a batch's last hop,
retune_kernel rebuilds the moved channel's coefficient columns on the device (every piece of the table at fft >= 1024) and repoints the work item between the
fleet's shared ("home") table and the group's private one.  helpers.afc_format_case() makes the inputs and screens them so that no walk hangs on a near-tie between
the float32 spectrum of the GPU and the float64 one of the oracle; tests/test_afc_generator.py (CPU) checks that the screen keeps at least three streams in four and
that every configuration below moves channels up, down and home again.

What maps to which test:
  retune_kernel with NP = 1, 2, 4, 8, 16 pieces; CF32 at fft 1024 ... 8192 (window segments at 4096 / 8192); s8 and CS16 with AFC; odd and unaligned hops; WAVE_RATE
  16000 with NFM + CTCSS + lowpass channels whose bin moves; FLAG_FORCE_FFT ......................... test_afc_matrix (axc, squelch trace, `bin` after EVERY batch, audio)
  the accuracy of device-built columns, channel by channel ............................................ test_afc_matrix (bins of every channel against the oracle's)
  the copy home, also after earlier moves and returns; a fleet sharing one home table ................. test_home_again_is_bit_identical, test_fleet_with_one_dongle_off_frequency
  more than eight channels: AFC in the last short group, in every group, beside groups without; a shared base bin; two walks ending on one bin; two channels of a
  group moving in one batch, one moving while another returns ......................................... test_group_structure (the generator test asserts the keying gives both)
  the walk's guards at bin 0 and N - 1, channels beside DC and beside N / 2 ........................... test_spectrum_ends_and_dc
  process_device (aligned and unaligned spans), FLAG_PIPELINE (runs sequentially), FLAG_REGROUP, FLAG_NO_REGROUP, FLAG_SERIAL_DEMOD ........ test_launch_paths_agree
  device_enable off / on while a dongle is away from home ............................................. test_device_enable_while_away_from_home
  process_bins, where AFC is skipped ................................................................... test_process_bins_leaves_afc_alone
  random plans ......................................................................................... test_random_afc_plans (AIRBAND_FUZZ_SEEDS_AFC, default 8)

Out of scope: scan lists with afc != 0 -- the oracle does not model a bin that moves under a frequency switch.
"""
import os

import numpy as np
import pytest

import helpers
import pyoracle

pytestmark = pytest.mark.gpu

N_BATCHES = 11   # the transmitters key for two batches out of five: two move / return cycles and the start of a third

# Stage-1 bins, channel by channel (relative RMS against the oracle's raw_wavein / raw_iq of the same channel and batch).
# HOME_BAR: the suite's bar for stage-1 bins (tests/test_gpu_parity.py), here per channel instead of per dongle.
# AWAY_BAR: a channel that is away from its base bin reads coefficient columns built on the device (sincospi) instead of the host's (libm): a coefficient may
# differ by one unit of the 24-bit scale.  Its bar is what the HOME columns showed on the same runs, times 2, and never more than HOME_BAR.
# HOME_MEASURED: the largest per-channel error of any channel at home in any batch of any test of this file, per channelizer, on an MI355X (`AIRBAND_AFC_FIGURES=1
# pytest -s` prints the figures of every run).  The largest error of a channel that was AWAY in those runs: dft_mfma_i8 1.11e-6, dft_mfma_f32 7.07e-6, fft_wave64 6.13e-7.
HOME_BAR = 1e-5
HOME_MEASURED = {"dft_mfma_i8": 1.37e-6, "dft_mfma_f32": 8.68e-6, "fft_wave64": 1.24e-6}
AWAY_BAR = {k: min(2 * v, HOME_BAR) for k, v in HOME_MEASURED.items()}


def _sfmt(pkg, name):
    return getattr(pkg.capi, name)


class Figures:
    """Largest per-channel bin errors of a run, split by whether the channel was on its base bin while the batch's stage 1 ran."""

    def __init__(self):
        self.v = dict(home_mag=0.0, home_iq=0.0, away_mag=0.0, away_iq=0.0)
        self.n_away = 0

    def add(self, away, mag, iq):
        k = "away" if away else "home"
        self.v[k + "_mag"] = max(self.v[k + "_mag"], mag)
        if iq is not None:
            self.v[k + "_iq"] = max(self.v[k + "_iq"], iq)
        self.n_away += int(away)

    def line(self, what):
        return "afc-figures %s: %s, %d away channel-batches" % (what, ", ".join("%s %.3g" % kv for kv in sorted(self.v.items())), self.n_away)


def _feed_submit(hip, case, pos):
    for d, iq in enumerate(case["iq"]):
        raw = iq.view(np.uint8)
        pos[d] += hip.submit(d, raw[pos[d]:])
    assert hip.process(), "not enough input queued"


def run_against_oracle(pkg, case, fft_log, wave_rate, flags=0, name=None, what="", feed=None, bins=True, keep=False, dongles=None, figures=None):
    """The case through one handle, batch by batch, against the oracle's results in case["ref"]: axc and squelch trace equal, `bin` stats equal after every batch,
    audio within 1e-4 RMS, and (bins=True) every channel's stage-1 bins within HOME_BAR / AWAY_BAR.  Every miss is collected and reported at the end, after the
    figures.  dongles: the ones to compare (default all).  keep=True: returns what the handle produced, per batch."""
    capi = pkg.capi
    devices, ref = case["devices"], case["ref"]
    n_dev, n_batches = len(devices), ref[0]["n_batches"]
    dongles = range(n_dev) if dongles is None else dongles
    fig = figures or Figures()
    misses, kept, moved = [], [], 0
    with pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=flags | capi.FLAG_TRACE_SQUELCH) as hip:
        if name is not None:
            assert hip.channelizer_name() == name, "%s: runs on %s" % (what, hip.channelizer_name())
        path = hip.channelizer_name()
        what = "%s [%s]" % (what, path)
        first = np.cumsum([0] + [len(d["channels"]) for d in devices])
        pos = [0] * n_dev
        for b in range(n_batches):
            if feed is None:
                _feed_submit(hip, case, pos)
            else:
                feed(hip, b)
            out = hip.collect(stats=True)
            tr = hip.read_trace()
            w, q = hip.read_bins() if (bins or keep) else (None, None)
            got_bin = np.array([s["bin"] for s in out["stats"]])
            if keep:
                kept.append(dict(waveout=out["waveout"].copy(), axc=out["axc"].copy(), trace=tr, mag=w, iq=q, bin=got_bin))
            moved += int(((out["axc"] == ord("<")) | (out["axc"] == ord(">"))).sum())
            for d in dongles:
                r, sl = ref[d], slice(first[d], first[d + 1])
                if not np.array_equal(out["axc"][sl], r["axc"][b]):
                    misses.append("batch %d dongle %d axc %r, oracle %r" % (b, d, bytes(out["axc"][sl]), bytes(r["axc"][b])))
                if not np.array_equal(got_bin[sl], r["bin"][b]):
                    misses.append("batch %d dongle %d bin %s, oracle %s" % (b, d, got_bin[sl].tolist(), r["bin"][b].tolist()))
                if not np.array_equal(tr[sl], r["trace"][b]):
                    misses.append("batch %d dongle %d: %d squelch-state mismatches" % (b, d, int((tr[sl] != r["trace"][b]).sum())))
                e = helpers.rms(out["waveout"][sl] - r["waveout"][b])
                if not e <= 1e-4:
                    misses.append("batch %d dongle %d audio %g" % (b, d, e))
                if not bins:
                    continue
                before = r["bin"][b - 1] if b else np.array(case["base"][d])   # the bins this batch's stage 1 ran on
                for j, ch in enumerate(devices[d]["channels"]):
                    away = bool(before[j] != case["base"][d][j])
                    bar = AWAY_BAR[path] if away else HOME_BAR
                    # a channel that keeps raw I/Q is compared on that; its |bin| only where read_bins recomputes it from the I/Q (NFM): stage 2 has by now
                    # written the filtered magnitude of an AM channel over stage 1's (src/rtl_airband.cpp:484-487 does the same to wavein[])
                    eq = helpers.rel_rms(q[first[d] + j], r["raw_iq"][b][j]) if case["needs_iq"][d][j] else None
                    em = helpers.rel_rms(w[first[d] + j], r["raw_wavein"][b][j]) if (eq is None or ch["modulation"] == 1) else eq
                    fig.add(away, em, eq)
                    if not em <= bar or not (eq is None or eq <= bar):
                        misses.append("batch %d dongle %d channel %d on bin %d (%s): |bin| %.3g, bin I/Q %s, bar %g" % (b, d, j, before[j], "away" if away else "home", em,
                                                                                                                   "%.3g" % eq if eq is not None else "-", bar))
    if os.environ.get("AIRBAND_AFC_FIGURES"):
        print(fig.line(what))
    assert not misses, "%s: %d misses, first: %s" % (what, len(misses), "; ".join(misses[:6]))
    return kept, moved


def _describe(sfmt_name, fft_log, sample_rate, wave_rate):
    return "%s, fft %d, %d S/s, WAVE_RATE %d" % (sfmt_name, 1 << fft_log, sample_rate, wave_rate)


# (sample format, fft_log, sample rate, WAVE_RATE, FLAG_FORCE_FFT, channelizer): every fft size with every format; NP = 1 (256, 512), 2, 4, 8, 16 on the int8 path;
# CF32 at 1024 ... 8192; hops that are 16-byte aligned (2.56 MS/s), unaligned (2.4 MS/s) and odd (2.0 MS/s); both WAVE_RATEs at every size
MATRIX = [
    ("SFMT_U8", 8, 2_560_000, 16000, False, "dft_mfma_i8"), ("SFMT_S8", 8, 2_400_000, 8000, False, "dft_mfma_i8"), ("SFMT_S16", 8, 2_560_000, 8000, False, "dft_mfma_i8"),
    ("SFMT_F32", 8, 2_560_000, 16000, False, "dft_mfma_f32"),
    ("SFMT_U8", 9, 2_000_000, 16000, False, "dft_mfma_i8"), ("SFMT_S8", 9, 2_560_000, 8000, False, "dft_mfma_i8"), ("SFMT_S16", 9, 2_400_000, 16000, False, "dft_mfma_i8"),
    ("SFMT_F32", 9, 2_400_000, 8000, False, "dft_mfma_f32"),
    ("SFMT_U8", 10, 2_560_000, 8000, False, "dft_mfma_i8"), ("SFMT_S8", 10, 2_000_000, 16000, False, "dft_mfma_i8"), ("SFMT_S16", 10, 2_560_000, 16000, False, "dft_mfma_i8"),
    ("SFMT_F32", 10, 2_560_000, 16000, False, "dft_mfma_f32"),
    ("SFMT_U8", 11, 2_400_000, 16000, False, "dft_mfma_i8"), ("SFMT_S8", 11, 2_560_000, 8000, False, "dft_mfma_i8"), ("SFMT_S16", 11, 2_400_000, 8000, False, "dft_mfma_i8"),
    ("SFMT_F32", 11, 2_560_000, 8000, False, "dft_mfma_f32"),
    ("SFMT_U8", 12, 2_560_000, 16000, False, "dft_mfma_i8"), ("SFMT_S8", 12, 2_560_000, 8000, False, "dft_mfma_i8"), ("SFMT_S16", 12, 2_400_000, 16000, False, "dft_mfma_i8"),
    ("SFMT_F32", 12, 2_000_000, 16000, False, "dft_mfma_f32"),
    ("SFMT_U8", 13, 2_560_000, 8000, False, "dft_mfma_i8"), ("SFMT_S8", 13, 2_560_000, 16000, False, "dft_mfma_i8"), ("SFMT_S16", 13, 2_560_000, 8000, False, "dft_mfma_i8"),
    ("SFMT_F32", 13, 2_560_000, 16000, False, "dft_mfma_f32"),
    ("SFMT_U8", 10, 2_560_000, 8000, True, "fft_wave64"), ("SFMT_S16", 12, 2_400_000, 16000, True, "fft_wave64")]


def _matrix_id(p):
    return "%s-fft%d-%dk-wr%d-%s" % (p[0], 1 << p[1], p[2] // 1000, p[3], p[5])


def matrix_case(pkg, p):
    return helpers.afc_format_case(pkg, _sfmt(pkg, p[0]), p[1], p[2], p[3], [helpers.afc_plan(8)] * 2, N_BATCHES)


@pytest.mark.parametrize("p", MATRIX, ids=_matrix_id)
def test_afc_matrix(pkg, built, p):
    """Two dongles of eight channels (afc 2, 1, 3, 10, 2, 255, 0, 0; transmitters +3, -2, 0, +5, -4, +1, 0, -1 bins off) at one point of MATRIX.  After every batch:
    axc, squelch trace and `bin` equal to the oracle's, audio within 1e-4 RMS, and every channel's stage-1 bins (|bin| and raw I/Q, against the oracle's float64 FFT
    at the bin the channel was on) within HOME_BAR = 1e-5 while the channel is on its base bin and AWAY_BAR while it is away.
    Measured on an MI355X (largest per-channel relative RMS of any batch; |bin| and I/Q alike): channels at home 1.37e-6 on the int8 matrix-core path, 8.68e-6 on
    the float32 one (CF32), 1.24e-6 on the wavefront FFT -- HOME_MEASURED; channels away 1.11e-6, 7.07e-6 and 6.13e-7.  AWAY_BAR = 2 x HOME_MEASURED,
    capped at HOME_BAR: 2.74e-6, 1e-5, 2.48e-6.  The relative error of a channel grows as its bin gets weaker against the dongle's whole input, which is why the
    figures of single runs scatter (3e-7 ... 8e-6 at home on the float32 path)."""
    sfmt_name, fft_log, sample_rate, wave_rate, force_fft, name = p
    case = matrix_case(pkg, p)
    _, moved = run_against_oracle(pkg, case, fft_log, wave_rate, flags=pkg.capi.FLAG_FORCE_FFT if force_fft else 0, name=name, what=_describe(*p[:4]))
    assert moved > 0 and case["ups"] > 0 and case["downs"] > 0 and case["returns"] > 0


# ---- (c) home again is bit-identical ------------------------------------------------------------------------------------------------------------------
HOME_AGAIN = [("SFMT_U8", 10, 2_560_000, 8000, "dft_mfma_i8"), ("SFMT_S8", 12, 2_560_000, 8000, "dft_mfma_i8"), ("SFMT_F32", 11, 2_560_000, 16000, "dft_mfma_f32")]


def home_again_case(pkg, p):
    return helpers.afc_format_case(pkg, _sfmt(pkg, p[0]), p[1], p[2], p[3], [helpers.afc_plan(8), helpers.afc_plan(12, shifts=[+2, -3, 0, -1, +4])], N_BATCHES)


def _plain(devices):
    return [dict(d, channels=[dict(c, afc=0) for c in d["channels"]]) for d in devices]


def _bits_of_plain_handle(pkg, case, fft_log, wave_rate, name):
    """Stage-1 bins per batch of a handle with the same plan and afc = 0 everywhere."""
    out = []
    with pkg.AirbandHip(_plain(case["devices"]), wave_rate=wave_rate, fft_log=fft_log) as hip:
        assert hip.channelizer_name() == name
        pos = [0] * len(case["iq"])
        for b in range(case["ref"][0]["n_batches"]):
            _feed_submit(hip, case, pos)
            hip.collect()
            out.append(hip.read_bins())
    return out


def _assert_home_bits(case, got, plain, what, dongles=None):
    """Whenever the oracle has every channel of a group of eight on its base bin, the group's stage-1 bins are the plain handle's, bit for bit -- and so are those
    of every single channel that is at home while a neighbour is away (retune_kernel copies its columns from the home table)."""
    first = np.cumsum([0] + [len(d["channels"]) for d in case["devices"]])
    groups_home = after_return = 0
    for d in (range(len(case["devices"])) if dongles is None else dongles):
        home = np.array(case["base"][d])
        ref = case["ref"][d]
        been_away = np.zeros(len(home), bool)
        for b in range(ref["n_batches"]):
            before = ref["bin"][b - 1] if b else home
            been_away |= before != home
            for g in range(0, len(home), 8):
                at_home = before[g:g + 8] == home[g:g + 8]
                groups_home += int(at_home.all())
                after_return += int(at_home.all() and been_away[g:g + 8].any())
                for j in np.nonzero(at_home)[0] + g:
                    k = first[d] + j
                    ch = case["devices"][d]["channels"][j]
                    pairs = [("bin I/Q", got[b]["iq"][k], plain[b][1][k])]
                    if not case["needs_iq"][d][j] or ch["modulation"] == 1:   # (stage 2 has overwritten |bin| of an AM channel that keeps raw I/Q: see run_against_oracle)
                        pairs.append(("|bin|", got[b]["mag"][k], plain[b][0][k]))
                    for name, a, p in pairs:
                        assert np.array_equal(a.view(np.uint32), p.view(np.uint32)), "%s: batch %d dongle %d channel %d (group %s): %s differs from the handle without AFC in %d places" % (
                            what, b, d, j, "at home" if at_home.all() else "away", name, int((a.view(np.uint32) != p.view(np.uint32)).sum()))
    return groups_home, after_return


@pytest.mark.parametrize("p", HOME_AGAIN, ids=lambda p: "%s-fft%d-%s" % (p[0], 1 << p[1], p[4]))
def test_home_again_is_bit_identical(pkg, built, p):
    """fft 1024 and 4096 on the int8 path, CF32 at 2048; dongles of 8 and 12 channels.  A second handle has the same plan with afc = 0.  In every batch whose stage 1
    ran with a whole group at home -- also AFTER the group's channels have moved and returned -- the group's bins equal the plain handle's bit for bit, and so do the
    bins of every channel that stayed at home while a neighbour was away."""
    sfmt_name, fft_log, sample_rate, wave_rate, name = p
    case = home_again_case(pkg, p)
    what = _describe(*p[:4])
    got, moved = run_against_oracle(pkg, case, fft_log, wave_rate, name=name, what=what, keep=True)
    plain = _bits_of_plain_handle(pkg, case, fft_log, wave_rate, name)
    groups_home, after_return = _assert_home_bits(case, got, plain, what)
    assert moved > 0 and case["returns"] > 0 and after_return > 0, (moved, groups_home, after_return)


def fleet_case(pkg):
    still = helpers.afc_plan(8, shifts=[0])
    return helpers.afc_format_case(pkg, pkg.capi.SFMT_U8, 11, 2_560_000, 8000, [still, still, helpers.afc_plan(8), still], N_BATCHES)


def test_fleet_with_one_dongle_off_frequency(pkg, built):
    """Four identical dongles (fft 2048, every channel with AFC) share ONE home table; only dongle 2's transmitters are off frequency.  Dongle 2 moves and returns as the
    oracle says; the other dongles never leave the home table: their bins equal those of a fleet without AFC bit for bit in every batch."""
    case = fleet_case(pkg)
    still = [d for d in (0, 1, 3) if (case["ref"][d]["bin"] == np.array(case["base"][d])).all()]   # (a walk over the noise floor may move a channel whose transmitter is on its bin)
    assert len(still) >= 2, "the dongles with their transmitters on frequency were meant to stay on their base bins"
    assert case["base"][0] == case["base"][2]
    got, moved = run_against_oracle(pkg, case, 11, 8000, name="dft_mfma_i8", what="fleet of four", keep=True)
    plain = _bits_of_plain_handle(pkg, case, 11, 8000, "dft_mfma_i8")
    _assert_home_bits(case, got, plain, "fleet of four")
    assert moved > 0 and case["returns"] > 0


# ---- (d) group structure --------------------------------------------------------------------------------------------------------------------------------
def group_plans(n_fft):
    """name -> (plans of the case's dongles).  Bins between 0.43 N and 0.57 N are free of the spread channels (afc_format_case)."""
    e = n_fft * 45 // 100
    last_only = [(0, 0, None)] * 8 + [(2, +2, None)]                                         # 9 channels: AFC only in the last group, which has one channel
    every = helpers.afc_plan(16)                                                             # 16: AFC in both groups
    shared = helpers.afc_plan(20, afcs=[0, 2, 0, 0, 3, 0, 0, 0, 0], shifts=[0, +2, 0, -3, +1])  # 20: groups with and without AFC side by side, a last group of four ...
    shared[17] = (3, +2, e)                                                                  # ... in which an AFC channel and one without share a base bin
    shared[18] = (0, None, e)
    same_end = helpers.afc_plan(24, afcs=[10, 0, 2, 255, 0, 1, 3, 0, 2, 0, 0])               # 24: three full groups ...
    same_end[21] = (1, +3, e)                                                                # ... two channels on ONE base bin (two column pairs), one transmitter three bins above:
    same_end[22] = (1, None, e)                                                             # both walks end on bin e + 3
    return dict(last_group_of_one=[last_only, last_only[:8] + [(3, -2, None)]], every_group=[every, helpers.afc_plan(16, shifts=[-1, +2, +4, 0, -3])], shared_base_bin=[shared, helpers.afc_plan(8)],
                walks_meet=[same_end, helpers.afc_plan(9)])


GROUPS = [("last_group_of_one", "SFMT_U8", 10, 2_560_000, 8000, "dft_mfma_i8"), ("every_group", "SFMT_S16", 11, 2_400_000, 16000, "dft_mfma_i8"),
          ("shared_base_bin", "SFMT_U8", 12, 2_560_000, 8000, "dft_mfma_i8"), ("walks_meet", "SFMT_F32", 11, 2_560_000, 8000, "dft_mfma_f32")]


def group_case(pkg, p):
    return helpers.afc_format_case(pkg, _sfmt(pkg, p[1]), p[2], p[3], p[4], group_plans(1 << p[2])[p[0]], N_BATCHES)


@pytest.mark.parametrize("p", GROUPS, ids=lambda p: "%s-%s-fft%d" % (p[0], p[1], 1 << p[2]))
def test_group_structure(pkg, built, p):
    """Dongles of 9, 16, 20 and 24 channels (two, two, three, three groups of eight column pairs): AFC only in a last group of one channel; AFC in every group; groups
    with and without AFC side by side with an AFC channel that shares its base bin with a channel without; two channels whose walks end on the same bin.  Checks of
    test_afc_matrix, plus: the unmoved groups' bins equal a plain handle's bit for bit."""
    which, sfmt_name, fft_log, sample_rate, wave_rate, name = p
    case = group_case(pkg, p)
    what = "%s: %s" % (which, _describe(*p[1:5]))
    if which == "shared_base_bin":
        assert case["base"][0][17] == case["base"][0][18] and (case["ref"][0]["bin"][:, 17] != case["base"][0][17]).any() and (case["ref"][0]["bin"][:, 18] == case["base"][0][18]).all()
    if which == "walks_meet":
        b = case["ref"][0]["bin"]
        assert ((b[:, 21] == b[:, 22]) & (b[:, 21] != case["base"][0][21])).any(), "the two walks were meant to end on one bin"
    got, moved = run_against_oracle(pkg, case, fft_log, wave_rate, name=name, what=what, keep=True)
    plain = _bits_of_plain_handle(pkg, case, fft_log, wave_rate, name)
    _assert_home_bits(case, got, plain, what)
    assert moved > 0 and case["returns"] > 0


# ---- (e) the ends of the spectrum and DC ----------------------------------------------------------------------------------------------------------------
def ends_plans(n_fft):
    """Dongle 0: channels on bins 1, 2, 3 with ONE transmitter below bin 0 (it aliases to bin N - 2): all three walk down into the guard at bin 0; N / 2 - 2 with its
    transmitter across N / 2.  Dongle 1: bins N - 2, N - 3 with one transmitter above N - 1 (bin 1), N / 2 + 2 with its transmitter below N / 2, and bin 3 with its
    transmitter ON the bin, which has to stay put beside whatever sits at DC."""
    h = n_fft // 2
    return [[(3, -3, 1), (2, None, 2), (10, None, 3), (2, +3, h - 2), (0, 0, None), (1, -1, None)],
            [(3, +3, n_fft - 2), (10, None, n_fft - 3), (2, -3, h + 2), (2, 0, 3), (0, 0, None), (255, +2, None)]]


ENDS = [("SFMT_U8", 10, 2_560_000, 8000, "dft_mfma_i8"), ("SFMT_S16", 9, 2_400_000, 16000, "dft_mfma_i8")]


def ends_case(pkg, p):
    return helpers.afc_format_case(pkg, _sfmt(pkg, p[0]), p[1], p[2], p[3], ends_plans(1 << p[1]), N_BATCHES)


@pytest.mark.parametrize("p", ENDS, ids=lambda p: "%s-fft%d" % (p[0], 1 << p[1]))
def test_spectrum_ends_and_dc(pkg, built, p):
    """Walks that run into afc_walk's guards (`bin < -step`, `bin + step >= fft_size`): see ends_plans.  u8 (whose offset of 127.5 leaves something at bin 0) and CS16
    (which has none).  The oracle's bins must include 0 and N - 1, so the guards were reached; checks of test_afc_matrix."""
    sfmt_name, fft_log, sample_rate, wave_rate, name = p
    case = ends_case(pkg, p)
    n_fft = 1 << fft_log
    assert (case["ref"][0]["bin"] == 0).any() and (case["ref"][1]["bin"] == n_fft - 1).any(), "no walk reached an end of the spectrum"
    _, moved = run_against_oracle(pkg, case, fft_log, wave_rate, name=name, what="spectrum ends: " + _describe(*p[:4]))
    assert moved > 0


# ---- (f) launch paths -----------------------------------------------------------------------------------------------------------------------------------
PATHS = [("SFMT_U8", 9, 2_000_000, 16000, "dft_mfma_i8"), ("SFMT_S16", 11, 2_560_000, 8000, "dft_mfma_i8"), ("SFMT_F32", 10, 2_560_000, 16000, "dft_mfma_f32")]


def paths_case(pkg, p):
    return helpers.afc_format_case(pkg, _sfmt(pkg, p[0]), p[1], p[2], p[3], [helpers.afc_plan(8), helpers.afc_plan(11), helpers.afc_plan(8, shifts=[-2, +3, +1, 0])], N_BATCHES)


def _resident(torch, case, extra):
    """The dongles' streams as rows of one device buffer; rows `extra` bytes apart in alignment."""
    raw = [iq.view(np.uint8) for iq in case["iq"]]
    n = min(len(r) for r in raw)
    stride = (n + extra + 255) // 256 * 256 + extra
    host = np.zeros((len(raw), stride), np.uint8)
    for d, r in enumerate(raw):
        host[d, :n] = r[:n]
    return torch.from_numpy(host).cuda(), stride


@pytest.mark.parametrize("p", PATHS, ids=lambda p: "%s-fft%d-%s" % (p[0], 1 << p[1], p[4]))
def test_launch_paths_agree(pkg, built, p):
    """One AFC case (dongles of 8, 11 and 8 channels) through submit / process, through process_device on HBM-resident I/Q (u8 at 2.0 MS/s: spans that start 8 bytes
    off a 16-byte boundary from the second batch on, rows 2 bytes apart), and through handles that asked for FLAG_PIPELINE (an AFC handle runs sequentially: AFC needs
    stage 2's verdict before the next stage 1), FLAG_REGROUP, FLAG_NO_REGROUP and FLAG_SERIAL_DEMOD.  Each equals the oracle as in test_afc_matrix, and all are
    bit-identical to each other: bins, squelch trace, audio, axc, `bin`."""
    torch = pytest.importorskip("torch")
    capi = pkg.capi
    sfmt_name, fft_log, sample_rate, wave_rate, name = p
    case = paths_case(pkg, p)
    what = _describe(*p[:4])
    runs = {}
    for label, flags in (("submit", 0), ("pipeline", capi.FLAG_PIPELINE), ("regroup", capi.FLAG_REGROUP), ("no_regroup", capi.FLAG_NO_REGROUP), ("serial_demod", capi.FLAG_SERIAL_DEMOD)):
        runs[label], moved = run_against_oracle(pkg, case, fft_log, wave_rate, flags=flags, name=name, what="%s, %s" % (what, label), keep=True)
        assert moved > 0
    extra = 2 if sfmt_name == "SFMT_U8" else 0
    dbuf, stride = _resident(torch, case, extra)
    state = dict(off=0)

    def feed(hip, b):
        g = hip.geometry
        if sfmt_name == "SFMT_U8" and b == 1:
            assert state["off"] % 16 == 8
        hip.process_device(dbuf.data_ptr() + state["off"], stride)
        state["off"] += g.first_batch_bytes if b == 0 else g.batch_bytes

    runs["process_device"], moved = run_against_oracle(pkg, case, fft_log, wave_rate, name=name, what=what + ", process_device", keep=True, feed=feed)
    assert moved > 0
    for label, got in runs.items():
        for b, (x, y) in enumerate(zip(runs["submit"], got)):
            for k in ("mag", "iq", "waveout"):
                assert np.array_equal(x[k].view(np.uint32), y[k].view(np.uint32)), "%s: batch %d: %s of %s differs from submit / process" % (what, b, k, label)
            for k in ("axc", "trace", "bin"):
                assert np.array_equal(x[k], y[k]), "%s: batch %d: %s of %s differs from submit / process" % (what, b, k, label)


def test_device_enable_while_away_from_home(pkg, built):
    """airband_hip_device_enable(h, d, 0) on a dongle whose channels are AWAY from their base bins (fft 1024: private table in use), for two batches, then on again.
    The reference's failed input is final (src/rtl_airband.cpp:383-391): while it is off the dongle reports ' ' and its state -- the moved `bin` included -- stays
    frozen, and the other dongles go on exactly as the oracle says, before, during and after.  Re-enabling is this library's extension (include/airband_hip.h: the
    dongle rejoins with the state it was frozen with, its first lead-in unspecified), so afterwards only this much is asserted of it: the handle goes on, and every
    `bin` it reports is a bin of the spectrum.  (No tighter bound: with afc 255 the oracle's own walks over a noise floor end two dozen bins from home.)"""
    capi = pkg.capi
    fft_log, wave_rate, n_fft = 10, 8000, 1024
    case = helpers.afc_format_case(pkg, capi.SFMT_U8, fft_log, 2_560_000, wave_rate, [helpers.afc_plan(8)] * 3, N_BATCHES)
    gone = 1
    home = np.array(case["base"][gone])
    away = [b for b in range(1, N_BATCHES - 3) if (case["ref"][gone]["bin"][b - 1] != home).any()]
    assert away, "dongle %d never leaves home" % gone
    off_at = away[0]
    with pkg.AirbandHip(case["devices"], wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH) as hip:
        assert hip.channelizer_name() == "dft_mfma_i8"
        pos = [0, 0, 0]
        frozen = out = None
        for b in range(N_BATCHES):
            if b == off_at:
                frozen = out["stats"][8:16]
                assert any(s["bin"] != h for s, h in zip(frozen, home))
                hip.device_enable(gone, False)
            if b == off_at + 2:
                hip.device_enable(gone, True)
            for d in range(3):
                raw = case["iq"][d].view(np.uint8)
                if d == gone and off_at <= b < off_at + 2:
                    pos[d] += hip.geometry.batch_bytes   # a failed input delivers nothing; the stream goes on without it
                elif d == gone and b == off_at + 2:      # it rejoins with an empty queue at the common read position: one batch and the look-ahead behind it
                    lo = pos[d] - hip.geometry.lookahead_bytes
                    pos[d] = lo + hip.submit(d, raw[lo:pos[d] + hip.geometry.batch_bytes])
                else:
                    pos[d] += hip.submit(d, raw[pos[d]:pos[d] + (hip.geometry.first_batch_bytes + hip.geometry.lookahead_bytes if b == 0 else hip.geometry.batch_bytes)])
            assert hip.process(), "batch %d" % b
            out = hip.collect(stats=True)
            tr = hip.read_trace()
            for d in (0, 2):
                sl, r = slice(8 * d, 8 * d + 8), case["ref"][d]
                assert np.array_equal(out["axc"][sl], r["axc"][b]), (b, d)
                assert np.array_equal(tr[sl], r["trace"][b]), (b, d)
                assert [s["bin"] for s in out["stats"][sl]] == r["bin"][b].tolist(), (b, d)
                assert helpers.rms(out["waveout"][sl] - r["waveout"][b]) <= 1e-4
            mine = out["stats"][8:16]
            if b < off_at:
                assert [s["bin"] for s in mine] == case["ref"][gone]["bin"][b].tolist(), b
            elif b < off_at + 2:
                assert (out["axc"][8:16] == ord(" ")).all()
                for j in range(8):
                    for k in ("bin", "open_count", "active_counter", "noise_level", "signal_level", "squelch_state"):
                        assert mine[j][k] == frozen[j][k], (b, j, k)
            else:
                for j in range(8):
                    assert 0 <= mine[j]["bin"] < n_fft, (b, j, mine[j]["bin"], home[j])


def test_process_bins_leaves_afc_alone(pkg, built):
    """airband_hip_process_bins on a handle with AFC channels: there is no spectrum, AFC is skipped -- `bin` never leaves the base bin, axc never shows '<' / '>', and
    stage 2 equals the oracle's run on the same bins (whose AFC finds an empty spectrum and stays, too)."""
    capi = pkg.capi
    fft_log, wave_rate = 10, 8000
    case = helpers.afc_format_case(pkg, capi.SFMT_U8, fft_log, 2_560_000, wave_rate, [helpers.afc_plan(8)] * 2, 6)
    assert case["ups"] + case["downs"] > 0   # through the channelizer these streams DO move channels
    orc = pyoracle.Oracle(case["devices"], wave_rate=wave_rate, fft_log=fft_log)
    opened = 0
    try:
        with pkg.AirbandHip(case["devices"], wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH) as hip:
            for b in range(6):
                w = np.concatenate([r["raw_wavein"][b] for r in case["ref"]])
                q = np.concatenate([r["raw_iq"][b] for r in case["ref"]])
                hip.process_bins(w, q)
                out = hip.collect(stats=True)
                tr = hip.read_trace()
                want = [orc.run_bins(d, case["ref"][d]["raw_wavein"][b], case["ref"][d]["raw_iq"][b]) for d in range(2)]
                assert set(bytes(out["axc"])) <= set(b" *"), bytes(out["axc"])
                assert [s["bin"] for s in out["stats"]] == case["base"][0] + case["base"][1], b
                assert np.array_equal(out["axc"], np.concatenate([r["axc"] for r in want]))
                assert np.array_equal(tr, np.concatenate([r["trace"] for r in want]))
                opened += int((out["axc"] == ord("*")).sum())
    finally:
        orc.close()
    assert opened > 0


# ---- (g) random AFC plans -------------------------------------------------------------------------------------------------------------------------------
AFC_RATES = {8000: [1_024_000, 2_000_000, 2_048_000, 2_400_000, 2_560_000], 16000: [1_024_000, 2_000_000, 2_048_000, 2_400_000, 2_560_000]}


def random_afc_case(pkg, seed, n_batches=N_BATCHES):
    """(case, what, fft_log, wave_rate, flags): random sample format, fft size, sample rate (hops aligned, unaligned, odd), 1 ... 5 dongles of 1 ... 24 channels with afc
    values from {0, 1, 2, 3, 10, 255} and transmitters -5 ... +5 bins off (none now and then), screened by afc_format_case."""
    capi = pkg.capi
    rng = np.random.default_rng(7700 + seed)
    sfmt_name = ["SFMT_U8", "SFMT_U8", "SFMT_S8", "SFMT_S16", "SFMT_F32"][int(rng.integers(0, 5))]
    fft_log = int(rng.choice([8, 9, 10, 11, 12, 13]))
    wave_rate = int(rng.choice([8000, 16000]))
    sample_rate = int(rng.choice(AFC_RATES[wave_rate] if fft_log < 12 else AFC_RATES[wave_rate][1:2] + AFC_RATES[wave_rate][3:]))   # (bins of 250 Hz and less: see below)
    reach = 3 if fft_log == 8 else 5
    plans = []
    for d in range(int(rng.integers(1, 6))):
        n = int(rng.integers(9, 25)) if rng.random() < 0.3 else int(rng.integers(1, 9))
        if fft_log >= 12:   # the noise floor's bins differ by about 1e-5 of the largest bin power there: two dozen walks per cycle rarely ALL clear the screen
            n = min(n, 12)
        plans.append([(int(rng.choice([0, 1, 2, 3, 10, 255, 2, 3])), None if rng.random() < 0.05 else int(rng.integers(-reach, reach + 1)), None) for _ in range(n)])
    plans[0][0] = (int(rng.choice([1, 2, 3, 10, 255])), int(rng.choice([-2, 2])), None)   # no seed without an AFC channel whose transmitter is off its bin
    flags = capi.FLAG_FORCE_FFT if rng.random() < 0.15 else 0
    what = "seed %d: %s, fft %d, %d S/s, WAVE_RATE %d, channels %s%s" % (seed, sfmt_name, 1 << fft_log, sample_rate, wave_rate, [len(p) for p in plans], ", FLAG_FORCE_FFT" if flags else "")
    try:
        case = helpers.afc_format_case(pkg, _sfmt(pkg, sfmt_name), fft_log, sample_rate, wave_rate, plans, n_batches, first_dongle=10 * seed)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None
    return case, what, fft_log, wave_rate, flags


FUZZ_SEEDS = range(int(os.environ.get("AIRBAND_FUZZ_SEEDS_AFC", "8")))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_afc_plans(pkg, built, seed):
    """Random AFC plans (random_afc_case) on whatever channelizer the library picks: the checks of test_afc_matrix, bins channel by channel included.  A failure names
    seed, path, format, fft size and rate."""
    case, what, fft_log, wave_rate, flags = random_afc_case(pkg, seed)
    run_against_oracle(pkg, case, fft_log, wave_rate, flags=flags, what=what)
