"""The band follow on the GPU (airband_hip_prepare_follow / _set_band_follow / _collect_band_follow_changes / _collect_band_followers / _device_band_follow,
csrc/band_follow.hip): followers, row records, the change count and the changes byte for byte what capi.band_follow_reference() makes of the handle's own
track tables, batch after batch; what a move does to stage 1 (the follower's bins are those of a channel configured on that bin) and what it does not do to
stage 2 and to the neighbours (nothing); and its lifetime.  Built on tests/test_gpu_band_watch.py's streams: 3 dongles x 8 channels, two followers on dongles 0
and 1 and none on dongle 2, 10 batches.  (tests/test_host_band_follow.py runs the kernel source on the CPU; this file is what a GPU says.)"""
import numpy as np
import pytest

import helpers
import survey_cases
import test_gpu_band_watch as wt
from test_gpu_afc import AWAY_BAR  # the bar a moved channel's stage-1 bins are held to (device-built coefficient columns)

pytestmark = pytest.mark.gpu

N_DEV, N_BATCHES, WAVE_RATE = 3, 10, 8000
FOLLOW = [6, 7, 14, 15]  # channels 6 and 7 of dongles 0 and 1
WATCH = dict(wt.WATCH)   # max_tracks 8, match_bins 2, confirm_hits 2, release_misses 2
TONE = 11.0              # amplitude of the steady tones in u8 counts (noise: sigma 9 per component); see test_follow_on_the_default_channelizer
CENTER = 120_000_000

_CASES = {}


def _bin_freq(pkg, devices, d, b, n_fft, fft_log):
    """A channel frequency that the library's bin formula (src/config.cpp:666-667) puts on bin b of dongle d."""
    rate = devices[d].get("sample_rate", 2_560_000)
    off = (b if b < n_fft // 2 else b - n_fft) * rate / n_fft
    for df in (0, 1, -1, 2, -2, rate // (4 * n_fft), -(rate // (4 * n_fft))):
        f = CENTER + int(round(off)) + df
        probe = [dict(devices[d], channels=[dict(devices[d]["channels"][0], frequency=f)])]
        if int(pkg.derive_constants(probe, 0, wave_rate=WAVE_RATE, fft_log=fft_log)[0]) == b:
            return f
    raise AssertionError("no frequency found for bin %d" % b)


def _case(pkg, sfmt_name="SFMT_U8", sample_rate=2_560_000, fft_log=9, afc=False):
    """Devices, streams and the tones' bins.  Every dongle: a steady tone S.  Dongle 0: a tone K keyed in batches 1 - 8 that sits one bin higher from batch 5 on
    (MOVE), and a transmitter on configured channel 1 in batches 2 - 7 (a neighbour with audio, in the followers' group of eight).  Dongle 1: K1 (batches 1 - 4) and
    K2 (batches 1 - 9): with S three carriers for two followers (n_unserved > 0), and K1's end sends its follower home.  Dongle 2: S only, and no followers."""
    key = (sfmt_name, sample_rate, fft_log, afc)
    if key not in _CASES:
        capi = pkg.capi
        n_fft = 1 << fft_log
        devices = helpers._format_devices(capi, getattr(capi, sfmt_name), sample_rate, WAVE_RATE, N_DEV)
        if afc:
            devices[0]["channels"][5]["afc"] = 2  # quiet: it never moves, but its group and the followers' share the re-tune epoch
        hop, B = round(sample_rate / WAVE_RATE), WAVE_RATE // 8
        bins = wt._channel_bins(pkg, devices, WAVE_RATE, fft_log)
        n_samples = (N_BATCHES * B + 100) * hop + n_fft + 8
        iq, tone_bins = [], []
        for d in range(N_DEV):
            free = wt._free_bins(n_fft, bins[d], 3)
            tones = [(wt._freq(free[0], n_fft), TONE, None)]
            mine = dict(S=free[0])
            if d == 0:
                tones += [(wt._freq(free[1], n_fft), 12.0, (1, 4)), (wt._freq(free[1] + 1, n_fft), 12.0, (5, 8)), (wt._freq(bins[0][1], n_fft), 12.0, (2, 7))]
                mine.update(K=free[1], K_moved=free[1] + 1)
            if d == 1:
                tones += [(wt._freq(free[1], n_fft), 14.0, (1, 4)), (wt._freq(free[2], n_fft), 10.0, (1, 9))]
                mine.update(K1=free[1], K2=free[2])
            iq.append(wt._stream(capi, devices[d], n_samples, [fft_log, d, sample_rate, 78], tones, B, hop))
            tone_bins.append(mine)
        # the twin whose channels are CONFIGURED on the tones' bins: channel j of dongle d sits on the j-th bin of its dongle's tones (the rest stay where they are)
        static, static_bins = [], []
        for d in range(N_DEV):
            want = sorted(set(tone_bins[d].values()))
            chans = [dict(c) for c in devices[d]["channels"]]
            for j, b in enumerate(want):
                chans[2 + j] = dict(chans[2 + j], frequency=_bin_freq(pkg, devices, d, b, n_fft, fft_log), afc=0)
            static.append(dict(devices[d], channels=chans))
            static_bins.append({b: 2 + j for j, b in enumerate(want)})
        _CASES[key] = dict(devices=devices, iq=iq, tones=tone_bins, bins=bins, static=static, static_bins=static_bins, n_fft=n_fft, B=B)
    return _CASES[key]


class FollowRef:
    """capi.band_follow_reference() advanced on collected track tables: the fleet's expected followers, records and changes."""

    def __init__(self, capi, follow, home, n_dev, chan_first):
        self.capi, self.n_dev, self.home, self.k = capi, n_dev, np.array(home), 0
        self.fol = capi.band_follow_blank(follow, home)
        self.rows = np.zeros(n_dev, capi.FOLLOW_ROW_DTYPE)
        dev_of = np.searchsorted(chan_first, follow, side="right") - 1
        self.range = [np.flatnonzero(dev_of == d) for d in range(n_dev)]

    def advance(self, tracks, off=()):
        changes = []
        for d in range(self.n_dev):
            if d in off:  # frozen
                self.rows[d]["n_changes"] = 0
                continue
            r = self.range[d]
            f, row, ch = self.capi.band_follow_reference(self.fol[r], tracks[d], self.home[r], self.k, dev=d)
            self.fol[r], self.rows[d] = f, row
            changes.append(ch)
        self.k += 1
        return np.concatenate(changes)


def _open(pkg, devices, follow, flags=0, max_changes=None):
    hip = pkg.AirbandHip(devices, wave_rate=WAVE_RATE, fft_log=9, flags=flags, follow=follow)
    hip.set_band_scope(windows=8)
    hip.set_band_survey(max_peaks=wt.MAX_PEAKS, guard_bins=wt.GUARD)
    hip.set_band_watch(**WATCH)
    if follow:
        hip.set_band_follow(max_changes)
    return hip


def _stats_but_bin(stats):
    return [{k: v for k, v in s.items() if k != "bin"} for s in stats]


def _run_checks_1_to_4(pkg, case, flags=0):
    """Four handles on the same bytes: A with followers; S, the twin with channels configured on the tones' bins; D, A's configuration without followers; and B,
    the same without followers, fed A's own stage-1 output through process_bins.  Returns what happened, for the caller's non-vacuity checks."""
    capi = pkg.capi
    devices, iq, n_fft, B = case["devices"], case["iq"], case["n_fft"], case["B"]
    first = np.cumsum([0] + [len(d["channels"]) for d in devices])
    home = [case["bins"][c // 8][c % 8] for c in FOLLOW]
    seen = dict(changes=[], rows=[], mags={}, moved_rows=0, worst=0.0, audio=0)
    with _open(pkg, devices, FOLLOW, flags) as A, _open(pkg, case["static"], None, flags) as S, _open(pkg, devices, None, flags) as D, \
            pkg.AirbandHip(devices, wave_rate=WAVE_RATE, fft_log=9, flags=flags) as Bh:
        name = A.channelizer_name()
        assert S.channelizer_name() == name == D.channelizer_name()
        with pytest.raises(pkg.AirbandError) as e:  # before any batch
            A.collect_band_follow_changes()
        assert e.value.code == capi.EAGAIN
        ref = FollowRef(capi, FOLLOW, home, N_DEV, first)
        pos = {h: [0] * N_DEV for h in (A, S, D)}
        in_force = np.array(home)  # the bins stage 1 of the batch runs the followers on
        for b in range(N_BATCHES):
            for h in (A, S, D):
                wt._feed(h, iq, pos[h])
            # ---- 1. the decision, byte for byte ----
            tracks = A.collect_band_tracks()
            fol, chg = A.collect_band_followers(), A.collect_band_follow_changes()
            want = ref.advance(tracks["tracks"])
            print("%s batch %d: changes %s, rows %s" % (name, b, [(int(c["kind"]), int(c["channel"]), int(c["bin"]), int(c["track"])) for c in want], ref.rows.tolist()))
            assert fol["followers"].tobytes() == ref.fol.tobytes(), (b, fol["followers"], ref.fol)
            assert fol["rows"].tobytes() == ref.rows.tobytes(), (b, fol["rows"], ref.rows)
            assert chg["n_changes"] == len(want) and chg["changes"].tobytes() == want[:A.follow_changes].tobytes(), (b, chg, want)
            assert A.collect_band_follow_changes()["changes"].tobytes() == chg["changes"].tobytes()  # repeatable
            assert D.collect_band_tracks()["tracks"].tobytes() == tracks["tracks"].tobytes()  # the survey does not see where the followers are
            # ---- 2. stage 1: the follower's rows are those of a channel configured on the bin it is on ----
            wa, qa = A.read_bins()
            ws, _ = S.read_bins()
            wd, _ = D.read_bins()
            for i, c in enumerate(FOLLOW):
                d = int(np.searchsorted(first, c, side="right") - 1)
                if in_force[i] == home[i]:
                    assert np.array_equal(survey_cases.bits(wa[c]), survey_cases.bits(wd[c])), (b, c, "a follower at home keeps its home table")
                    continue
                assert int(in_force[i]) in case["static_bins"][d], (b, c, int(in_force[i]), case["tones"][d])
                twin = first[d] + case["static_bins"][d][int(in_force[i])]
                err = helpers.rel_rms(wa[c], ws[twin])
                seen["worst"] = max(seen["worst"], err)
                seen["moved_rows"] += 1
                assert err <= AWAY_BAR[name], (b, c, int(in_force[i]), err, AWAY_BAR[name])
            seen["mags"][b] = wa[FOLLOW].mean(axis=1)
            # ---- 3. stage 2 knows nothing of it: A's own bins through a handle without followers ----
            Bh.process_bins(wa, qa)
            oa, ob, od = A.collect(stats=True), Bh.collect(stats=True), D.collect(stats=True)
            assert np.array_equal(survey_cases.bits(oa["waveout"]), survey_cases.bits(ob["waveout"])), (b, "waveout")
            assert np.array_equal(oa["axc"], ob["axc"]) and _stats_but_bin(oa["stats"]) == _stats_but_bin(ob["stats"]), (b, "axc / stats")
            assert [s["bin"] for s in oa["stats"]][FOLLOW[0]] == int(ref.fol["bin"][0])  # stats.bin: where the NEXT batch is channelized
            seen["audio"] += int(np.count_nonzero(oa["waveout"][FOLLOW]))
            # ---- 4. the neighbours ----
            others = np.setdiff1d(np.arange(first[-1]), FOLLOW)
            assert np.array_equal(survey_cases.bits(oa["waveout"][others]), survey_cases.bits(od["waveout"][others])), (b, "neighbours' waveout")
            assert np.array_equal(survey_cases.bits(wa[others]), survey_cases.bits(wd[others])), (b, "neighbours' bins")
            seen["neighbour_audio"] = seen.get("neighbour_audio", 0) + int(np.count_nonzero(oa["waveout"][others]))
            in_force = ref.fol["bin"].copy()
            seen["changes"].append(want)
            seen["rows"].append(ref.rows.copy())
    seen["name"] = name
    return seen


def _kinds(seen, capi):
    allc = np.concatenate(seen["changes"])
    return [int((allc["kind"] == k).sum()) for k in (capi.FOLLOW_TUNE, capi.FOLLOW_MOVE, capi.FOLLOW_HOME)]


def _tone_over_noise_db(case, d, b):
    """numpy on the CPU: the power of bin b over the median bin's, in the mean of 16 unwindowed 512-sample periodograms of dongle d's stream (inside batch 1)."""
    n = case["n_fft"]
    x = case["iq"][d].astype(np.float64) - 127.5
    z = (x[0::2] + 1j * x[1::2])[400_000:400_000 + 16 * n].reshape(16, n)
    p = (np.abs(np.fft.fft(z, axis=1)) ** 2).mean(axis=0)
    return 10 * np.log10(p[b] / np.median(p))


def test_follow_on_the_default_channelizer(pkg, built):
    """Checks 1 - 5 on the int8 matrix-core channelizer (u8, 2.56 MS/s, fft 512).
    The tones: amplitude 11 u8 counts over noise of sigma 9 per component; numpy puts the steady tone's bin of dongle 0 26.1 dB over the median bin of an
    unwindowed 512-point periodogram of this case's stream (printed and asserted below: >= 20 dB), a ratio of about 20 in RMS |bin|.  Asked of the follower: its
    mean |bin| over the batch after TUNE is at least 4 x that of the batch before; measured on an MI355X: 0.886 -> 11.95, x 13.5 (the library's window widens
    the noise bandwidth, and a mean of magnitudes over noise is not an RMS)."""
    capi = pkg.capi
    case = _case(pkg)
    db = _tone_over_noise_db(case, 0, case["tones"][0]["S"])
    print("steady tone over the noise in-bin: %.1f dB" % db)
    assert db >= 20.0
    seen = _run_checks_1_to_4(pkg, case)
    assert seen["name"] == "dft_mfma_i8"
    tune, move, home = _kinds(seen, capi)
    print("TUNE %d MOVE %d HOME %d, %d moved rows compared, worst %.3g, follower audio samples %d, neighbour audio samples %d" % (
        tune, move, home, seen["moved_rows"], seen["worst"], seen["audio"], seen["neighbour_audio"]))
    assert tune >= 4 and move >= 1 and home >= 1 and seen["moved_rows"] >= 16 and seen["audio"] > 0 and seen["neighbour_audio"] > 0
    assert max(int(r[1]["n_unserved"]) for r in seen["rows"]) >= 1  # three carriers for dongle 1's two followers
    assert max(int(r[2]["n_unserved"]) for r in seen["rows"]) >= 1 and all(int(r[2]["n_following"]) == 0 for r in seen["rows"])  # dongle 2 has no followers
    # the named events: S of dongle 0 confirmed at batch 1 (channel 6), K at batch 2 (channel 7), K's drift at batch 5, dongle 1's K1 gone at batch 6
    def has(b, kind, channel, bin_=None):
        return any(int(c["kind"]) == kind and int(c["channel"]) == channel and (bin_ is None or abs(int(c["bin"]) - bin_) <= 1) for c in seen["changes"][b])
    t = case["tones"]
    assert has(1, capi.FOLLOW_TUNE, 6, t[0]["S"]) and has(2, capi.FOLLOW_TUNE, 7, t[0]["K"]) and has(5, capi.FOLLOW_MOVE, 7, t[0]["K_moved"]), seen["changes"]
    assert has(1, capi.FOLLOW_TUNE, 14, t[1]["S"]) and has(6, capi.FOLLOW_HOME, 15) and has(7, capi.FOLLOW_TUNE, 15), seen["changes"]
    # ---- 5. it listens: channel 6 is tuned at batch 1, so batch 2 is channelized on the tone ----
    before, after = float(seen["mags"][1][0]), float(seen["mags"][2][0])
    print("channel 6 mean |bin|: %.4g in batch 1, %.4g in batch 2 (x %.1f)" % (before, after, after / before))
    assert after >= 4.0 * before


VARIANTS = [("force_fft", "SFMT_U8", 2_560_000, "FLAG_FORCE_FFT", False, "fft_wave64"), ("cs16_wide", "SFMT_S16", 10_000_000, "FLAG_WIDE_HOPS", False, "dft_mfma_i8"),
            ("cf32", "SFMT_F32", 2_560_000, None, False, "dft_mfma_f32"), ("afc_in_the_group", "SFMT_U8", 2_560_000, None, True, "dft_mfma_i8")]


@pytest.mark.parametrize("v", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_follow_on_the_other_channelizers(pkg, built, v):
    """Checks 1 - 3 (and 4) on every other channelizer a follower can meet: the wavefront FFT, CS16 at 10 MS/s on wide hops, CF32, and a handle with an AFC channel
    in the followers' group of eight (one re-tune epoch for both)."""
    capi = pkg.capi
    _, sfmt_name, rate, flag, afc, name = v
    seen = _run_checks_1_to_4(pkg, _case(pkg, sfmt_name, rate, 9, afc), flags=getattr(capi, flag) if flag else 0)
    assert seen["name"] == name
    tune, move, home = _kinds(seen, capi)
    print("%s: TUNE %d MOVE %d HOME %d, %d moved rows compared, worst %.3g" % (v[0], tune, move, home, seen["moved_rows"], seen["worst"]))
    assert tune >= 3 and move + home >= 1 and seen["moved_rows"] >= 8 and seen["audio"] > 0


def test_fewer_records_than_changes(pkg, built):
    """max_changes = 1: n_changes is exact and the one record is the reference's first."""
    capi = pkg.capi
    case = _case(pkg)
    first = np.cumsum([0] + [len(d["channels"]) for d in case["devices"]])
    home = [case["bins"][c // 8][c % 8] for c in FOLLOW]
    with _open(pkg, case["devices"], FOLLOW, max_changes=1) as A:
        ref, pos, most = FollowRef(capi, FOLLOW, home, N_DEV, first), [0] * N_DEV, 0
        for b in range(3):
            wt._feed(A, case["iq"], pos)
            want = ref.advance(A.collect_band_tracks()["tracks"])
            got = A.collect_band_follow_changes()
            assert got["n_changes"] == len(want) and got["changes"].tobytes() == want[:1].tobytes(), (b, got, want)
            assert A.collect_band_followers()["followers"].tobytes() == ref.fol.tobytes()
            most = max(most, len(want))
        assert most >= 2  # S of dongles 0 and 1 are confirmed in the same batch


def test_lifetime(pkg, built):
    """A dongle switched off mid-stream keeps its followers frozen and resumes; process_bins leaves followers, changes and bins alone; the schedule; set_band_scope
    again drops the follow; the setter's errors."""
    capi = pkg.capi
    case = _case(pkg)
    devices, iq = case["devices"], case["iq"]
    first = np.cumsum([0] + [len(d["channels"]) for d in devices])
    home = [case["bins"][c // 8][c % 8] for c in FOLLOW]
    with pkg.AirbandHip(devices, wave_rate=WAVE_RATE) as plain, pkg.AirbandHip(devices, wave_rate=WAVE_RATE, flags=capi.FLAG_PIPELINE, follow=FOLLOW) as piped:
        assert plain.schedule_info()["run_ahead"] and plain.schedule_info()["ring_batches"] == 2
        assert not piped.schedule_info()["run_ahead"] and piped.schedule_info()["ring_batches"] == 1  # FLAG_PIPELINE is ignored on a handle with followers
        plain.set_band_scope(windows=2)
        plain.set_band_survey(max_peaks=4)
        plain.set_band_watch(**WATCH)
        assert plain.L.airband_hip_set_band_follow(plain.h, 4) == capi.EINVAL  # no followers
    with pkg.AirbandHip(devices, wave_rate=WAVE_RATE, follow=FOLLOW) as hip:
        L = hip.L
        assert not hip.schedule_info()["run_ahead"] and hip.schedule_info()["ring_batches"] == 1
        assert L.airband_hip_set_band_follow(hip.h, 4) == capi.EINVAL  # no scope
        hip.set_band_scope(windows=8)
        hip.set_band_survey(max_peaks=wt.MAX_PEAKS, guard_bins=wt.GUARD)
        assert L.airband_hip_set_band_follow(hip.h, 4) == capi.EINVAL  # no watch
        hip.set_band_watch(**WATCH)
        most = len(FOLLOW) + N_DEV * WATCH["max_tracks"]
        for bad in (0, -1, most + 1):
            assert L.airband_hip_set_band_follow(hip.h, bad) == capi.EINVAL, bad
        with pytest.raises(pkg.AirbandError) as e:  # none of them left a follow behind
            hip.device_band_follow()
        assert e.value.code == capi.EINVAL
        hip.set_band_follow(most)
        hip.set_band_follow()  # again before the first batch: replaces it
        assert all(hip.device_band_follow().values())
        hip.set_band_scope(windows=8)  # a new scope drops the survey, the watch and the follow
        with pytest.raises(pkg.AirbandError) as e:
            hip.device_band_follow()
        assert e.value.code == capi.EINVAL
        hip.set_band_survey(max_peaks=wt.MAX_PEAKS, guard_bins=wt.GUARD)
        hip.set_band_watch(**WATCH)
        hip.set_band_follow()
        ref = FollowRef(capi, FOLLOW, home, N_DEV, first)
        pos, frozen = [0] * N_DEV, None
        for b in range(9):
            if b == 3:
                hip.device_enable(1, False)
            if b == 5:  # back on: its ring starts again where the fleet is
                hip.device_enable(1, True)
                pos[1] = hip.geometry.first_batch_bytes + 4 * hip.geometry.batch_bytes
            for d in range(N_DEV):
                if d != 1 or not 3 <= b < 5:
                    pos[d] += hip.submit(d, iq[d].view(np.uint8)[pos[d]:])
            assert hip.process(), "not enough input queued"
            off = (1,) if 3 <= b < 5 else ()
            want = ref.advance(hip.collect_band_tracks()["tracks"], off=off)
            fol, chg = hip.collect_band_followers(), hip.collect_band_follow_changes()
            assert fol["followers"].tobytes() == ref.fol.tobytes() and fol["rows"].tobytes() == ref.rows.tobytes(), (b, fol, ref.fol, ref.rows)
            assert chg["n_changes"] == len(want) and chg["changes"].tobytes() == want.tobytes(), (b, chg, want)
            if b == 2:
                frozen = fol["followers"][2:].tobytes()
                assert int(fol["rows"][1]["n_following"]) == 2  # both of dongle 1's followers are tuned when it goes off
            if off:
                assert fol["followers"][2:].tobytes() == frozen and int(fol["rows"][1]["n_changes"]) == 0 and int(fol["rows"][1]["n_following"]) == 2
                assert not any(int(c["dev"]) == 1 for c in chg["changes"])
            if b == 6:  # a batch without input: everything stays, the bins included
                stats = hip.collect(stats=True)["stats"]
                w, q = hip.read_bins()
                hip.process_bins(w, q)
                again, chg2 = hip.collect_band_followers(), hip.collect_band_follow_changes()
                assert again["followers"].tobytes() == fol["followers"].tobytes() and again["rows"].tobytes() == fol["rows"].tobytes()
                assert chg2["n_changes"] == chg["n_changes"] and chg2["changes"].tobytes() == chg["changes"].tobytes()
                assert [s["bin"] for s in hip.collect(stats=True)["stats"]] == [s["bin"] for s in stats]
        # the device views: the same bytes
        import torch

        v = hip.device_band_follow()
        n = torch.as_tensor(pkg.DevicePtr(v["n_changes"], (1,), "<i4"), device="cuda").cpu().numpy()
        f = torch.as_tensor(pkg.DevicePtr(v["followers"], (len(FOLLOW), 4), "<i4"), device="cuda").cpu().numpy()
        r = torch.as_tensor(pkg.DevicePtr(v["rows"], (N_DEV, 4), "<i4"), device="cuda").cpu().numpy()
        assert int(n[0]) == chg["n_changes"] and f.tobytes() == fol["followers"].tobytes() and r.tobytes() == fol["rows"].tobytes()
        with pytest.raises(pkg.AirbandError) as e:  # a batch has been enqueued
            hip.set_band_follow()
        assert e.value.code == capi.EINVAL
