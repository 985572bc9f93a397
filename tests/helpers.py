"""Shared helpers for the parity tests (test infrastructure)."""
from __future__ import annotations

import glob
import importlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sg = importlib.import_module("rtlsdr-airband_amd.siggen")


def plan_devices(n_dev: int, mixed: bool, tweak=None):
    """n_dev dongles with the BASELINE channel plan; returns (devices, carriers)."""
    chans, carriers = sg.baseline_plan(mixed=mixed)
    devices = []
    for d in range(n_dev):
        ch = [dict(c) for c in chans]
        if tweak:
            tweak(d, ch)
        devices.append(dict(channels=ch))
    return devices, carriers


def stream_bytes(n_batches: int, wave_rate: int, fft_size: int = 512, sample_rate: int = 2_560_000) -> int:
    """Bytes of u8 I/Q one dongle must deliver for n_batches output batches (incl. lead-in and look-ahead)."""
    hop = round(sample_rate / wave_rate)
    B = wave_rate // 8
    return 2 * ((n_batches * B + 100) * hop + fft_size)


def rel_rms(a: np.ndarray, b: np.ndarray) -> float:
    a = a.astype(np.float64)
    b = b.astype(np.float64)
    den = np.sqrt(np.mean(b * b))
    return float(np.sqrt(np.mean((a - b) ** 2)) / (den if den > 0 else 1.0))


def rms(a: np.ndarray) -> float:
    return float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))


def axc_str(axc: np.ndarray) -> str:
    return "\n".join("".join(chr(v) for v in row) for row in np.asarray(axc).T)


def afc_case(n_dev: int = 1):
    """Channels with AFC enabled whose transmitters sit a few FFT bins off the configured frequency
    (reference: class AFC, src/rtl_airband.cpp:180-251).  Returns (devices, carriers)."""
    chans, carriers = sg.baseline_plan(mixed=False)
    shifts = [+3, -2, 0, +5, -4, +1, 0, -1]           # in 5 kHz bins
    afcs = [2, 1, 3, 10, 2, 255, 0, 0]
    bin_hz = sg.SAMPLE_RATE / 512
    out = []
    for k, (c, car) in enumerate(zip(chans, carriers)):
        c["afc"] = afcs[k]
        off = sg.PLAN_OFFSETS_HZ[k] + shifts[k] * bin_hz
        out.append(sg.make_carrier(off, sg.SAMPLE_RATE, kind=0, key_slot=k, key_period_s=0.75, key_on_s=0.4, key_slot_s=0.05))
    return [dict(channels=[dict(c) for c in chans]) for _ in range(n_dev)], out


def convert_format(iq_u8, sfmt, capi, s16_gain=200.0):
    """Re-express the synthetic u8 stream in the other sample formats the input drivers deliver (src/input-soapysdr.cpp:45-64,
    src/input-mirisdr.cpp)."""
    x = iq_u8.astype(np.float32) - 127.5
    if sfmt == capi.SFMT_U8:
        return iq_u8
    if sfmt == capi.SFMT_S8:
        return np.clip(np.round(x), -127, 127).astype(np.int8)  # -128 indexes a table entry the reference never initialises
    if sfmt == capi.SFMT_S16:
        return np.round(x * s16_gain).astype(np.int16)
    return (x / 127.5).astype(np.float32)


def _format_plan(capi, sfmt, sample_rate, wave_rate, n_dev):
    """format_case's channels (the BASELINE plan scaled into the dongle's passband) and its per-dongle CS16 gains."""
    chans, _ = sg.baseline_plan(mixed=wave_rate == 16000)
    scale = sample_rate / 2_560_000
    for c in chans:  # keep every channel inside the dongle's (possibly narrower) passband
        c["frequency"] = 120_000_000 + int((c["frequency"] - 120_000_000) * scale * 0.8)
    gains = [200.0 if d % 2 == 0 else 50.0 for d in range(n_dev)] if sfmt == capi.SFMT_S16 else [1.0] * n_dev
    return chans, gains


def _format_devices(capi, sfmt, sample_rate, wave_rate, n_dev):
    chans, gains = _format_plan(capi, sfmt, sample_rate, wave_rate, n_dev)
    return [dict(channels=[dict(c) for c in chans], sample_rate=sample_rate, sfmt=sfmt, fullscale=0.0 if sfmt != capi.SFMT_S16 else 127.5 * gains[d])
            for d in range(n_dev)]


def format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, n_dev, n_batches, first_dongle=0):
    """n_dev dongles of the BASELINE channel plan re-expressed for another sample format / fft size / sample rate: channels scaled
    into the dongle's passband, every transmitter placed where the reference LOOKS -- its bin formula divides by the integer
    sample_rate / fft_size (src/config.cpp:666-667), which is off by many bins when that quotient is not exact (e.g. 2.56 MS/s /
    8192).  Two CS16 sources of one handle need not share a full scale (a 12-bit and a 16-bit SoapySDR device): odd dongles deliver
    the same signal at a quarter of the amplitude and say so in input->fullscale (src/rtl_airband.cpp:403).
    Returns (devices, iq list in the format's dtype)."""
    capi = pkg.capi
    chans, gains = _format_plan(capi, sfmt, sample_rate, wave_rate, n_dev)
    carriers = []
    probe = [dict(channels=[dict(c) for c in chans], sample_rate=sample_rate)]
    n_fft = 1 << fft_log
    for k, c in enumerate(chans):
        b = int(pkg.derive_constants(probe, k, wave_rate=wave_rate, fft_log=fft_log)[0])
        off = (b if b < n_fft // 2 else b - n_fft) * sample_rate / n_fft
        carriers.append(sg.make_carrier(off, sample_rate, kind=c["modulation"], ctcss_hz=c["ctcss_freq"], key_slot=k, key_period_s=0.5, key_on_s=0.3, key_slot_s=0.04))
    devices = _format_devices(capi, sfmt, sample_rate, wave_rate, n_dev)
    hop = round(sample_rate / wave_rate)
    n_samples = (n_batches * (wave_rate // 8) + 100) * hop + n_fft + 8  # + 8: hops of 300 / 600 bytes are staged in whole 16-byte pieces
    iq = [convert_format(sg.generate_u8(first_dongle + d, 0, n_samples, carriers), sfmt, capi, gains[d]) for d in range(n_dev)]
    return devices, iq


# ---- wide hops at every kernel variant (tests/test_wide_variants.py, tests/test_gpu_wide_variants.py) ------------------------------------------------
# Dongle 1 of a sweep case: channel offsets as fractions of the sample rate.  Five lie below the centre frequency (bins in the upper half of the spectrum), channels
# 4 and 5 share a frequency and so a bin, eleven channels are two column sets of the coefficient tables with the second holding three (a partly filled group).
WIDE_PLAN_B = [-0.41, -0.33, -0.21, -0.12, 0.07, 0.07, 0.16, 0.24, 0.31, 0.38, -0.05]
WIDE_PLAN_B_IQ_CHANNEL = 2   # an AM channel with has_iq_outputs: magnitude and raw I/Q stored from one lane
# Tone amplitude (u8 counts) and noise deviation of dongle 1: ten tones of amplitude a at unrelated frequencies and phases (the eleventh is a weak one, below) add
# up to a deviation of sqrt(10 a^2 / 2 + s^2) = 49.5 per rail, and the rails (+-127.5) are 2.57 of those away: about 1 % of the samples of either rail clip
WIDE_TONE_B, WIDE_NOISE_B = 21.7, 10.0
WIDE_TONE_A, WIDE_NOISE_A = 8.0, 6.0   # dongle 0: eight tones, 23.4 per rail -- 5.4 deviations inside the rails
# An AM channel that stores raw I/Q has its magnitudes REWRITTEN IN PLACE by stage 2 while its squelch sees a signal (|I/Q of 100 hops earlier|: src/rtl_airband.cpp,
# the oracle's stage2_channel; the library does the same in its rings), so what read_bins() returns for it is stage 1's output only while the squelch stays shut.
# Such a channel therefore gets a manual squelch level (-1 dBFS = 0.696 sqrt(fft size) in |bin| units, whatever the format) and a tone that stays at half of it:
# a tone of a u8 counts reads 0.00216 x fft size x a, so a = 161 / sqrt(fft size); the noise in a bin is a twentieth of the level at these deviations.
WIDE_SHUT_DBFS = -1


def shut_squelch_tone(n_fft):
    return 161.0 / float(np.sqrt(n_fft))


def wide_channel(frequency, modulation=0, has_iq_outputs=0):
    """(an AM channel with raw-I/Q outputs gets the manual squelch level of WIDE_SHUT_DBFS: see there)"""
    return dict(frequency=int(frequency), modulation=modulation, afc=0, squelch_threshold_dbfs=WIDE_SHUT_DBFS if has_iq_outputs and modulation == 0 else 0,
                squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0, ctcss_freq=0.0, bandwidth_hz=0, ampfactor=1.0, tau_us=-1, has_iq_outputs=has_iq_outputs)


def tone_stream(pkg, device, fft_log, wave_rate, n_samples, rng, *, noise, levels, gain=1.0):
    """One dongle's I/Q in its sample format: Gaussian noise plus a steady tone per channel within 0.3 bins of the bin the reference LOOKS at (the library's own
    constants: src/config.cpp:666-667), levels[k] u8 counts high, rounded and clipped to the u8 rails and then re-expressed (convert_format).  Returns (iq, the
    fraction of u8 values on a rail)."""
    n_fft = 1 << fft_log
    t = np.arange(n_samples, dtype=np.float64)
    z = rng.normal(0.0, noise, (n_samples, 2)) @ np.array([1.0, 1j])
    for k in range(len(device["channels"])):
        b = int(pkg.derive_constants([device], k, wave_rate=wave_rate, fft_log=fft_log)[0])
        f = ((b if b < n_fft // 2 else b - n_fft) + float(rng.uniform(-0.3, 0.3))) / n_fft
        z += levels[k] * np.exp(2j * np.pi * (f * t + rng.random()))
    u8 = np.empty(2 * n_samples, np.uint8)
    u8[0::2] = np.clip(np.round(z.real + 127.5), 0, 255)
    u8[1::2] = np.clip(np.round(z.imag + 127.5), 0, 255)
    railed = float(np.mean((u8 == 0) | (u8 == 255)))
    return convert_format(u8, device["sfmt"], pkg.capi, gain), railed


def wide_devices(capi, sfmt, sample_rate, wave_rate, n_dev):
    """The dongles of wide_case(), without streams."""
    devices = _format_devices(capi, sfmt, sample_rate, wave_rate, n_dev)
    for d in range(1, n_dev, 2):
        devices[d]["channels"] = [wide_channel(120_000_000 + int(f * sample_rate), modulation=1 if wave_rate == 16000 and k % 2 == 1 else 0,
                                               has_iq_outputs=1 if k == WIDE_PLAN_B_IQ_CHANNEL else 0) for k, f in enumerate(WIDE_PLAN_B)]
    return devices


def wide_case(pkg, sfmt, fft_log, sample_rate, wave_rate, n_dev, n_batches, first_dongle=0, only=None, info=None):
    """A wide-hop configuration with more than one plan shape on the handle.  Even dongles: format_case's plan (the eight BASELINE channels scaled into the passband).
    Odd dongles: the eleven channels of WIDE_PLAN_B -- two column sets, the second partly filled; bins in the upper half; two channels on one bin; one AM channel with
    raw-I/Q outputs (its squelch held shut: WIDE_SHUT_DBFS); WAVE_RATE 16000: odd channels NFM (raw I/Q stored, no magnitude).  CS16: odd dongles at a quarter of the full scale, as format_case.
    Input: tone_stream() -- even dongles well inside the rails, odd dongles driven into them on about 1 % of the samples (info["railed"][d] = the fraction).
    only: the dongles to make streams for (the others get None).  Returns (devices, iq list in the format's dtype)."""
    capi = pkg.capi
    devices = wide_devices(capi, sfmt, sample_rate, wave_rate, n_dev)
    hop, n_fft = round(sample_rate / wave_rate), 1 << fft_log
    n_samples = (n_batches * (wave_rate // 8) + 100) * hop + n_fft + 8
    iq, railed = [], []
    for d in range(n_dev):
        if only is not None and d not in only:
            iq.append(None)
            railed.append(None)
            continue
        rng = np.random.default_rng([7100, first_dongle + d, int(sfmt), fft_log, sample_rate, wave_rate])
        tone, noise = (WIDE_TONE_B, WIDE_NOISE_B) if d % 2 else (WIDE_TONE_A, WIDE_NOISE_A)
        gain = devices[d]["fullscale"] / 127.5 if sfmt == capi.SFMT_S16 else 1.0
        levels = [shut_squelch_tone(n_fft) if c["squelch_threshold_dbfs"] == WIDE_SHUT_DBFS else tone for c in devices[d]["channels"]]
        x, r = tone_stream(pkg, devices[d], fft_log, wave_rate, n_samples, rng, noise=noise, levels=levels, gain=gain)
        iq.append(x)
        railed.append(r)
    if info is not None:
        info["railed"] = railed
    return devices, iq


def feed_zero_copy(hip, iq, n_batches, misalign):
    """The construction of tests/test_gpu_wide_hops.py::test_zero_copy_spans_sized_to_the_byte for any alignment: every batch through process_device from one
    allocation in which dongle 0's span starts on the first byte, dongle d's d x misalign bytes (mod 16) behind a 16-byte boundary, and the last dongle's span ends
    where the allocation ends -- batch_bytes + lookahead_bytes and not a byte more, so a read past a span is a read past the allocation.
    Yields dict(waveout, axc, w, q) per batch."""
    import torch

    g = hip.geometry
    n_dev, pos = len(iq), 0
    for b in range(n_batches):
        nb = int(g.first_batch_bytes if b == 0 else g.batch_bytes)
        span = nb + int(g.lookahead_bytes)
        stride = (span + 15) // 16 * 16 + misalign
        buf = torch.empty(((n_dev - 1) * stride + span,), dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0 and stride % 16 == misalign % 16
        for d in range(n_dev):
            raw = iq[d].view(np.uint8)[pos:pos + span]
            assert len(raw) == span
            buf[d * stride:d * stride + span] = torch.from_numpy(raw.copy()).cuda()
        torch.cuda.synchronize()
        hip.process_device(buf.data_ptr(), stride)
        out = hip.collect()
        w, q = hip.read_bins()
        yield dict(waveout=out["waveout"].copy(), axc=out["axc"].copy(), w=w.copy(), q=q.copy())
        pos += nb
        del buf


def wait_for_gpu_memory(nbytes: int, timeout_s: float = 60.0) -> None:
    """The driver hands back a freed allocation of >100 GiB (the previous case's resident I/Q) with a delay: wait until that
    much device memory is actually free before asking for it again."""
    import time

    import torch

    t0 = time.time()
    while time.time() - t0 < timeout_s:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        if free >= nbytes:
            return
        time.sleep(0.5)


def boundary_devices(n_dev):
    """NFM + lowpass channels with a manual squelch level and frequencies at which dm_dphi is 0 (src/config.cpp:679-712): what boundary_streams() feeds."""
    chans = [dict(frequency=sg.CENTERFREQ + 16000 * (k + 3), modulation=1, afc=0, squelch_threshold_dbfs=-40, squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0,
                  ctcss_freq=0.0, bandwidth_hz=5000 if k % 2 == 0 else 6250, ampfactor=1.0, tau_us=-1, has_iq_outputs=0) for k in range(8)]
    return [dict(channels=[dict(c) for c in chans]) for _ in range(n_dev)], 0.17666475474834442  # Squelch::squelch_level() of -40 dBFS (the tests assert it)


def boundary_streams(orc_factory, n_dev, B, level):
    """Per channel: quiet, then a steady level just above the squelch level from an onset chosen (with the oracle, two passes) so that the OPENING
    delay runs out on sample 0 of batch 2; 101 samples before that boundary the level steps up by a height swept over the channels."""
    n_ch, n_batches, n0 = n_dev * 8, 3, 2 * B
    steady = 3.5 / 3.0 * level
    onset = np.full(n_ch, n0 - 420)
    step = level * np.geomspace(4.0, 120.0, n_ch)

    def streams(with_step):
        env = np.full((n_ch, n_batches * B), 0.1 * level, np.float64)
        for c in range(n_ch):
            env[c, onset[c]:] = steady
            if with_step:
                env[c, n0 - 101:] += step[c]
        iq = np.zeros((n_ch, 2 * n_batches * B), np.float32)
        iq[:, 0::2] = env.astype(np.float32)  # dm_dphi is 0 at these frequencies: the derotation leaves the samples alone, the lowpass passes their level
        return np.abs(iq[:, 0::2]), iq

    for _ in range(2):  # pass 1 finds where the delay runs out, pass 2 confirms the shifted onsets
        wave, iq = streams(False)
        orc = orc_factory()
        first = np.zeros(n_ch, int)
        for b in range(n_batches):
            for d in range(n_dev):
                r = orc.run_bins(d, wave[8 * d:8 * d + 8, b * B:(b + 1) * B], iq[8 * d:8 * d + 8, 2 * b * B:2 * (b + 1) * B])
                if b == 2:
                    for c in range(8):
                        assert r["trace"][c, 0] & 7 == 1 or _ == 1, "the onset guess leaves no OPENING delay across the boundary"
                        first[8 * d + c] = int(np.argmax((r["trace"][c] & 7) != 1))
        orc.close()
        onset -= first - 1
    assert (first == 1).all(), first
    return streams(True)


def mixer_reference_sum(conns, n_mixers, waveout, axc):
    """What mixer_thread() leaves in mixer->channel for ONE batch when every input was ready (src/mixer.cpp:189-214): inputs in input-index order
    (= connection order per mixer), sum[s] += in[s] * (ampfactor * ampl) in float32, only inputs with signal; right channel for stereo mixers
    (any input with a balance, src/mixer.cpp:84-85); axcindicate = SIGNAL as soon as one input had signal.
    conns: [(device, channel, mixer, ampfactor, balance)]; waveout [device][channel][B] float32, axc [device][channel]."""
    B = waveout.shape[-1]
    left = np.zeros((n_mixers, B), np.float32)
    right = np.zeros((n_mixers, B), np.float32)
    sig = np.zeros((n_mixers,), np.uint8)
    stereo = [any(c[2] == m and c[4] != 0.0 for c in conns) for m in range(n_mixers)]
    for (d, j, m, amp, bal) in conns:
        if axc[d][j] == ord(" "):
            continue
        sig[m] = 1
        ampl = np.float32(min(1.0, 1.0 - np.float32(bal)))
        ampr = np.float32(min(1.0, 1.0 + np.float32(bal)))
        ml, mr = np.float32(amp) * ampl, np.float32(amp) * ampr
        if ml != 0.0:
            left[m] = left[m] + waveout[d][j] * ml
        if stereo[m] and mr != 0.0:
            right[m] = right[m] + waveout[d][j] * mr
    return left, right, sig


def parse_waterfall(text: str):
    """The TUI lines demodulate() prints per channel and batch (src/rtl_airband.cpp:632-643): ESC [ y ; x f, then "%4.0f/%3.0f%c ".
    Returns [(y, x, signal_dBFS, noise_dBFS, symbol)] in print order."""
    import re

    out = []
    for m in re.finditer(r"\x1b\[(\d+);(\d+)f\s*(-?\d+)/\s*(-?\d+)(.) ", text):
        out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5)))
    return out


# ---- AFC at every format / fft size / rate ---------------------------------------------------------------------------------------------------------
AFC_DEFAULT_SHIFTS = [+3, -2, 0, +5, -4, +1, 0, -1]   # transmitter offsets in bins OF THE CHOSEN FFT SIZE
AFC_DEFAULT_AFCS = [2, 1, 3, 10, 2, 255, 0, 0]
# The decision screen's margin m (see afc_format_case): 16 x the largest deviation of a bin's power between a float32 FFT and the float64 one, relative to the
# hop's largest bin power, over the AFC hops of the parametrised configurations and the default fuzz seeds (test_afc_generator.py measures it again and asserts
# that it stays below AFC_SCREEN_MARGIN / 16).
AFC_FFT32_DEVIATION = 1.8e-7
AFC_SCREEN_MARGIN = 16 * AFC_FFT32_DEVIATION


def afc_plan(n_channels=8, afcs=AFC_DEFAULT_AFCS, shifts=AFC_DEFAULT_SHIFTS, base_bins=None):
    """One dongle's AFC plan: [(afc, shift, base_bin)] with the lists cycled over the channels.  shift None: the channel has no transmitter of its own;
    base_bin None: the channel's frequency comes from the spread of afc_format_case."""
    return [(afcs[k % len(afcs)], shifts[k % len(shifts)], None if base_bins is None else base_bins[k]) for k in range(n_channels)]


def afc_reference_bin(frequency, centerfreq, sample_rate, n_fft):
    """src/config.cpp:666-667 (with its INTEGER sample_rate / fft_size)."""
    import math

    return int(math.ceil((frequency + sample_rate - centerfreq) / float(sample_rate // n_fft) - 1.0)) % n_fft


def _afc_frequency_for_bin(want, sample_rate, n_fft):
    q = sample_rate // n_fft
    f = sg.CENTERFREQ + (want if want < n_fft // 2 else want - n_fft) * q
    for _ in range(64):
        got = afc_reference_bin(f, sg.CENTERFREQ, sample_rate, n_fft)
        if got == want:
            return f
        diff = (want - got + n_fft // 2) % n_fft - n_fft // 2
        f += diff * q
    raise AssertionError("no frequency for bin %d" % want)


def afc_last_hop_samples(iq, sfmt, fullscale, capi, n_fft, hop, B, batch):
    """The n_fft complex samples (float64, scaled as the reference scales them) of the LAST hop of output batch `batch`: the first batch consumes B + AGC_EXTRA
    hops, every later one B (src/rtl_airband.cpp:395-492), hop h reads the samples from h * hop on."""
    start = ((batch + 1) * B + capi.AGC_EXTRA - 1) * hop
    raw = np.asarray(iq[2 * start:2 * (start + n_fft)]).astype(np.float64)
    if sfmt == capi.SFMT_U8:
        raw = (raw - 127.5) / 127.5
    elif sfmt == capi.SFMT_S8:
        raw = raw / 128.0
    elif sfmt == capi.SFMT_S16:
        raw = raw / (fullscale if fullscale > 0 else 32766.5)
    return raw[0::2] + 1j * raw[1::2]


def afc_replay_walk(power, n_fft, base, afc):
    """class AFC's walk (src/rtl_airband.cpp:180-251) over float64 bin powers.  Returns (bin, gap): the bin the walk ends on and the smallest distance from a tie
    of any comparison it made (`value <= base_value`, `value - base_value < threshold`)."""
    bv = power[base]
    gap = [np.inf]

    def walk(step):
        thr, b = 0.0, base
        while True:
            if step < 0:
                if b < -step:
                    break
            elif b + step >= n_fft:
                break
            v = power[b + step]
            gap[0] = min(gap[0], abs(v - bv))
            if v <= bv:
                break
            if b == base:
                thr = (v - bv) / float(afc)
            else:
                gap[0] = min(gap[0], abs((v - bv) - thr))
                if (v - bv) < thr:
                    break
                thr = thr + thr / 10.0
            b += step
        return b

    b = walk(-1)
    if b == base:
        b = walk(+1)
    return b, gap[0]


def oracle_batches(orc, d, iq, n_batches):
    """orc.run_device batch by batch, with the channels' bins after EVERY batch: dict of stacked arrays + "bin" [n_batches][C]."""
    C = len(orc.devices[d]["channels"])
    parts, bins = [], []
    for b in range(n_batches):
        r = orc.run_device(d, iq if b == 0 else iq[:0], 1)
        assert r["n_batches"] == 1, "batch %d: the stream is too short" % b
        parts.append(r)
        bins.append([orc.stats(d, j)["bin"] for j in range(C)])
    out = {k: np.concatenate([p[k] for p in parts]) for k in ("waveout", "iq_out", "axc", "trace", "raw_wavein", "raw_iq")}
    out["bin"] = np.array(bins, np.int64)
    out["n_batches"] = n_batches
    return out


def afc_format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, plans, n_batches, first_dongle=0, amplitude=0.08, key=(0.625, 0.25, 0.0625), max_tries=6):
    """format_case with AFC.  plans = one list per dongle of (afc, shift, base_bin) (afc_plan): the channel's afc value, its transmitter's offset from the bin the
    reference LOOKS at (the oracle's constants; src/config.cpp:666-667) in bins of THIS fft size (None: no transmitter of its own), and the bin to put the channel
    on (None: channels spread over +-0.42 of the sample rate, clear of DC).  WAVE_RATE 16000: odd channels are NFM, k % 4 == 1 with a 100 Hz CTCSS tone and notch,
    k % 4 == 3 with a 12.5 kHz lowpass, as in the BASELINE plan.  Every third channel has I/Q outputs, so that its raw bins can be compared.
    key = (period, on, slot) in seconds: every transmitter keys for two batches out of five, (dongle + channel) % 8 slots of half a batch late -- channels k and
    k + 1 of a group open in the same batch, and channel k + 4 opens in the batch in which channel k returns home.

    DECISION SCREEN.  AFC compares float32 bin powers; the GPU's come from a float32 wavefront FFT, the oracle's from a float64 radix-2 rounded to float, so a
    near-tie may resolve either way.  For every batch in which the oracle opens an AFC channel the windowed spectrum of the batch's last hop is recomputed in numpy
    float64 and the walk replayed; a dongle's stream is kept only if every comparison of every such walk clears m * P, P = that hop's largest bin power (and the
    replayed walk must end where the oracle's did).  A stream that is not kept is replaced by the next synthetic dongle's (siggen's dongle index); the case
    counts both.
    m = AFC_SCREEN_MARGIN = 16 x AFC_FFT32_DEVIATION.  Measured on the CPU (tests/test_afc_generator.py, over every parametrised configuration of
    tests/test_gpu_afc.py and the default fuzz seeds, about 650 AFC hops): the largest |P32[k] - P64[k]| / max(P64) between numpy's complex64 FFT of the
    windowed samples and the complex128 one was 1.77e-7 (fft 512, u8); AFC_FFT32_DEVIATION = 1.8e-7, so m = 2.9e-6.

    Returns dict(devices, iq, ref, base, needs_iq, generated, dropped, ups, downs, returns, together, crossed, min_gap, fft32_dev, hops): ref[d] = oracle_batches() of the kept
    stream; ups / downs / returns count the oracle's '<', '>' and returns to the base bin; together = batches in which two channels of one group of eight
    moved, crossed = batches in which one moved while another of its group returned."""
    import pyoracle

    capi = pkg.capi
    n_fft, hop, B = 1 << fft_log, round(sample_rate / wave_rate), wave_rate // 8
    mixed = wave_rate == 16000
    devices = []
    for d, plan in enumerate(plans):
        chans = []
        n = len(plan)
        for k, (afc, shift, base_bin) in enumerate(plan):
            if base_bin is None:
                u = k / max(n - 1, 1)
                frac = -0.42 + 0.78 * u if u < 0.5 else 0.03 + 0.78 * (u - 0.5)
                freq = sg.CENTERFREQ + int(frac * sample_rate)
            else:
                freq = _afc_frequency_for_bin(base_bin, sample_rate, n_fft)
            c = dict(frequency=freq, modulation=0, afc=afc, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0, ctcss_freq=0.0,
                     bandwidth_hz=0, ampfactor=1.0, tau_us=-1, has_iq_outputs=1 if k % 3 == 0 else 0)
            if mixed and k % 2 == 1:
                c["modulation"] = 1
                if k % 4 == 1:
                    c["ctcss_freq"] = c["notch_freq"] = 100.0
                else:
                    c["bandwidth_hz"] = 12500
            chans.append(c)
        gain = (200.0 if d % 2 == 0 else 50.0) if sfmt == capi.SFMT_S16 else 1.0
        devices.append(dict(channels=chans, sample_rate=sample_rate, sfmt=sfmt, fullscale=0.0 if sfmt != capi.SFMT_S16 else 127.5 * gain))
    orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
    try:
        base = [[int(orc.constants(d, k)[0]) for k in range(len(p))] for d, p in enumerate(plans)]
        needs_iq = [[bool(orc.constants(d, k)[13]) for k in range(len(p))] for d, p in enumerate(plans)]
    finally:
        orc.close()
    for d, plan in enumerate(plans):
        for k, (_, _, want) in enumerate(plan):
            assert want is None or base[d][k] == want, (d, k, want, base[d][k])
    window = np.array([pyoracle.lib().orc_window_coeff(n_fft, i) for i in range(n_fft)], np.float64)
    n_samples = (n_batches * B + capi.AGC_EXTRA) * hop + n_fft + 8
    out = dict(devices=devices, iq=[], ref=[], generated=0, dropped=0, ups=0, downs=0, returns=0, together=0, crossed=0, min_gap=np.inf, fft32_dev=0.0, hops=0,
               base=base, needs_iq=needs_iq)
    next_dongle = first_dongle
    for d, plan in enumerate(plans):
        carriers = []
        for k, (afc, shift, _) in enumerate(plan):
            if shift is None:
                continue
            b = base[d][k]
            off = ((b if b < n_fft // 2 else b - n_fft) + shift) * sample_rate / n_fft
            c = devices[d]["channels"][k]
            carriers.append(sg.make_carrier(off, sample_rate, amplitude=amplitude, kind=c["modulation"], ctcss_hz=c["ctcss_freq"], key_slot=k, key_period_s=key[0],
                                            key_on_s=key[1], key_slot_s=key[2]))
        gain = devices[d]["fullscale"] / 127.5 if sfmt == capi.SFMT_S16 else 1.0
        for attempt in range(max_tries):
            iq = convert_format(sg.generate_u8(next_dongle, 0, n_samples, carriers), sfmt, capi, gain)
            next_dongle += 1
            out["generated"] += 1
            orc = pyoracle.Oracle(devices, wave_rate=wave_rate, fft_log=fft_log)
            try:
                ref = oracle_batches(orc, d, iq, n_batches)
            finally:
                orc.close()
            keep, gap_min, dev32, hops = True, np.inf, 0.0, 0
            for b in range(n_batches):
                opening = [k for k, (afc, _, _) in enumerate(plan) if afc and ref["axc"][b][k] != 32 and (b == 0 or ref["axc"][b - 1][k] == 32)]
                if not opening:
                    continue
                x = afc_last_hop_samples(iq, sfmt, devices[d]["fullscale"], capi, n_fft, hop, B, b) * window
                spec = np.fft.fft(x)
                power = spec.real ** 2 + spec.imag ** 2
                P = float(power.max())
                s32 = np.fft.fft(x.astype(np.complex64))
                assert s32.dtype == np.complex64
                p32 = s32.real.astype(np.float32) ** 2 + s32.imag.astype(np.float32) ** 2
                dev32 = max(dev32, float(np.abs(p32.astype(np.float64) - power).max()) / P)
                hops += 1
                for k in opening:
                    end, gap = afc_replay_walk(power, n_fft, base[d][k], plan[k][0] & 0xff)
                    gap_min = min(gap_min, gap / P)
                    if gap < AFC_SCREEN_MARGIN * P:
                        keep = False
                    else:
                        assert end == ref["bin"][b][k], "dongle %d batch %d channel %d: the float64 replay ends on bin %d, the oracle on %d" % (d, b, k, end, ref["bin"][b][k])
            if keep:
                break
            out["dropped"] += 1
        else:
            raise AssertionError("dongle %d: no decision-stable stream in %d tries" % (d, max_tries))
        out["iq"].append(iq)
        out["ref"].append(ref)
        out["min_gap"] = min(out["min_gap"], gap_min)
        out["fft32_dev"] = max(out["fft32_dev"], dev32)
        out["hops"] += hops
        bins, home = ref["bin"], np.array(base[d])
        prev = np.vstack([home[None, :], bins[:-1]])
        up, down = ref["axc"] == ord("<"), ref["axc"] == ord(">")
        back = (prev != home) & (bins == home)
        out["ups"] += int(up.sum())
        out["downs"] += int(down.sum())
        out["returns"] += int(back.sum())
        for g in range(0, len(plan), 8):
            mv = (up | down)[:, g:g + 8].sum(axis=1)
            out["together"] += int((mv >= 2).sum())
            out["crossed"] += int(((mv >= 1) & (back[:, g:g + 8].sum(axis=1) >= 1)).sum())
    return out


# ---- CTCSS at every tone, bank shape and wave rate -------------------------------------------------------------------------------------------------
CTCSS_STANDARD_TONES = [67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3, 131.8, 136.5,
                        141.3, 146.2, 150.0, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5,
                        206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1]  # src/ctcss.cpp:87-100
# Off-list targets (the reference accepts any positive `ctcss`, src/config.cpp:565-590): far below and far above the list (no standard tone is left out of the
# banks, and the target's own Goertzel bins are new ones), just outside it (nothing left out, but the fast bin is a standard tone's), and between two list tones
# (both neighbours left out).  The bank sizes they lead to are read from the library (tests/test_ctcss_sweep.py), not assumed here.
CTCSS_OFFLIST_TARGETS = [33.0, 60.0, 98.7, 260.0, 300.0]
CTCSS_SWEEP_TARGETS = CTCSS_STANDARD_TONES + CTCSS_OFFLIST_TARGETS
CTCSS_SWEEP_BATCHES = 16  # 2 s
_ctcss_sweep_cache = {}


def ctcss_fast_decoy(target, wave_rate):
    """The standard tone nearest to `target` that the detector banks keep (5 Hz or more away, src/ctcss.cpp:105-122) and whose bin of the FAST window (0.05 s, 20 Hz
    wide) is the target's: the fast detector cannot tell the two apart, the slow one (0.4 s, 2.5 Hz) can.  None where no standard tone qualifies.  The bin
    arithmetic is the oracle's restatement of ToneDetector's (orc_tone_coeff, pinned to the reference by tests/test_oracle_vs_reference.py)."""
    import pyoracle

    L, win = pyoracle.lib(), int(wave_rate * 0.05)
    own = L.orc_tone_coeff(target, float(wave_rate), win)
    near = [s for s in CTCSS_STANDARD_TONES if abs(np.float32(target) - np.float32(s)) >= 5 and L.orc_tone_coeff(s, float(wave_rate), win) == own]
    return min(near, key=lambda s: abs(s - target)) if near else None


def ctcss_sweep_plan(wave_rate):
    """The sweep's channels in order: [dict(target, sent, what, kind, notch, keys)].  Per target one channel for each of: the target itself, the next standard tone
    above, the next one below (where they exist), no tone, and a `decoy` -- ctcss_fast_decoy(), or, where there is none, a transmission that starts with the
    target's tone and changes to the nearest standard tone 5 Hz or more away after 0.17 s (`switch`): either way the fast detector finds the tone and the slow
    one overrules it while the squelch is open.  kind: WAVE_RATE 16000 spreads the targets over "nfm" (NFM + CTCSS, the packed hand-off), "nfm_lp" (NFM + lowpass +
    CTCSS) and "am" (AM + CTCSS, both the generic hand-off); WAVE_RATE 8000 has AM channels only.  Every third channel has a notch at its target.
    keys: 1 = one transmission of 1 ... 1.5 s, 2 = two with a closed gap (never on the `target` and `decoy` channels, whose window counts the tests assert)."""
    plan = []
    for i, t in enumerate(CTCSS_SWEEP_TARGETS):
        kind = ("nfm", "nfm_lp", "am")[i % 3] if wave_rate == 16000 else "am"
        above = [s for s in CTCSS_STANDARD_TONES if s > t]
        below = [s for s in CTCSS_STANDARD_TONES if s < t]
        decoy = ctcss_fast_decoy(t, wave_rate)
        sent = [("target", t)] + ([("above", min(above))] if above else []) + ([("below", max(below))] if below else []) + [("none", 0.0)]
        sent.append(("decoy", decoy) if decoy is not None else ("switch", min((s for s in CTCSS_STANDARD_TONES if abs(s - t) >= 5), key=lambda s: abs(s - t))))
        for k, (what, f) in enumerate(sent):
            plan.append(dict(target=t, sent=f, what=what, kind=kind, notch=len(plan) % 3 == 0, keys=2 if what in ("above", "below", "none") and (i + k) % 3 == 0 else 1))
    return plan


def ctcss_sweep_case(wave_rate, seed=0, meta=False):
    """(devices, B, n_batches, streams) in the shape of test_host_wave64.random_scenario: ctcss_sweep_plan()'s channels, eight to a dongle (the last one partly
    filled), and made-up stage-1 output for them -- streams[d] = (wavein [C][n], iq [C][2 n]) -- so that everything behind it is bit-exact against
    pyoracle.Oracle.run_bins.  meta=True: a fifth element, the plan entries per dongle.
    Per channel, seeded: a quiet floor, then a transmission 20 ... 28 dB above it that starts at a sample offset which is no multiple of 50 (detector windows end
    inside a step of the tone kernel) and lasts 1 ... 1.5 s -- the slow detector completes two or more windows, the fast -> slow hand-over of has_tone happens with
    the squelch open -- or two shorter ones with a closed gap (the detectors' reset at the transition to CLOSED, the standing verdict of an idle batch).  The
    sub-tone is a phase rotation exp(j beta sin 2 pi f t) on NFM channels (beta 1.5 ... 3) and amplitude modulation of the envelope on AM channels (depth
    0.3 ... 0.5); a channel without one carries a steady audio tone beyond the far end of the banks (301.3 Hz; 21.3 Hz under the targets at the top) over next to no noise.  Frequencies are those of boundary_devices(): dm_dphi is 0, the derotation in front of the lowpass leaves the samples alone."""
    key = (wave_rate, seed)
    if key not in _ctcss_sweep_cache:
        plan = ctcss_sweep_plan(wave_rate)
        B, n_batches = wave_rate // 8, CTCSS_SWEEP_BATCHES
        n = B * n_batches
        t = np.arange(n) / wave_rate
        devices, streams, metas = [], [], []
        for d0 in range(0, len(plan), 8):
            part = plan[d0:d0 + 8]
            chans = []
            wave = np.zeros((len(part), n), np.float32)
            iq = np.zeros((len(part), 2 * n), np.float32)
            for k, p in enumerate(part):
                rng = np.random.default_rng([seed, wave_rate, d0 + k])
                nfm = p["kind"] != "am"
                chans.append(dict(frequency=sg.CENTERFREQ + 16000 * (k + 3), modulation=1 if nfm else 0, afc=0, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0,
                                  notch_freq=p["target"] if p["notch"] else 0.0, notch_q=10.0 if p["notch"] else 0.0, ctcss_freq=p["target"],
                                  bandwidth_hz=12500 if p["kind"] == "nfm_lp" else 0, ampfactor=1.0, tau_us=-1, has_iq_outputs=0))
                floor = 0.2  # the squelch's noise floor comes down from 5.0 with a time constant of ~530 samples (src/squelch.cpp:477-490): it has settled by 0.35 s at either rate
                level = floor * float(10.0 ** rng.uniform(1.0, 1.4))
                env = np.full(n, floor)
                start = int(rng.uniform(0.35, 0.45) * wave_rate)
                start += 7 if start % 50 == 0 else 0
                if p["keys"] == 1:
                    spans = [(start, start + int(rng.uniform(1.0, 1.5) * wave_rate))]
                else:
                    on1, gap, on2 = int(rng.uniform(0.45, 0.6) * wave_rate), int(rng.uniform(0.15, 0.25) * wave_rate), int(rng.uniform(0.5, 0.6) * wave_rate)
                    gap += 3 if (start + on1 + gap) % 50 == 0 else 0
                    spans = [(start, start + on1), (start + on1 + gap, start + on1 + gap + on2)]
                for a, b in spans:
                    env[a:b] = level
                f = np.full(n, p["sent"] if p["what"] != "switch" else p["target"], np.float64)
                quiet = 1.0
                carrier = 0.0
                if p["what"] == "none":
                    # no sub-tone.  A detector window that holds the start of a transmission holds a decaying offset (the AGC's / the DC block's settling, ~200 samples), and
                    # under a target at the bottom of its banks that reads as the tone.  So these channels carry a steady audio tone next to the OTHER end of the banks
                    # (its leakage into the nearest bank bin outweighs the offset's into the target's), next to no noise, and -- NFM -- a carrier a quarter of the wave rate
                    # off, where the discriminator's mean is the value its DC block starts from (0.5)
                    f[:] = 301.3 if p["target"] < 250.0 else 21.3
                    quiet, carrier = 0.002, np.pi / 2
                if p["what"] == "switch":
                    f[start + int(0.17 * wave_rate):] = p["sent"]
                arg = 2 * np.pi * np.cumsum(f) / wave_rate
                if nfm:
                    beta = float(rng.uniform(1.5, 3.0))
                    ph = np.cumsum(rng.normal(0.0, 0.02 * quiet, n)) + beta * np.sin(arg) + carrier * np.arange(n)
                    z = env * np.exp(1j * ph) + 0.3 * quiet * floor * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
                    re, im = z.real.astype(np.float32), z.imag.astype(np.float32)
                    iq[k, 0::2], iq[k, 1::2] = re, im
                    wave[k] = np.sqrt(re * re + im * im)  # float32 throughout: what stage 1 hands over (src/rtl_airband.cpp:484-487)
                else:
                    depth = float(rng.uniform(0.3, 0.5))
                    wave[k] = np.abs(env * (1.0 + depth * np.sin(arg)) * (1.0 + 0.03 * quiet * rng.standard_normal(n))).astype(np.float32)
            devices.append(dict(channels=chans))
            streams.append((wave, iq))
            metas.append(part)
        _ctcss_sweep_cache[key] = (devices, B, n_batches, streams, metas)
    out = _ctcss_sweep_cache[key]
    return out if meta else out[:4]


def ctcss_bank_shape(pkg, target, wave_rate):
    """(n_tones_fast, n_tones_slow) of a channel with this CTCSS target, from the library's own host code (params.cpp::build_plan)."""
    c = dict(frequency=sg.CENTERFREQ + 48000, modulation=0, afc=0, squelch_threshold_dbfs=0, squelch_snr_threshold_db=-1.0, notch_freq=0.0, notch_q=0.0, ctcss_freq=target,
             bandwidth_hz=0, ampfactor=1.0, tau_us=-1, has_iq_outputs=0)
    v = pkg.derive_constants([dict(channels=[c])], 0, wave_rate=wave_rate)
    return int(v[11]), int(v[12])


def traced_kernels(script, args, must_contain):
    """scripts/<script> --child on a short run (4 dongles, 3 batches, then args) under `rocprofv3 --kernel-trace`: the text of the kernel-trace CSV files, in which
    a test looks for the kernels a handle launched.  The program goes after `--`; counters are not collected.  must_contain: what every such run launches, so
    that a trace without it is no trace -- each entry a kernel's name, or a tuple of names of which one must appear."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        import pytest  # (here: the scripts that borrow this module's signal plans need no pytest)
        pytest.skip("no rocprofv3")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tempfile.mkdtemp(prefix="airband_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.join(root, "scripts", script),
               "--child", "--dongles", "4", "--batches", "3"] + list(args)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:]
        text = "".join(open(f).read() for f in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True))
    finally:
        shutil.rmtree(out, ignore_errors=True)
    for names in must_contain:
        assert any(k in text for k in ([names] if isinstance(names, str) else names)), "the trace holds no %r: %s" % (names, r.stdout[-1000:])
    return text
