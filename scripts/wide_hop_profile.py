"""What AIRBAND_HIP_FLAG_WIDE_HOPS buys: the SAME handle built with the flag (int8 matrix-core channelizer, csrc/channelizer_dft_wide.hip) and without it (the
wavefront FFT), through airband_hip_process_device on HBM-resident I/Q, interleaved in one run.

Per shape -- at fft 512: CS16 10 MS/s in both builds, CS16 6 MS/s and s8 10 MS/s in the WAVE_RATE 8000 build; on the k-segmented staging: CS16 10 MS/s at fft 2048 in
both builds, s8 and CS16 10 MS/s at fft 4096 -- the largest power-of-two dongle count whose resident I/Q (two
batches) fits a quarter of the GPU's memory; eight distinct dongle streams of the test plan (helpers.format_case) repeated over the fleet; REPS interleaved
repetitions of BATCHES timed batches per side; the channelizer's HIP-event time from airband_hip_timing_totals; the bytes the reference consumes per launch (the
windows only where hop >= window, else every byte once) over that time as a fraction of 8 TB/s; and, after the timed region, sampled dongles of the flagged
handle against oracle twins that followed it batch by batch (decisions and counters exact, audio <= 1e-4 RMS: pyverify.SpotCheck).

    python scripts/wide_hop_profile.py profiles/wide_hops.json [--reps 3] [--batches 8] [--max-dongles N]

CF32 (--f32; csrc/channelizer_f32_wide.hip, profiles/wide_hops_f32.json): fft 512 at 6, 8, 10 and 20 MS/s in the WAVE_RATE 8000 build, 10 MS/s in the 16000 build, fft
1024 at 6 MS/s.  The unflagged side is the wavefront FFT exactly as the commit before the float wide-hop kernel ran these shapes (that kernel is untouched); at 20 MS/s
prepare() refuses the unflagged handle, so the record holds the flagged handle's time alone.  The float kernel is bound by the float32 matrix pipe, so every record also
carries its fraction of that pipe's peak: 64 x fft_size flop per hop and group of 8 channels over 256 CUs x 256 flop per clock x 2.4 GHz = 157.3 Tflop/s.

    python scripts/wide_hop_profile.py profiles/wide_hops_f32.json --f32
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

# (sample format, sample rate, WAVE_RATE, fft_log); --shapes takes indices into this list
SHAPES = [("SFMT_S16", 10_000_000, 8000, 9), ("SFMT_S16", 10_000_000, 16000, 9), ("SFMT_S16", 6_000_000, 8000, 9), ("SFMT_S8", 10_000_000, 8000, 9),
          ("SFMT_S16", 10_000_000, 8000, 11), ("SFMT_S16", 10_000_000, 16000, 11), ("SFMT_S8", 10_000_000, 8000, 12), ("SFMT_S16", 10_000_000, 8000, 12)]
F32_SHAPES = [("SFMT_F32", 6_000_000, 8000, 9), ("SFMT_F32", 8_000_000, 8000, 9), ("SFMT_F32", 10_000_000, 8000, 9), ("SFMT_F32", 20_000_000, 8000, 9),
              ("SFMT_F32", 10_000_000, 16000, 9), ("SFMT_F32", 6_000_000, 8000, 10)]
F32_MATRIX_FLOPS = 256 * 256 * 2.4e9
DISTINCT = 8
HBM_BYTES_PER_S = 8e12


def run_shape(pkg, torch, sfmt_name, sample_rate, wave_rate, fft_log, a):
    import helpers
    import pyverify

    capi = pkg.capi
    sfmt = getattr(capi, sfmt_name)
    devs8, iq8 = helpers.format_case(pkg, sfmt, fft_log, sample_rate, wave_rate, DISTINCT, 2)
    f32 = sfmt == capi.SFMT_F32
    # (geometry does not depend on the channelizer; CF32 at 20 MS/s has no wavefront-FFT handle to ask)
    with pkg.AirbandHip(devs8[:1], wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS if f32 else capi.FLAG_FORCE_FFT) as probe:
        g = probe.geometry
        first, batch, look = int(g.first_batch_bytes), int(g.batch_bytes), int(g.lookahead_bytes)
    span = first + batch + look
    stride = (span + 255) // 256 * 256
    quarter = torch.cuda.mem_get_info()[1] // 4
    n_dev = 1
    while 2 * n_dev * stride <= quarter and 2 * n_dev <= a.max_dongles:
        n_dev *= 2
    helpers.wait_for_gpu_memory(n_dev * stride + (8 << 30))
    iq = torch.empty((n_dev, stride), dtype=torch.uint8, device="cuda")
    for k in range(DISTINCT):  # dongle d replays stream d mod 8 (odd CS16 dongles have their own full scale: 8 is even)
        row = torch.from_numpy(iq8[k].view(np.uint8)[:span].copy()).cuda()
        iq[k::DISTINCT, :span] = row
    torch.cuda.synchronize()
    devices = [devs8[d % DISTINCT] for d in range(n_dev)]
    hop_bytes = 2 * round(sample_rate / wave_rate) * capi.BYTES_PER_SAMPLE[sfmt]
    win_bytes = 2 * (1 << fft_log) * capi.BYTES_PER_SAMPLE[sfmt]
    n_hops = batch // hop_bytes
    consumed = n_dev * (n_hops * win_bytes if hop_bytes >= win_bytes else n_hops * hop_bytes + win_bytes - hop_bytes)
    dongles = pyverify.sample_dongles(n_dev, 12)
    host = {d: iq8[d % DISTINCT].view(np.uint8) for d in dongles}
    wide = pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_WIDE_HOPS | capi.FLAG_TRACE_SQUELCH)
    try:
        base = pkg.AirbandHip(devices, wave_rate=wave_rate, fft_log=fft_log, flags=capi.FLAG_TRACE_SQUELCH)
    except pkg.AirbandError as e:  # CF32 at 20 MS/s: refused without the flag
        assert f32 and e.code == capi.EBADSIZE, e
        base, refusal = None, str(e)
    spot = pyverify.SpotCheck(lambda d: devices[d], dongles, wave_rate=wave_rate, fft_log=fft_log)
    try:
        assert wide.channelizer_name() == ("dft_mfma_f32" if f32 else "dft_mfma_i8"), wide.channelizer_reason()
        assert base is None or base.channelizer_name() == "fft_wave64", base.channelizer_reason()
        sides = [("wide", wide)] + ([("base", base)] if base is not None else [])

        def step(hip, off, follow):
            hip.process_device(iq.data_ptr() + off, stride)
            if follow:
                spot.feed([host[d][off:] for d in dongles])

        for _, hip in sides:  # the first batch (its AGC lead-in), untimed
            step(hip, 0, hip is wide)
            hip.synchronize()
        ms = {"wide": [], "base": []}
        for r in range(a.reps):
            for name, hip in sides:
                hip.timing_totals(reset=True)
                for b in range(a.batches):  # the second resident batch, over and over: the oracle twins follow the same spans
                    step(hip, first, hip is wide)
                t = hip.timing_totals(reset=True)
                assert t["batches"] == a.batches
                ms[name].append(t["channelizer_ms"] / a.batches)
        worst = spot.compare(wide, trace=True, what="%s %d S/s WAVE_RATE %d fft %d, %d dongles" % (sfmt_name, sample_rate, wave_rate, 1 << fft_log, n_dev))
        opened = sum(int((r["axc"] == ord("*")).sum()) for r in spot.last)
    finally:
        spot.close()
        wide.close()
        if base is not None:
            base.close()
        del iq
        torch.cuda.empty_cache()
    if f32:
        w = np.array(ms["wide"])
        flop = float(n_dev) * n_hops * 64 * (1 << fft_log) * ((len(devices[0]["channels"]) + 7) // 8)
        rec = dict(sfmt=sfmt_name, sample_rate=sample_rate, wave_rate=wave_rate, fft_size=1 << fft_log, segments=pkg.wide_hop_plan_f32(1 << fft_log, hop_bytes // 8)[0], hop_bytes=hop_bytes,
                   window_bytes=win_bytes, dongles=n_dev, hops_per_batch=n_hops, reps=a.reps, batches_per_rep=a.batches, wide_ms=[float(x) for x in w], wide_ms_median=float(np.median(w)),
                   matrix_flop_per_launch=flop, f32_matrix_peak_fraction_wide=float(flop / (np.median(w) * 1e-3) / F32_MATRIX_FLOPS),
                   consumed_bytes_per_launch=int(consumed), roofline_fraction_wide=float(consumed / (np.median(w) * 1e-3) / HBM_BYTES_PER_S),
                   spot_check=dict(dongles=len(dongles), batches=spot.batches, open_channels_last_batch=opened, worst_audio_rms=float(worst["audio_rms"])))
        if base is None:
            rec["fft_wave64"] = "refused: " + refusal
        else:
            b = np.array(ms["base"])
            spread = float(max(w.max() - w.min(), b.max() - b.min()))
            rec.update(fft_wave64_ms=[float(x) for x in b], fft_wave64_ms_median=float(np.median(b)), spread_ms=spread, speedup=float(np.median(b) / np.median(w)),
                       faster_by_more_than_spread=bool(b.min() - w.max() > spread), every_wide_rep_beats_every_fft_rep=bool(w.max() < b.min()),
                       roofline_fraction_fft_wave64=float(consumed / (np.median(b) * 1e-3) / HBM_BYTES_PER_S))
        print(json.dumps(rec), flush=True)
        return rec
    w, b = np.array(ms["wide"]), np.array(ms["base"])
    spread = float(max(w.max() - w.min(), b.max() - b.min()))
    rec = dict(sfmt=sfmt_name, sample_rate=sample_rate, wave_rate=wave_rate, fft_size=1 << fft_log, segments=pkg.wide_hop_plan(1 << fft_log, hop_bytes, sfmt)[0], hop_bytes=hop_bytes, window_bytes=win_bytes, dongles=n_dev, hops_per_batch=n_hops,
               reps=a.reps, batches_per_rep=a.batches, wide_ms=[float(x) for x in w], fft_wave64_ms=[float(x) for x in b], wide_ms_median=float(np.median(w)),
               fft_wave64_ms_median=float(np.median(b)), spread_ms=spread, speedup=float(np.median(b) / np.median(w)), faster_by_more_than_spread=bool(b.min() - w.max() > spread), every_wide_rep_beats_every_fft_rep=bool(w.max() < b.min()),
               consumed_bytes_per_launch=int(consumed), stream_bytes_per_launch=int(n_dev * batch), roofline_fraction_wide=float(consumed / (np.median(w) * 1e-3) / HBM_BYTES_PER_S),
               roofline_fraction_fft_wave64=float(consumed / (np.median(b) * 1e-3) / HBM_BYTES_PER_S), spot_check=dict(dongles=len(dongles), batches=spot.batches, open_channels_last_batch=opened,
                                                                                                                 worst_audio_rms=float(worst["audio_rms"])))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--max-dongles", type=int, default=1 << 20)
    ap.add_argument("--shapes", type=str, default="")
    ap.add_argument("--f32", action="store_true", help="the CF32 shapes (profiles/wide_hops_f32.json)")
    a = ap.parse_args()
    assert a.reps >= 3 and a.batches >= 8, "at least three interleaved repetitions of at least eight timed batches"
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    table = F32_SHAPES if a.f32 else SHAPES
    shapes = [table[int(i)] for i in a.shapes.split(",")] if a.shapes else table
    recs = [run_shape(pkg, torch, *s, a) for s in shapes]
    out = dict(gpu=torch.cuda.get_device_name(0), build_info=pkg.load_library().airband_hip_build_info().decode(), hbm_roofline_bytes_per_s=HBM_BYTES_PER_S, shapes=recs)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
