"""What the band watch (airband_hip_set_band_watch, csrc/band_watch.hip) costs and what it saves, at the shape scripts/band_survey_profile.py measures the survey
at: a synthetic fleet of N u8 dongles x 8 mixed channels at fft 512 (set_signal_plan, generate_iq, process_device on the handle's own stream), K = 8 windows per
batch, every dongle selected, the survey on the MEAN trace with its defaults (8 peaks, median floor, 10 dB, guard 8), the watch with its defaults (8 tracks, match 2,
confirm 2, release 4, 4 x rows event records).
Per batch:
    * GPU time of the survey's kernel and of the watch's two kernels behind it: the kernels' own times from a `rocprofv3 --kernel-trace` run of this script's child;
    * host wall time and bytes of collect_band_events() on a steady band (no event) and on a band that changes every batch (the input alternates between the
      fleet's signal and silence, confirm 1 / release 1: every carrier appears or vanishes, more events than records, max_events records copied);
    * host wall time and bytes of collect_band_survey() for all dongles: what a host without the watch copies every batch before it can track anything.
Every measurement is a child process of its own.  Writes profiles/band_watch.json.

    python scripts/band_watch_profile.py --dongles 65536
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS, MAX_PEAKS, PERMILLE, DB, GUARD = 8, 8, 500, 10.0, 8
TRACKS, MATCH, CONFIRM, RELEASE = 8, 2, 2, 4


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        hip.set_band_scope(windows=WINDOWS, mean=True, peak=True)
        hip.set_band_survey(trace="mean", max_peaks=MAX_PEAKS, floor_permille=PERMILLE, threshold_db=DB, guard_bins=GUARD)
        if a.busy:
            hip.set_band_watch(max_tracks=TRACKS, match_bins=MATCH, confirm_hits=1, release_misses=1)
        else:
            hip.set_band_watch(max_tracks=TRACKS, match_bins=MATCH, confirm_hits=CONFIRM, release_misses=RELEASE)
        hip.set_signal_plan(carriers)
        g = hip.geometry
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        hip.generate_iq(buf.data_ptr(), stride, 4 * g.batch_bytes, g.first_batch_bytes + g.lookahead_bytes)
        quiet = torch.full((n, stride), 128, dtype=torch.uint8, device="cuda") if a.busy else None
        hip.process_device(buf.data_ptr(), stride)  # the first batch, with its lead-in
        hip.synchronize()
        off = g.first_batch_bytes - g.batch_bytes  # later batches re-read the span's last WAVE_BATCH hops: the same work every step
        for _ in range(a.warmup + a.steps):
            hip.process_device(buf.data_ptr() + off, stride)
        hip.synchronize()
        out = dict(dongles=n, max_events=hip.watch_events)
        if a.collects > 0:
            t_events, t_survey, counts = [], [], []
            for i in range(a.collects):
                if a.busy:  # silence and the signal in turn: every batch every carrier vanishes or appears
                    hip.process_device((quiet if i % 2 == 0 else buf).data_ptr() + off, stride)
                else:
                    hip.process_device(buf.data_ptr() + off, stride)
                hip.synchronize()
                t0 = time.perf_counter()
                ev = hip.collect_band_events()
                t_events.append((time.perf_counter() - t0) * 1e3)
                counts.append(ev["n_events"])
                t0 = time.perf_counter()
                got = hip.collect_band_survey()
                t_survey.append((time.perf_counter() - t0) * 1e3)
            rows = hip.collect_band_tracks()["rows"]
            out.update(collect_events_ms=t_events, n_events=counts, events_bytes=[8 + 16 * min(c, hip.watch_events) for c in counts], collect_survey_ms=t_survey,
                       collect_survey_bytes=int(got["summary"].nbytes + got["peaks"].nbytes), tracks_live_mean=float(rows["n_live"].mean()),
                       tracks_confirmed_mean=float(rows["n_confirmed"].mean()), dropped_total=int(rows["dropped"].sum()))
        print("WATCH_PROFILE " + json.dumps(out), flush=True)
        del buf


def run_child(a, collects, busy=False, rocprof_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--steps", str(a.steps), "--warmup", str(a.warmup), "--collects", str(collects)]
    if busy:
        cmd.append("--busy")
    if rocprof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", rocprof_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise RuntimeError("child failed: %d" % r.returncode)
    return [json.loads(line[len("WATCH_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("WATCH_PROFILE ")][0]


def kernel_ms(out_dir, name):
    ms = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if name in r["Kernel_Name"]:
                ms.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [m for _, m in sorted(ms)]


def summary(v):
    return dict(runs=v, median=statistics.median(v), min=min(v), max=max(v)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--collects", type=int, default=6)
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_watch.json"))
    ap.add_argument("--child", action="store_true", help="run the workload itself")
    ap.add_argument("--busy", action="store_true", help="child: a band that changes every batch")
    a = ap.parse_args()
    if a.child:
        return child(a)
    survey, watch, pack = [], [], []
    for _ in range(a.runs):
        d = tempfile.mkdtemp(prefix="airband_watch_")
        try:
            run_child(a, 0, rocprof_dir=d)
            s, w, p = kernel_ms(d, "band_survey_kernel"), kernel_ms(d, "band_watch_kernel"), kernel_ms(d, "band_watch_pack_kernel")
        finally:
            shutil.rmtree(d, ignore_errors=True)
        survey.append(statistics.median(s[1:] or s))  # (the first batch's launches run beside the lead-in's longer stage 1)
        watch.append(statistics.median(w[1:] or w))
        pack.append(statistics.median(p[1:] or p))
    steady = run_child(a, a.collects)  # no profiler here: tracing slows the host
    busy = run_child(a, a.collects, busy=True)
    out = dict(dongles=a.dongles, fft_size=512, sample_format="u8", windows_per_batch=WINDOWS, survey_trace="mean", max_peaks=MAX_PEAKS, max_tracks=TRACKS, match_bins=MATCH,
               confirm_hits=CONFIRM, release_misses=RELEASE, max_events=steady["max_events"],
               survey_kernel_ms=summary(survey), watch_kernel_ms=summary(watch), pack_kernel_ms=summary(pack), watch_plus_pack_ms=summary([x + y for x, y in zip(watch, pack)]),
               steady=dict(collect_events_ms=summary(steady["collect_events_ms"]), n_events=steady["n_events"], events_bytes=steady["events_bytes"],
                           collect_survey_ms=summary(steady["collect_survey_ms"]), collect_survey_bytes=steady["collect_survey_bytes"],
                           tracks_live_mean=steady["tracks_live_mean"], tracks_confirmed_mean=steady["tracks_confirmed_mean"], dropped_total=steady["dropped_total"]),
               busy=dict(confirm_hits=1, release_misses=1, collect_events_ms=summary(busy["collect_events_ms"]), n_events=busy["n_events"], events_bytes=busy["events_bytes"],
                         collect_survey_ms=summary(busy["collect_survey_ms"])))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
