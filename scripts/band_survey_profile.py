"""What the band survey (airband_hip_set_band_survey, csrc/band_survey.hip) costs and what it saves, at the shape scripts/band_scope_profile.py measures the scope
at: a synthetic fleet of N u8 dongles x 8 mixed channels at fft 512 (set_signal_plan, generate_iq, process_device on the handle's own stream), K = 8 windows per
batch, every dongle selected, the scope keeping MEAN and PEAK as there, the survey on the MEAN trace with its defaults (8 peaks, median floor, 10 dB, guard 8).
Per batch:
    * GPU time of the scope launch alone and of scope + survey: the kernels' own times from a `rocprofv3 --kernel-trace` run of this script's child;
    * host wall time and bytes of collect_band_survey() for all dongles;
    * host wall time and bytes of the host doing the same work: collect the MEAN rows of all dongles, then capi.band_survey_reference() on every row.
Every measurement is a child process of its own.  Writes profiles/band_survey.json.

    python scripts/band_survey_profile.py --dongles 65536
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


def child(a):
    import numpy as np
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        hip.set_band_scope(windows=WINDOWS, mean=True, peak=True)
        hip.set_band_survey(trace="mean", max_peaks=MAX_PEAKS, floor_permille=PERMILLE, threshold_db=DB, guard_bins=GUARD)
        hip.set_signal_plan(carriers)
        g = hip.geometry
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        hip.generate_iq(buf.data_ptr(), stride, 4 * g.batch_bytes, g.first_batch_bytes + g.lookahead_bytes)
        hip.process_device(buf.data_ptr(), stride)  # the first batch, with its lead-in
        hip.synchronize()
        off = g.first_batch_bytes - g.batch_bytes  # later batches re-read the span's last WAVE_BATCH hops: the same work every step
        for _ in range(a.warmup + a.steps):
            hip.process_device(buf.data_ptr() + off, stride)
        hip.synchronize()
        out = dict(dongles=n)
        if a.collects > 0:
            bins = [int(hip.constants(j)[0]) for j in range(len(chans))]  # every dongle has the same plan
            ratio = np.float32(10.0 ** (DB / 10.0))
            t_survey, t_rows = [], []
            mean = np.empty((n, g.fft_size), np.float32)
            for _ in range(a.collects):
                t0 = time.perf_counter()
                got = hip.collect_band_survey()
                t_survey.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                hip._check(hip.L.airband_hip_collect_band_scope(hip.h, 0, n, mean.ctypes.data, None))
                t_rows.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            want = [capi.band_survey_reference(mean[d], bins, MAX_PEAKS, PERMILLE, ratio, GUARD) for d in range(n)]
            t_ref = (time.perf_counter() - t0) * 1e3
            same = all(int(got["summary"]["n_peaks"][d]) == want[d]["n_peaks"] and got["summary"]["floor"][d] == want[d]["floor"]
                       and np.array_equal(got["peaks"][d]["bin"], want[d]["peaks"]["bin"]) for d in range(n))
            out.update(collect_survey_ms=t_survey, collect_survey_bytes=int(got["summary"].nbytes + got["peaks"].nbytes), collect_rows_ms=t_rows,
                       collect_rows_bytes=int(mean.nbytes), host_reference_ms=t_ref, survey_equals_host_reference=bool(same),
                       peaks_per_dongle_mean=float(got["summary"]["n_peaks"].mean()))
        print("SURVEY_PROFILE " + json.dumps(out), flush=True)
        del buf


def run_child(a, collects, rocprof_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--steps", str(a.steps), "--warmup", str(a.warmup), "--collects", str(collects)]
    if rocprof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", rocprof_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise RuntimeError("child failed: %d" % r.returncode)
    return [json.loads(line[len("SURVEY_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("SURVEY_PROFILE ")][0]


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
    ap.add_argument("--collects", type=int, default=5)
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_survey.json"))
    ap.add_argument("--child", action="store_true", help="run the workload itself")
    a = ap.parse_args()
    if a.child:
        return child(a)
    scope, survey = [], []
    for _ in range(a.runs):
        d = tempfile.mkdtemp(prefix="airband_survey_")
        try:
            run_child(a, 0, rocprof_dir=d)
            k, s = kernel_ms(d, "band_scope_kernel"), kernel_ms(d, "band_survey_kernel")
        finally:
            shutil.rmtree(d, ignore_errors=True)
        scope.append(statistics.median(k[1:] or k))  # (the first batch's launches run beside the lead-in's longer stage 1)
        survey.append(statistics.median(s[1:] or s))
    host = run_child(a, a.collects)  # no profiler here: tracing slows the host
    out = dict(dongles=a.dongles, fft_size=512, sample_format="u8", windows_per_batch=WINDOWS, scope_traces="mean+peak", survey_trace="mean", max_peaks=MAX_PEAKS,
               floor_permille=PERMILLE, threshold_db=DB, guard_bins=GUARD,
               scope_kernel_ms=summary(scope), survey_kernel_ms=summary(survey), scope_plus_survey_ms=summary([x + y for x, y in zip(scope, survey)]),
               collect_survey_ms=summary(host["collect_survey_ms"]), collect_survey_bytes=host["collect_survey_bytes"],
               collect_rows_ms=summary(host["collect_rows_ms"]), collect_rows_bytes=host["collect_rows_bytes"], host_reference_ms=host["host_reference_ms"],
               collect_rows_plus_host_reference_ms=statistics.median(host["collect_rows_ms"]) + host["host_reference_ms"],
               survey_equals_host_reference=host["survey_equals_host_reference"], peaks_per_dongle_mean=host["peaks_per_dongle_mean"])
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
