"""What the band scope (airband_hip_set_band_scope, csrc/band_scope.hip) costs at the BASELINE configs[2] shape: a synthetic fleet of N u8 dongles x 8 mixed
channels at fft 512 (set_signal_plan, generate_iq, process_device on the handle's own stream: the default, run-ahead schedule), K windows per batch, every dongle
selected, MEAN and PEAK.  Interleaved on one box, RUNS times each:
    * the step time (wall, per batch, over STEPS batches enqueued back to back) with the scope and without it;
    * the same without the scope on another build of the library (--parent-lib: the parent commit's libairband_hip.so), when one is given;
    * the scope kernel's own time, from a `rocprofv3 --kernel-trace` run of this script's child.
Every measurement is a child process of its own (one library per process).  Writes profiles/band_scope.json: per variant the runs, their median and spread.

    python scripts/band_scope_profile.py --dongles 65536 --windows 8 [--parent-lib /path/to/parent/libairband_hip.so]
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


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        if a.windows > 0:
            hip.set_band_scope(windows=a.windows, mean=True, peak=True)
        hip.set_signal_plan(carriers)
        g = hip.geometry
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        start = 4 * g.batch_bytes
        hip.generate_iq(buf.data_ptr(), stride, start, g.first_batch_bytes + g.lookahead_bytes)
        hip.process_device(buf.data_ptr(), stride)  # the first batch, with its lead-in
        hip.synchronize()
        off = g.first_batch_bytes - g.batch_bytes  # later batches re-read the span's last WAVE_BATCH hops: the same work every step
        for _ in range(a.warmup):
            hip.process_device(buf.data_ptr() + off, stride)
        hip.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            hip.process_device(buf.data_ptr() + off, stride)
        hip.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        if a.windows > 0:
            assert hip.collect_band_scope(0, 1)["mean"].any()
        print("SCOPE_PROFILE " + json.dumps(dict(step_ms=ms, windows=a.windows, lib=os.environ.get("AIRBAND_HIP_LIB", ""))), flush=True)
        del buf


def run_child(a, windows, lib=None, rocprof_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--windows", str(windows), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    env = dict(os.environ)
    if lib:
        env["AIRBAND_HIP_LIB"] = lib
    if rocprof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", rocprof_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=a.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise RuntimeError("child failed: %d" % r.returncode)
    return [json.loads(line[len("SCOPE_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("SCOPE_PROFILE ")][0]


def scope_kernel_ms(out_dir):
    ms = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "band_scope_kernel" in r["Kernel_Name"]:
                ms.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    return [m for _, m in sorted(ms)]


def summary(v):
    return dict(runs=v, median=statistics.median(v), min=min(v), max=max(v)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libairband_hip.so of the parent commit: its step time without a scope, interleaved with this build's")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_scope.json"))
    ap.add_argument("--child", action="store_true", help="run the workload itself")
    a = ap.parse_args()
    if a.child:
        return child(a)
    with_scope, without, parent, kernel = [], [], [], []
    for _ in range(a.runs):  # interleaved: whatever else the box does hits every variant alike
        with_scope.append(run_child(a, a.windows)["step_ms"])
        without.append(run_child(a, 0)["step_ms"])
        if a.parent_lib:
            parent.append(run_child(a, 0, lib=a.parent_lib)["step_ms"])
        d = tempfile.mkdtemp(prefix="airband_scope_")
        try:
            run_child(a, a.windows, rocprof_dir=d)
            k = scope_kernel_ms(d)
        finally:
            shutil.rmtree(d, ignore_errors=True)
        kernel.append(statistics.median(k[1:] or k))  # (the first batch's launch runs beside the lead-in's longer stage 1)
    out = dict(dongles=a.dongles, channels=a.dongles * 8, fft_size=512, sample_format="u8", windows_per_batch=a.windows, traces="mean+peak", steps=a.steps,
               scope_kernel_ms=summary(kernel), step_ms_with_scope=summary(with_scope), step_ms_without_scope=summary(without),
               step_ms_parent_commit=summary(parent))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
