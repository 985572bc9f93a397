"""What the gated mixer collect (airband_hip_set_mixer_gate, csrc/mixer_gate.hip) costs and saves: a synthetic fleet of N dongles x 8 channels of the BASELINE
plan (set_signal_plan, generate_iq, process_device) with ONE STEREO MIXER PER DONGLE (its eight channels, balances alternating).  One process holds one handle per
delivery -- no mixer gate (airband_hip_collect_mixers: every mixer's left and right in float32), and gates SIGNAL on every mixer with float32, s16 and ulaw rows,
W = 2 -- fed the same input, so that every batch delivers the same mixers in each.  Per batch: n_active and the share of the mixers that is, the wall time of
collect_mixers() beside collect_active_mixers() of each format (the calls taking turns in who goes first, all into host arrays allocated and touched before the
first batch), and the GPU times of the select, index and pack kernels beside mix_runs_kernel / mix_final_kernel (from a `rocprofv3 --kernel-trace --stats` run of
this script's own child).  The comparison is against collect_mixers() of the same build.

    python scripts/mixer_gate_profile.py --dongles 65535 --batches 8 --out profiles/mixer_gate.json
    python scripts/mixer_gate_profile.py --child --dongles 4 --batches 3 --encoding ulaw    # the workload alone on ONE handle (tests/test_gpu_mixer_gate.py traces it)
    python scripts/mixer_gate_profile.py --child --dongles 4 --batches 3 --encoding off     # ... with mixers and no mixer gate
"""
import argparse
import csv
import ctypes as C
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FORMATS = ("f32", "s16", "ulaw")
PACK = {"f32": "mixer_pack_f32_stereo_kernel", "s16": "mixer_pack_s16_stereo_kernel", "ulaw": "mixer_pack_ulaw_stereo_kernel"}
KERNELS = ("mixer_gate_select_kernel", "mixer_gate_index_kernel", "mix_runs_kernel", "mix_final_kernel") + tuple(PACK.values())
DTYPES = {"f32": np.float32, "s16": np.dtype("<i2"), "ulaw": np.uint8, "alaw": np.uint8}


def child(a):
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    wiring = [(d, c, d, 0.5, 0.5 if c % 2 else -0.5) for d in range(n) for c in range(8)]
    formats = ["off"] + list(FORMATS) if a.encoding == "all" else [a.encoding]
    hips = []
    try:
        for f in formats:
            hip = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hips.append(hip)
            hip.set_mixers(n, wiring)
            if f != "off":
                hip.set_mixer_gate(np.full(n, capi.GATE_SIGNAL, np.uint8), None, None if f == "f32" else f, stereo=True)
            hip.set_signal_plan(carriers)
            print("MIXER_PROFILE_HANDLE %s: %d mixers" % (f, n), flush=True)
        g, B, L = hips[0].geometry, hips[0].B, hips[0].L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        left, right, sig = np.full((n, B), 1, np.float32), np.full((n, B), 1, np.float32), np.full(n, 1, np.uint8)
        out = {f: np.full((n, 2 * B), 1, DTYPES[f]) for f in formats if f != "off"}
        info = {f: np.full(n * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE) for f in formats if f not in ("off", "f32")}
        idx = {f: np.full(n, -1, np.int32) for f in formats if f != "off"}
        start = a.start_batch * g.batch_bytes  # signal time of the first batch: the transmitters key on and off over seconds
        for b in range(a.batches):
            nbytes = (g.first_batch_bytes if b == 0 else g.batch_bytes) + g.lookahead_bytes
            hips[0].generate_iq(buf.data_ptr(), stride, start, nbytes)
            hips[0].synchronize()
            torch.cuda.synchronize()
            start += g.first_batch_bytes if b == 0 else g.batch_bytes
            for hip in hips:  # one handle at a time: a kernel's duration is its own
                hip.process_device(buf.data_ptr(), stride)
                hip.synchronize()
            rec = dict(batch=b, mixers=n)
            order = list(range(len(formats)))
            order = order[b % len(order):] + order[:b % len(order)]  # who goes first takes turns
            for i in order:
                f, hip = formats[i], hips[i]
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                if f == "off":
                    rc = L.airband_hip_collect_mixers(hip.h, left.ctypes.data, right.ctypes.data, sig.ctypes.data)
                else:
                    rc = L.airband_hip_collect_active_mixers(hip.h, C.byref(cnt), idx[f].ctypes.data, out[f].ctypes.data if f == "f32" else None,
                                                             None if f == "f32" else out[f].ctypes.data, None if f == "f32" else info[f].ctypes.data, sig.ctypes.data)
                t1 = time.perf_counter()
                hip._check(rc)
                rec["collect_mixers_s" if f == "off" else "collect_active_%s_s" % f] = t1 - t0
                if f != "off":
                    rec.setdefault("n_active", int(cnt.value))
                    assert rec["n_active"] == int(cnt.value), "batch %d: the handles disagree about the count" % b
            if "n_active" in rec:
                rec["share_delivered"] = rec["n_active"] / n
            if "off" in formats and len(formats) > 1:  # (a sample of) the delivered rows are the definition's on collect_mixers()' sums
                k = min(rec["n_active"], 64)
                for f in formats[1:]:
                    rows, rinfo = capi.mixer_rows_reference(left, right, None if f == "f32" else f, True, idx[f][:k], np.ones(n, np.uint8))
                    assert out[f][:k].tobytes() == rows.tobytes(), "batch %d: %s rows differ from the definition" % (b, f)
                    assert rinfo is None or info[f][:k].tobytes() == rinfo.tobytes(), "batch %d: %s records differ from the definition" % (b, f)
            print("MIXER_PROFILE " + json.dumps(rec), flush=True)
        del buf
    finally:
        for hip in hips:
            hip.close()


def kernel_times(out_dir):
    """per kernel name: the durations (ms) of its dispatches in start order"""
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    out = {}
    for _, name, ms in sorted(rows):
        for k in KERNELS:
            if k in name:
                out.setdefault(k, []).append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65535, help="dongles = mixers (at most 65 535 mixers per handle)")
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--encoding", default="all", choices=("all", "off") + FORMATS + ("alaw",), help="child: one handle per delivery (all), or one handle with this one")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the GPU step (the child under rocprofv3) may take")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_mixer_gate_")
    try:
        # the one GPU step, under a time limit of its own
        cmd = ["timeout", "-k", "10", str(a.timeout), rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch)]
        lines = []
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("MIXER_PROFILE"):
                    print(line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return p.returncode
        recs = [json.loads(line[len("MIXER_PROFILE "):]) for line in lines if line.startswith("MIXER_PROFILE ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    H = 1 + len(FORMATS)  # handles, each with its mixer sums per batch; the gated ones with a select and an index
    for rec in recs:
        b = rec["batch"]

        def mean(name, per_batch):
            v = kt.get(name, [])[b * per_batch:(b + 1) * per_batch]
            return sum(v) / len(v) if v else None

        rec["mix_runs_ms"], rec["mix_final_ms"] = mean("mix_runs_kernel", H), mean("mix_final_kernel", H)
        rec["select_ms"], rec["index_ms"] = mean("mixer_gate_select_kernel", len(FORMATS)), mean("mixer_gate_index_kernel", len(FORMATS))
        for f in FORMATS:
            rec["pack_%s_ms" % f] = kt[PACK[f]][b] if len(kt.get(PACK[f], [])) > b else None
    summary = dict(dongles=a.dongles, channels=a.dongles * 8, mixers=a.dongles, stereo=True, wave_batch=2000, batches=recs)
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
