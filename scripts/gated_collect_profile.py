"""What the output gate (airband_hip_set_output_gate, csrc/gate.hip) costs and what it saves: a synthetic fleet of N dongles x 8 channels of the BASELINE plan
(set_signal_plan, generate_iq, process_device), gate SIGNAL on every channel.  Per batch: n_active, the GPU time of the select passes and of the gather
(from a `rocprofv3 --kernel-trace --stats` run of this script's own child), stage 2 and the emit slot from airband_hip_last_timings(), and the wall time
of the full copy (airband_hip_collect_channels of every channel, which does not consume the batch) against airband_hip_collect_active() of the SAME batch,
both into host arrays that were allocated and touched before the first batch.

    python scripts/gated_collect_profile.py --dongles 65536 --batches 8          # prints one line per batch and a JSON summary
    python scripts/gated_collect_profile.py --child --dongles 4 --no-gate       # the workload alone, without a gate (tests/test_gpu_gate.py traces it)
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

SELECT, GATHER = ("gate_select_kernel", "gate_index_kernel"), ("gate_gather_kernel",)


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_ch = a.dongles, a.dongles * 8
    rows = max(1, int(n_ch * a.max_rows_frac))
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000) as hip:
        if not a.no_gate:
            hip.set_output_gate(np.full(n_ch, pkg.capi.GATE_SIGNAL, np.uint8), rows)
        hip.set_signal_plan(carriers)
        g, B, L = hip.geometry, hip.B, hip.L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        wave = np.full((n_ch, B), -1.0, np.float32)  # (np.zeros would hand out untouched pages)
        axc = np.full(n_ch, 1, np.uint8)
        pw = np.full((rows, B), -1.0, np.float32)
        idx = np.full(rows, -1, np.int32)
        start = a.start_batch * g.batch_bytes  # signal time of the first batch: the transmitters key on and off over seconds
        for b in range(a.batches):
            nbytes = (g.first_batch_bytes if b == 0 else g.batch_bytes) + g.lookahead_bytes
            hip.generate_iq(buf.data_ptr(), stride, start, nbytes)
            start += g.first_batch_bytes if b == 0 else g.batch_bytes
            hip.process_device(buf.data_ptr(), stride)
            hip.synchronize()
            t0 = time.perf_counter()
            hip._check(L.airband_hip_collect_channels(hip.h, 0, n_ch, wave.ctypes.data, None, axc.ctypes.data, None))
            t1 = time.perf_counter()
            rec = dict(batch=b, collect_s=t1 - t0, signal_channels=int((axc != 32).sum()))
            if not a.no_gate:
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                hip._check(L.airband_hip_collect_active(hip.h, C.byref(cnt), idx.ctypes.data, pw.ctypes.data, None, axc.ctypes.data))
                t1 = time.perf_counter()
                k = min(int(cnt.value), rows)
                assert np.array_equal(pw[:k].view(np.uint32), wave[idx[:k]].view(np.uint32)), "batch %d: packed rows differ from the full copy" % b
                rec.update(n_active=int(cnt.value), rows_kept=k, collect_active_s=t1 - t0)
            else:
                hip.collect()
            t = hip.last_timings()
            rec.update(stage2_ms=t["demod_ms"], emit_ms=t["emit_ms"])
            print("GATE_PROFILE " + json.dumps(rec), flush=True)
        del buf


def kernel_times(out_dir):
    """per kernel name: the durations (ms) of its dispatches in start order"""
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
    out = {}
    for _, name, ms in sorted(rows):
        for k in SELECT + GATHER:
            if k in name:
                out.setdefault(k, []).append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--max-rows-frac", type=float, default=0.25, help="capacity of the packed buffers as a fraction of the channels")
    ap.add_argument("--no-gate", action="store_true")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_gate_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch), "--max-rows-frac", str(a.max_rows_frac)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode
        recs = [json.loads(line[len("GATE_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("GATE_PROFILE ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    for rec in recs:
        b = rec["batch"]
        rec["select_ms"] = sum(kt[k][b] for k in SELECT if len(kt.get(k, [])) > b)
        rec["gather_ms"] = sum(kt[k][b] for k in GATHER if len(kt.get(k, [])) > b)
        print("batch %(batch)d: n_active %(n_active)d of which kept %(rows_kept)d, select %(select_ms).4f ms, gather %(gather_ms).4f ms, stage 2 %(stage2_ms).3f ms, "
              "emit slot %(emit_ms).3f ms, collect %(collect_s).4f s, collect_active %(collect_active_s).4f s" % rec)
    print(json.dumps(dict(dongles=a.dongles, channels=a.dongles * 8, max_rows=max(1, int(a.dongles * 8 * a.max_rows_frac)), batches=recs)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
