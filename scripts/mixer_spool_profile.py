"""What the mixer transmission spool (airband_hip_set_mixer_spool, csrc/tx_spool.hip behind the mixer gate's pack) costs and saves: a synthetic fleet of N
dongles x 8 channels of the BASELINE plan (set_signal_plan, generate_iq, process_device) with ONE STEREO MIXER PER DONGLE, a SIGNAL mixer gate with mu-law rows,
W = 2, WAVE_BATCH 2000.  One process holds two handles fed the same input:
    spool   the gate and a mixer spool: per batch nothing is collected; collect_mixer_transmissions() is timed with nothing finished (mid-run) and, after a
            flush, with a full export;
    host    the gate alone and the HOST METHOD on the same build: collect_active_mixers() every batch plus vectorised numpy assembly (open / last-write
            clocks per mixer, rows appended into a host row pool, finished clips gathered), timed per batch.
The GPU times of the four step kernels beside the pack kernel come from a `rocprofv3 --kernel-trace` run of this script's own child.

    python scripts/mixer_spool_profile.py --dongles 65535 --batches 8 --out profiles/mixer_spool.json
    python scripts/mixer_spool_profile.py --child --dongles 4 --batches 3 --handles spool    # the workload alone on ONE handle (tests/test_gpu_mixer_spool.py traces it)
    python scripts/mixer_spool_profile.py --child --dongles 4 --batches 3 --handles host     # ... with the mixer gate and no spool
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

STEP_KERNELS = ("spool_scan_kernel", "spool_close_kernel", "spool_append_kernel", "spool_copy_kernel")
KERNELS = STEP_KERNELS + ("mixer_pack_ulaw_stereo_kernel", "mixer_gate_select_kernel", "mixer_gate_index_kernel", "spool_export_kernel", "spool_walk_kernel",
                          "spool_gather_kernel")
RULE = dict(min_batches=2, idle_batches=1, max_batches=16)


class HostMethod:
    """the spool's rule on the host over collect_active_mixers(): numpy, vectorised over the mixers"""

    def __init__(self, n, row_bytes, pool_rows):
        self.pool = np.zeros((pool_rows, row_bytes), np.uint8)
        self.free = list(range(pool_rows))
        self.is_open = np.zeros(n, bool)
        self.open_b, self.last_b, self.n_rows = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        self.slots = np.zeros((n, RULE["max_batches"] + 1), np.int64)
        self.clips = self.clip_rows = 0

    def close(self, c):
        if len(c):
            rows = self.slots[c][np.arange(self.slots.shape[1])[None, :] < self.n_rows[c][:, None]]
            audio = self.pool[rows]  # the finished clips' audio, contiguous in (mixer, step) order
            self.free.extend(rows.tolist())
            self.is_open[c] = False
            self.clips += len(c)
            self.clip_rows += len(audio)

    def step(self, k, mixers, audio):
        age, quiet = k - self.open_b, k - self.last_b
        self.close(np.flatnonzero(self.is_open & (((age > RULE["min_batches"]) & (quiet > RULE["idle_batches"])) | (age > RULE["max_batches"]))))
        new = mixers[~self.is_open[mixers]]
        self.open_b[new], self.n_rows[new], self.is_open[new] = k, 0, True
        take = min(len(mixers), len(self.free))
        if take:
            rows = np.array(self.free[len(self.free) - take:], np.int64)
            del self.free[len(self.free) - take:]
            m = mixers[:take]
            self.pool[rows] = audio[:take]
            self.slots[m, self.n_rows[m]] = rows
            self.n_rows[m] += 1
        self.last_b[mixers] = k

    def flush(self):
        self.close(np.flatnonzero(self.is_open))


def child(a):
    import torch

    torch.set_num_threads(min(16, torch.get_num_threads()))
    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    wiring = [(d, c, d, 0.5, 0.5 if c % 2 else -0.5) for d in range(n) for c in range(8)]
    kinds = ["spool", "host"] if a.handles == "both" else [a.handles]
    pool_rows, export_rows = 2 * n + RULE["max_batches"] + 1, n + RULE["max_batches"] + 1
    hips = {}
    try:
        for kind in kinds:
            hip = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hips[kind] = hip
            hip.set_mixers(n, wiring)
            hip.set_mixer_gate(np.full(n, capi.GATE_SIGNAL, np.uint8), None, "ulaw", stereo=True)
            if kind == "spool":
                hip.set_mixer_spool(pool_rows, export_rows=export_rows, max_records=n, **RULE)
            hip.set_signal_plan(carriers)
            print("MIXER_SPOOL_HANDLE %s: %d mixers" % (kind, n), flush=True)
        first = hips[kinds[0]]
        g, B, L = first.geometry, first.B, first.L
        row_bytes = 2 * B
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        idx, audio = np.full(n, -1, np.int32), np.full((n, row_bytes), 1, np.uint8)
        info, sig = np.full(n * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE), np.full(n, 1, np.uint8)
        records, clip_audio = np.full(n * 12, 0xFFFFFFFF, np.uint32).view(capi.TRANSMISSION_DTYPE), np.full((export_rows, row_bytes), 1, np.uint8)
        host = HostMethod(n, row_bytes, pool_rows) if "host" in hips else None
        cnt, nrec, nrows, nwait = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)

        def collect_spool(rec, name):
            t0 = time.perf_counter()
            first._check(L.airband_hip_collect_mixer_transmissions(hips["spool"].h, C.byref(nrec), records.ctypes.data, clip_audio.ctypes.data, C.byref(nrows), C.byref(nwait)))
            rec[name + "_s"], rec[name + "_n"], rec[name + "_rows"], rec[name + "_waiting"] = time.perf_counter() - t0, nrec.value, nrows.value, nwait.value

        start = a.start_batch * g.batch_bytes  # signal time of the first batch: the transmitters key on and off over seconds
        for b in range(a.batches):
            nbytes = (g.first_batch_bytes if b == 0 else g.batch_bytes) + g.lookahead_bytes
            first.generate_iq(buf.data_ptr(), stride, start, nbytes)
            first.synchronize()
            torch.cuda.synchronize()
            start += g.first_batch_bytes if b == 0 else g.batch_bytes
            rec = dict(batch=b, mixers=n)
            for kind in kinds:  # one handle at a time: a kernel's duration is its own
                hips[kind].process_device(buf.data_ptr(), stride)
                hips[kind].synchronize()
            if host is not None:
                t0 = time.perf_counter()
                first._check(L.airband_hip_collect_active_mixers(hips["host"].h, C.byref(cnt), idx.ctypes.data, None, audio.ctypes.data, info.ctypes.data, sig.ctypes.data))
                t1 = time.perf_counter()
                host.step(b, idx[:cnt.value].astype(np.int64), audio)
                rec["host_collect_s"], rec["host_assembly_s"], rec["n_active"] = t1 - t0, time.perf_counter() - t1, int(cnt.value)
            if "spool" in hips and b == a.batches // 2:
                collect_spool(rec, "collect_mid_run")  # whatever the idle rule finished so far
                collect_spool(rec, "collect_nothing_finished")  # ... and straight again: nothing is waiting
            print("MIXER_SPOOL_PROFILE " + json.dumps(rec), flush=True)
        rec = dict(batch="flush", mixers=n)
        if "spool" in hips:
            hips["spool"].mixer_spool_flush()
            hips["spool"].synchronize()
            collect_spool(rec, "collect_full_export")
            rec["counters"] = hips["spool"].mixer_spool_counters()
        if host is not None:
            t0 = time.perf_counter()
            host.flush()
            rec["host_flush_assembly_s"], rec["host_clips"], rec["host_clip_rows"] = time.perf_counter() - t0, host.clips, host.clip_rows
        print("MIXER_SPOOL_PROFILE " + json.dumps(rec), flush=True)
        del buf
    finally:
        for hip in hips.values():
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
    ap.add_argument("--handles", default="both", choices=("both", "spool", "host"), help="child: both handles, or one of them alone")
    ap.add_argument("--timeout", type=int, default=900, help="seconds the GPU step (the child under rocprofv3) may take")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_mixer_spool_")
    try:
        # the one GPU step, under a time limit of its own: tracing only, no counters
        cmd = ["timeout", "-k", "10", str(a.timeout), rocprof, "--kernel-trace", "--output-format", "csv", "-d", out_dir, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch)]
        lines = []
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("MIXER_SPOOL"):
                    print(line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return p.returncode
        recs = [json.loads(line[len("MIXER_SPOOL_PROFILE "):]) for line in lines if line.startswith("MIXER_SPOOL_PROFILE ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    for rec in recs:
        b = rec["batch"]
        if not isinstance(b, int):
            continue
        for k in STEP_KERNELS:  # one dispatch per batch, on the spooled handle alone
            rec[k.replace("_kernel", "_ms")] = kt[k][b] if len(kt.get(k, [])) > b else None
        pack = kt.get("mixer_pack_ulaw_stereo_kernel", [])  # two handles pack per batch: the spooled one first
        rec["pack_ms"] = pack[2 * b] if len(pack) > 2 * b else None
        steps = [rec[k.replace("_kernel", "_ms")] for k in STEP_KERNELS]
        rec["spool_step_ms"] = sum(steps) if all(s is not None for s in steps) else None
    summary = dict(dongles=a.dongles, channels=a.dongles * 8, mixers=a.dongles, stereo=True, encoding="ulaw", wave_batch=2000, rule=RULE, batches=recs,
                   collect_kernels_ms={k: kt.get(k, []) for k in ("spool_export_kernel", "spool_walk_kernel", "spool_gather_kernel")})
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
