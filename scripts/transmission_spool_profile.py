"""What the transmission spool (airband_hip_set_transmission_spool, csrc/tx_spool.hip) costs and saves: a synthetic fleet of N dongles x 8 channels of the
BASELINE plan (set_signal_plan, generate_iq, process_device), gate SIGNAL on every channel, G.711 rows, as in scripts/audio_encoding_profile.py.  One process
holds two handles fed the same input: one with a spool, and one without on which the HOST does the spool's work -- airband_hip_collect_active_encoded() every
batch and the same assembly in numpy (per-channel open / last-write clocks, a host row pool filled by one fancy-indexed copy per batch, a row table per channel,
the closing rule, clips cut by a gather).  Per batch: the GPU time of the spool's four kernels beside the encode kernel's (from a `rocprofv3 --kernel-trace
--stats` run of this script's own child) and the wall time of the host method; every `--collect-every` batches the wall time of
airband_hip_collect_transmissions() and what it returned.  Whether both methods finished the same transmissions is reported.

    python scripts/transmission_spool_profile.py --dongles 65536 --batches 16 --out profiles/transmission_spool.json
    python scripts/transmission_spool_profile.py --child --dongles 4 --handles spool   # the workload alone on ONE handle (tests/test_gpu_transmission_spool.py traces it)
    python scripts/transmission_spool_profile.py --child --dongles 4 --handles host    # ... with a gate and an encoding and no spool
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

ENCODE = "audio_pack_ulaw_kernel"
SPOOL_KERNELS = ("spool_scan_kernel", "spool_close_kernel", "spool_append_kernel", "spool_copy_kernel")
COLLECT_KERNELS = ("spool_export_kernel", "spool_walk_kernel", "spool_gather_kernel")


class HostSpool:
    """The definition on the host, vectorised: what a consumer of collect_active_encoded() has to do per batch, for the rows the gate
    it lists; rows past the gate's max_rows never reach the host."""

    def __init__(self, n_ch, B, pool_rows, min_batches, idle_batches, max_batches):
        self.min_b, self.idle_b, self.max_b = min_batches, idle_batches, max_batches
        self.open = np.zeros(n_ch, bool)
        self.open_batch = np.zeros(n_ch, np.int64)
        self.last_batch = np.zeros(n_ch, np.int64)
        self.n_rows = np.zeros(n_ch, np.int32)
        self.table = np.zeros((n_ch, max_batches + 1), np.int32)  # the pool rows of a channel's open transmission
        self.pool = np.zeros((pool_rows, B), np.uint8)
        self.free = np.arange(pool_rows, dtype=np.int32)
        self.n_free = pool_rows
        self.k = 0
        self.lost = 0

    def step(self, channels, audio):
        k = self.k
        age, quiet = k - self.open_batch, k - self.last_batch
        closing = np.flatnonzero(self.open & (((age > self.min_b) & (quiet > self.idle_b)) | (age > self.max_b)))
        clips = []
        if len(closing):
            counts = self.n_rows[closing]
            rows = np.concatenate([self.table[c, :n] for c, n in zip(closing, counts)]) if counts.sum() else np.zeros(0, np.int32)
            clips = [closing, counts, self.pool[rows]]  # the clips' audio, cut
            self.free[self.n_free:self.n_free + len(rows)] = rows
            self.n_free += len(rows)
            self.open[closing] = False
        n = len(channels)
        if n:
            fresh = channels[~self.open[channels]]
            self.open[fresh] = True
            self.open_batch[fresh] = k
            self.n_rows[fresh] = 0
            m = min(n, self.n_free)  # a dry pool stores the first rows in channel order, as the definition does
            rows = self.free[self.n_free - m:self.n_free][::-1]
            self.n_free -= m
            self.pool[rows] = audio[:m]
            self.table[channels[:m], self.n_rows[channels[:m]]] = rows
            self.n_rows[channels[:m]] += 1
            self.lost += n - m
            self.last_batch[channels] = k
        self.k += 1
        return clips


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_ch = a.dongles, a.dongles * 8
    rows = max(1, int(n_ch * a.max_rows_frac))
    pool_rows = rows * a.pool_batches
    export_rows = max(pool_rows, a.max_batches + 1)
    kinds = ["spool", "host"] if a.handles == "both" else [a.handles]
    hips = {}
    try:
        for kind in kinds:
            hip = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hips[kind] = hip
            hip.set_output_gate(np.full(n_ch, capi.GATE_SIGNAL, np.uint8), rows)
            hip.set_output_encoding("ulaw")
            if kind == "spool":
                hip.set_transmission_spool(pool_rows, export_rows=export_rows, max_records=n_ch, min_batches=a.min_batches, idle_batches=a.idle_batches,
                                           max_batches=a.max_batches)
            hip.set_signal_plan(carriers)
            print("SPOOL_PROFILE_HANDLE %s: %d channels, %d rows, pool %d rows" % (kind, n_ch, rows, pool_rows), flush=True)
        first = hips[kinds[0]]
        g, B, L = first.geometry, first.B, first.L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        if "host" in hips:
            audio = np.full((rows, B), 1, np.uint8)
            info = np.full(rows * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE)
            idx = np.full(rows, -1, np.int32)
            axc = np.full(n_ch, 1, np.uint8)
            host = HostSpool(n_ch, B, pool_rows, a.min_batches, a.idle_batches, a.max_batches)
            host.pool[:] = 1
        if "spool" in hips:
            records = np.zeros(n_ch, capi.TRANSMISSION_DTYPE)
            clips = np.full((export_rows, B), 1, np.uint8)
        host_finished = gpu_finished = host_clip_rows = gpu_clip_rows = 0
        start = a.start_batch * g.batch_bytes  # signal time of the first batch: the transmitters key on and off over seconds
        for b in range(a.batches):
            nbytes = (g.first_batch_bytes if b == 0 else g.batch_bytes) + g.lookahead_bytes
            first.generate_iq(buf.data_ptr(), stride, start, nbytes)
            first.synchronize()
            torch.cuda.synchronize()
            start += g.first_batch_bytes if b == 0 else g.batch_bytes
            for hip in hips.values():  # one handle at a time: a kernel's duration is its own
                hip.process_device(buf.data_ptr(), stride)
                hip.synchronize()
            rec = dict(batch=b)
            if "host" in hips:
                hip = hips["host"]
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                hip._check(L.airband_hip_collect_active_encoded(hip.h, C.byref(cnt), idx.ctypes.data, audio.ctypes.data, info.ctypes.data, axc.ctypes.data))
                t1 = time.perf_counter()
                k = min(int(cnt.value), rows)
                done = host.step(idx[:k], audio[:k])
                t2 = time.perf_counter()
                rec.update(n_active=int(cnt.value), host_collect_s=t1 - t0, host_assembly_s=t2 - t1, host_finished=len(done[0]) if done else 0)
                if done:
                    host_finished += len(done[0])
                    host_clip_rows += int(done[1].sum())
            if "spool" in hips and b % a.collect_every == a.collect_every - 1:
                hip = hips["spool"]
                nn, nr, nw = C.c_int64(0), C.c_int64(0), C.c_int64(0)
                t0 = time.perf_counter()
                hip._check(L.airband_hip_collect_transmissions(hip.h, C.byref(nn), records.ctypes.data, clips.ctypes.data, C.byref(nr), C.byref(nw)))
                t1 = time.perf_counter()
                rec.update(collect_transmissions_s=t1 - t0, transmissions=int(nn.value), clip_rows=int(nr.value), waiting=int(nw.value))
                gpu_finished += int(nn.value)
                gpu_clip_rows += int(nr.value)
            print("SPOOL_PROFILE " + json.dumps(rec), flush=True)
        if "spool" in hips:
            cn = hips["spool"].spool_counters()
            print("SPOOL_PROFILE_COUNTERS " + json.dumps(cn), flush=True)
            if "host" in hips:  # do both methods agree?  (They must where the gate listed every selected row: rows_lost_total == 0.)
                print("SPOOL_PROFILE_CHECK " + json.dumps(dict(host_finished=host_finished, host_clip_rows=host_clip_rows, gpu_collected=gpu_finished,
                                                               gpu_clip_rows=gpu_clip_rows, host_rows_lost=host.lost, same_transmissions=cn["finished_total"] == host_finished)), flush=True)
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
        for k in (ENCODE,) + SPOOL_KERNELS + COLLECT_KERNELS:
            if k in name:
                out.setdefault(k, []).append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--max-rows-frac", type=float, default=0.25, help="capacity of the gate's packed buffers as a fraction of the channels")
    ap.add_argument("--pool-batches", type=int, default=4, help="pool rows = this many batches of max_rows rows")
    ap.add_argument("--min-batches", type=int, default=8)
    ap.add_argument("--idle-batches", type=int, default=4)
    ap.add_argument("--max-batches", type=int, default=64)
    ap.add_argument("--collect-every", type=int, default=8)
    ap.add_argument("--handles", default="both", choices=("both", "spool", "host"), help="child: a spooled handle and one for the host method, or one of them")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_spool_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child"]
        for k in ("dongles", "batches", "start_batch", "max_rows_frac", "pool_batches", "min_batches", "idle_batches", "max_batches", "collect_every"):
            cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
        lines = []
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("SPOOL_PROFILE"):
                    print(line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return p.returncode
        recs = [json.loads(line[len("SPOOL_PROFILE "):]) for line in lines if line.startswith("SPOOL_PROFILE ")]
        counters = [json.loads(line[len("SPOOL_PROFILE_COUNTERS "):]) for line in lines if line.startswith("SPOOL_PROFILE_COUNTERS ")]
        checks = [json.loads(line[len("SPOOL_PROFILE_CHECK "):]) for line in lines if line.startswith("SPOOL_PROFILE_CHECK ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    for rec in recs:
        b = rec["batch"]
        enc = kt.get(ENCODE, [])[2 * b:2 * b + 2]  # two handles, each with an encode launch per batch
        rec["encode_ms"] = sum(enc) / len(enc) if enc else None
        for k in SPOOL_KERNELS:
            rec[k.replace("_kernel", "_ms")] = kt[k][b] if len(kt.get(k, [])) > b else None
        rec["spool_step_ms"] = sum(rec[k.replace("_kernel", "_ms")] or 0.0 for k in SPOOL_KERNELS)
    collects = [r for r in recs if "collect_transmissions_s" in r]
    for i, rec in enumerate(collects):
        for k in COLLECT_KERNELS:
            rec[k.replace("_kernel", "_ms")] = kt[k][i] if len(kt.get(k, [])) > i else None
    rows = max(1, int(a.dongles * 8 * a.max_rows_frac))
    summary = dict(dongles=a.dongles, channels=a.dongles * 8, max_rows=rows, pool_rows=rows * a.pool_batches, wave_batch=2000, encoding="ulaw",
                   min_batches=a.min_batches, idle_batches=a.idle_batches, max_batches=a.max_batches, collect_every=a.collect_every,
                   counters=counters[0] if counters else None, check=checks[0] if checks else None, batches=recs)
    text = json.dumps(summary)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
