"""What the RTP packet stream (airband_hip_set_rtp_stream, csrc/rtp_stream.hip) costs and saves: a synthetic fleet of N dongles x 8 channels of the BASELINE plan
(set_signal_plan, generate_iq, process_device), gate SIGNAL on every channel, mu-law, as in scripts/audio_encoding_profile.py.  One process holds two handles fed
the same input: one with an RTP stream of F samples per frame, one with gate and encoding only.  Per batch: n_active, the packet count, the GPU time of the three
rtp_ kernels beside the pack kernel's (from a `rocprofv3 --kernel-trace --stats` run of this script's own child), and the wall time of
airband_hip_collect_rtp_packets() beside the host method of a library without the stream: airband_hip_collect_active_encoded() plus the packetisation of those
rows by capi.rtp_stream_reference().  That reference is plain Python: it OVERSTATES what a C host loop would take by one to two orders of magnitude; read it as "the work
that no longer exists on the host", not as a benchmark of a competent host implementation.  The first --check-packets packets of every batch are compared with
the handle's, byte for byte, and so is the count.

    python scripts/rtp_stream_profile.py --dongles 65536 --batches 8 --out profiles/rtp_stream.json
    python scripts/rtp_stream_profile.py --child --dongles 4 --rtp 160      # the workload alone on ONE handle (tests/test_gpu_rtp_stream.py traces it)
    python scripts/rtp_stream_profile.py --child --dongles 4 --rtp none     # ... with a gate and an encoding and no stream
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

PACK = "audio_pack_ulaw_kernel"
KERNELS = (PACK, "rtp_count_kernel", "rtp_scan_kernel", "rtp_write_kernel")


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_ch = a.dongles, a.dongles * 8
    rows = max(1, int(n_ch * a.max_rows_frac))
    F = None if a.rtp == "none" else int(a.rtp)
    kinds = ["enc"] if F is None else (["rtp", "enc"] if a.compare else ["rtp"])
    hips = {}
    try:
        for kind in kinds:
            hip = hips[kind] = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hip.set_output_gate(np.full(n_ch, capi.GATE_SIGNAL, np.uint8), rows)
            hip.set_output_encoding("ulaw")
            if kind == "rtp":
                hip.set_rtp_stream(F, max_packets=rows * ((F - 4 + hip.B) // F + 1))  # every listed row's packets, and a flush for as many channels
            hip.set_signal_plan(carriers)
            print("RTP_PROFILE_HANDLE %s: %d channels, %d rows" % (kind, n_ch, rows), flush=True)
        first = hips[kinds[0]]
        g, B, L = first.geometry, first.B, first.L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        audio = np.full((rows, B), 1, np.uint8)
        info = np.full(rows * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE)
        idx = np.full(rows, -1, np.int32)
        axc = np.full(n_ch, 1, np.uint8)
        if F is not None:
            r = hips["rtp"].rtp
            records = np.full(r["max_packets"] * 4, 0xFFFFFFFF, np.uint32).view(capi.RTP_PACKET_DTYPE)
            slots = np.full((r["max_packets"], r["slot_bytes"]), 1, np.uint8)
            # the host method's model: the first --host-rows channels of the fleet, which is where the first listed rows come from
            model = capi.rtp_stream_reference(r["sources"], "ulaw", B, F, r["max_packets"]) if a.compare else None
        start = a.start_batch * g.batch_bytes
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
            if "enc" in hips:
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                rc = L.airband_hip_collect_active_encoded(hips["enc"].h, C.byref(cnt), idx.ctypes.data, audio.ctypes.data, info.ctypes.data, axc.ctypes.data)
                t1 = time.perf_counter()
                hips["enc"]._check(rc)
                rec.update(n_active=int(cnt.value), collect_encoded_s=t1 - t0)
            if F is not None:
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                rc = L.airband_hip_collect_rtp_packets(hips["rtp"].h, C.byref(cnt), records.ctypes.data, slots.ctypes.data, axc.ctypes.data)
                t1 = time.perf_counter()
                hips["rtp"]._check(rc)
                rec.update(n_packets=int(cnt.value), collect_rtp_s=t1 - t0)
                if a.compare:
                    k = min(rec["n_active"], rows)
                    t0 = time.perf_counter()
                    count, want_records, want_slots = model.step(idx[:k], audio[:k], ())
                    t1 = time.perf_counter()
                    rec.update(rows_kept=k, host_packetise_python_s=t1 - t0)
                    assert count == rec["n_packets"], "batch %d: %d packets, the reference has %d" % (b, rec["n_packets"], count)
                    m = min(count, a.check_packets)
                    assert records[:m].tobytes() == want_records[:m].tobytes(), "batch %d: records differ from the definition" % b
                    for i in range(m):
                        ln = int(want_records[i]["length"])
                        assert slots[i, :ln].tobytes() == want_slots[i, :ln].tobytes(), "batch %d: packet %d differs from the definition" % (b, i)
            print("RTP_PROFILE " + json.dumps(rec), flush=True)
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
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--max-rows-frac", type=float, default=0.25, help="capacity of the packed buffers as a fraction of the channels")
    ap.add_argument("--rtp", default="160", help="frame_samples of the stream, or none: a handle with gate and encoding only")
    ap.add_argument("--compare", action="store_true", help="child: a second handle without a stream, the host method timed and the packets compared")
    ap.add_argument("--check-packets", type=int, default=4096, help="packets per batch compared byte for byte with the definition")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_rtp_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child", "--compare",
               "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch), "--max-rows-frac", str(a.max_rows_frac), "--rtp", a.rtp,
               "--check-packets", str(a.check_packets)]
        lines = []
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("RTP_PROFILE"):
                    print(line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return p.returncode
        recs = [json.loads(line[len("RTP_PROFILE "):]) for line in lines if line.startswith("RTP_PROFILE ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    for rec in recs:
        b = rec["batch"]
        packs = kt.get(PACK, [])[2 * b:2 * b + 2]  # two handles, each with a pack launch per batch
        rec["pack_ms"] = sum(packs) / len(packs) if packs else None
        for k in KERNELS[1:]:
            rec[k.replace("_kernel", "_ms")] = kt[k][b] if len(kt.get(k, [])) > b else None
        rec["host_method_python_s"] = rec.get("collect_encoded_s", 0.0) + rec.get("host_packetise_python_s", 0.0)
        print("batch %(batch)d: n_active %(n_active)d packets %(n_packets)d | pack %(pack_ms).4f ms, rtp count %(rtp_count_ms).4f scan %(rtp_scan_ms).4f write "
              "%(rtp_write_ms).4f ms | collect_rtp_packets %(collect_rtp_s).4f s, host method (collect_active_encoded %(collect_encoded_s).4f s + Python "
              "packetisation %(host_packetise_python_s).4f s)" % rec)
    summary = dict(dongles=a.dongles, channels=a.dongles * 8, max_rows=max(1, int(a.dongles * 8 * a.max_rows_frac)), wave_batch=2000, encoding="ulaw", frame_samples=a.rtp,
                   note="host_packetise_python_s is capi.rtp_stream_reference in plain Python: it overstates a C host loop by far", batches=recs)
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
