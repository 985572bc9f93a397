"""What the encoded audio collect (airband_hip_set_output_encoding, csrc/audio_pack.hip) costs and saves: a synthetic fleet of N dongles x 8 channels of the
BASELINE plan (set_signal_plan, generate_iq, process_device), gate SIGNAL on every channel, as in scripts/gated_collect_profile.py.  One process holds one
handle per format -- float rows only, s16, ulaw, alaw -- fed the same input, so that every batch delivers the same rows in each.  Per batch: n_active, the GPU
time of each format's encode kernel beside gate_gather_kernel's (from a `rocprofv3 --kernel-trace --stats` run of this script's own child), and the wall time of
airband_hip_collect_active() beside airband_hip_collect_active_encoded() of each format, the calls taking turns in who goes first, all into host arrays that
were allocated and touched before the first batch.

    python scripts/audio_encoding_profile.py --dongles 65536 --batches 8 --out profiles/audio_encoding.json
    python scripts/audio_encoding_profile.py --child --dongles 4 --encoding ulaw     # the workload alone on ONE handle (tests/test_gpu_audio_encoding.py traces it)
    python scripts/audio_encoding_profile.py --child --dongles 4 --encoding none     # ... with a gate and no encoding
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

FORMATS = ("s16", "ulaw", "alaw")
GATHER = "gate_gather_kernel"
ENCODE = {f: "audio_pack_%s_kernel" % f for f in FORMATS}


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_ch = a.dongles, a.dongles * 8
    rows = max(1, int(n_ch * a.max_rows_frac))
    formats = ["none"] + list(FORMATS) if a.encoding == "all" else [a.encoding]
    hips = []
    try:
        for f in formats:
            hip = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hips.append(hip)
            hip.set_output_gate(np.full(n_ch, capi.GATE_SIGNAL, np.uint8), rows)
            if f != "none":
                hip.set_output_encoding(f)
            hip.set_signal_plan(carriers)
            print("AUDIO_PROFILE_HANDLE %s: %d channels, %d rows" % (f, n_ch, rows), flush=True)
        g, B, L = hips[0].geometry, hips[0].B, hips[0].L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults (np.zeros would hand out untouched pages)
        out = {f: np.full((rows, B), 1, np.float32 if f == "none" else np.dtype("<i2") if f == "s16" else np.uint8) for f in formats}
        info = {f: np.full(rows * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE) for f in formats if f != "none"}
        idx = {f: np.full(rows, -1, np.int32) for f in formats}
        axc = np.full(n_ch, 1, np.uint8)
        start = a.start_batch * g.batch_bytes  # signal time of the first batch: the transmitters key on and off over seconds
        for b in range(a.batches):
            nbytes = (g.first_batch_bytes if b == 0 else g.batch_bytes) + g.lookahead_bytes
            hips[0].generate_iq(buf.data_ptr(), stride, start, nbytes)
            hips[0].synchronize()
            torch.cuda.synchronize()
            start += g.first_batch_bytes if b == 0 else g.batch_bytes
            for hip in hips:  # one handle at a time: a kernel's duration is its own, not what it got beside another handle's stage 2
                hip.process_device(buf.data_ptr(), stride)
                hip.synchronize()
            rec = dict(batch=b)
            order = list(range(len(formats)))
            order = order[b % len(order):] + order[:b % len(order)]  # who goes first takes turns
            for i in order:
                f, hip = formats[i], hips[i]
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                if f == "none":
                    rc = L.airband_hip_collect_active(hip.h, C.byref(cnt), idx[f].ctypes.data, out[f].ctypes.data, None, axc.ctypes.data)
                else:
                    rc = L.airband_hip_collect_active_encoded(hip.h, C.byref(cnt), idx[f].ctypes.data, out[f].ctypes.data, info[f].ctypes.data, axc.ctypes.data)
                t1 = time.perf_counter()
                hip._check(rc)
                rec["collect_%s_s" % ("f32" if f == "none" else f)] = t1 - t0
                rec.setdefault("n_active", int(cnt.value))
                assert rec["n_active"] == int(cnt.value), "batch %d: the handles disagree about the count" % b
            k = min(rec["n_active"], rows)
            rec["rows_kept"] = k
            if "none" in formats:  # the same rows in every handle, and (a sample of) the encoded rows are the definition's
                for f in formats[1:]:
                    assert np.array_equal(idx[f][:k], idx["none"][:k]), "batch %d: the handles disagree about the list" % b
                    m = min(k, 64)
                    ref_audio, ref_info = capi.audio_encode_reference(out["none"][:m], f)
                    ref_info["channel"] = idx["none"][:m]
                    assert out[f][:m].tobytes() == ref_audio.tobytes() and info[f][:m].tobytes() == ref_info.tobytes(), "batch %d: %s rows differ from the definition" % (b, f)
            print("AUDIO_PROFILE " + json.dumps(rec), flush=True)
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
        for k in (GATHER,) + tuple(ENCODE.values()):
            if k in name:
                out.setdefault(k, []).append(ms)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--max-rows-frac", type=float, default=0.25, help="capacity of the packed buffers as a fraction of the channels")
    ap.add_argument("--encoding", default="all", choices=("all", "none") + FORMATS, help="child: one handle per format (all), or one handle with this format")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_audio_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch), "--max-rows-frac", str(a.max_rows_frac)]
        lines = []
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("AUDIO_PROFILE"):
                    print(line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return p.returncode
        recs = [json.loads(line[len("AUDIO_PROFILE "):]) for line in lines if line.startswith("AUDIO_PROFILE ")]
        kt = kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    H = 1 + len(FORMATS)  # handles, each with a gather per batch
    for rec in recs:
        b = rec["batch"]
        gathers = kt.get(GATHER, [])[b * H:(b + 1) * H]
        rec["gather_ms"] = sum(gathers) / len(gathers) if gathers else None
        for f in FORMATS:
            rec["encode_%s_ms" % f] = kt[ENCODE[f]][b] if len(kt.get(ENCODE[f], [])) > b else None
        print("batch %(batch)d: n_active %(n_active)d kept %(rows_kept)d | gather %(gather_ms).4f ms, encode s16 %(encode_s16_ms).4f ulaw %(encode_ulaw_ms).4f alaw "
              "%(encode_alaw_ms).4f ms | collect_active %(collect_f32_s).4f s, encoded s16 %(collect_s16_s).4f ulaw %(collect_ulaw_s).4f alaw %(collect_alaw_s).4f s" % rec)
    summary = dict(dongles=a.dongles, channels=a.dongles * 8, max_rows=max(1, int(a.dongles * 8 * a.max_rows_frac)), wave_batch=2000, batches=recs)
    text = json.dumps(summary)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
