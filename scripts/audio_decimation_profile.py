"""What the output decimation (airband_hip_set_output_decimation, csrc/audio_decimate.hip) costs and saves: a synthetic fleet of N dongles x 8 channels of the
BASELINE plan at WAVE_RATE 16000 (set_signal_plan, generate_iq, process_device), gate SIGNAL on every channel, as in scripts/audio_encoding_profile.py.  One
process holds, per format (mu-law and S16), a handle with the encoding alone and a handle with the encoding and the decimation, all fed the same input, so that
every batch lists the same rows in each.  Per batch: n_active, the GPU time of audio_decimate_<format>_kernel beside audio_pack_<format>_kernel ON THE SAME ROWS
(from a `rocprofv3 --kernel-trace --stats` run of this script's own child; audio_pack.hip is the file the decimation's parent commit shipped, unchanged: it reads
the same bytes and writes twice as many -- `encode_*_ms` is THIS library's audio_pack kernel; with --parent-lib a second child runs the full-rate handles alone on a
library built from the parent commit and its audio_pack times are recorded beside them as `parent_encode_*_ms`), and the wall time of airband_hip_collect_active_encoded() with and without decimation, the calls taking turns in who
goes first, all into host arrays that were allocated and touched before the first batch.

    python scripts/audio_decimation_profile.py --dongles 65536 --batches 6 --out profiles/audio_decimation.json
    python scripts/audio_decimation_profile.py --parent-lib /path/to/parent/libairband_hip.so ...   # also the parent build's own audio_pack kernel
    python scripts/audio_decimation_profile.py --child --dongles 4      # the workload alone
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

FORMATS = ("ulaw", "s16")
KERNELS = {(f, d): ("audio_decimate_%s_kernel" if d else "audio_pack_%s_kernel") % f for f in FORMATS for d in (False, True)}


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    capi = pkg.capi
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n, n_ch = a.dongles, a.dongles * 8
    rows = max(1, min(n_ch, a.max_rows if a.max_rows > 0 else n_ch // 4))
    kinds = [(f, d) for f in FORMATS for d in ((False,) if a.no_decimation else (False, True))]
    hips = []
    try:
        for f, d in kinds:
            hip = pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000)
            hips.append(hip)
            hip.set_output_gate(np.full(n_ch, capi.GATE_SIGNAL, np.uint8), rows)
            hip.set_output_encoding(f)
            if d:
                hip.set_output_decimation(2)
            hip.set_signal_plan(carriers)
            print("DECIMATION_PROFILE_HANDLE %s%s: %d channels, %d rows of %d" % (f, " / 2" if d else "", n_ch, rows, hip._encoded_row()), flush=True)
        g, B, L = hips[0].geometry, hips[0].B, hips[0].L
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        # host arrays: allocated and touched once, so that no batch pays for page faults
        out = {k: np.full((rows, B // 2 if k[1] else B), 1, np.dtype("<i2") if k[0] == "s16" else np.uint8) for k in kinds}
        info = {k: np.full(rows * 4, 0xFFFFFFFF, np.uint32).view(capi.AUDIO_ROW_DTYPE) for k in kinds}
        idx = {k: np.full(rows, -1, np.int32) for k in kinds}
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
            order = list(range(len(kinds)))
            order = order[b % len(order):] + order[:b % len(order)]  # who goes first takes turns
            for i in order:
                k, hip = kinds[i], hips[i]
                cnt = C.c_int64(0)
                t0 = time.perf_counter()
                rc = L.airband_hip_collect_active_encoded(hip.h, C.byref(cnt), idx[k].ctypes.data, out[k].ctypes.data, info[k].ctypes.data, axc.ctypes.data)
                t1 = time.perf_counter()
                hip._check(rc)
                rec["collect_%s%s_s" % (k[0], "_half" if k[1] else "")] = t1 - t0
                rec.setdefault("n_active", int(cnt.value))
                assert rec["n_active"] == int(cnt.value), "batch %d: the handles disagree about the count" % b
            kept = min(rec["n_active"], rows)
            rec["rows_kept"] = kept
            for k in kinds[1:]:
                assert np.array_equal(idx[k][:kept], idx[kinds[0]][:kept]), "batch %d: the handles disagree about the list" % b
            if b == 0 and kept and not a.no_decimation:  # every history is zero: (a sample of) the decimated rows are the definition's, of the q values the S16 encoder delivered
                m = min(kept, 64)
                x = (out[("s16", False)][:m].astype(np.float64) / 32767.0).astype(np.float32)
                for f in FORMATS:
                    assert out[(f, True)][:m].tobytes() == capi.audio_decimate_reference(x, f)[0].tobytes(), "batch 0: %s rows differ from the definition" % f
            print("DECIMATION_PROFILE " + json.dumps(rec), flush=True)
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
        for k in KERNELS.values():
            if k in name:
                out.setdefault(k, []).append(ms)
    return out


def traced_child(a, extra, lib):
    """the child under rocprofv3 (lib: AIRBAND_HIP_LIB for it, or None): (its records, kernel_times()), or (None, its exit status) where it failed"""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    out_dir = tempfile.mkdtemp(prefix="airband_decimate_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__), "--child",
               "--dongles", str(a.dongles), "--batches", str(a.batches), "--start-batch", str(a.start_batch), "--max-rows", str(a.max_rows)] + extra
        lines = []
        env = dict(os.environ, AIRBAND_HIP_LIB=lib) if lib else None
        with subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) as p:
            for line in p.stdout:  # the child's progress as it happens: a fleet of this size takes minutes
                lines.append(line.rstrip("\n"))
                if line.startswith("DECIMATION_PROFILE"):
                    print(("parent lib: " if lib else "") + line.rstrip("\n"), flush=True)
        if p.returncode != 0:
            sys.stderr.write("\n".join(lines[-60:]) + "\n")
            return None, p.returncode or 1
        return [json.loads(line[len("DECIMATION_PROFILE "):]) for line in lines if line.startswith("DECIMATION_PROFILE ")], kernel_times(out_dir)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--start-batch", type=int, default=4)
    ap.add_argument("--max-rows", type=int, default=131072, help="capacity of the packed buffers (cut to the channel count; 0: a quarter of the channels)")
    ap.add_argument("--out", default=None, help="write the JSON summary here as well")
    ap.add_argument("--child", action="store_true", help="run the workload itself (what the parent starts under rocprofv3)")
    ap.add_argument("--no-decimation", action="store_true", help="child: the full-rate handles alone (what a library without the decimation can run)")
    ap.add_argument("--parent-lib", default=None, help="a libairband_hip.so built from the parent commit: its audio_pack kernel is timed on the same rows in a second child")
    a = ap.parse_args()
    if a.child:
        return child(a)
    recs, kt = traced_child(a, [], None)
    if recs is None:
        return kt
    parent_kt = None
    if a.parent_lib:
        parent_recs, parent_kt = traced_child(a, ["--no-decimation"], os.path.abspath(a.parent_lib))
        if parent_recs is None:
            return parent_kt
        assert [r["n_active"] for r in parent_recs] == [r["n_active"] for r in recs], "the parent's library lists other rows"
    for rec in recs:
        b = rec["batch"]
        if parent_kt is not None:
            for f in FORMATS:
                name = KERNELS[(f, False)]
                rec["parent_encode_%s_ms" % f] = parent_kt[name][b] if len(parent_kt.get(name, [])) > b else None
        for (f, d), name in KERNELS.items():
            rec["%s_%s_ms" % ("decimate" if d else "encode", f)] = kt[name][b] if len(kt.get(name, [])) > b else None
        for f in FORMATS:
            e, d = rec["encode_%s_ms" % f], rec["decimate_%s_ms" % f]
            rec["kernel_ratio_%s" % f] = d / e if e and d else None
        print("batch %(batch)d: n_active %(n_active)d kept %(rows_kept)d | ulaw: encode %(encode_ulaw_ms).4f decimate %(decimate_ulaw_ms).4f ms | s16: encode "
              "%(encode_s16_ms).4f decimate %(decimate_s16_ms).4f ms | collect ulaw %(collect_ulaw_s).4f half %(collect_ulaw_half_s).4f s16 %(collect_s16_s).4f half "
              "%(collect_s16_half_s).4f s" % rec)
    n_ch = a.dongles * 8
    summary = dict(dongles=a.dongles, channels=n_ch, max_rows=max(1, min(n_ch, a.max_rows if a.max_rows > 0 else n_ch // 4)), wave_batch=2000, wave_rate=16000,
                   encode_kernel="audio_pack_<format>_kernel of THIS library (audio_pack.hip is unchanged from the parent commit)" + ("; parent_encode_*: the same kernel of --parent-lib" if a.parent_lib else ""),
                   batches=recs)
    print(json.dumps(summary))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
