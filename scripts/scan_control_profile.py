"""What scan control (airband_hip_set_scan_control, csrc/scan_control.hip) costs and what it saves: a fleet of N scan dongles of 4 entries each (u8, fft 512,
WAVE_RATE 8000; one channel per dongle, so every dongle takes a 64-slot block of stage 2), fed on the device (set_signal_plan, generate_iq, process_device on the
handle's own stream).  N is the largest power of two up to --max-dongles whose handle prepares: the script tries downwards.  It halves the fleet ONLY where the
child says in so many words that the library (AIRBAND_HIP_ENOMEM) or the input buffer's allocation refused the size -- exit status 3 and a SCAN_PROFILE_REFUSED
line; a child that ends in any other way ends the script.
Two bands, both with receiver noise: QUIET (no transmitter: once saturated every list hops every batch) and HALF (an unkeyed AM transmitter on the channel of every
even dongle, switched on after the squelches have learnt the noise: those lists stay where they are, the odd ones hop).  The script checks what the band did --
at least 95 % of the lists hop per batch on the quiet band, 45 - 55 % on the half band -- and fails otherwise: a band that does not do what its name says is not
written down.
Per batch, idle_batches = 2 and dwell_batches = 1:
    * GPU: the kernels' own times -- scan_control_kernel, scan_control_pack_kernel, scan_exchange_kernel -- from a `rocprofv3 --kernel-trace` run of a child, and
      the host wall time of collect_scan_events();
    * HOST, the method scan control replaces, on the same box in runs that take turns with the GPU's: airband_hip_collect() of the axcindicate bytes, the
      controller's counters (vectorised numpy), one airband_hip_set_freq_index() call per hopping dongle (through ctypes: a C host pays much less per call), and
      the process call with scan_before_demod()'s staging, copy and event wait inside.  --parent-lib runs these children on another build of the library; the
      file says which library every host figure came from.
Every measurement is a child process of its own.  Writes profiles/scan_control.json.

    python scripts/scan_control_profile.py --max-dongles 262144
"""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from band_watch_profile import kernel_ms, summary  # noqa: E402

KERNELS = ("scan_control_kernel", "scan_control_pack_kernel", "scan_exchange_kernel")
IDLE, DWELL, ENTRIES = 2, 1, 4
REFUSED = 3  # the child's exit status for "this fleet does not fit", and nothing else
SHARE = dict(quiet=(0.95, 1.0), half=(0.45, 0.55))  # of the lists, how many hop per batch


def refuse(what):
    print("SCAN_PROFILE_REFUSED " + what, flush=True)
    return REFUSED


def child(a):
    import numpy as np
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    sg = pkg.siggen
    sample_rate, n_fft = 2_560_000, 512
    chans, _ = sg.baseline_plan(mixed=False)
    c0 = dict(chans[0])
    entries = [c0, dict(c0, squelch_snr_threshold_db=12.0, ampfactor=0.7), dict(c0, notch_freq=1000.0, ampfactor=1.8), dict(c0, squelch_snr_threshold_db=6.0)]
    b = int(pkg.derive_constants([dict(channels=[c0])], 0, wave_rate=8000)[0])
    off_hz = (b if b < n_fft // 2 else b - n_fft) * sample_rate / n_fft
    silent = sg.make_carrier(off_hz, sample_rate, amplitude=0.0, key_period_s=0.0)  # receiver noise only
    steady = sg.make_carrier(off_hz, sample_rate, key_period_s=0.0)                # never unkeyed
    n = a.dongles
    t0 = time.perf_counter()
    try:
        hip = pkg.AirbandHip([dict(channels=[c0])] * n, wave_rate=8000, scan={d: entries for d in range(n)})
    except pkg.AirbandError as e:
        if e.code == pkg.capi.ENOMEM:
            return refuse("prepare: %s" % e)
        raise
    with hip:
        prepare_s = time.perf_counter() - t0
        gpu = a.mode == "gpu"
        if gpu:
            hip.set_scan_control(IDLE, DWELL)
        g = hip.geometry
        span = g.first_batch_bytes + g.lookahead_bytes
        stride = (span + 255) // 256 * 256
        try:
            buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        except torch.cuda.OutOfMemoryError as e:
            return refuse("input buffer of %d bytes: %s" % (n * stride, str(e)[:200]))
        hip.set_signal_plan([silent])
        hip.generate_iq(buf.data_ptr(), stride, 4 * g.batch_bytes, span)
        hip.synchronize()
        noise_row = buf[1].clone()
        hip.process_device(buf.data_ptr(), stride)
        hip.synchronize()
        off = g.first_batch_bytes - g.batch_bytes  # later batches re-read the span's last WAVE_BATCH hops: the same work every step
        axc = np.empty(n, np.uint8)
        idx, idle = np.zeros(n, np.int64), np.zeros(n, np.int64)
        t = dict(process=[], collect=[], decide=[], set_index=[], events=[])
        counts = []

        def step(timed):
            t0 = time.perf_counter()
            hip.process_device(buf.data_ptr() + off, stride)
            t1 = time.perf_counter()
            hip.synchronize()
            if gpu:
                t2 = time.perf_counter()
                ev = hip.collect_scan_events()
                t3 = time.perf_counter()
                if timed:
                    t["process"].append((t1 - t0) * 1e3)
                    t["events"].append((t3 - t2) * 1e3)
                    counts.append(int((ev["records"]["kind"] == pkg.capi.SCAN_HOP).sum()))
                return
            t2 = time.perf_counter()
            hip._check(hip.L.airband_hip_collect(hip.h, None, None, axc.ctypes.data, None))
            t3 = time.perf_counter()
            quiet = axc == 0x20  # the controller thread's counters for the fleet at once (dwell 1)
            hop = quiet & (idle >= IDLE)
            idle[:] = np.where(quiet, np.minimum(idle + 1, IDLE), 0)
            idx[hop] = (idx[hop] + 1) % ENTRIES
            who = np.flatnonzero(hop)
            t4 = time.perf_counter()
            f = hip.L.airband_hip_set_freq_index
            for d, e in zip(who.tolist(), idx[who].tolist()):
                f(hip.h, d, e)
            t5 = time.perf_counter()
            if timed:
                t["process"].append((t1 - t0) * 1e3)
                t["collect"].append((t3 - t2) * 1e3)
                t["decide"].append((t4 - t3) * 1e3)
                t["set_index"].append((t5 - t4) * 1e3)
                counts.append(int(who.size))

        for _ in range(a.warmup):  # noise for everybody: the squelches learn their floor, the lists saturate and hop
            step(False)
        if a.band == "half":
            hip.set_signal_plan([steady])
            hip.generate_iq(buf.data_ptr(), stride, 4 * g.batch_bytes, span)
            hip.synchronize()
            buf[1::2] = noise_row  # every odd dongle goes on hearing noise
            torch.cuda.synchronize()
            for _ in range(a.warmup):  # the even dongles' squelches open
                step(False)
        for _ in range(a.steps):
            step(True)
        lo, hi = SHARE[a.band]
        if not all(lo * n <= c <= hi * n for c in counts):
            raise RuntimeError("the %s band did not do what it says: %r of %d lists hopped per batch" % (a.band, counts, n))
        out = dict(dongles=n, mode=a.mode, band=a.band, prepare_s=prepare_s, hops_per_batch=counts, library=os.path.basename(pkg.LIB_PATH),
                   ms={k: statistics.median(v) for k, v in t.items() if v})
        print("SCAN_PROFILE " + json.dumps(out), flush=True)
        del buf
    return 0


def run_child(a, n, mode, band, rocprof_dir=None, lib=None):
    """One child.  Returns its result, or dict(refused=...) where it said the fleet does not fit; anything else it ends with ends the script."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dongles", str(n), "--steps", str(a.steps), "--warmup", str(a.warmup), "--mode", mode, "--band", band]
    if rocprof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", rocprof_dir, "--"] + cmd
    env = dict(os.environ, AIRBAND_HIP_LIB=lib) if lib else None
    print("child: %d dongles, %s method, %s band%s" % (n, mode, band, ", traced" if rocprof_dir else ""), file=sys.stderr, flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout, env=env)
    said = [line for line in r.stdout.split("\n") if line.startswith("SCAN_PROFILE_REFUSED ")]
    if r.returncode == REFUSED and said:
        return dict(refused=said[0][len("SCAN_PROFILE_REFUSED "):][:300])
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise RuntimeError("child ended with status %d (%d dongles, %s, %s): nothing more is started" % (r.returncode, n, mode, band))
    return [json.loads(line[len("SCAN_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("SCAN_PROFILE ")][0]


def traced(a, n, band):
    d = tempfile.mkdtemp(prefix="airband_scan_")
    try:
        if "refused" in run_child(a, n, "gpu", band, rocprof_dir=d):
            raise RuntimeError("the traced child did not fit where the plain one did")
        # the launches of the timed steps are the last a.steps of each kernel
        return {k: statistics.median(kernel_ms(d, k)[-a.steps:] or [0.0]) for k in KERNELS}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-dongles", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--parent-lib", default=None, help="the host method's children load this build of the library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_control.json"))
    ap.add_argument("--child", action="store_true", help="run the workload itself")
    ap.add_argument("--dongles", type=int, default=0, help="child: the fleet")
    ap.add_argument("--mode", choices=("gpu", "host"), default="gpu")
    ap.add_argument("--band", choices=("quiet", "half"), default="quiet")
    a = ap.parse_args()
    if a.child:
        return child(a)
    n, tried, first = a.max_dongles, [], None
    while n >= 64:  # the largest power-of-two fleet that prepares
        first = run_child(a, n, "gpu", "quiet")
        tried.append(dict(dongles=n, ok="refused" not in first, note=first.get("refused", "")))
        if "refused" not in first:
            break
        n //= 2
    if first is None or "refused" in first:
        raise RuntimeError("no fleet prepared: %r" % tried)
    out = dict(dongles=n, entries=ENTRIES, fft_size=512, sample_format="u8", idle_batches=IDLE, dwell_batches=DWELL, tried=tried, prepare_s=first["prepare_s"], bands={})
    for band in ("quiet", "half"):
        kernels = traced(a, n, band)
        gpu, host = [], []
        for _ in range(a.runs):  # interleaved: both methods see the same box in the same minutes
            gpu.append(run_child(a, n, "gpu", band))
            host.append(run_child(a, n, "host", band, lib=a.parent_lib))
        if any("refused" in r for r in gpu + host):
            raise RuntimeError("a child did not fit where the first one did")
        out["bands"][band] = dict(
            kernel_ms=dict(kernels, total=sum(kernels.values())),
            gpu=dict(hops_per_batch=gpu[-1]["hops_per_batch"], library=gpu[-1]["library"], collect_scan_events_ms=summary([r["ms"]["events"] for r in gpu]),
                     process_call_ms=summary([r["ms"]["process"] for r in gpu])),
            host=dict(hops_per_batch=host[-1]["hops_per_batch"], library=host[-1]["library"], collect_axc_ms=summary([r["ms"]["collect"] for r in host]),
                      counters_ms=summary([r["ms"]["decide"] for r in host]), set_freq_index_ms=summary([r["ms"]["set_index"] for r in host]),
                      process_call_ms=summary([r["ms"]["process"] for r in host]),
                      total_ms=summary([r["ms"]["collect"] + r["ms"]["decide"] + r["ms"]["set_index"] + r["ms"]["process"] for r in host])))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
