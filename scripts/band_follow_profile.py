"""What the band follow (airband_hip_prepare_follow / airband_hip_set_band_follow, csrc/band_follow.hip) costs, at the shape scripts/band_watch_profile.py measures
the watch at: a synthetic fleet of N u8 dongles x 8 mixed channels at fft 512 (set_signal_plan, generate_iq, process_device on the handle's own stream), the scope,
survey and watch with that script's settings, and two followers per dongle (its AM channels 4 and 6).
Per batch:
    * GPU time of the follow's two kernels and of the re-tune kernel behind them, beside the watch's two kernels, on a quiet band (no change) and on a band that
      changes every batch (the input alternates between the fleet's signal and silence, confirm 1 / release 1: every dongle has a TUNE or a HOME in every batch):
      the kernels' own times from a `rocprofv3 --kernel-trace` run of this script's child;
    * wall time per step of the fleet with followers and of the same fleet without them (a handle without followers does exactly the work the watch-only handle
      did before the follow existed: it runs ahead), runs interleaved: the price of giving up run-ahead;
    * host wall time of collect_band_follow_changes() against collect_band_followers().
Every measurement is a child process of its own.  Writes profiles/band_follow.json.

    python scripts/band_follow_profile.py --dongles 65536
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

from band_watch_profile import CONFIRM, DB, GUARD, MATCH, MAX_PEAKS, PERMILLE, RELEASE, TRACKS, WINDOWS, kernel_ms, summary  # noqa: E402

KERNELS = ("band_watch_kernel", "band_watch_pack_kernel", "band_follow_kernel", "band_follow_pack_kernel", "retune_kernel")


def child(a):
    import torch

    pkg = importlib.import_module("rtlsdr-airband_amd")
    chans, carriers = pkg.siggen.baseline_plan(mixed=True)
    n = a.dongles
    follow = [8 * d + j for d in range(n) for j in (4, 6)] if a.follow else None
    with pkg.AirbandHip([dict(channels=chans)] * n, wave_rate=16000, follow=follow) as hip:
        hip.set_band_scope(windows=WINDOWS, mean=True, peak=True)
        hip.set_band_survey(trace="mean", max_peaks=MAX_PEAKS, floor_permille=PERMILLE, threshold_db=DB, guard_bins=GUARD)
        hip.set_band_watch(max_tracks=TRACKS, match_bins=MATCH, confirm_hits=1 if a.busy else CONFIRM, release_misses=1 if a.busy else RELEASE)
        if follow:
            hip.set_band_follow()
        hip.set_signal_plan(carriers)
        g = hip.geometry
        stride = (g.first_batch_bytes + g.lookahead_bytes + 255) // 256 * 256
        buf = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
        hip.generate_iq(buf.data_ptr(), stride, 4 * g.batch_bytes, g.first_batch_bytes + g.lookahead_bytes)
        quiet = torch.full((n, stride), 128, dtype=torch.uint8, device="cuda") if a.busy else None
        hip.process_device(buf.data_ptr(), stride)  # the first batch, with its lead-in
        hip.synchronize()
        off = g.first_batch_bytes - g.batch_bytes  # later batches re-read the span's last WAVE_BATCH hops: the same work every step

        def step(i):
            hip.process_device((quiet if a.busy and i % 2 == 0 else buf).data_ptr() + off, stride)

        for i in range(a.warmup):
            step(i)
        hip.synchronize()
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(i)
        hip.synchronize()
        out = dict(dongles=n, followers=len(follow or []), ms_per_step=(time.perf_counter() - t0) * 1e3 / max(a.steps, 1), schedule=hip.schedule_info(),
                   channelizer=hip.channelizer_name())
        if follow and a.collects > 0:
            t_changes, t_followers, counts = [], [], []
            for i in range(a.collects):
                step(i)
                hip.synchronize()
                t0 = time.perf_counter()
                ch = hip.collect_band_follow_changes()
                t_changes.append((time.perf_counter() - t0) * 1e3)
                counts.append(ch["n_changes"])
                t0 = time.perf_counter()
                got = hip.collect_band_followers()
                t_followers.append((time.perf_counter() - t0) * 1e3)
            out.update(max_changes=hip.follow_changes, collect_changes_ms=t_changes, n_changes=counts, collect_followers_ms=t_followers,
                       collect_followers_bytes=int(got["followers"].nbytes + got["rows"].nbytes), following_mean=float(got["rows"]["n_following"].mean()),
                       unserved_mean=float(got["rows"]["n_unserved"].mean()))
        print("FOLLOW_PROFILE " + json.dumps(out), flush=True)
        del buf


def run_child(a, collects, follow=True, busy=False, rocprof_dir=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dongles", str(a.dongles), "--steps", str(a.steps), "--warmup", str(a.warmup), "--collects", str(collects)]
    cmd += ["--busy"] if busy else []
    cmd += [] if follow else ["--no-follow"]
    if rocprof_dir:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", rocprof_dir, "--"] + cmd
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise RuntimeError("child failed: %d" % r.returncode)
    return [json.loads(line[len("FOLLOW_PROFILE "):]) for line in r.stdout.split("\n") if line.startswith("FOLLOW_PROFILE ")][0]


def traced(a, busy):
    """Median GPU time of each kernel of KERNELS over one traced child's batches (the first launches run beside the lead-in's longer stage 1: left out)."""
    d = tempfile.mkdtemp(prefix="airband_follow_")
    try:
        run_child(a, 0, busy=busy, rocprof_dir=d)
        return {k: statistics.median(kernel_ms(d, k)[1:] or [0.0]) for k in KERNELS}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--collects", type=int, default=6)
    ap.add_argument("--child-timeout", type=float, default=400.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_follow.json"))
    ap.add_argument("--child", action="store_true", help="run the workload itself")
    ap.add_argument("--busy", action="store_true", help="child: a band that changes every batch")
    ap.add_argument("--no-follow", dest="follow", action="store_false", help="child: the same fleet without followers (the watch only)")
    a = ap.parse_args()
    if a.child:
        return child(a)
    kernels = dict(quiet=traced(a, False), busy=traced(a, True))
    with_f, without, steady, busy = [], [], None, None
    for _ in range(a.runs):  # interleaved: both arrangements see the same box in the same minutes
        steady = run_child(a, a.collects)
        with_f.append(steady["ms_per_step"])
        without.append(run_child(a, 0, follow=False)["ms_per_step"])
    busy = run_child(a, a.collects, busy=True)
    for k in kernels.values():
        k["follow_apply_retune_ms"] = k["band_follow_kernel"] + k["band_follow_pack_kernel"] + k["retune_kernel"]
        k["watch_ms"] = k["band_watch_kernel"] + k["band_watch_pack_kernel"]
    out = dict(dongles=a.dongles, fft_size=512, sample_format="u8", followers_per_dongle=2, max_tracks=TRACKS, channelizer=steady["channelizer"], kernel_ms=kernels,
               ms_per_step=dict(with_followers=summary(with_f), watch_only=summary(without), schedule_with_followers=steady["schedule"],
                                note="watch_only: the same library, the same fleet prepared without followers -- the work and schedule of the watch-only handle before the follow existed"),
               steady=dict(max_changes=steady["max_changes"], n_changes=steady["n_changes"], collect_changes_ms=summary(steady["collect_changes_ms"]),
                           collect_followers_ms=summary(steady["collect_followers_ms"]), collect_followers_bytes=steady["collect_followers_bytes"],
                           following_mean=steady["following_mean"], unserved_mean=steady["unserved_mean"]),
               busy=dict(confirm_hits=1, release_misses=1, n_changes=busy["n_changes"], collect_changes_ms=summary(busy["collect_changes_ms"]),
                         collect_followers_ms=summary(busy["collect_followers_ms"]), ms_per_step=busy["ms_per_step"]))
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
