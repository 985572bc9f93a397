"""Workload for timing the scan-mode exchange kernel (csrc/misc_kernels.hip, scan_exchange_kernel): N one-channel scan dongles with four AM entries
each, every dongle switching to another entry at every batch, run through airband_hip_process_bins on constant bins.  Run it under a kernel trace,
e.g.  rocprofv3 --kernel-trace --stats -d OUT -- python scripts/scan_exchange_profile.py --dongles 65536
and read scan_exchange_kernel's duration per dispatch (one dispatch per batch = N switches)."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("rtlsdr-airband_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dongles", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=6)
    a = ap.parse_args()
    e0 = dict(frequency=120_100_000, modulation=0)
    entries = [e0, dict(e0, squelch_snr_threshold_db=12.0), dict(e0, ampfactor=0.5), dict(e0, squelch_snr_threshold_db=6.0)]
    devs = [dict(channels=[e0]) for _ in range(a.dongles)]
    with pkg.AirbandHip(devs, wave_rate=8000, scan={d: entries for d in range(a.dongles)}) as hip:
        w = np.ones((a.dongles, hip.B), np.float32)
        q = np.zeros((a.dongles, 2 * hip.B), np.float32)
        for b in range(a.batches):
            for d in range(a.dongles):
                hip.set_freq_index(d, (b + d) % len(entries))
            hip.process_bins(w, q)
            hip.collect()
        hip.synchronize()
    print("%d batches of %d switches" % (a.batches, a.dongles))


if __name__ == "__main__":
    main()
