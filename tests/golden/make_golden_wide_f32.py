#!/usr/bin/env python3
"""Generates tests/golden/cf32_8000k.npz from the REAL reference (oracle/_ref): one CF32 dongle at 8 MS/s in the WAVE_RATE 8000 build -- hops of 1 000 samples
= 8 000 bytes, of which the reference reads the window's 4 096 (src/rtl_airband.cpp:421-455, :669) -- a shape AIRBAND_HIP_FLAG_WIDE_HOPS puts on the float
matrix-core channelizer (csrc/channelizer_f32_wide.hip).  The stream is regenerated from its seed (helpers.format_case); the fixture holds the reference's outputs
and the stream's SHA-256."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import helpers  # noqa: E402

NAME = "cf32_8000k"
# three batches: every keyed transmitter of the plan (period 0.5 s, 0.3 s on) opens and closes inside 0.375 s
CASE = dict(sfmt="SFMT_F32", fft_log=9, sample_rate=8_000_000, wave_rate=8000, dongle=2, n_batches=3)


def build_case():
    pkg = importlib.import_module("rtlsdr-airband_amd")
    c = CASE
    devices, iq = helpers.format_case(pkg, getattr(pkg.capi, c["sfmt"]), c["fft_log"], c["sample_rate"], c["wave_rate"], 1, c["n_batches"], first_dongle=c["dongle"])
    return c, devices, iq[0]


def main():
    import pyref

    c, devices, iq = build_case()
    ref = pyref.run_reference(devices, [iq], c["n_batches"], nfm=False, fm_demod=0, fft_log=c["fft_log"])[0]
    assert ref["n_batches"] == c["n_batches"]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), NAME + ".npz")
    np.savez_compressed(path, waveout=ref["waveout"].astype(np.float32), axc=ref["axc"], iq_sha256=np.frombuffer(hashlib.sha256(iq.tobytes()).digest(), np.uint8),
                        stats=json.dumps(ref["stats"]), case=json.dumps(c), channels=json.dumps(devices[0]["channels"]))
    print(NAME, os.path.getsize(path) // 1024, "KiB; open batches per channel:", (ref["axc"] == ord("*")).sum(axis=0), "closed:", (ref["axc"] == ord(" ")).sum(axis=0))


if __name__ == "__main__":
    main()
