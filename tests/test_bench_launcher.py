"""bench.py's own N-rank launch (no GPU needed): `python bench.py --gpus N` must form an N-rank job by itself -- the analogue
of the reference starting one demodulate() thread per device shard (src/rtl_airband.cpp:1110-1112) -- report that N, and
refuse to report anything for a different world size.  With a GPU: what a plain run reports and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def _json(stdout):
    lines = [ln for ln in stdout.strip().splitlines() if ln.startswith("{")]
    assert lines, stdout
    return json.loads(lines[-1])


def test_gpus_2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--dry-run", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = _json(r.stdout)
    assert out["n_gpus"] == 2 and out["max_rank_seen"] == 1 and out["dry_run"] is True
    assert len([ln for ln in r.stdout.splitlines() if ln.startswith("{")]) == 1, "only rank 0 prints"


def test_gpus_1_stays_single_process():
    r = _run(["--gpus", "1", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json(r.stdout)["n_gpus"] == 1


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "2", "--dry-run"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_uses_only_names_the_package_has():
    """bench.py reaches into the package and its multigpu module by attribute; a helper removed from either must not surface as an error string in a JSON field on the GPU box
    (round 5: `open_fraction` carried an AttributeError for one profile run after the dead torch all-reduce path had been deleted)."""
    import importlib
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    pkg = importlib.import_module("rtlsdr-airband_amd")
    mg = importlib.import_module("rtlsdr-airband_amd.multigpu")
    for name in set(re.findall(r"\bmg\.([A-Za-z_]\w*)", src)):
        assert hasattr(mg, name), "bench.py uses multigpu.%s" % name
    for name in set(re.findall(r"\bpkg\.([A-Za-z_]\w*)", src)):
        assert hasattr(pkg, name), "bench.py uses <package>.%s" % name
    for name in set(re.findall(r"\bhip\.([a-z_]\w*)\(", src)):
        assert hasattr(pkg.AirbandHip, name), "bench.py calls AirbandHip.%s" % name


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(built, tmp_path):
    """A plain run (no --full) times exactly --steps steps and does nothing else; --dump-outputs writes the last step's sampled results as float32 /
    float64 .npy files of at most 64 MB, and two runs with the same arguments write the same arrays."""
    import numpy as np

    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        r = _run(["--gpus", "1", "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs", d], timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = _json(r.stdout)
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"]
        assert not {"verify", "verify_all", "open_fraction", "throughput_mode", "host_path"} & set(out), sorted(out)
        assert out["cpu_baseline"] is None and out["roofline"]["traffic"] is None
        arrays = {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(os.path.getsize(os.path.join(d, f)) for f in arrays) <= 64 << 20
        dumps.append(arrays)
    a, b = dumps
    assert {"dongles.npy", "waveout.npy", "axcindicate.npy", "channel_stats.npy"} <= set(a) and set(a) == set(b)
    assert np.array_equal(a["dongles.npy"], np.arange(64)), "the tiny workload's 64 dongles all fit the sample"
    assert a["waveout.npy"].shape[0] == a["axcindicate.npy"].shape[0] == a["channel_stats.npy"].shape[0] == 64 * 8
    assert np.abs(a["waveout.npy"]).max() > 0
    for f in a:
        assert np.array_equal(a[f], b[f], equal_nan=True), f


def test_host_path_needs_full():
    r = _run(["--gpus", "1", "--host-path"])
    assert r.returncode != 0 and "--full" in r.stderr
