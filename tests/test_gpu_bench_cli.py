"""-m gpu: bench.py's command line -- a plain run prints the headline line only and honours --steps / --warmup,
--dump-outputs writes the last timed step's ordered match records (float64 .npy, identical from run to run), and the
side measurements appear only with --full (tests/test_gpu_multirank.py runs a --full line through the N>1 path)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 0.125   # 128 MiB: two planted occurrences per 4 MiB, a handful of random ones


def run_bench(outdir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--gib", str(GIB),
           "--dump-outputs", str(outdir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f: np.load(os.path.join(outdir, f + ".npy")) for f in ("pattern", "start", "end", "n_matches")}


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return run_bench(tmp_path_factory.mktemp("dump_a"))


def test_plain_line_is_the_headline_only(plain):
    d, _ = plain
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["unit"] == "GB/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    shard = int(GIB * (1 << 30))
    assert d["ms_per_step"] > 0 and abs(d["value"] - shard / (d["ms_per_step"] * 1e-3) / 1e9) / d["value"] < 0.01
    assert d["cpu_baseline"] is None and d["roofline"]["empirical_peak"] is None
    assert not {"engines", "also", "costs"} & set(d)


def test_dump_holds_the_ordered_records(plain):
    d, a = plain
    n = d["config"]["matches"]
    assert n >= 64   # the planted occurrences alone
    assert int(a["n_matches"][0]) == n
    for f in ("pattern", "start", "end"):
        assert a[f].dtype == np.float64 and a[f].shape == (n,)
    assert np.all(np.diff(a["end"]) >= 0)                       # the reference's order: by end
    length = a["end"] - a["start"]
    assert length.min() >= 4 and length.max() <= 16              # the workload's pattern lengths
    assert a["pattern"].min() >= 0 and a["pattern"].max() < d["config"]["patterns"]
    assert a["end"].max() <= GIB * (1 << 30)
    assert sum(a[f].nbytes for f in a) <= 64 << 20


def test_dump_is_identical_from_run_to_run(plain, tmp_path):
    _, a = plain
    _, b = run_bench(tmp_path)
    for f in a:
        assert np.array_equal(a[f], b[f]), f
