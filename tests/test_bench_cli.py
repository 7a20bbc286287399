"""bench.py's command line: --steps sets the timed steps, --dump-outputs writes the last
step's outputs reproducibly, and the 4K pass of the default run sits behind --full.  CPU
rehearsal (--cpu) only: the same step / dump code drives the GPU engines."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _run(extra, timeout=240):
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "1", "--batch", "2", "--gop", "4",
            "--threads", "1", *extra]
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, TV_NO_PIN="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(line) == 1, r.stdout
    return json.loads(line[0])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    """Two identical runs (3 timed steps, 1 warm-up) dumping into two directories."""
    out = []
    for name in ("a", "b"):
        d = tmp_path_factory.mktemp(name)
        out.append((_run(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]), d))
    return out


def test_steps_and_ms_per_step(dumps):
    rec, _ = dumps[0]
    c = rec["config"]
    assert rec["steps"] == 3 and rec["warmup"] == 1 and len(c["step_ms"]) == 3
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec
    assert rec["ms_per_step"] > 0
    frames_per_step = 2 * 4
    assert abs(rec["value"] * rec["ms_per_step"] / 1000 - frames_per_step) < 1e-3 * frames_per_step
    assert sum(c["step_ms"]) <= 3 * rec["ms_per_step"] * 1.001 + 0.03  # the steps lie inside the timed region
    assert "fps_4k" not in c


def test_dump_outputs_reproducible(dumps):
    (rec, a), (_, b) = dumps
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"bitstream.npy", "segment_bytes.npy", "segment_crc32.npy", "sse.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0
        assert np.array_equal(x, y), n
        total += os.path.getsize(a / n)
    assert total <= 64e6
    nbytes = np.load(a / "segment_bytes.npy")
    assert nbytes.shape == (2,) and np.load(a / "sse.npy").shape == (2, 3)
    assert np.load(a / "bitstream.npy").size == nbytes.sum()
    # the dump is the last step alone; the JSON counts the bytes of all 3 timed steps
    assert 0 < nbytes.sum() < rec["config"]["bytes_all_reduced_mb"] * 1e6


def test_dump_sample_is_fixed_and_bounded():
    a = np.arange(bench.DUMP_CAP + 12345, dtype=np.int64) % 251
    s1, s2 = bench._dump_sample(a, 1), bench._dump_sample(a.copy(), 1)
    assert s1.dtype == np.float32 and s1.shape == (bench.DUMP_CAP,) and np.array_equal(s1, s2)
    small = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert np.array_equal(bench._dump_sample(small, 1), small.astype(np.float32))
    assert 4 * 4 * bench.DUMP_CAP <= 64e6 - 1e6  # four sampled float32 arrays, 1 MB left for the per-segment ones


def test_4k_pass_only_with_full():
    base = dict(no_4k=False, cpu=False, res="1080p", kbps=0.0, bframes=bench._WORKER_BFRAMES, content="smooth")
    assert not bench._with_4k(argparse.Namespace(full=False, **base))
    assert bench._with_4k(argparse.Namespace(full=True, **base))
    assert not bench._with_4k(argparse.Namespace(full=True, **dict(base, no_4k=True)))
    assert not bench._with_4k(argparse.Namespace(full=True, **dict(base, res="4k")))


def test_full_and_job_dump_arguments():
    rec = _run(["--full", "--steps", "1", "--warmup", "0"])
    assert rec["steps"] == 1 and rec["warmup"] == 0
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--job", "--dump-outputs", "x"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
