"""bench.py itself: a plain run times the steps it is asked for and nothing else; --dump-outputs writes the last step's
archive as float arrays, the same for the same arguments."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def test_dump_outputs_is_seeded_and_bounded(tmp_path):
    """An archive longer than DUMP_SAMPLE is sampled at the same positions every time; a short one is written whole."""
    import bench
    rng = np.random.default_rng(3)
    big = [rng.integers(0, 256, bench.DUMP_SAMPLE + 12345, dtype=np.uint8).tobytes(), b"\x07" * 1000]
    st = {"nodes": 8, "symbols": 9, "rounds": 10, "sort_rounds": 11, "flushes": 12}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, st)
    sizes = 0
    for name in ("archive_lengths", "archive_sample", "counts"):
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("a", "b"))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
        sizes += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert sizes <= 64 << 20
    sample = np.load(tmp_path / "a" / "archive_sample.npy")
    assert len(sample) == bench.DUMP_SAMPLE and sample.min() >= 0 and sample.max() <= 255
    assert np.load(tmp_path / "a" / "archive_lengths.npy").tolist() == [bench.DUMP_SAMPLE + 12345, 1000]
    assert np.load(tmp_path / "a" / "counts.npy").tolist() == [8, 9, 10, 11, 12]
    bench.dump_outputs(str(tmp_path / "c"), [b"abc", b"de"], st)
    assert np.load(tmp_path / "c" / "archive_sample.npy").tolist() == list(b"abcde")


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_archive(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` at a small size: the line has the headline fields and none
    of --full's legs, K steps were timed, and DIR holds the oracle's archive of the input."""
    import oracle
    n = 3_000_000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", str(n),
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["metric"] == "MB/s compressed" and j["unit"] == "MB/s" and j["higher_is_better"] is True and j["dtype"] == "u8/u32 integer"
    assert j["steps"] == 3 and j["warmup"] == 1 and j["ms_per_step"] > 0
    assert abs(j["value"] - n / (j["ms_per_step"] * 1e-3) / 1e6) < 0.02 * j["value"]
    for leg in ("cli", "value_end_to_end", "value_stream", "decode", "workloads", "oracle_golden"):
        assert leg not in j, leg
    assert j["cpu_baseline"] is None
    ref = oracle.compress(oracle.synth_text(1, n))
    assert j["archive_sha256"] == hashlib.sha256(ref).hexdigest()
    d = tmp_path / "out"
    assert np.load(d / "archive_lengths.npy").tolist() == [len(ref)]
    sample = np.load(d / "archive_sample.npy")
    assert sample.dtype == np.float32 and bytes(sample.astype(np.uint8)) == ref
    assert np.load(d / "counts.npy")[0] == 8 * n - 8
