"""bench.py end to end on the GPU, as a child process on a small corpus: a
plain run is lean (no CPU baseline leg) and says how long a step took, and
--dump-outputs writes the probe step's matrices, finite, trained, and the same
in two runs of the same arguments."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--tokens", "400000", "--vocab", "30000", "--dim", "100",
        "--table-size", "1000000"]
STAT_WORDS, STAT_CENTERS, STAT_SENTENCES, STAT_NONFINITE = 0, 1, 5, 6


def test_plain_run_is_lean_and_dump_is_reproducible(tmp_path):
    runs = [subprocess.Popen([sys.executable, str(ROOT / "bench.py"), *ARGS, "--dump-outputs", str(tmp_path / n)],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=tmp_path)
            for n in ("a", "b")]
    outs = [p.communicate(timeout=120) for p in runs]
    for p, (so, se) in zip(runs, outs):
        assert p.returncode == 0, se[-3000:]
    line = json.loads(outs[0][0].strip().splitlines()[-1])
    assert line["cpu_baseline"] is None  # the CPU baseline leg is --full's
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "words/s" and line["higher_is_better"] is True and line["dtype"] == "fp32"
    words = line["config"]["in_vocab_tokens_per_gpu_per_step"]
    assert line["value"] == pytest.approx(words / (line["ms_per_step"] / 1e3), rel=1e-3)

    a = {p.name: np.load(p) for p in sorted((tmp_path / "a").iterdir())}
    b = {p.name: np.load(p) for p in sorted((tmp_path / "b").iterdir())}
    assert sorted(a) == sorted(b) == ["C.npy", "W.npy", "policy.npy", "probe_stats.npy", "rows.npy", "stats.npy"]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    V, d = line["config"]["vocab_size"], 100
    rows = a["rows.npy"].astype(np.int64)
    assert a["W.npy"].dtype == a["C.npy"].dtype == np.float32
    assert a["W.npy"].shape == a["C.npy"].shape == (rows.size, d) and 0 < rows.size <= V and rows.max() < V
    assert np.isfinite(a["W.npy"]).all() and np.isfinite(a["C.npy"]).all()
    # the probe step trained: C starts at zero and W within +-0.5 / d
    assert (np.abs(a["C.npy"]).max(1) > 0).sum() > 100
    assert np.abs(a["W.npy"]).max() > 0.5 / d
    # the timed steps trained the whole shard twice, the probe its first sentences
    assert a["stats.npy"][STAT_SENTENCES] == 2 * (400_000 // 1000) and a["stats.npy"][STAT_WORDS] == 2 * words
    assert 0 < a["probe_stats.npy"][STAT_SENTENCES] <= 400 and a["probe_stats.npy"][STAT_CENTERS] > 0
    assert a["stats.npy"][STAT_NONFINITE] == 0 and a["probe_stats.npy"][STAT_NONFINITE] == 0
    assert 0 < a["probe_stats.npy"][STAT_WORDS] <= 64 * 1000
    for k in a:  # same arguments, same outputs, to the bit: one wavefront applies its updates in a fixed order
        assert np.array_equal(a[k], b[k]), k
