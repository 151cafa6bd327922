#!/usr/bin/env python3
"""Time the word classes on the GPU (word2vec_amd/nn.py NearestIndex.classes,
word2vec's -classes) at the headline vocabulary against the only path a user
had before: a float32 rows @ centroids.T plus argmax on the host.

Shape: random normal rows, V 740,391, d 300, 10 iterations, K 500 (word2vec's
usual class count), 100 and 5,000. Per K one JSON line:
  ms_per_iteration      wall time of classes(K, 10) / 10, the best of --repeats
                        calls after one warm-up (index creation excluded; the
                        run's allocations and its result copies included)
  update_ms, assign_ms  device time of the two steps per iteration (event
                        timestamps around each step's kernels, w2v_nn_class_times)
  assign_frac_of_peak   2 V K pitch / assign time against the 157.3 TF f32 MFMA
                        peak bench.py uses (DESIGN.md 4.4 gives nn_score_kernel's)
  update_frac_of_hbm    V pitch 4 bytes / update time against 8 TB/s
  host_assign_ms        one assignment step with numpy at 16 threads (unless
                        OMP_NUM_THREADS says otherwise), in chunks of 65,536 rows

    python tools/classes_bench.py [--classes 500 100 5000] [--repeats 3] [--skip-baseline] [--vocab N] [--dim N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", os.environ["OMP_NUM_THREADS"])
os.environ.setdefault("MKL_NUM_THREADS", os.environ["OMP_NUM_THREADS"])

import numpy as np  # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from word2vec_amd.nn import NearestIndex, class_times  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # bench.py's PEAK_F32_MFMA_TFLOPS
PEAK_HBM_TBS = 8.0


def host_assign(rows, centroids, chunk=65_536):
    """The baseline: float32 scores and their argmax, a chunk of rows at a time."""
    out = np.empty(len(rows), np.int32)
    ct = np.ascontiguousarray(centroids.T)
    for r0 in range(0, len(rows), chunk):
        out[r0:r0 + chunk] = (rows[r0:r0 + chunk] @ ct).argmax(axis=1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vocab", type=int, default=740_391)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--classes", type=int, nargs="+", default=[500, 100, 5000])
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true", help="do not time the numpy path")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    V, d, n_it = a.vocab, a.dim, a.iterations
    vecs = np.random.default_rng(a.seed).standard_normal((V, d), dtype=np.float32)
    pitch = (d + 15) // 16 * 16
    t0 = time.perf_counter()
    index = NearestIndex.from_matrix(vecs)
    print(json.dumps({"index_create_s": round(time.perf_counter() - t0, 3), "vocab": V, "dim": d, "pitch": pitch}),
          flush=True)
    for k in a.classes:
        index.classes(k, 1)  # warm-up: code load
        best = None
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            r = index.classes(k, n_it)
            wall = time.perf_counter() - t0
            if best is None or wall < best[0]:
                best = (wall, class_times(), r)
        wall, t, r = best
        run = r["iterations"]
        up, asg = t["update_ms"] / run, t["assign_ms"] / run
        line = {"classes": k, "iterations": run, "ms_per_iteration": round(wall * 1e3 / run, 3),
                "update_ms": round(up, 3), "assign_ms": round(asg, 3),
                "assign_tflops": round(2.0 * V * k * pitch / (asg * 1e-3) / 1e12, 2),
                "assign_frac_of_peak": round(2.0 * V * k * pitch / (asg * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 3),
                "update_tb_s": round(V * pitch * 4 / (up * 1e-3) / 1e12, 3),
                "update_frac_of_hbm": round(V * pitch * 4 / (up * 1e-3) / 1e12 / PEAK_HBM_TBS, 3),
                "moved_last": int(r["moved"][-1])}
        if not a.skip_baseline:
            t0 = time.perf_counter()
            got = host_assign(vecs, r["centroids"])
            base = time.perf_counter() - t0
            line.update({"host_assign_ms": round(base * 1e3, 1), "host_threads": int(os.environ["OMP_NUM_THREADS"]),
                         "host_over_gpu_assign": round(base * 1e3 / asg, 1),
                         "host_agrees": round(float((got == r["classes"]).mean()), 5)})
        print(json.dumps(line), flush=True)
    index.close()


if __name__ == "__main__":
    main()
