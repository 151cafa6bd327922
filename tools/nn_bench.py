#!/usr/bin/env python3
"""Time the GPU nearest-neighbour queries (word2vec_amd/nn.py) at the headline
vocabulary against evaluate.analogy_accuracy's numpy path.

Shapes (V 740,391, d 300, random normal rows, random analogy questions):
  analogy       nq 19,544 (the size of questions-words.txt), k 1, all rows
  analogy_30k   the same questions, candidates restricted to the first 30,000 rows
  topk10        nq 1,024, k 10, all rows
Per shape one JSON line: ms per call (index creation excluded; the best and the
median of --repeats calls after one warm-up), 2 nq rows pitch / time against
the 157.3 TF f32 MFMA peak bench.py uses, and for the two analogy shapes the
time of evaluate.analogy_accuracy without an index on the same box (16 host
threads unless OMP_NUM_THREADS says otherwise) on the same questions, with
whether the two paths counted the same number of correct answers.

    python tools/nn_bench.py [--repeats 3] [--skip-baseline] [--vocab N] [--questions N]
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

from word2vec_amd.evaluate import analogy_accuracy  # noqa: E402
from word2vec_amd.nn import NearestIndex  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3  # bench.py's PEAK_F32_MFMA_TFLOPS


def timed(fn, repeats):
    fn()  # warm-up: scratch allocation, code load
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, min(ts), float(np.median(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--vocab", type=int, default=740_391)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--questions", type=int, default=19_544)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true", help="do not time the numpy path")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    rng = np.random.default_rng(a.seed)
    V, d = a.vocab, a.dim
    vecs = rng.standard_normal((V, d), dtype=np.float32)
    words = [str(i) for i in range(V)]
    lim = min(30_000, V)
    # questions over the first `lim` words, so the restricted shape answers all of them too
    Q = rng.integers(0, lim, size=(a.questions, 4))
    questions = [tuple(str(x) for x in row) for row in Q]
    pitch = (d + 15) // 16 * 16

    t0 = time.perf_counter()
    index = NearestIndex.from_matrix(vecs)
    print(json.dumps({"index_create_s": round(time.perf_counter() - t0, 3), "vocab": V, "dim": d, "pitch": pitch}),
          flush=True)

    def report(name, nq, rows, k, best, med, extra):
        flops = 2.0 * nq * rows * pitch
        line = {"shape": name, "nq": nq, "rows": rows, "k": k, "ms": round(best * 1e3, 3),
                "ms_median": round(med * 1e3, 3), "tflops": round(flops / best / 1e12, 2),
                "pct_of_f32_mfma_peak": round(100.0 * flops / best / 1e12 / PEAK_F32_MFMA_TFLOPS, 1),
                "plan": index.plan()}
        line.update(extra)
        print(json.dumps(line), flush=True)

    ids = np.stack([Q[:, 1], Q[:, 0], Q[:, 2]], axis=1).astype(np.int32)
    # make every second question "correct" (its expected word is the GPU's restricted answer), so that the
    # two paths' `correct` counts compare something: random rows have no analogy structure of their own
    best, _ = index.query_rows(ids, (1.0, -1.0, 1.0), k=1, restrict=lim)
    Q[::2, 3] = best[::2, 0]
    questions = [tuple(str(x) for x in row) for row in Q]
    for name, restrict in (("analogy", None), ("analogy_30k", lim)):
        rows = V if restrict is None else restrict
        _, best, med = timed(lambda: index.query_rows(ids, (1.0, -1.0, 1.0), k=1, restrict=restrict or 0), a.repeats)
        got = analogy_accuracy(words, vecs, questions, restrict=restrict, index=index)
        extra = {"correct_gpu": got["correct"], "answered": got["answered"]}
        if not a.skip_baseline:
            t0 = time.perf_counter()
            want = analogy_accuracy(words, vecs, questions, restrict=restrict)
            base = time.perf_counter() - t0
            t0 = time.perf_counter()
            analogy_accuracy(words, vecs, questions, restrict=restrict, index=index)
            whole = time.perf_counter() - t0
            extra.update({"numpy_s": round(base, 3), "numpy_threads": int(os.environ["OMP_NUM_THREADS"]),
                          "gpu_analogy_accuracy_s": round(whole, 3), "speedup_end_to_end": round(base / whole, 1),
                          "correct_numpy": want["correct"]})
        report(name, len(ids), rows, 1, best, med, extra)

    q10 = ids[:1024, :1].copy()
    _, best, med = timed(lambda: index.query_rows(q10, k=10), a.repeats)
    report("topk10", len(q10), V, 10, best, med, {})
    index.close()


if __name__ == "__main__":
    main()
