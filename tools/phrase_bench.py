#!/usr/bin/env python3
"""Time phrase detection on the GPU (word2vec_amd/phrases.py GpuPhrases,
word2phrase over the ingested ids) on one MI355X against two
yardsticks on the same box and the same corpus: the ingest's own count + map of
the corpus file, and tests/phrase_ref.py's numpy pass (np.unique over the
64-bit pair keys).

Corpus: --tokens tokens, Zipf over --vocab words in which one token in five is
its predecessor's fixed successor (collocations of every strength) plus 200
planted pairs, written as a "lines" file of 40-token lines. JSON lines:
  ingest   count_s, map_s (w2v_ingest_count / _map of the file) and tokens/s
  pass k   wall_s of w2v_phrase_pass, the steps' seconds (w2v_phrase_times:
           histogram, insert with growth, count, score + join, rewrite) and
           tokens/s per step, the distinct eligible pairs, the joins, the
           phrases and the pair table's final slots
  numpy    wall_s of phrase_ref.pass_vec for the first pass, and that its
           rewritten stream equals the GPU's

    python tools/phrase_bench.py [--tokens N] [--vocab N] [--passes 200 100] [--min-count 5] [--skip-numpy]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from tests import phrase_ref  # noqa: E402
from word2vec_amd.ingest import GpuIngest  # noqa: E402
from word2vec_amd.phrases import GpuPhrases  # noqa: E402

STEPS = ("histogram", "insert", "count", "score_join", "rewrite")


def corpus_ids(n, vocab, seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    ids = rng.choice(vocab, size=n, p=p / p.sum()).astype(np.int32)
    succ = rng.permutation(vocab).astype(np.int32)
    follow = np.flatnonzero(rng.random(n) < 0.2)[1:]
    ids[follow] = succ[ids[follow - 1]]
    for k in range(200):  # planted pairs of mid-frequency words
        at = rng.integers(0, n - 1, size=max(50, n // 100_000))
        ids[at], ids[at + 1] = vocab + 2 * k, vocab + 2 * k + 1
    return ids


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", type=int, default=16_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--passes", type=float, nargs="+", default=[200.0, 100.0], help="one threshold per pass")
    ap.add_argument("--min-count", type=int, default=5)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()

    n = a.tokens // 40 * 40
    ids = corpus_ids(n, a.vocab, a.seed)
    words = np.array([f"w{i}" for i in range(a.vocab + 400)])
    with tempfile.TemporaryDirectory() as d:
        path = Path(d) / "corpus.txt"
        with open(path, "w") as f:
            for row in words[ids].reshape(-1, 40):
                f.write(" ".join(row) + "\n")
        size = path.stat().st_size
        GpuIngest(path, "lines", device=0).close()  # warm-up: code load, context
        g = GpuIngest(path, "lines", device=0)
        t0 = time.perf_counter()
        found = g.count()
        t1 = time.perf_counter()
        g.map({w: i for i, (w, _) in enumerate(found)})
        t2 = time.perf_counter()
        print(json.dumps({"step": "ingest", "tokens": n, "bytes": size, "distinct_words": len(found),
                          "count_s": round(t1 - t0, 4), "map_s": round(t2 - t1, 4),
                          "tokens_per_s": round(n / (t2 - t0))}), flush=True)
        stream_ids, stream_off, _ = g.samples()
        warm = GpuPhrases.from_ids(stream_ids[:4096], [0, 4096], len(found), device=0)
        warm.run(a.min_count, a.passes[0])  # warm-up: code load
        warm.close()
        p = GpuPhrases.from_ingest(g, device=0)
        g.close()
    first = None
    for k, thr in enumerate(a.passes):
        before = p.summary()["n_ids"]
        t0 = time.perf_counter()
        s = p.run(a.min_count, thr)
        wall = time.perf_counter() - t0
        t = p.times()
        line = {"step": f"pass {k + 1}", "threshold": thr, "min_count": a.min_count, "tokens": before,
                "wall_s": round(wall, 4), "tokens_per_s": round(before / wall),
                "seconds": {x: round(t[x], 5) for x in STEPS},
                "tokens_per_s_by_step": {x: round(before / max(t[x], 1e-9)) for x in STEPS},
                "distinct_pairs": s["n_bigrams"], "joined": s["n_joined"], "phrases": s["n_phrases"],
                "table_slots": t["table_slots"]}
        print(json.dumps(line), flush=True)
        if k == 0:
            first = p.stream()
    p.close()
    if not a.skip_numpy:
        t0 = time.perf_counter()
        ref = phrase_ref.pass_vec(stream_ids, stream_off, len(found), a.min_count, a.passes[0])
        wall = time.perf_counter() - t0
        print(json.dumps({"step": "numpy pass 1", "wall_s": round(wall, 3), "tokens_per_s": round(n / wall),
                          "equals_gpu": bool(np.array_equal(ref.ids, first[0]) and np.array_equal(ref.offsets, first[1]))}),
              flush=True)


if __name__ == "__main__":
    main()
