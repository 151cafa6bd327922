#!/usr/bin/env python3
"""Time w2v_dev_score against the training kernel of the same mode (one MI355X).

The corpus is bench.py's synthetic Zipf corpus at configs[2]'s shape (skip-gram
NS, d 300, window 5, negative 5, 1 M ranks, 1000-token sentences; 20 M tokens by
default), plus one HS shape on the same corpus. Per mode, in one process on one
resident corpus: an untimed training epoch (warm-up; the model then has
content in every matrix), then `--repeats` alternations of a timed training
epoch and a timed score of the resident corpus. Both are timed with events on
the handle's stream around the call (the score call is synchronous and
includes its work-item table's upload). Reported per leg: seconds, words/s, ns
per target row (the device's own target counts), and the algorithmic bytes
(targets x row pitch x 4 plus the input rows) over time as a share of the
8 TB/s HBM peak — rows of a vocabulary that fits the caches are served from
them, so the share says how far the leg is from HBM-bound, not that it is.
One JSON line per leg on stdout.

  python tools/score_bench.py [--tokens 20000000] [--repeats 2] [--modes sg_ns,sg_hs]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM_PEAK_GBS = 8000.0


def corpus(args, torch, dev):
    """bench.py's generator: ranks ~ (r + q)^-s, vocabulary = the ranks seen >= min_count times, by count."""
    n_sent = args.tokens // args.sent_len
    n_tok = n_sent * args.sent_len
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed * 1000)
    p = torch.arange(1, args.vocab + 1, device=dev, dtype=torch.float64).pow_(-1.0)
    cdf = torch.cumsum(p, 0)
    cdf /= cdf[-1].clone()
    u = torch.rand(n_tok, generator=g, device=dev, dtype=torch.float64)
    ranks = torch.searchsorted(cdf, u, right=True).clamp_(max=args.vocab - 1)
    counts = torch.bincount(ranks, minlength=args.vocab)
    order = torch.argsort(counts, descending=True, stable=True)
    V = int((counts >= args.min_count).sum())
    remap = torch.full((args.vocab,), -1, dtype=torch.int64, device=dev)
    remap[order[:V]] = torch.arange(V, device=dev)
    ids = remap[ranks]
    inv = ids >= 0
    soff = torch.zeros(n_sent + 1, dtype=torch.int64, device=dev)
    soff[1:] = torch.cumsum(inv.view(n_sent, args.sent_len).sum(1), 0)
    return (counts[order[:V]].cpu().numpy().astype(np.int64), ids[inv].to(torch.int32).cpu().numpy(),
            soff.cpu().numpy(), n_tok)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=20_000_000)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--sent-len", type=int, default=1000)
    ap.add_argument("--min-count", type=int, default=5)
    ap.add_argument("--table-size", type=int, default=100_000_000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--modes", default="sg_ns,sg_hs")
    ap.add_argument("--item", type=int, default=0, help="centers per work item (0 = automatic)")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import torch

    from word2vec_amd import _native as N
    from word2vec_amd import host
    from word2vec_amd.device import Config, DeviceTrainer

    assert torch.cuda.is_available(), "score_bench needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    counts, ids, soff, n_tok = corpus(args, torch, dev)
    V, d = len(counts), args.dim
    print(f"[score_bench] {n_tok} raw tokens, {ids.size} in-vocab, V={V}", file=sys.stderr, flush=True)
    for mode in args.modes.split(","):
        hs, cbow = mode.endswith("hs"), mode.startswith("cbow")
        neg = 0 if hs else args.negative
        cfg = Config(word_dim=d, window=args.window, negative=neg, hs=hs, cbow=cbow, cbow_mean=True,
                     iter=1 + args.repeats, init_alpha=0.05 if cbow else 0.025, min_alpha=2.5e-6,
                     table_size=args.table_size, device=0)
        tr = DeviceTrainer(cfg)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.set_stream(stream)
        tr.set_stream(stream.cuda_stream)
        hf = host.huffman(counts) if hs else (None, None, None)
        tr.upload_vocab(host.sample_probs(counts, 1e-4), None if hs else host.table_bounds(counts, args.table_size), *hf)
        rng = np.random.default_rng(args.seed)
        W = ((rng.random((V, d), dtype=np.float32) - 0.5) / d).astype(np.float32)
        Cm = np.zeros((V, d), np.float32) if (neg > 0 or cbow) else None
        if cbow and hs:
            Cm = ((rng.random((V, d), dtype=np.float32) - 0.5) / d).astype(np.float32)
        tr.upload_model(W, Cm, np.zeros((V - 1, d), np.float32) if hs else None)
        del W, Cm
        tr.upload_corpus(ids, soff, n_tok)
        tr.set_rng(N.W2V_RNG_PHILOX, (args.seed << 32) | 1)
        tr.set_schedule(N.W2V_SCHED_PARALLEL)
        tr.set_progress(0)
        pitch = tr.row_pitch()

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record(stream)
            out = fn()
            b.record(stream)
            b.synchronize()
            return out, a.elapsed_time(b) * 1e-3, time.perf_counter() - t0

        def train(epoch):
            st0 = tr.read_stats()
            _, ev, wall = timed(lambda: (tr.train_epoch_async(epoch), tr.synchronize()))
            st1 = tr.read_stats()
            return {k: st1[k] - st0[k] for k in st1}, ev, wall

        def report(leg, rep, st, ev, wall, ll=None):
            inputs = st["centers"] if not cbow else st["contexts"] + st["centers"]
            gbs = (st["targets"] + inputs) * pitch * 4 / ev / 1e9
            row = {"mode": mode, "leg": leg, "repeat": rep, "seconds": round(ev, 4), "wall_seconds": round(wall, 4),
                   "words_per_s": round(st["words"] / ev), "targets": st["targets"],
                   "ns_per_target": round(ev / max(st["targets"], 1) * 1e9, 3), "algorithmic_GBs": round(gbs, 1),
                   "hbm_share": round(gbs / HBM_PEAK_GBS, 3), "dim": d, "pitch": pitch, "V": V, "tokens": int(ids.size)}
            if ll is not None:
                row["ll_per_target"] = ll / max(st["targets"], 1)
            print(json.dumps(row), flush=True)

        train(0)  # warm-up: code objects loaded, every matrix has content
        tr.score(item=args.item)  # ... and the scoring kernel's, with its buffers
        for rep in range(args.repeats):
            st, ev, wall = train(1 + rep)
            report("train", rep, st, ev, wall)
            sc, ev, wall = timed(lambda: tr.score(key=7, item=args.item))
            sm = dict(sc["summary"])
            report("score", rep, sm, ev, wall, sm["ll"])
        tr.close()


if __name__ == "__main__":
    main()
