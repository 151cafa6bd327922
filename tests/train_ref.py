"""Float64 restatement of one sentence's training update (the reference's
Word2Vec.cpp:232-353): skip-gram and CBOW, hierarchical softmax, negative
sampling or both (HS first, then NS, for each target), CBOW as a mean or as a
sum. Plain numpy, every product, sum and sigmoid in float64.

Philox mode only: the draws are the oracle's Philox draws (counter layout of
oracle/w2v_oracle.cpp:PhiloxDraws), taken from tests/refpy.philox4x32_10,
which tests/test_oracle_pins.py pins to the known answers and to the oracle's
own function. The NS targets are in canonical order: the positive first, then
the first occurrence of each negative in draw order. No hash-map order enters.

The decisions (subsampling, window shrink, table word) are integer and float32
comparisons and are restated exactly; only the arithmetic is wider.
"""
from __future__ import annotations

import numpy as np

from tests.refpy import philox4x32_10

M32 = 0xFFFFFFFF


def _key(key):
    return (int(key) & M32, (int(key) >> 32) & M32)


def token_draws(i, s, epoch, key, window):
    """(subsampling uniform as float32, window shrink) of position i of sentence s."""
    o = philox4x32_10((i & M32, s & M32, M32, epoch & M32), _key(key))
    u = np.float32(o[0]) / np.float32(4294967296.0)  # generate_canonical<float, 24> on one draw
    if u >= np.float32(1.0):
        u = np.nextafter(np.float32(1.0), np.float32(0.0))
    return u, (o[1] * max(window, 1)) >> 32


def table_pos(i, s, slot, k, epoch, key, table_size):
    ctr = (i & M32, s & M32, ((slot << 8) | (k & 255)) & M32, (epoch ^ ((k >> 8) << 20)) & M32)
    o = philox4x32_10(ctr, _key(key))
    return (((o[1] << 32) | o[0]) * table_size) >> 64


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


class TrainRef:
    """The model in float64 and the vocabulary products the update reads:
    `keep` (float32 sample probabilities), `table` (the unigram table's words),
    `huffman` = (codes, points, offsets) as Oracle.huffman() returns them."""

    def __init__(self, W, C, S, *, window, negative, hs, cbow, cbow_mean, keep, table=None, huffman=None):
        self.W = np.array(W, np.float64)
        self.C = None if C is None else np.array(C, np.float64)
        self.S = None if S is None else np.array(S, np.float64)
        self.window, self.negative, self.hs, self.cbow, self.cbow_mean = window, negative, hs, cbow, cbow_mean
        self.keep = np.asarray(keep, np.float32)
        self.table = table
        self.huffman = huffman
        self.centers = 0

    def _hs(self, word, x, g, alpha):
        codes, points, off = self.huffman
        for k in range(int(off[word]), int(off[word + 1])):
            r = self.S[points[k]]
            gg = (1.0 - float(codes[k]) - sigmoid(r @ x)) * alpha
            g += gg * r   # the row before its own update
            r += gg * x

    def _ns(self, word, x, g, M, alpha, i, s, slot, epoch, key):
        targets = [(word, 1.0)]
        for k in range(self.negative):
            n = int(self.table[table_pos(i, s, slot, k, epoch, key, len(self.table))])
            if all(n != t for t, _ in targets):
                targets.append((n, 0.0))
        for t, label in targets:
            r = M[t]
            gg = (label - sigmoid(r @ x)) * alpha
            g += gg * r
            r += gg * x

    def sentence(self, sent, s, alpha, epoch, key):
        """Train sentence number `s` (token ids `sent`) at `alpha`."""
        sent = [int(w) for w in sent]
        n_tok = len(sent)
        alpha = float(alpha)
        for i, c in enumerate(sent):
            u, rw = token_draws(i, s, epoch, key, self.window)
            if self.keep[c] < u:
                continue
            lo, hi = max(0, i - self.window + rw), min(n_tok, i + self.window + 1 - rw)
            if not self.cbow:
                if hi - lo <= 1:  # an empty window trains nothing and is no center (include/w2v_dev.h)
                    continue
                x = self.W[c].copy()  # held fixed over the window
                g = np.zeros_like(x)
                slot = 0
                for j in range(lo, hi):
                    if j == i:
                        continue
                    if self.hs:
                        self._hs(sent[j], x, g, alpha)
                    if self.negative > 0:
                        self._ns(sent[j], x, g, self.C, alpha, i, s, slot, epoch, key)
                    slot += 1
                self.W[c] += g
                self.centers += 1
                continue
            n = hi - lo - 1  # the positional count
            if n <= 0:
                continue
            ctx = sorted(set(sent[j] for j in range(lo, hi) if j != i))  # the set of ids, ascending
            h = np.zeros(self.W.shape[1])
            for w in ctx:
                h += self.C[w]
            if self.cbow_mean:
                h /= n
            g = np.zeros_like(h)
            if self.hs:
                self._hs(c, h, g, alpha)
            if self.negative > 0:
                self._ns(c, h, g, self.W, alpha, i, s, 0, epoch, key)
            if self.cbow_mean:
                g /= n
            for w in ctx:
                self.C[w] += g
            self.centers += 1
