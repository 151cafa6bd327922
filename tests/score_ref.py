"""Float64 restatement of w2v_dev_score (include/w2v_dev.h): the log-likelihood
of sentences under a model, every token a center with the full window.

Two forms of one definition: `score_loop` walks term by term and draws with
tests/refpy.philox4x32_10; `score_vec` evaluates a center's targets with one
matrix product and draws with a numpy Philox (pinned to refpy's in
tests/test_score_ref.py). Both return, per sentence, the score, the number of
terms and the a-priori bound on the device's error

    bound[s] = sum over terms of (NV + 14 + e) * 2^-24 * (sum_k |a_k b_k| + |term|)

NV = ceil(d / 64) is the serial additions of a lane's part of the dot product,
14 = 6 levels of the cross-lane reduction + 8 for expf, log1pf and the final
operations, e = (distinct context ids + 1) for CBOW's summed (and divided)
input, else 0. It is derived from the arithmetic, not from what the device
returns.
"""
from __future__ import annotations

import numpy as np

from tests.refpy import philox4x32_10

M32 = 0xFFFFFFFF
EPS = 2.0 ** -24


def logsig(z):
    z = np.asarray(z, np.float64)
    return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def philox_vec(c0, c1, c2, c3, key):
    """Philox4x32-10 over arrays of counters (uint64 arrays holding 32-bit words)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(M32) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(key) & M32, (int(key) >> 32) & M32
    m = np.uint64(M32)
    s = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> s) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> s) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def table_pos_vec(o0, o1, table_size):
    """mulhi64(o1:o0, table_size) for table_size < 2^32."""
    assert 0 < table_size < (1 << 32)
    t = np.uint64(table_size)
    return (o1 * t + ((o0 * t) >> np.uint64(32))) >> np.uint64(32)


def table_pos(i, s, slot, k, key, table_size):
    o = philox4x32_10((i & M32, s & M32, ((slot << 8) | (k & 255)) & M32, 0), (key & M32, (key >> 32) & M32))
    return (((o[1] << 32) | o[0]) * table_size) >> 64


def chain_tree(V):
    """A degenerate Huffman tree as CSR (codes, points, offsets): internal node k hangs under node k - 1; word
    w < V - 1 is node w's code-1 child, the last word node V - 2's code-0 child. Paths are 1 .. V - 1 nodes."""
    codes, points, off = [], [], [0]
    for w in range(V):
        n = min(w + 1, V - 1)
        points += list(range(n))
        codes += [0] * (n - 1) + [1 if w < V - 1 else 0]
        off.append(len(points))
    return np.asarray(codes, np.uint8), np.asarray(points, np.int32), np.asarray(off, np.int64)


def _path(huffman, w):
    codes, points, coff = huffman
    a, b = int(coff[w]), int(coff[w + 1])
    return np.asarray(points[a:b], np.int64), 1.0 - 2.0 * np.asarray(codes[a:b], np.float64)


def _window(n, i, b):
    return max(0, i - b), min(n, i + b + 1)


class _Out:
    def __init__(self, n_sent, n_tok):
        self.ll = np.zeros(n_sent, np.float64)
        self.targets = np.zeros(n_sent, np.int64)
        self.bound = np.zeros(n_sent, np.float64)
        self.summary = dict(sentences=n_sent, words=n_tok, centers=0, contexts=0, targets=0, draws=0, nonfinite=0,
                            ll=0.0)
        self.min_z = np.inf       # the most negative sigma argument
        self.collisions = 0       # draws equal to their positive
        self.duplicates = 0       # draws repeating an earlier draw of their context

    def done(self):
        self.summary["targets"] = int(self.targets.sum())
        acc = 0.0
        for v in self.ll:  # sentence order
            acc += float(v)
        self.summary["ll"] = acc
        return dict(ll=self.ll, targets=self.targets, bound=self.bound, summary=self.summary, min_z=self.min_z,
                    collisions=self.collisions, duplicates=self.duplicates)


def _ns_set(pos_word, draws, out):
    """The distinct negatives other than the positive, in draw order."""
    seen = []
    for u in draws:
        u = int(u)
        if u == pos_word:
            out.collisions += 1
        elif u in seen:
            out.duplicates += 1
        else:
            seen.append(u)
    return seen


def score_loop(W, C, S, ids, offsets, *, window, negative=0, hs=False, cbow=False, cbow_mean=False, huffman=None,
               bounds=None, key=0):
    """The definition, one term at a time."""
    W, C, S = (None if m is None else np.asarray(m, np.float64) for m in (W, C, S))
    d = (W if W is not None else C).shape[1]
    nv = -(-d // 64)
    ids = np.asarray(ids, np.int64)
    off = np.asarray(offsets, np.int64)
    out = _Out(len(off) - 1, len(ids))
    tsize = int(bounds[-1]) if bounds is not None else 0

    def term(s, row, x, sign, e):
        z = 0.0
        az = 0.0
        for k in range(d):
            z += row[k] * x[k]
            az += abs(row[k] * x[k])
        z *= sign
        t = float(logsig(z))
        out.ll[s] += t
        out.targets[s] += 1
        out.bound[s] += (nv + 14 + e) * EPS * (az + abs(t))
        out.min_z = min(out.min_z, z)

    def draws(s, i, slot):
        words = []
        for k in range(negative):
            p = table_pos(i, s, slot, k, key, tsize)
            words.append(int(np.searchsorted(bounds, p, "right")) - 1)
        out.summary["draws"] += negative
        return words

    for s in range(len(off) - 1):
        sent = ids[off[s]:off[s + 1]]
        n = len(sent)
        for i in range(n):
            lo, hi = _window(n, i, window)
            ctx = [j for j in range(lo, hi) if j != i]
            if not ctx:
                continue
            out.summary["centers"] += 1
            if not cbow:
                out.summary["contexts"] += len(ctx)
                x = W[sent[i]]
                for t, j in enumerate(ctx):
                    wj = int(sent[j])
                    if hs:
                        pts, sg = _path(huffman, wj)
                        for p, g in zip(pts, sg):
                            term(s, S[p], x, g, 0)
                    else:
                        term(s, C[wj], x, 1.0, 0)
                        for u in _ns_set(wj, draws(s, i, t), out):
                            term(s, C[u], x, -1.0, 0)
            else:
                uniq = sorted(set(int(sent[j]) for j in ctx))
                out.summary["contexts"] += len(uniq)
                h = np.zeros(d)
                for u in uniq:
                    h = h + C[u]
                if cbow_mean:
                    h = h / len(ctx)
                e = len(uniq) + 1
                wi = int(sent[i])
                if hs:
                    pts, sg = _path(huffman, wi)
                    for p, g in zip(pts, sg):
                        term(s, S[p], h, g, e)
                else:
                    term(s, W[wi], h, 1.0, e)
                    for u in _ns_set(wi, draws(s, i, 0), out):
                        term(s, W[u], h, -1.0, e)
    return out.done()


def score_vec(W, C, S, ids, offsets, *, window, negative=0, hs=False, cbow=False, cbow_mean=False, huffman=None,
              bounds=None, key=0):
    """The same, a center's targets at a time."""
    W, C, S = (None if m is None else np.asarray(m, np.float64) for m in (W, C, S))
    d = (W if W is not None else C).shape[1]
    nv = -(-d // 64)
    ids = np.asarray(ids, np.int64)
    off = np.asarray(offsets, np.int64)
    out = _Out(len(off) - 1, len(ids))
    if bounds is not None:
        bounds = np.asarray(bounds, np.int64)
    tsize = int(bounds[-1]) if bounds is not None else 0
    paths = {}

    def path(w):
        if w not in paths:
            paths[w] = _path(huffman, w)
        return paths[w]

    def center_terms(s, M, rows, signs, x, e):
        R = M[rows]
        z = (R @ x) * signs
        az = np.abs(R) @ np.abs(x)
        t = logsig(z)
        out.ll[s] += float(np.sum(t))
        out.targets[s] += len(rows)
        out.bound[s] += float(np.sum((nv + 14 + e) * EPS * (az + np.abs(t))))
        out.min_z = min(out.min_z, float(z.min()))

    def draw_words(s, i, nslots):
        slot = np.repeat(np.arange(nslots, dtype=np.uint64), negative)
        k = np.tile(np.arange(negative, dtype=np.uint64), nslots)
        o0, o1, _, _ = philox_vec(np.uint64(i), np.uint64(s), (slot << np.uint64(8)) | k, np.uint64(0), key)
        pos = table_pos_vec(o0, o1, tsize).astype(np.int64)
        out.summary["draws"] += nslots * negative
        return (np.searchsorted(bounds, pos, "right") - 1).reshape(nslots, negative)

    for s in range(len(off) - 1):
        sent = ids[off[s]:off[s + 1]]
        n = len(sent)
        for i in range(n):
            lo, hi = _window(n, i, window)
            ctx = np.concatenate([sent[lo:i], sent[i + 1:hi]])
            if ctx.size == 0:
                continue
            out.summary["centers"] += 1
            if cbow:
                uniq = np.unique(ctx)
                out.summary["contexts"] += len(uniq)
                x = C[uniq].sum(axis=0)
                if cbow_mean:
                    x = x / ctx.size
                e = len(uniq) + 1
                preds, M = [int(sent[i])], W
            else:
                out.summary["contexts"] += ctx.size
                x, e = W[sent[i]], 0
                preds, M = [int(w) for w in ctx], C
            rows, signs = [], []
            if hs:
                for w in preds:
                    p, g = path(w)
                    rows.append(p)
                    signs.append(g)
                M = S
            else:
                dw = draw_words(s, i, len(preds))
                for t, w in enumerate(preds):
                    negs = _ns_set(w, dw[t], out)
                    rows.append(np.asarray([w] + negs, np.int64))
                    signs.append(np.asarray([1.0] + [-1.0] * len(negs)))
            rows = np.concatenate(rows)
            if rows.size:
                center_terms(s, M, rows, np.concatenate(signs), x, e)
    return out.done()
