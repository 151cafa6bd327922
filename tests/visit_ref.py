"""The visits of a training epoch as integers: which (center, context, target)
triples a launch must make, whatever its grid, segmentation or wave cap.

In Philox mode the keep test, the window shrink and every table draw are pure
functions of (key, epoch, sentence, position, slot, k) (w2v_philox.hpp; the
counter layouts are tests/train_ref.py's token_draws and table_pos), so the
statistics of include/w2v_dev.h and the number of updates every row of W, C
and synapses1 receives are exact, schedule-independent integers. `visits`
computes them for the per-pair update over the whole corpus at once with the
numpy Philox of tests/score_ref.py; `visits_loop` is the same definition one
token at a time on tests/refpy's scalar Philox (tests/test_visit_ref.py holds
the two together). `shared_visits` / `shared_visits_loop` restate the shared-
negatives minibatch (oracle/w2v_oracle.cpp:sgsn_sentence).

Counters (include/w2v_dev.h):
  words      tokens of the sentences visited
  sentences  sentences visited
  centers    tokens kept by keep[c] >= u whose shrunk window holds at least
             one other position (a kept token with an empty window, as in a
             one-token sentence, moves no row and is not counted, in any mode)
  contexts   skip-gram: (center, context) pairs; CBOW: distinct context ids
  targets    per NS call 1 + the distinct drawn words that differ from the
             positive; per HS call the path length; HS+NS both
  draws      `negative` per NS call

An "update" of a row is one add to it: skip-gram W[center] once per kept
center with a context (the sum over its window), the NS target rows / Huffman
nodes once per (context, target); CBOW the target rows once per center and
C[u] once per distinct context id u. `updates[k]` counts them per row of
matrix k (0 W, 1 C, 2 synapses1; None where the mode has no such matrix); its
zero entries are the rows a launch must leave bit-identical.
"""
from __future__ import annotations

import numpy as np

from tests.score_ref import philox_vec, table_pos_vec
from tests.train_ref import table_pos, token_draws

M32 = 0xFFFFFFFF
COUNTERS = ("words", "centers", "contexts", "targets", "draws", "sentences")


def _token_draws_vec(pos, sent, epoch, key, window):
    """token_draws for arrays of (position, sentence): (u as float32, shrink)."""
    o0, o1, _, _ = philox_vec(pos, sent, np.uint64(M32), np.uint64(epoch & M32), key)
    u = o0.astype(np.float32) / np.float32(4294967296.0)
    u = np.where(u >= np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0.0)), u).astype(np.float32)
    return u, ((o1 * np.uint64(max(window, 1))) >> np.uint64(32)).astype(np.int64)


def _draw_words(pos, sent, slot, negative, epoch, key, bounds):
    """The `negative` table words of each (position, sentence, slot): shape (n, negative)."""
    k = np.arange(negative, dtype=np.uint64)[None, :]
    c2 = (slot.astype(np.uint64)[:, None] << np.uint64(8)) | (k & np.uint64(255))
    c3 = np.uint64(epoch & M32) ^ ((k >> np.uint64(8)) << np.uint64(20))
    o0, o1, _, _ = philox_vec(pos.astype(np.uint64)[:, None], sent.astype(np.uint64)[:, None], c2, c3, key)
    p = table_pos_vec(o0, o1, int(bounds[-1])).astype(np.int64)
    return np.searchsorted(bounds, p, "right") - 1


def _row_sets(ids):
    """Per row of `ids` (entries < 0 are holes) the first occurrence of every
    distinct id in sorted order: (sorted ids, mask of the distinct valid ones)."""
    s = np.sort(ids, axis=1)
    first = np.ones(s.shape, bool)
    first[:, 1:] = s[:, 1:] != s[:, :-1]
    return s, first & (s >= 0)


def _result(V, hs, cbow, negative):
    return dict({k: 0 for k in COUNTERS},
                updates=[np.zeros(V, np.int64), np.zeros(V, np.int64) if (negative > 0 or cbow) else None,
                         np.zeros(max(V - 1, 0), np.int64) if hs else None])


def _order(offsets, order):
    n = len(offsets) - 1
    return np.arange(n, dtype=np.int64) if order is None else np.asarray(order, np.int64)


def _finish(out, V, pred_hits, huffman, cbow, negative, hs):
    """Rows reached through the predicted word: its NS row once per call, its
    Huffman nodes once per call."""
    if negative > 0:
        out["updates"][0 if cbow else 1] += pred_hits
    if hs:
        _, points, coff = huffman
        L = np.diff(np.asarray(coff, np.int64))
        out["targets"] += int((pred_hits * L).sum())
        np.add.at(out["updates"][2], np.asarray(points, np.int64)[:int(coff[V])], np.repeat(pred_hits, L))
    return out


def visits(ids, offsets, keep, *, window, negative=0, hs=False, cbow=False, key=0, epoch=0, bounds=None,
           huffman=None, order=None, shrink=True, chunk=1 << 21):
    """The counters and per-row update counts of one epoch over the sentences
    `order` lists (default: all, each once). `bounds`: the unigram table as
    V + 1 boundaries (Oracle.table_bounds); `huffman` = (codes, points,
    offsets). shrink=False trains every center on its full window (for the
    comparison with tests/score_ref.py; the device always shrinks)."""
    ids = np.asarray(ids, np.int64)
    off = np.asarray(offsets, np.int64)
    keep = np.asarray(keep, np.float32)
    V = keep.size
    out = _result(V, hs, cbow, negative)
    order = _order(off, order)
    lens = off[order + 1] - off[order]
    out["sentences"] = int(order.size)
    out["words"] = int(lens.sum())
    if out["words"] == 0:
        return _finish(out, V, np.zeros(V, np.int64), huffman, cbow, negative, hs)
    # one entry per token visited: its sentence, position, sentence bounds in `ids`
    sent = np.repeat(order, lens)
    start = np.repeat(off[order], lens)
    pos = np.arange(out["words"], dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    end = start + np.repeat(lens, lens)
    u, rw = _token_draws_vec(pos, sent, epoch, key, window)
    if not shrink:
        rw[:] = 0
    kept = keep[ids[start + pos]] >= u
    sent, start, end, pos, rw = (a[kept] for a in (sent, start, end, pos, rw))
    pred_hits = np.zeros(V, np.int64)
    offs = np.concatenate([np.arange(-window, 0), np.arange(1, window + 1)]).astype(np.int64)
    rows = max(1, chunk // max(1, 2 * window * max(1, negative)))
    for a in range(0, sent.size, rows):
        sl = slice(a, a + rows)
        g = (start[sl] + pos[sl])[:, None]                       # the center's index in ids
        lo = np.maximum(start[sl], start[sl] + pos[sl] - window + rw[sl])[:, None]
        hi = np.minimum(end[sl], start[sl] + pos[sl] + window + 1 - rw[sl])[:, None]
        j = g + offs[None, :]
        valid = (j >= lo) & (j < hi)
        ctx = np.where(valid, ids[np.clip(j, 0, ids.size - 1)], -1)
        n = valid.sum(axis=1)                                     # positional count
        c = ids[g[:, 0]]
        has = n > 0
        out["centers"] += int(has.sum())
        if cbow:
            s, distinct = _row_sets(ctx)
            out["contexts"] += int(distinct.sum())
            np.add.at(out["updates"][1], s[distinct], 1)
            pred_hits += np.bincount(c[has], minlength=V)
            if negative > 0:
                dw = _draw_words(pos[sl][has], sent[sl][has], np.zeros(int(has.sum()), np.int64), negative, epoch,
                                 key, bounds)
                pred = c[has]
        else:
            out["contexts"] += int(n.sum())
            np.add.at(out["updates"][0], c[has], 1)
            pred = ctx[valid]                                     # row-major: a center's contexts in position order
            pred_hits += np.bincount(pred, minlength=V)
            if negative > 0:
                slot = (np.cumsum(valid, axis=1) - 1)[valid]
                r = np.nonzero(valid)[0]
                dw = _draw_words(pos[sl][r], sent[sl][r], slot, negative, epoch, key, bounds)
        if negative > 0:
            out["draws"] += int(dw.size)
            s, distinct = _row_sets(dw)
            distinct &= s != pred[:, None]
            out["targets"] += int(pred.size + distinct.sum())
            np.add.at(out["updates"][0 if cbow else 1], s[distinct], 1)
    return _finish(out, V, pred_hits, huffman, cbow, negative, hs)


def visits_loop(ids, offsets, keep, *, window, negative=0, hs=False, cbow=False, key=0, epoch=0, table=None,
                huffman=None, order=None):
    """The same definition, one token at a time, on the scalar Philox and the
    unigram table itself (`table`: the word of every table position)."""
    ids = [int(w) for w in ids]
    keep = np.asarray(keep, np.float32)
    V = keep.size
    out = _result(V, hs, cbow, negative)
    W, C, S = out["updates"]

    def predict(word, i, s, slot):
        if hs:
            _, points, coff = huffman
            nodes = [int(p) for p in points[int(coff[word]):int(coff[word + 1])]]
            out["targets"] += len(nodes)
            for p in nodes:
                S[p] += 1
        if negative > 0:
            M = W if cbow else C
            targets = [word]
            for k in range(negative):
                t = int(table[table_pos(i, s, slot, k, epoch, key, len(table))])
                if t not in targets:
                    targets.append(t)
            out["draws"] += negative
            out["targets"] += len(targets)
            for t in targets:
                M[t] += 1

    for s in _order(offsets, order):
        s = int(s)
        sent = ids[int(offsets[s]):int(offsets[s + 1])]
        out["sentences"] += 1
        out["words"] += len(sent)
        for i, c in enumerate(sent):
            u, rw = token_draws(i, s, epoch, key, window)
            if keep[c] < u:
                continue
            lo, hi = max(0, i - window + rw), min(len(sent), i + window + 1 - rw)
            ctx = [sent[j] for j in range(lo, hi) if j != i]
            if not ctx:
                continue
            if not cbow:
                out["centers"] += 1
                out["contexts"] += len(ctx)
                for slot, w in enumerate(ctx):
                    predict(w, i, s, slot)
                W[c] += 1
            else:
                out["centers"] += 1
                out["contexts"] += len(set(ctx))
                predict(c, i, s, 0)
                for w in set(ctx):
                    C[w] += 1
    return out


def shared_visits(ids, offsets, keep, *, window, negative, key=0, epoch=0, bounds=None, order=None):
    """The shared-negatives minibatch (sgsn_sentence): the window is taken over
    the KEPT tokens of the sentence; a kept center with at least one context
    counts as a center, its distinct context ids as contexts (the inputs: W
    rows, one update each), the center plus the distinct shared draws that
    differ from it as targets (the outputs: C rows), `negative` draws."""
    ids = np.asarray(ids, np.int64)
    off = np.asarray(offsets, np.int64)
    keep = np.asarray(keep, np.float32)
    V = keep.size
    out = _result(V, False, False, negative)
    order = _order(off, order)
    lens = off[order + 1] - off[order]
    out["sentences"] = int(order.size)
    out["words"] = int(lens.sum())
    if out["words"] == 0:
        return out
    visit = np.repeat(np.arange(order.size), lens)               # a sentence listed twice is two visits
    sent = np.repeat(order, lens)
    pos = np.arange(out["words"], dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    tok = ids[np.repeat(off[order], lens) + pos]
    u, rw = _token_draws_vec(pos, sent, epoch, key, window)
    kept = keep[tok] >= u
    visit, sent, pos, tok, rw = (a[kept] for a in (visit, sent, pos, tok, rw))
    nk = np.bincount(visit, minlength=order.size)                # kept tokens per visit
    start = np.repeat(np.cumsum(nk) - nk, nk)                    # the visit's first kept token
    end = start + np.repeat(nk, nk)
    t = np.arange(tok.size, dtype=np.int64)
    offs = np.concatenate([np.arange(-window, 0), np.arange(1, window + 1)]).astype(np.int64)
    lo = np.maximum(start, t - window + rw)[:, None]
    hi = np.minimum(end, t + window + 1 - rw)[:, None]
    j = t[:, None] + offs[None, :]
    valid = (j >= lo) & (j < hi)
    ctx = np.where(valid, tok[np.clip(j, 0, tok.size - 1)], -1)
    has = valid.any(axis=1)
    out["centers"] = int(has.sum())
    s, distinct = _row_sets(ctx)
    out["contexts"] = int(distinct.sum())
    np.add.at(out["updates"][0], s[distinct], 1)
    c = tok[has]
    dw = _draw_words(pos[has], sent[has], np.zeros(c.size, np.int64), negative, epoch, key, bounds)
    out["draws"] = int(dw.size)
    s, distinct = _row_sets(dw)
    distinct &= s != c[:, None]
    out["targets"] = int(c.size + distinct.sum())
    out["updates"][1] += np.bincount(c, minlength=V)
    np.add.at(out["updates"][1], s[distinct], 1)
    return out


def shared_visits_loop(ids, offsets, keep, *, window, negative, key=0, epoch=0, table=None, order=None):
    """shared_visits one center at a time (sgsn_sentence's own loops)."""
    ids = [int(w) for w in ids]
    keep = np.asarray(keep, np.float32)
    out = _result(keep.size, False, False, negative)
    W, C, _ = out["updates"]
    for s in _order(offsets, order):
        s = int(s)
        sent = ids[int(offsets[s]):int(offsets[s + 1])]
        out["sentences"] += 1
        out["words"] += len(sent)
        kept = []
        for i, c in enumerate(sent):
            u, rw = token_draws(i, s, epoch, key, window)
            if keep[c] >= u:
                kept.append((c, i, rw))
        for t, (c, i, rw) in enumerate(kept):
            lo, hi = max(0, t - window + rw), min(len(kept), t + window + 1 - rw)
            inputs = set(kept[j][0] for j in range(lo, hi) if j != t)
            if not inputs:
                continue
            outputs = [c]
            for k in range(negative):
                n = int(table[table_pos(i, s, 0, k, epoch, key, len(table))])
                if n not in outputs:
                    outputs.append(n)
            out["centers"] += 1
            out["contexts"] += len(inputs)
            out["targets"] += len(outputs)
            out["draws"] += negative
            for w in inputs:
                W[w] += 1
            for w in outputs:
                C[w] += 1
    return out
