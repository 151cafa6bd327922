"""CPU reference of phrase detection (include/w2v_ingest.h, w2v_phrase_*;
DESIGN.md §4.6): word2phrase's rule on a stream of token ids, as a plain
sequential loop (`pass_loop`, the definition) and vectorised (`pass_vec`,
np.unique over the 64-bit pair keys), a text writer and the corpus builders
the tests share.

A stream is ids[0, n) (int32, each in [0, n_words)) cut into sentences by
offsets[0..S] (int64). One pass with integer min_count >= 1 and float32
threshold >= 0:
  cnt[w]   occurrences of w, N = n;
  position i holds the eligible pair (a, b) = (ids[i-1], ids[i]) when i is not
           the first token of its sentence and cnt[a], cnt[b] >= min_count;
  pab      eligible positions holding (a, b);
  score    float32: (float)(pab - min_count) / (float)cnt[a] / (float)cnt[b] * (float)N;
  cand[i]  eligible and score > threshold (strict, float32);
  join[i]  cand[i] and not join[i-1];
a joined token disappears, the token before it becomes the phrase (a, b) with
id n_words + j, j numbering the distinct joined pairs by the position of their
first joined occurrence. Sentence boundaries stay where they were.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np


def _score(pab, min_count, ca, cb, n):
    f = np.float32
    return f(pab - min_count) / f(ca) / f(cb) * f(n)


def _result(ids, offsets, n_words, left, right, joined, bg, scores, n_joined):
    ids = np.asarray(ids, np.int32)
    total = n_words + len(left)
    count = np.bincount(ids, minlength=total).astype(np.int64)
    first = np.full(total, -1, np.int64)
    uniq, idx = np.unique(ids, return_index=True)
    first[uniq] = idx
    if isinstance(bg, dict):  # (a, b) -> pab, in key order
        bg = ([k[0] for k in bg], [k[1] for k in bg], list(bg.values()))
    return SimpleNamespace(
        ids=ids, offsets=np.asarray(offsets, np.int64), n_words=total,
        left=np.asarray(left, np.int32), right=np.asarray(right, np.int32), joined=np.asarray(joined, np.int64),
        bg_left=np.asarray(bg[0], np.int32), bg_right=np.asarray(bg[1], np.int32),
        bg_count=np.asarray(bg[2], np.int64), bg_score=np.asarray(scores, np.float32),
        count=count, first=first, n_joined=int(n_joined))


def pass_loop(ids, offsets, n_words, min_count, threshold):
    """The definition, token by token."""
    ids = [int(v) for v in ids]
    offsets = [int(v) for v in offsets]
    n = len(ids)
    thr = np.float32(threshold)
    cnt = [0] * n_words
    for w in ids:
        cnt[w] += 1
    eligible = [False] * n
    pab = {}
    for s in range(len(offsets) - 1):
        for i in range(offsets[s] + 1, offsets[s + 1]):
            a, b = ids[i - 1], ids[i]
            if cnt[a] >= min_count and cnt[b] >= min_count:
                eligible[i] = True
                pab[(a, b)] = pab.get((a, b), 0) + 1
    score = {k: _score(v, min_count, cnt[k[0]], cnt[k[1]], n) for k, v in pab.items()}
    join = [False] * n
    for i in range(1, n):
        cand = eligible[i] and bool(score[(ids[i - 1], ids[i])] > thr)
        join[i] = cand and not join[i - 1]
    pid, left, right, joined = {}, [], [], []
    for i in range(n):
        if join[i]:
            k = (ids[i - 1], ids[i])
            if k not in pid:
                pid[k] = n_words + len(left)
                left.append(k[0]), right.append(k[1]), joined.append(0)
            joined[pid[k] - n_words] += 1
    out, new_off = [], []
    starts = {}
    for s in range(len(offsets)):
        starts.setdefault(offsets[s], []).append(s)
    new_off = [0] * len(offsets)
    for i in range(n + 1):
        for s in starts.get(i, ()):
            new_off[s] = len(out)
        if i == n or join[i]:
            continue
        out.append(pid[(ids[i], ids[i + 1])] if i + 1 < n and join[i + 1] else ids[i])
    bg = {k: pab[k] for k in sorted(pab)}
    return _result(out, new_off, n_words, left, right, joined, bg, [score[k] for k in bg], sum(join))


def pass_vec(ids, offsets, n_words, min_count, threshold):
    """The same, vectorised: np.unique over the 64-bit keys, the joins as the parity of the candidate run."""
    ids = np.asarray(ids, np.int64)
    offsets = np.asarray(offsets, np.int64)
    n = ids.size
    if n == 0:
        return _result(ids, offsets, n_words, [], [], [], {}, [], 0)
    f = np.float32
    cnt = np.bincount(ids, minlength=n_words).astype(np.int64)
    pos = np.arange(n, dtype=np.int64)
    not_start = np.ones(n, bool)
    not_start[offsets[:-1][offsets[:-1] < offsets[1:]]] = False
    prev = np.concatenate([[0], ids[:-1]])
    eligible = not_start & (cnt[prev] >= min_count) & (cnt[ids] >= min_count)
    key = (prev << 32) | ids
    uk, inv, pab = np.unique(key[eligible], return_inverse=True, return_counts=True)
    ua, ub = uk >> 32, uk & 0xFFFFFFFF
    score = (pab - min_count).astype(f) / cnt[ua].astype(f) / cnt[ub].astype(f) * f(n)
    cand = np.zeros(n, bool)
    cand[eligible] = (score > f(threshold))[inv]
    z = np.maximum.accumulate(np.where(cand, -1, pos))  # the last non-candidate at or before i
    join = cand & (((pos - z) & 1) == 1)
    jpos = pos[join]
    jk, jfirst, jcount = np.unique(key[join], return_index=True, return_counts=True)
    order = np.argsort(jfirst, kind="stable")
    left, right, joined = (jk >> 32)[order], (jk & 0xFFFFFFFF)[order], jcount[order]
    pid_sorted = np.empty(jk.size, np.int64)
    pid_sorted[order] = n_words + np.arange(jk.size)
    keep = ~join
    out = ids[keep].copy()
    outpos = np.cumsum(keep) - keep
    if jpos.size:
        out[outpos[jpos - 1]] = pid_sorted[np.searchsorted(jk, key[jpos])]
    new_off = np.concatenate([outpos, [int(keep.sum())]])[offsets]
    return _result(out, new_off, n_words, left, right, joined, (ua, ub, pab), score, int(join.sum()))


def run_passes(ids, offsets, n_words, passes, fn=pass_vec):
    """[(min_count, threshold), ...] -> the result of every pass."""
    out = []
    for mc, thr in passes:
        r = fn(ids, offsets, n_words, mc, thr)
        out.append(r)
        ids, offsets, n_words = r.ids, r.offsets, r.n_words
    return out


def phrase_words(words, left, right):
    """The word of every id: a phrase is left + "_" + right, composed recursively."""
    words = list(words)
    for a, b in zip(left, right):
        words.append(words[int(a)] + "_" + words[int(b)])
    return words


def to_text(ids, offsets, words) -> str:
    """Single spaces, one newline per sentence."""
    return "".join(" ".join(words[int(t)] for t in ids[offsets[s]:offsets[s + 1]]) + "\n"
                   for s in range(len(offsets) - 1))


def from_text(text):
    """(ids, offsets, words): line_docs' reading, ids in order of first occurrence."""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines = lines[:-1]
    index, ids, off = {}, [], [0]
    for ln in lines:
        for t in ln.split():
            ids.append(index.setdefault(t, len(index)))
        off.append(len(ids))
    return np.array(ids, np.int32), np.array(off, np.int64), list(index)


def map_samples(ids, offsets, index):
    """build_sample of a stream: ids -> index[ids], dropping -1; (ids, offsets, train_words)."""
    index = np.asarray(index, np.int64)
    m = index[ids]
    keep = m >= 0
    kpos = np.concatenate([[0], np.cumsum(keep)])
    return m[keep].astype(np.int32), kpos[offsets].astype(np.int64), int(len(ids))


# ---------------------------------------------------------------------------
# corpus builders (every stream <= ~250 K tokens)
# ---------------------------------------------------------------------------
EXAMPLE = ("new york city is big\ni like new york city\nnew york new york\nyork new\na a a a a\n"
           "city of new york city\nbig city\n")
EXAMPLE_PASSES = ((2, 1.0), (2, 0.5))
EXAMPLE_AFTER = (
    "new_york city is big\ni like new_york city\nnew_york new_york\nyork new\na_a a_a a\n"
    "city of new_york city\nbig city\n",
    "new_york_city is big\ni like new_york_city\nnew_york new_york\nyork new\na_a a_a a\n"
    "city of new_york_city\nbig city\n")


def _ragged_offsets(rng, n_tokens, max_len=40):
    """Sentence lengths 0..max_len with runs of empty sentences, summing to n_tokens."""
    lens = []
    left = n_tokens
    while left > 0:
        if rng.random() < 0.03:
            lens.extend([0] * int(rng.integers(1, 5)))
        k = min(left, int(rng.integers(0, max_len + 1)))
        lens.append(k)
        left -= k
    lens.extend([0, 0])
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _zipf(rng, n, vocab):
    p = 1.0 / np.arange(1, vocab + 1)
    return rng.choice(vocab, size=n, p=p / p.sum())


def _plant(rng, ids, offsets, seqs, times):
    """Write each id sequence `times` times inside sentences long enough to hold it."""
    lens = np.diff(offsets)
    for seq in seqs:
        ok = np.flatnonzero(lens >= len(seq))
        for s in rng.choice(ok, size=times):
            j = int(offsets[s] + rng.integers(0, lens[s] - len(seq) + 1))
            ids[j:j + len(seq)] = seq


@functools.lru_cache(maxsize=None)
def zipf_stream(n=200_000, n_words=70_000, seed=1):
    """Zipf over a shuffled 66,000 ids (so ids pass 2^16) in which one token in five is its
    predecessor's fixed successor (collocations of every strength), ragged sentences, 20 planted
    collocations with ids from 66,000; the ids from 66,040 up never occur."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(66_000)
    succ = rng.permutation(66_000)
    ids = perm[_zipf(rng, n, 66_000)].astype(np.int32)
    for i in np.flatnonzero(rng.random(n) < 0.2)[1:]:
        ids[i] = succ[ids[i - 1]]
    offsets = _ragged_offsets(rng, n)
    _plant(rng, ids, offsets, [(66_000 + 2 * k, 66_001 + 2 * k) for k in range(20)], 40)
    return ids, offsets, n_words


@functools.lru_cache(maxsize=None)
def alternating_stream(variant="even"):
    """One 6,000-token sentence x y x y ... among filler, so that (x, y) and (y, x) both pass threshold 1
    with min_count 2: a candidate run thousands long. "shift": one token later in its sentence (flips the
    parity of every join); "cut": cut in two by a sentence boundary at an odd offset. z z z z z z z in one
    sentence gives z_z z_z z_z z."""
    rng = np.random.default_rng(5)
    x, y, z, w = 0, 1, 2, 3
    filler = (4 + _zipf(rng, 6_000, 500)).astype(np.int32)
    alt = np.tile(np.array([x, y], np.int32), 3_000)
    head = filler[:1_500]
    parts = [head]
    offs = [0] + list(range(30, 1_500, 30)) + [1_500]
    base = 1_500
    if variant == "shift":
        parts.append(np.array([w], np.int32))
        base += 1
    parts.append(alt)
    if variant == "cut":
        offs.append(base + 2_477)
    offs.append(base + 6_000)
    base += 6_000
    seven = np.concatenate([filler[1_500:1_510], np.full(7, z, np.int32), filler[1_510:1_520]])
    parts.append(seven)
    offs.append(base + seven.size)
    base += seven.size
    tail = filler[1_520:]
    parts.append(tail)
    offs.extend(range(base + 25, base + tail.size, 25))
    offs.append(base + tail.size)
    ids = np.concatenate(parts)
    if variant == "shift":
        ids = np.concatenate([ids, np.array([w], np.int32)])  # w occurs twice: eligible with min_count 2
        offs.append(ids.size)
    return ids, np.array(offs, np.int64), 504


BOUNDARY_MIN_COUNT = 3
BOUNDARY_TEXT = (
    # sentences of length 0, 1 and 2
    "\nsolo\nu v\n\n\n"
    # (p, q) only ever across a sentence boundary: never counted
    "k p\nq k\nk p\nq k\nk p\nq k\n"
    # r occurs min_count - 1 times: (r, s) and (s, r) are ineligible, absent from the bigram list
    "s r s\ns r s\ns s\n"
    # t occurs exactly min_count times, always before s: eligible
    "t s\nt s\nt s\n"
    # (u, v) occurs exactly min_count times: score 0, not above threshold 0
    "u v\nu v\nsolo\n"
    # (g, h) joins; a sentence of one token after it
    "g h g h\ng h g h\ng h\nk\n")


@functools.lru_cache(maxsize=None)
def boundary_stream():
    return from_text(BOUNDARY_TEXT)


@functools.lru_cache(maxsize=None)
def multipass_stream():
    """Zipf filler over 2,000 words with planted three-, four- and five-word collocations: a second pass
    makes (a_b, c) and (d_e, f_g), a third (h_i_j_k, l). Word 2,001 ("b") only ever follows "a": absorbed
    by pass 1, count 0."""
    rng = np.random.default_rng(9)
    n = 60_000
    ids = _zipf(rng, n, 2_000).astype(np.int32)
    offsets = _ragged_offsets(rng, n)
    _plant(rng, ids, offsets, [(2_000, 2_001, 2_002), (2_003, 2_004, 2_005, 2_006),
                                 (2_010, 2_011, 2_012, 2_013, 2_014)], 60)
    # every b follows an a in its sentence: repair the plants a later plant cut
    not_start = np.ones(n, bool)
    not_start[offsets[:-1][offsets[:-1] < offsets[1:]]] = False
    for i in np.flatnonzero(ids == 2_001):
        if not (not_start[i] and ids[i - 1] == 2_000):
            ids[i] = 7
    return ids, offsets, 2_020


MULTIPASS = ((5, 100.0), (5, 50.0), (5, 20.0))


def plant_text(text, seqs, times, seed):
    """Insert each word sequence `times` times into random space-separated lines of a corpus text."""
    rng = np.random.default_rng(seed)
    lines = text.split("\n")
    ok = [k for k, ln in enumerate(lines) if ln.strip() and "\t" not in ln]
    for seq in seqs:
        for k in rng.choice(ok, size=times):
            toks = lines[k].split(" ")
            j = int(rng.integers(0, len(toks) + 1))
            lines[k] = " ".join(toks[:j] + list(seq) + toks[j:])
    return "\n".join(lines)
