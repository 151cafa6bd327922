"""Float64 reference and checker for the nearest-neighbour queries
(word2vec_amd/nn.py, include/w2v_dev.h w2v_nn_*). CPU only.

Tolerance: tol(d) = (d + 16) * 2^-23. An f32 dot of two unit vectors errs by
at most d * 2^-24 * sum |q_i e_i| <= d * 2^-24; the two normalisations (row and
query, each a sum of squares, a square root, a reciprocal and a product) add a
few ulps each; a factor of 2 on top. 1.4e-5 at d 100, 3.8e-5 at d 300.

The checker asks, per query:
  1. every returned score is within tol of the float64 cosine of its id;
  2. scores are non-increasing, equal scores come in ascending id order, and
     -1 / -inf fill exactly the slots past the candidate count;
  3. no id is repeated, excluded, or >= restrict;
  4. completeness: every candidate not returned has a float64 cosine <= the
     returned k-th score + tol.
Where all reference gaps of a query's top k + 1 exceed 2 tol (gaps_clear),
1, 2 and 4 force the reference list itself, and the callers assert equality.
"""
from __future__ import annotations

import numpy as np


def tol(d: int) -> float:
    return (d + 16) * 2.0 ** -23


def unit64(m) -> np.ndarray:
    """Rows scaled to unit length in float64 (evaluate.normalize's 1e-12 rule)."""
    v = np.asarray(m, dtype=np.float64)
    if v.ndim == 1:
        v = v[None, :]
    n = np.sqrt((v * v).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore"):
        return v / np.fmax(n, 1e-12)


def queries_from_rows(rows, ids, weights) -> np.ndarray:
    """The by-row form's query vectors in float64: sum_t w_t unit(row[id_t]), id < 0 skipped."""
    E = unit64(rows)
    ids = np.asarray(ids, np.int64)
    w = np.broadcast_to(np.asarray(weights, np.float64), ids.shape)
    q = np.zeros((ids.shape[0], E.shape[1]), np.float64)
    for t in range(ids.shape[1]):
        ok = ids[:, t] >= 0
        q[ok] += w[ok, t][:, None] * E[ids[ok, t]]
    return q


def cosines(rows, q) -> np.ndarray:
    """nq x V float64 cosines of the query vectors q against the rows."""
    with np.errstate(invalid="ignore"):
        return unit64(q) @ unit64(rows).T


def _candidates(cos_q, exclude_q, restrict: int) -> np.ndarray:
    """Boolean mask of the rows a query may return."""
    V = cos_q.shape[0]
    ok = np.isfinite(cos_q)
    if restrict:
        ok[restrict:] = False
    if exclude_q is not None:
        ex = np.asarray(exclude_q, np.int64)
        ex = ex[(ex >= 0) & (ex < V)]
        ok[ex] = False
    return ok


def reference_topk(cos, k: int, exclude=None, restrict: int = 0):
    """(ids int32 [nq, k], scores float64 [nq, k]) by score descending, then id ascending."""
    nq = cos.shape[0]
    ids = np.full((nq, k), -1, np.int32)
    sc = np.full((nq, k), -np.inf, np.float64)
    for i in range(nq):
        ok = _candidates(cos[i], None if exclude is None else exclude[i], restrict)
        cand = np.flatnonzero(ok)
        order = cand[np.lexsort((cand, -cos[i, cand]))][:k]
        ids[i, :order.size] = order
        sc[i, :order.size] = cos[i, order]
    return ids, sc


def gaps_clear(cos, k: int, d: int, exclude=None, restrict: int = 0) -> np.ndarray:
    """Per query: every gap between consecutive reference scores of its top k + 1 exceeds 2 tol(d)."""
    _, sc = reference_topk(cos, k + 1, exclude, restrict)
    out = np.zeros(cos.shape[0], bool)
    for i in range(cos.shape[0]):
        s = sc[i][np.isfinite(sc[i])]
        out[i] = bool(np.all(-np.diff(s) > 2 * tol(d)))
    return out


def check(cos, ids, scores, d: int, exclude=None, restrict: int = 0) -> None:
    """Raise AssertionError unless (ids, scores) is a correct answer for every query (the module docstring)."""
    ids = np.asarray(ids)
    scores = np.asarray(scores)
    assert ids.shape == scores.shape and ids.ndim == 2 and ids.shape[0] == cos.shape[0], (ids.shape, scores.shape)
    nq, k = ids.shape
    t = tol(d)
    for i in range(nq):
        ok = _candidates(cos[i], None if exclude is None else exclude[i], restrict)
        n_cand = int(ok.sum())
        n = min(k, n_cand)
        gi, gs = ids[i], scores[i].astype(np.float64)
        # 2 (fill): exactly the slots past the candidate count hold -1 / -inf
        assert np.all(gi[n:] == -1) and np.all(np.isneginf(gs[n:])), f"query {i}: slots past {n} are not -1 / -inf"
        assert np.all(gi[:n] >= 0) and np.all(np.isfinite(gs[:n])), f"query {i}: a filler among the first {n} slots"
        got = gi[:n].astype(np.int64)
        # 3: no id repeated, excluded, or >= restrict (or not a candidate at all)
        assert np.unique(got).size == n, f"query {i}: repeated id"
        assert np.all(got < cos.shape[1]) and np.all(ok[got]), f"query {i}: returned a row that is not a candidate"
        # 1: scores against the float64 cosine of the returned id
        err = np.abs(gs[:n] - cos[i, got])
        assert np.all(err <= t), f"query {i}: score off by {err.max():.3g} > tol {t:.3g}"
        # 2 (order): non-increasing, ties by ascending id
        ds = np.diff(gs[:n])
        assert np.all(ds <= 0), f"query {i}: scores increase"
        tie = ds == 0
        assert np.all(np.diff(got)[tie] > 0), f"query {i}: equal scores not in ascending id order"
        # 4: completeness
        if n == k and n_cand > k:
            rest = ok.copy()
            rest[got] = False
            worst = cos[i, rest].max()
            assert worst <= gs[k - 1] + t, f"query {i}: a missing candidate scores {worst:.9g} > k-th {gs[k - 1]:.9g} + tol"
