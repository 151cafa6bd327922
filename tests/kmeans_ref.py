"""Float64 reference and checker for the word classes (word2vec_amd/nn.py
NearestIndex.assign / centroids / classes over include/w2v_dev.h
w2v_nn_assign / _centroids / _classes). CPU only.

The algorithm (spherical k-means, word2vec's -classes made well-defined):
  start    class[r] = r mod K; a row with a non-finite element is a member of
           nothing (-1), now and in every update.
  update   centroid[c] = the sum of the raw rows of c's members, scaled by
           x / max(|x|, 1e-12).
  assign   class[r] = the valid class of highest cosine with row r, equal
           scores to the lowest id. A centroid is valid when every element is
           finite and one is non-zero (an empty class, members that cancel and
           a NaN centroid take no rows). A non-finite row, and every row when
           no centroid is valid, gets -1 / -inf. A zero row scores 0 everywhere.
  stop     after `iterations` iterations, or after one that moved no row.

Tolerance for scores: nn_ref.tol(d) = (d + 16) * 2^-23, by the same derivation
(an f32 dot of two unit vectors errs by at most d * 2^-24, the two
normalisations add a few ulps each, a factor of 2 on top).

check_assign asks, per row: the score is within tol of the float64 cosine of
the chosen class; no other valid class has a float64 cosine above score + tol;
-1 / -inf appear exactly for non-finite rows and when no centroid is valid; and
where the reference's top-two gap exceeds 2 tol the class is the reference's.
"""
from __future__ import annotations

import numpy as np

from tests.nn_ref import tol, unit64


def finite_rows(x) -> np.ndarray:
    return np.isfinite(np.asarray(x, np.float64)).all(axis=1)


def valid_centroids(cen) -> np.ndarray:
    c = np.asarray(cen, np.float64)
    return np.isfinite(c).all(axis=1) & (c != 0).any(axis=1)


def start(x, K: int) -> np.ndarray:
    cls = (np.arange(len(x)) % K).astype(np.int32)
    cls[~finite_rows(x)] = -1
    return cls


def update(x, cls, K: int):
    """(unit centroids float64 [K, d], counts int64 [K], raw sums float64 [K, d]) of the classes; non-finite
    rows and class -1 are members of nothing."""
    x = np.asarray(x, np.float64)
    cls = np.where(finite_rows(x), np.asarray(cls, np.int64), -1)
    sums = np.zeros((K, x.shape[1]), np.float64)
    member = cls >= 0
    np.add.at(sums, cls[member], x[member])
    counts = np.bincount(cls[member], minlength=K).astype(np.int64)
    return unit64(sums), counts, sums


def cosines(x, cen) -> np.ndarray:
    """V x K float64 cosines; the columns of invalid centroids and the rows of non-finite rows are -inf."""
    x = np.asarray(x, np.float64)
    c = np.asarray(cen, np.float64)
    fr, vc = finite_rows(x), valid_centroids(c)
    cos = np.full((x.shape[0], c.shape[0]), -np.inf)
    if fr.any() and vc.any():
        cos[np.ix_(fr, vc)] = unit64(x[fr]) @ unit64(c[vc]).T
    return cos


def assign_from_cos(cos):
    """(classes int32, scores float64): the first maximum of each row (lowest id on ties), -1 / -inf where none."""
    best = cos.argmax(axis=1).astype(np.int32)
    sc = cos[np.arange(cos.shape[0]), best]
    best[np.isneginf(sc)] = -1
    return best, sc


def assign(x, cen):
    return assign_from_cos(cosines(x, cen))


def top_two_gap(cos) -> np.ndarray:
    """Per row: best minus second-best cosine among the valid classes (+inf with fewer than two)."""
    if cos.shape[1] < 2:
        return np.full(cos.shape[0], np.inf)
    part = -np.partition(-cos, 1, axis=1)[:, :2]
    with np.errstate(invalid="ignore"):
        gap = part[:, 0] - part[:, 1]
    gap[np.isneginf(part[:, 1])] = np.inf
    return gap


def run(x, K: int, iterations: int = 10) -> dict:
    """The whole run. Besides the outputs of w2v_nn_classes: `gaps`, per iteration the smallest top-two gap over
    the assigned rows, and `clear`, the share of them whose gap exceeds 2 tol(d)."""
    x = np.asarray(x, np.float64)
    d = x.shape[1]
    cls = start(x, K)
    moved, gaps, clear = [], [], []
    cen = sc = None
    for _ in range(iterations):
        cen, _, _ = update(x, cls, K)
        cos = cosines(x, cen)
        new, sc = assign_from_cos(cos)
        g = top_two_gap(cos)[new >= 0]
        gaps.append(float(g.min()) if g.size else np.inf)
        clear.append(float((g > 2 * tol(d)).mean()) if g.size else 1.0)
        moved.append(int((new != cls).sum()))
        cls = new
        if moved[-1] == 0:
            break
    counts = np.bincount(cls[cls >= 0], minlength=K).astype(np.int64)
    return {"classes": cls, "scores": sc, "centroids": cen, "counts": counts, "moved": np.array(moved, np.int64),
            "iterations": len(moved), "gaps": gaps, "clear": clear}


def check_assign(x, cen, classes, scores, d: int) -> np.ndarray:
    """Raise AssertionError unless (classes, scores) is a correct assignment of the rows x to the centroids cen
    (the module docstring). Returns the rows whose reference gap exceeds 2 tol (where equality was asked)."""
    classes = np.asarray(classes)
    scores = np.asarray(scores, np.float64)
    V = len(x)
    assert classes.shape == (V,) and scores.shape == (V,), (classes.shape, scores.shape)
    t = tol(d)
    cos = cosines(x, cen)
    ref, ref_sc = assign_from_cos(cos)
    none = ref < 0
    assert np.array_equal(classes < 0, none), "-1 must mark exactly the non-finite rows / the no-valid-centroid case"
    assert np.all(classes[none] == -1) and np.all(np.isneginf(scores[none])), "rows without a class need -1 / -inf"
    ok = ~none
    got = classes[ok].astype(np.int64)
    assert np.all(got < cos.shape[1]), "class id out of range"
    mine = cos[ok, got]
    assert np.all(np.isfinite(mine)), "a row was given to an invalid centroid"
    assert np.all(np.isfinite(scores[ok])), "non-finite score of an assigned row"
    err = np.abs(scores[ok] - mine)
    assert np.all(err <= t), f"score off by {err.max():.3g} > tol {t:.3g}"
    over = ref_sc[ok] - (scores[ok] + t)
    assert np.all(over <= 0), f"another class scores {over.max():.3g} above the returned score + tol"
    clear = ok & (top_two_gap(cos) > 2 * t)
    assert np.array_equal(classes[clear], ref[clear]), "class differs from the reference where the gap is clear"
    return clear


def planted(V, d, K, noise, p, seed):
    """Rows around K planted directions: a share p starts in its own class (r mod K), the rest anywhere."""
    rng = np.random.default_rng(seed)
    cen = unit64(rng.standard_normal((K, d)))
    g = np.where(rng.random(V) < p, np.arange(V) % K, rng.integers(0, K, V))
    x = cen[g] * rng.uniform(0.5, 4.0, (V, 1)) + noise * rng.standard_normal((V, d)) / np.sqrt(d)
    return x.astype(np.float32), g


PLANTED_SHAPES = [dict(V=1031, d=48, K=17, noise=0.9, p=0.35, seed=1), dict(V=2000, d=300, K=40, noise=1.2, p=0.3, seed=1)]


def random_rows(V, d, seed):
    """default_rng(seed).standard_normal rows with row 7 an exact copy of row 3 (tests/test_gpu_nn.py's)."""
    rows = np.random.default_rng(seed).standard_normal((V, d)).astype(np.float32)
    rows[7] = rows[3]
    return rows


def random_centroids(K, d, seed):
    """standard_normal x uniform(0.01, 30) per centroid: any length."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((K, d)) * rng.uniform(0.01, 30, (K, 1))).astype(np.float32)
