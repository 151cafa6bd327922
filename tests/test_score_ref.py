"""tests/score_ref.py, the float64 definition the GPU scores are held to, checked
on the CPU: hand-computed examples, loop against vectorised form, the Philox
draws against tests/refpy, HS normalisation, NS set semantics, the CBOW mean."""
import math

import numpy as np
import pytest

from tests import refpy
from tests import score_ref as R
from tests.corpus import zipf_sentences
from tests.harness import oracle_run


def ls(z):  # log sigma, the textbook form (fine at these small |z|)
    return math.log(1.0 / (1.0 + math.exp(-z)))


W3 = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
C3 = np.array([[0.5, -1.0], [2.0, 0.25], [-1.0, 1.0]])
S3 = np.array([[1.0, 2.0], [-0.5, 0.5]])
IDS3, OFF3 = np.array([0, 1, 2]), np.array([0, 3])
BOUNDS3 = np.array([0, 2, 3, 4])  # table of 4: word 0 twice, 1, 2


def draws3(i, slot, negative, key):
    return [int(np.searchsorted(BOUNDS3, R.table_pos(i, 0, slot, k, key, 4), "right")) - 1 for k in range(negative)]


def ns_sum(M, x, pos, draws):
    t = [ls(float(M[pos] @ x))]
    for u in dict.fromkeys(draws):  # distinct, in draw order
        if u != pos:
            t.append(ls(-float(M[u] @ x)))
    return t


@pytest.mark.parametrize("form", [R.score_loop, R.score_vec])
def test_hand_computed_v3_d2(form):
    hf = R.chain_tree(3)
    assert [list(hf[1][hf[2][w]:hf[2][w + 1]]) for w in range(3)] == [[0], [0, 1], [0, 1]]
    assert [list(hf[0][hf[2][w]:hf[2][w + 1]]) for w in range(3)] == [[1], [0, 1], [0, 0]]
    # skip-gram HS, window 1
    want = [ls(1), ls(0.5), ls(-2), ls(2), ls(0.5), ls(3), ls(0)]
    r = form(W3, None, S3, IDS3, OFF3, window=1, hs=True, huffman=hf)
    assert r["targets"].tolist() == [7] and r["ll"][0] == pytest.approx(sum(want), abs=1e-14)
    assert r["summary"] == dict(sentences=1, words=3, centers=3, contexts=4, targets=7, draws=0, nonfinite=0,
                                ll=r["ll"][0])
    # CBOW HS, sum
    want = [ls(-2.5), ls(-0.5), ls(-0.25), ls(2.5), ls(-0.875)]
    r = form(None, C3, S3, IDS3, OFF3, window=1, hs=True, cbow=True, huffman=hf)
    assert r["targets"].tolist() == [5] and r["ll"][0] == pytest.approx(sum(want), abs=1e-14)
    assert r["summary"]["contexts"] == 4 and r["summary"]["centers"] == 3
    # skip-gram NS, negative 3, key 9: slot = the context's ordinal
    key, want = 9, []
    for i, ctx in ((0, [1]), (1, [0, 2]), (2, [1])):
        for t, j in enumerate(ctx):
            want += ns_sum(C3, W3[i], j, draws3(i, t, 3, key))
    r = form(W3, C3, None, IDS3, OFF3, window=1, negative=3, bounds=BOUNDS3, key=key)
    assert r["targets"].tolist() == [len(want)] and r["ll"][0] == pytest.approx(sum(want), abs=1e-14)
    assert r["summary"]["draws"] == 12 and r["summary"]["contexts"] == 4
    # CBOW NS, mean: slot 0, target matrix W, positive the center
    want = []
    for i, ctx in ((0, [1]), (1, [0, 2]), (2, [1])):
        h = sum(C3[j] for j in ctx) / len(ctx)
        want += ns_sum(W3, h, i, draws3(i, 0, 3, key))
    r = form(W3, C3, None, IDS3, OFF3, window=1, negative=3, cbow=True, cbow_mean=True, bounds=BOUNDS3, key=key)
    assert r["targets"].tolist() == [len(want)] and r["ll"][0] == pytest.approx(sum(want), abs=1e-14)
    assert r["summary"]["draws"] == 9


def test_philox_vec_is_refpy_philox():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 1 << 32, (64, 4), dtype=np.uint64)
    key = int(rng.integers(0, 1 << 63))
    got = np.stack(R.philox_vec(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key), 1)
    for c, g in zip(ctr, got):
        assert tuple(int(x) for x in g) == refpy.philox4x32_10(tuple(int(x) for x in c), (key & R.M32, key >> 32))
    for c, k, out in refpy.PHILOX_KAT:
        got = R.philox_vec(*[np.uint64(x) for x in c], k[0] | (k[1] << 32))
        assert tuple(int(x) for x in got) == out
    for n in (1, 7, 1000, (1 << 32) - 1):
        pos = R.table_pos_vec(got[0][None], got[1][None], n)
        assert int(pos[0]) == (((int(got[1]) << 32) | int(got[0])) * n) >> 64


def _random_case(seed, V=9, d=5, cbow=False):
    rng = np.random.default_rng(seed)
    lens = [0, 1, 2, 7, 12]
    ids = rng.integers(0, V, sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)])
    W, C, S = rng.normal(size=(V, d)), rng.normal(size=(V, d)), rng.normal(size=(V - 1, d))
    return W, C, S, ids, off


@pytest.mark.parametrize("mode", ["sg_hs", "cbow_hs", "sg_ns", "cbow_ns"])
def test_loop_equals_vectorised(mode):
    W, C, S, ids, off = _random_case(3)
    kw = dict(window=3, hs=mode.endswith("hs"), cbow=mode.startswith("cbow"), cbow_mean=True, key=0x1234567890ABCDEF)
    if kw["hs"]:
        kw["huffman"] = R.chain_tree(9)
    else:
        kw.update(negative=4, bounds=np.array([0, 5, 9, 12, 14, 16, 17, 18, 19, 20]))
    a, b = R.score_loop(W, C, S, ids, off, **kw), R.score_vec(W, C, S, ids, off, **kw)
    assert a["targets"].tolist() == b["targets"].tolist()
    assert a["targets"][0] == a["targets"][1] == 0 and a["ll"][0] == a["ll"][1] == 0.0
    np.testing.assert_allclose(a["ll"], b["ll"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(a["bound"], b["bound"], rtol=1e-9)
    for k in ("sentences", "words", "centers", "contexts", "targets", "draws", "nonfinite"):
        assert a["summary"][k] == b["summary"][k], k
    assert (a["collisions"], a["duplicates"]) == (b["collisions"], b["duplicates"])
    assert a["min_z"] == pytest.approx(b["min_z"], rel=1e-12)


def _total_probability(huffman, V, d, seed):
    rng = np.random.default_rng(seed)
    S, h = rng.normal(size=(V - 1, d)), rng.normal(size=d) * 2
    total = 0.0
    for w in range(V):
        pts, sg = R._path(huffman, w)
        total += math.exp(float(np.sum(R.logsig((S[pts] @ h) * sg))))
    return total


def test_hs_terms_are_a_normalised_distribution():
    """sum over words of exp(log p(w | h)) = 1: the path terms are a distribution over the vocabulary."""
    o = oracle_run(zipf_sentences(40, 30, 50, seed=5), "sg_hs", dim=4, min_count=1, train=False)
    assert 30 <= o.V <= 50
    for seed in range(3):
        assert _total_probability(o.huffman(), o.V, 6, seed) == pytest.approx(1.0, abs=1e-12)
        assert _total_probability(R.chain_tree(50), 50, 6, seed) == pytest.approx(1.0, abs=1e-12)
    _, _, coff = R.chain_tree(70)
    assert sorted(set(np.diff(coff).tolist())) == list(range(1, 70))


def test_ns_set_semantics():
    """A draw equal to the positive, and a repeated draw, add no term."""
    W, C = np.array([[0.3, -0.2], [1.5, 0.5]]), np.array([[0.7, 0.1], [-0.4, 0.9]])
    bounds = np.array([0, 2, 3])  # two words: five draws must repeat, and (this key) hit the positive
    ids, off = np.array([0, 1]), np.array([0, 2])
    for form in (R.score_loop, R.score_vec):
        r = form(W, C, None, ids, off, window=2, negative=5, bounds=bounds, key=1)
        assert r["collisions"] >= 1 and r["duplicates"] >= 1
        want, n = 0.0, 0
        for i, j in ((0, 1), (1, 0)):
            dr = [int(np.searchsorted(bounds, R.table_pos(i, 0, 0, k, 1, 3), "right")) - 1 for k in range(5)]
            other = 1 - ids[j]
            want += ls(float(C[ids[j]] @ W[ids[i]])) + (ls(-float(C[other] @ W[ids[i]])) if other in dr else 0.0)
            n += 1 + (other in dr)
        assert r["targets"][0] == n and r["ll"][0] == pytest.approx(want, abs=1e-14)
        assert r["summary"]["draws"] == 10


def test_cbow_mean_divides_by_positions():
    """[0, 1, 1]: center 0 has two context positions and one distinct id: h = C[1] / 2."""
    hf = R.chain_tree(3)
    ids, off = np.array([0, 1, 1]), np.array([0, 3])
    for form in (R.score_loop, R.score_vec):
        r = form(None, C3, S3, ids, off, window=2, hs=True, cbow=True, cbow_mean=True, huffman=hf)
        h0 = C3[1] / 2
        h1 = (C3[0] + C3[1]) / 2
        want = (ls(-float(S3[0] @ h0))
                + 2 * (ls(float(S3[0] @ h1)) + ls(-float(S3[1] @ h1))))
        assert r["ll"][0] == pytest.approx(want, abs=1e-14)
        assert r["summary"]["contexts"] == 1 + 2 + 2 and r["targets"][0] == 5
        # e = distinct ids + 1 enters the bound
        nv = 1
        t0 = abs(ls(-float(S3[0] @ h0)))
        assert r["bound"][0] > (nv + 14 + 2) * R.EPS * t0
