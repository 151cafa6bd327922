"""Word2Vec::most_similar through the C bridge (w2v_model_most_similar) and
evaluate.analogy_accuracy(index=...) on the GPU, against the float64
reference and checker of tests/nn_ref.py."""
import numpy as np
import pytest

from tests import nn_ref as R
from tests.corpus import zipf_sentences
from word2vec_amd.evaluate import analogy_accuracy
from word2vec_amd.model import Word2Vec
from word2vec_amd.nn import NearestIndex

pytestmark = pytest.mark.gpu
DIM = 32


def _model():
    return Word2Vec(iter=2, window=5, min_count=2, table_size=50_000, word_dim=DIM, negative=5,
                    subsample_threshold=1e-3, init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True, train_method="ns",
                    model="sg")


@pytest.fixture(scope="module")
def trained():
    sents = zipf_sentences(10, 150, 300, seed=12, ragged=True)  # the tiny corpus of tests/test_gpu_class.py
    w = _model()
    w.seed(5)
    w.build_vocab(sents)
    w.init_weights()
    w.train(sents)
    return w


def _check_against(w, M, queries, k=8, restrict=0):
    for ids, weights in queries:
        got_ids, got_sc = w.most_similar_ids(ids, weights, k=k, restrict=restrict)
        q = R.queries_from_rows(M, np.array([ids]), np.array([weights]))
        R.check(R.cosines(M, q), got_ids[None, :], got_sc[None, :], DIM, exclude=np.array([ids]), restrict=restrict)


QUERIES = [([3], [1.0]), ([5, 2, 9], [1.0, -1.0, 1.0]), ([1, 4, 6, 8], [1.0, 1.0, -1.0, -1.0])]


def test_bridge_most_similar_matches_reference(trained):
    W = trained.matrix(0)
    assert W.shape[0] == trained.V > 40
    _check_against(trained, W, QUERIES)
    _check_against(trained, W, QUERIES, k=8, restrict=20)
    with pytest.raises(RuntimeError, match="terms"):
        trained.most_similar_ids(list(range(9)), k=3)
    with pytest.raises(RuntimeError, match="k must be"):
        trained.most_similar_ids([1], k=65)
    _check_against(trained, W, QUERIES[:1])  # still usable


def test_bridge_answer_follows_set_matrix(trained):
    W = trained.matrix(0)
    before = trained.most_similar_ids([3], k=8)
    M = np.random.default_rng(21).standard_normal(W.shape).astype(np.float32)
    trained.set_matrix(0, M)
    try:
        after = trained.most_similar_ids([3], k=8)
        assert not np.array_equal(before[0], after[0])
        _check_against(trained, M, QUERIES)
    finally:
        trained.set_matrix(0, W)
    _check_against(trained, W, QUERIES)


def test_bridge_query_after_load_needs_no_training(trained, tmp_path):
    trained.save_word2vec(tmp_path / "vec.txt", 0, False)
    trained.save_vocab(tmp_path / "vocab.txt")
    w = _model()
    w.read_vocab(tmp_path / "vocab.txt")
    w.load_word2vec(tmp_path / "vec.txt", False)
    M = w.matrix(0)
    assert M.shape == trained.matrix(0).shape and np.abs(M).max() > 0
    _check_against(w, M, QUERIES)


def test_class_most_similar_and_analogy_by_word(trained):
    """Word2Vec::most_similar / ::analogy (string lookup, signs, ids back to words) against the by-id bridge."""
    words, _ = trained.vocab()
    W = trained.matrix(0)
    pos, neg = [words[1], words[4]], [words[6], words[8]]
    got = trained.most_similar(pos, neg, topn=8)
    ids, sc = trained.most_similar_ids([1, 4, 6, 8], [1.0, 1.0, -1.0, -1.0], k=8)
    assert [w for w, _ in got] == [words[i] for i in ids]
    assert np.array_equal(np.array([s for _, s in got], np.float32), sc)
    assert not {w for w, _ in got} & set(pos + neg)
    q = R.queries_from_rows(W, np.array([[1, 4, 6, 8]]), np.array([[1.0, 1.0, -1.0, -1.0]]))
    R.check(R.cosines(W, q), ids[None, :], sc[None, :], DIM, exclude=np.array([[1, 4, 6, 8]]))
    # analogy(a, b, c) = most_similar({b, c}, {a}), default topn 1; restrict_vocab keeps the answer among the first rows
    a, b, c = words[2], words[5], words[9]
    (word, score), = trained.analogy(a, b, c)
    ids, sc = trained.most_similar_ids([5, 9, 2], [1.0, 1.0, -1.0], k=1)
    assert word == words[ids[0]] and np.float32(score) == sc[0]
    top = trained.analogy(a, b, c, topn=5, restrict_vocab=12)
    assert len(top) == 5 and all(words.index(w) < 12 and w not in (a, b, c) for w, _ in top)
    assert [s for _, s in top] == sorted((s for _, s in top), reverse=True)
    with pytest.raises(RuntimeError, match="no-such-word"):
        trained.most_similar([words[1], "no-such-word"])
    with pytest.raises(RuntimeError, match="terms"):
        trained.most_similar(words[:9])
    assert trained.most_similar([words[3]], topn=3) == trained.most_similar([words[3]], [], 3)


def _planted(rows=6, cols=4, filler=300, d=48, seed=31):
    """Entities e(r, c) = R_r + C_c + noise among filler words; questions e(r1, c1) : e(r1, c2) :: e(r2, c1) : e(r2, c2)."""
    rng = np.random.default_rng(seed)
    Rr = rng.standard_normal((rows, d))
    Cc = rng.standard_normal((cols, d))
    ent = (Rr[:, None, :] + Cc[None, :, :] + 0.15 * rng.standard_normal((rows, cols, d))).reshape(rows * cols, d)
    vecs = np.concatenate([rng.standard_normal((filler, d)), ent]).astype(np.float32)
    words = [f"f{i}" for i in range(filler)] + [f"e{r}_{c}" for r in range(rows) for c in range(cols)]
    qs = []
    for r1 in range(rows):
        for r2 in range(rows):
            for c1 in range(cols):
                for c2 in range(cols):
                    if r1 != r2 and c1 != c2:
                        qs.append((f"e{r1}_{c1}", f"e{r1}_{c2}", f"e{r2}_{c1}", f"e{r2}_{c2}"))
    qs.append(("f0", "f1", "f2", "nope"))  # skipped: a word outside the vocabulary
    return words, vecs, qs


@pytest.mark.parametrize("restrict", [None, 320])
def test_analogy_accuracy_with_index_equals_numpy(restrict):
    words, vecs, qs = _planted()
    idx = {w: i for i, w in enumerate(words)}
    known = [q for q in qs if all(x in idx for x in q) and (restrict is None or all(idx[x] < restrict for x in q))]
    ids = np.array([[idx[b], idx[a], idx[c]] for a, b, c, _ in known])
    cos = R.cosines(vecs, R.queries_from_rows(vecs, ids, (1.0, -1.0, 1.0)))
    # every question's top-1 gap in the reference exceeds 2 tol: the two paths must agree question by question
    assert R.gaps_clear(cos, 1, vecs.shape[1], ids, restrict or 0).all()
    want = analogy_accuracy(words, vecs, qs, restrict=restrict)
    assert want["answered"] == len(known) and 0 < want["correct"]
    with NearestIndex.from_matrix(vecs) as index:
        got = analogy_accuracy(words, vecs, qs, restrict=restrict, index=index)
    assert got == want
