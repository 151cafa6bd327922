"""Word classes through the upper layers: Word2Vec::word_classes over the C
bridge (w2v_model_word_classes) and the CLI's -classes, against
NearestIndex.classes (tests/test_gpu_classes.py checks that one against the
float64 reference)."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests.corpus import zipf_sentences
from word2vec_amd.model import Word2Vec
from word2vec_amd.nn import NearestIndex

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "word2vec_amd" / "bin" / "word2vec"
DIM = 32


@pytest.fixture(scope="module")
def trained():
    """The tiny trained model of tests/test_gpu_nn_class.py (skip-gram with negative sampling: it has C)."""
    sents = zipf_sentences(10, 150, 300, seed=12, ragged=True)
    w = Word2Vec(iter=2, window=5, min_count=2, table_size=50_000, word_dim=DIM, negative=5, subsample_threshold=1e-3,
                 init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True, train_method="ns", model="sg")
    w.seed(5)
    w.build_vocab(sents)
    w.init_weights()
    w.train(sents)
    return w


def _direct(M, k, iterations=10):
    with NearestIndex.from_matrix(M) as index:
        return index.classes(k, iterations)["classes"]


def test_bridge_word_classes_equal_the_index(trained):
    W = trained.matrix(0)
    assert W.shape[0] == trained.V > 40
    got = trained.word_classes(7)
    assert got.dtype == np.int32 and np.array_equal(got, _direct(W, 7))
    assert got.min() >= 0 and got.max() < 7 and np.unique(got).size > 1
    assert np.array_equal(trained.word_classes(7, iterations=1), _direct(W, 7, 1))
    trained.most_similar_ids([3], k=4)  # the cached index serves both
    assert np.array_equal(trained.word_classes(5), _direct(W, 5))
    with pytest.raises(RuntimeError, match="n_classes"):
        trained.word_classes(0)
    with pytest.raises(RuntimeError, match="iterations"):
        trained.word_classes(7, iterations=0)
    with pytest.raises(RuntimeError, match="selector"):
        trained.word_classes(7, which=5)
    assert np.array_equal(trained.word_classes(7), got)  # still usable


def test_bridge_word_classes_follow_set_matrix_and_take_c(trained):
    W = trained.matrix(0)
    before = trained.word_classes(7)
    M = np.random.default_rng(21).standard_normal(W.shape).astype(np.float32)
    trained.set_matrix(0, M)
    try:
        after = trained.word_classes(7)
        assert np.array_equal(after, _direct(M, 7)) and not np.array_equal(after, before)
    finally:
        trained.set_matrix(0, W)
    assert np.array_equal(trained.word_classes(7), before)
    Cm = trained.matrix(1)
    assert Cm.shape == W.shape and np.abs(Cm).max() > 0
    assert np.array_equal(trained.word_classes(6, which=1), _direct(Cm, 6))


def _run(args):
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_classes(tmp_path):
    sents = zipf_sentences(50, 1000, 2000, seed=16)  # the corpus of tests/test_gpu_class.py::test_cli_end_to_end
    corpus = tmp_path / "corpus.txt"
    corpus.write_text(" ".join(" ".join(s) for s in sents))
    out, vocab = tmp_path / "classes.txt", tmp_path / "vocab.txt"
    base = ["-train", corpus, "-size", 32, "-negative", 5, "-iter", 1]
    r = _run(base + ["-output", out, "-classes", 9, "-save-vocab", vocab])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in out.read_text().splitlines()]
    words = [l.split()[2] for l in vocab.read_text().splitlines()]
    assert len(lines) == len(words) > 9 and all(len(l) == 2 for l in lines)
    assert [l[0] for l in lines] == words
    ids = [int(l[1]) for l in lines]
    assert all(0 <= i < 9 for i in ids) and len(set(ids)) > 1
    vec = tmp_path / "vec.txt"
    r = _run(base + ["-output", vec, "-classes", 0])
    assert r.returncode == 0, r.stdout + r.stderr
    head = vec.read_text().splitlines()
    assert head[0].split() == [str(len(words)), "32"] and len(head[1].split()) == 33
    r = _run(base + ["-output", tmp_path / "no.txt", "-classes", -3])
    assert r.returncode == 1 and "-classes" in r.stdout and not (tmp_path / "no.txt").exists()
