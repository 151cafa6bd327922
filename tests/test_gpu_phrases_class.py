"""Word2Vec::phrase (include/Word2Vec.h) through the Python model: a model with
phrase_thresholds on a corpus file equals a plain model on the rewritten corpus
written as text by tests/phrase_ref.py — vocabulary (words, counts, tie order),
samples and train_words — on the host path and the gpu_ingest path; the text8
format keeps the original file's 1000-token sentences; train_file and the CLI
(-phrase) yield the joined words; the sentence API refuses phrase mode."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import phrase_ref as R
from tests.test_corpus_file import _write_corpus

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "word2vec_amd" / "bin" / "word2vec"
PASSES = ((5, 200.0), (5, 100.0))
PLANTS = [("pp", "qq"), ("new", "york", "city"), ("aa", "bb", "cc", "dd"), ("pp_qq",)]


def _model(**kw):
    from word2vec_amd.model import Word2Vec

    return Word2Vec(iter=1, window=5, min_count=3, table_size=10_000, word_dim=16, negative=5,
                    subsample_threshold=1e-3, train_method="ns", model="sg", verbose=False, **kw)


def _phrase_model():
    return _model(phrase_thresholds=[t for _, t in PASSES], phrase_min_count=PASSES[0][0])


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The corpus file F, its reference passes and the rewritten corpus G as text."""
    d = tmp_path_factory.mktemp("phrases")
    text = R.plant_text(_write_corpus(d / "plain.txt", 3_000, seed=13), PLANTS, 40, seed=2)
    f = d / "corpus.txt"
    f.write_text(text)
    ids, off, words = R.from_text(text)
    refs = R.run_passes(ids, off, len(words), PASSES)
    all_words = words
    for r in refs:
        all_words = R.phrase_words(all_words, r.left, r.right)
    assert {"pp_qq", "new_york_city", "aa_bb_cc_dd"} <= set(all_words[len(words):])
    assert all_words.count("pp_qq") == 2                      # the literal token and the phrase
    g = d / "rewritten.txt"
    g.write_text(R.to_text(refs[-1].ids, refs[-1].offsets, all_words))
    return SimpleCorpus(f, g, text, refs, all_words)


class SimpleCorpus:
    def __init__(self, f, g, text, refs, words):
        self.f, self.g, self.text, self.refs, self.words = f, g, text, refs, words


@pytest.mark.parametrize("gpu_ingest", [False, True])
def test_phrase_model_equals_plain_model_on_the_rewritten_corpus(corpus, gpu_ingest):
    ph, plain = _phrase_model(), _model(gpu_ingest=gpu_ingest)
    ph.build_vocab_file(corpus.f, "lines", 4)
    plain.build_vocab_file(corpus.g, "lines", 4)
    pw, pc = ph.vocab()
    qw, qc = plain.vocab()
    assert pw == qw                                           # words in the same (tie) order
    np.testing.assert_array_equal(pc, qc)
    assert "pp_qq" in pw and "new_york_city" in pw and "aa_bb_cc_dd" in pw
    merged = pc[pw.index("pp_qq")]
    assert merged > corpus.text.split().count("pp_qq") > 0    # the literal tokens and the joined pairs add
    a, b = ph.file_samples(corpus.f, "lines", 4), plain.file_samples(corpus.g, "lines", 4)
    assert a[2] == b[2] == corpus.refs[-1].ids.size           # train_words: the rewritten stream's length
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[0], b[0])


def test_text8_format_keeps_the_original_sentences(corpus):
    toks = corpus.text.split()
    index = {}
    ids = np.array([index.setdefault(t, len(index)) for t in toks], np.int32)
    off = np.append(np.arange(0, ids.size, 1000), ids.size).astype(np.int64)
    words = list(index)
    refs = R.run_passes(ids, off, len(words), PASSES)
    for r in refs:
        words = R.phrase_words(words, r.left, r.right)
    want = {}
    for w, c in zip(words, refs[-1].count):
        want[w] = want.get(w, 0) + int(c)
    want = {w: c for w, c in want.items() if c >= 3}
    m = _phrase_model()
    m.build_vocab_file(corpus.f, "text8", 4)
    vw, vc = m.vocab()
    assert dict(zip(vw, (int(c) for c in vc))) == want and len(vw) == len(want)
    assert list(vc) == sorted(vc, reverse=True)
    vocab_index = np.array([vw.index(w) if w in want else -1 for w in words], np.int32)
    got = m.file_samples(corpus.f, "text8", 4)
    want_ids, want_off, want_tw = R.map_samples(refs[-1].ids, refs[-1].offsets, vocab_index)
    assert got[2] == want_tw
    np.testing.assert_array_equal(got[1], want_off)
    np.testing.assert_array_equal(got[0], want_ids)


def test_train_file_with_phrases(corpus):
    m = _phrase_model()
    m.seed(3)
    m.build_vocab_file(corpus.f, "lines", 4)
    m.train_file(corpus.f, "lines", 4)
    words, _ = m.vocab()
    assert "new_york_city" in words and "pp_qq" in words
    W = m.matrix(0)
    assert W.shape == (len(words), 16) and np.isfinite(W).all()
    assert m.current_words > 0


def test_cli_phrase(tmp_path, corpus):
    out, vocab = tmp_path / "vec.txt", tmp_path / "vocab.txt"
    base = [str(CLI), "-train", str(corpus.f), "-size", "16", "-negative", "5", "-iter", "1", "-output", str(out)]
    r = subprocess.run(base + ["-phrase", "200,100", "-phrase-min-count", "5", "-save-vocab", str(vocab)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = [l.split()[2] for l in vocab.read_text().splitlines()]
    assert "new_york_city" in words and "aa_bb_cc_dd" in words
    assert out.read_text().splitlines()[0].split() == [str(len(words)), "16"]
    for bad in (["-phrase", "200,,100"], ["-phrase", "-5"], ["-phrase", "abc"], ["-phrase", "100", "-phrase-min-count", "0"]):
        r = subprocess.run(base + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "-phrase" in r.stdout


def test_sentence_api_refuses_phrase_mode():
    m = _phrase_model()
    with pytest.raises(RuntimeError, match="phrase mode reads files"):
        m.build_vocab([["a", "b", "a", "b"]] * 3)
