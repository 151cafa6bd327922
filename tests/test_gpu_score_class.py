"""Word2Vec::score_ids / score / score_file, the held-out objective per epoch
and the CLI's -score, through word2vec_amd.model.Word2Vec on the GPU."""
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import score_ref as R
from tests.corpus import zipf_sentences
from tests.harness import MODES
from word2vec_amd.model import Word2Vec

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
CLI = ROOT / "word2vec_amd" / "bin" / "word2vec"
TS = 20_000
SENTS = zipf_sentences(12, 90, 120, seed=21, ragged=True)


def make(mode, iters=1, dim=40, replay=False, seed=5, sents=SENTS):
    m = MODES[mode]
    w = Word2Vec(iter=iters, window=5, min_count=2, table_size=TS, word_dim=dim, negative=m["negative"],
                 subsample_threshold=1e-3, init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True,
                 train_method=m["train_method"], model=m["model"], replay_rng=replay)
    w.seed(seed)
    w.build_vocab(sents)
    w.init_weights()
    return w


def ids_of(w, sents):
    index = {t: i for i, t in enumerate(w.vocab()[0])}
    ids, off = [], [0]
    for s in sents:
        ids += [index[t] for t in s if t in index]
        off.append(len(ids))
    return np.asarray(ids, np.int32), np.asarray(off, np.int64)


def randomise(w, mode, seed=3):
    """Random content in every matrix the mode reads; returns (W, C, S) as the reference takes them."""
    rng = np.random.default_rng(seed)
    out = [None, None, None]
    for k in range(3):
        rows = w.matrix(k).shape[0]
        if rows:
            out[k] = (rng.normal(size=(rows, w.word_dim)) * rng.choice([0.1, 0.5, 1.5], size=(rows, 1))).astype(np.float32)
            w.set_matrix(k, out[k])
    return out


def reference(w, mode, mats, ids, off, key):
    m = MODES[mode]
    kw = dict(window=5, negative=m["negative"], hs=m["train_method"] == "hs", cbow=m["model"] == "cbow",
              cbow_mean=True, key=key)
    if kw["hs"]:
        kw["huffman"] = w.huffman()
    else:
        kw["bounds"] = np.searchsorted(w.table(), np.arange(w.V + 1), "left")  # the monotone table's first indices
        assert kw["bounds"][0] == 0 and kw["bounds"][-1] == TS
    return R.score_vec(*mats, ids, off, **kw)


@pytest.mark.parametrize("mode", list(MODES))
def test_score_ids_matches_the_reference_on_the_models_own_products(mode):
    w = make(mode)
    mats = randomise(w, mode)
    ids, off = ids_of(w, SENTS)
    got = w.score_ids(ids, off, key=77)
    ref = reference(w, mode, mats, ids, off, 77)
    assert got["targets"].tolist() == ref["targets"].tolist()
    for k in ("sentences", "words", "centers", "contexts", "targets", "draws", "nonfinite"):
        assert got["summary"][k] == ref["summary"][k], k
    err = np.abs(got["ll"] - ref["ll"])
    print(f"{mode}: largest |ll - ref| / bound = {np.max(err / np.maximum(ref['bound'], 1e-300)):.4f}")
    assert np.all(err <= ref["bound"])
    for k in range(3):  # scoring moved nothing on the host
        if mats[k] is not None:
            assert np.array_equal(w.matrix(k), mats[k])


def test_score_drops_unknown_words_and_score_file_reads_like_file_samples(tmp_path):
    w = make("sg_ns")
    randomise(w, "sg_ns")
    noisy = [s[:3] + ["never-seen"] + s[3:] + ["nor-this"] for s in SENTS] + [["never-seen"]]
    ids, off = ids_of(w, noisy)
    assert off[-1] == ids_of(w, SENTS)[1][-1] and off[-1] == off[-2]
    a, b = w.score(noisy, key=5), w.score_ids(ids, off, key=5)
    assert np.array_equal(a["ll"], b["ll"]) and a["summary"] == b["summary"] and a["ll"][-1] == 0.0
    path = tmp_path / "held.txt"
    path.write_text("\n".join(" ".join(s) for s in noisy) + "\n")
    for fmt in ("lines", "text8"):
        fi, fo, _ = w.file_samples(path, fmt)
        c, d = w.score_file(path, fmt, key=5), w.score_ids(fi, fo, key=5)
        assert np.array_equal(c["ll"], d["ll"]) and c["summary"] == d["summary"]
        assert np.array_equal(c["targets"], d["targets"])
    assert np.array_equal(w.score_file(path, "lines", key=5)["ll"], a["ll"])


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_train_after_score_is_train_without_it(mode):
    """Replay mode is deterministic: a score between two train calls must leave the second one's draws
    (the generator), its start (current_words, resume state) and so its matrices bit for bit alone."""
    ids, off = None, None
    out = []
    for with_score in (False, True):
        w = make(mode, iters=1, dim=32, replay=True)
        w.train(SENTS)
        cw = w.current_words
        if with_score:
            ids, off = ids_of(w, SENTS)
            before = [w.matrix(k).copy() for k in range(3)]
            s = w.score_ids(ids, off, key=1)
            assert np.isfinite(s["summary"]["ll"]) and s["summary"]["targets"] > 0
            assert w.current_words == cw and w.epochs_done == 1
            assert all(np.array_equal(w.matrix(k), before[k]) for k in range(3))
            assert w.most_similar([w.vocab()[0][0]], topn=3)  # the nearest-neighbour index still answers
        w.train(SENTS)
        out.append([w.matrix(k) for k in range(3)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def topic_sentences(n_sent, sent_len, seed, topics=6, block=20):
    """Sentences whose words all come from one of `topics` blocks of `block` words: the context predicts the
    word's block, so a trained model scores them far above an untrained one."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sent):
        t = rng.integers(topics)
        out.append([f"t{t}w{k}" for k in rng.integers(0, block, sent_len)])
    return out


def test_heldout_objective_per_epoch():
    train = topic_sentences(80, 100, seed=31)
    held = topic_sentences(8, 80, seed=32)  # the same distribution, other draws
    w = make("sg_hs", iters=2, dim=32, sents=train)
    ids, off = ids_of(w, held)
    w.train(train)
    assert w.epoch_heldout == []  # off until asked for
    w.set_heldout(ids, off, key=0)
    w.train(train)
    eh = w.epoch_heldout
    assert len(eh) == 2 and len(w.epoch_seconds) == 2
    after = w.score_ids(ids, off, key=0)
    assert eh[1] == (after["summary"]["ll"], after["summary"]["targets"])  # the resident model == the downloaded one
    for ll, tg in eh:
        # a sanity inequality, not a tolerance: an untrained HS model (synapses1 = 0) scores tg * log(1/2)
        assert tg == after["summary"]["targets"] > 0 and math.isfinite(ll) and ll > tg * math.log(0.5)
    print("held-out ll per target by epoch:", [ll / tg for ll, tg in eh], "untrained:", math.log(0.5))
    untrained = make("sg_hs", iters=2, dim=32, sents=train)
    u = untrained.score_ids(ids, off)
    # every term is the fp32 value of -log1p(exp(-0)): log(1/2) to one fp32 rounding
    assert u["summary"]["ll"] == pytest.approx(u["summary"]["targets"] * math.log(0.5), rel=2.0 ** -23)
    w.set_heldout(None)
    w.train(train)
    assert w.epoch_heldout == []


def test_cli_score(tmp_path):
    sents = zipf_sentences(4, 1000, 300, seed=41)
    held = zipf_sentences(3, 700, 300, seed=42)
    corpus, heldf, per = tmp_path / "corpus.txt", tmp_path / "held.txt", tmp_path / "scores.txt"
    corpus.write_text(" ".join(" ".join(s) for s in sents))
    heldf.write_text(" ".join(" ".join(s) for s in held))
    base = [str(CLI), "-train", str(corpus), "-output", str(tmp_path / "vec.txt"), "-size", "32", "-train_method", "hs",
            "-model", "sg", "-iter", "1", "-min-count", "2"]
    r = subprocess.run(base + ["-score", str(heldf), "-score-output", str(per)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("score:")]
    assert len(line) == 1, r.stdout
    f = line[0].split()
    assert f[1::2] == ["sentences", "targets", "ll", "ll_per_target"]
    n_sent, targets, ll, per_target = int(f[2]), int(f[4]), float(f[6]), float(f[8])
    rows = [l.split() for l in per.read_text().splitlines()]
    assert len(rows) == n_sent == 3 and all(len(x) == 2 for x in rows)  # 2100 tokens: 1000-token sentences
    acc = 0.0
    for x in rows:
        acc += float(x[0])
    assert acc == ll and sum(int(x[1]) for x in rows) == targets and per_target == ll / targets
    assert math.isfinite(ll) and ll < 0
    # the bridge on the same files: the same vocabulary, sentences and Huffman paths, so the same term counts
    # (the CLI seeds from std::random_device, so its weights and ll are its own)
    w = Word2Vec(iter=1, window=5, min_count=2, table_size=TS, word_dim=32, negative=0, subsample_threshold=1e-4,
                 cbow_mean=True, train_method="hs", model="sg")
    w.build_vocab_file(corpus, "text8")
    w.init_weights()
    b = w.score_file(heldf, "text8")
    assert b["targets"].tolist() == [int(x[1]) for x in rows] and b["summary"]["sentences"] == n_sent
    # refusals
    r = subprocess.run(base + ["-score-output", str(per)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-score" in r.stdout
    r = subprocess.run(base + ["-score", str(heldf), "-window", "128"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-window <= 127" in r.stdout
