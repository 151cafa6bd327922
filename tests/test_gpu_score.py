"""w2v_dev_score on the GPU against tests/score_ref.py (float64), through
DeviceTrainer: every sentence within the a-priori bound, every count equal, and
the determinism, isolation and refusals include/w2v_dev.h promises.

The model is random in all three matrices (the initial model's output matrix
is zero: every term would be log 1/2), with row scales that give the reference
sigma arguments below -20. V = 70; sentence lengths 0, 1, 2, 3, 63, 64, 65,
130, 200, 700 and one sentence of a single repeated word."""
import functools
import json
import os

import numpy as np
import pytest

from tests import score_ref as R
from tests.corpus import zipf_ids, zipf_sentences
from tests.harness import oracle_run
from word2vec_amd import _native as N
from word2vec_amd.device import Config, DeviceTrainer

pytestmark = pytest.mark.gpu

V = 70
LENS = [0, 1, 2, 3, 63, 64, 65, 130, 200, 700, 40]
TABLE = 1000
MODES = ["sg_ns", "sg_hs", "cbow_ns", "cbow_hs"]


@functools.lru_cache(maxsize=None)
def corpus():
    ids = zipf_ids(sum(LENS), V, seed=11).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    ids[off[-2]:] = 17  # one repeated word: a distinct-id set of size 1 under N_i > 1
    return ids, off


@functools.lru_cache(maxsize=None)
def oracle_tree():
    o = oracle_run(zipf_sentences(60, 40, V, seed=2), "sg_hs", dim=4, min_count=1, train=False)
    assert o.V == V
    return o.huffman()


@functools.lru_cache(maxsize=None)
def table_bounds():
    p = 1.0 / np.arange(1, V + 1) ** 0.75
    b = np.concatenate([[0], np.floor(np.cumsum(p) / p.sum() * TABLE)]).astype(np.int64)
    b[-1] = TABLE
    return b


@functools.lru_cache(maxsize=None)
def model(d, seed=0):
    """float32 matrices; a row's scale is one of 0.05 .. 3, so that dot products span |z| from ~0 to far past 20."""
    rng = np.random.default_rng(1000 * d + seed)
    out = []
    for rows in (V, V, V - 1):
        sc = rng.choice([0.05, 0.3, 1.0, 3.0], size=(rows, 1))
        out.append((rng.normal(size=(rows, d)) * sc).astype(np.float32))
    return tuple(out)


def config(mode, d, window=5, negative=5, cbow_mean=False):
    hs, cbow = mode.endswith("hs"), mode.startswith("cbow")
    return Config(word_dim=d, window=window, negative=0 if hs else negative, hs=hs, cbow=cbow, cbow_mean=cbow_mean,
                  iter=1, table_size=TABLE)


def ref_kwargs(cfg, tree):
    kw = dict(window=cfg.window, negative=cfg.negative, hs=cfg.hs, cbow=cfg.cbow, cbow_mean=cfg.cbow_mean)
    if cfg.hs:
        kw["huffman"] = R.chain_tree(V) if tree == "chain" else oracle_tree()
    else:
        kw["bounds"] = table_bounds()
    return kw


@functools.lru_cache(maxsize=None)
def reference(mode, d, window=5, negative=5, cbow_mean=False, tree="oracle", key=0):
    cfg = config(mode, d, window, negative, cbow_mean)
    ids, off = corpus()
    return R.score_vec(*model(d), ids, off, key=key, **ref_kwargs(cfg, tree))


def device(cfg, tree="oracle", mats=None, resident=False):
    W, C, S = mats if mats is not None else model(cfg.word_dim)
    d = DeviceTrainer(cfg)
    hf = ref_kwargs(cfg, tree).get("huffman", (None, None, None))
    d.upload_vocab(np.ones(V, np.float32), None if cfg.hs else table_bounds(), *hf)
    d.upload_model(W, C if (cfg.negative > 0 or cfg.cbow) else None, S if cfg.hs else None)
    if resident:
        ids, off = corpus()
        d.upload_corpus(ids, off, len(ids))
    return d


def log_ratio(tag, ratio):
    print(f"{tag}: largest |ll - ref| / bound = {ratio:.4f}")
    path = os.environ.get("W2V_SCORE_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"tag": tag, "ratio": ratio}) + "\n")


def check(got, ref, tag):
    assert got["targets"].tolist() == ref["targets"].tolist(), tag
    for k in ("sentences", "words", "centers", "contexts", "targets", "draws", "nonfinite"):
        assert got["summary"][k] == ref["summary"][k], (tag, k)
    err = np.abs(got["ll"] - ref["ll"])
    live = ref["bound"] > 0
    assert np.all(got["ll"][~live] == 0.0) and np.all(ref["ll"][~live] == 0.0)
    log_ratio(tag, float(np.max(err[live] / ref["bound"][live])))
    assert np.all(err <= ref["bound"]), (tag, err.tolist(), ref["bound"].tolist())
    acc = 0.0
    for v in got["ll"]:
        acc += float(v)
    assert got["summary"]["ll"] == acc  # the summary is the sentences' sum, in order
    assert got["per_target"] == acc / ref["summary"]["targets"]


def run(mode, d, window=5, negative=5, cbow_mean=False, tree="oracle", key=0):
    cfg = config(mode, d, window, negative, cbow_mean)
    ref = reference(mode, d, window, negative, cbow_mean, tree, key)
    dev = device(cfg, tree)
    try:
        ids, off = corpus()
        got = dev.score(ids, off, key=key)
    finally:
        dev.close()
    check(got, ref, f"{mode} d{d} w{window} n{cfg.negative} mean{int(cbow_mean)} {tree if cfg.hs else 'table'}")
    return got, ref


@pytest.mark.parametrize("d", [48, 100, 300, 700])
@pytest.mark.parametrize("mode", MODES)
def test_modes_and_widths(mode, d):
    got, ref = run(mode, d, key=0xC0FFEE12345)
    assert ref["min_z"] < -20.0  # the reference itself has terms where a naive fp32 log(sigmoid) is lost
    assert got["ll"][0] == 0.0 and got["ll"][1] == 0.0 and got["targets"][:2].tolist() == [0, 0]


def test_widest_row():
    run("sg_ns", 2048, key=5)


@pytest.mark.parametrize("mode", ["sg_hs", "cbow_hs"])
def test_chain_tree_paths_longer_than_a_batch_and_a_wave(mode):
    _, _, coff = R.chain_tree(V)
    assert np.diff(coff).max() == V - 1 > 64
    run(mode, 100, tree="chain")


@pytest.mark.parametrize("window", [1, 40, 127])
@pytest.mark.parametrize("mode", MODES)
def test_windows(mode, window):
    """1: two contexts; 40: a span above 64 lanes; 127: the limit, longer than most of the sentences."""
    run(mode, 48, window=window, key=3)


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("mode", ["cbow_ns", "cbow_hs"])
def test_cbow_mean(mode, mean):
    got, _ = run(mode, 100, cbow_mean=mean, key=3)
    other = reference(mode, 100, 5, 5, not mean, "oracle", 3)
    assert not np.allclose(got["ll"][4:], other["ll"][4:])  # the flag changes the score


@pytest.mark.parametrize("negative", [1, 5, 63])
@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns"])
def test_negatives(mode, negative):
    _, ref = run(mode, 100, negative=negative, key=0xFEEDFACE)
    assert ref["collisions"] >= 1  # a draw equal to its positive
    if negative > 1:  # one draw per context cannot repeat
        assert ref["duplicates"] >= 1


def test_keys():
    a, _ = run("sg_ns", 100, key=1)
    b, _ = run("sg_ns", 100, key=2)
    c, _ = run("sg_ns", 100, key=1)
    assert np.array_equal(a["ll"], c["ll"]) and a["summary"] == c["summary"]
    assert not np.array_equal(a["ll"][4:], b["ll"][4:])
    # the high half of the key counts too
    d, _ = run("sg_ns", 100, key=1 | (1 << 40))
    assert not np.array_equal(a["ll"][4:], d["ll"][4:])


@pytest.mark.parametrize("mode", MODES)
def test_same_bits_for_every_grid_and_regrouping_by_item(mode):
    cfg = config(mode, 100)
    ids, off = corpus()
    dev = device(cfg)
    try:
        base = dev.score(ids, off, key=7)
        again = dev.score(ids, off, key=7)
        dev.set_max_waves(1)
        one = dev.score(ids, off, key=7)
        dev.set_max_waves(3)
        three = dev.score(ids, off, key=7)
        dev.set_max_waves(0)
        fine = dev.score(ids, off, key=7, item=64)
        fine1 = dev.score(ids, off, key=7, item=64)
    finally:
        dev.close()
    for other in (again, one, three):
        assert np.array_equal(base["ll"], other["ll"]) and base["summary"] == other["summary"]
        assert np.array_equal(base["targets"], other["targets"])
    assert np.array_equal(fine["ll"], fine1["ll"])
    assert np.array_equal(base["targets"], fine["targets"])
    np.testing.assert_allclose(fine["ll"], base["ll"], rtol=1e-12, atol=0)  # fp64 regrouping only
    assert LENS[-2] > 256  # the automatic item splits the long sentence differently than 64 does


@pytest.mark.parametrize("mode", ["sg_hs", "cbow_hs"])
def test_hs_copies_of_a_sentence_score_the_same_bits(mode):
    ids, off = corpus()
    s = ids[off[8]:off[9]]
    two = np.concatenate([s, ids[off[5]:off[6]], s]).astype(np.int32)
    o2 = np.array([0, len(s), len(s) + LENS[5], 2 * len(s) + LENS[5]], np.int64)
    dev = device(config(mode, 100))
    try:
        r = dev.score(two, o2)
    finally:
        dev.close()
    assert r["ll"][0] == r["ll"][2] != 0.0 and r["targets"][0] == r["targets"][2]


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_resident_corpus_and_isolation(mode):
    """ids=None scores the resident corpus; scoring moves no statistic, no progress and no weight."""
    cfg = config(mode, 100)
    ids, off = corpus()
    dev = device(cfg, resident=True)
    try:
        dev.set_progress(1234)
        st0, m0 = dev.read_stats(), dev.download_model()
        res = dev.score(key=9)
        exp = dev.score(ids, off, key=9)
        other = dev.score(ids[:off[5]], off[:6], key=9)  # the scored buffers change; the resident corpus stays
        res2 = dev.score(key=9)
        assert dev.read_stats() == st0 and dev.get_progress() == 1234
        for a, b in zip(m0, dev.download_model()):
            assert (a is None and b is None) or np.array_equal(a, b)
    finally:
        dev.close()
    assert len(res["ll"]) == len(LENS)
    assert np.array_equal(res["ll"], exp["ll"]) and res["summary"] == exp["summary"]
    assert np.array_equal(res2["ll"], res["ll"]) and np.array_equal(other["ll"], exp["ll"][:5])
    check(res, reference(mode, 100, key=9), f"{mode} resident")


@pytest.mark.parametrize("mode,which", [("sg_ns", 0), ("sg_ns", 1), ("cbow_hs", 1), ("sg_hs", 2)])
def test_nan_row_marks_exactly_the_sentences_that_touch_it(mode, which):
    cfg = config(mode, 100)
    mats = [m.copy() for m in model(100)]
    rare = V - 8
    _, points, coff = oracle_tree()
    row = rare if which < 2 else int(points[coff[rare + 1] - 1])  # a rare word's row / the deepest node of its path
    mats[which][row, 3] = np.nan
    ids, off = corpus()
    ref = R.score_vec(*mats, ids, off, key=4, **ref_kwargs(cfg, "oracle"))
    hit = np.isnan(ref["ll"])
    assert hit.any() and not hit[ref["targets"] > 0].all()  # the reference: some sentences touch the row, some do not
    dev = device(cfg, mats=mats)
    try:
        got = dev.score(ids, off, key=4)  # returns: a diverged model is reported, not refused
    finally:
        dev.close()
    assert np.array_equal(np.isnan(got["ll"]), hit)
    assert got["summary"]["nonfinite"] >= 1 and np.isnan(got["summary"]["ll"])
    assert got["targets"].tolist() == ref["targets"].tolist()
    clean = reference(mode, 100, key=4)
    assert np.all(np.abs(got["ll"][~hit] - clean["ll"][~hit]) <= clean["bound"][~hit])


def test_refusals():
    ids, off = corpus()
    for kw, what in ((dict(window=128), b"window > 127"), (dict(negative=64), b"negative > 63")):
        dev = device(config("sg_ns", 48, **kw))
        try:
            with pytest.raises(N.DevError, match="unsupported") as e:
                dev.score(ids, off)
            assert e.value.code == N.W2V_ERR_UNSUPPORTED and what in str(e.value).encode()
        finally:
            dev.close()
    dev = device(config("sg_ns", 48))
    try:
        bad = ids.copy()
        bad[100] = V
        with pytest.raises(N.DevError, match="out of vocab range") as e:
            dev.score(bad, off)
        assert e.value.code == N.W2V_ERR_ARG
        with pytest.raises(N.DevError, match="multiple of 64"):
            dev.score(ids, off, item=100)
        with pytest.raises(N.DevError, match="resident"):
            dev.score()  # nothing resident to score
        assert dev.score(ids, off)["summary"]["sentences"] == len(LENS)  # the handle still works
    finally:
        dev.close()
