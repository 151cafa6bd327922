"""CPU checks of tests/visit_ref.py, the integer reference behind
tests/test_gpu_conservation.py: the vectorised form against a per-token loop,
against TrainRef's centers and against score_ref's summary; and (below) that
the conservation comparison of tests/conservation.py can fail: a dropped
sentence, a doubled sentence and 2 % of one private row's updates each put it
above the bounds the GPU test uses, while the oracle's own orders stay below.
"""
import numpy as np
import pytest

from tests import visit_ref as vr
from tests.corpus import zipf_sentences
from tests.harness import COMBINED_MODES, MODES, mode_config, oracle_run
from tests.score_ref import score_vec
from tests.train_ref import TrainRef

KEY = 0x5EED_0000_1234_ABCD
ALL_MODES = list(MODES) + list(COMBINED_MODES)


@pytest.fixture(scope="module")
def small():
    """About 300 tokens over the vocabulary of a 6-sentence Zipf text, among
    them an empty and a one-token sentence; the vocabulary products (keep,
    table, Huffman tree) come from the oracle."""
    sents = zipf_sentences(6, 90, 120, seed=11, ragged=True)
    o = oracle_run(sents, "sg_hsns", dim=8, window=5, table_size=5000, train=False, min_count=1)
    o.build_sample()
    ids, off = o.samples()
    lens = np.diff(off)
    assert 250 <= ids.size <= 400 and lens.max() > 41  # window 40 is cut by the sentence ends and is not
    # insert an empty sentence after the second and a one-token sentence at the end
    ids = np.concatenate([ids, ids[:1]])
    off = np.concatenate([off[:3], off[2:3], off[3:], [ids.size]])
    assert (np.diff(off) == 0).sum() == 1 and (np.diff(off) == 1).sum() >= 1
    keep = o.sample_probs()
    assert keep.min() < 0.2 and keep.max() > 0.7  # frequent words mostly dropped, rare ones mostly kept
    return dict(o=o, ids=ids, off=off, keep=keep, table=o.table(), bounds=o.table_bounds(), huffman=o.huffman())


def _kw(small, mode, window, negative):
    m = mode_config(mode)
    neg = negative if m["negative"] > 0 else 0
    return dict(window=window, negative=neg, hs=m["train_method"] == "hs", cbow=m["model"] == "cbow")


def _same(a, b, what):
    for k in vr.COUNTERS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in range(3):
        assert (a["updates"][k] is None) == (b["updates"][k] is None), (what, k)
        if a["updates"][k] is not None:
            np.testing.assert_array_equal(a["updates"][k], b["updates"][k], err_msg=f"{what}: matrix {k}")


@pytest.mark.parametrize("window,negative", [(1, 70), (5, 5), (40, 1)])
@pytest.mark.parametrize("mode", ALL_MODES)
def test_visits_match_the_loop(small, mode, window, negative):
    kw = _kw(small, mode, window, negative)
    n = small["off"].size - 1
    order = np.random.default_rng(3).permutation(n)
    for epoch, od in ((0, None), (1, np.concatenate([order, order[:2]]))):  # epoch 1: two sentences twice
        got = vr.visits(small["ids"], small["off"], small["keep"], key=KEY, epoch=epoch, bounds=small["bounds"],
                        huffman=small["huffman"], order=od, chunk=1 << 10, **kw)
        want = vr.visits_loop(small["ids"], small["off"], small["keep"], key=KEY, epoch=epoch, table=small["table"],
                              huffman=small["huffman"], order=od, **kw)
        _same(got, want, f"{mode} w{window} neg{negative} epoch {epoch}")
        assert want["words"] == small["ids"].size + (0 if od is None else int(np.diff(small["off"])[order[:2]].sum()))
        assert 0 < want["centers"] < want["words"] and want["contexts"] > 0 and want["targets"] > 0
        assert want["draws"] == (kw["negative"] * (want["centers"] if kw["cbow"] else want["contexts"]))
        if epoch == 0:
            first = got
    assert any(first[k] != got[k] for k in ("centers", "contexts", "targets"))  # the epoch enters the draws


@pytest.mark.parametrize("mode", ALL_MODES)
def test_centers_match_train_ref(small, mode):
    """TrainRef counts the centers it trains: the kept tokens with a non-empty
    window, in every mode."""
    kw = _kw(small, mode, 5, 5)
    V, d = small["keep"].size, 4
    ref = TrainRef(np.zeros((V, d)), np.zeros((V, d)), np.zeros((V - 1, d)), cbow_mean=True, keep=small["keep"],
                   table=small["table"], huffman=small["huffman"], **kw)
    off = small["off"]
    for s in range(off.size - 1):
        ref.sentence(small["ids"][off[s]:off[s + 1]], s, 0.01, 0, KEY)
    got = vr.visits(small["ids"], off, small["keep"], key=KEY, bounds=small["bounds"], huffman=small["huffman"], **kw)
    assert got["centers"] == ref.centers


@pytest.mark.parametrize("window,shrink", [(1, True), (5, False)])
@pytest.mark.parametrize("mode", list(MODES))
def test_counters_match_score_ref(small, mode, window, shrink):
    """w2v_dev_score makes every token a center with its full window and draws
    with epoch 0 in the counter: with keep = 1 and no shrink (window 1 never
    shrinks: the shrink is below the window) training visits the same pairs, so
    every counter coincides: both count as centers the tokens with a context
    (the input holds one-token sentences and an empty one)."""
    kw = _kw(small, mode, window, 5)
    ids, off = small["ids"], small["off"]
    V, d = small["keep"].size, 4
    got = vr.visits(ids, off, np.ones(V, np.float32), key=KEY, epoch=0, bounds=small["bounds"],
                    huffman=small["huffman"], shrink=shrink, **kw)
    z = np.zeros((V, d))
    sm = score_vec(z, z, z[:-1], ids, off, cbow_mean=True, huffman=small["huffman"], bounds=small["bounds"], key=KEY,
                   **kw)["summary"]
    for k in vr.COUNTERS:
        assert got[k] == sm[k], (k, got[k], sm[k])
    assert (np.diff(off) == 1).sum() >= 1 and sm["centers"] < sm["words"]


@pytest.mark.parametrize("window,negative", [(1, 15), (5, 5), (8, 15)])
def test_shared_visits_match_the_loop(small, window, negative):
    order = np.random.default_rng(5).permutation(small["off"].size - 1)
    for epoch, od in ((0, None), (1, np.concatenate([order, order[:2]]))):
        got = vr.shared_visits(small["ids"], small["off"], small["keep"], window=window, negative=negative, key=KEY,
                               epoch=epoch, bounds=small["bounds"], order=od)
        want = vr.shared_visits_loop(small["ids"], small["off"], small["keep"], window=window, negative=negative,
                                     key=KEY, epoch=epoch, table=small["table"], order=od)
        _same(got, want, f"shared w{window} neg{negative} epoch {epoch}")
        assert want["centers"] > 0 and want["draws"] == negative * want["centers"]
        assert want["centers"] < want["targets"] <= (negative + 1) * want["centers"]


# ---------------------------------------------------------------------------
# The conservation comparison can fail (tests/conservation.py, on the first 40
# sentences of corpus A, the oracle alone)
# ---------------------------------------------------------------------------
from tests import conservation as cv  # noqa: E402


def _emptied(ids, off, drop):
    """The samples with the sentences `drop` emptied (the others keep their
    numbers, which enter the Philox counters)."""
    lens = np.diff(off).copy()
    keep_tok = np.ones(ids.size, bool)
    for s in drop:
        keep_tok[off[s]:off[s + 1]] = False
        lens[s] = 0
    return ids[keep_tok], np.concatenate([[0], np.cumsum(lens)])


def _epoch(o, ids, off, order, start=None):
    """One oracle epoch over (ids, off) from `start` (default: the oracle's
    matrices); the oracle's samples and matrices are put back. Returns the
    resulting matrices."""
    ids0, off0 = o.samples()
    init = cv.matrices(o)
    for k, m in enumerate(start or []):
        if m is not None:
            o.set_matrix(k, m)
    o.set_samples(ids, off, int(off[-1]))
    o.train_philox(0, 1, order, cv.KEY, 0)
    out = cv.matrices(o)
    o.set_samples(ids0, off0, int(off0[-1]))
    for k, m in enumerate(init):
        if m is not None:
            o.set_matrix(k, m)
    return out


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_conservation_comparison_can_fail(mode):
    """Dropping the last sentence's updates, applying one sentence twice and
    leaving out 2 % of the updates of one private row each put the comparison
    above its bounds; the oracle's three sentence orders stay below them."""
    dim, n = 64, 40
    o = cv.corpus_oracle("A", mode, dim, n_sent=n)
    ids, off = o.samples()
    assert off.size - 1 == n
    order = cv.orders(n)[0]
    vis = cv.corpus_visits(o, "A", mode, n_sent=n)[0]
    init = cv.matrices(o)
    priv = cv.private_ranges(mode, o.V)

    def update(result):
        return [None if r is None else r.astype(np.float64) - i for r, i in zip(result, init)]

    want = update(_epoch(o, ids, off, order))
    others = [update(_epoch(o, ids, off, od)) for od in cv.other_orders(order)]
    errs = [cv.measure(u, want, vis, priv) for u in others]
    spread = {k: max(e[k] for e in errs) for k in errs[0]}
    bounds = cv.capped(spread)
    print(f"{mode}: spread {spread}")
    assert any(k.endswith(".rare") for k in bounds) and any(k.endswith(".priv") for k in bounds)
    for e in errs:
        assert all(e[k] < bounds[k] for k in e), (e, bounds)

    def over(u, what):
        e = cv.measure(u, want, vis, priv)
        bad = {k: (e[k], bounds[k]) for k in e if not e[k] < bounds[k]}
        print(f"{mode} {what}: over in {sorted(bad)}")
        return bad

    last = int(order[-1])
    assert off[last + 1] - off[last] > 5
    assert over(update(_epoch(o, *_emptied(ids, off, [last]), order)), "last sentence dropped")
    twice = _epoch(o, *_emptied(ids, off, [s for s in range(n) if s != last]), order, start=_epoch(o, ids, off, order))
    assert over(update(twice), "last sentence applied twice")
    # one private row without ~2 % of its updates: the hottest row of a private range, as trained without the
    # sentence that holds between 1 % and 2.5 % of that row's updates; every other row as the reference has it
    k = max(priv)
    r = int(priv[k][np.argmax(vis["updates"][k][priv[k]])])
    kw = dict(window=cv.WINDOW, negative=cv.mode_config(mode)["negative"], hs=o.hs, cbow=o.cbow, key=cv.KEY,
              bounds=o.table_bounds() if o.negative else None, huffman=o.huffman() if o.hs else None)
    share = np.array([vr.visits(ids, off, o.sample_probs(), order=[s], **kw)["updates"][k][r] for s in range(n)])
    assert share.sum() == vis["updates"][k][r]
    frac = share / share.sum()
    ok = np.nonzero((frac >= 0.01) & (frac <= 0.025))[0]
    assert ok.size, frac
    s = int(ok[np.argmax(frac[ok])])
    less = update(_epoch(o, *_emptied(ids, off, [s]), order))
    got = [None if w is None else w.copy() for w in want]
    got[k][r] = less[k][r]
    bad = over(got, f"row {r} of {cv.NAMES[k]} without {frac[s]:.1%} of its {share.sum()} updates")
    assert f"{cv.NAMES[k]}.priv" in bad, bad


@pytest.mark.parametrize("mode", list(cv.CONSERVED))
def test_committed_spreads_are_the_oracle_s(mode):
    """conservation.SPREADS (d 64; the GPU test checks d 300 too) against three
    oracle runs here, and which of the bounds the caps decide."""
    sp = cv.measured_spreads(mode, 64)
    committed = cv.SPREADS[(mode, 64)]
    assert set(sp) == set(committed)
    for k, v in committed.items():
        assert abs(sp[k] / v - 1) < 0.25, (mode, k, sp[k], v)
    for (m, d), b in cv.BOUNDS.items():
        for k, v in b.items():
            cls = k.split(".")[1]
            assert v <= cv.MARGIN * cv.SPREADS[(m, d)][k]
            assert cls == "norm" or v <= {"rare": cv.RARE_MAX, "priv": cv.PRIV_MAX_BOUND}[cls]
