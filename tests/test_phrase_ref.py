"""tests/phrase_ref.py, the CPU reference of phrase detection: the worked
example of DESIGN.md §4.6 (both passes, scores included), and the sequential
definition against the vectorised form on every builder's stream."""
import numpy as np
import pytest

from tests import phrase_ref as R


def _scores(r, words):
    return {(words[a], words[b]): (int(c), s) for a, b, c, s in zip(r.bg_left, r.bg_right, r.bg_count, r.bg_score)}


@pytest.mark.parametrize("fn", [R.pass_loop, R.pass_vec])
def test_worked_example(fn):
    ids, off, words = R.from_text(R.EXAMPLE)
    assert ids.size == 28
    p1, p2 = R.run_passes(ids, off, len(words), R.EXAMPLE_PASSES, fn)
    f = np.float32
    w1 = R.phrase_words(words, p1.left, p1.right)
    assert R.to_text(p1.ids, p1.offsets, w1) == R.EXAMPLE_AFTER[0]
    assert w1[len(words):] == ["new_york", "a_a"] and list(p1.joined) == [5, 2]
    s1 = _scores(p1, words)
    count = dict(zip(words, np.bincount(ids)))
    assert (count["new"], count["york"], count["a"]) == (6, 6, 5)
    assert s1[("new", "york")] == (5, f(2.3333335)) and s1[("a", "a")] == (4, f(2.24))
    assert s1[("york", "new")] == (2, f(0.0)) and s1[("big", "city")][1] == f(-2.8)
    assert s1[("new", "york")][1] == f(3) / f(6) / f(6) * f(28)
    assert p1.ids.size == 21 and p1.n_joined == 7
    w2 = R.phrase_words(w1, p2.left, p2.right)
    assert R.to_text(p2.ids, p2.offsets, w2) == R.EXAMPLE_AFTER[1]
    assert w2[len(w1):] == ["new_york_city"] and list(p2.joined) == [3]
    s2 = _scores(p2, w1)
    assert s2[("new_york", "city")] == (3, f(0.84)) and s2[("new_york", "new_york")][1] == f(-0.84)
    assert s2[("a_a", "a_a")][1] == f(-5.25)
    assert p1.count[w1.index("new_york")] == 5 and p2.count[w2.index("new_york")] == 2
    assert p2.count[w2.index("a_a")] == 2 and p2.first[w2.index("new_york_city")] == 0


def _streams():
    b_ids, b_off, b_words = R.boundary_stream()
    return {
        "zipf": (R.zipf_stream(), ((5, 50.0),)),
        "alternating": (R.alternating_stream(), ((2, 1.0),)),
        "alternating-shift": (R.alternating_stream("shift"), ((2, 1.0),)),
        "alternating-cut": (R.alternating_stream("cut"), ((2, 1.0),)),
        "boundary": ((b_ids, b_off, len(b_words)), ((R.BOUNDARY_MIN_COUNT, 0.0),)),
        "multipass": (R.multipass_stream(), R.MULTIPASS),
        "empty": ((np.zeros(0, np.int32), np.zeros(3, np.int64), 4), ((1, 0.0),)),
    }


@pytest.mark.parametrize("name", sorted(_streams()))
def test_loop_equals_vectorised(name):
    stream, passes = _streams()[name]
    for a, b in zip(R.run_passes(*stream, passes, R.pass_loop), R.run_passes(*stream, passes, R.pass_vec)):
        for k in vars(a):
            np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_builders_hold_what_the_gpu_tests_rely_on():
    ids, off, n_words = R.zipf_stream()
    assert ids.size == 200_000 and n_words == 70_000 and ids.max() > 1 << 16
    lens = np.diff(off)
    assert lens.min() == 0 and lens.max() == 40 and np.any((lens[:-1] == 0) & (lens[1:] == 0))
    r = R.pass_vec(ids, off, n_words, 5, 50.0)
    assert r.bg_count.size > 40_000 and r.n_joined > 5_000 and r.left.max() >= 66_000 and r.count[66_040:70_000].max() == 0
    # the alternating sentence: thousands of consecutive candidates, every other one joins
    for variant in ("even", "shift"):
        ids, off, n_words = R.alternating_stream(variant)
        r = R.pass_vec(ids, off, n_words, 2, 1.0)
        xy = r.n_words - r.left.size + int(np.flatnonzero((r.left == 0) & (r.right == 1))[0])
        assert r.count[xy] == 3_000 and r.count[0] == 0 and r.count[1] == 0
    ids, off, n_words = R.alternating_stream("cut")
    r = R.pass_vec(ids, off, n_words, 2, 1.0)
    assert set(zip(r.left[r.joined > 1_000], r.right[r.joined > 1_000])) == {(0, 1), (1, 0)}
    zz = r.n_words - r.left.size + int(np.flatnonzero((r.left == 2) & (r.right == 2))[0])
    assert r.count[zz] == 3 and r.count[2] == 1
    # the boundary stream
    ids, off, words = R.boundary_stream()
    r = R.pass_vec(ids, off, len(words), R.BOUNDARY_MIN_COUNT, 0.0)
    pairs = {(words[a], words[b]): c for a, b, c in zip(r.bg_left, r.bg_right, r.bg_count)}
    assert ("p", "q") not in pairs and ("s", "r") not in pairs and ("r", "s") not in pairs
    assert pairs[("t", "s")] == 3 and pairs[("u", "v")] == 3 and pairs[("g", "h")] == 5
    assert [(words[a], words[b]) for a, b in zip(r.left, r.right)] == [("g", "h")]
    # the multi-pass stream: later phrases are made of earlier ones, "b" is absorbed
    p = R.run_passes(*R.multipass_stream(), R.MULTIPASS)
    assert p[0].count[2_001] == 0 and p[0].first[2_001] == -1
    assert p[1].left.min() >= 2_020 and p[2].left.size >= 1 and p[2].left.min() >= p[1].n_words - p[1].left.size
