"""The float64 k-means reference and checker of tests/kmeans_ref.py on cases
worked by hand, the margins the GPU tests (tests/test_gpu_classes.py) rely on,
checked on the reference alone, and the argument checks of the C-ABI that need
no GPU."""
import ctypes

import numpy as np
import pytest

from tests import kmeans_ref as K
from tests.nn_ref import tol


def test_hand_worked_run():
    """Start [0, 1, 0, 1]: c0 = unit(1, 2), c1 = unit(3, 1); rows 0 and 1 swap sides, then nothing moves."""
    x = np.array([[1, 0], [0, 1], [0, 2], [3, 0]], np.float32)
    assert K.start(x, 2).tolist() == [0, 1, 0, 1]
    cen, counts, sums = K.update(x, [0, 1, 0, 1], 2)
    assert sums.tolist() == [[1, 2], [3, 1]] and counts.tolist() == [2, 2]
    assert np.allclose(cen, [[1 / np.sqrt(5), 2 / np.sqrt(5)], [3 / np.sqrt(10), 1 / np.sqrt(10)]], atol=1e-15)
    cls, sc = K.assign(x, cen)
    assert cls.tolist() == [1, 0, 0, 1]
    assert np.allclose(sc, [3 / np.sqrt(10), 2 / np.sqrt(5), 2 / np.sqrt(5), 3 / np.sqrt(10)], atol=1e-15)
    r = K.run(x, 2, 10)
    assert r["classes"].tolist() == [1, 0, 0, 1] and r["moved"].tolist() == [2, 0] and r["iterations"] == 2
    assert np.allclose(r["centroids"], [[0, 1], [1, 0]]) and np.allclose(r["scores"], 1.0)
    assert r["counts"].tolist() == [2, 2]
    one = K.run(x, 2, 1)
    assert one["classes"].tolist() == [1, 0, 0, 1] and one["iterations"] == 1 and one["moved"].tolist() == [2]
    assert np.allclose(one["centroids"], cen)  # the centroids the classes were scored against


def test_ties_go_to_the_lowest_class():
    x = np.array([[1, 1], [2, 0], [0, 0]], np.float32)
    cls, sc = K.assign(x, np.array([[0, 3], [5, 0], [0, 3]], np.float32))  # (1, 1) is as near to 0 as to 1; 2 copies 0
    assert cls.tolist() == [0, 1, 0] and sc[2] == 0.0  # the zero row: 0 everywhere, lowest class
    cls, _ = K.assign(x, np.array([[0, 0], [0, 3], [5, 0]], np.float32))
    assert cls.tolist() == [1, 2, 1]  # ... lowest valid class


def test_empty_nan_and_non_finite_rules():
    x = np.array([[1, 0], [np.nan, 1], [0, np.inf], [0, 2], [-1, 0]], np.float32)
    assert K.start(x, 2).tolist() == [0, -1, -1, 1, 0]
    cen, counts, _ = K.update(x, [0, 0, 1, 1, 0], 3)  # rows 0 and 4 cancel; class 2 is empty; 1 and 2 are left out
    assert counts.tolist() == [2, 1, 0]
    assert cen[0].tolist() == [0, 0] and cen[2].tolist() == [0, 0] and cen[1].tolist() == [0, 1]
    assert K.valid_centroids(cen).tolist() == [False, True, False]
    cls, sc = K.assign(x, cen)
    assert cls.tolist() == [1, -1, -1, 1, 1] and np.isneginf(sc[[1, 2]]).all() and sc[3] == 1.0
    cls, sc = K.assign(x, np.array([[0, 0], [np.nan, 1]], np.float32))  # no valid centroid
    assert cls.tolist() == [-1] * 5 and np.isneginf(sc).all()


def test_checker_accepts_the_reference_and_rejects_wrong_answers():
    x = K.random_rows(300, 24, 5)
    x[11] = np.nan
    cen = K.random_centroids(9, 24, 6)
    cen[4] = 0
    cls, sc = K.assign(x, cen)
    assert cls[11] == -1 and 4 not in cls and cls[3] == cls[7]
    K.check_assign(x, cen, cls, sc.astype(np.float32), 24)
    bad = sc.astype(np.float32).copy()
    bad[20] += 4 * tol(24)
    with pytest.raises(AssertionError, match="score off"):
        K.check_assign(x, cen, cls, bad, 24)
    wrong = cls.copy()
    wrong[20] = (cls[20] + 1) % 9 if (cls[20] + 1) % 9 != 4 else (cls[20] + 2) % 9
    with pytest.raises(AssertionError):
        K.check_assign(x, cen, wrong, sc.astype(np.float32), 24)
    wrong = cls.copy()
    wrong[11] = 0
    with pytest.raises(AssertionError, match="-1 must mark"):
        K.check_assign(x, cen, wrong, sc.astype(np.float32), 24)


ASSIGN_SHAPES = [(1031, 48, 17, 2), (600, 700, 33, 3), (5000, 300, 500, 4), (333, 400, 21, 5)]


@pytest.mark.parametrize("V,d,k,seed", ASSIGN_SHAPES)
def test_assign_cases_have_clear_gaps(V, d, k, seed):
    cos = K.cosines(K.random_rows(V, d, seed), K.random_centroids(k, d, seed + 10))
    assert (K.top_two_gap(cos) > 2 * tol(d)).mean() >= 0.97


@pytest.mark.parametrize("shape", K.PLANTED_SHAPES, ids=["d48", "d300"])
def test_planted_runs_keep_wide_margins(shape):
    """What lets the GPU run equal the reference exactly: in every iteration the smallest top-two gap is above
    100 tol, so f32 rounding of scores and centroids cannot flip a row."""
    x, _ = K.planted(**shape)
    r = K.run(x, shape["K"], 10)
    assert min(r["gaps"]) > 100 * tol(shape["d"]), [g / tol(shape["d"]) for g in r["gaps"]]
    assert r["iterations"] < 10 and r["moved"][-1] == 0 and r["moved"][0] > 0  # the early stop is exercised
    if shape["d"] == 48:
        assert r["moved"].tolist() == [634, 3, 0]
    else:
        assert r["iterations"] == 2


def test_null_index_is_refused_without_a_gpu():
    from word2vec_amd import _native as N

    lib = N.load_dev_lib()
    buf = (ctypes.c_int32 * 4)()
    f = (ctypes.c_float * 4)()
    assert lib.w2v_nn_assign(None, f, 1, buf, None) == N.W2V_ERR_ARG
    assert b"null index" in lib.w2v_dev_last_error()
    assert lib.w2v_nn_centroids(None, buf, 1, f, None) == N.W2V_ERR_ARG
    assert lib.w2v_nn_classes(None, 1, 1, buf, None, None, None, None, None) == N.W2V_ERR_ARG
    k, it = ctypes.c_int32(), ctypes.c_int32()
    assert lib.w2v_nn_class_limits(ctypes.byref(k), ctypes.byref(it)) == N.W2V_OK
    assert (k.value, it.value) == (65536, 1000)
