"""Word classes on the GPU (word2vec_amd/nn.py NearestIndex.assign / centroids /
classes over include/w2v_dev.h w2v_nn_assign / _centroids / _classes) against
the float64 reference and checker of tests/kmeans_ref.py. The shapes are the
smallest that reach the tail row tile, the tail centroid tile, the padded
columns (d 100 -> 112, d 300 -> 304) and the kernel that re-reads the row
fragments (d 700)."""
import numpy as np
import pytest

from tests import kmeans_ref as K
from tests.nn_ref import tol, unit64
from word2vec_amd import _native as N
from word2vec_amd.nn import NearestIndex, class_limits, class_times

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- 1. assign against the reference ---------------------------------------------------------
# 4, 7, 8, 13, 16, 19, 20, 24, 32 and 33 blocks of 16 columns: every instantiated resident width, and the
# streaming kernel
INSTANCE_WIDTHS = [64, 112, 128, 208, 256, 304, 320, 384, 512, 528]


@pytest.mark.parametrize("V,d,k,seed", [(1031, 48, 17, 2), (600, 700, 33, 3), (5000, 300, 500, 4), (333, 400, 21, 5)] +
                         [(333, d, 21, 5) for d in INSTANCE_WIDTHS])
def test_assign_matches_reference(V, d, k, seed):
    """(333, 400, 21, 5) takes the one-tile-per-wave kernel (rows of 321 to 512 floats); the shapes after it
    take every instantiated width in turn."""
    rows, cen = K.random_rows(V, d, seed), K.random_centroids(k, d, seed + 10)
    share = (K.top_two_gap(K.cosines(rows, cen)) > 2 * tol(d)).mean()
    assert share >= 0.97  # on the reference alone
    with NearestIndex.from_matrix(rows) as index:
        cls, sc = index.assign(cen)
        again = index.assign(cen)
    clear = K.check_assign(rows, cen, cls, sc, d)
    assert clear.mean() >= 0.97
    assert cls[3] == cls[7] and bits(sc)[3] == bits(sc)[7]  # duplicate rows
    assert same_bits(cls, again[0]) and same_bits(sc, again[1])


# ---- 2. degenerate inputs ---------------------------------------------------------------------
def test_assign_degenerate_inputs():
    V, d = 200, 40
    rows = K.random_rows(V, d, 5)
    rows[10] = 0.0
    rows[20, 5] = np.nan
    rows[30, 39] = np.inf
    cen = K.random_centroids(9, d, 15)
    cen[5] = cen[2]   # a bit copy: never chosen
    cen[0] = 0.0      # takes no rows
    cen[7, 3] = np.nan
    with NearestIndex.from_matrix(rows) as index:
        cls, sc = index.assign(cen)
        K.check_assign(rows, cen, cls, sc, d)
        assert not np.isin(cls, [0, 5, 7]).any()
        assert cls[10] == 1 and sc[10] == 0.0  # the zero row: the lowest valid class
        assert cls[20] == -1 and cls[30] == -1 and np.isneginf(sc[[20, 30]]).all()
        assert (cls >= 0).sum() == V - 2
        bad = np.zeros((3, d), np.float32)
        bad[1, 0] = np.nan
        bad[2, 1] = np.inf
        cls, sc = index.assign(bad)  # no valid centroid
        assert np.all(cls == -1) and np.isneginf(sc).all()
        cls, sc = index.assign(cen[1:2])  # K 1
        K.check_assign(rows, cen[1:2], cls, sc, d)
        assert set(cls.tolist()) == {0, -1}
        many = K.random_centroids(V, d, 16)  # K = n_rows
        cls, sc = index.assign(many)
        K.check_assign(rows, many, cls, sc, d)
        # every row starts as its own class: the zero row's own centroid is zero, so it goes to class 0; row 7
        # ties exactly with its copy, row 3, and goes to class 3; nothing else moves (own cosine 1, others far)
        r = index.classes(V, 3)
        want = np.arange(V, dtype=np.int32)
        want[[20, 30]] = -1
        want[10], want[7] = 0, 3
        assert r["classes"].tolist() == want.tolist()
        assert r["moved"].tolist() == [2, 0] and r["iterations"] == 2
        assert r["counts"][3] == 2 and r["counts"][0] == 2 and r["counts"][[7, 10, 20, 30]].tolist() == [0, 0, 0, 0]


# ---- 3. centroids against the reference -------------------------------------------------------
@pytest.mark.parametrize("V,d,k", [(1031, 48, 17), (700, 300, 17), (600, 700, 300)])
def test_centroids_match_reference(V, d, k):
    """Whole rows per workgroup; four column slabs (few classes, d 300); slabs wider than 256 columns (d 700)."""
    rows = K.random_rows(V, d, 6)
    rng = np.random.default_rng(26)
    cls = rng.integers(-1, k, V).astype(np.int32)
    cls[cls == 4] = 5        # class 4 is empty
    cls[cls == 9] = 10
    cls[200:215] = -1        # members of nothing
    cls[100] = 9             # class 9 has one member
    rows[50, 7] = np.nan
    cls[50] = 2              # a NaN row given to a class by the caller: left out
    assert (cls == -1).sum() > 10
    ref, ref_counts, sums = K.update(rows, cls, k)
    with NearestIndex.from_matrix(rows) as index:
        cen, counts = index.centroids(cls, k)
        again = index.centroids(cls, k)
    assert same_bits(cen, again[0]) and same_bits(counts, again[1])
    assert counts.dtype == np.int64 and np.array_equal(counts, ref_counts)
    assert counts[4] == 0 and counts[9] == 1 and counts[2] == (cls == 2).sum() - 1
    assert np.all(cen[4] == 0.0)
    assert np.abs(cen[9] - unit64(rows[100])[0]).max() <= tol(d)
    fin = K.finite_rows(rows)
    for c in range(k):
        if counts[c] == 0:
            continue
        member = (cls == c) & fin
        A = np.abs(rows[member].astype(np.float64)).sum(axis=0)
        bound = 2 * (counts[c] + 16) * 2.0 ** -24 * np.linalg.norm(A) / np.linalg.norm(sums[c])
        err = np.linalg.norm(cen[c].astype(np.float64) - ref[c])
        assert err <= bound, f"class {c}: {err:.3g} > {bound:.3g}"


# ---- 4. the full run equals the reference exactly on planted data ------------------------------
@pytest.mark.parametrize("shape", K.PLANTED_SHAPES, ids=["d48", "d300"])
def test_classes_equal_reference_on_planted_data(shape):
    x, _ = K.planted(**shape)
    k, d = shape["K"], shape["d"]
    ref = K.run(x, k, 10)
    assert min(ref["gaps"]) > 100 * tol(d)  # on the reference alone: no rounding can flip a row
    with NearestIndex.from_matrix(x) as index:
        got = index.classes(k, 10)
        one = index.classes(k, 1) if d == 48 else None
    assert np.array_equal(got["classes"], ref["classes"])
    assert got["moved"].tolist() == ref["moved"].tolist() and got["iterations"] == ref["iterations"] < 10
    assert np.array_equal(got["counts"], ref["counts"])
    K.check_assign(x, got["centroids"], got["classes"], got["scores"], d)
    if one is not None:
        ref1 = K.run(x, k, 1)
        assert one["iterations"] == 1 and one["moved"].tolist() == ref1["moved"].tolist()
        assert np.array_equal(one["classes"], ref1["classes"])


# ---- 5, 6. the full run on random rows; composition --------------------------------------------
@pytest.fixture(scope="module")
def random_case():
    V, d, k = 5000, 100, 37
    rows = K.random_rows(V, d, 8)
    index = NearestIndex.from_matrix(rows)
    yield rows, k, index
    index.close()


def test_classes_on_random_rows(random_case):
    rows, k, index = random_case
    d = rows.shape[1]
    a, b = index.classes(k, 10), index.classes(k, 10)
    t = class_times()  # the device time of the last run's two steps
    assert 0 < t["update_ms"] < 1e3 and 0 < t["assign_ms"] < 1e3
    for key in ("classes", "scores", "centroids", "counts", "moved"):
        assert same_bits(a[key], b[key]), key
    assert a["iterations"] == b["iterations"] == 10 and np.all(a["moved"] > 0)
    K.check_assign(rows, a["centroids"], a["classes"], a["scores"], d)
    cls, sc = index.assign(a["centroids"])
    assert same_bits(cls, a["classes"]) and same_bits(sc, a["scores"])
    assert np.array_equal(a["counts"], np.bincount(a["classes"], minlength=k))
    assert a["classes"][3] == a["classes"][7] and bits(a["scores"])[3] == bits(a["scores"])[7]


@pytest.mark.parametrize("iterations", [1, 2, 3, 4])
def test_classes_is_the_composition_of_the_steps(random_case, iterations):
    rows, k, index = random_case
    whole = index.classes(k, iterations)
    cls = (np.arange(len(rows)) % k).astype(np.int32)
    moved = []
    for _ in range(iterations):
        cen, _ = index.centroids(cls, k)
        new, sc = index.assign(cen)
        moved.append(int((new != cls).sum()))
        cls = new
    _, counts = index.centroids(cls, k)
    assert whole["iterations"] == iterations and whole["moved"].tolist() == moved
    assert same_bits(whole["classes"], cls) and same_bits(whole["scores"], sc)
    assert same_bits(whole["centroids"], cen) and same_bits(whole["counts"], counts)


# ---- 7. attached index --------------------------------------------------------------------------
def test_attached_index_equals_owned():
    """An attached d 100 matrix (the trainer's pitch is 128 floats, the scores cover 112 columns), W and C.
    No training: the uploaded rows are clustered."""
    from word2vec_amd.device import Config, DeviceTrainer

    V, d = 700, 100
    W, Cm = K.random_rows(V, d, 9), K.random_rows(V, d, 10)
    dev = DeviceTrainer(Config(word_dim=d, window=5, negative=5, hs=False, cbow=False, table_size=10_000))
    try:
        dev.upload_vocab(np.ones(V, np.float32), np.linspace(0, 10_000, V + 1).astype(np.int64))
        dev.upload_model(W, Cm, None)
        assert dev.row_pitch() == 128
        for which, M in ((0, W), (1, Cm)):
            with NearestIndex.attach(dev, which) as att, NearestIndex.from_matrix(M) as own:
                a, b = att.classes(12), own.classes(12)
            for key in ("classes", "scores", "centroids", "counts", "moved"):
                assert same_bits(a[key], b[key]), (which, key)
            assert a["iterations"] == b["iterations"] and a["moved"][0] > 0
    finally:
        dev.close()


# ---- 8. bad arguments ----------------------------------------------------------------------------
def test_bad_arguments_are_refused(random_case):
    rows, k, index = random_case
    V, d = rows.shape
    lim = class_limits()
    assert lim == {"max_classes": 65536, "max_iterations": 1000}
    cen = K.random_centroids(k, d, 18)
    ok_cls = np.zeros(V, np.int32)
    calls = [lambda: index.classes(0), lambda: index.classes(V + 1), lambda: index.classes(lim["max_classes"] + 1),
             lambda: index.classes(k, 0), lambda: index.classes(k, lim["max_iterations"] + 1),
             lambda: index.assign(np.zeros((0, d), np.float32)), lambda: index.centroids(ok_cls, 0),
             lambda: index.centroids(ok_cls, V + 1), lambda: index.centroids(ok_cls + k, k),
             lambda: index.centroids(ok_cls - 2, k)]
    for call in calls:
        with pytest.raises(RuntimeError) as e:
            call()
        assert e.value.code == N.W2V_ERR_ARG
    lib = index.lib
    assert lib.w2v_nn_classes(index.x, k, 1, None, None, None, None, None, None) == N.W2V_ERR_ARG  # null class output
    assert b"null class output" in lib.w2v_dev_last_error()
    assert lib.w2v_nn_assign(index.x, cen.ctypes.data, k, None, None) == N.W2V_ERR_ARG
    with pytest.raises(ValueError, match="centroids"):
        index.assign(np.zeros((k, d + 1), np.float32))
    with pytest.raises(ValueError, match="classes"):
        index.centroids(ok_cls[:-1], k)
    cls, sc = index.assign(cen)  # the index still answers
    K.check_assign(rows, cen, cls, sc, d)
