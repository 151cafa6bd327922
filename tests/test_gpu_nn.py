"""Nearest-neighbour and analogy queries on the GPU (word2vec_amd/nn.py over
include/w2v_dev.h w2v_nn_*) against the float64 reference and checker of
tests/nn_ref.py. Rows are default_rng(seed).standard_normal with row 7 an
exact copy of row 3. An owned index pads its rows to a multiple of 16 floats
(d 100 -> 112, d 700 -> 704: the streaming kernel past 512); the attached one
uses the trainer's pitch (d 100 -> 128)."""
import numpy as np
import pytest

from tests import nn_ref as R
from word2vec_amd import _native as N
from word2vec_amd.nn import NearestIndex

pytestmark = pytest.mark.gpu


def make_rows(V, d, seed):
    rows = np.random.default_rng(seed).standard_normal((V, d)).astype(np.float32)
    rows[7] = rows[3]
    return rows


def assert_matches_reference(cos, ids, sc, k, d, exclude=None, restrict=0, min_clear=0.0):
    """The full checker, and list equality where every reference gap of the top k + 1 exceeds 2 tol."""
    R.check(cos, ids, sc, d, exclude, restrict)
    clear = R.gaps_clear(cos, k, d, exclude, restrict)
    assert clear.mean() >= min_clear, f"only {clear.mean():.2f} of the queries have clear gaps"
    ref_ids, _ = R.reference_topk(cos, k, exclude, restrict)
    assert np.array_equal(ids[clear], ref_ids[clear])
    return clear


@pytest.fixture(scope="module")
def analogy_case():
    """V 5000, d 100, nq 256, k 10: the by-row analogy form (b, a, c) / (1, -1, 1)."""
    V, d, nq = 5000, 100, 256
    rows = make_rows(V, d, 1)
    ids = np.random.default_rng(11).integers(0, V, size=(nq, 3)).astype(np.int32)
    cos = R.cosines(rows, R.queries_from_rows(rows, ids, (1.0, -1.0, 1.0)))
    index = NearestIndex.from_matrix(rows)
    yield rows, ids, cos, index
    index.close()


def test_analogy_rows_match_reference(analogy_case):
    rows, ids, cos, index = analogy_case
    k, d = 10, rows.shape[1]
    clear = R.gaps_clear(cos, k, d, ids)
    assert clear.mean() >= 0.80  # on the reference alone; measured 0.94 or more
    index.set_strip_rows(0)
    got_ids, got_sc = index.query_rows(ids, (1.0, -1.0, 1.0), k=k)
    assert_matches_reference(cos, got_ids, got_sc, k, d, exclude=ids, min_clear=0.80)
    plan = index.plan()
    assert plan["strips"] >= 2 and plan["query_block"] >= 16 and plan["strip_rows"] % 16 == 0


def test_strip_rows_and_repeats_are_bit_identical(analogy_case):
    _, ids, _, index = analogy_case
    outs = []
    for strip in (16, 48, 1008, 0):
        index.set_strip_rows(strip)
        for _ in range(2):
            outs.append(index.query_rows(ids, (1.0, -1.0, 1.0), k=10))
        if strip:
            assert index.plan()["strip_rows"] == strip
    index.set_strip_rows(0)
    for got_ids, got_sc in outs[1:]:
        assert np.array_equal(got_ids, outs[0][0])
        assert np.array_equal(got_sc.view(np.uint32), outs[0][1].view(np.uint32))


def test_vectors_tail_tile_partial_block_max_k():
    """V 1031 (prime), d 48, nq 17, k 64, random non-unit query vectors, two exclusions each."""
    V, d, nq, k = 1031, 48, 17, 64
    rows = make_rows(V, d, 2)
    rng = np.random.default_rng(12)
    q = (rng.standard_normal((nq, d)) * rng.uniform(0.01, 30.0, size=(nq, 1))).astype(np.float32)
    cos = R.cosines(rows, q)
    top2 = R.reference_topk(cos, 2)[0]
    excl = np.stack([top2[:, 0], np.full(nq, -1)], axis=1).astype(np.int32)  # the best row, and a "none"
    excl[3] = (1030, 1029)
    with NearestIndex.from_matrix(rows) as index:
        ids, sc = index.query_vectors(q, k=k, exclude=excl)
        assert_matches_reference(cos, ids, sc, k, d, exclude=excl)
        assert not np.any(ids == excl[:, :1])
        index.set_strip_rows(16)  # 65 strips, the last one 7 rows
        ids2, sc2 = index.query_vectors(q, k=k, exclude=excl)
        assert np.array_equal(ids, ids2) and np.array_equal(sc.view(np.uint32), sc2.view(np.uint32))


# 4, 7, 8, 13, 16, 19, 20, 24, 32 and 33 blocks of 16 columns: every instantiated resident width, and the
# streaming kernel
INSTANCE_WIDTHS = [64, 112, 128, 208, 256, 304, 320, 384, 512, 528]


@pytest.mark.parametrize("d", INSTANCE_WIDTHS)
def test_every_instantiated_width(d):
    """V 333 (a tail tile), nq 40 (a partial query block), k 5, random non-unit query vectors, at each width."""
    V, nq, k = 333, 40, 5
    rows = make_rows(V, d, 2)
    rng = np.random.default_rng(12)
    q = (rng.standard_normal((nq, d)) * rng.uniform(0.01, 30.0, size=(nq, 1))).astype(np.float32)
    cos = R.cosines(rows, q)
    with NearestIndex.from_matrix(rows) as index:
        ids, sc = index.query_vectors(q, k=k)
        # on the reference alone 0.85 (d 528) to 1.00 of the queries have clear gaps
        assert_matches_reference(cos, ids, sc, k, d, min_clear=0.80)
        assert index.plan()["query_block"] == (128 if d <= 320 else 64)
        index.set_strip_rows(16)  # 21 strips, the last one 13 rows
        ids2, sc2 = index.query_vectors(q, k=k)
        assert np.array_equal(ids, ids2) and np.array_equal(sc.view(np.uint32), sc2.view(np.uint32))


def test_wide_rows_padding_and_long_k_loop():
    """V 3000, d 700 (padded to 704: the kernel without resident query fragments), nq 64, k 10."""
    V, d, nq, k = 3000, 700, 64, 10
    rows = make_rows(V, d, 3)
    ids = np.random.default_rng(13).integers(0, V, size=(nq, 1)).astype(np.int32)
    cos = R.cosines(rows, R.queries_from_rows(rows, ids, 1.0))
    with NearestIndex.from_matrix(rows) as index:
        got_ids, got_sc = index.query_rows(ids, k=k)
        # (2 tol = 1.7e-4 at d 700: about half of the queries have all ten gaps clear, on the reference alone)
        assert_matches_reference(cos, got_ids, got_sc, k, d, exclude=ids, min_clear=0.40)
        v_ids, v_sc = index.query_vectors(rows[ids[:, 0]] * 3.0, k=k, exclude=ids)  # the same queries as vectors
        assert_matches_reference(cos, v_ids, v_sc, k, d, exclude=ids, min_clear=0.40)


@pytest.fixture(scope="module")
def restrict_case():
    V, d, nq = 5000, 300, 33
    rows = make_rows(V, d, 4)
    ids = np.random.default_rng(14).integers(0, V, size=(nq, 3)).astype(np.int32)
    cos = R.cosines(rows, R.queries_from_rows(rows, ids, (1.0, -1.0, 1.0)))
    index = NearestIndex.from_matrix(rows)
    yield rows, ids, cos, index
    index.close()


@pytest.mark.parametrize("restrict", [1000, 1003])
def test_restrict_masks_mid_tile(restrict_case, restrict):
    rows, ids, cos, index = restrict_case
    got_ids, got_sc = index.query_rows(ids, (1.0, -1.0, 1.0), k=40, restrict=restrict)
    assert got_ids.max() < restrict
    assert_matches_reference(cos, got_ids, got_sc, 40, rows.shape[1], exclude=ids, restrict=restrict)


def test_restrict_below_k_fills_with_minus_one(restrict_case):
    rows, ids, cos, index = restrict_case
    ids = ids.copy()
    ids[0] = (100, 200, 300)  # no term among the five candidates: exactly five fillers
    cos = cos.copy()
    cos[0] = R.cosines(rows, R.queries_from_rows(rows, ids[:1], (1.0, -1.0, 1.0)))[0]
    got_ids, got_sc = index.query_rows(ids, (1.0, -1.0, 1.0), k=10, restrict=5)
    R.check(cos, got_ids, got_sc, rows.shape[1], exclude=ids, restrict=5)
    assert np.all(got_ids[0, :5] >= 0) and np.all(got_ids[0, 5:] == -1) and np.all(np.isneginf(got_sc[0, 5:]))
    assert np.all(got_ids[:, 5:] == -1)


def test_single_query_and_bit_exact_tie(analogy_case):
    rows, _, _, index = analogy_case
    d = rows.shape[1]
    ids, sc = index.query_rows(np.array([[11]], np.int32), k=1)  # nq 1, k 1
    cos = R.cosines(rows, rows[11:12])
    assert_matches_reference(cos, ids, sc, 1, d, exclude=np.array([[11]]))
    # a query equal to row 3, nothing excluded: rows 3 and 7 are the same bits, so are their scores
    for strip in (0, 16):
        index.set_strip_rows(strip)
        ids, sc = index.query_vectors(rows[3:4], k=2)
        assert ids.tolist() == [[3, 7]]
        assert sc.view(np.uint32)[0, 0] == sc.view(np.uint32)[0, 1]
        assert abs(float(sc[0, 0]) - 1.0) <= R.tol(d)
    index.set_strip_rows(0)


def test_zero_row_zero_query_and_nan_row():
    V, d = 200, 40
    rows = make_rows(V, d, 5)
    rows[0] = 0.0
    rows[50, 3] = np.nan
    rows[120, 0] = np.inf
    q = np.zeros((2, d), np.float32)
    q[1] = rows[9]
    with NearestIndex.from_matrix(rows) as index:
        ids, sc = index.query_vectors(q, k=64)
        # the zero query: every score is 0 and the lowest ids are returned (never the non-finite rows)
        assert np.all(sc[0] == 0.0)
        assert ids[0].tolist() == [i for i in range(66) if i != 50][:64]
        cos = R.cosines(rows, q)
        R.check(cos[1:], ids[1:], sc[1:], d)
        all_ids, all_sc = index.query_vectors(q[1:], k=64, restrict=0)
        assert 50 not in all_ids and 120 not in all_ids
        # the zero row scores exactly 0 against any query
        z_ids, z_sc = index.query_vectors(q[1:], k=5, restrict=1)
        assert z_ids[0].tolist() == [0, -1, -1, -1, -1] and z_sc[0, 0] == 0.0
        # by row: a query made of the zero row alone is the zero query
        r_ids, r_sc = index.query_rows(np.array([[0]], np.int32), k=3)
        assert r_ids[0].tolist() == [1, 2, 3] and np.all(r_sc == 0.0)


def test_attach_and_refresh_follow_the_trainer():
    from tests.corpus import zipf_sentences
    from tests.harness import device_config, device_from_oracle, oracle_run

    sents = zipf_sentences(4, 150, 120, seed=3)
    o = oracle_run(sents, "sg_ns", dim=100, window=5, iters=1, table_size=10_000)
    cfg = device_config(o, "sg_ns", 100, 5, 1, 10_000, True, 0.05, 2.5e-6)
    dev = device_from_oracle(o, cfg, initial=True)
    stream, offs, orders = o.stream(1)
    dev.upload_replay(stream, offs)
    dev.set_rng(N.W2V_RNG_REPLAY, 0)
    dev.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    dev.set_progress(0)
    V = dev.V
    ids = np.random.default_rng(15).integers(0, V, size=(40, 3)).astype(np.int32)
    k = min(10, V - 3)
    index = NearestIndex.attach(dev, 0)
    try:
        W0 = dev.download_model()[0]
        got = index.query_rows(ids, (1.0, -1.0, 1.0), k=k)
        R.check(R.cosines(W0, R.queries_from_rows(W0, ids, (1.0, -1.0, 1.0))), *got, 100, exclude=ids)
        dev.train_epoch(0, orders)
        W1 = dev.download_model()[0]
        assert not np.array_equal(W0, W1)
        index.refresh()
        got = index.query_rows(ids, (1.0, -1.0, 1.0), k=k)
        R.check(R.cosines(W1, R.queries_from_rows(W1, ids, (1.0, -1.0, 1.0))), *got, 100, exclude=ids)
    finally:
        index.close()
        dev.close()


def test_bad_arguments_leave_the_index_usable(analogy_case):
    rows, ids, cos, index = analogy_case
    V = rows.shape[0]
    one = ids[:4]
    bad = [
        lambda: index.query_rows(one, (1.0, -1.0, 1.0), k=0),
        lambda: index.query_rows(one, (1.0, -1.0, 1.0), k=65),
        lambda: index.query_rows(np.zeros((2, 9), np.int32), k=1),
        lambda: index.query_rows(np.array([[1, V, 2]], np.int32), (1.0, -1.0, 1.0), k=1),
        lambda: index.query_rows(one, (1.0, -1.0, 1.0), k=1, restrict=-1),
        lambda: index.query_vectors(rows[:2], k=1, restrict=-5),
        lambda: index.set_strip_rows(24),
    ]
    for call in bad:
        with pytest.raises(N.DevError) as e:
            call()
        assert e.value.code == N.W2V_ERR_ARG
    got_ids, got_sc = index.query_rows(one, (1.0, -1.0, 1.0), k=10)
    R.check(cos[:4], got_ids, got_sc, rows.shape[1], exclude=one)


def test_attach_wide_pitch_past_the_scored_columns():
    """An attached d 700 matrix: the trainer's pitch is 768 floats, the scores cover 704 columns (the kernel
    that re-reads the query fragments); C (which 1) as well as W. No training: the uploaded rows are queried."""
    from word2vec_amd.device import Config, DeviceTrainer

    V, d, k = 600, 700, 10
    W, Cm = make_rows(V, d, 6), make_rows(V, d, 7)
    dev = DeviceTrainer(Config(word_dim=d, window=5, negative=5, hs=False, cbow=False, table_size=10_000))
    try:
        dev.upload_vocab(np.ones(V, np.float32), np.linspace(0, 10_000, V + 1).astype(np.int64))
        dev.upload_model(W, Cm, None)
        assert dev.row_pitch() == 768
        ids = np.random.default_rng(16).integers(0, V, size=(20, 3)).astype(np.int32)
        for which, M in ((0, W), (1, Cm)):
            with NearestIndex.attach(dev, which) as index:
                got_ids, got_sc = index.query_rows(ids, (1.0, -1.0, 1.0), k=k)
                cos = R.cosines(M, R.queries_from_rows(M, ids, (1.0, -1.0, 1.0)))
                assert_matches_reference(cos, got_ids, got_sc, k, d, exclude=ids)
    finally:
        dev.close()


def test_plan_whose_partial_lists_pass_the_budget_is_refused():
    """16-row strips over 600,000 rows at k 64: 37,500 strips x 64 x 128 queries x 4 B = 1.2 GB per partial array
    for one query block. Refused with W2V_ERR_ARG before any launch; the automatic plan answers."""
    V, d = 600_000, 16
    rows = np.random.default_rng(8).standard_normal((V, d), dtype=np.float32)
    with NearestIndex.from_matrix(rows) as index:
        index.set_strip_rows(16)
        with pytest.raises(N.DevError, match="strip") as e:
            index.query_vectors(rows[:2], k=64)
        assert e.value.code == N.W2V_ERR_ARG
        index.set_strip_rows(0)
        ids, sc = index.query_vectors(rows[5:6], k=3)
        assert ids[0, 0] == 5 and abs(float(sc[0, 0]) - 1.0) <= R.tol(d)
