"""The nearest-neighbour checker bites (tests/nn_ref.py), and what the query
side guarantees without a GPU: the limits, argument validation before any
device call, and evaluate.analogy_accuracy's unchanged numpy path."""
import ctypes
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import nn_ref as R

D, V, NQ, K = 24, 400, 12, 5


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(4)
    rows = rng.standard_normal((V, D)).astype(np.float32)
    ids = rng.integers(0, V, size=(NQ, 3))
    excl = ids.astype(np.int32)
    cos = R.cosines(rows, R.queries_from_rows(rows, ids, (1.0, -1.0, 1.0)))
    ref_ids, ref_sc = R.reference_topk(cos, K, excl)
    clear = R.gaps_clear(cos, K, D, excl)
    assert clear.all()  # d 24, V 400: gaps ~1e-2 against 2 tol = 9.5e-6
    return cos, excl, ref_ids, ref_sc.astype(np.float32)


def test_checker_accepts_the_reference(case):
    cos, excl, ids, sc = case
    R.check(cos, ids, sc, D, excl)
    # ... and a restricted, under-full answer with its fillers
    ids5, sc5 = R.reference_topk(cos, K, None, restrict=3)
    assert np.all(ids5[:, 3:] == -1) and np.all(np.isneginf(sc5[:, 3:]))
    R.check(cos, ids5, sc5.astype(np.float32), D, None, restrict=3)


def _rejected(case, ids, sc):
    cos, excl, _, _ = case
    with pytest.raises(AssertionError):
        R.check(cos, ids, sc, D, excl)


def test_checker_rejects_a_dropped_best(case):
    cos, excl, _, _ = case
    ids6, sc6 = R.reference_topk(cos, K + 1, excl)
    _rejected(case, ids6[:, 1:].copy(), sc6[:, 1:].astype(np.float32))


def test_checker_rejects_swapped_entries(case):
    _, _, ids, sc = case
    ids, sc = ids.copy(), sc.copy()
    ids[2, [1, 3]] = ids[2, [3, 1]]
    sc[2, [1, 3]] = sc[2, [3, 1]]
    _rejected(case, ids, sc)
    ids2 = case[2].copy()  # ids alone: each score now belongs to another row
    ids2[2, [1, 3]] = ids2[2, [3, 1]]
    _rejected(case, ids2, case[3])


def test_checker_rejects_an_excluded_id(case):
    cos, excl, ids, sc = case
    ids, sc = ids.copy(), sc.copy()
    ids[5, 0] = excl[5, 0]
    sc[5, 0] = np.float32(cos[5, excl[5, 0]])
    _rejected(case, ids, sc)


def test_checker_rejects_a_score_off_by_three_tol(case):
    _, _, ids, sc = case
    for sign in (1.0, -1.0):
        s = sc.copy()
        s[7, 2] = np.float32(s[7, 2] + sign * 3 * R.tol(D))
        _rejected(case, ids, s)


def test_checker_rejects_a_repeat_and_a_wrong_fill(case):
    cos, _, ids, sc = case
    ids = ids.copy()
    ids[0, 1] = ids[0, 0]
    _rejected(case, ids, sc)
    ids5, sc5 = R.reference_topk(cos, K, None, restrict=3)
    ids5[1, 4] = 7  # a row past the restriction in a filler slot
    with pytest.raises(AssertionError):
        R.check(cos, ids5, sc5.astype(np.float32), D, None, restrict=3)


def test_nn_limits():
    from word2vec_amd import nn

    assert nn.limits() == {"max_dim": 2048, "max_k": 64, "max_terms": 8}


def test_nn_create_rejects_bad_arguments_without_gpu():
    """Argument validation runs before any HIP call, so it is testable here."""
    from word2vec_amd import _native as N

    lib = N.load_dev_lib()
    m = np.zeros((4, 8), np.float32)
    p = m.ctypes.data_as(ctypes.c_void_p)
    for rows, n_rows, dim, word in ((p, 4, 0, b"dim"), (p, 4, 2049, b"dim"), (p, 0, 8, b"n_rows"),
                                    (None, 4, 8, b"null matrix")):
        x = ctypes.c_void_p()
        assert lib.w2v_nn_create(0, rows, n_rows, dim, ctypes.byref(x)) == N.W2V_ERR_ARG
        assert word in lib.w2v_dev_last_error()
        assert not x.value
    assert lib.w2v_nn_set_strip_rows(None, 16) == N.W2V_ERR_ARG
    assert lib.w2v_nn_query_rows(None, None, None, 1, 0, 0, 1, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_nn_attach(None, 0, ctypes.byref(ctypes.c_void_p())) == N.W2V_ERR_ARG


def test_analogy_accuracy_default_is_the_numpy_path():
    """index=None: the result of the dense numpy path on a small fixed case (three of the
    four questions hold by construction, one has its answer outside `restrict`)."""
    from word2vec_amd.evaluate import analogy_accuracy

    words = ["king", "queen", "man", "woman", "paris", "france", "rome", "italy", "x"]
    g, r, c = np.eye(6, dtype=np.float32)[:3]
    cap, cty, fr, it = np.eye(6, dtype=np.float32)[[3, 4, 5, 2]]
    vecs = np.stack([r + g * 0, r + g, 0.5 * c + g * 0, 0.5 * c + g, cap + fr, cty + fr, cap + it + r * 0, cty + it + r * 0,
                     np.ones(6, np.float32)]).astype(np.float32)
    qs = [("man", "woman", "king", "queen"), ("king", "queen", "man", "woman"), ("paris", "france", "rome", "italy"),
          ("paris", "france", "rome", "x"), ("paris", "france", "rome", "nope")]
    got = analogy_accuracy(words, vecs, qs)
    assert got == {"accuracy": 75.0, "correct": 3, "answered": 4, "skipped": 1}
    assert analogy_accuracy(words, vecs, qs, index=None) == got
    assert analogy_accuracy(words, vecs, qs, restrict=4) == {"accuracy": 100.0, "correct": 2, "answered": 2,
                                                             "skipped": 3}


@pytest.mark.parametrize("header", ["w2v_dev.h", "w2v_model.h", "w2v_ingest.h"])
def test_c_headers_compile_as_c(header, tmp_path):
    """The C-ABI headers are for C callers (cgo, FFI generators): no C++-only construct, no C keyword as a name."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    inc = Path(__file__).resolve().parents[1] / "include"
    src = tmp_path / "use.c"
    src.write_text(f'#include "{header}"\nint main(void) {{ return 0; }}\n')
    r = subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", f"-I{inc}", str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
