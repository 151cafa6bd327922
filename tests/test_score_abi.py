"""The scoring entry points of include/w2v_dev.h exist, are bound, report their
limits and refuse bad arguments before any device call (no GPU needed)."""
import ctypes as C

import pytest

from word2vec_amd import _native as N

NAMES = ("w2v_dev_score_limits", "w2v_dev_set_score_item", "w2v_dev_score")


def test_symbols_exist_and_are_bound():
    lib = N.load_dev_lib()
    for n in NAMES:
        assert n in N.SIGNATURES, n
        assert getattr(lib, n).argtypes == N.SIGNATURES[n][1]
    assert C.sizeof(N.ScoreSummary) == 8 * 8
    assert [k for k, _ in N.ScoreSummary._fields_] == ["sentences", "words", "centers", "contexts", "targets",
                                                       "draws", "nonfinite", "ll"]


def test_limits():
    lib = N.load_dev_lib()
    d, w, n = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.w2v_dev_score_limits(C.byref(d), C.byref(w), C.byref(n)) == N.W2V_OK
    assert (d.value, w.value, n.value) == (2048, 127, 63)
    assert lib.w2v_dev_score_limits(None, None, None) == N.W2V_OK  # any pointer may be NULL
    assert lib.w2v_dev_score_limits(None, C.byref(w), None) == N.W2V_OK and w.value == 127


def test_null_handles_are_refused_with_a_message():
    lib = N.load_dev_lib()
    assert lib.w2v_dev_set_score_item(None, 64) == N.W2V_ERR_ARG
    assert b"null handle" in lib.w2v_dev_last_error()
    sm = N.ScoreSummary()
    assert lib.w2v_dev_score(None, None, 0, None, 0, 0, None, None, C.byref(sm)) == N.W2V_ERR_ARG
    assert b"w2v_dev_score" in lib.w2v_dev_last_error()


@pytest.mark.parametrize("item", [-64, 1, 63, 100])
def test_bad_item_is_refused_with_a_message(item):
    """The item is checked before the handle, so the refusal needs no device."""
    lib = N.load_dev_lib()
    assert lib.w2v_dev_set_score_item(None, item) == N.W2V_ERR_ARG
    assert b"multiple of 64" in lib.w2v_dev_last_error()
