"""The argument and state errors of the phrase calls (include/w2v_ingest.h,
w2v_phrase_*), through _native. They are checked before any device call
(w2v_phrase_create makes none), so they are testable without a GPU."""
import ctypes as C

import numpy as np
import pytest

from word2vec_amd import _native as N


@pytest.fixture()
def lib():
    return N.load_dev_lib()


@pytest.fixture()
def handle(lib):
    p = C.c_void_p()
    assert lib.w2v_phrase_create(0, C.byref(p)) == N.W2V_OK
    yield p
    lib.w2v_phrase_destroy(p)


def _upload(lib, p, ids, offsets, n_words):
    i = np.ascontiguousarray(ids, np.int32)
    o = np.ascontiguousarray(offsets, np.int64)
    return lib.w2v_phrase_upload(p, i.ctypes.data, i.size, o.ctypes.data, o.size - 1, n_words)


def test_null_arguments(lib, handle):
    assert lib.w2v_phrase_create(0, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_create(-2, C.byref(C.c_void_p())) == N.W2V_ERR_ARG
    o = np.zeros(1, np.int64)
    assert lib.w2v_phrase_upload(None, None, 0, o.ctypes.data, 0, 1) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_upload(handle, None, 0, None, 0, 1) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_upload(handle, None, 2, o.ctypes.data, 0, 1) == N.W2V_ERR_ARG
    assert b"null" in lib.w2v_dev_last_error()
    assert lib.w2v_phrase_set_table(None, 0) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_set_table(handle, -1) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_set_table(handle, 100) == N.W2V_OK
    assert lib.w2v_phrase_adopt_ingest(handle, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_adopt_ingest(None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_pass(None, 5, 1.0) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_summary(None, None, None, None, None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_times(None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_phrases(None, None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_bigrams(None, None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_words(None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_stream(None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_map(None, None, 0) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_samples_size(None, None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_phrase_download(None, None, None) == N.W2V_ERR_ARG
    assert lib.w2v_dev_adopt_phrases(None, handle) == N.W2V_ERR_ARG
    assert lib.w2v_dev_adopt_phrases(None, None) == N.W2V_ERR_ARG


def test_pass_rejects_min_count_and_threshold(lib, handle):
    for mc, thr, word in ((0, 1.0, b"min_count"), (-3, 1.0, b"min_count"), (5, -0.5, b"threshold"),
                          (5, float("nan"), b"threshold"), (5, float("inf"), b"threshold")):
        assert lib.w2v_phrase_pass(handle, mc, thr) == N.W2V_ERR_ARG
        assert word in lib.w2v_dev_last_error()


def test_upload_rejects_bad_streams(lib, handle):
    assert _upload(lib, handle, [0, 1, 2], [0, 3], 2) == N.W2V_ERR_ARG        # id == n_words
    assert b"n_words" in lib.w2v_dev_last_error()
    assert _upload(lib, handle, [0, -1, 1], [0, 3], 2) == N.W2V_ERR_ARG       # negative id
    assert _upload(lib, handle, [0, 1], [0, 3], 2) == N.W2V_ERR_ARG           # offsets past the ids
    assert _upload(lib, handle, [0, 1], [1, 2], 2) == N.W2V_ERR_ARG           # offsets do not start at 0
    assert _upload(lib, handle, [0, 1, 1], [0, 2, 1, 3], 2) == N.W2V_ERR_ARG  # decreasing offsets
    assert _upload(lib, handle, [0], [0, 1], -1) == N.W2V_ERR_ARG
    # words + phrases must stay below 2^31
    assert _upload(lib, handle, [0], [0, 1], 1 << 31) == N.W2V_ERR_ARG
    assert b"2^31" in lib.w2v_dev_last_error()


def test_calls_in_the_wrong_state(lib, handle):
    idx = np.zeros(4, np.int32)
    assert lib.w2v_phrase_pass(handle, 5, 1.0) == N.W2V_ERR_STATE             # no stream yet
    assert lib.w2v_phrase_map(handle, idx.ctypes.data, 4) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_summary(handle, None, None, None, None, None, None) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_stream(handle, None, None) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_words(handle, None, None) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_bigrams(handle, None, None, None) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_phrases(handle, None, None, None) == N.W2V_ERR_STATE
    assert lib.w2v_phrase_samples_size(handle, None, None, None) == N.W2V_ERR_STATE   # not mapped
    assert lib.w2v_phrase_download(handle, None, None) == N.W2V_ERR_STATE
    assert b"map" in lib.w2v_dev_last_error()


def test_model_refuses_the_sentence_api_in_phrase_mode():
    from word2vec_amd.model import Word2Vec

    m = Word2Vec(min_count=1, negative=5, train_method="ns", model="sg", table_size=1000, word_dim=8,
                 phrase_thresholds=[10.0], phrase_min_count=1)
    with pytest.raises(RuntimeError, match="phrase mode reads files"):
        m.build_vocab([["a", "b"], ["a", "b"]])
    with pytest.raises(RuntimeError, match="phrase mode reads files"):
        m.train([["a", "b"]])
    plain = Word2Vec(min_count=1, negative=5, train_method="ns", model="sg", table_size=1000, word_dim=8,
                     phrase_thresholds=[])
    plain.build_vocab([["a", "b"], ["a", "b"]])
    assert plain.V == 2
