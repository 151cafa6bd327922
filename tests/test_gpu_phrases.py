"""Phrase detection on the GPU (include/w2v_ingest.h, w2v_phrase_*; DESIGN.md
§4.6) against tests/phrase_ref.py, bit for bit: the eligible pairs and their
counts, the joins (through the rewritten stream), the phrases in id order, the
per-id counts and first positions and the summary — on a Zipf stream whose ids
pass 2^16, candidate runs thousands long that cross every wave, workgroup and
scan-tile boundary (both parities, and cut by a sentence boundary), sentence
and min_count boundaries, thresholds tied with an achieved score, a pair table
that starts at 64 slots, two and three passes, the map to samples and the
hand-over to a training handle."""
import numpy as np
import pytest

from tests import phrase_ref as R
from tests.test_corpus_file import _write_corpus
from tests.test_gpu_ingest import make_trainer_for

pytestmark = pytest.mark.gpu


def _open(stream, initial_slots=0):
    from word2vec_amd.phrases import GpuPhrases

    ids, off, n_words = stream
    return GpuPhrases.from_ids(ids, off, n_words, device=0, initial_slots=initial_slots)


def _outputs(p):
    return dict(summary=p.summary(), bigrams=p.bigrams(), phrases=p.phrases(), words=p.words(), stream=p.stream())


def _check(p, ref, n_sentences):
    """Everything the handle reports after a pass equals the reference's pass `ref`."""
    got = _outputs(p)
    for g, want, what in zip(got["bigrams"], (ref.bg_left, ref.bg_right, ref.bg_count), ("left", "right", "count")):
        np.testing.assert_array_equal(g, want, err_msg=f"bigram {what}")
    np.testing.assert_array_equal(got["stream"][1], ref.offsets, err_msg="offsets")
    np.testing.assert_array_equal(got["stream"][0], ref.ids, err_msg="ids")
    np.testing.assert_array_equal(got["words"][0], ref.count, err_msg="count")
    np.testing.assert_array_equal(got["words"][1], ref.first, err_msg="first")
    assert got["summary"]["n_words"] == ref.n_words and got["summary"]["n_ids"] == ref.ids.size
    assert got["summary"]["n_sentences"] == n_sentences
    assert got["summary"]["n_bigrams"] == ref.bg_count.size and got["summary"]["n_joined"] == ref.n_joined
    return got


def _run_and_check(stream, passes, initial_slots=0):
    p = _open(stream, initial_slots)
    refs = R.run_passes(*stream, passes)
    left, right, joined = [], [], []
    for (mc, thr), ref in zip(passes, refs):
        p.run(mc, thr)
        got = _check(p, ref, len(stream[1]) - 1)
        left.append(ref.left), right.append(ref.right), joined.append(ref.joined)
        for g, want in zip(got["phrases"], (left, right, joined)):
            np.testing.assert_array_equal(g, np.concatenate(want))
        assert got["summary"]["n_phrases"] == sum(x.size for x in left)
    return p, refs


def test_zipf_stream():
    p, (ref,) = _run_and_check(R.zipf_stream(), ((5, 50.0),))
    assert ref.left.size > 100 and p.times()["table_slots"] >= 2 * ref.bg_count.size
    p.close()


@pytest.mark.parametrize("variant", ["even", "shift", "cut"])
def test_long_candidate_runs(variant):
    p, _ = _run_and_check(R.alternating_stream(variant), ((2, 1.0),))
    p.close()


def test_boundaries():
    ids, off, words = R.boundary_stream()
    p, _ = _run_and_check((ids, off, len(words)), ((R.BOUNDARY_MIN_COUNT, 0.0),))
    p.close()


def test_empty_stream_and_sentences():
    p, _ = _run_and_check((np.zeros(0, np.int32), np.zeros(4, np.int64), 3), ((1, 0.0),))
    p.close()


def test_threshold_ties():
    """An achieved score as the threshold: its pairs do not join (strict compare); one ulp lower, they do."""
    stream = R.zipf_stream()
    base = R.pass_vec(*stream, 5, 50.0)
    above = np.sort(base.bg_score[base.bg_score > 50.0])
    s = float(above[above.size // 2])
    tied = set(zip(base.bg_left[base.bg_score == np.float32(s)], base.bg_right[base.bg_score == np.float32(s)]))
    assert tied
    for thr, joins in ((s, False), (float(np.nextafter(np.float32(s), np.float32(-np.inf))), True)):
        p = _open(stream)
        p.run(5, thr)
        ref = R.pass_vec(*stream, 5, thr)
        _check(p, ref, len(stream[1]) - 1)
        left, right, _ = p.phrases()
        assert bool(tied & set(zip(left, right))) == joins
        p.close()


def test_table_growth_and_determinism():
    """From 64 slots the table doubles many times; nothing depends on it, and two runs are bit-identical."""
    stream = R.zipf_stream()
    runs = []
    for slots in (0, 64, 64):
        p = _open(stream, slots)
        p.run(5, 50.0)
        runs.append(_outputs(p))
        slots_used = p.times()["table_slots"]
        assert slots_used >= 2 * runs[-1]["summary"]["n_bigrams"] and slots_used & (slots_used - 1) == 0
        p.close()
    for other in runs[1:]:
        assert other["summary"] == runs[0]["summary"]
        for k in ("bigrams", "phrases", "words", "stream"):
            for a, b in zip(runs[0][k], other[k]):
                assert a.tobytes() == b.tobytes(), k


def test_two_and_three_passes():
    p, refs = _run_and_check(R.multipass_stream(), R.MULTIPASS)
    left, right, _ = p.phrases()
    base = 2_020
    assert np.any(left[refs[0].left.size:] >= base)           # later phrases are made of earlier phrase ids
    count, first = p.words()
    assert count[2_001] == 0 and first[2_001] == -1            # every occurrence absorbed
    p.close()


def test_map_and_adopt():
    """Samples through an index that drops some ids and merges two; train_words is the pre-drop length;
    a training handle that adopts them trains the same words as one that uploads them."""
    import torch

    stream = R.multipass_stream()
    p = _open(stream)
    for mc, thr in R.MULTIPASS[:2]:
        p.run(mc, thr)
    ref = R.run_passes(*stream, R.MULTIPASS[:2])[-1]
    order = np.argsort(-ref.count, kind="stable")
    index = np.full(ref.n_words, -1, np.int32)
    keep = order[ref.count[order] >= 5]
    index[keep] = np.arange(keep.size)
    index[keep[3]] = index[keep[2]]                            # two ids, one vocab index
    index[keep[-1]] = -1
    p.map(index)
    ids, off, tw = p.samples()
    want_ids, want_off, want_tw = R.map_samples(ref.ids, ref.offsets, index)
    np.testing.assert_array_equal(off, want_off)
    np.testing.assert_array_equal(ids, want_ids)
    assert tw == want_tw == ref.ids.size and ids.size < tw
    counts = np.maximum(np.bincount(ids, minlength=keep.size), 1).astype(np.int64)
    ta, tb = make_trainer_for(counts), make_trainer_for(counts)
    ta.adopt_phrases(p)
    tb.upload_corpus(ids, off, tw)
    sa, sb = ta.train_epoch(0), tb.train_epoch(0)
    assert sa["words"] == sb["words"] and sa["sentences"] == sb["sentences"]
    assert ta.policy() == tb.policy()
    torch.cuda.synchronize()
    p.close()


def test_from_ids_and_from_ingest_agree(tmp_path):
    from word2vec_amd.ingest import GpuIngest
    from word2vec_amd.phrases import GpuPhrases

    path = tmp_path / "corpus.txt"
    text = R.plant_text(_write_corpus(path, 3_000, seed=11), [("new", "york"), ("san", "jose", "ca")], 40, seed=4)
    path.write_text(text)
    g = GpuIngest(path, "lines", device=0, chunk_bytes=65_536)
    words = [w for w, _ in g.count()]
    g.map({w: i for i, w in enumerate(words)})
    ids, off, tw = g.samples()
    want_ids, want_off, want_words = R.from_text(text)
    assert words == want_words
    np.testing.assert_array_equal(ids, want_ids)
    a = GpuPhrases.from_ingest(g, device=0)
    g.close()
    b = GpuPhrases.from_ids(ids, off, len(words), device=0)
    ref = R.pass_vec(ids, off, len(words), 5, 20.0)
    assert ref.left.size > 0
    for p in (a, b):
        p.run(5, 20.0)
        _check(p, ref, off.size - 1)
        p.close()
