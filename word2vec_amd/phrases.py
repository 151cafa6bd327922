"""Phrase detection on the GPU (include/w2v_ingest.h, w2v_phrase_*): word2phrase's
rule over a corpus that is already token ids in HBM — exact, deterministic, and
independent of the pair table's size.

    g = GpuIngest("corpus.txt", "lines"); words = [w for w, _ in g.count()]
    g.map({w: i for i, w in enumerate(words)})        # identity: every token stays
    p = GpuPhrases.from_ingest(g); g.close()
    p.run(min_count=5, threshold=200.0)               # "new york" -> one id
    p.run(min_count=5, threshold=100.0)               # ("new_york", "city") -> one id
    left, right, joined = p.phrases()                 # per phrase, in id order
    ids, offsets = p.stream()                         # the rewritten corpus
    p.map(index); trainer.adopt_phrases(p)            # the samples stay in HBM
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


class GpuPhrases:
    def __init__(self, device: int = -1, initial_slots: int = 0):
        self.lib = N.load_dev_lib()
        p = C.c_void_p()
        N.check(self.lib, self.lib.w2v_phrase_create(int(device), C.byref(p)), "w2v_phrase_create")
        self.p = p
        N.check(self.lib, self.lib.w2v_phrase_set_table(self.p, int(initial_slots)), "w2v_phrase_set_table")

    @classmethod
    def from_ids(cls, ids, offsets, n_words: int, device: int = -1, initial_slots: int = 0) -> "GpuPhrases":
        """A stream from the host: ids (int32, each in [0, n_words)), sentence offsets (int64)."""
        self = cls(device, initial_slots)
        i = np.ascontiguousarray(ids, np.int32)
        o = np.ascontiguousarray(offsets, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_upload(self.p, i.ctypes.data, i.size, o.ctypes.data, o.size - 1,
                                                     int(n_words)), "w2v_phrase_upload")
        return self

    @classmethod
    def from_ingest(cls, ingest, device: int = -1, initial_slots: int = 0) -> "GpuPhrases":
        """The samples of a mapped GpuIngest on the same device, device to device."""
        self = cls(device, initial_slots)
        N.check(self.lib, self.lib.w2v_phrase_adopt_ingest(self.p, ingest.g), "w2v_phrase_adopt_ingest")
        return self

    def run(self, min_count: int = 5, threshold: float = 100.0) -> dict:
        """One pass; returns summary()."""
        N.check(self.lib, self.lib.w2v_phrase_pass(self.p, int(min_count), float(threshold)), "w2v_phrase_pass")
        return self.summary()

    def summary(self) -> dict:
        v = [C.c_int64() for _ in range(6)]
        N.check(self.lib, self.lib.w2v_phrase_summary(self.p, *[C.byref(x) for x in v]), "w2v_phrase_summary")
        return dict(zip(("n_words", "n_phrases", "n_ids", "n_sentences", "n_bigrams", "n_joined"),
                        (x.value for x in v)))

    def times(self) -> dict:
        """Wall seconds of the last pass's steps and the pair table's final slots."""
        sec = (C.c_double * 5)()
        slots = C.c_int64()
        N.check(self.lib, self.lib.w2v_phrase_times(self.p, sec, C.byref(slots)), "w2v_phrase_times")
        out = dict(zip(("histogram", "insert", "count", "score_join", "rewrite"), (float(s) for s in sec)))
        out["table_slots"] = slots.value
        return out

    def phrases(self):
        """(left int32, right int32, joined int64) per phrase of all passes, in id order."""
        n = self.summary()["n_phrases"]
        left, right, joined = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_phrases(self.p, left.ctypes.data, right.ctypes.data, joined.ctypes.data),
                "w2v_phrase_phrases")
        return left, right, joined

    def bigrams(self):
        """(left, right, count) of the last pass's eligible pairs, by (left, right) ascending."""
        n = self.summary()["n_bigrams"]
        left, right, count = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_bigrams(self.p, left.ctypes.data, right.ctypes.data, count.ctypes.data),
                "w2v_phrase_bigrams")
        return left, right, count

    def words(self):
        """(count int64, first int64) per id of the current stream; first = -1 when count 0."""
        n = self.summary()["n_words"]
        count, first = np.empty(n, np.int64), np.empty(n, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_words(self.p, count.ctypes.data, first.ctypes.data), "w2v_phrase_words")
        return count, first

    def stream(self):
        """(ids int32, offsets int64) of the current stream, copied to the host."""
        s = self.summary()
        ids, off = np.empty(s["n_ids"], np.int32), np.empty(s["n_sentences"] + 1, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_stream(self.p, ids.ctypes.data, off.ctypes.data), "w2v_phrase_stream")
        return ids, off

    def map(self, index) -> None:
        """ids -> index[ids] (int32 per id of the stream; -1 drops the token)."""
        vi = np.ascontiguousarray(index, np.int32)
        N.check(self.lib, self.lib.w2v_phrase_map(self.p, vi.ctypes.data, vi.size), "w2v_phrase_map")

    def samples(self):
        """(ids int32, offsets int64, train_words) of map(), copied to the host."""
        ni, ns, tw = C.c_int64(), C.c_int64(), C.c_int64()
        N.check(self.lib, self.lib.w2v_phrase_samples_size(self.p, C.byref(ni), C.byref(ns), C.byref(tw)),
                "w2v_phrase_samples_size")
        ids, off = np.empty(ni.value, np.int32), np.empty(ns.value + 1, np.int64)
        N.check(self.lib, self.lib.w2v_phrase_download(self.p, ids.ctypes.data, off.ctypes.data), "w2v_phrase_download")
        return ids, off, tw.value

    def close(self):
        if getattr(self, "p", None):
            self.lib.w2v_phrase_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
