"""The inputs of tests/test_gpu_combined.py, shared with tests/test_train_ref.py,
which asserts on the CPU that each of them discriminates: that the oracle's
result with the feature under test (hs together with negative sampling, CBOW
as a sum, the alpha floor) differs from its result without it by at least 100
times the bound the GPU case is held to.

The corpora and shapes are those of the existing tests of the same kind
(tests/test_gpu_parity.py, tests/test_gpu_parallel_parity.py)."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from tests.corpus import zipf_sentences
from tests.harness import mode_config, oracle_run

# test_gpu_parity.py's classes: (norm-wise, per element)
SINGLE = (1e-5, 2e-3)
MULTI = (2e-5, 2e-3)
LIFTED = (2e-5, 5e-3)

KEY = 0x0C0B_1ED0_0000_0001

CORPORA = {
    # test_replay_single_sentence
    "single": dict(zipf=(1, 48, 400), zkw=dict(seed=3), min_count=1, table_size=10_000, window=5, seed=1234),
    # test_replay_epoch
    "epoch": dict(zipf=(12, 200, 400), zkw=dict(seed=5, ragged=True), min_count=2, table_size=100_000, window=5,
                  seed=1234),
    # test_philox_sequential_row_widths
    "widths": dict(zipf=(8, 160, 300), zkw=dict(seed=37, ragged=True), min_count=2, table_size=100_000, window=5,
                   seed=1234),
    # One sentence whose rows repeat (200 tokens over 40 types). On "single" the combined update cannot be told
    # from hs alone by synapses1, from ns alone by C (skip-gram: both see W only through a center that occurs
    # again; measured 0) or by CBOW's W (1.0e-4 to 1.5e-4, under 100 x 1e-5); here every matrix tells them apart
    # (>= 1.5e-3). tests/test_train_ref.py asserts both statements.
    "single_rep": dict(zipf=(1, 200, 40), zkw=dict(seed=3), min_count=1, table_size=10_000, window=5, seed=1234),
    # test_replay_many_negatives' shape with more tokens over fewer types: on its (4, 150, 3000) CBOW's W differs
    # from ns alone by 1.6e-3, under 100 x 2e-5; on this one every matrix differs by >= 5.5e-3
    "many_neg": dict(zipf=(6, 150, 500), zkw=dict(seed=41, ragged=True), min_count=1, table_size=100_000, window=5,
                     seed=4321),
    # test_replay_wide_window (window 40) / test_replay_huge_window (window 200)
    "wide": dict(zipf=(6, 300, 150), zkw=dict(seed=21, ragged=True), min_count=2, table_size=10_000, window=40,
                 seed=1234),
    "huge": dict(zipf=(3, 700, 300), zkw=dict(seed=45, ragged=True), min_count=2, table_size=10_000, window=200,
                 seed=1234),
    # test_gpu_parallel_parity.py's _reference
    "one_wave": dict(zipf=(60, 120, 400), zkw=dict(seed=43, ragged=True), min_count=2, table_size=100_000, window=5,
                     seed=1234),
    # test_gpu_shared.py's epochs (shared-negatives minibatch skip-gram, negative 15)
    "shared": dict(zipf=(12, 200, 300), zkw=dict(seed=23, ragged=True), min_count=2, table_size=100_000, window=5,
                   seed=1234),
}


def sentences(corpus):
    c = CORPORA[corpus]
    return zipf_sentences(*c["zipf"], **c["zkw"])


class Case(NamedTuple):
    corpus: str
    mode: str
    dim: int
    tol: tuple
    iters: int = 1
    negative: Optional[int] = None
    cw0_epochs: int = 0      # the word counter starts at cw0_epochs * iter * train_words
    shared: bool = False     # the shared-negatives kernel

    @property
    def id(self):
        return f"{self.corpus}-{self.mode}-d{self.dim}" + (f"-it{self.iters}" if self.iters > 1 else "") + \
            (f"-neg{self.negative}" if self.negative else "")


def lifted(dim):
    return LIFTED if dim > 512 else MULTI


HSNS = ("sg_hsns", "cbow_hsns")
NV_DIMS = [40, 100, 150, 200, 300, 350, 512, 700, 1000]

# hs together with negative sampling
HSNS_SINGLE = [Case(c, m, d, SINGLE) for c in ("single", "single_rep") for m in HSNS for d in (48, 100, 200, 300, 512)]
# (corpus, mode, the objective it is compared with) -> the matrices that comparison cannot tell apart
SECOND_ORDER = {("single", "sg_hsns", "hs"): "S", ("single", "sg_hsns", "ns"): "C", ("single", "cbow_hsns", "ns"): "W"}
HSNS_EPOCH = [Case("epoch", m, d, MULTI, iters=2) for m in HSNS for d in (100, 300)]
HSNS_WIDTHS = [Case("widths", m, d, lifted(d)) for m in HSNS for d in NV_DIMS] + \
              [Case("widths", "cbow_hsns", d, LIFTED) for d in (1100, 2048)]
HSNS_MANY = [Case("many_neg", m, 100, LIFTED, negative=100) for m in HSNS]
HSNS_WINDOW = [Case("wide", "cbow_hsns", 64, MULTI), Case("huge", "cbow_hsns", 48, LIFTED),
               Case("wide", "sg_hsns", 64, MULTI)]
HSNS_ONE_WAVE = [Case("one_wave", m, d, MULTI) for m in HSNS for d in (100, 300)]
HSNS_CASES = HSNS_SINGLE + HSNS_EPOCH + HSNS_WIDTHS + HSNS_MANY + HSNS_WINDOW + HSNS_ONE_WAVE

# CBOW as a sum (cbow_mean off on both sides)
SUM_MODES = ("cbow_ns", "cbow_hs", "cbow_hsns")
SUM_SINGLE = [Case("single", m, d, SINGLE) for m in SUM_MODES for d in (48, 300)]
SUM_WIDTHS = [Case("widths", m, d, lifted(d)) for m in SUM_MODES for d in (100, 300, 700)]
SUM_WINDOW = [Case(c, m, d, t) for m in SUM_MODES for c, d, t in (("wide", 64, MULTI), ("huge", 48, LIFTED))]
SUM_ONE_WAVE = [Case("one_wave", m, 300, MULTI) for m in SUM_MODES]
SUM_CASES = SUM_SINGLE + SUM_WIDTHS + SUM_WINDOW + SUM_ONE_WAVE

# the alpha floor (min_alpha 0.02 against the suite's 2.5e-6)
FLOOR_ALPHA = 0.02
# Two epochs: the schedule is under the floor at 6 (sg_ns) or 8 of the 24 sentence starts, and alpha is
# refreshed there once (the 11th sentence of the second epoch), so 2 sentences train at the floor. Three epochs:
# the schedule is under the floor from the third epoch's first sentence on, and all 12 of its 36 sentences train
# at min_alpha exactly.
FLOOR_EPOCH = [Case("epoch", m, 100, MULTI, iters=i) for i in (2, 3) for m in ("sg_ns", "sg_hs", "cbow_ns", "cbow_hs")]
FLOOR_PAST_END = [Case("widths", m, 100, MULTI, cw0_epochs=2) for m in ("sg_ns", "cbow_hs")]
FLOOR_SHARED = [Case("shared", "sg_ns", 200, (1e-4, 5e-3), iters=2, negative=15, shared=True)]
FLOOR_CASES = FLOOR_EPOCH + FLOOR_PAST_END + FLOOR_SHARED


def case_oracle(case, mode=None, cbow_mean=True, min_alpha=2.5e-6):
    """The oracle of a case before training (weights initialised, samples
    built); `mode` replaces the case's own for a comparison run."""
    c = CORPORA[case.corpus]
    if case.shared:
        return _shared_oracle(case, min_alpha)
    mode = mode or case.mode
    neg = case.negative if mode_config(mode)["negative"] > 0 else None
    o = oracle_run(sentences(case.corpus), mode, dim=case.dim, window=c["window"], iters=case.iters, seed=c["seed"],
                   min_count=c["min_count"], table_size=c["table_size"], cbow_mean=cbow_mean, min_alpha=min_alpha,
                   train=False, negative=neg)
    o.build_sample()
    return o


def _shared_oracle(case, min_alpha):
    from tests.test_gpu_shared import _oracle

    assert CORPORA[case.corpus]["min_count"] == 2 and CORPORA[case.corpus]["seed"] == 1234  # _oracle's own
    return _oracle(sentences(case.corpus), case.dim, negative=case.negative, iters=case.iters, min_alpha=min_alpha)[0]


def philox_orders(o, iters):
    n = o.samples()[1].size - 1
    return np.concatenate([np.random.default_rng(1 + e).permutation(n) for e in range(iters)])


def philox_update(case, o, init=None):
    """Train `o` in Philox mode on the case's schedule from `init` (default:
    its own start); returns (init, update) per matrix, None where the
    configuration has no such matrix."""
    if init is not None:
        for k in range(3):
            if init[k] is not None and o.matrix(k).size:
                o.set_matrix(k, init[k])
    start = [o.matrix(k) if o.matrix(k).size else None for k in range(3)]
    cw0 = case.cw0_epochs * case.iters * o.train_words
    o.train_philox(0, case.iters, philox_orders(o, case.iters), KEY, cw0)
    upd = [None if start[k] is None else o.matrix(k).astype(np.float64) - start[k] for k in range(3)]
    return start, upd
