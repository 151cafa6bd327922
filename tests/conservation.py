"""Corpora, reference runs and the comparison shared by
tests/test_gpu_conservation.py (GPU) and tests/test_visit_ref.py (CPU).

Corpus A: 2048 ragged Zipf sentences of up to 64 tokens over TYPES_A types.
The vocabulary is built (min_count 1) from those sentences plus one sentence
that lists every type once, which is then cut from the training samples: V is
exactly TYPES_A, and the types the 2048 sentences never draw are vocabulary
rows that training must not touch. Corpus B: 96 sentences of 700 tokens.

Conservation (test_gpu_conservation.py section 3): with every non-private row
on atomics, every flush scale 1 and a constant small learning rate, a parallel
launch applies every update exactly once in the same g * x form as the
sequential oracle, so it differs from Oracle.train_philox only at second order
in alpha plus fp32 rounding, like the oracle run in another sentence order.
`reference` runs the oracle in three orders; `spreads` measures, per matrix
and row class, how far the other two are from the first; the bounds
(BOUNDS, below) are MARGIN times that, capped for the row classes.
"""
from __future__ import annotations

import json
import os

import numpy as np

from tests import visit_ref as vr
from tests.corpus import zipf_sentences
from tests.harness import mode_config, oracle_run, rel_err  # noqa: F401 (mode_config: re-exported)

KEY = 0xC0_45E2_7A71_0001
WINDOW, TABLE = 5, 100_000
TYPES_A, N_SENT_A = 5000, 2048
TYPES_B, N_SENT_B, LEN_B = 2000, 96, 700
PRIV_MAX, CTX_MAX = 128, 64   # kPrivMax, kCtxMax (w2v_limits.hpp)

# The constant learning rate per mode (and row width, where one value does not
# serve both) and the row norm of the random start. Both sides of every dot
# product are ~ROW_NORM long, so sigma is ~1/2 and one update moves a row by
# ~alpha / 2 of the other row. Two things separate a launch from the oracle's
# run in the same order, and the learning rate trades them:
#   second order: a hot row of corpus A takes 20 K to 250 K updates, so rows
#     read late in the epoch have moved. It grows like alpha, in the oracle's
#     spread over sentence orders as in a launch (measured: the spread x 1/4
#     from 2^-13 to 2^-15 in every class, at any row norm);
#   rounding: the oracle rounds each add at 2^-24 of the ROW, 2^-23 / alpha of
#     the update, and on a hot row the same few thousand (center, sign)
#     increments repeat, so the rounding does not average out. It is the same
#     in every sentence order: the spread does not show it, a launch (which
#     sums a private row's updates in a small LDS delta) does. At 2^-17 the
#     oracle's update of skip-gram HS's top nodes is 2.2 to 5.3 % from a
#     float64 sum of the same terms, the launch's 0.2 to 0.4 %.
# So alpha must be large enough for the second-order spread to cover the
# oracle's rounding, and small enough for the row classes' bounds to stay
# below RARE_MAX and PRIV_MAX_BOUND. Measured on the GPU at 2^-13 .. 2^-17
# (profiles/r11a_conservation.jsonl, "sweep"): skip-gram HS misses its norm-wise
# and private-range bounds at 2^-17 and 2^-16 (rounding) and its rare-row cap at
# 2^-13, and meets all at 2^-15; CBOW-NS misses one norm-wise bound at 2^-16 and
# 2^-15 and meets all at 2^-14; CBOW-HS meets all at 2^-16 (d 64) and 2^-15
# (d 300) and misses a norm-wise bound one step to either side. The row norm
# cancels in both terms (0.05 and 0.2 measured the same).
ALPHAS = {"sg_ns": 2.0 ** -15, "cbow_ns": 2.0 ** -14, "sg_hs": 2.0 ** -15, "cbow_hs": 2.0 ** -16,
          "sg_hsns": 2.0 ** -16, "cbow_hsns": 2.0 ** -16}
ALPHA_AT = {("cbow_hs", 300): 2.0 ** -15}


def alpha(mode, dim):
    return ALPHA_AT.get((mode, dim), ALPHAS[mode])


ROW_NORM = 0.2
MARGIN = 4.0           # a bound is MARGIN x the oracle's own spread over three sentence orders
RARE_MAX = 0.05        # the rare-row bound must stay below this (one lost update of a 4-update row: 0.25)
PRIV_MAX_BOUND = 0.02  # the private-range bound must stay below this (2 % of a row's updates lost: 0.02)

NAMES = "WCS"


def _listing(types):
    return [[f"w{r}" for r in range(types)]]


_ORACLES = {}


def corpus_oracle(corpus, mode, dim, window=WINDOW, negative=None, table_size=TABLE, n_sent=None, shared=False):
    """The oracle on corpus "A" or "B" at its constant learning rate (alpha(mode, dim)) and a
    random start of row norm ROW_NORM in every matrix (so that the NS matrices
    do not start at zero). Cached and never trained in place: `run_oracle`
    puts the start back. n_sent: train on the first n_sent sentences only."""
    k = (corpus, mode, dim, window, negative, table_size, n_sent, shared)
    if k in _ORACLES:
        return _ORACLES[k]
    if corpus == "A":
        sents = zipf_sentences(N_SENT_A, 64, TYPES_A, seed=61, ragged=True)
        text, n = sents + _listing(TYPES_A), N_SENT_A
    else:
        sents = zipf_sentences(N_SENT_B, LEN_B, TYPES_B, seed=67)
        text, n = sents, N_SENT_B
    o = oracle_run(text, mode, dim=dim, window=window, iters=1, min_count=1, table_size=table_size,
                   init_alpha=alpha(mode, dim), min_alpha=alpha(mode, dim), train=False, negative=negative)
    o.build_sample()
    ids, off = o.samples()
    n = min(n, n_sent or n)
    o.set_samples(ids[:off[n]], off[:n + 1], int(off[n]))
    assert corpus != "A" or o.V == TYPES_A
    rng = np.random.default_rng(1000 + dim)
    for m in range(3):
        shape = o.matrix(m).shape
        if shape[0]:
            o.set_matrix(m, (rng.standard_normal(shape) * (ROW_NORM / np.sqrt(dim))).astype(np.float32))
    if shared:
        o.set_shared_negatives(True)
    _ORACLES[k] = o
    return o


def orders(n, epochs=2):
    """The sentence order of each epoch: the same for every case of a corpus."""
    return [np.random.default_rng(7 + e).permutation(n) for e in range(epochs)]


_VISITS = {}


def corpus_visits(o, corpus, mode, window=WINDOW, negative=None, table_size=TABLE, n_sent=None, shared=False,
                  epochs=2):
    """The visit reference of each epoch (orders(n)) of a corpus_oracle, cached
    per everything the visits depend on (the row width is not among it)."""
    m = mode_config(mode, negative)
    k = (corpus, m["model"], m["train_method"], m["negative"], window, table_size, n_sent, shared, epochs)
    if k not in _VISITS:
        ids, off = o.samples()
        hs, cbow = m["train_method"] == "hs", m["model"] == "cbow"
        bounds = o.table_bounds() if m["negative"] > 0 else None
        out = []
        for e, od in enumerate(orders(off.size - 1, epochs)):
            if shared:
                out.append(vr.shared_visits(ids, off, o.sample_probs(), window=window, negative=m["negative"], key=KEY,
                                            epoch=e, bounds=bounds, order=od))
            else:
                out.append(vr.visits(ids, off, o.sample_probs(), window=window, negative=m["negative"], hs=hs,
                                     cbow=cbow, key=KEY, epoch=e, bounds=bounds, huffman=o.huffman() if hs else None,
                                     order=od))
        _VISITS[k] = out
    return _VISITS[k]


def trained(mode, shared=False):
    """The matrices a mode trains (CBOW-HS holds a W it never reads or writes)."""
    m = mode_config(mode)
    hs, ns, cbow = m["train_method"] == "hs", m["negative"] > 0, m["model"] == "cbow"
    return [k for k, on in enumerate((not cbow or ns, cbow or ns, hs)) if on]


def ns_output(mode):
    """The matrix whose rows the table draws reach (None without negatives): with
    a 100 K-slot table over 5 K types every word owns a slot and a launch draws
    every slot several times, so this matrix has no untouched row."""
    m = mode_config(mode)
    return None if m["negative"] <= 0 else (0 if m["model"] == "cbow" else 1)


def matrices(o):
    return [o.matrix(k) if o.matrix(k).shape[0] else None for k in range(3)]


def run_oracle(o, order, epoch=0, key=KEY):
    """One sequential Philox epoch from the oracle's current matrices, which
    are put back afterwards. Returns (start, result) per matrix."""
    init = matrices(o)
    o.train_philox(epoch, 1, order, key, 0)
    want = matrices(o)
    for k in range(3):
        if init[k] is not None:
            o.set_matrix(k, init[k])
    return init, want


def other_orders(order):
    """The two further orders the oracle's spread is measured with."""
    return [order[::-1].copy(), np.random.default_rng(99).permutation(order)]


_REFS = {}


def reference(mode, dim, runs=3, shared=False, **kw):
    """Corpus A's oracle trained one epoch from the same start in orders(n)[0]
    and (runs 3) in its reverse and in one other permutation: init, the
    updates (float64, result - start) and the visit reference. The runs are
    made when first asked for and kept."""
    k = (mode, dim, shared, tuple(sorted(kw.items())))
    ref = _REFS.get(k)
    if ref is None:
        o = corpus_oracle("A", mode, dim, shared=shared, **kw)
        order = orders(o.samples()[1].size - 1)[0]
        vis = corpus_visits(o, "A", mode, shared=shared, **kw)[0]
        ref = _REFS[k] = dict(o=o, init=matrices(o), upd=[], order=order, visits=vis, V=o.V)
    all_orders = [ref["order"]] + other_orders(ref["order"])
    while len(ref["upd"]) < runs:
        init, want = run_oracle(ref["o"], all_orders[len(ref["upd"])])
        ref["upd"].append([None if w is None else w.astype(np.float64) - i for w, i in zip(want, init)])
    return ref


def private_ranges(mode, V, priv_lo=None, priv_n=PRIV_MAX, ctx_n=CTX_MAX, shared=False):
    """{matrix: rows} of the LDS-private ranges: the output range [priv_lo,
    priv_lo + priv_n) of the NS target matrix or of synapses1, CBOW's context
    rows [0, ctx_n) of C. Defaults: the largest ranges the policy can choose
    (the hottest kPrivMax output rows / Huffman nodes nearest the root,
    kCtxMax context rows), of which a launch's own ranges are a part."""
    m = mode_config(mode)
    hs, cbow = m["train_method"] == "hs", m["model"] == "cbow"
    if hs and m["negative"] > 0:
        raise ValueError("the combined modes have no conservation case")
    out = {}
    if hs:
        lo = V - 1 - priv_n if priv_lo is None else priv_lo
        out[2] = np.arange(lo, lo + priv_n)
    else:
        lo = 0 if priv_lo is None else priv_lo
        out[0 if cbow else 1] = np.arange(lo, lo + priv_n)
    if cbow and not shared:
        out[1] = np.arange(0, ctx_n)
    return {k: r for k, r in out.items() if r.size}


def row_rel(dg, dw, rows):
    """max over `rows` of |dg_r - dw_r| / |dw_r| (2-norms of the rows' updates)."""
    if len(rows) == 0:
        return 0.0
    den = np.linalg.norm(dw[rows], axis=1)
    assert (den > 0).all(), "a row of this class has no reference update"
    return float((np.linalg.norm(dg[rows] - dw[rows], axis=1) / den).max())


def measure(dgot, dwant, visits, priv):
    """{"<matrix>.<class>": error} of one update against another: norm-wise over
    the matrix (harness.rel_err), and per row over the rare rows (1 to 4
    updates by the visit reference) and the private ranges `priv`."""
    out = {}
    for k, (g, w) in enumerate(zip(dgot, dwant)):
        if w is None or not np.abs(w).max():
            continue
        u = visits["updates"][k]
        out[f"{NAMES[k]}.norm"] = rel_err(g, w)
        rare = np.nonzero((u >= 1) & (u <= 4))[0]
        if rare.size:
            out[f"{NAMES[k]}.rare"] = row_rel(g, w, rare)
        if k in priv:
            out[f"{NAMES[k]}.priv"] = row_rel(g, w, priv[k][u[priv[k]] > 0])
    return out


def spreads(ref, mode, shared=False, priv=None):
    """The oracle's own order-plus-rounding spread: per class the larger error
    of the reversed and the permuted order against orders(n)[0]."""
    priv = private_ranges(mode, ref["V"], shared=shared) if priv is None else priv
    a, b = (measure(u, ref["upd"][0], ref["visits"], priv) for u in ref["upd"][1:])
    return {k: max(a[k], b[k]) for k in a}


def log(tag, what, values, **more):
    """Append a measurement to W2V_PARITY_LOG (as harness.check_parity does)."""
    print(f"{tag} {what}: " + " ".join(f"{k} {v:.2e}" for k, v in values.items()))
    path = os.environ.get("W2V_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(tag=tag, what=what, **values, **more)) + "\n")


CONSERVED = ("sg_ns", "sg_hs", "cbow_ns", "cbow_hs")

# The oracle's spreads on corpus A at ALPHAS, as measured and committed in
# profiles/r11a_conservation.jsonl ("oracle spread"); tests/test_visit_ref.py
# and the GPU test recompute them. BOUNDS are MARGIN x these, and never above
# RARE_MAX / PRIV_MAX_BOUND for the two row classes.
SPREADS = {
    ("sg_ns", 64): {"W.norm": 1.663e-03, "W.rare": 6.026e-03, "C.norm": 6.890e-03, "C.priv": 5.972e-03},
    ("sg_ns", 300): {"W.norm": 1.662e-03, "W.rare": 6.390e-03, "C.norm": 6.796e-03, "C.priv": 4.669e-03},
    ("sg_hs", 64): {"W.norm": 4.961e-03, "W.rare": 2.460e-02, "S.norm": 4.325e-03, "S.rare": 7.594e-03, "S.priv": 7.613e-03},
    ("sg_hs", 300): {"W.norm": 3.760e-03, "W.rare": 2.890e-02, "S.norm": 2.810e-03, "S.rare": 8.494e-03, "S.priv": 6.639e-03},
    ("cbow_ns", 64): {"W.norm": 1.950e-03, "W.rare": 1.171e-02, "W.priv": 5.943e-03, "C.norm": 5.456e-04, "C.rare": 1.559e-02, "C.priv": 3.844e-03},
    ("cbow_ns", 300): {"W.norm": 1.402e-03, "W.rare": 1.149e-02, "W.priv": 7.069e-03, "C.norm": 7.220e-04, "C.rare": 1.231e-02, "C.priv": 3.095e-03},
    ("cbow_hs", 64): {"C.norm": 4.045e-04, "C.rare": 1.726e-02, "C.priv": 4.106e-03, "S.norm": 6.827e-04, "S.rare": 2.367e-02, "S.priv": 1.266e-02},
    ("cbow_hs", 300): {"C.norm": 8.235e-04, "C.rare": 1.701e-02, "C.priv": 7.340e-03, "S.norm": 1.263e-03, "S.rare": 3.133e-02, "S.priv": 1.808e-02},
}


def capped(spread):
    """{class: bound}: MARGIN x the spread, the row classes capped at the
    values that keep them able to fail."""
    cap = {"rare": RARE_MAX, "priv": PRIV_MAX_BOUND}
    return {k: min(MARGIN * v, cap.get(k.split(".")[1], np.inf)) for k, v in spread.items()}


BOUNDS = {k: capped(v) for k, v in SPREADS.items()}


def measured_spreads(mode, dim, **kw):
    """The spreads recomputed from three oracle runs (logged)."""
    sp = spreads(reference(mode, dim, **kw), mode)
    log(f"{mode} d{dim}", "oracle spread", sp, alpha=alpha(mode, dim))
    return sp
