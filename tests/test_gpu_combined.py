"""GPU parity of the configurations the four MODES never run.

1. Hierarchical softmax together with negative sampling (train_method "hs"
   with negative > 0): both updates per target, HS first (Word2Vec.cpp:304-311,
   :342-349). The kernels are the <HS, NS> instantiations of train_epoch_kernel;
   the private rows are the Huffman nodes (priv_M = synapses1) while the NS
   target matrix stays on plain or atomic rows, and there is no deep variant.
2. CBOW as a sum (cbow_mean off): cbow_tail's two divisions by n.
3. The alpha floor (alpha = max(min_alpha, ...)) in train_epoch and in the
   shared-negatives kernel, and a word counter past iter * train_words.

Every case checks W, C and synapses1 against the oracle's own matrices with
check_parity, asserts that the matrices the configuration trains all moved,
and compares the word counter. The inputs are tests/combined_cases.py's;
tests/test_train_ref.py shows on the CPU that each of them tells the feature
from its absence by >= 100 x the bound used here, and pins the oracle itself
to a float64 reference in these configurations.

Bounds: the class of the existing sibling (SINGLE for one sentence, MULTI,
LIFTED for rows past 512 floats, negative >= 64 and window 200); no case has
a bound of its own and none uses check_parity's 2-ulp clause. Measured
(profiles/r09a_parity_errors.jsonl; sequential or one wave, so a build
reproduces them exactly): single updates <= 3.4e-6 norm-wise (CBOW-HS as a
sum, C) and 1.5e-3 per element (CBOW-NS as a sum, W at d 300); all other cases
<= 4.8e-6 (SG hs+ns synapses1, one wave, d 100) and 6.6e-4.
"""
import numpy as np
import pytest

from tests import combined_cases as cc
from tests.corpus import zipf_sentences
from tests.harness import check_parity, device_config, device_from_oracle, mode_config, oracle_run
from tests.test_gpu_parallel_parity import (CTX_MAX, KEY as WAVE_KEY, PRIV_MAX, TABLE, WINDOW, _assert_identical,
                                            _lds_for, _run_case)

pytestmark = pytest.mark.gpu

from word2vec_amd import _native as N  # noqa: E402

ids = lambda c: c.id  # noqa: E731


def _moved(want, init, tag, mode=None):
    """Every matrix the configuration trains moved (CBOW-HS leaves W as it is:
    check_parity then wants it back bit for bit)."""
    for k, (w, i) in enumerate(zip(want, init)):
        if w is not None and not (k == 0 and mode == "cbow_hs"):
            assert np.abs(w.astype(np.float64) - i).max() > 0, f"{tag}: matrix {k} did not move"


def _matrices(o, got, initial):
    return [o.matrix(k, initial) if got[k] is not None else None for k in range(3)]


def _replay(case, cbow_mean=True, min_alpha=2.5e-6):
    """The reference's own mt19937 draws on the sequential schedule."""
    c = cc.CORPORA[case.corpus]
    o = oracle_run(cc.sentences(case.corpus), case.mode, dim=case.dim, window=c["window"], iters=case.iters,
                   seed=c["seed"], min_count=c["min_count"], table_size=c["table_size"], cbow_mean=cbow_mean,
                   min_alpha=min_alpha, negative=case.negative)
    cfg = device_config(o, case.mode, case.dim, c["window"], case.iters, c["table_size"], cbow_mean, 0.05, min_alpha,
                        negative=case.negative)
    d = device_from_oracle(o, cfg, initial=True)
    stream, offs, orders = o.stream(case.iters)
    d.upload_replay(stream, offs)
    d.set_rng(N.W2V_RNG_REPLAY, 0)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    n = orders.size // case.iters
    for e in range(case.iters):
        st = d.train_epoch(e, orders[e * n:(e + 1) * n])
    assert st["nonfinite"] == 0
    assert d.get_progress() == o.current_words
    got = list(d.download_model())
    d.close()
    return o, got, _matrices(o, got, False), _matrices(o, got, True)


def _philox(case, cbow_mean=True, min_alpha=2.5e-6):
    """Philox draws on the sequential schedule, from the case's word counter."""
    c = cc.CORPORA[case.corpus]
    o = cc.case_oracle(case, cbow_mean=cbow_mean, min_alpha=min_alpha)
    cfg = device_config(o, case.mode, case.dim, c["window"], case.iters, c["table_size"], cbow_mean, 0.05, min_alpha,
                        negative=case.negative)
    d = device_from_oracle(o, cfg, initial=False)
    init = [o.matrix(k) if o.matrix(k).size else None for k in range(3)]
    order = cc.philox_orders(o, case.iters)
    cw0 = case.cw0_epochs * case.iters * o.train_words
    o.train_philox(0, case.iters, order, cc.KEY, cw0)
    d.set_rng(N.W2V_RNG_PHILOX, cc.KEY)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(cw0)
    n = order.size // case.iters
    words = 0
    for e in range(case.iters):
        st = d.train_epoch(e, order[e * n:(e + 1) * n])
        words += st["words"]
        assert st["nonfinite"] == 0
    assert cw0 + words == o.current_words == d.get_progress()
    assert d.policy()["deep"] == 0 or mode_config(case.mode)["negative"] == 0
    got = list(d.download_model())
    d.close()
    return o, got, _matrices(o, got, False), init


def _check(case, run, tag, **kw):
    o, got, want, init = run
    _moved(want, init, tag, case.mode)
    check_parity(got, want, init, *case.tol, tag=f"{tag} {case.id}", **kw)
    return o


# ---------------------------------------------------------------------------
# 1. hs together with negative sampling
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.HSNS_SINGLE, ids=ids)
def test_combined_replay_single_update(case):
    """One sentence, the reference's draws, every row width of the configs: the
    48-token sentence of test_replay_single_sentence, and a 200-token one over
    40 types on which every matrix tells the combined update from either
    objective alone (tests/combined_cases.py)."""
    o = _check(case, _replay(case), "combined single")
    assert all(o.matrix(k).size for k in range(3))


@pytest.mark.parametrize("case", cc.HSNS_EPOCH, ids=ids)
def test_combined_replay_two_epochs(case):
    _check(case, _replay(case), "combined epochs")


@pytest.mark.parametrize("case", cc.HSNS_WIDTHS, ids=ids)
def test_combined_philox_sequential_row_widths(case):
    """Every instantiated row width (NV 1 .. 16), and for CBOW the 24 and 32
    floats-per-lane kernels (kMaxT = 4 batches)."""
    _check(case, _philox(case), "combined philox widths")


@pytest.mark.parametrize("rng", ["replay", "philox"])
@pytest.mark.parametrize("case", cc.HSNS_MANY, ids=ids)
def test_combined_many_negatives(case, rng):
    """negative 100: ns_word_many (64 draws at a time) behind hs_word."""
    _check(case, _replay(case) if rng == "replay" else _philox(case), f"combined {rng}")


@pytest.mark.parametrize("case", cc.HSNS_WINDOW, ids=ids)
def test_combined_replay_wide_windows(case):
    """Window 40 (2 * window + 1 > 64): CBOW's wide-window kernel, skip-gram's
    contexts past the first 64 positions read one by one; window 200: CBOW
    walks the span from the sentence (cbow_center_huge)."""
    _check(case, _replay(case), "combined window")


def _auto_rows(mode, dim, want=None, ctx=CTX_MAX):
    """The private ranges of a one-wave launch and the LDS budget that holds
    them (plan_private_rows): skip-gram with hs takes kPrivMax Huffman nodes,
    CBOW 64 and up to kCtxMax context rows beside them, as far as they fit."""
    cbow = mode.startswith("cbow")
    if want is None:
        want = 64 if cbow else PRIV_MAX
    lds, fit = _lds_for(want + (ctx if cbow else 0), dim)
    p = min(fit, want)
    return lds, p, min(fit - p, ctx) if cbow else 0


def _env(lds):
    return {"W2V_DEBUG_LDS_PER_WAVE": lds} if lds > 64 else None


@pytest.mark.parametrize("deep_knob", [None, 1])
@pytest.mark.parametrize("case", cc.HSNS_ONE_WAVE, ids=ids)
def test_combined_one_wave_default_policy(case, deep_knob, monkeypatch):
    """One wave of the parallel schedule: the private rows are Huffman nodes
    (priv_lo = V - 1 - priv_n, asserted by _check_path) and the launch is the
    per-pair kernel (shared 0, grid 1). The combined kernels have no deep
    variant: W2V_DEEP_HS=1 must fall back and train the same result."""
    lds, p, q = _auto_rows(case.mode, case.dim)
    assert p >= 64 and (q >= 63 or not case.mode.startswith("cbow"))
    env = dict(_env(lds))
    if deep_knob is not None:
        env["W2V_DEEP_HS"] = deep_knob
    plan = _run_case(case.mode, case.dim, monkeypatch, f"combined default knob{deep_knob}", p, q, 0, env=env,
                     tol=case.tol)
    assert plan["deep"] == 0 and plan["shared"] == 0 and plan["priv_lo"] == 320 - 1 - p


@pytest.mark.parametrize("rows", [0, 65])
@pytest.mark.parametrize("mode", cc.HSNS)
def test_combined_one_wave_private_rows(mode, rows, monkeypatch):
    lds, p, q = _auto_rows(mode, 300, want=rows)
    assert p == rows
    _run_case(mode, 300, monkeypatch, f"combined rows{rows}", p, q, 0, env=_env(lds),
              settings=lambda d: d.set_private_rows(rows), tol=cc.MULTI)


@pytest.mark.parametrize("hot", [-1, 0])
@pytest.mark.parametrize("mode", cc.HSNS)
def test_combined_one_wave_hot_rows(mode, hot, monkeypatch):
    """No private rows: every update a memory-side atomic add (-1: all rows of
    the NS target matrix and all Huffman nodes) or a plain read-modify-write."""
    def settings(d):
        d.set_private_rows(0)
        d.set_context_private(0, 0)
        d.set_hot_rows(hot)

    plan = _run_case(mode, 300, monkeypatch, f"combined hot{hot}", 0, 0, 0, settings=settings, tol=cc.MULTI)
    V = 320
    assert plan["lds_bytes"] == 0
    assert plan["hot_wc"] == (V if hot < 0 else 0)
    assert plan["hot_s"] == (0 if hot < 0 else V - 1)


@pytest.mark.parametrize("flush,ctx_flush", [(1, 1), (7, 3)])
@pytest.mark.parametrize("mode", cc.HSNS)
def test_combined_one_wave_flush_intervals(mode, flush, ctx_flush, monkeypatch):
    lds, p, q = _auto_rows(mode, 300)

    def settings(avg):
        def f(d):
            d.set_private_sync(flush, avg)
            d.set_context_private(-1, ctx_flush)
        return f

    plan = _run_case(mode, 300, monkeypatch, f"combined flush{flush}/{ctx_flush}", p, q, 0, env=_env(lds),
                     settings=settings(8.0), tol=cc.MULTI, also=[("plain sum (private_average 0)", settings(0.0))])
    assert (plan["flush_every"], plan["ctx_flush_every"]) == (flush, ctx_flush), plan


@pytest.mark.parametrize("rows,ctx", [(0, 64), (64, 64)])
def test_combined_one_wave_context_rows(rows, ctx, monkeypatch):
    """CBOW's private context rows beside the private nodes. At d 300 the
    production budget holds 127 rows, so (64, 64) runs 64 nodes + 63 rows."""
    lds, p, q = _auto_rows("cbow_hsns", 300, want=rows, ctx=ctx)
    assert p == rows and q == (64 if rows == 0 else 63)

    def settings(d):
        d.set_private_rows(rows)
        d.set_context_private(ctx, 0)

    _run_case("cbow_hsns", 300, monkeypatch, f"combined rows{rows}+ctx{ctx}", p, q, 0, env=_env(lds),
              settings=settings, tol=cc.MULTI)


# ---------------------------------------------------------------------------
# 2. CBOW as a sum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.SUM_SINGLE, ids=ids)
def test_sum_replay_single_update(case):
    _check(case, _replay(case, cbow_mean=False), "sum single")


@pytest.mark.parametrize("case", cc.SUM_WIDTHS, ids=ids)
def test_sum_philox_sequential(case):
    _check(case, _philox(case, cbow_mean=False), "sum philox")


@pytest.mark.parametrize("case", cc.SUM_WINDOW, ids=ids)
def test_sum_replay_wide_windows(case):
    """cbow_center's wide (window 40) and huge (window 200) siblings share cbow_tail."""
    _check(case, _replay(case, cbow_mean=False), "sum window")


_SUM_REFS = {}


def _sum_reference(case):
    ref = _SUM_REFS.get(case)
    if ref is None:
        o = cc.case_oracle(case, cbow_mean=False)
        init = [o.matrix(k) if o.matrix(k).size else None for k in range(3)]
        order = np.random.default_rng(7).permutation(o.samples()[1].size - 1)
        assert o.V == 320 and np.diff(o.samples()[1]).max() <= 128  # one work item per sentence
        o.train_philox(0, 1, order, WAVE_KEY, 0)
        want = [o.matrix(k) if init[k] is not None else None for k in range(3)]
        words = o.current_words
        for k in range(3):
            if init[k] is not None:
                o.set_matrix(k, init[k])  # device_from_oracle(initial=False) uploads the start again
        ref = _SUM_REFS[case] = dict(o=o, init=init, want=want, order=order, words=words)
    return ref


def _sum_launch(case, ref, env, monkeypatch):
    cfg = device_config(ref["o"], case.mode, case.dim, WINDOW, 1, TABLE, False, 0.05, 2.5e-6)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    d = device_from_oracle(ref["o"], cfg, initial=False)
    for k in env:
        monkeypatch.delenv(k)
    d.set_rng(N.W2V_RNG_PHILOX, WAVE_KEY)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_max_waves(1)
    d.set_private_rate(0)
    d.set_progress(0)
    st = d.train_epoch(0, ref["order"])
    plan = d.launch_plan()
    got = list(d.download_model())
    d.close()
    return got, plan, st


# CBOW-HS also on the regular kernel (W2V_DEEP_HS=0); the deep kernel serves hs without negatives only
SUM_ONE_WAVE = [(c, None) for c in cc.SUM_ONE_WAVE] + [(c, 0) for c in cc.SUM_ONE_WAVE if c.mode == "cbow_hs"]


@pytest.mark.parametrize("case,deep_knob", SUM_ONE_WAVE, ids=lambda v: v.id if isinstance(v, cc.Case) else f"knob{v}")
def test_sum_one_wave_private_context_rows(case, deep_knob, monkeypatch):
    """One wave of the parallel schedule with the default policy: the context
    rows summed into h come from LDS (global row + pending delta) and the
    undivided g goes back to them. CBOW-HS runs the deep kernel the wave cap
    chooses, and (W2V_DEEP_HS=0) the regular one."""
    hs_only = case.mode == "cbow_hs"
    lds, p, q = _auto_rows(case.mode, case.dim)
    env = dict(_env(lds))
    if deep_knob is not None:
        env["W2V_DEEP_HS"] = deep_knob
    ref = _sum_reference(case)
    tag = f"sum one wave knob{deep_knob} {case.id}"
    got, plan, st = _sum_launch(case, ref, env, monkeypatch)
    assert plan["shared"] == 0 and plan["grid"] == 1 and plan["wpb"] == 1 and plan["threads"] == 64, plan
    assert (plan["priv_n"], plan["ctx_n"]) == (p, q) and q >= 63, plan
    assert plan["deep"] == (1 if hs_only and deep_knob is None else 0)
    assert st["words"] == ref["words"] and st["nonfinite"] == 0
    want = [ref["want"][k] if got[k] is not None else None for k in range(3)]
    _moved(want, ref["init"], tag, case.mode)
    check_parity(got, want, ref["init"], *case.tol, tag=tag)
    again, _, st2 = _sum_launch(case, ref, env, monkeypatch)
    assert st2 == st
    _assert_identical(got, again, f"{tag}: repeat on a fresh handle")


# ---------------------------------------------------------------------------
# 3. The alpha floor
# ---------------------------------------------------------------------------
def _last_alpha(o):
    return o.L.orc_last_alpha(o.h)


@pytest.mark.parametrize("case", cc.FLOOR_EPOCH, ids=ids)
def test_floor_replay_epochs(case):
    """init_alpha 0.05, min_alpha 0.02: the schedule init_alpha * (1 - words /
    (iter * train_words)) is under the floor from 60 % of the schedule on.
    Alpha is refreshed at every tenth sentence of an epoch's order
    (Word2Vec.cpp:379), so the floor is the value used from the first refresh
    past that point. Both are computed from the oracle's word counts.
    Two epochs: under the floor at 8 of the 24 sentence starts (6 for SG-NS,
    whose shuffle puts longer sentences last), used by the last 2 sentences.
    Three epochs: under the floor at a third of the sentence starts, and the
    whole third epoch, a third of the sentences, trains at min_alpha exactly."""
    run = _replay(case, min_alpha=cc.FLOOR_ALPHA)
    o = run[0]
    _, off = o.samples()
    _, _, orders = o.stream(case.iters)
    starts = np.concatenate([[0], np.cumsum(np.diff(off)[orders])[:-1]])
    sched = (0.05 * (1.0 - starts / (case.iters * o.train_words))).astype(np.float32)
    floor = np.float32(cc.FLOOR_ALPHA)
    below = sched < floor
    n = orders.size // case.iters
    used = np.empty(orders.size, np.float32)
    for i in range(orders.size):
        if i % n % 10 == 0:
            alpha = max(floor, sched[i])
        used[i] = alpha
    at_floor = used == floor
    print(f"floor {case.id}: schedule under the floor at {below.sum()} of {orders.size} sentence "
          f"starts, {at_floor.sum()} sentences train at the floor")
    assert at_floor[-1] and not at_floor[0]
    if case.iters == 3:
        assert 3 * below.sum() >= orders.size and 3 * at_floor.sum() >= orders.size
    else:
        assert below.sum() >= 6 and at_floor.sum() == 2
    assert _last_alpha(o) == floor
    _check(case, run, f"floor {case.iters} epochs")


@pytest.mark.parametrize("case", cc.FLOOR_PAST_END, ids=ids)
def test_floor_from_the_first_sentence(case):
    """The word counter starts at twice iter * train_words (a resumed run, or
    more epochs than cfg.iter): the unfloored alpha is negative, so every update
    uses min_alpha exactly."""
    run = _philox(case, min_alpha=cc.FLOOR_ALPHA)
    o = run[0]
    assert 0.05 * (1.0 - case.cw0_epochs) < 0 and _last_alpha(o) == np.float32(cc.FLOOR_ALPHA)
    assert o.current_words > case.cw0_epochs * case.iters * o.train_words
    _check(case, run, "floor past the end")


@pytest.mark.parametrize("case", cc.FLOOR_SHARED, ids=ids)
def test_floor_shared_negatives(case):
    """The shared-negatives kernel has its own copy of the line (w2v_shared.hpp)."""
    from tests.test_gpu_shared import _compare, _setup

    o, d = _setup(cc.sentences(case.corpus), case.dim, negative=case.negative, iters=case.iters,
                  min_alpha=cc.FLOOR_ALPHA)
    n = o.samples()[1].size - 1
    order = np.concatenate([np.random.default_rng(1 + e).permutation(n) for e in range(case.iters)])
    _compare(o, d, order, *case.tol, f"floor shared {case.id}", epochs=case.iters)
    assert _last_alpha(o) == np.float32(cc.FLOOR_ALPHA)
    d.close()


# ---------------------------------------------------------------------------
# 4. The Word2Vec class with train_method "hs" and negative 5
# ---------------------------------------------------------------------------
def _model(model, sents, iters):
    from word2vec_amd.model import Word2Vec

    w = Word2Vec(iter=iters, window=5, min_count=2, table_size=50_000, word_dim=32, negative=5,
                 subsample_threshold=1e-3, init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True, train_method="hs",
                 model=model, replay_rng=True)
    w.seed(5)
    w.build_vocab(sents)
    w.init_weights()
    return w


@pytest.mark.parametrize("model", ["sg", "cbow"])
def test_class_combined_train_replay_matches_oracle(model):
    sents = zipf_sentences(10, 150, 300, seed=12, ragged=True)
    w = _model(model, sents, 2)
    w.train(sents)
    o = oracle_run(sents, f"{model}_hsns", dim=32, iters=2, table_size=50_000, seed=5)
    got, want, init = ([m(k) for k in range(3)] for m in (w.matrix, o.matrix, lambda k: o.matrix(k, True)))
    for k in range(3):
        assert got[k].shape == want[k].shape and want[k].size
    _moved(want, init, f"class train {model}_hsns")
    assert w.current_words == o.current_words
    check_parity(got, want, init, *cc.MULTI, tag=f"class train {model}_hsns")


@pytest.mark.parametrize("model", ["sg", "cbow"])
def test_class_combined_train_sentence_matches_oracle(model):
    """The row-sparse upload / download path: a sentence touches rows of W, C
    and synapses1."""
    sents = zipf_sentences(6, 120, 200, seed=13)
    w = _model(model, sents, 1)
    o = oracle_run(sents, f"{model}_hsns", dim=32, iters=1, table_size=50_000, seed=5, train=False)
    o.build_sample()
    tok, off = o.samples()
    init = [o.matrix(k) for k in range(3)]
    for s in range(3):
        sent = tok[off[s]:off[s + 1]]
        w.train_sentence(sent, 0.03, model == "cbow")
        o.train_sentence(sent, 0.03, model == "cbow")
    want = [o.matrix(k) for k in range(3)]
    _moved(want, init, f"class train_sentence {model}_hsns")
    check_parity([w.matrix(k) for k in range(3)], want, init, *cc.SINGLE, tag=f"class train_sentence {model}_hsns")


@pytest.mark.parametrize("model", ["sg", "cbow"])
def test_class_heldout_with_hs_and_negative_is_refused_before_training(model, tmp_path):
    """A held-out set has no single objective under hs together with negative >
    0 (w2v_dev_score refuses it): train() must refuse before any epoch trains,
    not after the first one, and so must score_ids / score_file."""
    sents = zipf_sentences(10, 150, 300, seed=12, ragged=True)
    w = _model(model, sents, 2)
    before = [w.matrix(k).copy() for k in range(3)]
    held = np.arange(8, dtype=np.int32)
    w.set_heldout(held, np.array([0, 8], np.int64))
    with pytest.raises(RuntimeError, match="heldout: hs together with negative > 0 has no single objective"):
        w.train(sents)
    assert w.epochs_done == 0 and w.current_words == 0 and w.epoch_heldout == []
    for k in range(3):
        np.testing.assert_array_equal(w.matrix(k), before[k])
    with pytest.raises(RuntimeError, match="score_ids: hs together with negative > 0 has no single objective"):
        w.score_ids(held, np.array([0, 8], np.int64))
    path = tmp_path / "c.txt"
    path.write_text("\n".join(" ".join(s) for s in sents[:2]) + "\n")
    with pytest.raises(RuntimeError, match="hs together with negative > 0 has no single objective"):
        w.score_file(path, "lines", 1)
    # without the held-out set the same object trains
    w.set_heldout(None)
    w.train(sents)
    assert w.epochs_done == 2 and w.current_words > 0
    assert all(np.abs(w.matrix(k) - before[k]).max() > 0 for k in range(3))
