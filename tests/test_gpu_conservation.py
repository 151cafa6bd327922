"""Full-concurrency training applies every update exactly once.

tests/test_gpu_parallel_parity.py checks the parallel schedule's update paths
against the oracle on a grid of ONE one-wave workgroup, where no lock is
contended, no flush races an add and no two workgroups meet on a row. Here the
launches are the ones that are benchmarked: a grid of 16-wave workgroups,
LDS-private rows under priv_lock, atomics on the hot rows, sentence segments,
wave caps, the deep HS kernel.

1. Exact accounting. In Philox mode every keep test, window shrink and table
   draw is a pure function of (key, epoch, sentence, position, slot, k), so
   the five counters of w2v_dev_stats and the number of updates every row
   receives are integers tests/visit_ref.py computes on the CPU, for any grid,
   segmentation or wave cap. Every case asserts from the launch plan that the
   intended path ran and that all counters equal the reference after one epoch
   and, on the same handle, after a second (epoch 1 enters the Philox counter).
   On a bound model at a wider pitch the rows the reference never updates must
   come back bit-identical, the padding columns zero, and the updated rows
   changed.
2. Conservation (tests/conservation.py). With every non-private row on atomics
   (hot rows -1), every flush scale 1 (private_average 0, hs_hot_avg 0) and a
   constant learning rate, every update lands exactly once in the oracle's
   g * x form, so the launch may differ from Oracle.train_philox only as the
   oracle differs from itself in another sentence order: at second order in
   alpha plus fp32 rounding. A lost, doubled or misdirected update is a
   first-order difference. tests/test_visit_ref.py shows on the CPU that the
   comparison catches each of them at these bounds.
"""
import numpy as np
import pytest

from tests import conservation as cv
from tests import visit_ref as vr
from tests.harness import bound_device_from_oracle, device_config, device_from_oracle, mode_config

pytestmark = pytest.mark.gpu

from word2vec_amd import _native as N  # noqa: E402

ALL_MODES = ["sg_ns", "sg_hs", "cbow_ns", "cbow_hs", "sg_hsns", "cbow_hsns"]
DEEP_WPB = 4  # kDeepBlock / 64: the deep HS kernel's workgroup


def _cbow(mode):
    return mode_config(mode)["model"] == "cbow"


def _handle(o, mode, dim, monkeypatch, window=cv.WINDOW, negative=None, table_size=cv.TABLE, env=None, bound=False,
            shared=False):
    """A parallel-schedule Philox handle on the oracle's corpus and current
    matrices; bound: on caller-owned tensors 64 floats wider than the row."""
    a = cv.alpha(mode, dim)
    cfg = device_config(o, mode, dim, window, 1, table_size, True, a, a, negative)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    tens = None
    if bound:
        d, tens, pitch = bound_device_from_oracle(o, cfg, extra=64)
        assert pitch == d.row_pitch() + 64
    else:
        d = device_from_oracle(o, cfg, initial=False)
    for k in (env or {}):
        monkeypatch.delenv(k)
    if shared:
        d.set_update(N.W2V_UPDATE_SHARED_NEGATIVES)
    d.set_rng(N.W2V_RNG_PHILOX, cv.KEY)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_private_rate(0)  # no rate limit, as in the one-wave tests: the automatic one would shrink the ranges
    d.set_progress(0)
    return d, tens


def _model(d, tens, dim):
    """([W, C, S] blocks of width dim, [padding columns] of a bound model)."""
    if tens is None:
        return list(d.download_model()), None
    full = [None if t is None else t.cpu().numpy() for t in tens]
    return ([None if m is None else np.ascontiguousarray(m[:, :dim]) for m in full],
            [None if m is None else m[:, dim:] for m in full])


def _show(tag, plan):
    print(f"{tag}: shared {plan['shared']} deep {plan['deep']} grid {plan['grid']} x {plan['wpb']} waves, nseg "
          f"{plan['nseg']} seg_len {plan['seg_len']}, priv {plan['priv_n']} from {plan['priv_lo']} ctx {plan['ctx_n']}, "
          f"flush {plan['flush_every']} / {plan['ctx_flush_every']} avg {plan['priv_avg']:g}, hot_wc {plan['hot_wc']} "
          f"hot_s {plan['hot_s']} hot_atomic {plan['hot_atomic']} hs_hot_avg {plan['hs_hot_avg']:g}, wave_cap "
          f"{plan['wave_cap']} lds {plan['lds_bytes']} wide_scratch {plan['wide_scratch']}")


def _full_grid(mode, wpb=16, nseg_one=True):
    """The plan of a case on the full grid: several workgroups of `wpb` waves
    with LDS-private output rows (and context rows for CBOW)."""
    def check(plan):
        assert plan["shared"] == 0 and plan["grid"] > 1 and plan["wpb"] == wpb and plan["threads"] == 64 * wpb, plan
        assert plan["priv_n"] > 0, plan
        assert plan["ctx_n"] > 0 or not _cbow(mode), plan
        assert (plan["nseg"] == 1) if nseg_one else (plan["nseg"] > 1), plan
    return check


# ---------------------------------------------------------------------------
# 1. Exact accounting
# ---------------------------------------------------------------------------
def _conditions(mode, vis, tag, all_matrices=False):
    """The reference alone must leave the row checks something to find: of
    every matrix the mode trains at least 5 % of the rows are never updated
    and at least 50 % are. The matrix the table draws reach is excepted from
    the first rule at the 100 K-slot table (conservation.ns_output): the
    short-table cases (all_matrices) hold it to both."""
    for k in cv.trained(mode):
        u = vis[0]["updates"][k]
        untouched, touched = float((u == 0).mean()), float((u > 0).mean())
        print(f"{tag}: {cv.NAMES[k]} {u.size} rows, untouched {untouched:.3f}, touched {touched:.3f}")
        assert touched >= 0.5, (tag, k, touched)
        if all_matrices or k != cv.ns_output(mode):
            assert untouched >= 0.05, (tag, k, untouched)
        else:
            assert untouched < 0.05, (tag, k, untouched)  # (the exception is needed)


def _check_rows(tag, got, pad, init, counts, moved=None):
    """Rows with no update are bit-identical to the upload, the padding is
    zero; `moved` (the oracle's update, result - start): a row the reference
    updates, by at least one ulp of its largest entry, differs from its start.
    (Below one ulp an exact implementation may round the update away.)"""
    for k, u in enumerate(counts):
        if got[k] is None:
            continue
        if u is None:                      # a matrix the mode never trains (CBOW-HS's W)
            u = np.zeros(got[k].shape[0], np.int64)
        same = (got[k].view(np.uint32) == init[k].view(np.uint32)).all(axis=1)
        wrong = np.nonzero((u == 0) & ~same)[0]
        assert wrong.size == 0, f"{tag}: {cv.NAMES[k]} rows without an update changed: {wrong[:10]} of {wrong.size}"
        assert not pad[k].any(), f"{tag}: {cv.NAMES[k]} wrote past column {got[k].shape[1]}"
        if moved is not None and moved[k] is not None:
            ulp = np.spacing(np.abs(init[k]).max(axis=1))
            must = (u > 0) & (np.abs(moved[k]).max(axis=1) >= ulp)
            assert must.sum() >= 0.99 * (u > 0).sum(), (tag, k, int(must.sum()), int((u > 0).sum()))
            still = np.nonzero(must & same)[0]
            assert still.size == 0, f"{tag}: {cv.NAMES[k]} rows with updates did not change: {still[:10]} of {still.size}"


def _account(tag, corpus, mode, dim, monkeypatch, check_plan, env=None, settings=None, bound=False, slices=None,
             shared=False, short_table=False, **kw):
    o = cv.corpus_oracle(corpus, mode, dim, shared=shared, **kw)
    vis = cv.corpus_visits(o, corpus, mode, shared=shared, **kw)
    ords = cv.orders(o.samples()[1].size - 1)
    init = cv.matrices(o)
    if bound:
        _conditions(mode, vis, tag, all_matrices=short_table)
    hkw = {k: v for k, v in kw.items() if k != "n_sent"}
    d, tens = _handle(o, mode, dim, monkeypatch, env=env, bound=bound, shared=shared, **hkw)
    if settings:
        settings(d)
    counts = [None if u is None else np.zeros_like(u) for u in vis[0]["updates"]]
    for e in (0, 1):
        if slices is None:
            st = d.train_epoch(e, ords[e])
        else:
            before = d.read_stats()
            d.set_order(ords[e])
            first = 0
            for n in slices:
                d.train_slice_async(e, first, n)
                first += n
            assert first == ords[e].size
            d.synchronize()
            st = {k: v - before[k] for k, v in d.read_stats().items()}
        if e == 0:
            plan = d.launch_plan()
            _show(tag, plan)
            check_plan(plan)
        want = {k: vis[e][k] for k in vr.COUNTERS}
        print(f"{tag} epoch {e}: device {st}, reference {want}")
        assert {k: st[k] for k in vr.COUNTERS} == want, (tag, e)
        assert st["nonfinite"] == 0
        total = d.read_stats()  # cumulative on the handle
        assert {k: total[k] for k in vr.COUNTERS} == {k: sum(v[k] for v in vis[:e + 1]) for k in vr.COUNTERS}, (tag, e)
        if bound:
            counts = [None if c is None else c + u for c, u in zip(counts, vis[e]["updates"])]
            got, pad = _model(d, tens, dim)
            moved = cv.reference(mode, dim, runs=1, shared=shared, **kw)["upd"][0] if e == 0 else None
            _check_rows(f"{tag} epoch {e}", got, pad, init, counts, moved)
    d.close()


@pytest.mark.parametrize("dim", [64, 300])
@pytest.mark.parametrize("mode", ALL_MODES)
def test_counts_and_untouched_rows(mode, dim, monkeypatch):
    """The four modes and the two combined ones on corpus A, default policy, on
    a bound model 64 floats wider than the row."""
    _account(f"A {mode} d{dim} bound", "A", mode, dim, monkeypatch, _full_grid(mode), bound=True)


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns", "sg_hsns", "cbow_hsns"])
def test_counts_and_untouched_rows_short_table(mode, monkeypatch):
    """A 2 000-slot table over the 5 000 types: the rarer words own no slot, so
    the matrix the draws reach has rows no update may touch as well."""
    _account(f"A {mode} d64 bound, table 2000", "A", mode, 64, monkeypatch, _full_grid(mode), bound=True,
             short_table=True, table_size=2000)


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs", "sg_hs"])
def test_counts_segments(mode, monkeypatch):
    """Corpus B: 700-token sentences cut into segments as work items."""
    _account(f"B {mode} d100", "B", mode, 100, monkeypatch, _full_grid(mode, nseg_one=False))


@pytest.mark.parametrize("mode", ["sg_hs", "cbow_hs"])
def test_counts_deep_hs(mode, monkeypatch):
    def check(plan):
        assert plan["deep"] == 1
        _full_grid(mode, wpb=DEEP_WPB)(plan)

    _account(f"A {mode} d100 deep", "A", mode, 100, monkeypatch, check, env={"W2V_DEEP_HS": 1})


def test_counts_large_vocab_hs_policy(monkeypatch):
    """W2V_WIDE_HS=1: the large-vocabulary HS policy (its wave cap, the deep
    kernel, skip-gram's write-combining node cache summed after every center of
    a wave), as test_one_wave_large_vocab_hs_policy asserts it on one wave."""
    def check(plan):
        assert plan["shared"] == 0 and plan["deep"] == 1 and plan["grid"] > 1, plan
        assert plan["wave_cap"] > 0 and plan["grid"] * plan["wpb"] <= plan["wave_cap"], plan
        assert plan["priv_n"] > 0 and plan["priv_avg"] == 0 and plan["flush_every"] == plan["wpb"], plan
        assert plan["nseg"] == 1, plan

    _account("A sg_hs d100 large-vocabulary policy", "A", "sg_hs", 100, monkeypatch, check, env={"W2V_WIDE_HS": 1})


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_counts_wave_cap_48(mode, monkeypatch):
    """A cap that is no multiple of 16 (nor of the CU count)."""
    def check(plan):
        assert plan["shared"] == 0 and plan["grid"] > 1 and plan["grid"] * plan["wpb"] <= 48, plan
        assert plan["nseg"] == 1, plan

    _account(f"A {mode} d64 max_waves 48", "A", mode, 64, monkeypatch, check, settings=lambda d: d.set_max_waves(48))


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns"])
def test_counts_window_150_negative_80(mode, monkeypatch):
    """ns_word_many (negative >= 64) and cbow_center_huge (window > 127, each
    wave its own scratch slice) on the first 200 sentences of corpus A."""
    def check(plan):
        if _cbow(mode):
            _full_grid(mode)(plan)
            assert plan["wide_scratch"] > 0, plan
        else:  # 81 targets per context: the automatic wave cap leaves one-wave workgroups
            assert plan["shared"] == 0 and plan["grid"] > 1 and plan["nseg"] == 1 and plan["priv_n"] > 0, plan
            assert 0 < plan["wave_cap"] < 200 and plan["grid"] * plan["wpb"] <= plan["wave_cap"], plan

    _account(f"A[:200] {mode} d64 window 150 negative 80", "A", mode, 64, monkeypatch, check, window=150, negative=80,
             n_sent=200)


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_counts_epoch_in_five_slices(mode, monkeypatch):
    _account(f"A {mode} d64 5 slices", "A", mode, 64, monkeypatch, _full_grid(mode), slices=[100, 700, 37, 1000, 211])


@pytest.mark.parametrize("dim,window,negative", [(128, 5, 5), (128, 8, 15), (300, 5, 15), (300, 8, 5)])
def test_counts_shared_negatives(dim, window, negative, monkeypatch):
    def check(plan):
        assert plan["shared"] == 1 and plan["grid"] > 1 and plan["wpb"] == 2, plan

    _account(f"A shared d{dim} window {window} negative {negative}", "A", "sg_ns", dim, monkeypatch, check,
             shared=True, window=window, negative=negative)


# ---------------------------------------------------------------------------
# 2. Conservation under the lossless policy
# ---------------------------------------------------------------------------
_LAUNCHES = {}


def _conserve(mode, dim, flush, deep, monkeypatch):
    """One lossless launch per case, shared by the two tests below: its plan is
    asserted, its counters are exact, and its errors against the oracle's run
    in the same order are measured per class and logged."""
    case = (mode, dim, flush, deep)
    if case in _LAUNCHES:
        return _LAUNCHES[case]
    tag = f"conservation {mode} d{dim} flush {flush}" + (" deep" if deep else "")
    ref = cv.reference(mode, dim)
    o, V = ref["o"], ref["V"]
    d, _ = _handle(o, mode, dim, monkeypatch, env={"W2V_DEEP_HS": 1} if deep else None)
    d.set_hot_rows(-1)
    d.set_private_sync(flush, 0.0)
    if _cbow(mode):
        d.set_context_private(-1, flush)
    st = d.train_epoch(0, ref["order"])
    plan = d.launch_plan()
    got = d.download_model()
    d.close()
    _show(tag, plan)
    # the plan is lossless: every update lands once, unscaled
    _full_grid(mode, wpb=DEEP_WPB if deep else 16)(plan)
    assert plan["deep"] == deep, plan
    assert plan["priv_avg"] == 0 and plan["hs_hot_avg"] == 0 and plan["hot_sc"].size == 0, plan
    assert (plan["priv_sc"] == 1.0).all() and (plan["ctx_sc"] == 1.0).all(), plan
    assert plan["hot_wc"] == V and plan["hot_s"] == 0, plan  # every W / C row and Huffman node takes atomics
    assert plan["flush_every"] == flush and (plan["ctx_flush_every"] == flush or not _cbow(mode)), plan
    assert {k: st[k] for k in vr.COUNTERS} == {k: ref["visits"][k] for k in vr.COUNTERS}
    assert st["nonfinite"] == 0
    # the launch's private ranges are part of the ranges the bounds were measured over
    widest = cv.private_ranges(mode, V)
    priv = cv.private_ranges(mode, V, plan["priv_lo"], plan["priv_n"], plan["ctx_n"])
    assert all(set(r) <= set(widest[k]) for k, r in priv.items()), (priv, widest)
    dgot = [None if g is None or i is None else g.astype(np.float64) - i for g, i in zip(got, ref["init"])]
    err = cv.measure(dgot, ref["upd"][0], ref["visits"], priv)
    bounds = cv.BOUNDS[(mode, dim)]
    assert set(err) == set(bounds), (sorted(err), sorted(bounds))
    # the committed spreads are the ones the oracle gives here
    sp = cv.measured_spreads(mode, dim)
    for k, v in cv.SPREADS[(mode, dim)].items():
        assert abs(sp[k] / v - 1) < 0.25, (tag, k, sp[k], v)
    cv.log(tag, "gpu", err, bounds=bounds)
    _LAUNCHES[case] = (tag, err, bounds)
    return _LAUNCHES[case]


def _assert_classes(tag, err, bounds, classes):
    over = {k: (err[k], bounds[k]) for k in err if k.split(".")[1] in classes and not err[k] < bounds[k]}
    assert any(k.split(".")[1] in classes for k in err), (tag, sorted(err))
    assert not over, (tag, over)


# flush 8: flushes interleave with the other waves' adds all through the
# launch; 1 000 000: the only flush is the one at the end of the kernel.
CONSERVATION_CASES = [(m, d, f, 0) for m in cv.CONSERVED for d in (64, 300) for f in (8, 1_000_000)] + \
                     [(m, 64, 8, 1) for m in ("sg_hs", "cbow_hs")]


@pytest.mark.parametrize("mode,dim,flush,deep", CONSERVATION_CASES)
def test_conservation_rare_rows(mode, dim, flush, deep, monkeypatch):
    """Rows with 1 to 4 updates: one lost update of a 4-update row is 0.25.
    Measured (profiles/r11a_conservation.jsonl): the GPU is as far from the
    oracle as the oracle's other orders are (0.67 to 1.03 of the spread), at most
    0.50 of bounds of 0.024 to 0.05."""
    tag, err, bounds = _conserve(mode, dim, flush, deep, monkeypatch)
    _assert_classes(tag, err, bounds, ("rare",))


@pytest.mark.parametrize("mode,dim,flush,deep", CONSERVATION_CASES)
def test_conservation_hot_rows(mode, dim, flush, deep, monkeypatch):
    """Norm-wise per matrix (the hottest rows decide it) and the private ranges.

    What these classes need from the learning rate (tests/conservation.py,
    ALPHAS): a hot row takes 40 K to 250 K adds, and in fp32 the oracle rounds
    each at 2^-24 of the ROW; the same few thousand (center, sign) increments
    repeat, so that rounding does not average out and is the same in every
    sentence order, where the three-order spread cannot show it. The launch
    sums a private row's updates in an LDS delta 100 times smaller than the
    row. At 2^-17 skip-gram HS at d 64 is 0.032 (norm-wise) and 0.053 (private
    range) from the oracle against bounds of 0.021 and 0.020, while against a
    float64 sum of the same terms at the start model the root node's update is
    0.40 % off on the GPU and 2.24 % in the oracle (nodes V-3, V-4, V-10: 0.34 /
    2.89, 0.21 / 5.28, 0.31 / 2.35 %), and two launches agree to 0.05 %. At the
    rates the cases run at, the second-order spread covers that rounding.
    Measured there over three runs (profiles/r11a_conservation.jsonl holds one),
    error / bound at worst: skip-gram NS 0.40, skip-gram HS 0.50 (deep the
    same), CBOW-NS 0.29 with flushes every 8 centers and 0.78 with the only
    flush at the end (norm-wise, C at d 64), CBOW-HS 0.63 and 0.80 (norm-wise,
    d 300). One power of two to either side CBOW-NS and CBOW-HS miss a norm-wise
    bound ("sweep" lines of that file)."""
    tag, err, bounds = _conserve(mode, dim, flush, deep, monkeypatch)
    _assert_classes(tag, err, bounds, ("norm", "priv"))
