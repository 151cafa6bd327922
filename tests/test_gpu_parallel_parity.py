"""GPU parity of the PARALLEL schedule's update paths, one wave at a time.

Every benchmarked configuration trains on the parallel schedule: LDS-private
output rows / Huffman nodes and CBOW context rows (priv_read, priv_add,
flush_private), memory-side atomic hot rows, the deep HS kernel under a wave
cap. With a grid of ONE one-wave workgroup every flush scale is exactly 1
(priv_scales: n <= 1) and a privatised row is read as the global row plus the
pending delta, so the launch must train what the sequential oracle trains
(sentences <= 128 tokens: one work item per sentence): what differs is the
summation order, and the delta accumulated in LDS before it reaches the row.
Each case asserts from the launch plan that the intended path ran, checks W, C
and synapses1 against Oracle.train_philox, and repeats the launch on a fresh
handle: one wave has no concurrency, so the repeat must be bit-identical.
"""
import numpy as np
import pytest

from tests.corpus import zipf_sentences
from tests.harness import (MODES, bound_device_from_oracle, check_parity, device_config, device_from_oracle,
                           mode_config, oracle_run)

# Bounds: test_gpu_parity.py's measured multi-sentence bound MULTI (2e-5 norm-
# wise, 2e-3 per element), LIFTED (2e-5 / 5e-3) for rows past 512 floats as
# there; no case has a bound of its own. Measured here
# (profiles/r07a_parity_errors.jsonl; one wave, deterministic, so a build
# reproduces them exactly): <= 5.9e-6 norm-wise (SG-HS's synapses1, d 100,
# flushed every center), <= 1.5e-3 per element (CBOW-HS's C, d 300).
MULTI = (2e-5, 2e-3)
LIFTED = (2e-5, 5e-3)

pytestmark = pytest.mark.gpu

from word2vec_amd import _native as N  # noqa: E402

WINDOW, TABLE = 5, 100_000
KEY = 0x0DEE_9000_0000_7777
LDS_MAX = 163840   # the production workgroup's LDS budget (16 waves x 10 KiB)
LDS_HEADER = 64    # kLdsHeaderWords x 4 bytes (w2v_limits.hpp)
PRIV_MAX, CTX_MAX = 128, 64  # kPrivMax, kCtxMax


def _nv(dim):
    """Floats per lane of the kernels' row (pick_nv, w2v_dev.hip)."""
    need = (dim + 63) // 64
    return next(nv for nv in (1, 2, 3, 4, 5, 6, 8, 12, 16) if nv >= need)


def _lds_for(rows, dim):
    """The smallest W2V_DEBUG_LDS_PER_WAVE that holds `rows` private rows of
    `dim` floats (a row is NV x 64 floats), never above the production budget;
    and the rows that budget holds (plan_private_rows: `fit`)."""
    row_bytes = _nv(dim) * 64 * 4
    lds = min(LDS_MAX, LDS_HEADER + rows * row_bytes)
    return lds, (lds - LDS_HEADER) // row_bytes


# One oracle run per (mode, dim), shared by every case at that shape and left
# unchanged: the oracle's matrices are put back to their initial values after
# the run, so device_from_oracle(initial=False) uploads the same start.
_REFS = {}


def _reference(mode, dim):
    ref = _REFS.get((mode, dim))
    if ref is not None:
        return ref
    sents = zipf_sentences(60, 120, 400, seed=43, ragged=True)
    o = oracle_run(sents, mode, dim=dim, window=WINDOW, iters=1, table_size=TABLE, train=False)
    o.build_sample()
    ids, off = o.samples()
    # the corpus keeps the cases on their path: one work item per sentence, and
    # 128 private rows are a strict subset of the rows / Huffman nodes
    # (4,024 tokens, 3,963 of them in the vocabulary at min_count 2)
    assert len(sents) == 60 and max(map(len, sents)) == 120 and o.train_words == 4024
    assert off.size - 1 == 60 and np.diff(off).max() <= 128
    assert o.V == 320
    init = [o.matrix(k) for k in range(3)]
    order = np.random.default_rng(7).permutation(off.size - 1)
    key = KEY + dim
    o.train_philox(0, 1, order, key, 0)
    want = [o.matrix(k) for k in range(3)]
    words = o.current_words
    for k in range(3):
        if init[k].size:
            o.set_matrix(k, init[k])
    ref = dict(o=o, init=init, want=want, words=words, order=order, key=key, V=o.V)
    _REFS[(mode, dim)] = ref
    return ref


def _launch(ref, mode, dim, monkeypatch, env=None, settings=None, bound=False):
    """The one-wave parallel Philox launch on a fresh handle. `env`: the
    experiment variables read at w2v_dev_create; `settings(d)`: the case's
    setters. Returns (matrices, launch plan, policy, stats, padding), padding
    = the columns past dim of a bound model (None otherwise)."""
    o = ref["o"]
    cfg = device_config(o, mode, dim, WINDOW, 1, TABLE, True, 0.05, 2.5e-6)
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
    d.set_rng(N.W2V_RNG_PHILOX, ref["key"])
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_max_waves(1)
    d.set_private_rate(0)  # no rate limit: the automatic one of a small launch would shrink the ranges
    d.set_progress(0)
    if settings:
        settings(d)
    st = d.train_epoch(0, ref["order"])
    plan, pol = d.launch_plan(), d.policy()
    pad = None
    if bound:
        full = [t.cpu().numpy() if t is not None else None for t in tens]
        got = [np.ascontiguousarray(m[:, :dim]) if m is not None else None for m in full]
        pad = [m[:, dim:] if m is not None else None for m in full]
    else:
        got = list(d.download_model())
    d.close()
    return got, plan, pol, st, pad


def _check_path(ref, mode, plan, pol, st, priv_n, ctx_n, deep, tag):
    print(f"{tag}: priv_n {plan['priv_n']} (from {plan['priv_lo']}) ctx_n {plan['ctx_n']} deep {plan['deep']} "
          f"flush {plan['flush_every']} / {plan['ctx_flush_every']} priv_avg {plan['priv_avg']:g} "
          f"hot_wc {plan['hot_wc']} hot_s {plan['hot_s']} lds {plan['lds_bytes']}")
    assert plan["shared"] == 0
    assert plan["grid"] == 1 and plan["wpb"] == 1 and plan["threads"] == 64, plan
    assert plan["nseg"] == 1, plan
    assert (plan["priv_n"], plan["ctx_n"]) == (priv_n, ctx_n), (plan["priv_n"], plan["ctx_n"], priv_n, ctx_n)
    assert (pol["private_rows"], pol["context_rows"]) == (priv_n, ctx_n), pol
    assert (plan["priv_sc"] == 1.0).all() and (plan["ctx_sc"] == 1.0).all()
    assert plan["hs_hot_avg"] == 0 and plan["hot_sc"].size == 0
    assert plan["deep"] == deep and pol["deep"] == deep, (plan["deep"], deep)
    if mode_config(mode)["train_method"] == "hs" and priv_n > 0:
        assert plan["priv_lo"] == ref["V"] - 1 - priv_n  # the nodes nearest the root
    elif priv_n > 0:
        assert plan["priv_lo"] == 0
    assert st["words"] == ref["words"]
    assert st["nonfinite"] == 0


def _assert_identical(a, b, what):
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: matrix {k}")


def _run_case(mode, dim, monkeypatch, tag, priv_n, ctx_n, deep, env=None, settings=None, bound=False,
              tol=None, also=()):
    """Path + parity + bit-identical repeat of one case; `also`: further
    settings whose launch must give the same bits. Returns the first plan."""
    ref = _reference(mode, dim)
    tag = f"{tag} {mode} d{dim}"
    got, plan, pol, st, pad = _launch(ref, mode, dim, monkeypatch, env, settings, bound)
    _check_path(ref, mode, plan, pol, st, priv_n, ctx_n, deep, tag)
    want = [ref["want"][k] if got[k] is not None else None for k in range(3)]
    if tol is None:
        tol = LIFTED if dim > 512 else MULTI
    check_parity(got, want, ref["init"], *tol, tag=tag)
    if pad is not None:
        for k, p in enumerate(pad):
            if p is not None:
                assert p.shape[1] == _nv(dim) * 64 + 64 - dim
                assert not p.any(), f"{tag}: matrix {k} wrote past column {dim}"
    again, plan2, _, st2, pad2 = _launch(ref, mode, dim, monkeypatch, env, settings, bound)
    assert st2 == st
    _assert_identical(got, again, f"{tag}: repeat on a fresh handle")
    for name, other in also:
        g3, plan3, pol3, st3, _ = _launch(ref, mode, dim, monkeypatch, env, other, bound)
        _check_path(ref, mode, plan3, pol3, st3, priv_n, ctx_n, deep, f"{tag} [{name}]")
        _assert_identical(got, g3, f"{tag}: {name}")
    return plan


def _auto_rows(mode, dim):
    """The automatic private ranges of a capped launch (plan_private_rows, V
    320): 64 output rows or nodes, kPrivMax nodes for skip-gram HS, and CBOW's
    kCtxMax context rows beside them, as far as they fit the production
    budget. Returns (the LDS budget that holds them, output rows, context rows)."""
    cbow = mode.startswith("cbow")
    want = PRIV_MAX if mode == "sg_hs" else 64
    lds, fit = _lds_for(want + (CTX_MAX if cbow else 0), dim)
    p = min(fit, want)
    return lds, p, min(fit - p, CTX_MAX) if cbow else 0


def _hs(mode):
    return mode_config(mode)["train_method"] == "hs"


# 1. Default policy: the automatic ranges with an LDS budget that holds them
# (d 300: 127 rows fit the production budget). The HS modes once on the deep
# kernel the cap chooses, once on the regular kernel (W2V_DEEP_HS=0: the
# private-node path uncapped CBOW-HS runs); CBOW-HS also at configs[1]'s d 200.
DEFAULT_CASES = [(m, d, None) for m in MODES for d in (100, 300)] + \
                [(m, d, 0) for m in ("sg_hs", "cbow_hs") for d in (100, 300)] + \
                [("cbow_hs", 200, None), ("cbow_hs", 200, 0)]


@pytest.mark.parametrize("mode,dim,deep_knob", DEFAULT_CASES)
def test_one_wave_default_policy(mode, dim, deep_knob, monkeypatch):
    lds, p, q = _auto_rows(mode, dim)
    assert p >= 64 and (q >= 63 or not mode.startswith("cbow"))
    env = {"W2V_DEBUG_LDS_PER_WAVE": lds}
    if deep_knob is not None:
        env["W2V_DEEP_HS"] = deep_knob
    deep = 1 if _hs(mode) and deep_knob is None else 0
    _run_case(mode, dim, monkeypatch, f"default deep{deep}", p, q, deep, env=env)


# 2. Private-row counts on the regular kernel: 65 and 128 rows reach the dirty
# mask's second word; 64 context rows are all of kCtxMax.
@pytest.mark.parametrize("mode", ["sg_ns", "sg_hs"])
@pytest.mark.parametrize("rows", [1, 64, 65, 128])
def test_one_wave_private_row_counts(mode, rows, monkeypatch):
    lds, fit = _lds_for(rows, 100)
    assert fit == rows
    _run_case(mode, 100, monkeypatch, f"rows{rows}", rows, 0, 0,
              env={"W2V_DEBUG_LDS_PER_WAVE": lds, "W2V_DEEP_HS": 0}, settings=lambda d: d.set_private_rows(rows))


@pytest.mark.parametrize("mode", ["cbow_ns", "cbow_hs"])
@pytest.mark.parametrize("rows,ctx", [(0, 64), (64, 64), (128, 1)])
def test_one_wave_context_row_counts(mode, rows, ctx, monkeypatch):
    lds, fit = _lds_for(rows + ctx, 100)
    assert fit == rows + ctx

    def settings(d):
        d.set_private_rows(rows)
        d.set_context_private(ctx, 0)

    _run_case(mode, 100, monkeypatch, f"rows{rows}+ctx{ctx}", rows, ctx, 0,
              env={"W2V_DEBUG_LDS_PER_WAVE": lds, "W2V_DEEP_HS": 0}, settings=settings)


# 3. Flush intervals: every center, mid-sentence at counts that divide
# nothing, and only at the end of the kernel. The one-wave scales are 1 with
# and without averaging, so the plain sum must give the same bits.
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("flush,ctx_flush", [(1, 1), (7, 3), (1_000_000, 1_000_000)])
def test_one_wave_flush_intervals(mode, flush, ctx_flush, monkeypatch):
    lds, p, q = _auto_rows(mode, 100)

    def settings(avg):
        def f(d):
            d.set_private_sync(flush, avg)
            d.set_context_private(-1, ctx_flush)
        return f

    plan = _run_case(mode, 100, monkeypatch, f"flush{flush}/{ctx_flush}", p, q, 1 if _hs(mode) else 0,
                     env={"W2V_DEBUG_LDS_PER_WAVE": lds}, settings=settings(8.0),
                     also=[("plain sum (private_average 0)", settings(0.0))])
    assert (plan["flush_every"], plan["ctx_flush_every"]) == (flush, ctx_flush), plan
    assert plan["priv_avg"] == 8.0


# 4. No private rows: every update a memory-side atomic add (hot rows -1: all W
# / C rows and Huffman nodes), or every update a plain read-modify-write (0).
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("hot", [-1, 0])
def test_one_wave_hot_rows(mode, hot, monkeypatch):
    def settings(d):
        d.set_private_rows(0)
        d.set_context_private(0, 0)
        d.set_hot_rows(hot)

    plan = _run_case(mode, 100, monkeypatch, f"hot{hot}", 0, 0, 1 if _hs(mode) else 0, settings=settings)
    V = 320
    assert plan["lds_bytes"] == 0
    assert plan["hot_wc"] == (V if hot < 0 else 0)
    assert plan["hot_s"] == (0 if hot < 0 else V - 1)  # nodes [hot_s, V - 1) take atomics


# 5. Row widths: with case 1 every NV (1, 2, 3, 4, 5, 6, 8, 12, 16; the LDS
# delta rows are NV x 64 floats apart). Skip-gram NS takes its automatic rows;
# CBOW-HS asks for half of what fits, so context rows fit beside the nodes at
# every width (the automatic 64 nodes would fill the budget from d 700 up).
@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
@pytest.mark.parametrize("dim", [40, 150, 200, 350, 512, 700, 1000])
def test_one_wave_row_widths(mode, dim, monkeypatch):
    if mode == "sg_ns":
        lds, fit = _lds_for(64, dim)
        p, q, settings = min(64, fit), 0, None
    else:
        lds, fit = _lds_for(64 + CTX_MAX, dim)
        p = min(64, fit // 2)
        q = min(fit - p, CTX_MAX)

        def settings(d):
            d.set_private_rows(p)
    assert p >= 1 and (q >= 1 or mode == "sg_ns")
    print(f"widths {mode} d{dim}: NV {_nv(dim)}, {fit} rows fit {lds} B -> {p} output + {q} context rows")
    deep = 1 if mode == "cbow_hs" and _nv(dim) <= 12 else 0  # the deep kernel serves NV <= 12
    _run_case(mode, dim, monkeypatch, "widths", p, q, deep, env={"W2V_DEBUG_LDS_PER_WAVE": lds}, settings=settings)


# 6. A bound model at a wider pitch (the benchmark's path: caller-owned torch
# tensors, here 64 floats wider than the kernels' row): parity on the [:V, :d]
# block, and every column from d up to the pitch still exactly zero.
@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
def test_one_wave_bound_model_wider_pitch(mode, monkeypatch):
    lds, p, q = _auto_rows(mode, 100)
    _run_case(mode, 100, monkeypatch, "bound pitch+64", p, q, 1 if _hs(mode) else 0,
              env={"W2V_DEBUG_LDS_PER_WAVE": lds}, bound=True)
