"""GPU parity: the HIP kernels (through the C-ABI) against the CPU oracle.

Replay mode feeds the kernels the reference's own mt19937 draw stream (recorded
by the oracle in the reference's order), so every subsampling decision, window
shrink and negative is identical; the remaining difference is fp32 summation
order (wave-tree dot products vs the oracle's sequential sum). Philox mode
checks the throughput-mode RNG bit-for-bit and its arithmetic the same way.
Tolerance: north_star's 1e-5 relative for a single deterministic update
(one sentence); looser bounds for multi-sentence runs where rounding
differences compound through repeated rows.
"""
import numpy as np
import pytest

from tests.corpus import zipf_sentences
from tests.harness import MODES, check_parity, device_config, device_from_oracle, oracle_run

# Bounds, per test, from the measured errors (profiles/r03b_,
# r03c_parity_errors.jsonl; the runs are one wavefront, deterministic, so a
# build reproduces them exactly):
#   single update (48 tokens over 400 types), north_star's 1e-5 norm-wise:
#     measured <= 2.1e-6 except CBOW-NS's W (5.7e-5: ulp_matrices, harness);
#     per element <= 8.5e-4 -> 2e-3, CBOW-NS's W 3.4e-3 -> 5e-3 (the same
#     last-bit roundings of a ~1e-6 update)
#   the original single sentence (120 tokens over 60 types, every row updated
#     dozens of times): 1e-5 norm-wise too, except CBOW-NS's W, measured
#     2.2e-5 (its own bound, 5e-5); per element <= 1.1e-3 (SG-HS's W), CBOW-NS's
#     W 2.1e-3 (5e-3)
#   multi-sentence runs (epochs, widths, Philox, wide windows): measured
#     <= 3.0e-6 norm-wise, <= 9.2e-4 per element -> 2e-5 / 2e-3
#   round 4's lifted limits (rows of 1100 / 2048 floats, negative 64-300,
#     window 200): measured <= 1.7e-5 norm-wise, 4.1e-3 per element (CBOW-HS's
#     C at d 2048: 2048-term dot products, rows updated dozens of times;
#     profiles/r04a_parity_errors.jsonl) -> 2e-5 / 5e-3
SINGLE = (1e-5, 2e-3)
MULTI = (2e-5, 2e-3)
LIFTED = (2e-5, 5e-3)

pytestmark = pytest.mark.gpu

from word2vec_amd import _native as N  # noqa: E402


def _run_replay(mode, sentences, dim, window, iters, table_size=100_000, cbow_mean=True, min_count=2):
    o = oracle_run(sentences, mode, dim=dim, window=window, iters=iters, table_size=table_size,
                   cbow_mean=cbow_mean, min_count=min_count)
    cfg = device_config(o, mode, dim, window, iters, table_size, cbow_mean, 0.05, 2.5e-6)
    d = device_from_oracle(o, cfg, initial=True)
    stream, offs, orders = o.stream(iters)
    d.upload_replay(stream, offs)
    d.set_rng(N.W2V_RNG_REPLAY, 0)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    n = orders.size // iters
    for e in range(iters):
        d.train_epoch(e, orders[e * n:(e + 1) * n])
    got = d.download_model()
    want = (o.matrix(0), o.matrix(1) if cfg.negative > 0 or cfg.cbow else None, o.matrix(2) if cfg.hs else None)
    init = (o.matrix(0, True), o.matrix(1, True) if want[1] is not None else None,
            o.matrix(2, True) if want[2] is not None else None)
    assert d.get_progress() == o.current_words
    return got, want, init


# The low-occupancy deep-pipeline HS kernel (train_epoch_deep_kernel, round 6:
# the large-vocabulary HS policy's capped launches) gathers a Huffman path
# 8-16 nodes at a time instead of 4; forced on the sequential Philox schedule
# (W2V_DEEP_HS=1, read at w2v_dev_create) it must train what the oracle does,
# at every row width it serves (NV <= 12).
@pytest.mark.parametrize("mode", ["sg_hs", "cbow_hs"])
@pytest.mark.parametrize("dim", [40, 100, 200, 300, 512, 700])
def test_philox_sequential_deep_hs(mode, dim, monkeypatch):
    sents = zipf_sentences(8, 160, 300, seed=41, ragged=True)
    o = oracle_run(sents, mode, dim=dim, window=5, iters=1, table_size=100_000, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, 5, 1, 100_000, True, 0.05, 2.5e-6)
    monkeypatch.setenv("W2V_DEEP_HS", "1")
    d = device_from_oracle(o, cfg, initial=False)
    monkeypatch.delenv("W2V_DEEP_HS")
    init = [o.matrix(k) for k in range(3)]
    key = 0x0DEE_9000_0000_0001 + dim
    order = np.random.default_rng(dim).permutation(o.samples()[1].size - 1)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    assert d.policy()["deep"] == 1
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *MULTI, tag=f"philox deep {mode} d{dim}")
    d.close()


def test_one_wave_large_vocab_hs_policy(monkeypatch):
    """The large-vocabulary HS policy's parallel path — the wave cap, the deep
    kernel and skip-gram's per-wave write-combining node cache (summed after
    every center) — forced at a small vocabulary (W2V_WIDE_HS=1) and run on ONE
    wave of the parallel Philox schedule, where it must train what the
    sequential oracle does: each wave reads node + its own pending delta, so
    the cache keeps the reference's per-thread view (sentences <= 128 tokens:
    one work item per sentence, the alpha refresh at sentence starts as in the
    sequential loop)."""
    sents = zipf_sentences(60, 120, 400, seed=43, ragged=True)
    o = oracle_run(sents, "sg_hs", dim=300, window=5, iters=1, table_size=100_000, train=False)
    o.build_sample()
    cfg = device_config(o, "sg_hs", 300, 5, 1, 100_000, True, 0.05, 2.5e-6)
    monkeypatch.setenv("W2V_WIDE_HS", "1")
    d = device_from_oracle(o, cfg, initial=False)
    monkeypatch.delenv("W2V_WIDE_HS")
    init = [o.matrix(k) for k in range(3)]
    key = 0x0DEE_9000_0000_7777
    order = np.random.default_rng(7).permutation(o.samples()[1].size - 1)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_max_waves(1)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    pol = d.policy()
    assert pol["deep"] == 1 and pol["private_rows"] > 0 and pol["flush_centers"] == 1, pol
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *MULTI, tag="one-wave large-vocabulary HS policy sg_hs d300")
    d.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dim", [48, 100, 200, 300, 512])
def test_replay_single_sentence(mode, dim):
    """north_star: a single deterministic update (one sentence, the reference's
    own draws) within 1e-5 relative, at the configs' row widths (configs[0]
    d100, configs[1] d200, configs[2]/[3] d300, configs[4] d512)."""
    # 48 tokens over 400 word types: a single deterministic minibatch (the
    # measured 120-token / 60-type sentence reached 2.2e-5 on CBOW-NS's W at
    # d200: its few rows were updated dozens of times and the rounding
    # compounds, which is the multi-update regime below)
    sents = zipf_sentences(1, 48, 400, seed=3)
    got, want, init = _run_replay(mode, sents, dim=dim, window=5, iters=1, table_size=10_000, min_count=1)
    cbow_ns = mode == "cbow_ns"
    check_parity(got, want, init, *SINGLE, tag=f"single {mode} d{dim}", ulp_matrices=(0,) if cbow_ns else (),
                 overrides={0: (SINGLE[0], 5e-3)} if cbow_ns else None)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dim", [100, 200, 300, 512])
def test_replay_repeated_rows_sentence(mode, dim):
    """The original single-sentence input (one 120-token sentence over 60 word
    types, every row updated many times within it), held to north_star's 1e-5
    so a regression stays visible; CBOW-NS's W keeps its measured
    2.2e-5 under a bound of its own (5e-5), printed against 1e-5."""
    sents = zipf_sentences(1, 120, 60, seed=3)
    got, want, init = _run_replay(mode, sents, dim=dim, window=5, iters=1, table_size=10_000)
    over = {0: (5e-5, 5e-3)} if mode == "cbow_ns" else {}
    check_parity(got, want, init, 1e-5, 2e-3, tag=f"sentence {mode} d{dim}", overrides=over)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dim", [100, 300])
def test_replay_epoch(mode, dim):
    sents = zipf_sentences(12, 200, 400, seed=5, ragged=True)
    got, want, init = _run_replay(mode, sents, dim=dim, window=5, iters=2)
    check_parity(got, want, init, *MULTI, tag=f"epoch {mode} d{dim}")


# Every instantiated row width (floats per lane NV = ceil(d / 64): 1, 2, 3, 4,
# 5, 6, 8, 12, 16; w2v_dev.hip pick_nv), including configs[1]'s d=200 (NV 4),
# and dims that leave part of the last 64-lane chunk idle.
NV_DIMS = [40, 100, 150, 200, 300, 350, 512, 700, 1000]


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
@pytest.mark.parametrize("dim", NV_DIMS)
def test_replay_epoch_row_widths(mode, dim):
    sents = zipf_sentences(8, 160, 300, seed=31, ragged=True)
    got, want, init = _run_replay(mode, sents, dim=dim, window=5, iters=2)
    check_parity(got, want, init, *MULTI, tag=f"widths {mode} d{dim}")


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
@pytest.mark.parametrize("dim", NV_DIMS)
def test_philox_sequential_row_widths(mode, dim):
    sents = zipf_sentences(8, 160, 300, seed=37, ragged=True)
    o = oracle_run(sents, mode, dim=dim, window=5, iters=1, table_size=100_000, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, 5, 1, 100_000, True, 0.05, 2.5e-6)
    d = device_from_oracle(o, cfg, initial=False)
    init = [o.matrix(k) for k in range(3)]
    key = 0x0DDB_A11C_AFE0_0001 + dim
    order = np.random.default_rng(dim).permutation(o.samples()[1].size - 1)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *MULTI, tag=f"philox widths {mode} d{dim}")
    d.close()


@pytest.mark.parametrize("mode", list(MODES))
def test_philox_sequential(mode):
    sents = zipf_sentences(10, 150, 300, seed=9, ragged=True)
    dim, window, iters, ts = 64, 5, 1, 100_000
    o = oracle_run(sents, mode, dim=dim, window=window, iters=iters, table_size=ts, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, window, iters, ts, True, 0.05, 2.5e-6)
    d = device_from_oracle(o, cfg, initial=False)
    init = [o.matrix(k) for k in range(3)]
    key = 0x1234_5678_9ABC_DEF0
    n = o.samples()[1].size - 1
    order = np.random.default_rng(0).permutation(n)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *MULTI, tag=f"philox {mode}")


@pytest.mark.parametrize("mode,dim", [("sg_ns", 300), ("cbow_hs", 300), ("cbow_hs", 200), ("sg_ns", 100)])
def test_parallel_runs_and_counts(mode, dim):
    """Full-concurrency parallel schedule with the default update policy (for
    CBOW-HS: LDS-private Huffman top nodes and context rows; configs[1] is
    CBOW-HS d200): size-independent properties."""
    sents = zipf_sentences(400, 300, 2000, seed=11, ragged=True)
    o = oracle_run(sents, mode, dim=dim, window=5, iters=1, table_size=1_000_000, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, 5, 1, 1_000_000, True, 0.05, 2.5e-6)
    d = device_from_oracle(o, cfg, initial=False)
    d.set_rng(N.W2V_RNG_PHILOX, 7)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_progress(0)
    st = d.train_epoch(0, None)
    ids, off = o.samples()
    assert st["words"] == ids.size
    assert st["sentences"] == off.size - 1
    assert st["nonfinite"] == 0
    W, Cm, S = d.download_model()
    for m in (W, Cm, S):
        if m is not None:
            assert np.isfinite(m).all()
    # kept fraction matches E[min(p,1)] over tokens within a few sigma
    p = o.sample_probs()[ids].astype(np.float64)
    exp_kept = p.sum()
    sd = np.sqrt((p * (1 - p)).sum()) + 1
    assert abs(st["centers"] - exp_kept) < 6 * sd + (0 if mode.startswith("sg") else 0.01 * exp_kept)
    pol = d.policy()
    if mode == "cbow_hs":
        # automatic HS flush interval (w2v_policy.cpp auto_hs_flush): a 120 K-token
        # launch gives each workgroup far fewer than 128 x 128 centers -> 64 / 32
        assert (pol["flush_centers"], pol["context_flush"]) == (64, 32), pol
        d.set_private_sync(32, 8.0)  # explicit intervals win over the automatic one
        d.set_context_private(-1, 16)
        d.set_progress(0)
        assert d.train_epoch(0, None)["nonfinite"] == 0
        pol = d.policy()
        assert (pol["flush_centers"], pol["context_flush"]) == (32, 16), pol
    else:
        assert pol["context_flush"] == 0 and pol["flush_centers"] in (0, 1024), pol


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs", "sg_hs"])
def test_parallel_segments_match_whole_sentences(mode, monkeypatch):
    """Sentence segments as work items (w2v_policy.hpp kSegLen): one wave taking a
    sentence's segments in turn trains exactly what it trains taking the whole
    sentence (same centers, windows over the whole sentence, same Philox draws,
    same flush points); fixed alpha, since the schedule reads the word counter,
    which segments advance earlier."""
    sents = zipf_sentences(6, 700, 300, seed=13, ragged=True)
    dim = 100
    o = oracle_run(sents, mode, dim=dim, window=5, iters=1, table_size=100_000, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, 5, 1, 100_000, True, 0.05, 2.5e-6)
    ids, off = o.samples()
    assert np.diff(off).max() > 128  # more than one segment per sentence
    order = np.random.default_rng(1).permutation(off.size - 1)
    out = {}
    for seg in ("0", "64", "128"):
        monkeypatch.setenv("W2V_SEG_LEN", seg)
        d = device_from_oracle(o, cfg, initial=False)
        d.set_rng(N.W2V_RNG_PHILOX, 99)
        d.set_schedule(N.W2V_SCHED_PARALLEL)
        d.set_max_waves(1)
        d.set_fixed_alpha(0.025)
        d.set_progress(0)
        st = d.train_epoch(0, order)
        out[seg] = (st, d.download_model())
        d.close()
    st0, m0 = out["0"]
    assert st0["words"] == ids.size and st0["sentences"] == off.size - 1
    for seg in ("64", "128"):
        st, m = out[seg]
        assert st == st0, seg
        for a, b in zip(m0, m):
            if a is not None:
                np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("window", [40, 127])
def test_replay_wide_window(mode, window):
    """Windows wider than a wavefront (2 * window + 1 > 64): skip-gram loads
    the contexts past the first 64 positions one by one, CBOW runs the
    wide-window kernel (the span's positions held 4 per lane)."""
    sents = zipf_sentences(6, 300, 150, seed=21, ragged=True)
    got, want, init = _run_replay(mode, sents, dim=64, window=window, iters=1, table_size=10_000)
    check_parity(got, want, init, *MULTI, tag=f"wide replay {mode} w{window}")


@pytest.mark.parametrize("mode", ["cbow_ns", "cbow_hs"])
@pytest.mark.parametrize("window", [31, 32])
def test_replay_cbow_widest_lane_window(mode, window):
    """The two sides of the CBOW kernels' window threshold: window 31 is the
    widest the one-position-per-lane form takes (a span of 63 positions), window
    32 the narrowest of the four-per-lane form (65). Every sentence has 150
    tokens and min_count 1 drops none, so a center whose shrink draw is 0 has
    the full span (the shrink is uniform over [0, window): of the 472 centers
    that survive subsampling, 10 have a span of 63 at window 31 and 9 a span of
    65 at window 32, read off the recorded stream)."""
    sents = zipf_sentences(8, 150, 150, seed=27)
    assert min(len(s) for s in sents) >= 70
    got, want, init = _run_replay(mode, sents, dim=48, window=window, iters=1, table_size=10_000, min_count=1)
    check_parity(got, want, init, *MULTI, tag=f"lane-window replay {mode} w{window}")


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns", "cbow_hs"])
def test_philox_sequential_wide_window(mode):
    sents = zipf_sentences(6, 300, 150, seed=23, ragged=True)
    dim, window, iters, ts = 64, 60, 1, 100_000
    o = oracle_run(sents, mode, dim=dim, window=window, iters=iters, table_size=ts, train=False)
    o.build_sample()
    cfg = device_config(o, mode, dim, window, iters, ts, True, 0.05, 2.5e-6)
    d = device_from_oracle(o, cfg, initial=False)
    init = [o.matrix(k) for k in range(3)]
    key = 0x0BAD_F00D_1234_5678
    n = o.samples()[1].size - 1
    order = np.random.default_rng(1).permutation(n)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *MULTI, tag=f"wide philox {mode}")


def _philox_sequential(mode, sents, dim, window, negative, key, ts=100_000, seed=1, tag=""):
    """Philox draws, one wavefront, against the oracle's Philox mode (the
    restated counter, incl. the draw index's high bits past 255)."""
    from oracle import Oracle

    from tests.harness import MODES as HM

    m = HM[mode]
    neg = negative if m["train_method"] == "ns" else 0
    o = Oracle(iter=1, window=window, min_count=2, table_size=ts, word_dim=dim, negative=neg,
               subsample_threshold=1e-3, init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True,
               train_method=m["train_method"], model=m["model"])
    o.load_sentences(sents)
    o.seed(1234)
    o.build_vocab()
    o.init_weights()
    o.build_sample()
    from word2vec_amd.device import Config

    cfg = Config(word_dim=dim, window=window, negative=neg, hs=m["train_method"] == "hs", cbow=m["model"] == "cbow",
                 cbow_mean=True, iter=1, init_alpha=0.05, min_alpha=2.5e-6, table_size=ts)
    d = device_from_oracle(o, cfg, initial=False)
    init = [o.matrix(k) for k in range(3)]
    order = np.random.default_rng(seed).permutation(o.samples()[1].size - 1)
    o.train_philox(0, 1, order, key, 0)
    d.set_rng(N.W2V_RNG_PHILOX, key)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    st = d.train_epoch(0, order)
    assert st["words"] == o.current_words
    got = d.download_model()
    want = [o.matrix(k) if got[k] is not None else None for k in range(3)]
    check_parity(got, want, init, *LIFTED, tag=tag)
    d.close()
    return st


# Round 4: the reference's unbounded hyper-parameters (Word2Vec.cpp:254, 285,
# 335). Negatives past 63 are drawn and deduplicated 64 at a time
# (ns_word_many); CBOW windows past 127 are walked from the sentence
# (cbow_center_huge); rows past 1024 floats take the 24 / 32 floats-per-lane
# kernels.
@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns"])
@pytest.mark.parametrize("negative", [64, 100])
def test_replay_many_negatives(mode, negative):
    """The reference's own mt19937 draws (table positions recorded in its
    order) at negative 64 / 100: targets are the positive plus the distinct
    negatives (parity at negative 100)."""
    sents = zipf_sentences(4, 150, 3000, seed=41, ragged=True)
    got, want, init = _run_replay_neg(mode, sents, negative)
    check_parity(got, want, init, *LIFTED, tag=f"replay {mode} neg{negative}")


def _run_replay_neg(mode, sents, negative, dim=48, window=5):
    from oracle import Oracle

    from tests.harness import MODES as HM

    m = HM[mode]
    o = Oracle(iter=1, window=window, min_count=1, table_size=100_000, word_dim=dim, negative=negative,
               subsample_threshold=1e-3, init_alpha=0.05, min_alpha=2.5e-6, cbow_mean=True,
               train_method=m["train_method"], model=m["model"])
    o.load_sentences(sents)
    o.seed(4321)
    o.build_vocab()
    o.init_weights()
    o.train(record=True)
    from word2vec_amd.device import Config

    cfg = Config(word_dim=dim, window=window, negative=negative, hs=False, cbow=m["model"] == "cbow", cbow_mean=True,
                 iter=1, init_alpha=0.05, min_alpha=2.5e-6, table_size=100_000)
    d = device_from_oracle(o, cfg, initial=True)
    stream, offs, orders = o.stream(1)
    d.upload_replay(stream, offs)
    d.set_rng(N.W2V_RNG_REPLAY, 0)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    d.train_epoch(0, orders)
    got = d.download_model()
    want = (o.matrix(0), o.matrix(1), None)
    init = (o.matrix(0, True), o.matrix(1, True), None)
    assert d.get_progress() == o.current_words
    d.close()
    return got, want, init


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns"])
@pytest.mark.parametrize("negative", [100, 300])
def test_philox_sequential_many_negatives(mode, negative):
    """Philox at negative 100 and 300 (draw indices past 255 use the counter's
    high bits, restated in the oracle)."""
    sents = zipf_sentences(4, 150, 3000, seed=43, ragged=True)
    _philox_sequential(mode, sents, 48, 5, negative, 0x5151_0000_0000_0000 + negative, tag=f"philox {mode} neg{negative}")


@pytest.mark.parametrize("mode", list(MODES))
def test_replay_huge_window(mode):
    """Window 200 (span up to 401 positions): CBOW walks the span from the
    sentence (cbow_center_huge), skip-gram reads contexts past 64 one by one
    (parity at window 200)."""
    sents = zipf_sentences(3, 700, 300, seed=45, ragged=True)
    got, want, init = _run_replay(mode, sents, dim=48, window=200, iters=1, table_size=10_000)
    check_parity(got, want, init, *LIFTED, tag=f"huge replay {mode} w200")


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_ns", "cbow_hs"])
def test_philox_sequential_huge_window(mode):
    sents = zipf_sentences(3, 700, 300, seed=47, ragged=True)
    _philox_sequential(mode, sents, 48, 200, 5, 0x7777_0000_1111_0000, tag=f"huge philox {mode}")


@pytest.mark.parametrize("mode", ["sg_ns", "cbow_hs"])
@pytest.mark.parametrize("dim", [1100, 2048])
def test_replay_wide_rows(mode, dim):
    """Rows past 1024 floats (24 and 32 floats per lane)."""
    sents = zipf_sentences(2, 120, 200, seed=49, ragged=True)
    got, want, init = _run_replay(mode, sents, dim=dim, window=5, iters=1, table_size=10_000)
    check_parity(got, want, init, *LIFTED, tag=f"wide rows {mode} d{dim}")


def _huge_window_trainer(mode, vmax, alpha):
    from word2vec_amd.device import Config

    sents = zipf_sentences(200, 400, vmax, seed=51, ragged=True)
    o = oracle_run(sents, mode, dim=64, window=150, iters=1, table_size=100_000, train=False)
    o.build_sample()
    m = MODES[mode]
    cfg = Config(word_dim=64, window=150, negative=80, hs=False, cbow=m["model"] == "cbow", cbow_mean=True,
                 iter=1, init_alpha=alpha, min_alpha=2.5e-6, table_size=100_000)
    d = device_from_oracle(o, cfg, initial=False)
    d.set_rng(N.W2V_RNG_PHILOX, 99)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_progress(0)
    return o, d, np.random.default_rng(3).permutation(o.samples()[1].size - 1)


def test_parallel_huge_window_and_many_negatives_run():
    """The parallel schedule with window 150 and negative 80 on 64 waves
    (several workgroups, each wave its own slice of the huge-window scratch),
    alpha 0.0025, 20 K Zipf ranks: trains, counts every word once, stays finite."""
    for mode in ("cbow_ns", "sg_ns"):
        o, d, order = _huge_window_trainer(mode, 20000, 0.0025)
        d.set_max_waves(64)
        st = d.train_epoch(0, order)
        ids, _ = o.samples()
        assert st["words"] == ids.size and st["nonfinite"] == 0
        W, Cm, _ = d.download_model()
        assert np.isfinite(W).all() and np.isfinite(Cm).all()
        d.close()


def test_parallel_huge_window_reference_alpha_full_concurrency():
    """The r04a input at the reference's alpha 0.025 with the library's
    default concurrency (window 150, negative 80, V 1,807: each skip-gram
    center updates ~12 K target rows, every row ~7 times). VERDICT r04 "next"
    2. The sequential reference stays finite on it (max |W| 72 with its own
    draws, 119 with the Philox draws), but the reference's OWN parallel loop
    does not: its OpenMP Hogwild (Word2Vec.cpp:375-394, the oracle's
    orc_train_omp_shared) reaches max |W| 152 / 1.0e3 / 1.6e5 on 2 / 4 / 8
    threads (tests/probes/divergence_probe.py,
    profiles/r05_divergence_oracle.log). On the GPU skip-gram's max |W| is 115
    / 124 / 130 / 142 at 1 / 2 / 4 / 8 waves, 667 at 16, 1e7-1e16 at 32-64 and
    non-finite from 128 waves up (profiles/r05a_1_*, r05b_2_*, r05d_4_*), so
    a parallel launch caps its waves in flight by the vocabulary's pressure
    (effective_max_waves, w2v_policy.cpp: here 9; every benchmarked shape stays
    uncapped) and trains this input to the sequential run's magnitude. An
    explicit 512-wave launch fails LOUDLY (W2V_ERR_DIVERGED) when it diverges,
    never with silent non-finite weights: with round 4's 64 private rows it
    diverged in every suite run; the 96 rows skip-gram NS privatises since
    round 5 damp more of this small vocabulary, and one suite
    run in four then stayed finite (profiles/r05ag_tests.log), so that launch
    may end either way — but which way is checked: a divergence must come
    with the device's non-finite counter set, and a finite end must be the
    Hogwild inflation the cap exists for (max |W| above the capped run's, as
    at 16 waves: 667 against ~140-290). A launch at alpha 5 must fail
    loudly."""
    capped_max = None
    for mode, wmax in (("cbow_ns", 10.0), ("sg_ns", 400.0)):
        o, d, order = _huge_window_trainer(mode, 2000, 0.025)
        st = d.train_epoch(0, order)
        pol = d.policy()
        assert st["words"] == o.samples()[0].size and st["nonfinite"] == 0
        W, Cm, _ = d.download_model()
        print(f"huge window {mode} alpha 0.025: wave cap {pol['wave_cap']}, max |W| {np.abs(W).max():.3g}")
        assert np.isfinite(W).all() and np.isfinite(Cm).all() and np.abs(W).max() < wmax
        # skip-gram: ~12 K rows per center, capped; CBOW-NS: 232, below its 200 sentences' waves
        assert (0 < pol["wave_cap"] <= 16) if mode == "sg_ns" else pol["wave_cap"] == 0
        if mode == "sg_ns":
            capped_max = float(np.abs(W).max())
        d.close()
    o, d, order = _huge_window_trainer("sg_ns", 2000, 0.025)
    d.set_max_waves(512)
    try:
        st = d.train_epoch(0, order)
    except N.DevError as e:
        assert e.code == N.W2V_ERR_DIVERGED
        assert d.read_stats()["nonfinite"] > 0  # the counter that raised it
        print("huge window sg_ns at 512 waves: diverged (W2V_ERR_DIVERGED)")
    else:
        W, Cm, _ = d.download_model()
        assert st["nonfinite"] == 0 and np.isfinite(W).all() and np.isfinite(Cm).all()
        print(f"huge window sg_ns at 512 waves: finite, max |W| {np.abs(W).max():.3g} (capped {capped_max:.3g})")
        assert np.abs(W).max() > capped_max  # without the cap the weights inflate
    assert d.policy()["wave_cap"] == 0  # the caller's cap, not the library's
    d.close()
    o, d, order = _huge_window_trainer("sg_ns", 2000, 5.0)
    with pytest.raises(N.DevError) as e:
        d.train_epoch(0, order)
    assert e.value.code == N.W2V_ERR_DIVERGED
    d.close()


def test_window_limit():
    from word2vec_amd.device import Config, DeviceTrainer

    DeviceTrainer(Config(word_dim=16, window=4096, negative=4096, cbow=True, table_size=1000))
    with pytest.raises(N.DevError, match="window"):
        DeviceTrainer(Config(word_dim=16, window=4097, negative=5, table_size=1000))
    with pytest.raises(N.DevError, match="negative"):
        DeviceTrainer(Config(word_dim=16, window=5, negative=4097, table_size=1000))
