"""GPU parity of the shared-negatives minibatch skip-gram (BASELINE configs[4],
W2V_UPDATE_SHARED_NEGATIVES) against its sequential CPU restatement
(oracle/w2v_oracle.cpp:sgsn_sentence), through the C-ABI.

Both sides draw from the same Philox streams, so every subsampling decision,
window shrink and shared negative is identical; the difference left is fp32
summation order (MFMA 16x16x4 chains + a 4-wave partial sum vs the oracle's
sequential sums). Tolerance: the north star's 1e-5 relative for a single
deterministic update (one sentence); 1e-4 over a multi-sentence epoch, where
rounding differences compound through repeated rows. Measured
(profiles/r07a_parity_errors.jsonl): single sentence <= 2.2e-7 norm-wise at
every width, epochs and the one-workgroup parallel launches <= 8.8e-7.
"""
import numpy as np
import pytest

from oracle import Oracle
from tests.corpus import zipf_sentences
from tests.harness import bound_device_from_oracle, check_parity, device_from_oracle
from word2vec_amd import _native as N
from word2vec_amd.device import Config

pytestmark = pytest.mark.gpu

KEY = 0x0DDC_0FFE_E0DD_F00D


def _oracle(sents, dim, window=5, negative=15, table_size=100_000, subsample=1e-3, alpha=0.05, iters=1,
            min_alpha=2.5e-6):
    o = Oracle(iter=iters, window=window, min_count=2, table_size=table_size, word_dim=dim, negative=negative,
               subsample_threshold=subsample, init_alpha=alpha, min_alpha=min_alpha, cbow_mean=True,
               train_method="ns", model="sg")
    o.load_sentences(sents)
    o.seed(1234)
    o.build_vocab()
    o.init_weights()
    o.build_sample()
    # C starts at zero in the reference (init_weights); give it small random rows
    # so the first update exercises every GEMM term (L != 0, dW != 0).
    rng = np.random.default_rng(5)
    o.set_matrix(1, ((rng.random((o.V, dim)) - 0.5) / dim).astype(np.float32))
    o.set_shared_negatives(True)
    cfg = Config(word_dim=dim, window=window, negative=negative, hs=False, cbow=False, cbow_mean=True, iter=iters,
                 init_alpha=alpha, min_alpha=min_alpha, table_size=table_size)
    return o, cfg


def _setup(sents, dim, window=5, negative=15, table_size=100_000, subsample=1e-3, alpha=0.05, pitch=None,
           iters=1, min_alpha=2.5e-6):
    """The oracle and a sequential-schedule handle on its matrices; `pitch`:
    the matrices as caller-owned torch tensors of that row pitch (bind_model),
    returned as d.bound."""
    o, cfg = _oracle(sents, dim, window, negative, table_size, subsample, alpha, iters, min_alpha)
    if pitch is None:
        d = device_from_oracle(o, cfg, initial=False)
    else:
        d, d.bound, _ = bound_device_from_oracle(o, cfg, pitch=pitch)
    d.set_update(N.W2V_UPDATE_SHARED_NEGATIVES)
    d.set_rng(N.W2V_RNG_PHILOX, KEY)
    d.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    d.set_progress(0)
    return o, d


def _compare(o, d, order, tol, elem_tol, tag, epochs=1):
    """`order`: one epoch's sentence order, or `epochs` of them in a row."""
    init = [o.matrix(0), o.matrix(1)]
    o.train_philox(0, epochs, order, KEY, 0)
    n = len(order) // epochs
    for e in range(epochs):
        st = d.train_epoch(e, order[e * n:(e + 1) * n])
    assert d.get_progress() == o.current_words
    assert epochs > 1 or st["words"] == o.current_words
    dim = init[0].shape[1]
    if getattr(d, "bound", None):  # caller-owned matrices: the columns past dim are padding, and stay zero
        full = [t.cpu().numpy() for t in d.bound[:2]]
        W, Cm = (np.ascontiguousarray(m[:, :dim]) for m in full)
        for k, m in enumerate(full):
            assert m.shape[1] > dim and not m[:, dim:].any(), f"{tag}: matrix {k} wrote past column {dim}"
    else:
        W, Cm, _ = d.download_model()
    for k in (0, 1):
        assert np.abs(o.matrix(k) - init[k]).max() > 0, k
    check_parity([W, Cm], [o.matrix(0), o.matrix(1)], init, tol, elem_tol, tag=tag)
    return st


# Every row width the kernel is instantiated for by word_dim alone (pick_shared_neg:
# pitch / 64 = 1, 2, 3, 4, 5, 6, 8 on two waves, 12 and 16 on four); 64 as before.
SN_DIMS = {40: 1, 64: 1, 100: 2, 150: 3, 200: 4, 300: 5, 350: 6, 512: 8, 700: 12, 1000: 16}


@pytest.mark.parametrize("dim", list(SN_DIMS))
def test_shared_single_sentence(dim):
    sents = zipf_sentences(1, 160, 80, seed=21)
    o, d = _setup(sents, dim)
    assert d.row_pitch() == 64 * SN_DIMS[dim]
    st = _compare(o, d, np.arange(1), 1e-5, 5e-3, f"shared single d{dim}")
    assert st["centers"] > 0 and st["targets"] > st["centers"]
    d.close()


@pytest.mark.parametrize("window,negative", [(5, 15), (8, 15), (3, 5), (1, 1)])
def test_shared_epoch(window, negative):
    sents = zipf_sentences(12, 200, 300, seed=23, ragged=True)
    o, d = _setup(sents, 128, window=window, negative=negative)
    n = o.samples()[1].size - 1
    _compare(o, d, np.random.default_rng(1).permutation(n), 1e-4, 5e-3, f"shared epoch w{window} neg{negative}")
    d.close()


@pytest.mark.parametrize("dim", [200, 700, 1000])
def test_shared_two_epochs_widths(dim):
    """Two epochs over test_shared_epoch's corpus on a 2-wave width and both
    4-wave ones (pitch 768, 1024): rows updated hundreds of times."""
    sents = zipf_sentences(12, 200, 300, seed=23, ragged=True)
    o, d = _setup(sents, dim, iters=2)
    n = o.samples()[1].size - 1
    order = np.concatenate([np.random.default_rng(1 + e).permutation(n) for e in range(2)])
    _compare(o, d, order, 1e-4, 5e-3, f"shared two epochs d{dim}", epochs=2)
    d.close()


# The three instantiations only a bound model reaches (pick_shared_neg's pitch
# / 64 = 7, and 10 and 14 on four waves): no word_dim's own row width is 448,
# 640 or 896 floats.
@pytest.mark.parametrize("dim,pitch", [(384, 448), (512, 640), (768, 896)])
def test_shared_single_sentence_bound_pitch(dim, pitch):
    sents = zipf_sentences(1, 160, 80, seed=21)
    o, d = _setup(sents, dim, pitch=pitch)
    assert d.row_pitch() < pitch and d.model_layout()[3] == pitch
    st = _compare(o, d, np.arange(1), 1e-5, 5e-3, f"shared single d{dim} pitch{pitch}")
    assert st["centers"] > 0 and st["targets"] > st["centers"]
    d.close()


# One workgroup of the PARALLEL schedule: the private C rows (c_priv,
# sn_flush_private) and the staged atomic rows, which the sequential schedule
# never runs. One workgroup takes the sentences in order and every flush scale
# is 1 (priv_scales: one workgroup), so it must train what the oracle trains,
# and the same bits on every run. One oracle run per width, shared by its cases.
_SN_REFS = {}
SN_SLOT_BYTES = 20 * 1024  # kSnPrivBytes: the LDS row slots, at most 32


def _sn_reference(dim):
    ref = _SN_REFS.get(dim)
    if ref is None:
        sents = zipf_sentences(12, 200, 300, seed=23, ragged=True)
        o, cfg = _oracle(sents, dim)
        init = [o.matrix(0), o.matrix(1)]
        order = np.random.default_rng(1).permutation(o.samples()[1].size - 1)
        o.train_philox(0, 1, order, KEY, 0)
        want = [o.matrix(0), o.matrix(1)]
        for k in (0, 1):
            assert np.abs(want[k] - init[k]).max() > 0, k
            o.set_matrix(k, init[k])  # device_from_oracle(initial=False) uploads the start again
        ref = _SN_REFS[dim] = dict(o=o, cfg=cfg, init=init, want=want, order=order, words=o.current_words, V=o.V)
    return ref


def _sn_one_workgroup(ref, dim, private_rows, flush_centers, atomic_rows, monkeypatch):
    if atomic_rows is not None:
        monkeypatch.setenv("W2V_SN_ATOMIC_ROWS", str(atomic_rows))
    d = device_from_oracle(ref["o"], ref["cfg"], initial=False)
    if atomic_rows is not None:
        monkeypatch.delenv("W2V_SN_ATOMIC_ROWS")
    d.set_update(N.W2V_UPDATE_SHARED_NEGATIVES)
    d.set_rng(N.W2V_RNG_PHILOX, KEY)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    d.set_max_waves(2 if dim <= 512 else 4)
    d.set_private_rows(private_rows)
    d.set_private_sync(flush_centers, 8.0)
    d.set_progress(0)
    st = d.train_epoch(0, ref["order"])
    plan = d.launch_plan()
    W, Cm, _ = d.download_model()
    d.close()
    return [W, Cm], plan, st


@pytest.mark.parametrize("dim", [128, 300, 700])
@pytest.mark.parametrize("private_rows,flush_centers", [(0, 0), (4, 1), (10, 7), (4, 1_000_000)])
@pytest.mark.parametrize("atomic", ["auto", "none", "all"])
def test_shared_one_workgroup_parallel(dim, private_rows, flush_centers, atomic, monkeypatch):
    ref = _sn_reference(dim)
    V = ref["V"]
    atomic_rows = {"auto": None, "none": 0, "all": V}[atomic]
    pitch = 64 * {128: 2, 300: 5, 700: 12}[dim]
    waves = 2 if dim <= 512 else 4
    slots = min(32, SN_SLOT_BYTES // (pitch * 4))
    priv_n = min(private_rows, slots)  # d 700: 6 slots, so 10 rows leave none to stage atomic rows in
    tag = f"shared one workgroup d{dim} priv{private_rows} flush{flush_centers} atomic-{atomic}"
    got, plan, st = _sn_one_workgroup(ref, dim, private_rows, flush_centers, atomic_rows, monkeypatch)
    print(f"{tag}: priv_n {plan['priv_n']} of {slots} slots, flush {plan['flush_every']}, "
          f"hot_atomic {plan['hot_atomic']} hot_wc {plan['hot_wc']} of V {V}")
    assert plan["shared"] == 1 and plan["grid"] == 1 and plan["wpb"] == waves and plan["threads"] == 64 * waves, plan
    assert plan["priv_n"] == priv_n, plan
    assert plan["flush_every"] == (flush_centers or 1024), plan
    assert plan["hot_atomic"] == (0 if atomic == "none" else V), plan  # automatic: at least 1000 rows, so all V
    assert (plan["priv_sc"] == 1.0).all()
    assert st["words"] == ref["words"] and st["nonfinite"] == 0
    check_parity(got, ref["want"], ref["init"], 1e-4, 5e-3, tag=tag)
    again, _, st2 = _sn_one_workgroup(ref, dim, private_rows, flush_centers, atomic_rows, monkeypatch)
    assert st2 == st
    for k in (0, 1):
        np.testing.assert_array_equal(got[k], again[k], err_msg=f"{tag}: repeat on a fresh handle, matrix {k}")


def test_shared_parallel_runs_and_counts():
    sents = zipf_sentences(300, 300, 3000, seed=25, ragged=True)
    o, d = _setup(sents, 512, table_size=1_000_000, subsample=1e-4)
    d.set_schedule(N.W2V_SCHED_PARALLEL)
    st = d.train_epoch(0, None)
    ids, off = o.samples()
    assert st["words"] == ids.size
    assert st["sentences"] == off.size - 1
    assert st["draws"] == 15 * st["centers"]  # every center with a context draws 15
    W, Cm, _ = d.download_model()
    assert np.isfinite(W).all() and np.isfinite(Cm).all()
    d.close()


def test_shared_rejects_unsupported():
    from word2vec_amd.device import DeviceTrainer

    for kw in (dict(hs=True, negative=0), dict(cbow=True), dict(negative=16), dict(window=9)):
        base = dict(word_dim=64, window=5, negative=5, hs=False, cbow=False, iter=1, table_size=10_000)
        base.update(kw)
        d = DeviceTrainer(Config(**base))
        with pytest.raises(N.DevError, match="shared negatives"):
            d.set_update(N.W2V_UPDATE_SHARED_NEGATIVES)
        d.close()
