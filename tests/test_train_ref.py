"""CPU checks behind tests/test_gpu_combined.py.

1. The oracle (fp32, oracle/w2v_oracle.cpp) against a float64 restatement of
   one sentence's update (tests/train_ref.py) in the configurations no other
   test pins: hs together with negative sampling, and CBOW as a sum.
2. The inputs of the GPU cases discriminate: on each of them the oracle's
   result with the feature differs from its result without it by at least 100
   times the norm-wise bound the GPU case is held to, on every matrix both
   runs update. A GPU kernel that ignored the feature could not pass.
"""
import numpy as np
import pytest

from tests import combined_cases as cc
from tests.harness import mode_config, rel_err
from tests.train_ref import TrainRef

# (mode, cbow_mean): the combined modes, then every CBOW objective as a sum
PIN_CONFIGS = [("sg_hsns", True), ("cbow_hsns", True), ("cbow_ns", False), ("cbow_hs", False), ("cbow_hsns", False)]

# The fp32 oracle against float64, one 48-token sentence over 400 types at
# dim 48: the suite's single-update class, 1e-5 norm-wise on each matrix's
# update. Measured <= 6.8e-6 (CBOW-HS as a sum, C; then CBOW-NS as a sum, W:
# 5.7e-6; the combined modes <= 2.3e-6), so no matrix has a bound of its own.
PIN_TOL = 1e-5


@pytest.mark.parametrize("mode,cbow_mean", PIN_CONFIGS)
def test_oracle_matches_float64_reference(mode, cbow_mean):
    case = cc.Case("single", mode, 48, cc.SINGLE)
    m = mode_config(mode)
    o = cc.case_oracle(case, cbow_mean=cbow_mean)
    ids, off = o.samples()
    assert off.size == 2 and ids.size == 48 and o.V <= 400
    hs, cbow = m["train_method"] == "hs", m["model"] == "cbow"
    init = [o.matrix(k) if o.matrix(k).size else None for k in range(3)]
    ref = TrainRef(*init, window=5, negative=m["negative"], hs=hs, cbow=cbow, cbow_mean=cbow_mean,
                   keep=o.sample_probs(), table=o.table() if m["negative"] else None,
                   huffman=o.huffman() if hs else None)
    # the first sentence of an epoch trains at init_alpha (the schedule at word 0), as a float
    ref.sentence(ids, 0, np.float32(0.05), 0, cc.KEY)
    o.train_philox(0, 1, np.arange(1), cc.KEY, 0)
    assert 4 <= ref.centers < 48  # subsampling drops some centers and keeps others (keep ~0.27 at count 1)
    assert o.L.orc_last_alpha(o.h) == np.float32(0.05)
    for k, (M, name) in enumerate(zip((ref.W, ref.C, ref.S), "WCS")):
        if M is None:
            continue
        want = M - init[k]
        got = o.matrix(k).astype(np.float64) - init[k]
        if cbow and not m["negative"] and name == "W":  # CBOW-HS reads and writes C and synapses1 only
            np.testing.assert_array_equal(o.matrix(k), init[k])
            assert not want.any()
            continue
        assert np.abs(want).max() > 0, f"{name} did not move"
        e = rel_err(got, want)
        print(f"pin {mode} mean{int(cbow_mean)} {name}: rel_err {e:.2e}, update {np.abs(want).max():.2e} of "
              f"{np.abs(M).max():.2e}")
        assert e < PIN_TOL, (mode, cbow_mean, name, e)


def _discriminates(case, with_upd, without_upd, what, second_order=""):
    """Every matrix both runs update differs by >= 100 x the case's norm-wise
    bound; a matrix in `second_order` is known not to (and must not: the
    table documents the input, it is no allowance)."""
    compared = 0
    for k, name in enumerate("WCS"):
        a, b = with_upd[k], without_upd[k]
        if a is None or b is None or np.abs(a).max() == 0 or np.abs(b).max() == 0:
            continue
        e = rel_err(a, b)
        print(f"{case.id} {what} {name}: differs by {e:.2e} (needs {100 * case.tol[0]:.0e})")
        if name in second_order:
            assert e < 100 * case.tol[0], (case.id, what, name, e)
            continue
        assert e >= 100 * case.tol[0], (case.id, what, name, e)
        compared += 1
    assert compared > 0, (case.id, what)


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


@pytest.mark.parametrize("case", _unique(cc.HSNS_CASES), ids=lambda c: c.id)
def test_combined_inputs_discriminate(case):
    """hs together with negative sampling against hs alone and against
    negative sampling alone: same start, same Philox draws, same schedule."""
    o = cc.case_oracle(case)
    init, upd = cc.philox_update(case, o)
    assert all(u is not None and np.abs(u).max() > 0 for u in upd)  # W, C and synapses1 all move
    model = mode_config(case.mode)["model"]
    for alone in ("hs", "ns"):
        _, u = cc.philox_update(case, cc.case_oracle(case, mode=f"{model}_{alone}"), init)
        _discriminates(case, upd, u, f"against {alone} alone", cc.SECOND_ORDER.get((case.corpus, case.mode, alone), ""))


def test_every_second_order_case_has_a_discriminating_sibling():
    """The single 48-token sentence is kept for parity, but some of its matrices
    cannot tell the combined update from one objective alone; each of its cases
    has a sibling at the same mode and dim on "single_rep", which
    test_combined_inputs_discriminate holds to the full rule."""
    for corpus, mode, _ in cc.SECOND_ORDER:
        for c in cc.HSNS_SINGLE:
            if (c.corpus, c.mode) == (corpus, mode):
                assert c._replace(corpus="single_rep") in cc.HSNS_SINGLE
    assert not any(k[0] == "single_rep" for k in cc.SECOND_ORDER)


@pytest.mark.parametrize("case", _unique(cc.SUM_CASES), ids=lambda c: c.id)
def test_sum_inputs_discriminate(case):
    """cbow_mean off against on."""
    _, upd = cc.philox_update(case, cc.case_oracle(case, cbow_mean=False))
    _, u = cc.philox_update(case, cc.case_oracle(case, cbow_mean=True))
    _discriminates(case, upd, u, "sum against mean")


@pytest.mark.parametrize("case", _unique(cc.FLOOR_CASES), ids=lambda c: c.id)
def test_floor_inputs_discriminate(case):
    """min_alpha 0.02 against the suite's 2.5e-6."""
    _, upd = cc.philox_update(case, cc.case_oracle(case, min_alpha=cc.FLOOR_ALPHA))
    _, u = cc.philox_update(case, cc.case_oracle(case, min_alpha=2.5e-6))
    _discriminates(case, upd, u, "floor 0.02 against 2.5e-6")
