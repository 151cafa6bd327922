"""The launch-policy case matrix (tests/test_gpu_policy.py): one small launch per
case, each hitting a branch of the policy (word2vec_amd/csrc/device/w2v_policy.cpp).
tests/golden/launch_plans.json holds the plan every case gave on the commit
before the policy was separated from the launch code (write_golden)."""
from __future__ import annotations

import functools

import numpy as np

from tests.corpus import zipf_ids

# Defaults of a case; every entry of CASES overrides some.
BASE = dict(mode="sg_ns", dim=100, V=3000, n_sent=3000, sent_len=30, window=5, negative=None, shared=False,
            sequential=False, replicas=1, slice_of=0, calls=(), env={}, huge_window=False)

# the chip holds 8192 waves at d <= 128 and 4096 above: 3,000 sentences leave
# it partly empty (the small-launch rate limit applies), 12,000 fill it
SMALL = dict(n_sent=3000, sent_len=30)
FULL = dict(n_sent=12000, sent_len=20)
SG_NS, SG_HS = dict(mode="sg_ns", dim=100), dict(mode="sg_hs", dim=100)
CBOW_NS, CBOW_HS = dict(mode="cbow_ns", dim=200), dict(mode="cbow_hs", dim=200)
SN = dict(mode="sg_ns", dim=512, shared=True, **FULL)

CASES = {
    # modes, against the chip's size
    "sg_ns_d100_small": dict(SG_NS, **SMALL),
    "sg_ns_d300_small": dict(mode="sg_ns", dim=300, **SMALL),
    "cbow_ns_d200_small": dict(CBOW_NS, **SMALL),
    "cbow_hs_d200_small": dict(CBOW_HS, **SMALL),
    "sg_hs_d100_small": dict(SG_HS, **SMALL),
    "sg_ns_d100_full": dict(SG_NS, **FULL),
    "sg_ns_d300_full": dict(mode="sg_ns", dim=300, **FULL),
    "cbow_ns_d200_full": dict(CBOW_NS, **FULL),
    "cbow_hs_d200_full": dict(CBOW_HS, **FULL),
    "sg_hs_d100_full": dict(SG_HS, **FULL),
    "sg_ns_d100_full_long": dict(SG_NS, n_sent=10000, sent_len=200),  # sentences > 128 tokens: nseg > 1
    "cbow_hs_d200_full_long": dict(CBOW_HS, n_sent=6000, sent_len=300),
    # vocabulary thresholds
    "cbow_hs_d200_V49999": dict(CBOW_HS, V=49999, **FULL),
    "cbow_hs_d200_V50001": dict(CBOW_HS, V=50001, **FULL),
    "cbow_hs_d300_V50001": dict(mode="cbow_hs", dim=300, V=50001, **FULL),  # 96 nodes + 63 context rows do not fit
    "sg_ns_d64_V500000": dict(mode="sg_ns", dim=64, V=500000, n_sent=12000, sent_len=100),
    "sg_hs_d64_V500000": dict(mode="sg_hs", dim=64, V=500000, n_sent=12000, sent_len=100),
    "sg_ns_d64_V499999": dict(mode="sg_ns", dim=64, V=499999, n_sent=12000, sent_len=100),
    # the large-vocabulary HS rule at a small V
    "sg_hs_d100_wide_hs": dict(SG_HS, env={"W2V_WIDE_HS": "1"}, **FULL),
    "cbow_hs_d200_wide_hs": dict(CBOW_HS, env={"W2V_WIDE_HS": "1"}, **FULL),
    # the caller's wave caps
    "sg_ns_d100_cap2048": dict(SG_NS, calls=(("set_max_waves", 2048),), **FULL),
    "sg_ns_d100_cap4096": dict(SG_NS, calls=(("set_max_waves", 4096),), **FULL),
    "sg_hs_d100_cap2048": dict(SG_HS, calls=(("set_max_waves", 2048),), **FULL),
    "sg_hs_d100_cap4096": dict(SG_HS, calls=(("set_max_waves", 4096),), **FULL),
    "cbow_hs_d200_cap4096": dict(CBOW_HS, calls=(("set_max_waves", 4096),), **FULL),
    # the library's own cap: test_gpu_parity.py's huge-window input (window 150, negative 80)
    "sg_ns_huge_window": dict(mode="sg_ns", huge_window=True),
    "cbow_ns_huge_window": dict(mode="cbow_ns", huge_window=True),  # and the per-wave id slices of a window > 127
    # shared negatives, pitch 512
    "shared_neg5": dict(SN, negative=5),
    "shared_neg15": dict(SN, negative=15),
    "shared_neg15_replicas2": dict(SN, negative=15, replicas=2),
    "shared_neg5_cap512": dict(SN, negative=5, calls=(("set_max_waves", 512),)),
    "shared_neg5_small": dict(SN, negative=5, n_sent=300, sent_len=30),
    "shared_neg5_sequential": dict(SN, negative=5, n_sent=300, sent_len=30, sequential=True),
    # the sequential schedule, 4-wave workgroups, wide CBOW windows, a slice
    "sg_ns_d100_sequential": dict(SG_NS, n_sent=300, sent_len=30, sequential=True),
    "cbow_hs_d200_sequential": dict(CBOW_HS, n_sent=300, sent_len=30, sequential=True),
    "sg_ns_d512_full": dict(mode="sg_ns", dim=512, **FULL),
    "cbow_hs_d512_full": dict(mode="cbow_hs", dim=512, **FULL),
    "cbow_ns_d100_window40": dict(mode="cbow_ns", dim=100, window=40, **FULL),
    "cbow_hs_d100_window130": dict(mode="cbow_hs", dim=100, window=130, n_sent=6000, sent_len=40),
    "sg_ns_d100_slice16": dict(SG_NS, n_sent=160000, sent_len=20, slice_of=16),
    "cbow_hs_d200_slice16": dict(CBOW_HS, n_sent=160000, sent_len=20, slice_of=16),
    # setters
    "sg_ns_private_rows0": dict(SG_NS, calls=(("set_private_rows", 0),), **FULL),
    "sg_ns_private_rows128": dict(SG_NS, calls=(("set_private_rows", 128),), **FULL),
    "cbow_hs_private_rows0": dict(CBOW_HS, calls=(("set_private_rows", 0),), **FULL),
    "cbow_hs_private_rows128": dict(CBOW_HS, calls=(("set_private_rows", 128),), **FULL),
    "cbow_hs_context_rows0": dict(CBOW_HS, calls=(("set_context_private", 0, 0),), **FULL),
    "cbow_hs_flush_explicit": dict(CBOW_HS, calls=(("set_private_sync", 128, 8.0), ("set_context_private", -1, 16)),
                                   **FULL),
    "sg_ns_flush_explicit": dict(SG_NS, calls=(("set_private_sync", 256, 8.0),), **FULL),
    "sg_ns_private_average0": dict(SG_NS, calls=(("set_private_sync", 0, 0.0),), **FULL),
    "cbow_hs_private_average0": dict(CBOW_HS, calls=(("set_private_sync", 0, 0.0),), **FULL),
    "sg_hs_hot_rows_all": dict(SG_HS, calls=(("set_hot_rows", -1),), **FULL),
    "sg_hs_hot_rows0": dict(SG_HS, calls=(("set_hot_rows", 0),), **FULL),
    "sg_hs_hot_rows500": dict(SG_HS, calls=(("set_hot_rows", 500),), **FULL),
    "shared_hot_rows_all": dict(SN, negative=5, calls=(("set_hot_rows", -1),)),
    "cbow_hs_private_rate05": dict(CBOW_HS, calls=(("set_private_rate", 0.5),), **FULL),
    "sg_ns_private_rate05": dict(SG_NS, calls=(("set_private_rate", 0.5),), **FULL),
    "sg_hs_hot_auto": dict(SG_HS, calls=(("set_hot_auto", 2.0, 0.5),), **FULL),
    "cbow_ns_hot_auto": dict(CBOW_NS, calls=(("set_hot_auto", 2.0, 0.5),), **FULL),
    # experiment knobs (d300: an uncapped skip-gram NS launch with 112 private rows)
    "knob_scale_resident": dict(CBOW_HS, env={"W2V_SCALE_RESIDENT": "1"}, **SMALL),
    "knob_priv_tail_avg": dict(mode="sg_ns", dim=300, env={"W2V_PRIV_TAIL_AVG": "24"}, **FULL),
    "knob_ctx_avg": dict(CBOW_NS, env={"W2V_CTX_AVG": "32"}, **FULL),
    "knob_hs_hot_avg": dict(SG_HS, env={"W2V_HS_HOT_AVG": "8"}, **FULL),
    "knob_hs_hot_avg_cbow": dict(CBOW_HS, env={"W2V_HS_HOT_AVG": "8"}, **SMALL),
    "knob_wpb": dict(mode="sg_ns", dim=300, env={"W2V_DEBUG_WPB": "4"}, **FULL),
    "knob_lds_per_wave": dict(CBOW_HS, env={"W2V_DEBUG_LDS_PER_WAVE": "4096"}, **FULL),
    "knob_max_blocks": dict(SG_NS, env={"W2V_DEBUG_MAX_BLOCKS": "8"}, **FULL),
    "knob_seg_len0": dict(SG_NS, env={"W2V_SEG_LEN": "0"}, n_sent=10000, sent_len=200),
}


@functools.lru_cache(maxsize=4)
def corpus(V: int, n_sent: int, sent_len: int):
    """A Zipf id corpus over exactly V words, ids by descending count: (counts, ids, sentence offsets)."""
    n = n_sent * sent_len
    assert n >= 2 * V
    raw = np.concatenate([np.arange(V, dtype=np.int64), zipf_ids(n - V, V, seed=17)])  # every word at least once
    np.random.default_rng(5).shuffle(raw)
    counts = np.bincount(raw, minlength=V)
    by_count = np.argsort(-counts, kind="stable")
    rank = np.empty(V, np.int64)
    rank[by_count] = np.arange(V)
    return counts[by_count].astype(np.int64), rank[raw].astype(np.int32), np.arange(0, n + 1, sent_len, dtype=np.int64)


def _trainer(c):
    from tests.planted_ids import gpu_trainer

    counts, ids, soff = corpus(c["V"], c["n_sent"], c["sent_len"])
    V, dim = counts.size, c["dim"]
    hs, cbow = c["mode"].endswith("hs"), c["mode"].startswith("cbow")
    negative = c["negative"] if c["negative"] is not None else (0 if hs else 5)
    W0 = (np.random.default_rng(1).random((V, dim), np.float32) - 0.5) / dim
    Z = np.zeros((V, dim), np.float32)
    t = gpu_trainer(counts, ids, soff, ids.size, c["mode"], dim, negative, 1e-4, W0, None if hs and not cbow else Z,
                    Z if hs else None, 7, window=c["window"], table_size=max(1_000_000, 20 * V))
    return t, soff.size - 1


def run_case(name: str, setenv) -> dict:
    """Run the case's one launch and return DeviceTrainer.launch_plan(). `setenv(name, value)` sets the
    case's experiment knobs (read when the handle is created)."""
    from word2vec_amd import _native as N

    c = dict(BASE, **CASES[name])
    for k, v in c["env"].items():
        setenv(k, v)
    if c["huge_window"]:
        from tests.test_gpu_parity import _huge_window_trainer

        _, t, order = _huge_window_trainer(c["mode"], 2000, 0.025)
        t.set_fixed_alpha(1e-6)  # the plan is what is checked: keep the weights finite at any concurrency
        t.train_epoch(0, order)
        plan = t.launch_plan()
        t.close()
        return plan
    t, n_sent = _trainer(c)
    if c["shared"]:
        t.set_update(N.W2V_UPDATE_SHARED_NEGATIVES)
    if c["sequential"]:
        t.set_schedule(N.W2V_SCHED_SEQUENTIAL)
    if c["replicas"] > 1:
        t._chk(t.lib.w2v_dev_set_replica_count(t.h, c["replicas"]), "w2v_dev_set_replica_count")
    for call in c["calls"]:
        getattr(t, call[0])(*call[1:])
    if c["slice_of"]:
        t.set_order(np.random.default_rng(3).permutation(n_sent))
        t.train_slice_async(0, 0, n_sent // c["slice_of"])
        t.synchronize()
    else:
        t.train_epoch(0)
    plan = t.launch_plan()
    t.close()
    return plan


def to_json(plan: dict) -> dict:
    """Integers and doubles as they are; of the flush scales the float32 bit patterns of the private rows
    (base64; every scale past them must be exactly 1); of the hot-node scales, thousands per case, the count
    and the SHA-256 of their bit patterns."""
    import base64
    import hashlib

    out = {k: v for k, v in plan.items() if not isinstance(v, np.ndarray)}
    for k, n in (("priv_sc", plan["priv_n"]), ("ctx_sc", plan["ctx_n"])):
        v = plan[k].astype("<f4")
        assert (v[n:].view(np.uint32) == np.float32(1).view(np.uint32)).all(), (k, n, v[n:])
        out[k] = base64.b64encode(v[:n].tobytes()).decode()
    hot = plan["hot_sc"].astype("<f4").tobytes()
    out["hot_sc"] = [len(hot) // 4, hashlib.sha256(hot).hexdigest() if hot else ""]
    return out


def write_golden(path, commit: str, n_cu: int, plans: dict) -> None:
    """One line per case: its parameters (what it overrides of BASE) and its plan (to_json)."""
    import json

    lines = [' "%s": %s' % (name, json.dumps({"params": CASES[name], "plan": plans[name]}, separators=(",", ":")))
             for name in sorted(plans)]
    path.write_text('{"commit": "%s", "n_cu": %d, "cases": {\n%s\n}}\n' % (commit, n_cu, ",\n".join(lines)))
