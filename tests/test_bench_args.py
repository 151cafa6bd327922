"""bench.py's argument handling (CPU only): a BASELINE preset (--config) sets
defaults, and flags given explicitly win over it (DESIGN.md §4.1's per-mode
table runs `--config c3 --mode cbow_hs`)."""
import importlib.util
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _parse(argv, monkeypatch):
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return mod.parse()


def test_preset_sets_defaults(monkeypatch):
    a = _parse(["--config", "c1"], monkeypatch)
    assert (a.mode, a.dim, a.negative, a.vocab, a.tokens) == ("sg_ns", 100, 5, 350_000, 17_000_000)


def test_explicit_flags_override_preset(monkeypatch):
    a = _parse(["--config", "c3", "--mode", "cbow_hs", "--dim", "200"], monkeypatch)
    assert (a.mode, a.dim, a.vocab, a.tokens) == ("cbow_hs", 200, 1_000_000, 50_000_000)


def test_no_preset_is_the_headline(monkeypatch):
    a = _parse([], monkeypatch)
    assert (a.mode, a.dim, a.negative, a.gpus) == ("sg_ns", 300, 5, 1)


def test_plain_run_is_lean_by_default(monkeypatch):
    """--full (the CPU baseline leg) and --dump-outputs are off unless asked for."""
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    a = _parse(["--full", "--dump-outputs", "out"], monkeypatch)
    assert (a.full, a.dump_outputs) == (True, "out")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_rows_fixed_and_within_budget():
    """--dump-outputs keeps the same rows for the same arguments: the most
    frequent half and a seeded sample of the rest, within the 64 MB of a dump."""
    import numpy as np

    mod = _bench()
    r = mod.dump_rows(740_391, 2, 300, 1)
    assert np.array_equal(r, mod.dump_rows(740_391, 2, 300, 1))
    assert r.size == mod.PROBE_ROWS and np.array_equal(r[:r.size // 2], np.arange(r.size // 2))
    assert (np.diff(r) > 0).all() and r[-1] < 740_391
    wide = mod.dump_rows(740_391, 3, 2048, 1)  # the widest rows: fewer of them
    assert 3 * wide.size * 2048 * 4 + wide.size * 8 <= 64 << 20
    assert np.array_equal(mod.dump_rows(100, 3, 300, 1), np.arange(100))  # a small matrix goes out whole


def test_dump_outputs_files(tmp_path):
    """dump_outputs writes the sampled rows of the matrices it is handed,
    unpadded and as float32, and the counters and the policy as float64
    vectors in the fixed order of STAT_KEYS / POLICY_KEYS."""
    import numpy as np

    mod = _bench()
    V, d, pitch = 50, 6, 8
    W = np.arange(V * pitch, dtype=np.float32).reshape(V, pitch)
    stats = {k: 10 + i for i, k in enumerate(mod.STAT_KEYS)}
    pstats = {k: 20 + i for i, k in enumerate(mod.STAT_KEYS)}
    policy = {k: 0.5 * i for i, k in enumerate(mod.POLICY_KEYS)}
    out = tmp_path / "out"
    mod.dump_outputs(out, dict(reversed(list(stats.items()))), dict(reversed(list(policy.items()))), pstats,
                     {"W": W, "C": -W, "S": None}, V, d, 1)
    assert sorted(p.name for p in out.iterdir()) == ["C.npy", "W.npy", "policy.npy", "probe_stats.npy", "rows.npy",
                                                      "stats.npy"]
    got = np.load(out / "W.npy")
    assert got.dtype == np.float32 and np.array_equal(got, W[:, :d]) and np.array_equal(np.load(out / "C.npy"), -got)
    assert np.array_equal(np.load(out / "rows.npy"), np.arange(V, dtype=np.float64))
    for name, want in (("stats", stats), ("probe_stats", pstats)):
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float64 and a.tolist() == [want[k] for k in mod.STAT_KEYS]
    assert np.load(out / "policy.npy").tolist() == [0.5 * i for i in range(len(mod.POLICY_KEYS))]


def test_replica_auto_matches_the_class(monkeypatch):
    """bench.py --gpus N exchanges like Word2Vec::replica_mode auto on
    configs[3]'s 10 B / N-token shards (Word2Vec.cpp run_epochs_replicas)."""
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert [mod.auto_replica_mode(n) for n in (2, 4, 8)] == ["average", "average", "adaptive"]
    assert mod.auto_replica_mode(2, 200_000_000) == "sum"  # short shards: the sum for two
    assert mod.auto_replica_mode(3, 200_000_000) == "adaptive"
    assert mod.config3_sync_words(8) == 10_000_000_000 // 8 // 128  # the adaptive divisor's cadence
    assert mod.config3_sync_words(4, "average") == 10_000_000_000 // 4 // 64
    hdr = (ROOT / "include" / "Word2Vec.h").read_text()
    assert "kAutoReplicaRounds = 64;" in hdr and "kAutoAverageWords = 4000000;" in hdr
    assert "kAutoAdaptiveRounds = 128;" in hdr
    assert "kAutoAverageReplicas = 4;" in hdr
