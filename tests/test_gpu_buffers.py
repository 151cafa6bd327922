"""Device memory over the whole life cycle of the C-ABI's handles: four cycles of
create / upload / train / share / ingest / query / exchange / destroy at sizes
where every large buffer is at least 16 MiB, so that a buffer leaked once per
cycle shows in the device's free memory (an allocation granule cannot hide it).

Sizes: vocabulary 16384 x dimension 256 (row pitch 256 floats: W and C are
16 MiB each), a unigram table of 4 Mi entries (16 MiB), a corpus of 4 Mi token
ids (16 MiB) in 1000-token sentences, a 16 MiB text for the ingest. The
vocabulary products are synthetic (keep-probabilities of 1, uniform table
bounds): nothing here is compared with the oracle.

Bound: after cycles 2..4 the free memory is at least the value after cycle 1
(the warm-up: code objects, the runtime's own lazy allocations) minus 16 MiB.
That is less than the smallest of these buffers, so any of them leaked once
per cycle fails. The buffers below 1 MiB (Huffman arrays, counters, scratch)
are beneath what this can see.

Corpus ownership: a handle that shares another's corpus keeps training on it
after the owner is destroyed (the last handle to let go frees it)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
V, DIM = 16384, 256
TABLE = 4 * MIB
N_TOK, SENT = 4 * MIB, 1000
TEXT_BYTES = 16 * MIB
CYCLES = 4


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    rng = np.random.default_rng(7)
    ids = rng.integers(0, V, N_TOK, dtype=np.int32)
    offsets = np.append(np.arange(0, N_TOK, SENT, dtype=np.int64), N_TOK)
    W = (rng.random((V, DIM), np.float32) - 0.5) / DIM
    # the text: 8 bytes per token, a 7-digit word and a space (a newline after every 1000th)
    words = np.array([list(b"%07d " % w) for w in range(V)], np.uint8)
    text = words[rng.integers(0, V, TEXT_BYTES // 8)]
    text[SENT - 1::SENT, 7] = ord("\n")
    path = tmp_path_factory.mktemp("buffers") / "text.txt"
    path.write_bytes(text.tobytes())
    return {
        "ids": ids, "offsets": offsets, "W": W, "C": np.zeros((V, DIM), np.float32),
        "keep": np.ones(V, np.float32), "bounds": np.arange(V + 1, dtype=np.int64) * (TABLE // V),
        "table": np.repeat(np.arange(V, dtype=np.uint32), TABLE // V), "text": path,
        "index": {"%07d" % w: w for w in range(V)},
    }


def _trainer(inp):
    from word2vec_amd.device import Config, DeviceTrainer

    cfg = Config(word_dim=DIM, window=2, negative=2, hs=False, cbow=False, cbow_mean=True, iter=1, init_alpha=0.025,
                 min_alpha=1e-4, table_size=TABLE)
    d = DeviceTrainer(cfg)
    d.upload_vocab(inp["keep"], inp["bounds"])
    d.upload_model(inp["W"], inp["C"])
    return d


def _cycle(inp):
    from word2vec_amd.ingest import GpuIngest
    from word2vec_amd.nn import NearestIndex
    from word2vec_amd.replicas import NativeAverager, group_unique_id

    a = _trainer(inp)
    assert a.row_pitch() == DIM
    a.upload_corpus(inp["ids"], inp["offsets"], N_TOK)
    a.upload_table(inp["table"])
    st_a = a.train_epoch(0)
    # a second handle trains on the first's corpus, and goes on after the owner is gone
    b = _trainer(inp)
    b.share_corpus(a)
    a.close()
    st_b = b.train_epoch(0)  # raises unless W2V_OK
    print(f"words: owner {st_a['words']}, borrower {st_b['words']} of {N_TOK}")
    assert st_b["words"] == N_TOK
    # ingest: count, map, and hand the samples over (b lets go of the shared corpus, its last holder)
    g = GpuIngest(inp["text"], "lines")
    counted = g.count()
    assert sum(c for _, c in counted) == TEXT_BYTES // 8
    g.map(inp["index"])
    b.adopt_corpus(g)
    g.close()
    assert b.n_sent == -(-(TEXT_BYTES // 8) // SENT)  # the last line is shorter and unterminated
    # nearest neighbours on the borrowed W
    with NearestIndex.attach(b, 0) as nn:
        nbr, _ = nn.query_rows(np.arange(4, dtype=np.int32), k=8)
        assert nbr.shape == (4, 8)
    # a one-rank group: the full exchange round trip (P, D, A per matrix)
    grp = NativeAverager([b], unique_id=group_unique_id(), nranks=1)
    grp.average()
    grp.finish()
    assert grp.info()["rounds"] == 1
    grp.close()
    b.close()


def test_life_cycle_returns_device_memory(inputs):
    import torch

    free = []
    for _ in range(CYCLES):
        _cycle(inputs)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    drift = [(f - free[0]) / MIB for f in free]
    print(f"free device memory after each cycle, MiB relative to the first: {drift}")
    for k in range(1, CYCLES):
        assert free[k] >= free[0] - 16 * MIB, f"cycle {k + 1}: {-drift[k]:.1f} MiB fewer free than after cycle 1"
