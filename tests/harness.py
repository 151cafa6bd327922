"""Shared setup: run the oracle, mirror its products onto the device C-ABI."""
from __future__ import annotations

import numpy as np

from oracle import Oracle


MODES = {
    "sg_ns": dict(model="sg", train_method="ns", negative=5),
    "sg_hs": dict(model="sg", train_method="hs", negative=0),
    "cbow_ns": dict(model="cbow", train_method="ns", negative=5),
    "cbow_hs": dict(model="cbow", train_method="hs", negative=0),
}

# Hierarchical softmax together with negative sampling: both updates per target
# (Word2Vec.cpp:304-311, :342-349). Kept out of MODES, which parametrises the
# golden-keyed quality tests.
COMBINED_MODES = {
    "sg_hsns": dict(model="sg", train_method="hs", negative=5),
    "cbow_hsns": dict(model="cbow", train_method="hs", negative=5),
}


def mode_config(mode: str, negative=None):
    """The entry of MODES or COMBINED_MODES; `negative` overrides its draw
    count (only for a mode that draws negatives)."""
    m = dict(MODES[mode] if mode in MODES else COMBINED_MODES[mode])
    if negative is not None:
        assert m["negative"] > 0 and negative > 0, (mode, negative)
        m["negative"] = negative
    return m


def oracle_run(sentences, mode: str, dim=32, window=5, iters=1, seed=1234, min_count=2,
               table_size=100_000, subsample=1e-3, cbow_mean=True, init_alpha=0.05, min_alpha=2.5e-6,
               train=True, negative=None):
    m = mode_config(mode, negative)
    o = Oracle(iter=iters, window=window, min_count=min_count, table_size=table_size, word_dim=dim,
               negative=m["negative"], subsample_threshold=subsample, init_alpha=init_alpha,
               min_alpha=min_alpha, cbow_mean=cbow_mean, train_method=m["train_method"], model=m["model"])
    o.load_sentences(sentences)
    o.seed(seed)
    o.build_vocab()
    o.init_weights()  # main.cpp:190 — train() re-inits (Word2Vec.cpp:358)
    if train:
        o.train(record=True)
    return o


def device_config(o: Oracle, mode: str, dim, window, iters, table_size, cbow_mean, init_alpha, min_alpha,
                  negative=None):
    from word2vec_amd.device import Config

    m = mode_config(mode, negative)
    return Config(word_dim=dim, window=window, negative=m["negative"], hs=m["train_method"] == "hs",
                  cbow=m["model"] == "cbow", cbow_mean=cbow_mean, iter=iters, init_alpha=init_alpha,
                  min_alpha=min_alpha, table_size=table_size)


def device_from_oracle(o: Oracle, cfg, initial=True):
    from word2vec_amd.device import DeviceTrainer

    d = DeviceTrainer(cfg)
    keep = o.sample_probs()
    bounds = o.table_bounds() if cfg.negative > 0 else None
    codes = points = off = None
    if cfg.hs:
        codes, points, off = o.huffman()
    d.upload_vocab(keep, bounds, codes, points, off)
    W = o.matrix(0, initial)
    Cm = o.matrix(1, initial) if (cfg.negative > 0 or cfg.cbow) else None
    S = o.matrix(2, initial) if cfg.hs else None
    d.upload_model(W, Cm, S)
    ids, soff = o.samples()
    d.upload_corpus(ids, soff, o.train_words)
    return d


def bound_device_from_oracle(o: Oracle, cfg, pitch=None, extra=64):
    """device_from_oracle(initial=False) on caller-owned matrices, bench.py's
    path: W / C / synapses1 are zero-initialised torch tensors of row pitch
    `pitch` floats (default: the kernels' row width + `extra`), their
    [:rows, :dim] blocks filled from the oracle's current matrices and handed
    to bind_model. Returns (trainer, [W, C, S] tensors or None, pitch)."""
    import torch

    from word2vec_amd.device import DeviceTrainer

    d = DeviceTrainer(cfg)
    codes = points = off = None
    if cfg.hs:
        codes, points, off = o.huffman()
    d.upload_vocab(o.sample_probs(), o.table_bounds() if cfg.negative > 0 else None, codes, points, off)
    if pitch is None:
        pitch = d.row_pitch() + extra
    have = (True, cfg.negative > 0 or cfg.cbow, cfg.hs)
    tens = []
    for k in range(3):
        if not have[k]:
            tens.append(None)
            continue
        m = o.matrix(k)
        t = torch.zeros(m.shape[0], pitch, dtype=torch.float32, device="cuda")
        t[:, :cfg.word_dim] = torch.from_numpy(m).to(t.device)
        tens.append(t)
    torch.cuda.synchronize()  # the handle trains on a stream of its own
    d.bind_model(*[t.data_ptr() if t is not None else None for t in tens], pitch)
    ids, soff = o.samples()
    d.upload_corpus(ids, soff, o.train_words)
    return d, tens, pitch


def rel_err(a, b):
    """Norm-wise: max |a - b| over the whole matrix / max |b| (a matrix-level bound)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    den = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / den)


def elem_rel_err(a, b, floor_frac=1e-3):
    """Per-element: max over elements of |a - b| / max(|b|, floor), floor =
    floor_frac * max |b| (an element far below the matrix's scale, or an exact
    zero, is compared against that floor instead of its own magnitude, since
    its own relative error is dominated by the rounding of the larger terms it
    was summed from)."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    floor = max(np.abs(b).max() * floor_frac, 1e-30)
    return float((np.abs(a - b) / np.maximum(np.abs(b), floor)).max())


def errs(a, b):
    """(norm-wise, per-element) relative error, for messages and logs."""
    return rel_err(a, b), elem_rel_err(a, b)


def check_parity(got, want, init, norm_tol, elem_tol, tag="", ulp_matrices=(), overrides=None):
    """Assert both bounds on every matrix's update (got - init vs want - init):
    norm-wise rel_err < norm_tol AND per-element elem_rel_err < elem_tol; a
    matrix the oracle left untouched must come back bit-identical.
    `overrides` = {matrix index: (norm_tol, elem_tol)} gives a matrix its own
    measured bounds. A matrix listed in `ulp_matrices` — only CBOW-NS's W in a
    single update (test_replay_single_sentence): C starts at zero, so W moves
    by ~1e-6 of its magnitude — may instead meet the fp32 rounding of its
    stored values: max |got - want| <= 2 ulp of max |want| (one rounding of
    `row + g * x` differing in the last bit, from a g that differs in the 7th
    digit, is 1 ulp of the row, which relative to such an update exceeds
    1e-5); when that clause is what passes, it is printed and logged. Each
    measurement is printed and, with W2V_PARITY_LOG=<file>, appended to it as a
    JSON line (the measured errors the bounds in the tests come from)."""
    import json
    import os

    overrides = overrides or {}
    out = []
    for k, (g, w, i) in enumerate(zip(got, want, init)):
        if w is None:
            continue
        dw = np.asarray(w, np.float64) - i
        if np.abs(dw).max() == 0:
            np.testing.assert_array_equal(g, w)
            continue
        en, ee = errs(np.asarray(g, np.float64) - i, dw)
        abs_err = float(np.abs(np.asarray(g, np.float64) - np.asarray(w, np.float64)).max())
        ulps = abs_err / float(np.spacing(np.float32(np.abs(w).max())))
        nt, et = overrides.get(k, (norm_tol, elem_tol))
        by_ulp = en >= nt and k in ulp_matrices and ulps <= 2.0
        out.append((k, en, ee, ulps, nt, et, by_ulp))
        print(f"{tag} matrix {k}: rel_err {en:.2e} elem_rel_err {ee:.2e} max_abs_err {ulps:.2f} ulp"
              + (f" (norm-wise above {nt:g}: passes on the 2-ulp clause)" if by_ulp else ""))
        path = os.environ.get("W2V_PARITY_LOG")
        if path:
            with open(path, "a") as f:
                f.write(json.dumps({"tag": tag, "matrix": k, "rel_err": en, "elem_rel_err": ee, "ulps": ulps,
                                    "norm_tol": nt, "elem_tol": et, "ulp_clause": by_ulp}) + "\n")
    for k, en, ee, ulps, nt, et, by_ulp in out:
        assert en < nt or by_ulp, (tag, k, en, nt, ulps)
        assert ee < et, (tag, k, ee, et)
    return out
