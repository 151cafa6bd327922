"""Nearest-neighbour and analogy queries on the GPU (include/w2v_dev.h, w2v_nn_*).

``NearestIndex`` owns one w2v_nn handle: a matrix on the device (a copy of a
numpy array, or a ``DeviceTrainer``'s resident W / C borrowed in place) and its
row norms. Queries return, per query, the ``k`` rows of highest cosine as
``(ids int32 [nq, k], scores float32 [nq, k])``, ordered by score descending
and then by row id ascending; slots past the number of candidates hold id -1
and score -inf. The scores are computed by the HIP kernels of libw2v_hip.so
(an exact-f32 GEMM on the matrix cores with the top-k fused behind it); there
is no host fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def limits() -> dict:
    """w2v_nn_limits: the largest dim, k and terms a query takes."""
    lib = N.load_dev_lib()
    d, k, t = C.c_int32(), C.c_int32(), C.c_int32()
    N.check(lib, lib.w2v_nn_limits(C.byref(d), C.byref(k), C.byref(t)), "w2v_nn_limits")
    return {"max_dim": d.value, "max_k": k.value, "max_terms": t.value}


def class_limits() -> dict:
    """w2v_nn_class_limits: the most classes and iterations a k-means run takes."""
    lib = N.load_dev_lib()
    k, it = C.c_int32(), C.c_int32()
    N.check(lib, lib.w2v_nn_class_limits(C.byref(k), C.byref(it)), "w2v_nn_class_limits")
    return {"max_classes": k.value, "max_iterations": it.value}


def class_times() -> dict:
    """w2v_nn_class_times: device ms of the update and assign steps of this thread's last classes() run."""
    lib = N.load_dev_lib()
    u, a = C.c_double(), C.c_double()
    N.check(lib, lib.w2v_nn_class_times(C.byref(u), C.byref(a)), "w2v_nn_class_times")
    return {"update_ms": u.value, "assign_ms": a.value}


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class NearestIndex:
    """Owns one w2v_nn handle (one GPU). Build it with from_matrix or attach."""

    def __init__(self, handle, lib, n_rows: int, dim: int, owner=None):
        self.x = handle
        self.lib = lib
        self.n_rows = int(n_rows)
        self.dim = int(dim)
        self._owner = owner  # keeps an attached trainer alive as long as the index

    @classmethod
    def from_matrix(cls, rows, device: int = -1) -> "NearestIndex":
        """Copy `rows` (n_rows x dim) to the device (-1 = the current one)."""
        lib = N.load_dev_lib()
        m = np.ascontiguousarray(rows, dtype=np.float32)
        if m.ndim != 2:
            raise ValueError(f"from_matrix: expected a 2-d array, got shape {m.shape}")
        x = C.c_void_p()
        N.check(lib, lib.w2v_nn_create(int(device), _ptr(m), m.shape[0], m.shape[1], C.byref(x)), "w2v_nn_create")
        return cls(x, lib, m.shape[0], m.shape[1])

    @classmethod
    def attach(cls, trainer, which: int = 0) -> "NearestIndex":
        """Borrow a DeviceTrainer's resident W (which 0) or C (1): no copy. Close the index before the trainer."""
        lib = N.load_dev_lib()
        x = C.c_void_p()
        N.check(lib, lib.w2v_nn_attach(trainer.h, int(which), C.byref(x)), "w2v_nn_attach")
        return cls(x, lib, trainer.V, trainer.cfg.word_dim, owner=trainer)

    # -- lifecycle -----------------------------------------------------------
    def close(self):
        if getattr(self, "x", None):
            self.lib.w2v_nn_destroy(self.x)
            self.x = None
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc, what):
        N.check(self.lib, rc, what)

    # -- settings ------------------------------------------------------------
    def refresh(self):
        """Recompute the row norms after training moved an attached matrix."""
        self._chk(self.lib.w2v_nn_refresh(self.x), "w2v_nn_refresh")

    def set_strip_rows(self, rows: int):
        """Candidate rows per strip: 0 = automatic, otherwise a multiple of 16 (the answer does not depend on it)."""
        self._chk(self.lib.w2v_nn_set_strip_rows(self.x, int(rows)), "w2v_nn_set_strip_rows")

    def plan(self) -> dict:
        """How the last query was cut: strips, queries per workgroup, rows per strip."""
        s, qb, sr = C.c_int64(), C.c_int32(), C.c_int64()
        self._chk(self.lib.w2v_nn_plan(self.x, C.byref(s), C.byref(qb), C.byref(sr)), "w2v_nn_plan")
        return {"strips": s.value, "query_block": qb.value, "strip_rows": sr.value}

    # -- queries -------------------------------------------------------------
    def query_vectors(self, q, k: int = 10, exclude=None, restrict: int = 0):
        """The k nearest rows of each vector of q (nq x dim, any length). exclude: nq x n_excl row ids a query
        must not return (-1 = none). restrict: candidates are rows [0, restrict) (0 = all)."""
        qa = np.ascontiguousarray(q, dtype=np.float32)
        if qa.ndim == 1:
            qa = qa[None, :]
        if qa.ndim != 2 or qa.shape[1] != self.dim:
            raise ValueError(f"query_vectors: expected (nq, {self.dim}), got {qa.shape}")
        nq = qa.shape[0]
        ex, n_excl = None, 0
        if exclude is not None:
            ex = np.ascontiguousarray(exclude, dtype=np.int32).reshape(nq, -1)
            n_excl = ex.shape[1]
        ids = np.empty((nq, max(int(k), 0)), np.int32)
        sc = np.empty((nq, max(int(k), 0)), np.float32)
        self._chk(self.lib.w2v_nn_query_vectors(self.x, _ptr(qa), nq, _ptr(ex), n_excl, int(restrict), int(k),
                                                _ptr(ids), _ptr(sc)), "w2v_nn_query_vectors")
        return ids, sc

    def query_rows(self, ids, weights=None, k: int = 10, restrict: int = 0):
        """Queries built from the index's own rows: q = sum_t weights[t] * unit(row[ids[t]]), ids nq x terms
        (-1 = unused), weights alike (default: all 1). A query never returns its own term ids. The analogy
        a : b :: c : ? is ids (b, a, c) with weights (1, -1, 1)."""
        ia = np.ascontiguousarray(ids, dtype=np.int32)
        if ia.ndim == 1:
            ia = ia[:, None]
        if ia.ndim != 2:
            raise ValueError(f"query_rows: expected (nq, terms) ids, got {ia.shape}")
        nq, terms = ia.shape
        if weights is None:
            wa = np.ones((nq, terms), np.float32)
        else:
            wa = np.ascontiguousarray(np.broadcast_to(np.asarray(weights, np.float32), (nq, terms)))
        out = np.empty((nq, max(int(k), 0)), np.int32)
        sc = np.empty((nq, max(int(k), 0)), np.float32)
        self._chk(self.lib.w2v_nn_query_rows(self.x, _ptr(ia), _ptr(wa), terms, nq, int(restrict), int(k),
                                             _ptr(out), _ptr(sc)), "w2v_nn_query_rows")
        return out, sc

    # -- word classes (spherical k-means over the rows; include/w2v_dev.h) ----
    def assign(self, centroids):
        """One assignment step: (classes int32 [n_rows], scores float32 [n_rows]) of the rows against the
        centroids (n_classes x dim, any length; a zero or non-finite centroid takes no rows). Highest cosine,
        equal scores to the lowest class; -1 / -inf for a non-finite row or when no centroid is valid."""
        ca = np.ascontiguousarray(centroids, dtype=np.float32)
        if ca.ndim != 2 or ca.shape[1] != self.dim:
            raise ValueError(f"assign: expected (n_classes, {self.dim}) centroids, got {ca.shape}")
        cls = np.empty(self.n_rows, np.int32)
        sc = np.empty(self.n_rows, np.float32)
        self._chk(self.lib.w2v_nn_assign(self.x, _ptr(ca), ca.shape[0], _ptr(cls), _ptr(sc)), "w2v_nn_assign")
        return cls, sc

    def centroids(self, classes, n_classes: int):
        """One update step: (unit centroids float32 [n_classes, dim], counts int64 [n_classes]) of the classes
        (n_rows ids in [-1, n_classes); -1 and non-finite rows are members of nothing; a class without members
        gets a zero row)."""
        ca = np.ascontiguousarray(classes, dtype=np.int32)
        if ca.shape != (self.n_rows,):
            raise ValueError(f"centroids: expected {self.n_rows} classes, got shape {ca.shape}")
        cen = np.empty((max(int(n_classes), 0), self.dim), np.float32)
        cnt = np.empty(max(int(n_classes), 0), np.int64)
        self._chk(self.lib.w2v_nn_centroids(self.x, _ptr(ca), int(n_classes), _ptr(cen), _ptr(cnt)), "w2v_nn_centroids")
        return cen, cnt

    def classes(self, n_classes: int, iterations: int = 10) -> dict:
        """word2vec's -classes: k-means from class[r] = r mod n_classes, update then assign, `iterations` times or
        until an iteration moves no row. Keys: classes, scores, centroids (those the classes were scored
        against), counts (of the final classes), moved (rows moved per iteration run), iterations (run)."""
        k, n_it = max(int(n_classes), 0), max(int(iterations), 0)
        cls = np.empty(self.n_rows, np.int32)
        sc = np.empty(self.n_rows, np.float32)
        cen = np.empty((k, self.dim), np.float32)
        cnt = np.empty(k, np.int64)
        moved = np.zeros(n_it, np.int64)
        run = C.c_int32()
        self._chk(self.lib.w2v_nn_classes(self.x, int(n_classes), int(iterations), _ptr(cls), _ptr(sc), _ptr(cen),
                                          _ptr(cnt), _ptr(moved), C.byref(run)), "w2v_nn_classes")
        return {"classes": cls, "scores": sc, "centroids": cen, "counts": cnt, "moved": moved[:run.value],
                "iterations": run.value}
