"""The elastic net's fit-predict functions through their DuckDB glue (duckdb_shim/elasticnet_family_hip.cpp, compiled against the
stand-in of DuckDB's headers, driven by tests/tools/elasticnet_family_capi.cpp through family_driver.hpp) on the GPU: the
aggregate as a threaded GROUP BY with Combine, the window aggregate under the naive window aggregator and a segment tree's
Combine — each against the batch entry points on the same rows."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_elasticnet_family_capi.so")
SPLIT_STRINGS = [None, "train", "Training", "test", "TRAIN", "a-validation-partition-name", "training"]   # family_driver.hpp
_P = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.enf_open.restype = _P
    lib.enf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.enf_close.argtypes = [_P]
    lib.enf_group_by.restype = C.c_int64
    lib.enf_group_by.argtypes = [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P, C.c_int, C.c_size_t, _P, _P, _P, _P, C.c_char_p]
    lib.enf_window.argtypes = [_P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, C.c_char_p]
    return lib


def _open(lib, fn, spec=None, as_map=False, split=False):
    msg = C.create_string_buffer(512)
    q = lib.enf_open(fn.encode(), None if spec is None else spec.encode(), int(as_map), int(split), msg)
    assert q, msg.value.decode()
    return q


def _driver_order(key, n_keys, n_threads, vector_size):
    """Output order of a group's rows: thread by thread, within a thread in input order (family_driver.hpp)."""
    n = len(key)
    thread = (np.arange(n) // vector_size) % n_threads
    return [np.concatenate([np.nonzero((key == g) & (thread == t))[0] for t in range(n_threads)]) for g in range(n_keys)]


def _close(got, want, tol=1e-9):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn)
    d = np.abs(np.where(wn, 0.0, got - want)) / np.maximum(np.abs(np.where(wn, 1.0, want)), 1.0)
    assert d.max(initial=0.0) < tol, d.max()


@pytest.mark.parametrize("fn,spec,split,drop_zero,kw", [
    ("anofox_stats_elasticnet_fit_predict_agg", None, False, False, {}),
    ("elasticnet_fit_predict_agg", "alpha=0.2;l1_ratio=0.7", False, False, {"alpha": 0.2, "l1_ratio": 0.7}),
    ("elasticnet_predict_agg", "alpha=0.1", True, False, {"alpha": 0.1}),
    ("anofox_stats_elasticnet_predict_agg", "alpha=0.3;null_policy=drop_y_zero_x;confidence_level=0.9", True, True, {"alpha": 0.3}),
    # the aggregate's bind reads alpha only: lambda is ignored (alpha stays 1)
    ("elasticnet_fit_predict_agg", "lambda=0.05", False, False, {}),
])
def test_fit_predict_agg_group_by(lib, fn, spec, split, drop_zero, kw):
    pkg = import_pkg()
    rng = np.random.default_rng(5)
    K, p, n_threads, vsize = 24, 3, 4, 64
    sizes = rng.integers(10, 40, size=K)
    sizes[2] = 1                                                    # < 2 training rows -> NULL
    key = np.repeat(np.arange(K), sizes).astype(np.uint32)
    rng.shuffle(key)
    n = len(key)
    X = rng.normal(size=(n, p))
    X[rng.random(n) < 0.05, 1] = 0.0
    y = X @ [1.0, -0.5, 2.0] + 0.3 * rng.normal(size=n)
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    sp = rng.integers(0, len(SPLIT_STRINGS), size=n).astype(np.uint8) if split else None
    q = _open(lib, fn, spec, False, split)
    offs = np.zeros(K + 1, dtype=np.int64)
    vals = np.full((n, 4), np.nan)
    flags = np.zeros(n, dtype=np.uint8)
    isn = np.zeros(K, dtype=np.uint8)
    msg = C.create_string_buffer(512)
    rows = lib.enf_group_by(q, n, p, _ptr(key), K, _ptr(y), _ptr(X), _ptr(y_null), None, _ptr(sp), n_threads, vsize, _ptr(offs), _ptr(vals),
                            _ptr(flags), _ptr(isn), msg)
    lib.enf_close(q)
    assert rows >= 0, msg.value.decode()
    # expected: per group, in driver order; training = y not NULL [& split says train] [& no zero feature]
    order = _driver_order(key, K, n_threads, vsize)
    train = y_null == 0
    if split:
        train &= np.array([s is not None and s.lower() in ("train", "training") for s in (SPLIT_STRINGS[c] for c in sp)])
    if drop_zero:
        train &= ~np.any(X == 0.0, axis=1)
    conf = 0.9 if spec and "confidence_level" in spec else 0.95
    for g in range(K):
        idx = order[g]
        nt = int(train[idx].sum())
        if nt < 2:
            assert isn[g]
            continue
        off = np.array([0, len(idx)])
        yf = np.where(train[idx], y[idx], np.nan)
        core, pred = pkg.elasticnet_fit_predict_batch_host(off, yf, [X[idx, j].copy() for j in range(p)], pkg.ElasticNetOptions(**kw).batch_options(),
                                                           conf, train_counts=np.array([nt]))
        if core[0, p + 5] != 0:
            assert isn[g]
            continue
        assert not isn[g]
        a, b = offs[g], offs[g + 1]
        assert b - a == len(idx)
        got_y = np.where(flags[a:b] & 1, np.nan, vals[a:b, 0])
        assert np.array_equal(got_y, np.where(y_null[idx] == 1, np.nan, y[idx]), equal_nan=True)
        assert np.array_equal((flags[a:b] & 16) != 0, train[idx])
        _close(vals[a:b, 1:], pred)
    assert isn[2]


@pytest.mark.parametrize("fn,spec,kw", [
    ("anofox_stats_elasticnet_fit_predict", None, {}),
    ("elasticnet_fit_predict", "lambda=0.2;l1_ratio=0.3", {"alpha": 0.2, "l1_ratio": 0.3}),   # the window's bind: lambda used
])
def test_fit_predict_window_naive_and_tree(lib, fn, spec, kw):
    pkg = import_pkg()
    rng = np.random.default_rng(11)
    n, p = 120, 2
    X = rng.normal(size=(n, p))
    y = X @ [0.7, -1.2] + 0.5 + 0.2 * rng.normal(size=n)
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    yv = np.where(y_null == 1, np.nan, y)
    o = pkg.ElasticNetOptions(**kw).batch_options()
    q = _open(lib, fn, spec)
    out = np.full((n, 3), np.nan)
    isn = np.zeros(n, dtype=np.uint8)
    msg = C.create_string_buffer(512)
    preceding = 15
    assert lib.enf_window(q, n, p, _ptr(y), _ptr(X), _ptr(y_null), None, preceding, 0, 0, 64, _ptr(out), _ptr(isn), msg) == 0, msg.value.decode()
    want = pkg.elasticnet_fit_predict_window_host(np.array([0, n]), yv, [X[:, j].copy() for j in range(p)], o, (preceding, 0))
    _close(np.where(isn[:, None] == 1, np.nan, out), want, 1e-8)
    # segment tree: leaves of 8 rows, frames of 3 leaves
    leaf, back = 8, 2
    nl = (n + leaf - 1) // leaf
    tout = np.full((nl, 3), np.nan)
    tisn = np.zeros(nl, dtype=np.uint8)
    assert lib.enf_window(q, n, p, _ptr(y), _ptr(X), _ptr(y_null), None, 0, leaf, back, 64, _ptr(tout), _ptr(tisn), msg) == 0, msg.value.decode()
    lib.enf_close(q)
    lo = np.array([max(0, o_ - back) * leaf for o_ in range(nl)], dtype=np.int64)
    hi = np.array([min(n, (o_ + 1) * leaf) for o_ in range(nl)], dtype=np.int64)
    # the explicit-frames entry point: one output per frame (pad to n rows, read the first nl)
    lo_n = np.concatenate([lo, np.zeros(n - nl, dtype=np.int64)])
    hi_n = np.concatenate([hi, np.zeros(n - nl, dtype=np.int64)])
    ref = pkg.elasticnet_fit_predict_frames_host(yv, [X[:, j].copy() for j in range(p)], lo_n, hi_n, o)[:nl]
    _close(np.where(tisn[:, None] == 1, np.nan, tout), ref, 1e-8)
