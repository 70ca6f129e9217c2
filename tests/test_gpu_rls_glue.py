"""Recursive least squares through its DuckDB glue (duckdb_shim/rls_family_hip.cpp, compiled against the stand-in of DuckDB's
headers, driven by tests/tools/rls_family_capi.cpp through family_driver.hpp) on the GPU: the fit-predict aggregate as a
threaded GROUP BY whose Combine appends each thread's rows after the previous ones, the window aggregate under the naive window
aggregator and under a segment tree's PRESERVE_INPUT Combine of fixed leaf states.  RLS depends on row order, so every value is
compared BIT FOR BIT with the NumPy restatement of fit_rls (tests/rls_restate.py) over the rows in the order the glue saw them."""
import ctypes as C
import os

import sys

import numpy as np
import pytest

from conftest import ROOT, import_pkg

sys.path.insert(0, os.path.dirname(__file__))
import rls_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_rls_family_capi.so")
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


def _bits_equal(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


@pytest.mark.parametrize("fn,spec,split,drop_zero,kw", [
    ("anofox_stats_rls_fit_predict_agg", None, False, False, {}),
    ("rls_fit_predict_agg", "forgetting_factor=0.97;p_diagonal=10", False, False, {"forgetting_factor": 0.97, "initial_p_diagonal": 10.0}),
    ("rls_predict_agg", "forgetting_factor=0.9;null_policy=drop_y_zero_x", True, True, {"forgetting_factor": 0.9}),
    ("anofox_stats_rls_predict_agg", "lambda=0.5", False, False, {}),                       # lambda is ignored
])
def test_fit_predict_agg_group_by(lib, fn, spec, split, drop_zero, kw):
    import_pkg()
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
    order = _driver_order(key, K, n_threads, vsize)              # Combine appends thread t's rows after threads < t
    train = y_null == 0
    if split:
        train &= np.array([s is not None and s.lower() in ("train", "training") for s in (SPLIT_STRINGS[c] for c in sp)])
    if drop_zero:
        train &= ~np.any(X == 0.0, axis=1)
    for g in range(K):
        idx = order[g]
        nt = int(train[idx].sum())
        if nt < 2:
            assert isn[g]
            continue
        rec = R.rls_fit(np.where(train[idx], y[idx], np.nan), X[idx], **kw)
        if rec[p + 5] != 0:
            assert isn[g]
            continue
        assert not isn[g]
        a, b = offs[g], offs[g + 1]
        assert b - a == len(idx)
        assert np.array_equal((flags[a:b] & 16) != 0, train[idx])
        want = np.array([R.predict(rec, X[r]) for r in idx])
        for k in range(1, 4):
            assert _bits_equal(vals[a:b, k], want), (g, k)
    assert isn[2]


@pytest.mark.parametrize("fn,spec,kw", [
    ("anofox_stats_rls_fit_predict", None, {}),
    ("rls_fit_predict", "forgetting_factor=0.95;intercept=false", {"forgetting_factor": 0.95, "fit_intercept": False}),
])
def test_fit_predict_window_naive_and_tree(lib, fn, spec, kw):
    rng = np.random.default_rng(11)
    n, p = 120, 2
    X = rng.normal(size=(n, p))
    y = X @ [0.7, -1.2] + 0.5 + 0.2 * rng.normal(size=n)
    y_null = (rng.random(n) < 0.1).astype(np.uint8)
    yv = np.where(y_null == 1, np.nan, y)
    q = _open(lib, fn, spec)
    out = np.full((n, 3), np.nan)
    isn = np.zeros(n, dtype=np.uint8)
    msg = C.create_string_buffer(512)
    preceding = 15
    assert lib.enf_window(q, n, p, _ptr(y), _ptr(X), _ptr(y_null), None, preceding, 0, 0, 64, _ptr(out), _ptr(isn), msg) == 0, msg.value.decode()
    want = np.array([R.frame_prediction(yv, X, max(0, e - preceding), e + 1, **kw) for e in range(n)])
    got = np.where(isn == 1, np.nan, out[:, 0])
    assert _bits_equal(got, want)
    # segment tree: leaves of 8 rows combined (PRESERVE_INPUT) into frames of 3 leaves: target rows, then each source's
    leaf, back = 8, 2
    nl = (n + leaf - 1) // leaf
    tout = np.full((nl, 3), np.nan)
    tisn = np.zeros(nl, dtype=np.uint8)
    assert lib.enf_window(q, n, p, _ptr(y), _ptr(X), _ptr(y_null), None, 0, leaf, back, 64, _ptr(tout), _ptr(tisn), msg) == 0, msg.value.decode()
    lib.enf_close(q)
    want = np.array([R.frame_prediction(yv, X, max(0, o_ - back) * leaf, min(n, (o_ + 1) * leaf), **kw) for o_ in range(nl)])
    assert _bits_equal(np.where(tisn == 1, np.nan, tout[:, 0]), want)
