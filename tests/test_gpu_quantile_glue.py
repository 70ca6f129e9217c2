"""Quantile regression through its DuckDB glue (duckdb_shim/quantile_family_hip.cpp, compiled against the stand-in of DuckDB's
headers, driven by tests/tools/quantile_family_capi.cpp) on the GPU: the fit-predict aggregate and the tau path aggregate as a
threaded GROUP BY, the window aggregate under the naive window aggregator and under a segment tree's PRESERVE_INPUT Combine.

Two oracles, neither the code under test, apply to every fitted group or output row:
  * the C ABI called directly (runtime.quantile_fit_predict_batch_host / quantile_fit_predict_path_batch_host) on the rows in
    the order the glue saw them: the glue adds no arithmetic and a group's fit reads only its own rows, so BIT FOR BIT;
  * the numpy restatement (tests/quantile_restate.py::solve): yhat = design . beta within the sweep's 1e-9 max(1, |yhat|).
    X and the noise are Gaussian; tests/test_quantile_glue_cpu.py certifies without a GPU that with the fixed seeds of
    tests/quantile_glue_cases.py every fitted group's optimum is unique, and here no fitted group is left out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, import_pkg

sys.path.insert(0, os.path.dirname(__file__))
import quantile_glue_cases as G  # noqa: E402
import quantile_restate as Q  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_quantile_family_capi.so")
_P = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.qg_open.restype = _P
    lib.qg_open.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.qg_close.argtypes = [_P]
    lib.qg_group_by.restype = C.c_int64
    lib.qg_group_by.argtypes = [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_size_t, C.c_int, C.c_size_t,
                                _P, _P, _P, _P, C.c_char_p]
    lib.qg_window.argtypes = [_P, C.c_size_t, C.c_size_t, _P, _P, _P, _P, _P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _P, _P, _P, C.c_char_p]
    return lib


def _bits_equal(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def _options(tau=0.5, fit_intercept=True, max_iterations=1000, tolerance=1e-6):
    return import_pkg("_abi").AnofoxHipQuantileBatchOptions(tau, fit_intercept, max_iterations, tolerance)


def _group_by(lib, kind, fn, spec, as_map, split, case, fields, per_row=1):
    """-> (entries or -1, offsets, vals [entries, fields], flags, is_null, message)"""
    msg = C.create_string_buffer(512)
    q = lib.qg_open(kind, fn.encode(), None if spec is None else spec.encode(), int(as_map), int(split), 1, msg)
    assert q, msg.value.decode()
    cap = case["n"] * per_row
    offs = np.zeros(case["K"] + 1, dtype=np.int64)
    vals = np.full((cap, fields), np.nan)
    flags = np.zeros(cap, dtype=np.uint8)
    isn = np.zeros(case["K"], dtype=np.uint8)
    entries = lib.qg_group_by(q, case["n"], case["p"], _ptr(case["key"]), case["K"], _ptr(case["y"]), _ptr(case["X"]), _ptr(case["y_null"]), None, None,
                              None, _ptr(case["split"]) if split else None, G.N_THREADS, G.VECTOR_SIZE, 0, cap, _ptr(offs), _ptr(vals), _ptr(flags),
                              _ptr(isn), msg)
    lib.qg_close(q)
    return entries, offs, vals, flags, isn, msg.value.decode()


def _restated_yhat(X_fit, y_fit, X_all, tau, fit_intercept):
    beta, certified = G.restated_fit(X_fit, y_fit, tau, fit_intercept)
    assert certified                                           # a unique optimum: the comparison leaves no group out
    return Q.design(X_all, fit_intercept) @ beta


def _within_sweep_tolerance(got, want):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("restatement: worst |yhat - design.beta| / max(1, |yhat|) = %.3g" % err.max())
    return err.max() <= 1e-9


def _check_aggregate(lib, case, fn, spec, as_map, split, tau, fit_intercept):
    rt = import_pkg("runtime")
    entries, offs, vals, flags, isn, text = _group_by(lib, G.AGG, fn, spec, as_map, split, case, 2)
    assert entries >= 0, text
    train = G.training_mask(case, split)
    groups, order, boff, y_fit, Xb, counts = G.group_batch(case, split)
    core, pred = rt.quantile_fit_predict_batch_host(boff, y_fit, [np.ascontiguousarray(Xb[:, j]) for j in range(case["p"])],
                                                    _options(tau, fit_intercept), train_counts=counts)
    p, fitted = case["p"], 0
    for g in range(case["K"]):
        if g not in groups:
            assert isn[g]                                      # fewer than 2 training rows
            continue
        i = groups.index(g)
        a, b = int(boff[i]), int(boff[i + 1])
        status = G.restated_status(Xb[a:b], y_fit[a:b], tau, fit_intercept, int(counts[i]))
        assert (core[i, p + 5] != 0) == (status != 0)
        if status != 0:
            assert isn[g]                                      # a failed fit
            continue
        assert not isn[g]
        fitted += 1
        idx = order[g]
        oa, ob = int(offs[g]), int(offs[g + 1])
        assert ob - oa == len(idx)
        assert np.array_equal((flags[oa:ob] & 16) != 0, train[idx])
        assert np.array_equal((flags[oa:ob] & 1) != 0, case["y_null"][idx] == 1)
        keep = case["y_null"][idx] == 0
        assert _bits_equal(vals[oa:ob, 0][keep], case["y"][idx][keep])       # y as given, a non-NULL NaN included
        assert not (flags[oa:ob] & 2).any()                    # every x is finite: no NULL yhat
        assert _bits_equal(vals[oa:ob, 1], pred[a:b, 0]), g    # oracle 1: the ABI called directly
        want = _restated_yhat(Xb[a:b], y_fit[a:b], Xb[a:b], tau, fit_intercept)
        assert _within_sweep_tolerance(vals[oa:ob, 1], want), g               # oracle 2: the restatement
    return fitted, (offs, vals, flags, isn)


@pytest.mark.parametrize("fn,spec,as_map,split,tau,fit_intercept", G.AGG_RUNS)
def test_fit_predict_agg_group_by(lib, fn, spec, as_map, split, tau, fit_intercept):
    case = G.group_by_case()
    fitted, (offs, vals, flags, isn) = _check_aggregate(lib, case, fn, spec, as_map, split, tau, fit_intercept)
    assert fitted == case["K"] - 1 and isn[G.ONE_ROW_GROUP]   # one training row -> NULL; every other group is fitted and compared
    # the non-NULL NaN y: the flag stays is_training, y comes back NaN and not NULL, the row does not train (the restatement
    # and the direct call drop it)
    at = int(offs[G.NAN_Y_GROUP]) + list(G.driver_order(case["key"], case["K"])[G.NAN_Y_GROUP]).index(case["nan_row"])
    assert flags[at] & 16 and not flags[at] & 1 and np.isnan(vals[at, 0])


def test_fit_predict_agg_invalid_tau_is_null_not_an_error(lib):
    case = G.group_by_case()
    entries, offs, vals, flags, isn, text = _group_by(lib, G.AGG, G.ALIAS, "tau=1.5", False, False, case, 2)
    assert entries == 0 and isn.all(), text                    # as in the reference: the fit reports tau, every group is NULL


def test_fit_predict_agg_widest_design(lib):
    """p = 32 with an intercept: k = 33, the widest design the kernel is built for."""
    case = G.group_by_case(wide=True)
    fitted, _ = _check_aggregate(lib, case, G.NAME, None, False, False, 0.5, True)
    assert fitted == case["K"]


def test_fit_predict_agg_too_wide_raises_the_library_message(lib):
    rng = np.random.default_rng(7)
    n, p = 80, 33
    case = dict(K=1, p=p, n=n, key=np.zeros(n, dtype=np.uint32), X=np.ascontiguousarray(rng.normal(size=(n, p))), y=rng.normal(size=n),
                y_null=np.zeros(n, dtype=np.uint8), split=None)
    entries, _, _, _, _, text = _group_by(lib, G.AGG, G.ALIAS, None, False, False, case, 2)
    assert entries == -1 and "n_features > 32 is not built" in text, text


@pytest.mark.parametrize("fn,spec,as_map,split,fit_intercept", G.PATH_RUNS)
def test_path_fit_predict_agg_group_by(lib, fn, spec, as_map, split, fit_intercept):
    rt = import_pkg("runtime")
    case = G.group_by_case()
    taus = G.PATH_TAUS
    T, p = len(taus), case["p"]
    entries, offs, vals, flags, isn, text = _group_by(lib, G.PATH, fn, spec, as_map, split, case, 3, per_row=T)
    assert entries >= 0, text
    train = G.training_mask(case, split)
    groups, order, boff, y_fit, Xb, counts = G.group_batch(case, split)
    rec, _, pred = rt.quantile_fit_predict_path_batch_host(boff, y_fit, [np.ascontiguousarray(Xb[:, j]) for j in range(p)],
                                                           _options(0.5, fit_intercept), taus, train_counts=counts)
    fitted = 0
    for g in range(case["K"]):
        if g not in groups:
            assert isn[g]
            continue
        i = groups.index(g)
        a, b = int(boff[i]), int(boff[i + 1])
        assert G.restated_status(Xb[a:b], y_fit[a:b], 0.5, fit_intercept, int(counts[i])) == 0 and not isn[g]
        fitted += 1
        idx = order[g]
        oa, ob = int(offs[g]), int(offs[g + 1])
        assert ob - oa == len(idx) * T
        v = vals[oa:ob].reshape(len(idx), T, 3)                 # row-major: per row in arrival order one entry per tau
        f = flags[oa:ob].reshape(len(idx), T)
        assert np.array_equal((f & 16) != 0, np.repeat(train[idx][:, None], T, axis=1))
        assert np.array_equal((f & 1) != 0, np.repeat((case["y_null"][idx] == 1)[:, None], T, axis=1))
        assert not (f & 2).any() and np.array_equal(v[:, :, 1], np.tile(taus, (len(idx), 1)))        # the caller's order
        assert _bits_equal(v[:, 2, 2], v[:, 3, 2])             # the duplicate tau: identical values
        assert (f[:, 4] & 4).all() and not (f[:, :4] & 4).any()                                       # only the invalid tau is NULL
        assert _bits_equal(v[:, :4, 2], pred[a:b, :4]) and np.isnan(pred[a:b, 4]).all() and rec[i, 4, p + 5] == 1
        for t in range(4):
            want = _restated_yhat(Xb[a:b], y_fit[a:b], Xb[a:b], taus[t], fit_intercept)
            assert _within_sweep_tolerance(v[:, t, 2], want), (g, t)
    assert fitted == case["K"] - 1 and isn[G.ONE_ROW_GROUP]


@pytest.mark.parametrize("fn,spec,tau,fit_intercept", G.WINDOW_RUNS)
def test_fit_predict_window_naive_and_tree(lib, fn, spec, tau, fit_intercept):
    rt = import_pkg("runtime")
    agg = import_pkg("aggregate")
    w = G.window_case()
    n, p, X = w["n"], w["p"], w["X"]
    yv = np.where(w["y_null"] == 1, np.nan, w["y"])
    msg = C.create_string_buffer(512)
    q = lib.qg_open(G.WINDOW, fn.encode(), None if spec is None else spec.encode(), 0, 0, 1, msg)
    assert q, msg.value.decode()
    naive_null = None
    for tree in (False, True):
        frames = G.window_frames(w, tree)
        out = np.full((len(frames), 3), np.nan)
        flags = np.zeros(len(frames), dtype=np.uint8)
        isn = np.zeros(len(frames), dtype=np.uint8)
        rc = lib.qg_window(q, n, p, _ptr(w["y"]), _ptr(X), _ptr(w["y_null"]), None, None, G.WINDOW_PRECEDING, G.TREE_LEAF if tree else 0, G.TREE_BACK,
                           G.VECTOR_SIZE, _ptr(out), _ptr(flags), _ptr(isn), msg)
        assert rc == 0, msg.value.decode()
        # what the glue hands the ABI: per output row the materialised frame plus the current x as a last row that does not train
        fit = [k for k, (lo, hi, _) in enumerate(frames) if int(np.isfinite(yv[lo:hi]).sum()) >= 2]
        ys = np.concatenate([np.append(yv[lo:hi], np.nan) for lo, hi, _ in (frames[k] for k in fit)])
        Xs = np.concatenate([np.vstack([X[lo:hi], X[cur]]) for lo, hi, cur in (frames[k] for k in fit)])
        boff = np.concatenate([[0], np.cumsum([frames[k][1] - frames[k][0] + 1 for k in fit])]).astype(np.int64)
        counts = np.array([int(np.isfinite(yv[frames[k][0]:frames[k][1]]).sum()) for k in fit], dtype=np.int64)
        core, pred = rt.quantile_fit_predict_batch_host(boff, ys, [np.ascontiguousarray(Xs[:, j]) for j in range(p)], _options(tau, fit_intercept),
                                                        train_counts=counts)
        got, want, compared = [], [], 0
        for k, (lo, hi, cur) in enumerate(frames):
            if k not in fit:
                assert isn[k]                                  # fewer than 2 training rows in the frame
                continue
            i = fit.index(k)
            status = G.restated_status(X[lo:hi], yv[lo:hi], tau, fit_intercept, int(counts[i]))
            assert (core[i, p + 5] != 0) == (status != 0)
            if status != 0:
                assert isn[k]                                  # a failed fit: fewer valid rows than p + [intercept]
                continue
            assert not isn[k] and flags[k] == 6                # both bounds are always NULL
            assert _bits_equal(out[k, 0], pred[int(boff[i + 1]) - 1, 0]), k                     # oracle 1
            got.append(out[k, 0])
            want.append(_restated_yhat(X[lo:hi], yv[lo:hi], X[cur:cur + 1], tau, fit_intercept)[0])
            compared += 1
        assert compared > len(frames) // 2
        assert tree or isn[0]                                  # ROWS: the first row's frame has one training row
        assert _within_sweep_tolerance(np.array(got), np.array(want))                           # oracle 2
        if not tree:
            naive_null = isn.copy()
    lib.qg_close(q)
    # the NULL pattern of the Python window function on the same data
    options = None if spec is None else {"tau": tau, "max_iter": 500}
    yhat, lower, upper = agg.quantile_fit_predict(np.zeros(n, dtype=np.int64), np.arange(n), [None if m else float(v) for v, m in zip(w["y"], w["y_null"])],
                                                  [list(r) for r in X], options, frame=(G.WINDOW_PRECEDING, 0))
    assert np.array_equal(np.isnan(yhat), naive_null == 1) and w["y_null"][40] == 1 and not naive_null[40]
    assert np.isnan(lower).all() and np.isnan(upper).all()
