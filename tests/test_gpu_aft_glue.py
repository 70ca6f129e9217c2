"""GPU tier of the AFT family's DuckDB glue: duckdb_shim/aft_family_hip.cpp driven through tests/tools/aft_family_capi.cpp
(libanofox_aft_family_capi.so) on the REAL library.  One GROUP BY over the groups of two small calls of
tests/aft_predict_cases.py with different feature counts (8 and 1, so one Finalize vector holds both), Update from two
threads (so every group is a Combine of two states), a key whose rows are all NULL, a key no row has, and failed groups: every
field of aft_fit_agg equals the C ABI record of the same rows in the same order, and aft_fit_predict_agg's lists have the
batch entry point's values with the glue's NULL mapping."""
import ctypes as C
import os

import numpy as np
import pytest

import aft_cases as AC
import aft_predict_cases as PC
from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_aft_family_capi.so")
R = AC.R
THREADS, VSIZE, PMAX = 2, 64, 8
_P, _U8, _DP = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.ag_open.restype = _P
    lib.ag_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.ag_close.argtypes = [_P]
    lib.ag_group_by.restype = C.c_int64
    lib.ag_group_by.argtypes = [_P, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, _DP, _DP, _DP, _U8, _U8, _U8, _U8,
                                C.POINTER(C.c_uint32), C.c_int, C.c_size_t, C.c_int, C.c_size_t, C.POINTER(C.c_int64), _DP, _U8, _U8,
                                C.POINTER(C.c_size_t), C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def table():
    """The rows of the query: the groups of a p = 8 call (keys 0 .. 6) and of a p = 1 call (keys 7 .. 13) interleaved, key 14 with
    NULL rows only, key 15 without a row.  NaN time / event / x of the calls become SQL NULLs; every 17th row's x list is NULL."""
    calls = [PC.make_call(R.WEIBULL, 8, True, small=True), PC.make_call(R.WEIBULL, 1, True, small=True)]
    key, time, event, x, x_len, call_of, row_of = [], [], [], [], [], [], []
    for c, call in enumerate(calls):
        o = call["offsets"]
        g = np.repeat(np.arange(len(o) - 1), np.diff(o)) + 7 * c
        key.append(g), time.append(call["time"]), event.append(call["event"])
        xx = np.zeros((len(g), PMAX))
        xx[:, :call["p"]] = call["x"]
        x.append(xx), x_len.append(np.full(len(g), call["p"])), call_of.append(np.full(len(g), c)), row_of.append(np.arange(len(g)))
    key, time, event, x = np.concatenate(key), np.concatenate(time), np.concatenate(event), np.vstack(x)
    x_len, call_of, row_of = np.concatenate(x_len), np.concatenate(call_of), np.concatenate(row_of)
    # interleave the two calls' rows, each call's own order kept
    order = np.argsort(np.concatenate([np.arange(np.sum(call_of == c)) for c in (0, 1)]), kind="stable")
    key, time, event, x, x_len, call_of, row_of = (a[order] for a in (key, time, event, x, x_len, call_of, row_of))
    n_null = 5   # key 14: rows whose time is NULL (the fit aggregate skips them) and whose x list is NULL (both aggregates do)
    key = np.concatenate([key, np.full(n_null, 14)])
    time, event = np.concatenate([time, np.full(n_null, np.nan)]), np.concatenate([event, np.ones(n_null)])
    x, x_len = np.vstack([x, np.ones((n_null, PMAX))]), np.concatenate([x_len, np.full(n_null, 3)])
    call_of, row_of = np.concatenate([call_of, np.full(n_null, -1)]), np.concatenate([row_of, np.full(n_null, -1)])
    x_null = (np.arange(len(key)) % 17 == 0) | (key == 14)
    return dict(calls=calls, key=key.astype(np.uint32), time=time, event=event, x=x, x_len=x_len.astype(np.uint32), call_of=call_of,
                row_of=row_of, x_null=x_null, n_keys=16)


def arrival(t, k, predict):
    """The rows of key k in the order the driver makes them arrive: thread by thread (Combine appends the later thread's state),
    within a thread vector by vector.  The fit aggregate skips a NULL time / event / x list, the other one a NULL x list only."""
    idx = np.arange(len(t["key"]))
    keep = (t["key"] == k) & ~t["x_null"]
    if not predict:
        keep &= ~np.isnan(t["time"]) & ~np.isnan(t["event"])
    rows = idx[keep]
    return np.concatenate([rows[(rows // VSIZE) % THREADS == th] for th in range(THREADS)]) if len(rows) else rows


def group_by(lib, t, fn, spec, capacity_per_row):
    msg = C.create_string_buffer(512)
    q = lib.ag_open(fn.encode(), spec.encode(), 0, 1, msg)
    assert q, msg.value.decode()
    n, K = len(t["key"]), t["n_keys"]
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    time_null, event_null, xe_null = u8(np.isnan(t["time"])), u8(np.isnan(t["event"])), u8(np.isnan(t["x"]))
    x_null = u8(t["x_null"])
    cap = max(n, K * (6 * PMAX + 14)) * capacity_per_row
    vals, flags, is_null = np.zeros(cap), np.zeros(cap, np.uint8), np.zeros(K, np.uint8)
    offs, out_q = np.zeros(K + 1, np.int64), C.c_size_t(0)
    pu8 = lambda a: a.ctypes.data_as(_U8)
    rc = lib.ag_group_by(q, n, PMAX, t["key"].ctypes.data_as(C.POINTER(C.c_uint32)), K, np.nan_to_num(t["time"]).ctypes.data_as(_DP),
                         np.ascontiguousarray(np.nan_to_num(t["x"])).ctypes.data_as(_DP), np.nan_to_num(t["event"]).ctypes.data_as(_DP),
                         pu8(time_null), pu8(x_null), pu8(xe_null), pu8(event_null), t["x_len"].ctypes.data_as(C.POINTER(C.c_uint32)),
                         THREADS, VSIZE, 0, cap, offs.ctypes.data_as(C.POINTER(C.c_int64)), vals.ctypes.data_as(_DP), pu8(flags),
                         pu8(is_null), C.byref(out_q), msg)
    lib.ag_close(q)
    assert rc >= 0, msg.value.decode()
    return rc, vals, flags, is_null, offs, out_q.value


def reference(t, c, predict, opts, popts=None):
    """The batch entry point on the rows of call c's keys, in arrival order: -> (records, inference, pred or None, rows per key)."""
    aft = import_pkg("aft")
    call = t["calls"][c]
    rows = [arrival(t, 7 * c + g, predict) for g in range(7)]
    allr = np.concatenate(rows)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    cols = [np.ascontiguousarray(t["x"][allr, j]) for j in range(call["p"])]
    if predict:
        rec, inf, pred = aft.aft_fit_predict_batch_host(off, t["time"][allr], cols, t["event"][allr], opts, popts, inference=True)
        return rec, inf, pred, rows, off
    rec, inf = aft.aft_fit_batch_host(off, t["time"][allr], cols, t["event"][allr], opts, inference=True)
    return rec, inf, None, rows, off


def same(a, b):
    return np.array_equal(np.asarray(a, float), np.asarray(b, float), equal_nan=True)


def test_aft_fit_agg_equals_the_c_abi_record(lib, table):
    abi = import_pkg("_abi")
    rc, vals, _, is_null, _, q = group_by(lib, table, "aft_fit_agg", "dist=weibull;inference=true;confidence=0.9", 1)
    assert rc == 0 and q == PMAX
    width = q + 12 + 5 * q + 2
    opts = abi.AnofoxHipAftBatchOptions(0, 1, 100, 1e-9, 1, 0.9)
    n_fitted = 0
    for c in (0, 1):
        p = table["calls"][c]["p"]
        rec, inf, _, rows, _ = reference(table, c, False, opts)
        for g in range(7):
            k, v = 7 * c + g, vals[(7 * c + g) * width:(7 * c + g + 1) * width]
            assert len(rows[g]) > 0
            assert bool(is_null[k]) == (rec[g, p + 12] != 0), (k, rec[g, p + 12])
            if is_null[k]:
                continue
            n_fitted += 1
            assert same(v[:p], rec[g, :p]) and np.all(np.isnan(v[p:q]))
            assert same(v[q:q + 6], rec[g, p:p + 6]) and same(v[q + 6:q + 9], rec[g, p + 6:p + 9])
            assert v[q + 9] == p and v[q + 10] == rec[g, p + 10] and v[q + 11] == rec[g, p + 11] == 1.0
            for d in range(5):
                assert same(v[q + 12 + d * q:q + 12 + d * q + p], inf[g, d * p:(d + 1) * p])
            assert same(v[6 * q + 12:6 * q + 14], inf[g, 5 * p:5 * p + 2])
    # the groups that are all censored, the NULL-row key, the key without rows (the other failed groups: by the record's status above)
    assert n_fitted >= 8 and list(is_null[[6, 13, 14, 15]]) == [1] * 4


def test_aft_fit_predict_agg_equals_the_batch_entry(lib, table):
    abi = import_pkg("_abi")
    h = PC.horizon_of(table["calls"][0])
    rc, vals, flags, is_null, offs, _ = group_by(lib, table, "anofox_stats_aft_fit_predict_agg", "quantile=0.25;horizon=%r" % h, 6)
    vals = vals.reshape(-1, 6)
    opts, popts = abi.AnofoxHipAftBatchOptions(0, 1, 100, 1e-9, 1, 0.95), abi.AnofoxHipAftPredictOptions(0.25, h)
    total = 0
    for c in (0, 1):
        rec, _, pred, rows, off = reference(table, c, True, opts, popts)
        p = table["calls"][c]["p"]
        for g in range(7):
            k, r = 7 * c + g, rows[g]
            assert not is_null[k] and offs[k + 1] - offs[k] == len(r)          # list length: every row with an x list
            v, fl = vals[offs[k]:offs[k + 1]], flags[offs[k]:offs[k + 1]]
            t, e = table["time"][r], table["event"][r]
            assert same(np.where(fl & 1, np.nan, v[:, 0]), t) and same(np.where(fl & 2, np.nan, v[:, 1]), e)   # arrival order, NULL where NULL
            assert np.array_equal((fl & 1) != 0, np.isnan(t)) and np.array_equal((fl & 2) != 0, np.isnan(e))
            assert np.array_equal((fl & 64) != 0, ~np.isnan(t) & ~np.isnan(e))                                # is_training
            want = pred[off[g]:off[g + 1]]
            for s in range(4):
                null = (fl & (4 << s)) != 0
                assert np.array_equal(null, ~np.isfinite(want[:, s])) and same(v[~null, 2 + s], want[~null, s])
            if rec[g, p + 12] != 0:
                assert np.all((fl & 60) == 60)                                   # a failed group: the rows, four NULLs each
            total += len(r)
    assert list(is_null[14:16]) == [1, 1] and rc == total and total > 600
