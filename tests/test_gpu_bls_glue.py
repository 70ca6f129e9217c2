"""The DuckDB glue of the bounded least squares aggregates (duckdb_shim/bls_family_hip.cpp) on the MI355X through its test
driver (tests/tools/bls_family_capi.cpp): bls_fit_agg / nnls_fit_agg / bls_fit_predict_agg as a threaded GROUP BY with
Combine against the restatement; the reference's test_bls_nnls_pivot.test; the twenty cases of
test/sql/fit_predict_agg/test_bls_fit_predict_agg.test restated with its tables and expected values (list lengths, the 7 / 3 and
10 / 0 splits, IS NULL, counts of non-NULL yhat, lower <= yhat <= upper, a wider interval at 0.99 than at 0.90, the collinear
tables asserting what the reference asserts: the list length); the unsigned-df quirk."""
import ctypes as C

import numpy as np
import pytest

import bls_restate as br
from conftest import import_pkg
from test_bls_cpu import glue_lib

pytestmark = pytest.mark.gpu
U8P, DP = C.POINTER(C.c_uint8), C.POINTER(C.c_double)


def _u8(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint8).ctypes.data_as(U8P)


def _fit_agg(fn, spec, key, n_keys, y, X, y_null=None, xe_null=None, threads=4, vec=64):
    lib = glue_lib()
    msg = C.create_string_buffer(512)
    q = lib.blsf_open(fn.encode(), None if spec is None else spec.encode(), 1 if spec else 0, msg)
    assert q, msg.value.decode()
    n, p = X.shape
    y, X, key = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(key, dtype=np.uint32)
    out = np.empty((n_keys, 3 * p + 6))
    is_null = np.zeros(n_keys, dtype=np.uint8)
    rc = lib.blsf_group_by(C.c_void_p(q), C.c_size_t(n), C.c_size_t(p), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(n_keys),
                           y.ctypes.data_as(DP), X.ctypes.data_as(DP), _u8(y_null), None, _u8(xe_null), threads, C.c_size_t(vec),
                           out.ctypes.data_as(DP), is_null.ctypes.data_as(U8P), msg)
    lib.blsf_close(C.c_void_p(q))
    assert rc == 0, msg.value.decode()
    return out, is_null.astype(bool)


def _predict_agg(spec, key, n_keys, y, X, y_null=None, xe_null=None, split=None, threads=3, vec=64):
    lib = glue_lib()
    lib.blsp_group_by.restype = C.c_int64
    msg = C.create_string_buffer(512)
    q = lib.blsp_open(b"bls_fit_predict_agg", None if spec is None else spec.encode(), 0, 1 if split is not None else 0, msg)
    assert q, msg.value.decode()
    n, p = X.shape
    y, X, key = np.ascontiguousarray(y, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(key, dtype=np.uint32)
    off = np.zeros(n_keys + 1, dtype=np.int64)
    vals, flags, is_null = np.empty((n, 4)), np.zeros(n, dtype=np.uint8), np.zeros(n_keys, dtype=np.uint8)
    rows = lib.blsp_group_by(C.c_void_p(q), C.c_size_t(n), C.c_size_t(p), key.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_size_t(n_keys),
                             y.ctypes.data_as(DP), X.ctypes.data_as(DP), _u8(y_null), None, _u8(xe_null), _u8(split), threads, C.c_size_t(vec),
                             off.ctypes.data_as(C.POINTER(C.c_int64)), vals.ctypes.data_as(DP), flags.ctypes.data_as(U8P),
                             is_null.ctypes.data_as(U8P), msg)
    lib.blsp_close(C.c_void_p(q))
    assert rows >= 0, msg.value.decode()
    return off, vals[:rows], flags[:rows], is_null.astype(bool)


def _shuffled(groups, seed):
    rng = np.random.default_rng(seed)
    key = np.concatenate([np.full(len(y), g) for g, (y, _) in enumerate(groups)])
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0)
    perm = rng.permutation(len(y))
    return key[perm], y[perm], X[perm]


@pytest.mark.parametrize("p", [3, 12])
def test_fit_aggregates_group_by_with_combine(p):
    rng = np.random.default_rng(500 + p)
    groups = [br.make_case(rng, 3 * p + 25 + g, p) for g in range(9)]
    key, y, X = _shuffled(groups, p)
    for fn, spec, kw in (("bls_fit_agg", "lower=-0.5;upper=0.75;fit_intercept=true", dict(fit_intercept=True, lower=-0.5, upper=0.75)),
                         ("anofox_stats_bls_fit_agg", None, {}), ("nnls_fit_agg", "lower=-5", {}),
                         ("anofox_stats_nnls_fit_agg", "fit_intercept=true", dict(fit_intercept=True))):
        out, is_null = _fit_agg(fn, spec, key, len(groups), y, X)
        assert not is_null.any()
        for g, (yg, Xg) in enumerate(groups):
            res = br.fit_bls(yg, Xg, **kw)
            assert br.input_conditions(res, yg, Xg, kw.get("fit_intercept", False)) == []
            br.assert_record_matches(out[g], br.record(res), p, xbar=Xg.mean(axis=0), what=f"{fn} group {g}")


def test_pivot_queries_of_the_reference():
    y, X = br.pivot_table()
    key = np.zeros(12, dtype=np.uint32)
    for fn in ("nnls_fit_agg", "bls_fit_agg"):
        out, is_null = _fit_agg(fn, None, key, 1, y, X, threads=2, vec=5)
        assert not is_null[0] and np.array_equal(np.round(out[0, :3], 3), [7.0, 2.0, 0.5])
    pkg = import_pkg()
    r = pkg.ols_fit_agg(np.zeros(12, dtype=np.int64), y, X, {"intercept": False})
    assert np.array_equal(np.round(r.coefficients[0], 3), [7.0, 2.0, 0.5])


def test_fit_aggregate_nulls():
    rng = np.random.default_rng(8)
    y, X = br.make_case(rng, 40, 3)
    key = np.concatenate([np.zeros(39), [1]]).astype(np.uint32)          # group 1: one row -> NULL
    y_null = np.zeros(40, dtype=np.uint8)
    y_null[:4] = 1                                                       # NULL y rows are skipped
    xe = np.zeros((40, 3), dtype=np.uint8)
    xe[5, 1] = 1                                                         # a NULL list element: the fit's filter drops the row
    out, is_null = _fit_agg("bls_fit_agg", None, key, 2, y, X, y_null=y_null, xe_null=xe)
    assert list(is_null) == [False, True]
    keep = np.ones(39, dtype=bool)
    keep[:4] = False
    keep[5] = False
    res = br.fit_bls(y[:39][keep], X[:39][keep])
    br.assert_record_matches(out[0], br.record(res), 3, what="nulls")


# ---- test/sql/fit_predict_agg/test_bls_fit_predict_agg.test restated: its tables as data, its twenty cases by number ----
def _tbl(lo, hi, y, *cols):
    """A table over i in range(lo, hi): y(i) -> value or None (NULL), cols: i -> feature value.  Returns (y, y_null, X)."""
    i = np.arange(lo, hi, dtype=np.float64)
    yv = [y(v) for v in i]
    y_null = np.array([v is None for v in yv], dtype=np.uint8)
    return np.array([0.0 if v is None else v for v in yv]), y_null, np.stack([np.array([c(v) for v in i], dtype=np.float64) for c in cols], axis=1)


def _query(table, cols=None, spec=None, limit=None, key=None, n_keys=1):
    y, y_null, X = table
    if cols is not None:
        X = X[:, cols]
    if limit is not None:
        y, y_null, X = y[:limit], y_null[:limit], X[:limit]
    if key is None:
        key = np.zeros(len(y), dtype=np.uint32)
    return _predict_agg(spec, key, n_keys, y, X, y_null=y_null)


TEST_DATA = _tbl(1, 11, lambda i: 2.0 * i + 1.0 if i <= 7 else None, lambda i: i, lambda i: i * 0.5)
TRAIN, YHAT_NULL = 16, 2


def test_reference_cases_01_to_04_and_06_basic_split_intervals():
    off, vals, flags, is_null = _query(TEST_DATA)                         # 1: [x1, x2] (x2 = 0.5 x1): 10 rows
    assert not is_null[0] and off[1] == 10
    assert int(((flags & YHAT_NULL) == 0).sum()) == 10                    # 6: yhat IS NOT NULL on all 10
    off, vals, flags, is_null = _query(TEST_DATA, cols=[0])
    assert not is_null[0] and off[1] == 10
    assert int(((flags & TRAIN) != 0).sum()) == 7 and int(((flags & TRAIN) == 0).sum()) == 3          # 2: 7 / 3
    assert int((((flags & TRAIN) == 0) & ((flags & YHAT_NULL) == 0)).sum()) == 3                      # 3: predictions not NULL
    ok = ((flags & 14) == 0) & (vals[:, 2] <= vals[:, 1]) & (vals[:, 1] <= vals[:, 3])
    assert int(ok.sum()) == 10                                                                        # 4: lower <= yhat <= upper


def test_reference_case_05_group_by():
    grouped = _tbl(1, 11, lambda i: i * 2.0 if i <= 4 or 5 < i <= 9 else None, lambda i: i)
    key = np.array([0] * 5 + [1] * 5, dtype=np.uint32)                   # grp 'A' for i <= 5, else 'B'
    off, vals, flags, is_null = _query(grouped, key=key, n_keys=2)
    assert not is_null.any() and list(np.diff(off)) == [5, 5]


def test_reference_cases_07_and_08_options():
    for spec in ("lower_bound=0.0", "lower_bound=0.0;upper_bound=10.0"):  # 7
        off, vals, flags, is_null = _query(TEST_DATA, cols=[0], spec=spec)
        assert not is_null[0] and off[1] == 10
    width = {}
    for c in ("0.99", "0.90"):                                            # 8: AVG(upper - lower) wider at 0.99
        off, vals, flags, is_null = _query(TEST_DATA, cols=[0], spec="confidence_level=" + c)
        assert not is_null[0] and off[1] == 10 and not (flags & 14).any()
        width[c] = float(np.mean(vals[:, 3] - vals[:, 2]))
    assert width["0.99"] > width["0.90"]


def test_reference_case_09_two_rows():
    off, vals, flags, is_null = _query(TEST_DATA, limit=2)               # n = p = 2, x2 = 0.5 x1, no intercept
    assert not is_null[0] and off[1] == 2


def test_reference_case_10_constant_feature():
    t = _tbl(1, 11, lambda i: 2.0 * i + 1.0 if i <= 7 else None, lambda i: i, lambda i: 5.0)
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and off[1] == 10 and int(((flags & YHAT_NULL) == 0).sum()) == 10


def test_reference_cases_11_and_12_nan_and_infinity_features():
    for bad_i, bad in ((3, np.nan), (4, np.inf)):
        t = _tbl(1, 11, lambda i: 2.0 * i if i <= 7 else None, lambda i: bad if i == bad_i else i)
        off, vals, flags, is_null = _query(t)
        assert not is_null[0] and off[1] == 10
        assert int(((flags & YHAT_NULL) != 0).sum()) == 1                 # (beyond the reference: only that row's yhat is NULL)


def test_reference_cases_13_to_15_all_training_all_prediction_single():
    t = _tbl(1, 11, lambda i: 2.0 * i + 1.0, lambda i: i)                 # 13
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and int(((flags & TRAIN) != 0).sum()) == 10 and int(((flags & TRAIN) == 0).sum()) == 0
    t = _tbl(1, 11, lambda i: None, lambda i: i)                          # 14: IS NULL
    off, vals, flags, is_null = _query(t)
    assert is_null[0] and off[1] == 0
    t = _tbl(1, 5, lambda i: 5.0 if i == 1 else None, lambda i: i)        # 15: IS NULL
    off, vals, flags, is_null = _query(t)
    assert is_null[0] and off[1] == 0


def test_reference_case_16_five_proportional_columns():
    t = _tbl(1, 26, lambda i: i * 1.5 if i <= 20 else None, lambda i: i, lambda i: i * 2, lambda i: i * 3, lambda i: i * 4, lambda i: i * 5)
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and off[1] == 25


def test_reference_cases_17_and_18_perfect_fit_and_outlier():
    t = _tbl(1, 11, lambda i: 3.0 * i + 2.0 if i <= 8 else None, lambda i: i)                       # 17
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and int(((flags & YHAT_NULL) == 0).sum()) == 10
    t = _tbl(1, 11, lambda i: 1000.0 if i == 5 else (2.0 * i if i <= 8 else None), lambda i: i)     # 18
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and int(((flags & YHAT_NULL) == 0).sum()) == 10


def test_reference_cases_19_and_20_collinear_and_larger():
    t = _tbl(1, 11, lambda i: 2.0 * i if i <= 8 else None, lambda i: i, lambda i: i * 2.0)          # 19: LENGTH = 10
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and off[1] == 10
    t = _tbl(1, 101, lambda i: 2.0 * i + 1.0 if i <= 80 else None, lambda i: i, lambda i: i * 0.5)  # 20: LENGTH = 100
    off, vals, flags, is_null = _query(t)
    assert not is_null[0] and off[1] == 100


def test_split_column_and_null_list_element():
    """Beyond the reference's file: the (y, x, split) overload ('train' / 'Training' / 'TRAIN' / 'training' train, 'test' and
    NULL do not), and a group with fewer than two training rows next to a good one."""
    rng = np.random.default_rng(2)
    n = 20
    X = np.stack([np.arange(1.0, n + 1), rng.uniform(0, 5, size=n)], axis=1)
    y = 2.0 * X[:, 0] + 0.5 * X[:, 1] + 0.3 * rng.normal(size=n)
    key = np.zeros(n, dtype=np.uint32)
    split = np.array([1, 2, 4, 6] * 3 + [3, 0] * 4, dtype=np.uint8)
    off, vals, flags, is_null = _predict_agg(None, key, 1, y, X, split=split)
    assert off[1] == n and int(((flags & TRAIN) != 0).sum()) == 12
    key2 = np.concatenate([np.zeros(n - 1), [1]]).astype(np.uint32)
    off, vals, flags, is_null = _predict_agg(None, key2, 2, y, X)
    assert list(is_null) == [False, True] and off[2] == n - 1


def test_fit_predict_rows_against_restatement_and_the_unsigned_df():
    from scipy import stats as sps
    rng = np.random.default_rng(21)
    p = 4
    groups = [br.make_case(rng, 45, p) for _ in range(3)]
    yq, Xq = br.make_case(rng, p, p)
    Xq[:, 1:] = 1.5                      # three constant columns, n = p rows: n - p - 1 wraps with an intercept
    groups.append((yq, Xq))
    key = np.concatenate([np.full(len(g[0]), i) for i, g in enumerate(groups)]).astype(np.uint32)   # (rows in order: outputs align)
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0)
    off, vals, flags, is_null = _predict_agg("fit_intercept=true;lower=-0.5;upper=0.8;confidence=0.9", key, 4, y, X, threads=1)
    assert not is_null.any()
    for g, (yg, Xg) in enumerate(groups):
        res = br.fit_bls(yg, Xg, True, -0.5, 0.8)
        if g < 3:
            assert br.input_conditions(res, yg, Xg, True) == []
        yhat = res["intercept"] + Xg @ np.where(np.isnan(res["coefficients"]), 0.0, res["coefficients"])
        n = res["n_observations"]
        df = (n - p - 1) % (1 << 64)
        sigma = np.sqrt(res["ssr"] / df)
        margin = 0.0 if n <= p + 1 else sps.t.ppf(0.95, n - p - 1) * sigma * np.sqrt(1 + 1 / n)
        v = vals[off[g]:off[g + 1]]
        scale = np.maximum(np.abs(yhat), 1.0)
        assert (np.abs(v[:, 1] - yhat) <= 1e-8 * scale).all()
        assert (np.abs(v[:, 2] - (yhat - margin)) <= 1e-6 * scale).all() and (np.abs(v[:, 3] - (yhat + margin)) <= 1e-6 * scale).all()
        if g == 3:
            assert df > (1 << 62) and (v[:, 2] == v[:, 1]).all()
