"""GPU tier of the mixed-model family's DuckDB glue (duckdb_shim/glmm_family_hip.cpp through tests/tools/glmm_family_capi.cpp on
the real library): one GROUP BY with two Update threads (every key is a Combine), dictionary vectors, keys with different feature
counts, a key with only NULL rows, VARCHAR and BIGINT group columns.  Every field of glmm_fit_agg equals the C ABI record of the
same rows in arrival order, and glmm_fit_predict_agg's lists equal the batch entry point's values with the glue's NULL mapping."""
import importlib

import numpy as np
import pytest

import glmm_glue_driver as D

pytestmark = pytest.mark.gpu
VS, THREADS, K = 64, 2, 6


@pytest.fixture(scope="module")
def lib():
    return D.load()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("anofox-statistics_amd")


def data():
    rng = np.random.default_rng(17)
    n, p = 900, 3
    key = rng.integers(0, K - 2, n)
    key[:60] = K - 2                       # a key with two features
    key[60:75] = K - 1                     # a key whose rows are all NULL somewhere
    group = rng.integers(0, 9, n) + 10 * key
    X = rng.normal(size=(n, p))
    b = rng.normal(size=200)[group]
    y = 1.0 + X @ np.array([0.5, -0.3, 0.2]) + b + 0.5 * rng.normal(size=n)
    x_len = np.where(key == K - 2, 2, 3)
    y[key == K - 2] -= 0.2 * X[key == K - 2, 2]   # (the third column does not reach that key)
    y_null, x_null, g_null = rng.random(n) < 0.08, rng.random(n) < 0.05, rng.random(n) < 0.05
    x_null[60:75] = True
    train = rng.random(n) < 0.8
    return dict(n=n, p=p, key=key, group=group, X=X, y=y, x_len=x_len, y_null=y_null, x_null=x_null, g_null=g_null, train=train)


def arrival(d, k):
    """the rows of key k in the order the driver's two threads and its Combine deliver them"""
    rows = np.arange(d["n"])
    thread = (rows // VS) % THREADS
    return np.concatenate([rows[(thread == t) & (d["key"] == k)] for t in range(THREADS)])


@pytest.mark.parametrize("kind", [D.VARCHAR, D.BIGINT])
def test_fit_agg_equals_the_c_abi_on_the_arrival_order(lib, pkg, kind):
    d = data()
    q, msg = D.open_query(lib, "glmm_fit_agg", "compute_inference=true;reml=false", group_kind=kind)
    assert q, msg
    out = D.group_by(lib, q, d["key"], K, d["y"], d["X"], d["group"], d["y_null"], d["x_null"], d["g_null"], x_len=d["x_len"], threads=THREADS, vector_size=VS)
    lib.ag_close(q)
    assert list(out["is_null"]) == [False] * (K - 1) + [True] and out["q"] == 3
    for k in range(K - 1):
        rows = arrival(d, k)
        rows = rows[~(d["y_null"] | d["x_null"] | d["g_null"])[rows]]
        pk = 2 if k == K - 2 else 3
        ref = pkg.glmm_fit_agg(None, d["y"][rows], [d["X"][rows, j] for j in range(pk)], [int(g) for g in d["group"][rows]],
                               {"compute_inference": True, "reml": False})
        rec, inf = ref.records[0], ref.inference[0]
        c, qw = out["vals"][k], out["q"]
        assert rec[pk + 12] == 0
        assert np.array_equal(c[:pk], rec[:pk]) and np.array_equal(c[qw:qw + 8], rec[pk:pk + 8], equal_nan=True)
        assert list(c[qw + 8:qw + 13]) == [rec[pk + 8], rec[pk + 9], pk, rec[pk + 10], rec[pk + 11]]
        assert c[qw + 13] == rec[pk + 1] and list(c[qw + 14:qw + 17]) == [1, 1, 0]     # random_cov = [var_group], random_dim, no factors
        for j in range(5):
            assert np.array_equal(c[qw + 17 + j * qw:qw + 17 + j * qw + pk], inf[j * pk:(j + 1) * pk])
        assert c[6 * qw + 17] == inf[5 * pk]
        ranef = out["ranef"][out["r_offsets"][k]:out["r_offsets"][k + 1]]
        want = ref.ranef(0)
        assert [int(v) for v in ranef[:, 0]] == [e["group"] for e in want]            # first-seen order, rendered and read back
        assert np.array_equal(ranef[:, 1], [e["intercept"] for e in want]) and np.all(np.isnan(ranef[:, 2]))
        assert [int(v) for v in ranef[:, 3]] == [e["n"] for e in want]


@pytest.mark.parametrize("kind, split", [(D.VARCHAR, False), (D.BIGINT, True)])
def test_fit_predict_agg_equals_the_batch_entry(lib, pkg, kind, split):
    d = data()
    q, msg = D.open_query(lib, "anofox_stats_glmm_fit_predict_agg", "interval=prediction;level=0.9" if split else None, group_kind=kind, split=split)
    assert q, msg
    out = D.group_by(lib, q, d["key"], K, d["y"], d["X"], d["group"], d["y_null"], d["x_null"], d["g_null"], split_train=d["train"] if split else None,
                     x_len=d["x_len"], threads=THREADS, vector_size=VS)
    lib.ag_close(q)
    assert list(out["is_null"]) == [False] * (K - 1) + [True]
    for k in range(K - 1):
        rows = arrival(d, k)
        rows = rows[~(d["x_null"] | d["g_null"])[rows]]
        pk = 2 if k == K - 2 else 3
        trains = ~d["y_null"][rows] & (d["train"][rows] if split else True)
        y = np.where(trains, d["y"][rows], np.nan)
        ref = pkg.glmm_fit_predict_agg(None, y, [d["X"][rows, j] for j in range(pk)], [int(g) for g in d["group"][rows]],
                                       {"interval": "prediction", "level": 0.9} if split else None)
        assert ref.records[0][pk + 12] == 0
        got, flags = out["vals"][out["offsets"][k]:out["offsets"][k + 1]], out["flags"][out["offsets"][k]:out["offsets"][k + 1]]
        assert len(got) == len(rows)
        assert np.array_equal((flags & 64) != 0, trains) and np.array_equal((flags & 1) != 0, d["y_null"][rows])
        assert np.array_equal(got[:, 0][~d["y_null"][rows]], d["y"][rows][~d["y_null"][rows]])
        assert np.array_equal(got[:, 1], ref.yhat) and np.array_equal(got[:, 2], ref.yhat_fixed) and not np.any(flags & 6)
        if split:
            assert np.array_equal(got[:, 3], ref.lower) and np.array_equal(got[:, 4], ref.upper) and not np.any(flags & 24)
        else:
            assert np.all((flags & 24) == 24)   # without interval: NULL
