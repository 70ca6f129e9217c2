"""Grouped quantile regression on the MI355X: the records of anofox_hip_quantile_fit_batch_host on the golden cases
(tests/golden/quantile/cases.json, scipy's HiGHS), every (p, intercept, tau) as ONE call of groups of different sizes (the
options and the width belong to a call), with the assertions of
tests/test_quantile_cpu.py::check_record:
  unique cases     coefficients within 1e-9 max(1, |b|_inf) of the golden ones (the project's sweep tolerance) and the
                   certificate of tests/quantile_restate.py true;
  every case       loss <= golden loss (1 + 1e-9); the certificate true wherever it exists (k zero residuals, A_Z non-singular;
                   the reference's aliased table x2 = 0.5 x1 has a singular A_Z and is held to the loss alone).
Only cases the golden file marks non-unique (the reference's integer tables) and groups the row rules refuse (n = k = 1:
status 100) go without a coefficient comparison; among the 180 Gaussian cases that is 3, below the 5 % allowed.
Then: group counts, the row and option rules, masking, determinism (also on stale scratch), the iteration bound, fit-predict, the C symbols, the
Python aggregate."""
import ctypes as C

import numpy as np
import pytest

import quantile_restate as qr
from conftest import import_pkg
from test_quantile_cpu import check_record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return qr.load_cases()


def _fit(pkg, groups, tau=0.5, fit_intercept=True, max_iterations=1000):
    off = np.concatenate([[0], np.cumsum([len(y) for y, _ in groups])]).astype(np.int64)
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0)
    o = pkg.QuantileOptions(tau=tau, fit_intercept=fit_intercept, max_iterations=max_iterations)
    return pkg.quantile_fit_batch_host(off, y, [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], o.batch_options())


def test_golden_cases_in_one_call_per_option_set(cases):
    """Options (tau, intercept) and the width p are per call: the cases of one (p, intercept, tau) — groups of 6 different
    sizes, or the integer table — go in ONE call."""
    pkg = import_pkg()
    compared, calls = 0, {}
    for c in cases:
        calls.setdefault((c["X"].shape[1], c["fit_intercept"], c["tau"]), []).append(c)
    for (p, icpt, tau), cs in calls.items():
        rec, its = _fit(pkg, [(c["y"], c["X"]) for c in cs], tau, icpt)
        for g, c in enumerate(cs):
            compared += check_record(c, rec[g], int(its[g]), c["name"])
    gauss = sum(c["name"].startswith("gauss") for c in cases)
    assert compared >= 0.95 * gauss


@pytest.mark.parametrize("G", [1, 65, 257])
def test_group_counts(cases, G):
    pkg = import_pkg()
    pool = [c for c in cases if c["X"].shape[1] == 8 and c["fit_intercept"] and c["tau"] == 0.5]
    cs = [pool[g % len(pool)] for g in range(G)]
    rec, its = _fit(pkg, [(c["y"], c["X"]) for c in cs], 0.5, True)
    for g in list(range(min(G, 6))) + [G - 1]:
        check_record(cs[g], rec[g], int(its[g]), f"G={G} group {g}")
    for g in range(len(pool), G):
        assert rec[g].tobytes() == rec[g % len(pool)].tobytes() and its[g] == its[g % len(pool)]


def test_rules_masking_and_tau(cases):
    pkg = import_pkg()
    c = next(c for c in cases if c["name"] == "gauss p=2 icpt=1 n=64 tau=0.5")
    X, y = c["X"], c["y"]
    Xn = np.vstack([X[:20], [[np.nan, 1.0]], X[20:], [[0.0, np.inf]], [[0.5, 0.5]]])
    yn = np.concatenate([y[:20], [1.0], y[20:], [2.0], [np.nan]])
    groups = [(y, X), (yn, Xn), (np.full(64, np.nan), X), (y[:2], X[:2]), (y[:1], X[:1]), (y[:3], X[:3])]
    rec, its = _fit(pkg, groups, 0.5, True)
    assert list(rec[:, 7]) == [0, 0, 10, 6, 100, 0]
    assert np.max(np.abs(rec[1, :3] - rec[0, :3])) <= 1e-12 * max(1.0, np.abs(rec[0, :3]).max()) and rec[1, 6] == 64   # NaN rows sprinkled in: the same fit
    assert np.isnan(rec[2:5, :7]).all()
    assert rec[5, 5] == 3 and rec[5, 4] <= 1e-12 * np.abs(y[:3]).max()            # n = k interpolates
    for tau in (0.0, 1.0, float("nan")):
        rec, its = _fit(pkg, groups, tau, True)
        assert (rec[:, 7] == 1).all() and np.isnan(rec[:, :7]).all() and (its == 0).all()


def test_more_than_32_features_is_an_error():
    pkg = import_pkg()
    rng = np.random.default_rng(1)
    with pytest.raises(pkg.AnofoxStatsError, match="quantile regression: n_features > 32 is not built"):
        _fit(pkg, [(rng.normal(size=40), rng.normal(size=(40, 33)))])


def test_two_calls_are_bit_identical(cases):
    pkg = import_pkg()
    cs = [c for c in cases if c["X"].shape[1] == 9 and not c["fit_intercept"] and c["tau"] == 0.9] * 8
    a, ia = _fit(pkg, [(c["y"], c["X"]) for c in cs], 0.9, False)
    b, ib = _fit(pkg, [(c["y"], c["X"]) for c in cs], 0.9, False)
    assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()


def test_iteration_bound_returns_the_last_vertex(cases):
    pkg = import_pkg()
    c = next(c for c in cases if c["name"] == "gauss p=2 icpt=1 n=64 tau=0.5")
    rec, its = _fit(pkg, [(c["y"], c["X"])], 0.5, True, max_iterations=1)
    assert its[0] == -1 and rec[0, 7] == 0 and np.isfinite(rec[0, :3]).all()
    assert rec[0, 4] > c["loss"] and rec[0, 5] == 1                               # one row in the basis, a worse loss


def test_fit_predict(cases):
    pkg = import_pkg()
    cs = [c for c in cases if c["X"].shape[1] == 2 and c["fit_intercept"] and c["tau"] == 0.5 and len(c["y"]) >= 63]
    groups = [(c["y"], c["X"]) for c in cs] + [(cs[0]["y"][:6], cs[0]["X"][:6])]
    off = np.concatenate([[0], np.cumsum([len(y) for y, _ in groups])]).astype(np.int64)
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0).copy()
    G = len(groups)
    y_fit = y.copy()
    counts = np.zeros(G, dtype=np.int64)
    for g in range(G):
        n_train = (off[g + 1] - off[g]) - 5 if g < G - 1 else 1                   # the training rows are a prefix
        y_fit[off[g] + n_train:off[g + 1]] = np.nan
        counts[g] = n_train
    X[off[1] - 1, 0] = np.nan                                                      # a prediction row with a NaN feature
    cols = [np.ascontiguousarray(X[:, j]) for j in range(2)]
    o = pkg.QuantileOptions(tau=0.5, fit_intercept=True).batch_options()
    core, pred = pkg.quantile_fit_predict_batch_host(off, y_fit, cols, o, train_counts=counts)
    assert np.isnan(pred[:, 1:]).all()                                             # no interval
    for g in range(G - 1):
        sl = slice(off[g], off[g + 1])
        rec, _ = pkg.quantile_fit_batch_host(np.array([0, counts[g]], dtype=np.int64), y[sl][:counts[g]],
                                             [c[sl][:counts[g]].copy() for c in cols], o)
        assert core[g, 7] == 0 and np.isnan(core[g, 3:6]).all() and core[g, 6] == counts[g]
        assert np.max(np.abs(core[g, :3] - rec[0, :3])) <= 1e-12 * max(1.0, np.abs(rec[0, :3]).max())   # the same vertex, to rounding
        yhat = rec[0, 2] + X[sl] @ rec[0, :2]
        ok = np.isfinite(yhat)
        assert (np.abs(pred[sl, 0][ok] - yhat[ok]) <= 1e-12 * np.maximum(1.0, np.abs(yhat[ok]))).all()
        assert np.isnan(pred[sl, 0][~ok]).all()
    assert np.isnan(pred[off[1] - 1, 0])
    assert core[G - 1, 7] == 100 and np.isnan(pred[off[G - 1]:, 0]).all()         # fewer than 2 training rows: a NULL list


def test_stale_scratch_of_an_earlier_call_changes_nothing(cases):
    """The row scratch lives in the context's workspace and arrives as earlier calls left it.  A fit with prediction rows
    (y NaN) gives the same bytes and pivot counts fresh, after a call of another layout, and after a ridge fit that fills the
    workspace with moments; so does the fit-predict call."""
    pkg = import_pkg()
    c8 = [c for c in cases if c["X"].shape[1] == 8 and c["fit_intercept"] and c["tau"] == 0.5 and len(c["y"]) >= 63]
    groups = []
    for c in c8:
        y = c["y"].copy()
        y[-15:] = np.nan                                                           # prediction rows
        groups.append((y, c["X"]))
    off = np.concatenate([[0], np.cumsum([len(y) for y, _ in groups])]).astype(np.int64)
    y = np.concatenate([g[0] for g in groups])
    cols = [np.ascontiguousarray(np.concatenate([g[1][:, j] for g in groups])) for j in range(8)]
    counts = np.array([len(g[0]) - 15 for g in groups], dtype=np.int64)
    ctx = pkg.Context(0)
    o = pkg.QuantileOptions(tau=0.5).batch_options()
    a, ia = ctx.quantile_fit_batch_host(off, y, cols, o)
    pa = ctx.quantile_fit_predict_batch_host(off, y, cols, o, train_counts=counts)
    # another layout: one long group of other data, all rows valid, whose z and t land in the slots of the rows above
    big = next(c for c in cases if c["name"] == "gauss p=2 icpt=0 n=130 tau=0.9")
    yb, Xb = np.tile(big["y"], 3), np.tile(big["X"], (3, 1))
    ctx.quantile_fit_batch_host(np.array([0, len(yb)], dtype=np.int64), yb, [np.ascontiguousarray(Xb[:, j]) for j in range(2)],
                                pkg.QuantileOptions(tau=0.9, fit_intercept=False).batch_options())
    b, ib = ctx.quantile_fit_batch_host(off, y, cols, o)
    pb = ctx.quantile_fit_predict_batch_host(off, y, cols, o, train_counts=counts)
    ctx.fit_batch_host(off, np.nan_to_num(y), cols, None, pkg.RegressionOptions(alpha=1.0).batch_options("ridge"))
    d, id_ = ctx.quantile_fit_batch_host(off, y, cols, o)
    pd = ctx.quantile_fit_predict_batch_host(off, y, cols, o, train_counts=counts)
    ctx.close()
    assert (a[:, 13] == 0).all() and (ia > 0).all() and (a[:, 12] == counts).all()
    assert a.tobytes() == b.tobytes() == d.tobytes() and ia.tobytes() == ib.tobytes() == id_.tobytes()
    for k in (0, 1):
        assert pa[k].tobytes() == pb[k].tobytes() == pd[k].tobytes()
    assert pa[0][:, :9].tobytes() == a[:, :9].tobytes()                            # fit-predict fits the same vertex


def _data_array(abi, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return abi.AnofoxDataArray(v.ctypes.data_as(C.POINTER(C.c_double)), None, len(v)), v


def test_c_symbols(cases):
    pkg = import_pkg()
    abi = import_pkg("_abi")
    lib = abi.load()
    c = next(c for c in cases if c["name"] == "gauss p=8 icpt=0 n=65 tau=0.9")
    X, y, p = c["X"], c["y"], 8
    ya, _ky = _data_array(abi, y)
    keep = [_data_array(abi, X[:, j]) for j in range(p)]
    xs = (abi.AnofoxDataArray * p)(*[k[0] for k in keep])
    err = abi.AnofoxError()
    out = abi.AnofoxQuantileFitResultCore()
    o = pkg.QuantileOptions(tau=0.9, fit_intercept=False)
    assert lib.anofox_quantile_fit(ya, xs, p, o.ffi_options(), C.byref(out), C.byref(err)), err.text()
    rec, _ = _fit(pkg, [(y, X)], 0.9, False)
    got = np.array([out.coefficients[j] for j in range(p)])
    assert got.tobytes() == rec[0, :p].tobytes()                                   # the one-group batch call
    assert np.isnan(out.intercept) and out.tau == 0.9 and out.n_observations == 65 and out.n_features == p and out.coefficients_len == p
    lib.anofox_free_quantile_result(C.byref(out))
    assert not out.coefficients and out.coefficients_len == 0
    lib.anofox_free_quantile_result(C.byref(out))                                  # twice: nothing left to free
    for tau in (0.0, 1.0, float("nan")):
        fresh = abi.AnofoxQuantileFitResultCore()
        bad = pkg.QuantileOptions(tau=tau).ffi_options()
        assert not lib.anofox_quantile_fit(ya, xs, p, bad, C.byref(fresh), C.byref(err))
        assert err.code == abi.ERROR_INVALID_INPUT and "tau must be in (0, 1)" in err.text() and not fresh.coefficients
    assert not lib.anofox_quantile_fit(ya, xs, p, o.ffi_options(), None, C.byref(err)) and err.code == abi.ERROR_INVALID_INPUT
    ynan, _k = _data_array(abi, np.full(65, np.nan))
    assert not lib.anofox_quantile_fit(ynan, xs, p, o.ffi_options(), C.byref(out), C.byref(err))
    assert err.code == abi.ERROR_NO_VALID_DATA and err.text() == "All rows filtered due to NULL/NaN values"
    r = pkg.quantile_fit(list(y), [list(X[:, j]) for j in range(p)], {"tau": 0.9, "intercept": False})
    assert np.array(r["coefficients"]).tobytes() == rec[0, :p].tobytes() and r["tau"] == 0.9 and r["n_observations"] == 65


def test_python_aggregate_on_the_reference_table():
    """test_data of the reference's SQL test: 10 rows, y NULL on the last 3, x2 = 0.5 x1 (aliased)."""
    pkg = import_pkg()
    y, X = qr.reference_tables()["test_data"]
    keys = np.zeros(10, dtype=np.int64)
    r = pkg.quantile_fit_predict_agg(keys, [None if np.isnan(v) else float(v) for v in y], X.tolist())
    assert list(r.is_null) == [False]
    rows = r.rows(0)
    assert len(rows) == 10 and sum(x["is_training"] for x in rows) == 7 and all(x["yhat"] is not None for x in rows)
    ok = np.isfinite(y)
    golden = next(c for c in qr.load_cases() if c["name"] == "test_data icpt=1 tau=0.5")
    yhat = np.array([x["yhat"] for x in rows])
    r_train = y[ok] - yhat[ok]
    loss = float(np.sum(np.where(r_train >= 0, 0.5 * r_train, -0.5 * r_train)))
    assert loss <= golden["loss"] * (1 + 1e-9)
    for tau in (0.25, 0.75, 0.9):
        assert len(pkg.quantile_fit_predict_agg(keys, [None if np.isnan(v) else float(v) for v in y], X.tolist(), {"tau": tau}).rows(0)) == 10
    two = pkg.quantile_fit_predict_agg(keys[:2], list(y[:2]), X[:2].tolist())      # the reference's TEST 10: two rows -> NULL
    assert list(two.is_null) == [True]
    none = pkg.quantile_fit_predict_agg(keys, [None] * 10, X.tolist())
    assert list(none.is_null) == [True] and none.rows(0) is None
