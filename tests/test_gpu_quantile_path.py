"""The tau path of grouped quantile regression on the MI355X (anofox_hip_quantile_fit_path_batch_*,
anofox_hip_quantile_fit_predict_path_batch_host, anofox_quantile_fit_path and the Python functions over them) on the data sets
of tests/golden/quantile/path_cases.json at the grid 0.05 .. 0.95: every (p, intercept) as ONE call of 67 groups that cycle
through the data sets of that width (more groups than one grid-stride pass of a small grid needs, a ragged tail), each record
under tests/test_quantile_cpu.py::check_record against the fixture entry of its tau.  Then the records against T separate
single-tau calls, the fused prediction, stale scratch, the limits, the scalar function and the aggregate."""
import numpy as np
import pytest

import quantile_restate as qr
from conftest import import_pkg
from test_quantile_cpu import check_record
from test_quantile_path_cpu import load_path_sets

pytestmark = pytest.mark.gpu

G = 67
TAUS, SETS = load_path_sets()
CALLS = {}                                                               # (p, intercept) -> the data sets of that call
for _s in SETS:
    CALLS.setdefault((_s["X"].shape[1], _s["fit_intercept"]), []).append(_s)
CALL_KEYS = sorted(CALLS)


def _layout(groups):
    off = np.concatenate([[0], np.cumsum([len(y) for y, _ in groups])]).astype(np.int64)
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0)
    return off, y, [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def _call_groups(key):
    pool = CALLS[key]
    return [pool[g % len(pool)] for g in range(G)]


@pytest.fixture(scope="module")
def path_calls():
    """The seven-tau fit-predict path of every (p, intercept) call, computed once: key -> (rec[G, T, p+6], its[G, T], pred[N, T])."""
    pkg = import_pkg()
    out = {}
    for key in CALL_KEYS:
        off, y, cols = _layout([(s["y"], s["X"]) for s in _call_groups(key)])
        o = pkg.QuantileOptions(tau=float("nan"), fit_intercept=key[1]).batch_options()      # options.tau is ignored
        out[key] = pkg.quantile_fit_predict_path_batch_host(off, y, cols, o, TAUS)
    return out


@pytest.fixture(scope="module")
def cold_calls():
    """T separate single-tau calls per (p, intercept): key -> (rec[G, T, p+6], its[G, T])."""
    pkg = import_pkg()
    out = {}
    for key in CALL_KEYS:
        off, y, cols = _layout([(s["y"], s["X"]) for s in _call_groups(key)])
        parts = [pkg.quantile_fit_batch_host(off, y, cols, pkg.QuantileOptions(tau=tau, fit_intercept=key[1]).batch_options()) for tau in TAUS]
        out[key] = np.stack([r for r, _ in parts], axis=1), np.stack([i for _, i in parts], axis=1)
    return out


@pytest.mark.parametrize("key", CALL_KEYS, ids=lambda k: f"p={k[0]} icpt={int(k[1])}")
def test_one_call_of_67_groups_meets_check_record(path_calls, key):
    """The p = 5 call is the reference's aliased high_dim table, whose optimum at tau = 0.25 and 0.75 lies behind a degenerate
    vertex (tests/test_quantile_path_cpu.py::test_every_tau_of_the_path_meets_the_single_fit_assertions)."""
    rec, its, _ = path_calls[key]
    sets = _call_groups(key)
    for g in range(len(CALLS[key])):                                     # each data set once against its fixture entries ...
        for t, c in enumerate(sets[g]["cases"]):
            check_record(c, rec[g, t], int(its[g, t]), f"group {g} {c['name']}")
    for g in range(len(CALLS[key]), G):                                  # ... and every later group is the bytes of its first copy
        assert rec[g].tobytes() == rec[g % len(CALLS[key])].tobytes() and its[g].tobytes() == its[g % len(CALLS[key])].tobytes(), g


@pytest.mark.parametrize("key", CALL_KEYS, ids=lambda k: f"p={k[0]} icpt={int(k[1])}")
def test_path_records_against_separate_single_tau_calls(path_calls, cold_calls, key):
    pkg = import_pkg()
    p, icpt = key
    rec, its, pred = path_calls[key]
    cold, cold_its = cold_calls[key]
    sets = _call_groups(key)
    for col in (p + 1, p + 4, p + 5):                                    # tau, n_observations, status: the same bytes
        assert rec[:, :, col].tobytes() == cold[:, :, col].tobytes(), col
    assert rec[:, 0].tobytes() == cold[:, 0].tobytes() and its[:, 0].tobytes() == cold_its[:, 0].tobytes()   # the walk starts cold
    for g in range(len(CALLS[key])):
        ymax = np.max(np.abs(sets[g]["y"]))
        for t, c in enumerate(sets[g]["cases"]):
            lp, lc = rec[g, t, p + 2], cold[g, t, p + 2]
            assert abs(lp - lc) <= 1e-9 * max(lc, 1e-300) + 1e-12 * ymax, f"{c['name']}: loss {lp!r} vs cold {lc!r}"
            if c["unique"]:
                scale = max(1.0, np.max(np.abs(c["b"])))
                assert np.max(np.abs(rec[g, t, :p] - cold[g, t, :p])) <= 1e-9 * scale, c["name"]
                if icpt:
                    assert abs(rec[g, t, p] - cold[g, t, p]) <= 1e-9 * max(scale, abs(c["b0"])), c["name"]
    off, y, cols = _layout([(s["y"], s["X"]) for s in sets])
    o = pkg.QuantileOptions(fit_intercept=icpt).batch_options()
    rec2, its2, pred2 = pkg.quantile_fit_predict_path_batch_host(off, y, cols, o, TAUS)
    assert rec2.tobytes() == rec.tobytes() and its2.tobytes() == its.tobytes() and pred2.tobytes() == pred.tobytes()
    rec3, its3 = pkg.quantile_fit_path_batch_host(off, y, cols, o, TAUS)  # the entry without a prediction: the same fit
    assert rec3.tobytes() == rec.tobytes() and its3.tobytes() == its.tobytes()
    for t, tau in enumerate(TAUS):                                       # a path of one tau is the single-tau entry point
        one, one_its = pkg.quantile_fit_path_batch_host(off, y, cols, o, [tau])
        assert one[:, 0].tobytes() == cold[:, t].tobytes() and one_its[:, 0].tobytes() == cold_its[:, t].tobytes(), tau


def test_pivots_on_the_gpu_are_fewer_than_cold(path_calls, cold_calls):
    path = sum(int(path_calls[k][1][:len(CALLS[k])].sum()) for k in CALL_KEYS)
    cold = sum(int(cold_calls[k][1][:len(CALLS[k])].sum()) for k in CALL_KEYS)
    assert all((path_calls[k][1] >= 0).all() for k in CALL_KEYS)
    print(f"pivots over the fixture: path {path}, cold {cold}")
    assert path < cold


def test_device_entry_order_duplicates_and_invalid_positions(path_calls):
    import torch
    pkg = import_pkg()
    key = (4, True)
    rec, its, pred = path_calls[key]
    off, y, cols = _layout([(s["y"], s["X"]) for s in _call_groups(key)])
    o = pkg.QuantileOptions(fit_intercept=True).batch_options()
    ctx = pkg.Context(0)
    dev = torch.device("cuda:0")
    d_rec, d_its = ctx.quantile_fit_path_batch_device(torch.from_numpy(off).to(dev), torch.from_numpy(y).to(dev),
                                                      [torch.from_numpy(c).to(dev) for c in cols], o, TAUS)
    torch.cuda.synchronize()
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes() and d_its.cpu().numpy().tobytes() == its.tobytes()
    ctx.close()
    mixed = [0.9, float("nan"), 0.05, 0.5, 0.25, 1.0, 0.5, 0.95, 0.1, 0.0, 0.75]              # shuffled, 0.5 twice, three invalid
    rec2, its2, pred2 = pkg.quantile_fit_predict_path_batch_host(off, y, cols, o, mixed)
    for j, tau in enumerate(mixed):
        if not 0.0 < tau < 1.0:
            assert (rec2[:, j, 9] == 1).all() and np.isnan(rec2[:, j, :9]).all() and (its2[:, j] == 0).all() and np.isnan(pred2[:, j]).all()
            continue
        t = TAUS.index(tau)
        assert rec2[:, j].tobytes() == rec[:, t].tobytes() and pred2[:, j].tobytes() == pred[:, t].tobytes(), tau
        assert j == 6 and (its2[:, j] == 0).all() or its2[:, j].tobytes() == its[:, t].tobytes()   # the second 0.5 starts at its optimum


def _ulp_error(pred, A, beta):
    """|pred - A beta| in units of ulp(S), S = sum_j |a_ij beta_j|; A beta in extended precision (its own error < 2^-10 ulp(S))."""
    ref = (A.astype(np.longdouble) * beta.astype(np.longdouble)).sum(axis=1)
    S = np.abs(A) @ np.abs(beta)
    return np.abs(pred.astype(np.longdouble) - ref).astype(np.float64) / np.spacing(np.maximum(S, np.finfo(float).tiny))


@pytest.mark.parametrize("key", CALL_KEYS, ids=lambda k: f"p={k[0]} icpt={int(k[1])}")
def test_fused_prediction_is_the_design_times_the_returned_coefficients(path_calls, key):
    """pred[i, t] against a_i'beta_t recomputed from the returned record, within 4 ulp(S_i), S_i = sum_j |a_ij beta_j|.

    The wavefront evaluates fit = fma(a_ic, beta_c, fit) for c = 0 .. k-1 from fit = 0: k roundings (the first is the rounding
    of the product a_i0 beta_0 — or exact, 1.0 * intercept), i.e. k - 1 additions on top of correctly rounded products.  Every
    partial sum is at most S_i in size, so each rounding errs by at most ulp(S_i) / 2 and the result by k / 2 ulp(S_i): within
    4 ulp for every k <= 8 a priori.  For the wider fixture (k = 33, a priori 16.5 ulp) 4 ulp holds because the partial sums
    stay well below S_i and the errors do not line up; the bound is the same for every width and the largest figure of each
    call is printed.  The reference side is summed in extended precision so that it adds nothing to the figure."""
    p, icpt = key
    rec, _, pred = path_calls[key]
    sets = _call_groups(key)
    off = np.concatenate([[0], np.cumsum([len(s["y"]) for s in sets])])
    worst = 0.0
    for g, s in enumerate(sets):
        A = qr.design(s["X"], icpt)
        for t in range(len(TAUS)):
            assert rec[g, t, p + 5] == 0
            beta = np.concatenate([[rec[g, t, p]], rec[g, t, :p]]) if icpt else rec[g, t, :p]
            worst = max(worst, float(_ulp_error(pred[off[g]:off[g + 1], t], A, beta).max()))
    print(f"p={p} icpt={int(icpt)}: largest |pred - a'beta| = {worst:.3f} ulp(S)")
    assert worst <= 4.0


def test_prediction_rows_bad_rows_and_failed_groups(path_calls):
    pkg = import_pkg()
    s = next(s for s in SETS if s["name"] == "gauss p=8 n=65 icpt=1")
    X, y = s["X"].copy(), s["y"].copy()
    y[50:] = np.nan                                                      # 15 prediction rows
    X[60, 3] = np.inf                                                    # a prediction row with a bad x
    X[7, 0] = np.nan                                                     # a training row the mask drops
    groups = [(y, X), (s["y"][:6], s["X"][:6]), (np.where(np.arange(65) < 1, s["y"], np.nan), s["X"]), (s["y"], s["X"])]
    counts = np.array([49, 6, 1, 65], dtype=np.int64)                    # group 1: 6 rows < k = 9; group 2: one training row
    off, yy, cols = _layout(groups)
    o = pkg.QuantileOptions(fit_intercept=True).batch_options()
    rec, its, pred = pkg.quantile_fit_predict_path_batch_host(off, yy, cols, o, TAUS, train_counts=counts)
    assert (rec[0, :, 13] == 0).all() and (rec[0, :, 12] == 49).all() and (rec[1, :, 13] == 6).all() and (rec[2, :, 13] == 100).all()
    assert np.isnan(rec[1:3, :, :13]).all() and (its[1:3] == 0).all() and np.isnan(pred[off[1]:off[3]]).all()
    bad = np.zeros(65, dtype=bool)
    bad[[7, 60]] = True
    assert np.isnan(pred[:65][bad]).all() and np.isfinite(pred[:65][~bad]).all()              # finite on the rows whose y is NaN
    A = qr.design(np.where(bad[:, None], 0.0, X), True)
    for t in range(len(TAUS)):
        beta = np.concatenate([[rec[0, t, 8]], rec[0, t, :8]])
        assert _ulp_error(pred[:65, t][~bad], A[~bad], beta).max() <= 4.0
    full = path_calls[(8, True)]
    assert rec[3].tobytes() == full[0][0].tobytes() and pred[off[3]:].tobytes() == full[2][:65].tobytes()   # a neighbour's failure changes nothing


def test_stale_scratch_of_an_earlier_call_changes_nothing():
    """As tests/test_gpu_quantile.py's single-tau test: the path with prediction rows gives the same bytes fresh, after a
    single-tau call of another layout, and after a ridge fit that fills the workspace with moments."""
    pkg = import_pkg()
    s = next(s for s in SETS if s["name"] == "gauss p=8 n=65 icpt=1")
    y = s["y"].copy()
    y[-15:] = np.nan
    off, yy, cols = _layout([(y, s["X"])] * 5)
    counts = np.full(5, 50, dtype=np.int64)
    ctx = pkg.Context(0)
    o = pkg.QuantileOptions().batch_options()
    a = ctx.quantile_fit_predict_path_batch_host(off, yy, cols, o, TAUS, train_counts=counts)
    big = next(s for s in SETS if s["name"] == "tied p=2 n=64 icpt=0")
    yb, Xb = np.tile(big["y"], 6), np.tile(big["X"], (6, 1))
    ctx.quantile_fit_batch_host(np.array([0, len(yb)], dtype=np.int64), yb, [np.ascontiguousarray(Xb[:, j]) for j in range(2)],
                                pkg.QuantileOptions(tau=0.9, fit_intercept=False).batch_options())
    b = ctx.quantile_fit_predict_path_batch_host(off, yy, cols, o, TAUS, train_counts=counts)
    ctx.fit_batch_host(off, np.nan_to_num(yy), cols, None, pkg.RegressionOptions(alpha=1.0).batch_options("ridge"))
    c = ctx.quantile_fit_predict_path_batch_host(off, yy, cols, o, TAUS, train_counts=counts)
    ctx.close()
    assert (a[0][:, :, 13] == 0).all() and (a[1] >= 0).all() and (a[0][:, :, 12] == 50).all()
    for k in range(3):
        assert a[k].tobytes() == b[k].tobytes() == c[k].tobytes(), k


def test_limits():
    pkg = import_pkg()
    s = SETS[1]
    off, y, cols = _layout([(s["y"], s["X"])])
    o = pkg.QuantileOptions().batch_options()
    with pytest.raises(pkg.AnofoxStatsError, match="n_taus > 64 is not built"):
        pkg.quantile_fit_path_batch_host(off, y, cols, o, np.linspace(0.01, 0.99, 65))
    rec, _ = pkg.quantile_fit_path_batch_host(off, y, cols, o, np.linspace(0.01, 0.99, 64))
    assert (rec[0, :, -1] == 0).all()
    with pytest.raises(pkg.AnofoxStatsError, match="taus is NULL or empty"):
        pkg.quantile_fit_path_batch_host(off, y, cols, o, [])
    rng = np.random.default_rng(1)
    with pytest.raises(pkg.AnofoxStatsError, match="quantile regression: n_features > 32 is not built"):
        pkg.quantile_fit_path_batch_host(np.array([0, 40], dtype=np.int64), rng.normal(size=40), list(rng.normal(size=(33, 40))), o, TAUS)


def test_scalar_path():
    pkg = import_pkg()
    s = next(s for s in SETS if s["name"] == "gauss p=4 n=40 icpt=0")
    res = pkg.quantile_fit_path(list(s["y"]), [list(s["X"][:, j]) for j in range(4)], {"taus": TAUS, "intercept": False})
    assert isinstance(res, list) and len(res) == len(TAUS)
    for r, c in zip(res, s["cases"]):
        b = np.array(r["coefficients"])
        loss = qr.pinball_loss(s["X"], s["y"], c["tau"], b, None)
        rec = np.concatenate([b, [r["intercept"], r["tau"], loss, 4.0, r["n_observations"], 0.0]])
        check_record(c, rec, 0, c["name"])
        assert r["n_features"] == 4
    with pytest.raises(pkg.InvalidInputException, match=r"tau must be in \(0, 1\)") as e:
        pkg.quantile_fit_path(list(s["y"]), [list(s["X"][:, j]) for j in range(4)], {"taus": [0.5, 1.0]})
    assert e.value.code == import_pkg("_abi").ERROR_INVALID_INPUT


def test_aggregate_on_the_reference_table():
    """test_data of the reference's SQL test (10 rows, y NULL on the last 3, x2 = 0.5 x1) plus a group with one training row."""
    pkg = import_pkg()
    y, X = qr.reference_tables()["test_data"]
    ylist = [None if np.isnan(v) else float(v) for v in y]
    keys = np.concatenate([np.zeros(10, dtype=np.int64), np.ones(3, dtype=np.int64)])
    r = pkg.quantile_path_fit_predict_agg(keys, ylist + [5.0, None, None], X.tolist() + X[:3].tolist(), {"taus": [0.1, 0.5, 0.9]})
    yhat = r.yhat_of(0)
    assert yhat.shape == (10, 3) and np.isfinite(yhat).all() and not r.is_null[0].any() and r.is_training[:10].sum() == 7
    single = pkg.quantile_fit_predict_agg(keys[:10], ylist, X.tolist(), {"tau": 0.5})
    mid = np.array([row["yhat"] for row in single.rows(0)])
    golden = {c["tau"]: c for c in qr.load_cases() if c["name"].startswith("test_data icpt=1")}
    ok = np.isfinite(y)
    for t, tau in enumerate((0.1, 0.5, 0.9)):
        res = y[ok] - yhat[ok, t]
        assert float(np.sum(np.where(res >= 0, tau * res, (tau - 1.0) * res))) <= golden[tau]["loss"] * (1 + 1e-9), tau
    if golden[0.5]["unique"]:
        assert np.max(np.abs(yhat[:, 1] - mid)) <= 1e-9 * max(1.0, np.max(np.abs(mid)))
    assert r.is_null[1].all() and r.yhat_of(1).shape == (3, 3) and np.isnan(r.yhat_of(1)).all()    # one training row: every column NULL
    assert (r.records[1, :, -1] == 100).all()
