"""Elastic net fit-predict on the MI355X: anofox_hip_elasticnet_fit_predict_{batch,window,frames}_*.

The fit-predict batch is checked row by row against the elastic net batch record of its group followed by the simplified
interval of anofox_predict_with_interval; the window functions against the same batch fit of every frame materialised as
a group; the in-register window kernels (p <= 8) against the frames path, ridge (l1_ratio = 0) and OLS (alpha = 0)."""
import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

UNB = None


def _data(n_part, n, p, seed, nan_y=0.1):
    rng = np.random.default_rng(seed)
    rows = [n + int(k) for k in rng.integers(0, 5, size=n_part)]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    N = int(off[-1])
    X = rng.normal(size=(N, p)) + 0.01 * np.arange(N)[:, None] / N
    beta = rng.normal(size=p)
    y = X @ beta + 0.3 + 0.5 * rng.normal(size=N)
    y[rng.random(N) < nan_y] = np.nan
    return off, y, X


def _cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def _opts(pkg, **kw):
    return pkg.ElasticNetOptions(**kw).batch_options()


def _predict_rows(pkg, rec, Xrows, p, icpt, conf):
    """anofox_predict_with_interval's simplified interval for every row of x given one p + 6 record."""
    out = np.full((len(Xrows), 3), np.nan)
    if rec[p + 5] != 0:
        return out
    coef = rec[:p]
    b0 = rec[p] if icpt else 0.0
    c = np.where(np.isnan(coef), 0.0, coef)
    xs = np.where(np.isnan(coef)[None, :], 0.0, Xrows)
    v = b0 + xs @ c
    rse, nobs = rec[p + 3], rec[p + 4]
    df = nobs - (p + (1 if icpt else 0))
    margin = np.nan
    if not (np.isnan(rse) or rse <= 0 or nobs <= p + 1) and df > 0:
        margin = pkg.t_critical(conf, int(df)) * rse * np.sqrt(1.0 + 1.0 / nobs)
    for i in range(len(Xrows)):
        if np.isfinite(v[i]):
            out[i] = (v[i], v[i] - margin, v[i] + margin) if np.isfinite(margin) else (v[i], v[i], v[i])
    return out


def _frames_of(off, frame):
    """[lo, hi) of every row's ROWS frame (start, end) in rows PRECEDING (None = UNBOUNDED), clipped to the partition."""
    start, end = frame
    N = int(off[-1])
    lo = np.empty(N, dtype=np.int64)
    hi = np.empty(N, dtype=np.int64)
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        for e in range(a, b):
            f = a if start is None else max(a, e - start)
            l_ = b - 1 if end is None else min(b - 1, e - end)
            if l_ < f:
                lo[e] = hi[e] = e
            else:
                lo[e], hi[e] = f, l_ + 1
    return lo, hi


def _window_reference(pkg, y, X, lo, hi, o, icpt, conf=0.95):
    """Every frame materialised as a group of the elastic net batch fit, predicting the frame's last x; NULL unless MORE
    than p + [intercept] rows with non-NaN y."""
    p = X.shape[1]
    idx = [np.arange(lo[e], hi[e]) for e in range(len(y))]
    goff = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    cat = np.concatenate(idx) if goff[-1] else np.zeros(0, dtype=np.int64)
    core, _ = pkg.elasticnet_fit_batch_host(goff, y[cat], _cols(X[cat]), o)
    out = np.full((len(y), 3), np.nan)
    for e in range(len(y)):
        if hi[e] <= lo[e]:
            continue
        nt = int(np.sum(~np.isnan(y[lo[e]:hi[e]])))
        if nt <= p + (1 if icpt else 0):
            continue
        out[e] = _predict_rows(pkg, core[e], X[hi[e] - 1:hi[e]], p, icpt, conf)[0]
    return out


def _assert_close(got, ref, tol_yhat, tol_bounds, what=""):
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn), f"{what}: NULL pattern differs at rows {np.nonzero((gn != rn).any(axis=1))[0][:10]}"
    m = ~rn
    scale = np.maximum(np.abs(ref), 1.0)
    err = np.where(m, np.abs(got - ref) / scale, 0.0)
    assert err[:, 0].max(initial=0.0) < tol_yhat, f"{what}: yhat error {err[:, 0].max()}"
    assert err[:, 1:].max(initial=0.0) < tol_bounds, f"{what}: bound error {err[:, 1:].max()}"


# ---- fit-predict batch ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", [1, 3, 8, 9, 33, 128])
def test_fit_predict_batch_matches_fit_then_predict(p):
    pkg = import_pkg()
    n = max(40, 2 * p + 20)
    off, y, X = _data(12, n, p, 100 + p)
    X[5, 0] = np.nan                                 # a non-finite feature: no training, NaN prediction
    X[int(off[3]) + 2, p - 1] = np.inf
    # group 6: all rows NaN (status 100); group 7: a constant design (the intercept-only shortcut)
    y[off[6]:off[7]] = np.nan
    X[off[7]:off[8], :] = 2.5
    o = _opts(pkg, alpha=0.2, l1_ratio=0.5)
    # the aggregate's training counts: rows with a non-NULL y (group 6 has none -> status 100)
    counts = np.array([np.sum(~np.isnan(y[off[g]:off[g + 1]])) for g in range(len(off) - 1)], dtype=np.int64)
    core, pred = pkg.elasticnet_fit_predict_batch_host(off, y, _cols(X), o, 0.9, train_counts=counts)
    rcore, _ = pkg.elasticnet_fit_batch_host(off, y, _cols(X), o)
    assert rcore[6, p + 5] == 10                     # without the counts: no valid row
    keep = np.arange(len(off) - 1) != 6
    np.testing.assert_array_equal(core[keep], rcore[keep])
    assert core[6, p + 5] == 100
    assert core[7, p + 5] == 0 and np.all(np.isnan(core[7, :p]))
    for g in range(len(off) - 1):
        a, b = int(off[g]), int(off[g + 1])
        ref = _predict_rows(pkg, core[g], X[a:b], p, True, 0.9)
        _assert_close(pred[a:b], ref, 1e-12, 1e-9, f"group {g}")
    assert np.all(np.isnan(pred[5]))
    # determinism
    core2, pred2 = pkg.elasticnet_fit_predict_batch_host(off, y, _cols(X), o, 0.9, train_counts=counts)
    assert np.array_equal(core, core2, equal_nan=True) and np.array_equal(pred, pred2, equal_nan=True)


def test_fit_predict_batch_statuses_and_train_counts():
    pkg = import_pkg()
    p = 3
    off, y, X = _data(6, 30, p, 7, nan_y=0.0)
    counts = np.diff(off).astype(np.int64)
    counts[2] = 1                                    # the aggregate's "< 2 training rows" -> NULL
    for kw, status in (({"alpha": -1.0}, 4), ({"l1_ratio": 1.5}, 5)):
        core, pred = pkg.elasticnet_fit_predict_batch_host(off, y, _cols(X), _opts(pkg, **kw))
        assert np.all(core[:, p + 5] == status) and np.all(np.isnan(pred))
    Xs = X.copy()
    Xs[off[4]:off[5], :] = 1.0                       # constant design without an intercept: status 6
    core, pred = pkg.elasticnet_fit_predict_batch_host(off, y, _cols(Xs), _opts(pkg, fit_intercept=False), train_counts=counts)
    assert core[2, p + 5] == 100 and np.all(np.isnan(pred[off[2]:off[3]]))
    assert core[4, p + 5] == 6 and np.all(np.isnan(pred[off[4]:off[5]]))
    assert np.all(core[[0, 1, 3, 5], p + 5] == 0)


def test_fit_predict_batch_device_matches_host():
    pkg = import_pkg()
    import torch
    off, y, X = _data(20, 50, 4, 11)
    o = _opts(pkg, alpha=0.1)
    core, pred = pkg.elasticnet_fit_predict_batch_host(off, y, _cols(X), o)
    ctx = pkg.Context(0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dcore, dpred = ctx.elasticnet_fit_predict_batch_device(dev(off), dev(y), [dev(c) for c in _cols(X)], o)
    torch.cuda.synchronize()
    assert np.array_equal(dcore.cpu().numpy(), core, equal_nan=True)
    assert np.array_equal(dpred.cpu().numpy(), pred, equal_nan=True)


# ---- window functions -----------------------------------------------------------------------------------------------

FRAMES = [(UNB, 0), (5, 1), (7, 0), (3, -2), (UNB, -1), (4, UNB)]
TIGHT = dict(tolerance=1e-13, max_iterations=100000)


@pytest.mark.parametrize("p", [1, 3, 8, 9, 33])
@pytest.mark.parametrize("frame", FRAMES)
def test_window_matches_materialised_frames_tight(p, frame):
    pkg = import_pkg()
    n = 3 * p + 14 if p > 8 else 40
    off, y, X = _data(4 if p > 8 else 7, n, p, 31 * p + 3)
    lo, hi = _frames_of(off, frame)
    for icpt, l1, scaling in ((True, 0.5, "raw"), (False, 1.0, "glmnet"), (True, 0.0, "glmnet")):
        if p > 8 and (icpt, l1) != (True, 0.5):
            continue
        o = _opts(pkg, alpha=0.05, l1_ratio=l1, fit_intercept=icpt, lambda_scaling=scaling, **TIGHT)
        got = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), o, frame)
        ref = _window_reference(pkg, y, X, lo, hi, o, icpt)
        _assert_close(got, ref, 1e-8, 1e-6, f"p={p} frame={frame} icpt={icpt} l1={l1} {scaling}")
        # the _window_ output equals the _frames_ output for the bounds the ROWS spec implies
        fr = pkg.elasticnet_fit_predict_frames_host(y, _cols(X), lo, hi, o)
        _assert_close(got, fr, 1e-8, 1e-6, f"frames p={p} frame={frame}")


@pytest.mark.parametrize("p", [1, 3, 8])
@pytest.mark.parametrize("frame", [(UNB, 0), (20, 0)])
def test_window_default_options_within_stopping_bound(p, frame):
    """At the default tolerance the window kernels and the batch path run the same sweeps on moments that differ by
    rounding only, so they stop after the same number of sweeps almost everywhere; where the summation order tips the
    stopping test one way in one path and the other way in the other, the two iterates are one sweep apart.  The stopping
    rule bounds one sweep's change of every coefficient by tol * sqrt(tss / C_jj), so the change of a prediction
    b0 + x'b is at most sum_j |x_j - xbar_j| tol sqrt(tss / C_jj) <= tol * sqrt(tss) * sum_j |x_j - xbar_j| / sqrt(C_jj).
    With |x_j - xbar_j| / sqrt(C_jj) <= 1 per column (x_j's deviation is one term of C_jj) the prediction moves by at most
    p * tol * sqrt(tss); the test allows 4x that, relative to max(|yhat|, 1)."""
    pkg = import_pkg()
    off, y, X = _data(6, 60, p, 900 + p)
    lo, hi = _frames_of(off, frame)
    o = _opts(pkg, alpha=0.05)
    got = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), o, frame)
    ref = _window_reference(pkg, y, X, lo, hi, o, True)
    gn, rn = np.isnan(got), np.isnan(ref)
    assert np.array_equal(gn, rn)
    tss_max = max(np.nansum((y[off[g]:off[g + 1]] - np.nanmean(y[off[g]:off[g + 1]])) ** 2) for g in range(len(off) - 1))
    bound = 4 * p * 1e-6 * np.sqrt(tss_max)
    d = np.where(rn, 0.0, np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))
    assert d[:, 0].max(initial=0.0) < bound, (d[:, 0].max(), bound)


def test_explicit_frames_overlapping_empty_single():
    pkg = import_pkg()
    p = 2
    off, y, X = _data(1, 50, p, 5, nan_y=0.0)
    N = len(y)
    rng = np.random.default_rng(3)
    lo = rng.integers(0, N, size=N).astype(np.int64)
    hi = np.minimum(lo + rng.integers(0, 25, size=N), N).astype(np.int64)
    lo[:3], hi[:3] = 10, 10          # empty
    lo[3:6], hi[3:6] = 7, 8          # single row -> NULL
    o = _opts(pkg, alpha=0.1, **TIGHT)
    got = pkg.elasticnet_fit_predict_frames_host(y, _cols(X), lo, hi, o)
    ref = _window_reference(pkg, y, X, lo, hi, o, True)
    _assert_close(got, ref, 1e-10, 1e-8, "explicit frames")
    assert np.all(np.isnan(got[:6]))


@pytest.mark.parametrize("frame", [(UNB, 0), (12, 0)])
@pytest.mark.parametrize("icpt", [True, False])
def test_window_identities_with_ridge_and_ols(frame, icpt):
    pkg = import_pkg()
    p = 3
    off, y, X = _data(5, 50, p, 77)
    en = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), _opts(pkg, alpha=0.7, l1_ratio=0.0, fit_intercept=icpt, **TIGHT), frame)
    ridge = pkg.fit_predict_window_host(off, y, _cols(X), None,
                                        pkg.RegressionOptions(alpha=0.7, fit_intercept=icpt).batch_options("ridge"), frame)
    _assert_close(en, ridge, 1e-8, 1e-6, "l1_ratio = 0 vs ridge")
    en0 = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), _opts(pkg, alpha=0.0, fit_intercept=icpt, **TIGHT), frame)
    ols = pkg.fit_predict_window_host(off, y, _cols(X), None, pkg.RegressionOptions(fit_intercept=icpt).batch_options("ols"), frame)
    _assert_close(en0, ols, 1e-8, 1e-6, "alpha = 0 vs OLS")


def test_window_near_exact_fits_are_refitted():
    """y exactly linear in x (plus 1e-9 noise) over a stretch of the partition: the moment rss cancels, the kernels flag
    those frames and the frames path sums their rss from the rows, so sigma and the bounds match the materialised fit."""
    pkg = import_pkg()
    p = 2
    rng = np.random.default_rng(21)
    N = 120
    off = np.array([0, N], dtype=np.int64)
    X = rng.normal(size=(N, p))
    y = 1.5 + X @ np.array([2.0, -1.0]) + 1e-9 * rng.normal(size=N)
    y[60:] += 0.5 * rng.normal(size=N - 60)
    ctx = pkg.Context(0)
    o = _opts(pkg, alpha=0.0, **TIGHT)
    for frame in ((UNB, 0), (15, 0)):
        got = ctx.elasticnet_fit_predict_window_host(off, y, _cols(X), o, frame)
        assert ctx.last_window_refit_count() > 0
        lo, hi = _frames_of(off, frame)
        ref = _window_reference(pkg, y, X, lo, hi, o, True)
        _assert_close(got, ref, 1e-8, 1e-6, f"near-exact {frame}")


def test_window_switch_to_frames_path_and_determinism():
    pkg = import_pkg()
    off, y, X = _data(30, 45, 3, 8)
    o = _opts(pkg, alpha=0.1)
    a = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), o, (UNB, 0))
    b = pkg.elasticnet_fit_predict_window_host(off, y, _cols(X), o, (UNB, 0))
    assert np.array_equal(a, b, equal_nan=True)
    import torch
    ctx = pkg.Context(0)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    d = ctx.elasticnet_fit_predict_window_device(dev(off), dev(y), [dev(c) for c in _cols(X)], o, (UNB, 0))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), a, equal_nan=True)


# ---- Python surface --------------------------------------------------------------------------------------------------

def test_python_fit_predict_agg_with_split():
    pkg = import_pkg()
    rng = np.random.default_rng(4)
    n = 90
    keys = np.repeat([1, 2, 3], n // 3)
    X = rng.normal(size=(n, 2))
    y = X @ [1.0, -2.0] + 0.2 * rng.normal(size=n)
    split = ["train" if rng.random() < 0.8 else "test" for _ in range(n)]
    yl = [float(v) for v in y]
    yl[4] = None
    res = pkg.elasticnet_fit_predict_agg(keys, yl, X.tolist(), {"alpha": 0.05, "lambda": 9.0}, split=split)
    # the aggregate reads alpha only; lambda is ignored
    for gi, k in enumerate(res.keys):
        m = keys == k
        tr = np.array([s == "train" for s in split])[m] & ~np.array([v is None for v in yl])[m]
        Xg, yg = X[m], np.where(tr, y[m], np.nan)
        core, _ = pkg.elasticnet_fit_batch_host(np.array([0, m.sum()]), yg, _cols(Xg), _opts(pkg, alpha=0.05))
        ref = _predict_rows(pkg, core[0], Xg, 2, True, 0.95)
        a, b = res.row_offsets[gi], res.row_offsets[gi + 1]
        np.testing.assert_allclose(res.yhat[a:b], ref[:, 0], rtol=1e-12, atol=1e-12)
        assert np.array_equal(res.is_training[a:b], tr)
    win = pkg.elasticnet_fit_predict(keys, np.arange(n), yl, X.tolist(), {"lambda": 0.05})
    off = np.array([0, 30, 60, 90])
    yw = np.array([np.nan if v is None else v for v in yl])
    ref = pkg.elasticnet_fit_predict_window_host(off, yw, _cols(X), _opts(pkg, alpha=0.05), (UNB, 0))
    np.testing.assert_array_equal(np.stack(win, axis=1), ref)
    for name in ("anofox_stats_elasticnet_fit_predict_agg", "elasticnet_fit_predict_agg", "elasticnet_predict_agg",
                 "anofox_stats_elasticnet_predict_agg", "anofox_stats_elasticnet_fit_predict", "elasticnet_fit_predict"):
        assert callable(pkg.SQL_FUNCTIONS[name])
