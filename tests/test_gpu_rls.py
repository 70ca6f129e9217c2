"""Recursive least squares on the MI355X: anofox_hip_rls_fit_{batch,predict_batch,predict_window,predict_frames}_*.

The contract is the reference's exact operation order, so every record is compared BIT FOR BIT (NaN positions included)
with the NumPy restatement of fit_rls in tests/rls_restate.py: the lane kernels (p <= 8), the wavefront kernel (p > 8 and
long groups), the fit-predict batch, and the window functions over ROWS and explicit frames."""
import os
import sys

import numpy as np
import pytest

from conftest import import_pkg

sys.path.insert(0, os.path.dirname(__file__))
import rls_restate as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_bits(got, want, what=""):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bad = np.nonzero(_bits(got).ravel() != _bits(want).ravel())[0]
    assert len(bad) == 0, f"{what}: {len(bad)} entries differ, first at {bad[0]}: {got.ravel()[bad[0]]!r} vs {want.ravel()[bad[0]]!r}"


def _opts(pkg, **kw):
    return pkg.RlsOptions(**kw).batch_options()


def _groups(rng, sizes, p, const_cols=(), nan_frac=0.0, inf_rows=0):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    X = rng.normal(size=(N, p))
    for j in const_cols:
        X[:, j] = 3.0
    y = X @ rng.normal(size=p) + 0.5 + 0.3 * rng.normal(size=N)
    if nan_frac:
        y[rng.random(N) < nan_frac] = np.nan
    for _ in range(inf_rows):
        X[rng.integers(0, N), rng.integers(0, p)] = np.inf
    return off, y, X


def _cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 33])
@pytest.mark.parametrize("icpt", [True, False])
def test_batch_bit_identical(p, icpt):
    pkg = import_pkg()
    rng = np.random.default_rng(100 + p + 1000 * icpt)
    sizes = [0, 1, 2, 3, 40, 57, 120] + [int(k) for k in rng.integers(p + 2, 60, size=5)]
    off, y, X = _groups(rng, sizes, p, const_cols=(0,) if p > 2 else (), nan_frac=0.05, inf_rows=2)
    kw = dict(forgetting_factor=0.99, initial_p_diagonal=100.0, fit_intercept=icpt)
    core = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw))
    want = R.batch(off, y, _cols(X), **kw)
    _assert_bits(core, want, f"p={p} icpt={icpt}")
    again = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw))
    assert core.tobytes() == again.tobytes()


@pytest.mark.parametrize("p", [64, 128])
def test_batch_wide_bit_identical(p):
    pkg = import_pkg()
    rng = np.random.default_rng(7 + p)
    off, y, X = _groups(rng, [p + 20, 5, 1], p, const_cols=(3,))
    for lam in (1.0, 0.95):
        kw = dict(forgetting_factor=lam, initial_p_diagonal=10.0)
        _assert_bits(pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw)), R.batch(off, y, _cols(X), **kw), f"p={p}")


@pytest.mark.parametrize("lam", [1.0, 0.99, 0.95])
def test_divergent_filter_bit_identical(lam):
    """lambda = 0.99 over 1000 rows: the reference's filter grows to ~1e11 and is chaotic; only its exact order matches."""
    pkg = import_pkg()
    rng = np.random.default_rng(5)
    off, y, X = _groups(rng, [1000, 300], 3)
    kw = dict(forgetting_factor=lam)
    _assert_bits(pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw)), R.batch(off, y, _cols(X), **kw), f"lam={lam}")


def test_statuses_shortcut_and_option_quirk():
    pkg = import_pkg()
    p = 2
    y = np.array([1.0, 2.0, 4.0, 1.0, 2.0, 3.0, np.nan, np.nan, 1.0, 2.0, 3.0, 5.0])
    X = np.array([[1, 1], [1, 1], [1, 1],                    # all constant: intercept-only shortcut
                  [1, 1], [2, 1], [3, 1],                    # column 1 constant
                  [1, 2], [2, 3],                            # no valid row
                  [1, 2], [2, 1], [4, 3], [3, 3]], dtype=np.float64)
    off = np.array([0, 3, 6, 8, 12], dtype=np.int64)
    for kw in (dict(), dict(fit_intercept=False), dict(forgetting_factor=0.0), dict(initial_p_diagonal=-1.0),
               dict(forgetting_factor=1.5, fit_intercept=False)):
        core = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw))
        _assert_bits(core, R.batch(off, y, _cols(X), **kw), str(kw))
    core = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, forgetting_factor=0.0))
    assert core[0, p + 5] == 0 and core[0, p] == 7.0 / 3.0       # the shortcut never checks the options
    assert core[1, p + 5] == 1 and core[2, p + 5] == 10 and core[3, p + 5] == 1
    core = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, fit_intercept=False))
    assert core[0, p + 5] == 6


def test_long_group_route():
    """A group above the long-group threshold runs on a wavefront at p <= 8; it must give the lane's bits."""
    pkg = import_pkg()
    rng = np.random.default_rng(11)
    off, y, X = _groups(rng, [100_003, 50, 7], 4, nan_frac=0.01)
    kw = dict(forgetting_factor=0.999, initial_p_diagonal=50.0)
    core = pkg.rls_fit_batch_host(off, y, _cols(X), _opts(pkg, **kw))
    _assert_bits(core, R.batch(off, y, _cols(X), **kw), "long group")
    assert core[0, 4 + 4] == np.sum(np.isfinite(y[:100_003]))


def test_fit_predict_batch():
    pkg = import_pkg()
    rng = np.random.default_rng(3)
    p = 3
    off, y, X = _groups(rng, [30, 1, 25, 4], p, nan_frac=0.2)
    tc = np.array([int(np.sum(~np.isnan(y[off[g]:off[g + 1]]))) for g in range(4)], dtype=np.int64)
    tc[3] = 1
    kw = dict(forgetting_factor=0.98)
    core, pred = pkg.rls_fit_predict_batch_host(off, y, _cols(X), _opts(pkg, **kw), 0.95, train_counts=tc)
    want_core = R.batch(off, y, _cols(X), train_counts=tc, **kw)
    _assert_bits(core, want_core, "records")
    want = np.full((len(y), 3), np.nan)
    for g in range(4):
        rec = want_core[g]
        if rec[p + 5] != 0:
            continue
        for r in range(off[g], off[g + 1]):
            want[r] = R.predict(rec, X[r])
    _assert_bits(pred, want, "predictions")
    assert np.all(np.isnan(pred[off[3]:off[4]]))


def _rows_frames(off, start, end):
    N = int(off[-1])
    lo = np.zeros(N, dtype=np.int64)
    hi = np.zeros(N, dtype=np.int64)
    for g in range(len(off) - 1):
        s, t = int(off[g]), int(off[g + 1])
        for e in range(s, t):
            a = s if start is None else max(s, min(t, e - start))
            b = t if end is None else max(s, min(t, e - end + 1))
            lo[e], hi[e] = a, b
    return lo, hi


def _want_frames(y, X, lo, hi, **kw):
    out = np.array([R.frame_prediction(y, X, int(a), int(b), **kw) for a, b in zip(lo, hi)])
    return np.repeat(out[:, None], 3, axis=1)


@pytest.mark.parametrize("p", [2, 9])
@pytest.mark.parametrize("frame", [(None, 0), (5, 0), (3, -2), (None, 1)])
def test_window_rows_frames(p, frame):
    pkg = import_pkg()
    rng = np.random.default_rng(21 + p)
    off, y, X = _groups(rng, [40, 3, 25], p, nan_frac=0.1)
    X[:12, 0] = 1.0                                        # partition 0: column 0 becomes non-constant at row 12
    kw = dict(forgetting_factor=0.97)
    got = pkg.rls_fit_predict_window_host(off, y, _cols(X), _opts(pkg, **kw), frame)
    lo, hi = _rows_frames(off, frame[0], frame[1])
    _assert_bits(got, _want_frames(y, X, lo, hi, **kw), f"frame {frame}")
    _assert_bits(got, pkg.rls_fit_predict_frames_host(y, _cols(X), lo, hi, _opts(pkg, **kw)), "frames path")


def test_window_invalid_options_null_until_a_column_varies():
    pkg = import_pkg()
    N = 12
    X = np.ones((N, 1))
    X[7:, 0] = np.arange(5.0)
    y = np.arange(N, dtype=np.float64)
    off = np.array([0, N], dtype=np.int64)
    got = pkg.rls_fit_predict_window_host(off, y, [X[:, 0].copy()], _opts(pkg, forgetting_factor=2.0), (None, 0))
    lo, hi = _rows_frames(off, None, 0)
    want = _want_frames(y, X, lo, hi, forgetting_factor=2.0)
    _assert_bits(got, want)
    assert np.all(np.isfinite(got[2:7, 0])) and np.all(np.isnan(got[7:, 0]))   # row 7 is the first that varies


def test_explicit_frames_and_scalar():
    pkg = import_pkg()
    rng = np.random.default_rng(9)
    N, p = 60, 12
    X = rng.normal(size=(N, p))
    y = X.sum(axis=1) + rng.normal(size=N)
    lo = rng.integers(0, N, size=N)
    hi = np.minimum(N, lo + rng.integers(0, 40, size=N))
    got = pkg.rls_fit_predict_frames_host(y, _cols(X), lo, hi, _opts(pkg))
    _assert_bits(got, _want_frames(y, X, lo, hi), "explicit frames p=12")
    xs = np.arange(1.0, 21.0)
    out = pkg.rls_fit([2 * v + 1 for v in xs], [list(xs)])
    rec = R.rls_fit(2 * xs + 1, xs[:, None])
    assert out["n_observations"] == 20 and 1.9 < out["coefficients"][0] < 2.1
    _assert_bits([out["coefficients"][0], out["intercept"]], [rec[0], rec[1]], "scalar")
    assert np.isnan(out["r_squared"]) and np.isnan(out["residual_std_error"])


def test_sql_aggregates():
    pkg = import_pkg()
    rng = np.random.default_rng(4)
    keys = np.repeat([1, 2, 3], [15, 20, 1])
    X = rng.normal(size=(36, 2))
    y = X @ np.array([1.5, -2.0]) + 0.2 * rng.normal(size=36)
    res = pkg.SQL_FUNCTIONS["rls_fit_agg"](keys, y, X.tolist(), {"forgetting_factor": 0.98, "lambda": 0.5})
    off = np.array([0, 15, 35, 36], dtype=np.int64)
    want = R.batch(off, y, _cols(X), forgetting_factor=0.98)
    _assert_bits(res.coefficients, want[:, :2], "rls_fit_agg coefficients")   # `lambda` is ignored: 0.98 stays
    _assert_bits(res.intercept, want[:, 2], "rls_fit_agg intercept")
    assert list(res.is_null) == [False, False, True]
    for name in ("anofox_stats_rls_fit_predict_agg", "rls_fit_predict_agg", "rls_predict_agg", "anofox_stats_rls_predict_agg",
                 "anofox_stats_rls_fit_predict", "rls_fit_predict", "anofox_stats_rls_fit", "rls_fit", "anofox_stats_rls_fit_agg"):
        assert name in pkg.SQL_FUNCTIONS
    yh, lo_, up_ = pkg.rls_fit_predict(keys, np.arange(36), y, X.tolist())
    assert np.array_equal(_bits(yh), _bits(lo_)) and np.array_equal(_bits(yh), _bits(up_))


@pytest.mark.parametrize("p", [1, 3, 5, 8])
@pytest.mark.parametrize("icpt", [True, False])
def test_expanding_one_pass_equals_frames_path(p, icpt):
    """The one-pass expanding kernel (p <= 8) against the frames path and the restatement, bit for bit: columns that become
    non-constant part-way (restarts), NaN y rows, non-finite x rows, and invalid options that null frames only once a column
    varies."""
    pkg = import_pkg()
    rng = np.random.default_rng(300 + p + 10 * icpt)
    off, y, X = _groups(rng, [60, 1, 2, 35, 80], p, nan_frac=0.1, inf_rows=3)
    X[:20, :] = 2.0                                       # partition 0: every column constant first ...
    X[20:30, p - 1] = 2.0                                 # ... then they start to vary one by one
    X[off[3]:off[4], 0] = -1.0                            # partition 3: column 0 constant throughout
    lo, hi = _rows_frames(off, None, 0)
    for kw in (dict(forgetting_factor=0.98, fit_intercept=icpt), dict(forgetting_factor=0.0, fit_intercept=icpt)):
        got = pkg.rls_fit_predict_window_host(off, y, _cols(X), _opts(pkg, **kw), (None, 0))
        _assert_bits(got, pkg.rls_fit_predict_frames_host(y, _cols(X), lo, hi, _opts(pkg, **kw)), f"frames path {kw}")
        _assert_bits(got, _want_frames(y, X, lo, hi, **kw), f"restatement {kw}")


def test_window_null_x_list_does_not_train():
    """A row whose x list is NULL is never buffered by the window aggregate: it does not count toward the NULL rule."""
    pkg = import_pkg()
    keys = np.zeros(4, dtype=np.int64)
    x = [[1.0], None, [3.0], [4.0]]
    y = [1.0, 2.0, 3.1, 3.9]
    yh, _, _ = pkg.rls_fit_predict(keys, np.arange(4), y, x)
    assert np.isnan(yh[2])                                # rows 0 and 2 train (row 1 is not buffered): 2 <= p + 1, NULL
    assert np.isfinite(yh[3])                             # three training rows: a value
