"""The quantile regression window function on the MI355X (anofox_hip_quantile_fit_predict_{window,frames}_{host,device},
quantile_fit_predict): the frame shapes and the forced cold starts of tests/test_quantile_window_cpu.py and calls of 64 mixed
partitions at p = 1, 8, 31 and 32 (k up to 33), sampled frames under tests/quantile_window_cases.py::check_frame against the restatement; grid-stride reuse of a
dirty scratch slab; many runs against one run; repeatability; the Python window function; the four entry points against each
other."""
import functools

import numpy as np
import pytest

import quantile_fuzz_cases as qf
import quantile_restate as qr
import quantile_window_cases as qw
from conftest import import_pkg

pytestmark = pytest.mark.gpu


def _opts(pkg, tau, icpt, **kw):
    return pkg.QuantileOptions(tau=tau, fit_intercept=icpt, **kw).batch_options()


def _cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


@pytest.fixture()
def hooks():
    pkg = import_pkg()
    yield pkg.quantile_window_test_hooks
    pkg.quantile_window_test_hooks(0, 0)


def _dirty_the_workspace(pkg):
    """Another quantile call first: the window call then finds positive stale residuals, weights and breakpoints."""
    rng = np.random.default_rng(1)
    X, y = rng.normal(size=(4000, 2)) + 3.0, rng.normal(size=4000) + 5.0
    pkg.quantile_fit_batch_host(np.array([0, 1000, 4000]), y, _cols(X), _opts(pkg, 0.3, True))


SHAPES = [(5, 0), (3, -2), (None, 0), (0, None), (0, 0)]


@pytest.mark.parametrize("icpt", [True, False], ids=["icpt", "noicpt"])
def test_frame_shapes_through_the_window_entry_point(icpt):
    pkg = import_pkg()
    X, y = qw.small_partition()
    n, p = X.shape
    k = p + int(icpt)
    off = np.array([0, n], dtype=np.int64)
    _dirty_the_workspace(pkg)
    for start, end in SHAPES:
        lo, hi = qw.rows_frames(off, start, end)
        for tau in (0.1, 0.5, 0.9):
            pred, rec, its = pkg.quantile_fit_predict_window_host(off, y, _cols(X), _opts(pkg, tau, icpt), (start, end), want_records=True)
            assert np.isnan(pred[:, 1:]).all()
            qw.check_partition(X, y, lo, hi, tau, icpt, rec, its, pred[:, 0], "plain", f"frame {start}..{end} icpt={int(icpt)} tau={tau}")
            if (start, end) == (0, 0):
                assert (rec[:, p + 5] != 0).all() and np.isnan(pred).all()
    Xc, yc = X.copy(), y.copy()
    yc[11], Xc[23] = 0.25, [0.5, 1.5]
    lo, hi = qw.rows_frames(off, k - 1, 0)                       # exactly k valid rows: interpolates
    pred, rec, its = pkg.quantile_fit_predict_window_host(off, yc, _cols(Xc), _opts(pkg, 0.5, icpt), (k - 1, 0), want_records=True)
    qw.check_partition(Xc, yc, lo, hi, 0.5, icpt, rec, its, pred[:, 0], "plain", f"k rows icpt={int(icpt)}")
    full = hi - lo == k
    assert (rec[full, p + 5] == 0).all() and (rec[full, p + 2] <= 1e-12 * np.max(np.abs(yc))).all() and (rec[~full, p + 5] != 0).all()


def test_forced_cold_starts_through_the_frames_entry_point():
    pkg = import_pkg()
    rng = np.random.default_rng([20261018, 10])
    n, p, icpt = 40, 2, True
    k = p + 1
    X = rng.normal(size=(n, p))
    y = X @ [1.0, 2.0] + rng.normal(size=n)
    off = np.array([0, n])
    lo, hi = qw.rows_frames(off, k, 0)                           # k + 1 rows: the leaving row is a basis row on most steps
    lo2, hi2 = (a.copy() for a in qw.rows_frames(off, 9, 0))
    lo2[21], hi2[21] = 2, 14                                     # non-monotone
    lo2[30], hi2[30] = 5, 17
    lo2[31], hi2[31] = 17, 29                                    # disjoint
    lo2[35], hi2[35] = 35, 35                                    # a failed (empty) frame, then the frame after it
    o = _opts(pkg, 0.5, icpt)
    for a, b, what in ((lo, hi, "leaving basis row"), (lo2, hi2, "explicit frames")):
        pred, rec, its = pkg.quantile_fit_predict_frames_host(y, _cols(X), a, b, o, want_records=True)
        qw.check_partition(X, y, a, b, 0.5, icpt, rec, its, pred[:, 0], "plain", what)
        st = pkg.quantile_window_stats()
        assert st["frames"] == n and st["walkers"] == 1 and 1 <= st["restarts"] < st["cold_starts"] <= n
        if what == "leaving basis row":
            assert st["restarts"] >= 0.6 * (n - k - 1)           # k of the k + 1 rows are the basis: the oldest row is one of them 3 times in 4
        else:
            # begun afresh: rows 0 .. k - 1 (too few rows yet; the first fitted frame follows a failed one), 21, 22, 30, 31, 36 and
            # every frame that lost a basis row; restarts are those after a fitted frame: 21, 22, 30, 31 and the basis rows, not 36
            assert st["cold_starts"] - st["restarts"] == k + 1 and 4 <= st["restarts"] < n - 10
    assert rec[35, p + 5] == qr.STATUS_TOO_FEW_ROWS and np.isnan(pred[35]).all()
    # tau outside (0, 1): status 1 on every row, nothing fitted
    pred, rec, its = pkg.quantile_fit_predict_frames_host(y, _cols(X), lo, hi, _opts(pkg, 1.0, icpt), want_records=True)
    assert (rec[:, p + 5] == 1).all() and np.isnan(rec[:, :p + 5]).all() and (its == 0).all() and np.isnan(pred).all()


@functools.lru_cache(maxsize=None)
def mixed_case(p, icpt):
    """64 partitions of 0 to 150 rows, a data kind each (quantile_fuzz_cases._rows); k = p + [intercept] up to 33."""
    rng = np.random.default_rng([20261018, 11, p, int(icpt)])
    ns = rng.integers(0, 151, size=64)
    k = p + int(icpt)
    ns[:6] = [0, 1, 150, k, k + 1, 2 * k]
    off, y, X, kinds, _ = qf._rows(rng, p, icpt, ns.astype(np.int64), False)
    for a in (off, y, X):
        a.setflags(write=False)
    return off, y, X, kinds


@pytest.fixture(scope="module")
def mixed():
    return mixed_case(8, True)


# (p, intercept, output rows checked against the restatement: every STEP-th; the reference costs about k^2 per frame, the GPU
# call fits every row of all 64 partitions whatever the step, and every row's status and NaN pattern is checked below)
MIXED = [(1, True, 8), (8, True, 10), (31, True, 40), (32, False, 40), (32, True, 40)]


@pytest.mark.parametrize("p,icpt,step", MIXED, ids=["p=1", "p=8", "p=31 k=32", "p=32 k=32", "p=32 k=33"])
def test_64_mixed_partitions(p, icpt, step, capsys):
    pkg = import_pkg()
    off, y, X, kinds = mixed_case(p, icpt)
    k = p + int(icpt)
    W = k + 15                                                   # frame W PRECEDING: k + 16 rows, more than k and well inside 150
    lo, hi = qw.rows_frames(off, W, 0)
    pred, rec, its = pkg.quantile_fit_predict_window_host(off, y, _cols(X), _opts(pkg, 0.5, icpt), (W, 0), want_records=True)
    tally = qf.Tally()
    rows = np.arange(step // 2, int(off[-1]), step)
    for g in range(64):
        sel = rows[(rows >= off[g]) & (rows < off[g + 1])]
        qw.check_partition(X, y, lo, hi, 0.5, icpt, rec, its, pred[:, 0], kinds[g], f"p={p} partition {g} ({kinds[g]})", sel, tally)
    with capsys.disabled():
        print("\n  " + tally.line(f"64 mixed partitions, p = {p}, k = {k}, frame {W} preceding, every {step}th row"))
    # every row: the status the row rules give, NaN exactly where the status is not 0, no budget exhausted
    st = rec[:, p + 5]
    for e in range(int(off[-1])):
        Xf, yf = X[lo[e]:hi[e]], y[lo[e]:hi[e]]
        assert st[e] == qr.rule_status(Xf, yf, 0.5, icpt, int(np.sum(~np.isnan(yf)))), e
    assert np.isnan(rec[st != 0, :p + 5]).all() and np.isnan(pred[st != 0]).all() and np.isfinite(rec[st == 0, :p]).all()
    assert (its[st == 0] >= 0).all() and (its[st != 0] == 0).all()
    assert set(np.unique(st)) >= {0.0, 6.0} and len(set(kinds)) >= 5 and tally.groups >= 64
    with pytest.raises(pkg.AnofoxStatsError, match="n_features > 32 is not built"):
        pkg.quantile_fit_predict_window_host([0, 4], np.zeros(4), [np.zeros(4)] * 33, _opts(pkg, 0.5, True))


def test_more_walkers_than_wavefronts_on_a_dirty_slab(mixed, hooks):
    pkg = import_pkg()
    off, y, X, kinds = mixed
    o = _opts(pkg, 0.5, True)
    want = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (24, 0), want_records=True)
    lo, hi = qw.rows_frames(off, 24, 0)
    _, span, _ = pkg.quantile_window_plan(off, lo, hi)
    _dirty_the_workspace(pkg)
    hooks(0, 24 * span * 3)                                      # room for three slabs: three wavefronts stride over ~70 walkers
    got = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (24, 0), want_records=True)
    st = pkg.quantile_window_stats()
    assert st["waves"] == 3 and st["walkers"] > 60 and st["span_rows"] == span
    for a, b in zip(want, got):                                  # a walker's result does not depend on which wavefront ran it
        assert a.tobytes() == b.tobytes()
    hooks(0, 24 * span - 1)
    with pytest.raises(pkg.AnofoxStatsError, match="exceeds the scratch budget"):
        pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (24, 0))


def test_many_runs_equal_one_run_in_loss(hooks):
    pkg = import_pkg()
    rng = np.random.default_rng([20261018, 13])
    n, p = 3000, 3
    X = rng.normal(size=(n, p))
    y = X @ [0.5, 1.0, -1.0] + rng.standard_t(3, size=n)
    off = np.array([0, n])
    o = _opts(pkg, 0.9, True)
    hooks(n, 0)
    one = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (64, 0), want_records=True)
    s1 = pkg.quantile_window_stats()
    hooks(0, 0)
    many = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (64, 0), want_records=True)
    s2 = pkg.quantile_window_stats()
    assert s1["walkers"] == 1 and s2["walkers"] == 3000 // 64 and s2["cold_starts"] >= s2["walkers"]
    assert np.array_equal(one[1][:, p + 3:], many[1][:, p + 3:], equal_nan=True)                 # n_basis_rows, n, status
    ok = one[1][:, p + 5] == 0
    assert ok.sum() == n - 3 and (one[2][ok] >= 0).all() and (many[2][ok] >= 0).all()
    a, b = one[1][ok, p + 2], many[1][ok, p + 2]
    assert (np.abs(a - b) <= 1e-9 * b + 1e-12 * np.max(np.abs(y))).all()          # check_record's tolerance on a loss
    # continuous data: the vertex is unique almost surely, and then both walks return it
    assert (np.abs(one[0][ok, 0] - many[0][ok, 0]) <= 1e-9 * np.max(np.abs(y))).mean() >= 0.99
    lo, hi = qw.rows_frames(off, 64, 0)
    qw.check_partition(X, y, lo, hi, 0.9, True, many[1], many[2], many[0][:, 0], "plain", "many runs", range(0, n, 97))
    # the property the walk exists for, on the device's own counts: fewer pivots than a cold fit per frame needs (k = 4 at least)
    assert np.abs(one[2][ok]).mean() < 4 and np.abs(many[2][ok]).mean() < 4


def test_two_identical_calls_return_identical_bytes(mixed):
    pkg = import_pkg()
    off, y, X, _ = mixed
    o = _opts(pkg, 0.75, True)
    a = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (10, -3), want_records=True)
    _dirty_the_workspace(pkg)
    pkg.quantile_fit_predict_window_host(off, y[::-1].copy(), _cols(X), _opts(pkg, 0.2, False), (None, 0))
    b = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (10, -3), want_records=True)
    for u, v in zip(a, b):
        assert u.tobytes() == v.tobytes()


def test_python_window_function_on_shuffled_input():
    pkg = import_pkg()
    rng = np.random.default_rng([20261018, 14])
    n = 300
    keys = rng.integers(0, 5, size=n)
    order = rng.permutation(n)
    X = rng.normal(size=(n, 2))
    y = X @ [1.0, -1.0] + rng.normal(size=n)
    y[rng.choice(n, 10, replace=False)] = np.nan
    ylist = [None if np.isnan(v) else float(v) for v in y]
    xs = [list(map(float, r)) for r in X]
    opts = {"tau": 0.25, "fit_intercept": True}
    got = pkg.quantile_fit_predict(keys, order, ylist, xs, opts, frame=(15, 0))
    perm = np.lexsort((order, keys))
    srt = pkg.quantile_fit_predict(keys[perm], order[perm], [ylist[i] for i in perm], [xs[i] for i in perm], opts, frame=(15, 0))
    for g, s in zip(got, srt):
        assert np.array_equal(g[perm], s, equal_nan=True)
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and np.isfinite(got[0]).sum() > 250
    off = np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=5))])
    raw = pkg.quantile_fit_predict_window_host(off, y[perm], _cols(X[perm]), _opts(pkg, 0.25, True), (15, 0))
    assert np.array_equal(raw[:, 0], srt[0], equal_nan=True)


def test_entry_points_agree(mixed):
    import torch
    pkg = import_pkg()
    off, y, X, _ = mixed
    o = _opts(pkg, 0.5, True)
    lo, hi = qw.rows_frames(off, 12, -1)
    w_host = pkg.quantile_fit_predict_window_host(off, y, _cols(X), o, (12, -1), want_records=True)
    f_host = pkg.quantile_fit_predict_frames_host(y, _cols(X), lo, hi, o, want_records=True)
    ctx = pkg.Context(0)
    dev = "cuda:0"
    d = lambda a: torch.from_numpy(np.array(a)).to(dev)  # noqa: E731  (a writable copy: the case arrays are read-only)
    w_dev = ctx.quantile_fit_predict_window_device(d(off), d(y), [d(c) for c in _cols(X)], o, (12, -1), want_records=True)
    f_dev = ctx.quantile_fit_predict_frames_device(d(y), [d(c) for c in _cols(X)], d(lo), d(hi), o, want_records=True)
    torch.cuda.synchronize()
    for a, b in zip(w_host, w_dev):                              # the same planner, the same kernel: identical bytes
        assert a.tobytes() == b.cpu().numpy().tobytes()
    for a, b in zip(f_host, f_dev):
        assert a.tobytes() == b.cpu().numpy().tobytes()
    # window and frames cut their runs differently (the frames entry sees one partition): status and n exactly, the loss within
    # check_record's tolerance, yhat wherever both vertices are the unique one
    p = X.shape[1]
    assert np.array_equal(w_host[1][:, p + 4:], f_host[1][:, p + 4:], equal_nan=True)
    ok = w_host[1][:, p + 5] == 0
    a, b = w_host[1][ok, p + 2], f_host[1][ok, p + 2]
    ymax = np.nanmax(np.abs(y))
    assert (np.abs(a - b) <= 1e-9 * b + 1e-12 * ymax).all()
    assert np.array_equal(np.isnan(w_host[0][:, 0]), np.isnan(f_host[0][:, 0]))
    assert np.isnan(ctx.quantile_fit_predict_window_device(d(off), d(y), [d(c) for c in _cols(X)], o, (12, -1))[:, 1:].cpu().numpy()).all()
    ctx.close()
