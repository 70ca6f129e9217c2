"""Grouped elastic net on the MI355X: the batch records against the NumPy coordinate-descent reference
(test_elasticnet_cpu.en_reference) and its KKT conditions, the identities with ridge (l1_ratio = 0) and OLS (alpha = 0),
exact sparsity beyond lambda_max, per-group statuses, determinism, and the agreement of the three entry points."""
import numpy as np
import pytest

from conftest import assert_records_match, import_pkg
from test_elasticnet_cpu import en_lambda, en_moments, en_reference, lambda_max

pytestmark = pytest.mark.gpu

WIDTHS = [1, 3, 8, 9, 16, 27, 33, 64, 128]


def _groups(G, n, p, seed, intercept_shift=0.7):
    rng = np.random.default_rng(seed)
    rows = [n + int(k) for k in rng.integers(0, 7, size=G)]
    off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    N = int(off[-1])
    X = rng.normal(size=(N, p)) + rng.normal(size=p)
    beta = rng.normal(size=p) * (rng.random(size=p) < 0.6)
    y = X @ beta + intercept_shift + 0.5 * rng.normal(size=N)
    return off, y, X


def _opts(pkg, **kw):
    o = pkg.ElasticNetOptions(**kw)
    return o.batch_options()


def _fit(pkg, off, y, X, **kw):
    return pkg.elasticnet_fit_batch_host(off, y, [X[:, j].copy() for j in range(X.shape[1])], _opts(pkg, **kw))


def _kkt(y, X, rec, alpha, l1, fit_intercept, scaling):
    m = en_moments(y, X, fit_intercept)
    lam = en_lambda(m, alpha, scaling)
    act = m["nonconst"]
    b = np.where(act, rec[:X.shape[1]], 0.0)
    g = m["c"] - m["C"] @ b
    scale = max(lam * l1, np.max(np.abs(m["c"])))
    worst = 0.0
    for j in np.nonzero(act)[0]:
        if b[j] != 0.0:
            worst = max(worst, abs(g[j] - lam * (1 - l1) * b[j] - lam * l1 * np.sign(b[j])) / scale)
        else:
            worst = max(worst, max(abs(g[j]) - lam * l1 * (1 + 1e-8), 0.0) / scale)
    return worst


@pytest.mark.parametrize("p", WIDTHS)
def test_against_reference_and_kkt(p):
    pkg = import_pkg()
    G, n = 6, max(3 * p, 40)
    off, y, X = _groups(G, n, p, 100 + p)
    for fit_intercept in (True, False):
        for scaling in ("raw", "glmnet"):
            for l1 in (0.0, 0.3, 1.0):
                g0 = slice(off[0], off[1])
                lm = lambda_max(y[g0], X[g0], max(l1, 1e-3), fit_intercept)
                if scaling == "glmnet":
                    m = en_moments(y[g0], X[g0], fit_intercept)
                    lm /= en_lambda(m, 1.0, "glmnet")
                for alpha in (0.0, 0.05 * lm, 0.5 * lm, 1.5 * lm):
                    if alpha == 0.0 and p >= 64:
                        continue  # OLS by coordinate descent at p = 64..128: slow to 1e-13, covered at alpha > 0
                    core, its = _fit(pkg, off, y, X, alpha=alpha, l1_ratio=l1, fit_intercept=fit_intercept,
                                     lambda_scaling=scaling, tolerance=1e-13, max_iterations=100000)
                    for g in range(G):
                        s = slice(off[g], off[g + 1])
                        ref = en_reference(y[s], X[s], alpha, l1, fit_intercept, scaling)
                        assert core[g, p + 5] == 0 and its[g] > 0, (g, core[g, p + 5], its[g])
                        err = np.linalg.norm(core[g, :p] - ref[:p]) / max(np.linalg.norm(ref[:p]), 1.0)
                        assert err <= 1e-8, (p, fit_intercept, scaling, l1, alpha, g, err)
                        assert _kkt(y[s], X[s], core[g], alpha, l1, fit_intercept, scaling) <= 1e-8
                        if fit_intercept:
                            assert abs(core[g, p] - ref[p]) <= 1e-8 * max(abs(ref[p]), 1.0)
                        else:
                            assert np.isnan(core[g, p])
                        assert np.allclose(core[g, p + 1:p + 5], ref[p + 1:p + 5], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("p", [3, 8, 16, 64])
@pytest.mark.parametrize("scaling", ["raw", "glmnet"])
def test_l1_zero_matches_the_ridge_batch(p, scaling):
    pkg = import_pkg()
    off, y, X = _groups(40, 5 * p + 30, p, 7 + p)
    cols = [X[:, j].copy() for j in range(p)]
    ridge = pkg.RegressionOptions(alpha=2.5, lambda_scaling=scaling).batch_options("ridge")
    rcore, _ = pkg.fit_batch_host(off, y, cols, None, ridge)
    core, its = pkg.elasticnet_fit_batch_host(off, y, cols, _opts(pkg, alpha=2.5, l1_ratio=0.0, lambda_scaling=scaling,
                                                                   tolerance=1e-14, max_iterations=100000))
    assert np.all(its > 0)
    assert_records_match(core, rcore, p)


@pytest.mark.parametrize("p", [2, 8, 12, 40])
def test_alpha_zero_matches_ols(p):
    pkg = import_pkg()
    off, y, X = _groups(30, 8 * p + 40, p, 21 + p)
    cols = [X[:, j].copy() for j in range(p)]
    ocore, _ = pkg.fit_batch_host(off, y, cols, None, pkg.RegressionOptions().batch_options("ols"))
    core, its = pkg.elasticnet_fit_batch_host(off, y, cols, _opts(pkg, alpha=0.0, l1_ratio=0.5, tolerance=1e-14,
                                                                   max_iterations=100000))
    assert np.all(its > 0)
    assert_records_match(core, ocore, p)


@pytest.mark.parametrize("p", [4, 20])
def test_exact_sparsity_beyond_lambda_max(p):
    pkg = import_pkg()
    off, y, X = _groups(10, 60, p, 31 + p)
    lm = max(lambda_max(y[off[g]:off[g + 1]], X[off[g]:off[g + 1]], 0.6) for g in range(10))
    core, its = _fit(pkg, off, y, X, alpha=lm * 1.01, l1_ratio=0.6)
    assert np.all(core[:, :p] == 0.0) and np.all(its == 1)
    means = np.array([y[off[g]:off[g + 1]].mean() for g in range(10)])
    assert np.allclose(core[:, p], means, rtol=1e-13)
    assert np.all(core[:, p + 1] == 0.0)


@pytest.mark.parametrize("p", [3, 12])
def test_edge_cases_per_group(p):
    pkg = import_pkg()
    rng = np.random.default_rng(5)
    n = 30
    blocks_y, blocks_x = [], []
    y0 = rng.normal(size=n)
    x0 = rng.normal(size=(n, p))
    # 0: NaN rows; 1: a constant column; 2: every column constant; 3: no valid row; 4: too few rows; 5: one row
    y1 = y0.copy(); y1[[2, 5]] = np.nan
    x1 = x0.copy(); x1[7, 0] = np.nan
    blocks_y += [y1]; blocks_x += [x1]
    x2 = x0.copy(); x2[:, 1] = 4.0
    blocks_y += [y0]; blocks_x += [x2]
    blocks_y += [y0]; blocks_x += [np.full((n, p), 2.5)]
    blocks_y += [np.full(n, np.nan)]; blocks_x += [x0]
    blocks_y += [y0[:p]]; blocks_x += [x0[:p]]
    blocks_y += [y0[:1]]; blocks_x += [x0[:1]]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blocks_y])]).astype(np.int64)
    y = np.concatenate(blocks_y)
    X = np.concatenate(blocks_x)
    core, its = _fit(pkg, off, y, X, alpha=0.3, l1_ratio=0.4, tolerance=1e-13, max_iterations=100000)
    for g in range(6):
        s = slice(off[g], off[g + 1])
        ref = en_reference(y[s], X[s], 0.3, 0.4)
        assert core[g, p + 5] == ref[p + 5], g
        assert np.allclose(core[g], ref, rtol=1e-8, atol=1e-10, equal_nan=True), (g, core[g], ref)
    assert list(core[3:, p + 5]) == [10, 6, 100]
    assert np.isnan(core[1, 1]) and np.all(np.isnan(core[2, :p])) and core[2, p + 1] == 0.0
    # alpha < 0, l1_ratio outside [0, 1]: every group carries the status, the call succeeds
    for kw, st in (({"alpha": -1.0}, 4), ({"l1_ratio": 1.5}, 5), ({"l1_ratio": -0.1}, 5)):
        c2, _ = _fit(pkg, off[:3], y[:off[2]], X[:off[2]], **kw)
        assert np.all(c2[:, p + 5] == st) and np.all(np.isnan(c2[:, :p + 5]))
    # no intercept with every column constant -> 6
    c3, _ = _fit(pkg, off[2:4] - off[2], y[off[2]:off[3]], X[off[2]:off[3]], fit_intercept=False)
    assert c3[0, p + 5] == 6


@pytest.mark.parametrize("p", [5, 30])
def test_iteration_limit_reports_negative_sweeps(p):
    pkg = import_pkg()
    off, y, X = _groups(8, 80, p, 41)
    core, its = _fit(pkg, off, y, X, alpha=0.01, l1_ratio=0.5, max_iterations=1, tolerance=1e-14)
    assert np.all(its == -1) and np.all(core[:, p + 5] == 0)
    core2, its2 = _fit(pkg, off, y, X, alpha=0.01, l1_ratio=0.5, max_iterations=100000, tolerance=1e-10)
    assert np.all(its2 > 1)


@pytest.mark.parametrize("p", [8, 9, 64])
def test_determinism_and_entry_points_agree(p):
    import torch
    pkg = import_pkg()
    off, y, X = _groups(300, 50 + p, p, 51 + p)
    o = _opts(pkg, alpha=1.5, l1_ratio=0.5, tolerance=1e-10)
    cols = [X[:, j].copy() for j in range(p)]
    c1, i1 = pkg.elasticnet_fit_batch_host(off, y, cols, o)
    c2, i2 = pkg.elasticnet_fit_batch_host(off, y, cols, o)
    assert c1.tobytes() == c2.tobytes() and np.array_equal(i1, i2)
    ctx = pkg.Context(0)
    try:
        d = torch.device("cuda:0")
        dc, di = ctx.elasticnet_fit_batch_device(torch.from_numpy(off).to(d), torch.from_numpy(y).to(d),
                                                 [torch.from_numpy(c).to(d) for c in cols], o)
        torch.cuda.synchronize()
        assert dc.cpu().numpy().tobytes() == c1.tobytes() and np.array_equal(di.cpu().numpy(), i1)
    finally:
        ctx.close()
    s = slice(off[0], off[1])
    r = pkg.elasticnet_fit(list(y[s]), [list(X[s, j]) for j in range(p)],
                           {"alpha": 1.5, "l1_ratio": 0.5, "tolerance": 1e-10})
    assert np.array_equal(np.array(r["coefficients"]), c1[0, :p])
    assert [r["intercept"], r["r_squared"], r["adj_r_squared"], r["residual_std_error"], r["n_observations"]] == list(c1[0, p:p + 5])
    assert r["n_features"] == p


def test_scalar_errors_follow_the_reference():
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="All rows filtered due to NULL/NaN values"):
        pkg.elasticnet_fit([None, None, None], [[1.0, 2.0, 3.0]])
    with pytest.raises(pkg.InvalidInputException, match="Insufficient data: 1 rows, 2 features"):
        pkg.elasticnet_fit([1.0, 2.0], [[1.0, None], [3.0, 5.0]], {"intercept": False, "alpha": 0.1})


@pytest.mark.parametrize("p", [4, 20])
def test_near_exact_fit_takes_the_rss_from_the_rows(p):
    """rss / tss far below 1e-7: the moment identity S_yy - 2 b'c + b'C b has cancelled, the statistics come from the rows."""
    pkg = import_pkg()
    rng = np.random.default_rng(61 + p)
    G, n = 12, 5 * p + 40
    off = (np.arange(G + 1) * n).astype(np.int64)
    X = rng.normal(size=(G * n, p)) * 3.0 + 10.0
    fit = X @ rng.normal(size=p) + 1e-6 * rng.normal(size=G * n)
    for fit_intercept in (True, False):
        y = fit + (2.0 if fit_intercept else 0.0)
        core, its = _fit(pkg, off, y, X, alpha=1e-6, l1_ratio=0.5, fit_intercept=fit_intercept, tolerance=1e-14, max_iterations=100000)
        for g in range(G):
            s = slice(off[g], off[g + 1])
            ref = en_reference(y[s], X[s], 1e-6, 0.5, fit_intercept)
            assert core[g, p + 5] == 0
            assert 1.0 - ref[p + 1] < 1e-9                   # the regime of the row path
            assert abs(core[g, p + 1] - ref[p + 1]) <= 1e-12 and abs(core[g, p + 2] - ref[p + 2]) <= 1e-12
            # the statistics of the record's own coefficients, summed over the rows
            b0 = core[g, p] if fit_intercept else 0.0
            rss = float(((y[s] - b0 - X[s] @ core[g, :p]) ** 2).sum())
            tss = float(((y[s] - y[s].mean()) ** 2).sum()) if fit_intercept else float(y[s] @ y[s])
            df = n - p - (1 if fit_intercept else 0)
            r2 = 1.0 - rss / tss
            assert abs(core[g, p + 1] - r2) <= 1e-13
            assert abs(core[g, p + 2] - (1.0 - (1.0 - r2) * (n - (1 if fit_intercept else 0)) / df)) <= 1e-13
            assert abs(core[g, p + 3] / np.sqrt(rss / df) - 1.0) <= 1e-6, (core[g, p + 3], np.sqrt(rss / df))


def test_several_slabs_of_wide_records_match_single_slab_calls():
    """p = 128: more groups than one slab of wide records holds (two streams, group_base > 0 in the solve and rows kernels)."""
    pkg = import_pkg()
    p, n = 128, 130
    G = 13800                      # one slab holds (1 << 30) / record bytes = 13 785 groups at p = 128
    rng = np.random.default_rng(71)
    off = (np.arange(G + 1) * n).astype(np.int64)
    N = G * n
    cols = [rng.standard_normal(N) for _ in range(p)]
    y = sum(cols[j] * (0.5 if j % 3 == 0 else 0.0) for j in range(p)) + 1.0 + 0.3 * rng.standard_normal(N)
    y[off[G - 1]:off[G]] = 5.0 + 1e-9 * rng.standard_normal(n)   # (a group whose rss is tiny: the rows kernel in the last slab)
    o = _opts(pkg, alpha=2.0, l1_ratio=0.5, tolerance=1e-8)
    core, its = pkg.elasticnet_fit_batch_host(off, y, cols, o)
    h = G // 2
    c1, i1 = pkg.elasticnet_fit_batch_host(off[:h + 1], y[:off[h]], [c[:off[h]] for c in cols], o)
    c2, i2 = pkg.elasticnet_fit_batch_host(off[h:] - off[h], y[off[h]:], [c[off[h]:] for c in cols], o)
    assert np.all(core[:, p + 5] == 0) and np.all(its > 0)
    assert np.array_equal(core, np.vstack([c1, c2]), equal_nan=True)
    assert np.array_equal(its, np.concatenate([i1, i2]))


@pytest.mark.parametrize("p", [1, 8, 9, 64, 65, 128])
def test_five_kinds_of_group_at_the_path_boundaries(p):
    """Both ends of the narrow path, the first wide width and both sides of the wide kernel's one / two columns per lane: a plain
    group of 2p + 3 rows, an exact fit (the moment identity cancels: the rows give the statistics), every column constant (the
    shortcut), p rows (status 6) and an empty group (status 100; the reference takes no empty input), twice with identical bytes."""
    pkg = import_pkg()
    rng = np.random.default_rng(900 + p)
    n_plain, n_exact = 2 * p + 3, 5 * p + 40
    Xp = rng.normal(size=(n_plain, p)) * 3.0 + 10.0
    Xe = rng.normal(size=(n_exact, p)) * 3.0 + 10.0
    blocks = [(Xp @ rng.normal(size=p) + 2.0 + 0.5 * rng.normal(size=n_plain), Xp), (Xe @ rng.normal(size=p) + 2.0, Xe),
              (rng.normal(size=n_plain), np.full((n_plain, p), 2.5)), (rng.normal(size=p), rng.normal(size=(p, p))),
              (np.zeros(0), np.zeros((0, p)))]
    off = np.concatenate([[0], np.cumsum([len(b[0]) for b in blocks])]).astype(np.int64)
    y, X = np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks])
    kw = dict(alpha=1e-6, l1_ratio=0.5, tolerance=1e-13, max_iterations=100000)
    core, its = _fit(pkg, off, y, X, **kw)
    assert list(core[:, p + 5]) == [0, 0, 0, 6 if p > 1 else 100, 100]    # (p = 1: the group of p rows has fewer than 2)
    for g in range(4):
        ref = en_reference(blocks[g][0], blocks[g][1], 1e-6, 0.5)
        assert core[g, p + 5] == ref[p + 5], g
        if g == 1:
            assert 1.0 - ref[p + 1] < 1e-9                      # the regime of the row path
            err = np.linalg.norm(core[g, :p] - ref[:p]) / max(np.linalg.norm(ref[:p]), 1.0)
            assert err <= 1e-8 and abs(core[g, p] - ref[p]) <= 1e-8 * max(abs(ref[p]), 1.0)
            assert abs(core[g, p + 1] - ref[p + 1]) <= 1e-12 and abs(core[g, p + 2] - ref[p + 2]) <= 1e-12 and core[g, p + 4] == ref[p + 4]
        else:
            assert np.allclose(core[g], ref, rtol=1e-8, atol=1e-10, equal_nan=True), (g, core[g], ref)
    assert np.all(np.isnan(core[2, :p])) and core[2, p + 1] == 0.0 and np.all(np.isnan(core[3:, :p + 5]))
    core2, its2 = _fit(pkg, off, y, X, **kw)
    assert core.tobytes() == core2.tobytes() and its.tobytes() == its2.tobytes()
