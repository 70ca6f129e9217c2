"""CPU tier of tests/elasticnet_restate.py, the extended-precision yardstick of the elastic net sweeps: against
test_elasticnet_cpu.en_reference (another algorithm's answer to the same contract) at 1e-10, the ridge and OLS closed forms,
the orthonormal soft-threshold case, scikit-learn where it is installed, the statuses, and every input condition on one
constructed case that trips it.  Also bls_restate.moment_conditions and the sweeps' generator (no GPU needed for either)."""
import numpy as np
import pytest

import bls_restate as br
import elasticnet_restate as er
from test_elasticnet_cpu import en_reference


def _data(n, p, seed, shift=1.0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, p)) + shift * rng.normal(size=p)
    y = X @ rng.normal(size=p) + 0.5 + 0.3 * rng.normal(size=n)
    return y, X


def _close(rec, ref, p, tol):
    assert np.array_equal(np.isnan(rec), np.isnan(ref))
    scale = max(np.nanmax(np.abs(ref[:p + 1])), 1e-300)
    err = np.abs(rec - ref)[~np.isnan(ref)] / np.maximum(np.abs(ref[~np.isnan(ref)]), 1e-3 * scale)
    assert err.max() <= tol, err.max()


def test_extended_precision_is_extended():
    assert np.finfo(er.LD).eps < 1e-18


@pytest.mark.parametrize("p,n", [(1, 30), (3, 40), (8, 300), (20, 120)])
@pytest.mark.parametrize("fit_intercept", [True, False])
@pytest.mark.parametrize("scaling", ["raw", "glmnet"])
def test_against_the_coordinate_descent_reference(p, n, fit_intercept, scaling):
    y, X = _data(n, p, 10 + p)
    X[3, 0] = np.nan
    y[5] = np.inf
    if p >= 3:
        X[:, 1] = 2.5                                   # a constant column
    for l1, alpha in ((0.0, 2.0), (0.4, 5.0), (1.0, 12.0), (0.5, 0.0), (0.7, 1e4)):
        a = alpha / n if scaling == "glmnet" else alpha
        res = er.fit_en(y, X, a, l1, fit_intercept, scaling)
        assert res["status"] == 0 and er.input_conditions(res, y, X) == []
        _close(er.record(res), en_reference(y, X, a, l1, fit_intercept, scaling), p, 1e-10)


@pytest.mark.parametrize("fit_intercept", [True, False])
def test_ridge_and_ols_closed_forms(fit_intercept):
    y, X = _data(80, 5, 1)
    A = np.column_stack([X, np.ones(80)]) if fit_intercept else X
    ols = np.linalg.lstsq(A, y, rcond=None)[0]
    rec = er.record(er.fit_en(y, X, 0.0, 0.5, fit_intercept))
    assert np.allclose(rec[:5], ols[:5], rtol=1e-11, atol=0)
    lam = 3.0
    Xc, yc = (X - X.mean(axis=0), y - y.mean()) if fit_intercept else (X, y)
    ridge = np.linalg.solve(Xc.T @ Xc + lam * np.eye(5), Xc.T @ yc)
    rec = er.record(er.fit_en(y, X, lam, 0.0, fit_intercept))
    assert np.allclose(rec[:5], ridge, rtol=1e-11, atol=0)
    r = y - X @ rec[:5] - (rec[5] if fit_intercept else 0.0)
    df = 80 - 5 - int(fit_intercept)
    assert np.isclose(rec[8], np.sqrt(r @ r / df), rtol=1e-12) and np.isclose(rec[6], 1 - r @ r / (yc @ yc), rtol=1e-12)
    assert np.isclose(rec[7], 1 - (1 - rec[6]) * (80 - int(fit_intercept)) / df, rtol=1e-12) and rec[9] == 80


def test_orthonormal_design_gives_the_soft_threshold():
    rng = np.random.default_rng(2)
    Q = rng.normal(size=(50, 4))
    Q, _ = np.linalg.qr(Q - Q.mean(axis=0))
    y = Q @ np.array([3.0, -0.2, 1.0, 0.05]) + 0.01 * rng.normal(size=50)
    lam, l1 = 0.5, 0.7
    rec = er.record(er.fit_en(y, Q, lam, l1))
    c = Q.T @ (y - y.mean())
    expect = np.sign(c) * np.maximum(np.abs(c) - lam * l1, 0.0) / (1 + lam * (1 - l1))
    assert np.allclose(rec[:4], expect, atol=1e-13) and rec[1] == 0.0 and rec[3] == 0.0


def test_against_scikit_learn():
    lm = pytest.importorskip("sklearn.linear_model")
    y, X = _data(120, 6, 5)
    for lam, l1 in ((5.0, 0.5), (20.0, 1.0), (1.0, 0.2)):
        rec = er.record(er.fit_en(y, X, lam, l1))
        sk = lm.ElasticNet(alpha=lam / 120, l1_ratio=l1, fit_intercept=True, tol=1e-14, max_iter=100000).fit(X, y)
        assert np.allclose(rec[:6], sk.coef_, atol=1e-8) and np.isclose(rec[6], sk.intercept_, atol=1e-8)


def test_statuses_and_shortcut():
    y, X = _data(30, 3, 6)
    st = lambda *a, **k: er.fit_en(*a, **k)["status"]  # noqa: E731
    assert st(y, X, alpha=-1.0) == 4 and st(y, X, alpha=np.nan) == 4 and st(y, X, l1_ratio=1.5) == 5
    assert st(y[:1], X[:1]) == 100 and st(y, X, rule_count=1) == 100 and st(y[:0], X[:0]) == 100
    assert st(np.full(5, np.nan), np.ones((5, 3))) == 10
    assert st(y[:3], X[:3]) == 6 and st(y[:3], X[:3], fit_intercept=False) == 0 and st(y[:4], X[:4]) == 0
    rec = er.record(er.fit_en(y, np.ones((30, 3))))
    assert rec[8] == 0 and np.all(np.isnan(rec[:3])) and np.isclose(rec[3], y.mean(), rtol=1e-15)
    assert rec[4] == 0 and rec[5] == 0 and np.isclose(rec[6], np.std(y, ddof=1), rtol=1e-14) and rec[7] == 30
    assert st(y, np.ones((30, 3)), fit_intercept=False) == 6


def test_minimiser_does_not_depend_on_the_column_order():
    y, X = _data(60, 7, 8)
    perm = np.random.default_rng(0).permutation(7)
    a = er.fit_en(y, X, 9.0, 0.8)["coefficients"]
    b = er.fit_en(y, X[:, perm], 9.0, 0.8)["coefficients"]
    assert np.any(a == 0.0) and np.allclose(a[perm], b, rtol=1e-14, atol=0)


def test_each_input_condition_trips_on_a_constructed_case():
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.normal(size=(40, 3)))
    # C = I, no intercept: b_j = S(c_j, lam l1) / (1 + lam (1 - l1)).  c_2 sits 1e-8 below the threshold
    y = Q @ np.array([3.0, 1.0, 0.5 * (1 - 1e-8)])
    res = er.fit_en(y, Q, 1.0, 0.5, False)
    assert er.input_conditions(res, y, Q) == ["an inactive column's gradient lies within 1e-6 of the threshold (degenerate support)"]
    y = Q @ np.array([3.0, 1.0, 0.5 + 1e-7])           # ... and here 1e-7 above it: an active coefficient of 1e-7 / 1.5
    res = er.fit_en(y, Q, 1.0, 0.5, False)
    assert er.input_conditions(res, y, Q) == ["an active coefficient is below 1e-6 of the largest one"]
    y, X = _data(50, 3, 4, shift=0.0)                  # two nearly equal columns: kappa ~ 2e3 > 548 = the bound at p = 3
    X[:, 2] = X[:, 1] + 1e-3 * rng.normal(size=50)
    res = er.fit_en(y, X, 1e-6, 0.5)
    bad = er.input_conditions(res, y, X)
    assert len(bad) == 1 and bad[0].startswith("p kappa^2 2^-53 above 1e-10") and res["kappa"] > er.kappa_bound(3)
    assert abs(er.kappa_bound(8) - 335.5) < 0.5 and abs(er.kappa_bound(128) - 83.9) < 0.1
    res = er.fit_en(y, X, 1e3, 0.0)                    # the ridge rows restore the conditioning
    assert er.input_conditions(res, y, X) == []
    y, X = _data(50, 3, 5)
    yb = y - y.mean() + 1000.0                         # nearly constant far from zero: q_yy / c_yy ~ 1e5
    res = er.fit_en(yb, X, 0.01, 0.5, False, "glmnet")
    assert er.input_conditions(res, yb, X) == ["glmnet scaling without an intercept with q_yy >= 1e4 c_yy"]
    assert er.input_conditions(er.fit_en(yb, X, 0.01, 0.5, True, "glmnet"), yb, X) == []
    assert er.input_conditions(er.fit_en(yb, X, 0.01, 0.5, False, "raw"), yb, X) == []


def test_bls_moment_conditions_carry_the_kappa_bound():
    rng = np.random.default_rng(6)
    y, X = br.make_case(rng, 60, 4, offsets=False)
    res = br.fit_bls(y, X)
    assert br.input_conditions(res, y, X, False) == [] and br.moment_conditions(res, y, X, False) == []
    X[:, 3] = X[:, 2] + 1e-3 * rng.normal(size=60)     # kappa ~ 1e4: inside input_conditions' 1e6, outside the moment bound
    res = br.fit_bls(y, X)
    assert br.input_conditions(res, y, X, False) == []
    bad = br.moment_conditions(res, y, X, False)
    assert len(bad) == 1 and bad[0].startswith("p kappa^2 2^-53 above 1e-10")


def test_sweep_generator_draws_what_it_promises():
    """The generator of tests/test_gpu_fuzz_families.py: both regimes, every width class, no group count a multiple of 64,
    a long group, groups on both sides of n = k + [intercept]; and the first seeds' cases meet the input conditions."""
    import test_gpu_fuzz_families as T
    regimes, classes, long_seen, edge = set(), set(), False, set()
    for seed in range(110_000, 110_040):
        rng = np.random.default_rng(seed)
        icpt = int(rng.integers(0, 2))
        p, G, ns, plain = T._shape(rng, T.CLASS_OF_SEED[seed % 10], icpt)
        assert G % 64 != 0 and (ns.mean() > 128) == plain and (p > 8 or G > 64)
        regimes.add(plain)
        classes.add(next(i for i, (lo, hi) in enumerate(T.CLASSES) if lo <= p <= hi))
        long_seen |= bool((ns > 8192).any())
        edge |= {int(d) for d in (ns - p - icpt) if -1 <= d <= 1}
    assert regimes == {True, False} and classes == {0, 1, 2, 3, 4} and long_seen and edge == {-1, 0, 1}
    statuses = set()
    for seed in (110_000, 110_003):                    # one narrow batch of many groups, one wide batch
        p, offs, y, X, kw, plain = T._en_case(seed)
        rcore, skip, xbar, fits = T._en_restate(p, offs, y, X, kw, f"seed {seed}")
        statuses |= set(int(s) for s in rcore[:, p + 5])
    assert {0, 6, 100} <= statuses
    p, offs, y, X, kw, plain, name = T._bls_case(120_001)
    T._bls_restate(p, offs, y, X, kw, "bls seed 120001")
