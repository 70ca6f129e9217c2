"""The prediction-error variance of the mixed model, pinned before any kernel: Henderson's mixed-model-equation inverse
(tests/glmm_predict_restate.py, dense) against the closed form of DESIGN.md §1 "Mixed-model fit-predict" on tiny well-conditioned
panels (3 levels x 2 to 4 rows, p = 1 and 2), with unseen levels, theta = 0 and a dropped column."""
import numpy as np
import pytest

import glmm_predict_restate as PR

# ten times the largest deviation between the two float64 computations over the cases below, relative to the largest element of
# the vector compared, measured once (4.95e-15: p = 2, seed 2, theta = 10; docs/PARITY.md, "Mixed-model fit-predict")
TOL = 5e-14


def tiny(p, seed, sizes=(2, 3, 4)):
    rng = np.random.default_rng(seed)
    levels = np.repeat(np.arange(len(sizes)), sizes)
    X = np.column_stack([np.ones(len(levels)), rng.normal(size=(len(levels), p))])
    y = 1.0 + X[:, 1:].sum(axis=1) + rng.normal(size=len(sizes))[levels] + 0.5 * rng.normal(size=len(levels))
    return y, X, levels


def worst(a, b):
    """the largest deviation of a vector, relative to its largest element"""
    return max(float(np.max(np.abs(x - y)) / np.max(np.abs(y))) for x, y in zip(a, b))


CASES = [(p, seed, theta) for p in (1, 2) for seed in (1, 2, 3) for theta in (0.0, 1e-3, 0.4, 2.5, 10.0)]


@pytest.mark.parametrize("p, seed, theta", CASES)
def test_the_closed_form_is_the_henderson_inverse(p, seed, theta):
    y, X, levels = tiny(p, seed)
    rng = np.random.default_rng(100 + seed)
    # the training rows themselves, new rows of the three levels, and rows of two levels that have no training row
    A_new = np.vstack([X, np.column_stack([np.ones(8), rng.normal(size=(8, p))])])
    lev_new = np.concatenate([levels, [0, 1, 2, 2, 3, 3, 4, 4]])
    h = PR.henderson(y, X, levels, 5, theta, 0.7, A_new, lev_new)
    c = PR.closed_form(y, X, levels, 5, theta, 0.7, A_new, lev_new)
    dev = worst(c, h)
    print("p %d seed %d theta %g: largest relative deviation %.2e" % (p, seed, theta, dev))
    assert dev <= TOL
    if theta > 0.0:   # an unseen level: s2 (a'A^-1 a + theta), and its prediction is the population one
        assert np.array_equal(c[0][-4:], c[1][-4:]) and np.all(c[2][-4:] > 0.7 * theta)
    else:
        assert np.array_equal(c[0], c[1])


def test_theta_zero_is_the_ols_confidence_variance():
    y, X, levels = tiny(2, 7)
    var = PR.closed_form(y, X, levels, 3, 0.0, 1.3, X, levels)[2]
    assert worst([var], [1.3 * np.einsum("ij,jk,ik->i", X, np.linalg.inv(X.T @ X), X)]) <= TOL


def test_a_dropped_column_contributes_nothing():
    y, X, levels = tiny(2, 9)
    cols = [X[:, 1], X[:, 2], 2.0 * X[:, 1] - X[:, 2]]   # the third is aliased: the pivot rule keeps (1, x1, x2)
    out = PR.panel_reference(y, cols, levels, 3, True, 0.4, 0.7, keep=[True, True, True, False])
    ref = PR.closed_form(y, X, levels, 3, 0.4, 0.7, X, levels)
    assert worst(out, (ref[0], ref[1], np.sqrt(ref[2]))) <= TOL


def test_prediction_rows_and_nan_rows():
    y, X, levels = tiny(1, 11, sizes=(3, 3, 3))
    y2, x2 = y.copy(), X[:, 1].copy()
    y2[6:] = np.nan   # level 2 has prediction rows only: an unseen level
    x2[0] = np.nan
    out = PR.panel_reference(y2, [x2], levels, 3, True, 0.4, 0.7)
    assert np.all(np.isnan(out[:, 0])) and np.all(np.isfinite(out[:, 1:]))
    assert np.array_equal(out[0, 6:], out[1, 6:])
    ok = np.arange(1, 6)
    A = X[ok]
    unseen = PR.closed_form(y[ok], A, levels[ok], 3, 0.4, 0.7, X[6:], levels[6:])
    assert worst([out[2, 6:] ** 2], [unseen[2]]) <= TOL
