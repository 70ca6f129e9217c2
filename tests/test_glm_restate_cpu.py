"""The yardstick's own checks: tests/glm_restate.py against closed forms."""
import math

import numpy as np

import glm_restate as R


def test_intercept_only_poisson_is_log_mean():
    y = np.array([0.0, 3.0, 1.0, 7.0, 2.0, 2.0])
    x = np.full((6, 1), 2.0)                       # a constant column: dropped
    r = R.fit(R.POISSON, y, x)
    assert r["status"] == 0 and not r["separated"] and np.isnan(r["coef"][0]) and r["n_params"] == 1
    assert abs(r["intercept"] - math.log(y.mean())) <= 1e-12


def test_intercept_only_logistic_is_logit_mean():
    y = np.array([0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0])
    r = R.fit(R.BINOMIAL, y, np.full((7, 1), -1.0))
    m = y.mean()
    assert abs(r["intercept"] - math.log(m / (1 - m))) <= 1e-12
    assert abs(r["deviance"] - r["null_deviance"]) <= 1e-12 * r["null_deviance"]


def test_saturated_two_by_two_table():
    # cells (x = 0: 3 of 10), (x = 1: 8 of 12): intercept = logit(0.3), slope = logit(8 / 12) - logit(0.3)
    y = np.array([1.0] * 3 + [0.0] * 7 + [1.0] * 8 + [0.0] * 4)
    x = np.array([0.0] * 10 + [1.0] * 12)[:, None]
    r = R.fit(R.BINOMIAL, y, x)
    logit = lambda v: math.log(v / (1 - v))
    assert abs(r["intercept"] - logit(0.3)) <= 1e-11 and abs(r["coef"][0] - (logit(8 / 12) - logit(0.3))) <= 1e-11
    se = math.sqrt(1 / 3 + 1 / 7 + 1 / 8 + 1 / 4)    # the log odds ratio's standard error
    assert abs(r["se"][0] - se) <= 1e-9


def test_noise_free_poisson_mean_is_recovered():
    x = np.array([float(i % 10) for i in range(40)])[:, None]
    y = np.exp(0.5 + 0.3 * x[:, 0])
    r = R.fit(R.POISSON, y, x)
    assert abs(r["intercept"] - 0.5) <= 1e-10 and abs(r["coef"][0] - 0.3) <= 1e-10
    assert abs(r["deviance"]) <= 1e-10 and r["converged"]


def test_large_lambda_drives_coefficients_to_zero():
    rng = np.random.default_rng(0)
    x = rng.uniform(-1, 1, (50, 3))
    y = rng.poisson(np.exp(0.4 + x @ [0.8, -0.5, 0.3])).astype(float)
    small, large = R.fit(R.POISSON, y, x, lam=0.0), R.fit(R.POISSON, y, x, lam=1e8)
    assert np.max(np.abs(large["coef"])) <= 1e-6 < np.max(np.abs(small["coef"]))
    assert abs(large["intercept"] - math.log(y.mean())) <= 1e-6     # the intercept is not penalised


def test_offset_recovers_the_rate_model():
    n = 40
    x = np.array([float(i % 8) for i in range(n)])[:, None]
    expo = np.array([1.0 + (i % 3) for i in range(n)])
    y = expo * np.exp(0.2 + 0.4 * x[:, 0])
    r = R.fit(R.POISSON, y, x, offset=np.log(expo))
    assert abs(r["intercept"] - 0.2) <= 1e-10 and abs(r["coef"][0] - 0.4) <= 1e-10


def test_flags_and_statuses():
    x = np.linspace(-1, 1, 20)[:, None]
    sep = R.fit(R.BINOMIAL, (x[:, 0] > 0).astype(float), x)
    assert sep["status"] == 0 and (sep["separated"] or sep["max_abs_eta"] > 20)
    assert R.fit(R.POISSON, np.array([1.0, -1.0, 2.0]), x[:3])["status"] == 1
    assert R.fit(R.BINOMIAL, np.array([1.0, 1.5, 0.0]), x[:3])["status"] == 1
    assert R.fit(R.POISSON, np.array([np.nan, np.nan]), x[:2])["status"] == 10
    assert R.fit(R.POISSON, np.array([1.0]), np.array([[0.3, 0.1]]), fit_intercept=False)["status"] == 6
    dup = R.fit(R.POISSON, np.array([1.0, 2.0, 0.0, 4.0, 3.0, 1.0]), np.column_stack([x[:6, 0], x[:6, 0]]))
    assert dup["n_params"] == 2 and dup["kappa"] == np.inf
