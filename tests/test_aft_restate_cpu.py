"""The AFT yardstick checked on its own (tests/aft_restate.py): derivatives against central differences, the lognormal / OLS
identity, the reference's unit-test fixtures rebuilt from their formula, information x vcov = I, the row rules and statuses, and
the share of the generated GPU-tier groups that is inside the tests' condition.  The fixture inputs and the restatement's outputs
are stored under tests/golden/aft/ (data only)."""
import json
import math
import os

import numpy as np
import pytest

import aft_cases as AC
import aft_restate as R
from conftest import GOLDEN

DISTS = (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC, R.EXPONENTIAL)


def survival_fixture(dist, beta0, beta1, sigma, n, censor_at=None):
    """The reference's deterministic fixture (aft.rs, survival_fixture): x = (i mod 10) / 3, the time the model's own quantile at
    p = (i + 1/2) / n, censored at censor_at + 0.9 (i mod 7) when it is later than that."""
    time, event, xs = [], [], []
    for i in range(n):
        x = (i % 10) / 3.0
        t = R.quantile_time(dist, (i + 0.5) / n, beta0 + beta1 * x, sigma)
        c = None if censor_at is None else censor_at + (i % 7) * 0.9
        if c is not None and t > c:
            time.append(c), event.append(0.0)
        else:
            time.append(t), event.append(1.0)
        xs.append(x)
    return np.array(time), np.array(xs)[:, None], np.array(event)


def golden(name):
    with open(os.path.join(GOLDEN, "aft", name)) as f:
        return json.load(f)


@pytest.mark.parametrize("dist", DISTS)
def test_gradient_and_hessian_against_central_differences(dist):
    t, x, e = survival_fixture(dist, 1.2, 0.4, 1.0 if dist == R.EXPONENTIAL else 0.7, 60, 6.0)
    assert 0 < np.sum(e == 0) < 60
    A, logt = np.column_stack([np.ones(60), x]), np.log(t)
    fs = not R.scale_is_fixed(dist)
    theta = np.array([1.1, 0.35, -0.3]) if fs else np.array([1.1, 0.35])
    ll, g, H = R.derivatives(dist, A, logt, e, theta, fs)
    assert ll == R.loglik(dist, A, logt, e, theta, fs)
    h = 1e-5
    for j in range(len(theta)):
        d = np.zeros(len(theta))
        d[j] = h
        num = (R.loglik(dist, A, logt, e, theta + d, fs) - R.loglik(dist, A, logt, e, theta - d, fs)) / (2 * h)
        assert abs(g[j] - num) <= 1e-6 * max(1.0, abs(g[j])), (dist, j, g[j], num)
        gp, gm = R.derivatives(dist, A, logt, e, theta + d, fs)[1], R.derivatives(dist, A, logt, e, theta - d, fs)[1]
        numh = (gp - gm) / (2 * h)
        assert np.all(np.abs(H[j] - numh) <= 1e-6 * np.maximum(1.0, np.abs(H[j]))), (dist, j, H[j], numh)
    assert np.allclose(H, H.T, rtol=1e-13, atol=0)


@pytest.mark.parametrize("dist", (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC))
def test_row_terms_against_central_differences(dist):
    for ev in (True, False):
        for z in (-7.5, -2.0, -0.5, 0.0, 0.5, 1.5, 4.0, 7.5):
            zz = np.array([z - 1e-5, z, z + 1e-5])
            c, u, v = R.terms(dist, np.array([ev] * 3), zz)
            assert abs(u[1] - (c[2] - c[0]) / 2e-5) <= 1e-7 * max(1.0, abs(u[1])), (dist, ev, z)
            assert abs(v[1] - (u[2] - u[0]) / 2e-5) <= 1e-7 * max(1.0, abs(v[1])), (dist, ev, z)
            assert v[1] <= 0.0
    # the normal kernel in the far right tail: finite, and continuous across the switch to the Mills-ratio expansion
    c, u, v = R.terms(R.LOGNORMAL, np.array([False, False]), np.array([37.0, 50.0]))
    assert np.all(np.isfinite(c)) and np.all(u < 0) and c[1] < -1000.0


def test_uncensored_lognormal_is_ols_of_log_time():
    t, x, e = survival_fixture(R.LOGNORMAL, 1.0, 0.4, 0.5, 200)
    fit = R.fit(R.LOGNORMAL, t, x, e)
    ols = np.linalg.lstsq(np.column_stack([np.ones(200), x]), np.log(t), rcond=None)[0]
    assert fit["status"] == 0 and abs(fit["intercept"] - ols[0]) <= 1e-9 and abs(fit["coef"][0] - ols[1]) <= 1e-9
    rss = np.sum((np.log(t) - ols[0] - ols[1] * x[:, 0]) ** 2)
    assert abs(fit["scale"] - math.sqrt(rss / 200)) <= 1e-9     # the maximum likelihood scale divides by n


def test_reference_fixtures_recover_their_parameters():
    """aft.rs: recovers_the_generating_parameters_without_censoring, censoring_is_accounted_for_rather_than_ignored,
    exponential_holds_the_scale_at_one, with the reference's stated bounds; the outputs are the stored ones."""
    stored = golden("fixtures.json")
    for dist in (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC):
        t, x, e = survival_fixture(dist, 1.5, 0.35, 0.6, 400)
        f = R.fit(dist, t, x, e)
        assert f["status"] == 0 and abs(f["coef"][0] - 0.35) < 0.05 and abs(f["intercept"] - 1.5) < 0.1 and abs(f["scale"] - 0.6) < 0.1
        s = stored["uncensored_%s" % R.NAMES[dist]]
        assert np.allclose(t[:8], s["time_head"], rtol=1e-13, atol=0)
        assert np.allclose(f["theta"], s["theta"], rtol=0, atol=1e-9) and abs(f["ll"] - s["ll"]) <= 1e-9 * abs(s["ll"])
    t, x, e = survival_fixture(R.WEIBULL, 2.0, 0.3, 0.5, 300, 9.0)
    assert np.sum(e == 0) > 50
    honest, naive = R.fit(R.WEIBULL, t, x, e), R.fit(R.WEIBULL, t, x, np.ones(300))
    assert honest["n_censored"] == int(np.sum(e == 0)) and naive["n_censored"] == 0
    assert abs(honest["intercept"] - 2.0) < 0.1 and abs(honest["coef"][0] - 0.3) < 0.05 and abs(honest["scale"] - 0.5) < 0.05
    assert naive["coef"][0] < 0.5 * honest["coef"][0] and naive["scale"] < 0.8 * honest["scale"]
    s = stored["censored_weibull"]
    assert np.allclose(honest["theta"], s["theta"], rtol=0, atol=1e-9) and np.allclose(naive["theta"], s["naive_theta"], rtol=0, atol=1e-9)
    assert abs(honest["null_ll"] - s["null_ll"]) <= 1e-9 * abs(s["null_ll"]) and np.allclose(honest["se"], s["se"], rtol=1e-8)
    t, x, e = survival_fixture(R.EXPONENTIAL, 1.0, 0.2, 1.0, 200)
    f = R.fit(R.EXPONENTIAL, t, x, e)
    assert f["scale"] == 1.0 and f["n_params"] == 2 and len(f["se"]) == 2


def test_information_times_vcov_is_identity():
    for dist in (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC):
        t, x, e = survival_fixture(dist, 1.5, 0.35, 0.6, 400, 0.3)
        f = R.fit(dist, t, x, e)
        assert f["status"] == 0 and np.all(np.diag(f["information"]) > 0)
        assert np.max(np.abs(f["information"] @ f["vcov"] - np.eye(3))) <= 1e-8
        assert np.allclose(f["se"], np.sqrt(np.diag(f["vcov"])), rtol=0, atol=0) and abs(f["vcov"][0, 1]) > 1e-12
        assert np.max(np.abs(f["score"])) <= 1e-12 * max(1.0, np.max(np.abs(np.column_stack([np.ones(400), x]).T @ np.log(t))))


def test_row_rules_and_statuses():
    t, x, e = survival_fixture(R.WEIBULL, 1.5, 0.35, 0.6, 100)
    clean = R.fit(R.WEIBULL, t, x, e)
    # rows that are not finite are dropped: a NaN time, an infinite x, a NaN event
    t2, x2, e2 = np.append(t, [np.nan, 2.0, 3.0]), np.vstack([x, [[1.0], [np.inf], [1.0]]]), np.append(e, [1.0, 1.0, np.nan])
    dropped = R.fit(R.WEIBULL, t2, x2, e2)
    assert dropped["n_obs"] == 100 and np.array_equal(dropped["theta"], clean["theta"])
    # a bad value in a row that is not otherwise finite does not count
    assert R.fit(R.WEIBULL, np.append(t, -1.0), np.vstack([x, [[np.nan]]]), np.append(e, 1.0))["status"] == 0
    bad_t = t.copy()
    bad_t[2] = 0.0
    assert R.fit(R.WEIBULL, bad_t, x, e)["status"] == 1
    bad_e = e.copy()
    bad_e[2] = 2.0
    assert R.fit(R.WEIBULL, t, x, bad_e)["status"] == 1
    assert R.fit(R.WEIBULL, t, x, np.zeros(100))["status"] == 1                      # every row censored
    assert R.fit(R.WEIBULL, np.full(5, np.nan), x[:5], e[:5])["status"] == 10
    assert R.fit(R.WEIBULL, t[:3], x[:3], e[:3])["status"] == 6 and R.fit(R.WEIBULL, t[:4], x[:4], e[:4])["status"] != 6
    assert R.fit(R.EXPONENTIAL, t[:2], x[:2], e[:2])["status"] == 6 and R.fit(R.WEIBULL, t[:4], x[:4], e[:4], fit_intercept=False)["status"] != 6
    # the order: a bad value comes before "no valid row" and before "every row censored"
    assert R.fit(R.WEIBULL, np.array([-1.0, np.nan]), x[:2], np.zeros(2))["status"] == 1
    assert math.isnan(R.fit(R.WEIBULL, t, x, e, fit_intercept=False)["null_ll"])


def test_generated_groups_are_inside_the_condition():
    """The cap of the GPU tier is a condition on the inputs: at least 90 % of the generated groups that the restatement fits have
    max|z| <= 8 and k kappa 2^-53 <= 1e-10.  Asserted on the restatement alone."""
    refs = [r for c in AC.calls() for r in AC.reference(AC.make_call(*c))]
    fitted = [r for r in refs if r["status"] == 0]
    inside = sum(AC.compared(r) for r in fitted)
    print("%d groups, %d fitted, %d inside the condition (%.1f %%)" % (len(refs), len(fitted), inside, 100.0 * inside / len(fitted)))
    assert inside >= 0.9 * len(fitted)
    for c in AC.calls():   # every status kind is what it is meant to be
        call = AC.make_call(*c)
        for kind, ref in zip(call["kinds"], AC.reference(call)):
            assert kind not in AC.EXPECTED_STATUS or ref["status"] == AC.EXPECTED_STATUS[kind], (c, kind)
