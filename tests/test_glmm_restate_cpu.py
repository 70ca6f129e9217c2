"""The dense restatement of the mixed model (tests/glmm_restate.py) against the fixture values of the reference's SQL test and
against the closed form of a balanced one-way layout without a covariate, where the ANOVA estimator is the REML estimate
whenever it is positive."""
import numpy as np

import glmm_cases as GC
import glmm_restate as R


def fit(name, reml=True, scale=1.0):
    sizes, y, X = GC.fixture_panel(name, scale)
    return R.fit_panel(y, [X[:, 0]], np.repeat(np.arange(len(sizes)), sizes), True, reml)


def test_fixture_values():
    r = fit("sql_panel")
    e = GC.FIXTURES["sql_panel"]["expect"]
    assert round(r["beta"][0], 4) == e["intercept"] and round(r["beta"][1], 4) == e["slope"]
    assert r["n"] == e["n_observations"] and r["n_groups"] == e["n_groups"] and r["icc"] > e["icc_above"]
    assert fit("flat_panel")["icc"] < GC.FIXTURES["flat_panel"]["expect"]["icc_below"]
    d = fit("sql_panel", scale=2.0)
    lo, hi = GC.FIXTURES["doubling"]["var_group_ratio"]
    assert lo <= d["var_group"] / r["var_group"] <= hi and np.allclose(d["beta"], 2.0 * r["beta"], rtol=1e-9)


def test_balanced_one_way_closed_form():
    rng = np.random.default_rng(0)
    J, m = 12, 7
    y = np.repeat(1.5 * rng.normal(size=J), m) + rng.normal(size=J * m)
    levels = np.repeat(np.arange(J), m)
    d = R.Dense(y, np.ones((J * m, 1)), levels, True).fit()
    means = y.reshape(J, m).mean(axis=1)
    msw = np.sum((y.reshape(J, m) - means[:, None]) ** 2) / (J * (m - 1))
    msb = m * np.sum((means - y.mean()) ** 2) / (J - 1)
    assert msb > msw
    assert abs(d["sigma2"] / msw - 1.0) < 1e-7 and abs(d["var_group"] / ((msb - msw) / m) - 1.0) < 1e-7
    assert abs(d["beta"][0] - y.mean()) < 1e-12 and abs(d["se"][0] - np.sqrt(msb / (J * m))) < 1e-8


def test_the_listed_cases_are_well_conditioned():
    worst = 0.0
    for name, call in GC.calls().items():
        for r in GC.reference(name, call):
            assert isinstance(r, dict), (name, r)
            worst = max(worst, r["cond"])
    print("largest condition number of X'V^-1 X over the cases: %.3g; share left out: 0" % worst)
    assert worst <= 1e10
