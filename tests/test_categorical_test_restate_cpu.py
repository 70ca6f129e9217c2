"""CPU tier of the categorical tests, first half: tests/categorical_test_restate.py held to scipy.  X2 (with and without Yates'
correction), V, C, McNemar's statistic: ratios of integers, 1e-12 relative; G the same; the chi-square tails 1e-12 relative (the bound
the rank tests hold Kruskal-Wallis' p to); Fisher's p and the conditional odds ratio with its interval: the largest deviation over
the case set is measured and printed, and asserted at ten times the figure docs/PARITY.md records."""
import math
import os

import numpy as np
import pytest
from scipy import stats as sps
from scipy.stats import contingency

import categorical_test_restate as R
from conftest import ROOT

# the largest relative deviations from scipy 1.15 over FISHER_TABLES, three alternatives, levels 0.9 and 0.95 (docs/PARITY.md)
FISHER_P_SEEN = 6.78e-13
FISHER_ODDS_SEEN = 2.23e-10


def _rel(a, b):
    if np.isinf(b) or b == 0.0:
        return 0.0 if a == b else np.inf
    return abs(a - b) / abs(b)


def _tables():
    rng = np.random.default_rng(5)
    out = [np.array([[10, 20], [30, 40]]), np.array([[12, 5], [3, 9]]), np.array([[1, 1], [1, 2]]), np.array([[7, 0], [2, 5]])]
    for r, c, n in ((2, 2, 40), (2, 3, 75), (3, 3, 200), (5, 7, 900), (5, 7, 1463), (2, 2, 5000), (4, 2, 33)):
        for _ in range(4):
            t = rng.multinomial(n, rng.dirichlet(np.ones(r * c) * 2.0)).reshape(r, c)
            if np.all(t.sum(axis=0) > 0) and np.all(t.sum(axis=1) > 0):
                out.append(t)
    return out


def test_chi_square_g_and_the_association_measures_against_scipy():
    worst = {}
    for t in _tables():
        for correction in (False, True):
            rec = R.table_record(R.CHI_SQUARE, t, correction)
            ref = sps.chi2_contingency(t, correction=correction)
            worst["X2"] = max(worst.get("X2", 0.0), _rel(rec[0], ref.statistic))
            worst["p"] = max(worst.get("p", 0.0), _rel(rec[1], ref.pvalue))
            assert rec[2] == ref.dof and rec[11] == 0 and rec[6] == t.sum()
            assert _rel(rec[0], ref.statistic) <= 1e-12 and _rel(rec[1], ref.pvalue) <= 1e-12, (t, correction)
            for j, method in ((3, "cramer"), (9, "pearson")):      # from the uncorrected X2 whatever the correction
                worst[method] = max(worst.get(method, 0.0), _rel(rec[j], contingency.association(t, method=method)))
                assert _rel(rec[j], contingency.association(t, method=method)) <= 1e-12, (t, method)
            if t.shape == (2, 2):
                phi = (t[0, 0] * t[1, 1] - t[0, 1] * t[1, 0]) / math.sqrt(float(np.prod(t.sum(axis=0)) * np.prod(t.sum(axis=1))))
                assert abs(rec[10] - phi) <= 1e-15 and abs(abs(rec[10]) - rec[3]) <= 1e-12
            else:
                assert np.isnan(rec[10])
        rec = R.table_record(R.G_TEST, t, False)
        ref = sps.chi2_contingency(t, lambda_="log-likelihood", correction=False)
        worst["G"] = max(worst.get("G", 0.0), _rel(rec[0], ref.statistic))
        assert _rel(rec[0], ref.statistic) <= 1e-12 and _rel(rec[1], ref.pvalue) <= 1e-12 and rec[2] == ref.dof, t
        assert np.all(np.isnan(rec[[3, 4, 5, 9, 10]]))
    print({k: "%.2e" % v for k, v in worst.items()})


def test_rows_and_tables_give_the_same_record_and_the_codes_are_dense():
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 3, 80) * 10 - 7, rng.integers(0, 4, 80) * 1000
    rec = R.record(R.CHI_SQUARE, a, b)
    assert np.array_equal(rec, R.table_record(R.CHI_SQUARE, R.dense_table(a, b), False), equal_nan=True) and list(rec[6:9]) == [80, 3, 4]
    assert R.record(R.CHI_SQUARE, [1, 1, 2], [5, 5, 5])[11] == 6 and R.record(R.G_TEST, [], [])[11] == 6
    rec = R.record(R.CHI_SQUARE, [R.NULL, 1, 2, 1], [3, R.NULL, 3, 4])
    assert list(rec[6:9]) == [2, 2, 2] and rec[11] == 0


def test_fisher_against_scipy():
    """p for the three alternatives against fisher_exact; the conditional MLE and its interval against odds_ratio(kind=
    'conditional') at the levels 0.9 and 0.95.  The deviations are measured over the whole set, then asserted."""
    names = {R.TWO_SIDED: "two-sided", R.LESS: "less", R.GREATER: "greater"}
    worst_p = worst_odds = 0.0
    where = None
    for cells in R.FISHER_TABLES:
        assert R.tie_free(cells)
        t = np.array(cells).reshape(2, 2)
        fit = contingency.odds_ratio(t, kind="conditional")
        for alt, name in names.items():
            for level in (0.9, 0.95):
                p, mle, lower, upper = R.fisher_values(cells, alt, level)
                worst_p = max(worst_p, _rel(p, sps.fisher_exact(t, alternative=name).pvalue))
                ci = fit.confidence_interval(level, alternative=name)
                for ours, theirs in ((mle, fit.statistic), (lower, ci.low), (upper, ci.high)):
                    if _rel(ours, theirs) > worst_odds:
                        worst_odds, where = _rel(ours, theirs), (cells, name, level, ours, theirs)
    print("Fisher against scipy: p %.3e, conditional odds ratio and interval %.3e at %s" % (worst_p, worst_odds, where))
    assert worst_p <= 10 * FISHER_P_SEEN and worst_odds <= 10 * FISHER_ODDS_SEEN


def test_fisher_edges_follow_r():
    p, mle, lower, upper = R.fisher_values((7, 0, 2, 9), R.TWO_SIDED, 0.95)      # x at the top of the support
    assert mle == np.inf and upper == np.inf and 0 < lower < np.inf
    p, mle, lower, upper = R.fisher_values((0, 5, 4, 3), R.TWO_SIDED, 0.95)      # x at the bottom
    assert mle == 0.0 and lower == 0.0 and 0 < upper < np.inf
    assert R.fisher_values((3, 1, 1, 3), R.LESS, 0.95)[2] == 0.0 and R.fisher_values((3, 1, 1, 3), R.GREATER, 0.95)[3] == np.inf
    assert np.isnan(R.fisher_values((3, 1, 1, 3), R.TWO_SIDED, None)[2])
    # R's tea-tasting example, fisher.test(matrix(c(3, 1, 1, 3), 2)): p = 17/35, odds ratio 6.408309 (uniroot's default tolerance)
    p, mle, lower, upper = R.fisher_values((3, 1, 1, 3), R.TWO_SIDED, 0.95)
    assert abs(p - 17.0 / 35.0) <= 1e-14 and abs(mle - 6.408309) <= 1e-4 and lower < 1.0 < mle < upper
    assert R.record(R.FISHER_EXACT, [2, 3], [0, 1])[11] == 6 and R.record(R.FISHER_EXACT, [0, 1, 5], [1, 1, 0])[6] == 2


def test_mcnemar_against_scipy():
    for cells in R.MCNEMAR_TABLES:
        n00, b, c, n11 = cells
        for correction in (False, True):
            rec = R.mcnemar_record(cells, correction, False)
            assert list(rec[6:9]) == [sum(cells), 2, 2] and rec[9] == b and rec[10] == c and rec[11] == 0
            if b + c == 0:
                assert np.isnan(rec[0]) and np.isnan(rec[1]) and np.isnan(rec[3])
                continue
            stat = (abs(b - c) - correction) ** 2 / (b + c)
            assert _rel(rec[0], stat) <= 1e-12 and _rel(rec[1], sps.chi2.sf(stat, 1)) <= 1e-12 and rec[2] == 1
        rec = R.mcnemar_record(cells, True, True)
        if b + c:
            assert _rel(rec[1], sps.binomtest(min(b, c), b + c, 0.5).pvalue) <= 1e-12 and np.isnan(rec[0]) and np.isnan(rec[2])
    a, b = np.array([0, 0, 5, -3, 0, 2]), np.array([0, 7, 0, 1, R.NULL, 0])
    assert R.cells_of(R.MCNEMAR, a[b != R.NULL], b[b != R.NULL]) == [1, 1, 2, 1]


def test_the_sql_tables():
    fixtures = R.load_tables(os.path.join(ROOT, "tests", "golden", "categorical_tests"))
    R.check_known_answers(fixtures, restated_aggregate)


def restated_aggregate(function, a, b):
    """What the aggregate `function` returns for one group, from the restatement's record (the views of categorical_tests.py)."""
    test = {"chisq_test": R.CHI_SQUARE, "g_test": R.G_TEST, "fisher_exact": R.FISHER_EXACT, "mcnemar": R.MCNEMAR}.get(function, R.CHI_SQUARE)
    rec = R.record(test, a, b, dict(correction=function == "mcnemar"))
    least = {"chisq_test": 1, "cramers_v": 2}.get(function, 4)
    if rec[11] != 0 or rec[6] < least:
        return None
    if function == "fisher_exact":
        return dict(statistic=rec[0], p_value=rec[1], odds_ratio=rec[0], conditional_odds_ratio=rec[3], ci_lower=rec[4], ci_upper=rec[5], n=rec[6])
    if function in ("cramers_v", "contingency_coef", "phi_coefficient"):
        v = rec[{"cramers_v": 3, "contingency_coef": 9, "phi_coefficient": 10}[function]]
        return None if np.isnan(v) else float(v)
    return dict(statistic=rec[0], p_value=rec[1], df=rec[2])


@pytest.mark.parametrize("content", R.CONTENTS)
def test_case_set_statuses(content):
    call = R.make_call(content)
    for test in R.TESTS.values():
        ref = R.reference(test, call)
        assert ref.shape == (len(R.SIZES), 12) and list(ref[:, 6]) == [float(n) for n in R.SIZES] or test == R.FISHER_EXACT
        if content == "constant" and test in (R.CHI_SQUARE, R.G_TEST):
            assert np.all(ref[:, 11] == 6)
        if content == "distinct" and test == R.CHI_SQUARE:
            big = ref[-1]
            assert big[11] == 0 and big[7] == big[8] == 1463 and abs(big[0] - 1463 * 1462) <= 1e-6
