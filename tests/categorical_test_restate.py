"""A numpy restatement of the categorical tests' contract (DESIGN.md §1 "Categorical tests", csrc/categorical_tests.h), the case set
of the CPU and GPU tiers and the bounds they hold the library to.  The restatement builds the dense table the library does not
build, sums (O - E)^2 / E as scipy does, and restates R's fisher.test (dnhyper over the support, brentq on the log odds); it is held
to scipy in tests/test_categorical_test_restate_cpu.py."""
import csv
import math
import os
from fractions import Fraction

import numpy as np
from scipy import optimize, special
from scipy import stats as sps

CHI_SQUARE, G_TEST, FISHER_EXACT, MCNEMAR = 0, 1, 2, 3
TESTS = {"chisq_test": CHI_SQUARE, "g_test": G_TEST, "fisher_exact": FISHER_EXACT, "mcnemar": MCNEMAR}
RECORD_NAMES = ("statistic", "p_value", "df", "estimate", "ci_lower", "ci_upper", "n", "n_row_levels", "n_col_levels", "aux", "aux2", "status")
NULL = -2 ** 31
I32_MAX = 2 ** 31 - 1
NAN = float("nan")
EPS = 2.0 ** -52
TWO_SIDED, LESS, GREATER = 0, 1, 2
DEFAULTS = dict(alternative=TWO_SIDED, correction=False, exact=False, confidence_level=0.95)


def options(**kw):
    out = dict(DEFAULTS)
    out.update(kw)
    return out


def _failed(n, r, c):
    rec = np.full(12, NAN)
    rec[6:9] = n, r, c
    rec[11] = 6
    return rec


# ---- tests 0 and 1 ----
def dense_table(a, b):
    """The table of the labels that occur, in ascending order of the labels."""
    ra, ia = np.unique(a, return_inverse=True)
    rb, ib = np.unique(b, return_inverse=True)
    t = np.zeros((len(ra), len(rb)), np.int64)
    np.add.at(t, (ia, ib), 1)
    return t


def table_record(test, t, correction):
    t = np.asarray(t, np.int64)
    t = t[t.sum(axis=1) > 0][:, t.sum(axis=0) > 0] if t.size else t.reshape(0, 0)
    r, c = t.shape
    n = int(t.sum())
    if n < 1 or r < 2 or c < 2:
        return _failed(n, r, c)
    o = t.astype(np.float64)
    e = np.outer(t.sum(axis=1), t.sum(axis=0)).astype(np.float64) / n
    df = (r - 1) * (c - 1)
    rec = np.full(12, NAN)
    if test == G_TEST:
        occ = t > 0
        stat = 2.0 * float(np.sum(o[occ] * np.log(o[occ] / e[occ])))
    else:
        x2 = float(np.sum((o - e) ** 2 / e))
        stat = x2
        rec[3] = math.sqrt(x2 / (n * min(r - 1, c - 1)))
        rec[9] = math.sqrt(x2 / (x2 + n))
        if r == 2 and c == 2:
            det = int(t[0, 0]) * int(t[1, 1]) - int(t[0, 1]) * int(t[1, 0])
            rec[10] = det / math.sqrt(float(int(t[0].sum()) * int(t[1].sum()) * int(t[:, 0].sum()) * int(t[:, 1].sum())))
            if correction:
                d = np.abs(o - e)
                stat = float(np.sum((d - np.minimum(0.5, d)) ** 2 / e))
    rec[0], rec[1], rec[2] = stat, sps.chi2.sf(stat, df), df
    rec[6:9] = n, r, c
    rec[11] = 0
    return rec


# ---- Fisher ----
def _support(cells):
    n11, n12, n21, n22 = cells
    m, n2, k = n11 + n12, n21 + n22, n11 + n21
    lo, hi = max(0, k - n2), min(k, m)
    s = np.arange(lo, hi + 1, dtype=np.float64)
    logdc = -(special.gammaln(s + 1) + special.gammaln(m - s + 1) + special.gammaln(k - s + 1) + special.gammaln(n2 - k + s + 1))
    return s, logdc, lo, hi


def _dnhyper(s, logdc, theta):
    d = logdc + theta * s
    d = np.exp(d - d.max())
    return d / d.sum()


def _root(f, rising):
    """theta with f(theta) = 0 for a monotone f, bracketed from 0 by doubling steps."""
    f0 = f(0.0)
    if f0 == 0.0:
        return 0.0
    step = 1.0 if (f0 < 0) == rising else -1.0
    a, b = 0.0, step
    while (f(b) < 0) == (f0 < 0):
        a, step = b, 2.0 * step
        b = a + step
    return optimize.brentq(f, min(a, b), max(a, b), xtol=1e-15, rtol=4 * EPS, maxiter=500)


def fisher_values(cells, alternative=TWO_SIDED, level=0.95):
    """-> (p, conditional MLE, lower, upper) of [[n11, n12], [n21, n22]] as R's fisher.test."""
    s, logdc, lo, hi = _support(cells)
    x = cells[0]
    d = _dnhyper(s, logdc, 0.0)
    if alternative == LESS:
        p = d[s <= x].sum()
    elif alternative == GREATER:
        p = d[s >= x].sum()
    else:
        p = d[d <= d[x - lo] * (1.0 + 1e-7)].sum()
    lower_tail = lambda th: _dnhyper(s, logdc, th)[s <= x].sum()   # noqa: E731
    upper_tail = lambda th: _dnhyper(s, logdc, th)[s >= x].sum()   # noqa: E731
    mle = 0.0 if x == lo else np.inf if x == hi else math.exp(_root(lambda th: float(np.sum((s - x) * _dnhyper(s, logdc, th))), True))
    lower = upper = NAN
    if level is not None and level == level:
        alpha = 0.5 * (1.0 - level) if alternative == TWO_SIDED else 1.0 - level
        lower = 0.0 if alternative == LESS or x == lo else math.exp(_root(lambda th: upper_tail(th) - alpha, True))
        upper = np.inf if alternative == GREATER or x == hi else math.exp(_root(lambda th: lower_tail(th) - alpha, False))
    return min(p, 1.0), mle, lower, upper


def fisher_record(cells, alternative, level):
    n11, n12, n21, n22 = (int(v) for v in cells)
    n = n11 + n12 + n21 + n22
    if n < 1:
        return _failed(0, 2, 2)
    p, mle, lower, upper = fisher_values((n11, n12, n21, n22), alternative, level)
    with np.errstate(divide="ignore", invalid="ignore"):
        sample = np.float64(n11 * n22) / np.float64(n12 * n21)
    return np.array([sample, p, NAN, mle, lower, upper, n, 2, 2, NAN, NAN, 0], np.float64)


def tie_free(cells):
    """No support point's probability lies in (1 + 1e-14, 1 + 1e-7] times the observed one, in exact arithmetic: scipy, which cuts
    ties at 1e-14 relative, and this project, which cuts at 1e-7, then sum the same points."""
    n11, n12, n21, n22 = (int(v) for v in cells)
    m, n2, k = n11 + n12, n21 + n22, n11 + n21
    at = lambda j: math.comb(m, j) * math.comb(n2, k - j)   # noqa: E731
    w = at(n11)
    lo_cut, hi_cut = 1 + Fraction(1, 10 ** 14), 1 + Fraction(1, 10 ** 7)
    return all(not (lo_cut < Fraction(at(j), w) <= hi_cut) for j in range(max(0, k - n2), min(k, m) + 1))


# ---- McNemar ----
def mcnemar_record(cells, correction, exact):
    n00, b, c, n11 = (int(v) for v in cells)
    n = n00 + b + c + n11
    if n < 1:
        return _failed(0, 2, 2)
    stat = p = NAN
    if b + c > 0 and exact:
        p = min(1.0, 2.0 * sps.binom.cdf(min(b, c), b + c, 0.5))
    elif b + c > 0:
        num = abs(b - c) - (1.0 if correction else 0.0)
        stat = num * num / (b + c)
        p = sps.chi2.sf(stat, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float64(b) / np.float64(c)
    return np.array([stat, p, NAN if exact else 1.0, ratio, NAN, NAN, n, 2, 2, b, c, 0], np.float64)


def cells_of(test, a, b):
    """The four cells the 2 x 2 tests count among the valid rows."""
    if test == FISHER_EXACT:
        keep = ((a == 0) | (a == 1)) & ((b == 0) | (b == 1))
        a, b = a[keep], b[keep]
    else:
        a, b = (a != 0).astype(np.int64), (b != 0).astype(np.int64)
    return [int(np.sum((a == i) & (b == j))) for i in (0, 1) for j in (0, 1)]


def record(test, a, b, opts=None):
    """The record of one group of int32 label pairs (NULL marks a row that is not valid)."""
    o = options(**(opts or {}))
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    valid = (a != NULL) & (b != NULL)
    a, b = a[valid], b[valid]
    if test in (CHI_SQUARE, G_TEST):
        return table_record(test, dense_table(a, b), o["correction"]) if len(a) else _failed(0, 0, 0)
    cells = cells_of(test, a, b)
    if test == FISHER_EXACT:
        return fisher_record(cells, o["alternative"], o["confidence_level"])
    return mcnemar_record(cells, o["correction"], o["exact"])


def reference(test, call):
    off = call["off"]
    return np.array([record(test, call["a"][off[g]:off[g + 1]], call["b"][off[g]:off[g + 1]], call.get("opts")) for g in range(len(off) - 1)],
                    np.float64).reshape(-1, 12)


def as_row(rec):
    return None if rec[11] != 0 else dict(zip(RECORD_NAMES, rec))


# ---- the case set ----
SIZES = (0, 1, 3, 4, 63, 64, 65, 255, 256, 257, 1462, 1463)
CONTENTS = ("2x2", "2x3", "5x7", "distinct", "constant", "extreme", "sentinel")
EXTREME = np.array([NULL + 1, -7, 0, 1, I32_MAX], np.int64)


def make_group(content, n, seed=0):
    """One group with n VALID rows of the content -> (a, b) as int32."""
    rng = np.random.default_rng(100003 * seed + 1009 * CONTENTS.index(content) + n)
    if content == "distinct":                    # n occupied cells with O = 1
        a, b = rng.permutation(n) - n // 2, rng.permutation(n) * 3 - 5
    elif content == "constant":                  # one level on the column side: status 6 for the chi-square and the G-test
        a, b = rng.integers(0, 3, n), np.full(n, 1)
    elif content == "extreme":
        a, b = EXTREME[rng.integers(0, 5, n)], EXTREME[rng.integers(0, 5, n)]
    else:
        r, c = {"2x2": (2, 2), "2x3": (2, 3), "5x7": (5, 7), "sentinel": (2, 2)}[content]
        a = rng.integers(0, r, n)
        b = (a + rng.integers(0, c, n) * (rng.random(n) < 0.7)) % c      # associated, not independent
        if content == "sentinel":                # NULL rows scattered, the first and the last row among them
            extra = n // 3 + 2
            keep = np.ones(n + extra, bool)
            keep[[0, n + extra - 1]] = False
            keep[1 + rng.permutation(n + extra - 2)[:extra - 2]] = False
            fa, fb = np.full(n + extra, NULL), np.full(n + extra, NULL)
            fa[keep], fb[keep] = a, b
            half = ~keep & (rng.random(n + extra) < 0.5)   # a NULL on one side only is as good as on both
            fa[half] = 1
            a, b = fa, fb
    return np.asarray(a, np.int32), np.asarray(b, np.int32)


def make_call(content, sizes=SIZES, seed=0, opts=None):
    """-> dict(off, a, b, opts): one group per size, the group's valid rows as many as its size."""
    groups = [make_group(content, n, seed) for n in sizes]
    cat = lambda k: np.concatenate([g[k] for g in groups]) if groups else np.zeros(0, np.int32)   # noqa: E731
    return dict(off=np.concatenate([[0], np.cumsum([len(g[0]) for g in groups])]).astype(np.int64), a=cat(0), b=cat(1), opts=dict(opts or {}))


def rows_of_cells(cells, seed=0):
    """Label pairs in {0, 1} whose table is [[n11, n12], [n21, n22]], shuffled."""
    a = np.repeat([0, 0, 1, 1], cells)
    b = np.repeat([0, 1, 0, 1], cells)
    perm = np.random.default_rng(seed).permutation(len(a))
    return np.asarray(a[perm], np.int32), np.asarray(b[perm], np.int32)


def cells_call(tables, opts=None):
    """One group per 2 x 2 table."""
    groups = [rows_of_cells(t, i) for i, t in enumerate(tables)]
    return dict(off=np.concatenate([[0], np.cumsum([len(g[0]) for g in groups])]).astype(np.int64),
                a=np.concatenate([g[0] for g in groups]), b=np.concatenate([g[1] for g in groups]), opts=dict(opts or {}))


# Fisher: margins of 1000 with the observed cell at both ends of the support and in the middle, a zero cell, small and lopsided tables
FISHER_TABLES = ((3, 1, 1, 3), (10, 2, 3, 15), (8, 2, 1, 6), (0, 5, 4, 3), (7, 0, 2, 9), (1, 9, 11, 3), (2, 3, 4, 1), (12, 5, 7, 9),
                 (500, 500, 500, 500), (480, 520, 520, 480), (1000, 0, 0, 1000), (0, 1000, 1000, 0), (30, 970, 5, 995), (100, 1, 2, 300))
MCNEMAR_TABLES = ((5, 0, 0, 7), (4, 6, 6, 3), (10, 15, 4, 20), (3, 1, 9, 2), (0, 25, 3, 0), (100, 41, 17, 80), (1, 1, 0, 1))
assert all(tie_free(t) for t in FISHER_TABLES)      # scipy alone defines the expected two-sided p


# ---- the bounds of the host program and of the GPU against this file ----
def p_bound(a, x):
    """The relative bound of a chi-square tail Q(a, x): 1e-9, the bound of Kruskal-Wallis' p, plus what rounding the exponent
    a ln x - x - lgamma(a) of its prefactor costs, eight roundings of its three terms (material from df of about 1e5 on)."""
    return 1e-9 + 8 * EPS * (a * abs(math.log(x)) + x + abs(math.lgamma(a))) if x > 0 else 1e-9


def check_records(test, got, ref, errs=None):
    """Counts, statuses, df and the NaN / infinity pattern exactly.  X2, McNemar's statistic and the sample odds ratio within 1e-12
    max(1, |ref|) (ratios of integers, a few roundings each); V, C and phi within 1e-12 absolute; G within 8 eps n ln n + 1e-12 |G|
    (every term O ln(O/E) carries a few roundings of a term of size at most O ln n); chi-square tails within p_bound relative where
    p > 1e-300; Fisher's and the binomial p, the conditional odds ratio and the interval ends within 1e-9 relative."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(ref, np.float64).reshape(-1, 12)
    assert got.shape == ref.shape
    errs = {} if errs is None else errs

    def near(name, a, b, bound, scale):
        if np.isnan(b):
            return
        e = abs(a - b) / scale if np.isfinite(b) else (0.0 if a == b else np.inf)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e <= bound, (name, a, b, e, bound)

    for g in range(len(ref)):
        a, b = got[g], ref[g]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (g, a, b)
        assert np.array_equal(a[[6, 7, 8, 11]], b[[6, 7, 8, 11]]), (g, a, b)
        if b[11] != 0:
            continue
        assert a[2] == b[2] or (np.isnan(a[2]) and np.isnan(b[2])), (g, a, b)
        n = b[6]
        if test == G_TEST:
            near("G", a[0], b[0], 1.0, 8 * EPS * n * math.log(max(n, 2.0)) + 1e-12 * abs(b[0]))
        else:
            near("statistic", a[0], b[0], 1e-12, max(1.0, abs(b[0])))
        if test == CHI_SQUARE:
            for j, name in ((3, "V"), (9, "C"), (10, "phi")):
                near(name, a[j], b[j], 1e-12, 1.0)
        elif test == FISHER_EXACT:
            for j, name in ((3, "mle"), (4, "ci_lower"), (5, "ci_upper")):
                near(name, a[j], b[j], 1e-9, max(abs(b[j]), 1e-300))
        elif test == MCNEMAR:
            near("estimate", a[3], b[3], 1e-15, max(abs(b[3]), 1e-300))
            assert a[9] == b[9] and a[10] == b[10], (g, a, b)
        if np.isnan(b[1]):
            continue
        tail = test in (CHI_SQUARE, G_TEST) or (test == MCNEMAR and not np.isnan(b[2]))
        bound = p_bound(0.5 * b[2], 0.5 * b[0]) if tail else 1e-9
        if b[1] > 1e-300:
            near("p_value", a[1], b[1], bound, b[1])
        else:
            assert a[1] <= 1e-299, (g, a, b)
    return errs


# ---- the tables of the reference's SQL tests (tests/golden/categorical_tests/*.csv) ----
FIXTURES = ("chisq_test", "fisher_exact", "g_test", "mcnemar", "association")


def load_tables(folder):
    """-> ({file: {(table, group): (a, b)}}, the facts as a list of dicts)"""
    out = {}
    for name in FIXTURES:
        tables = {}
        with open(os.path.join(folder, name + ".csv"), newline="") as f:
            for row in csv.DictReader(f):
                pair = tables.setdefault((row["table"], row["group"]), ([], []))
                pair[0].append(int(row["a"]))
                pair[1].append(int(row["b"]))
        out[name] = {k: (np.array(v[0], np.int32), np.array(v[1], np.int32)) for k, v in tables.items()}
    with open(os.path.join(folder, "facts.csv"), newline="") as f:
        facts = list(csv.DictReader(f))
    return out, facts


def check_known_answers(fixtures, run):
    """Every fact of test/sql/categorical/*.test that the fixtures record.  run(function, a, b) -> what the aggregate returns for
    the rows: a dict with statistic, p_value, df (and for Fisher odds_ratio, conditional_odds_ratio, ci_lower, ci_upper, n), a float
    for the three association measures, None for a NULL.  Which odds ratio the reference's Fisher result reports is not known:
    its facts are held for both."""
    tables, facts = fixtures
    seen = 0
    for fact in facts:
        a, b = tables[fact["file"]][(fact["table"], fact["group"])]
        got = run(fact["function"], a, b)
        assert got is not None, fact
        field, op = fact["field"], fact["op"]
        value = float(fact["value"]) if fact["value"] else None
        names = ("odds_ratio", "conditional_odds_ratio") if field == "odds_ratio" else (field,)
        for name in names:
            v = got if field == "value" else got[name]
            if op == "near":
                assert abs(v - value) < float(fact["tolerance"]), (fact, v)
            elif op == "eq":
                assert v == value, (fact, v)
            elif op in ("gt", "lt"):
                assert (v > value) if op == "gt" else (v < value), (fact, v)
            elif op in ("not_gt", "not_lt"):
                assert not ((v > value) if op == "not_gt" else (v < value)), (fact, v)
            elif op == "abs_lt":
                assert abs(v) < value, (fact, v)
            elif op == "between":
                assert value <= v <= float(fact["tolerance"]), (fact, v)
            elif op == "inside_interval":
                assert got["ci_lower"] < v < got["ci_upper"], (fact, got)
            elif op == "not_null":
                assert v is not None and not (isinstance(v, float) and np.isnan(v)), (fact, v)
            else:
                raise AssertionError("unknown fact " + op)
        seen += 1
    assert seen == len(facts) == 37
