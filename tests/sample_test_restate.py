"""A row-based restatement of the sample test contract ("Parametric and studentised-rank tests") for the tests, in
numpy and scipy.stats' distribution functions; it does not import the package.  R's t.test, oneway.test, the median-centred Levene
test, Yuen's test and brunner.munzel.test in closed form.  Also the shapes and the known answers the CPU and GPU tiers share."""
import numpy as np
from scipy import stats as sps

from rank_test_restate import midranks

T_TEST, YUEN, ANOVA, BROWN_FORSYTHE, BRUNNER_MUNZEL = 0, 1, 2, 3, 4
TESTS = {"t_test": T_TEST, "yuen": YUEN, "anova": ANOVA, "brown_forsythe": BROWN_FORSYTHE, "brunner_munzel": BRUNNER_MUNZEL}
TWO_SIDED, LESS, GREATER = 0, 1, 2
WELCH, STUDENT, PAIRED = 0, 1, 2          # the t-test's kinds
FISHER, WELCH_ANOVA = 0, 1                # ANOVA's kinds
NAN, INF = float("nan"), float("inf")
RECORD_NAMES = ("statistic", "p_value", "df", "df2", "estimate", "ci_lower", "ci_upper", "n", "n1", "n2", "aux", "status")


def _failed(n, n1, n2):
    return [NAN] * 7 + [float(n), float(n1), float(n2), NAN, 6.0]


def _t_p(t, df, alt):
    if np.isnan(t):
        return NAN
    if np.isinf(t):                        # (complete separation: df is NaN there)
        return 0.0 if alt == TWO_SIDED else float((t > 0) != (alt == GREATER))
    if alt == TWO_SIDED:
        return float(2.0 * sps.t.sf(abs(t), df))
    return float(sps.t.cdf(t, df) if alt == LESS else sps.t.sf(t, df))


def _studentised(est, num, se, df, alt, cl, n, n1, n2):
    """The record of t = num / se: R's interval around est (a one-sided alternative leaves its far side open)."""
    if not se > 0:
        return [NAN, NAN, NAN, NAN, est, NAN, NAN, float(n), float(n1), float(n2), se, 0.0]
    t = num / se
    lo = hi = NAN
    if cl is not None and not np.isnan(cl):
        if alt == TWO_SIDED:
            q = float(sps.t.isf(0.5 * (1.0 - cl), df))
            lo, hi = est - q * se, est + q * se
        else:
            q = float(sps.t.isf(1.0 - cl, df))
            lo, hi = (-INF, est + q * se) if alt == LESS else (est - q * se, INF)
    return [t, _t_p(t, df, alt), df, NAN, est, lo, hi, float(n), float(n1), float(n2), se, 0.0]


def _centred(v):
    m = v.mean()
    return m, float(((v - m) ** 2).sum())


def _f_record(arms, n):
    """Fisher's F of the arms (each at least 2 rows): statistic, p, df, df2, SSB, SSW."""
    k = len(arms)
    grand = sum(float(a.sum()) for a in arms) / n
    ssb = sum(len(a) * (a.mean() - grand) ** 2 for a in arms)
    ssw = sum(_centred(a)[1] for a in arms)
    df, df2 = k - 1.0, float(n - k)
    if ssw > 0:
        f = (ssb / df) / (ssw / df2)
        p = float(sps.f.sf(f, df, df2))
    elif ssb > 0:
        f, p = INF, 0.0
    else:
        f = p = NAN
    return f, p, df, df2, float(ssb), float(ssw)


def record(test, v, y=None, sample=None, alternative=TWO_SIDED, kind=0, mu=0.0, trim=0.2, confidence_level=0.95):
    """The 12 doubles of one group: RECORD_NAMES."""
    v = np.asarray(v, np.float64)
    alt, cl = alternative, confidence_level
    if test == T_TEST and kind == PAIRED:
        with np.errstate(invalid="ignore"):
            d = v - np.asarray(y, np.float64)
            d = d[~np.isnan(d - mu)]
        n = len(d)
        if n < 2:
            return _failed(n, n, n)
        m, s = _centred(d)
        return _studentised(m, m - mu, np.sqrt(s / (n - 1.0) / n), n - 1.0, alt, cl, n, n, n)
    sample = np.asarray(sample, np.int64)
    keep = ~np.isnan(v)
    v, sample = v[keep], sample[keep]
    n = len(v)
    if test in (T_TEST, YUEN, BRUNNER_MUNZEL):
        a, b = v[sample == 0], v[sample != 0]
        n1, n2 = len(a), len(b)
    if test == T_TEST:
        if n1 < 2 or n2 < 2:
            return _failed(n, n1, n2)
        (m1, s1), (m2, s2) = _centred(a), _centred(b)
        est = m1 - m2
        if kind == STUDENT:
            df = n1 + n2 - 2.0
            se = np.sqrt((s1 + s2) / df * (1.0 / n1 + 1.0 / n2))
        else:
            e1, e2 = s1 / (n1 - 1.0) / n1, s2 / (n2 - 1.0) / n2
            se = np.sqrt(e1 + e2)
            with np.errstate(invalid="ignore", divide="ignore"):
                df = float((e1 + e2) ** 2 / np.float64(e1 * e1 / (n1 - 1.0) + e2 * e2 / (n2 - 1.0)))
        return _studentised(est, est - mu, se, df, alt, cl, n, n1, n2)
    if test == YUEN:
        g1, g2 = int(np.floor(trim * n1)), int(np.floor(trim * n2))
        h1, h2 = n1 - 2 * g1, n2 - 2 * g2
        if n1 < 4 or n2 < 4 or h1 < 2 or h2 < 2:
            return _failed(n, n1, n2)
        out = []
        for s, g, h in ((np.sort(a), g1, h1), (np.sort(b), g2, h2)):
            w = np.clip(s, s[g], s[len(s) - g - 1])
            out.append((float(s[g:len(s) - g].mean()), _centred(w)[1] / (h * (h - 1.0))))
        (tm1, d1), (tm2, d2) = out
        est, se = tm1 - tm2, np.sqrt(d1 + d2)
        with np.errstate(invalid="ignore", divide="ignore"):
            df = float((d1 + d2) ** 2 / np.float64(d1 * d1 / (h1 - 1.0) + d2 * d2 / (h2 - 1.0)))
        return _studentised(est, est, se, df, alt, cl, n, n1, n2)
    if test == BRUNNER_MUNZEL:
        if n1 < 2 or n2 < 2:
            return _failed(n, n1, n2)
        R = midranks(np.concatenate([a, b]))
        R1, R2, r1, r2 = R[:n1], R[n1:], midranks(a), midranks(b)
        m1, m2 = R1.sum() / n1, R2.sum() / n2
        v1 = float(((R1 - r1 + ((n1 + 1.0) / 2.0 - m1)) ** 2).sum()) / (n1 - 1.0)
        v2 = float(((R2 - r2 + ((n2 + 1.0) / 2.0 - m2)) ** 2).sum()) / (n2 - 1.0)
        phat = float((m2 - (n2 + 1.0) / 2.0) / n1)
        se = float(np.sqrt(v1 / (n1 * float(n2) * n2) + v2 / (n2 * float(n1) * n1)))
        s = n1 * v1 + n2 * v2
        tail = {TWO_SIDED: TWO_SIDED, LESS: GREATER, GREATER: LESS}[alt]    # `greater`: the lower tail of W (scipy, lawstat)
        has_level = cl is not None and not np.isnan(cl)
        if s > 0:
            w = float(n1 * float(n2) * (m2 - m1) / ((n1 + n2) * np.sqrt(s)))
            df = float(s * s / ((n1 * v1) ** 2 / (n1 - 1.0) + (n2 * v2) ** 2 / (n2 - 1.0)))
            q = float(sps.t.isf(0.5 * (1.0 - cl), df)) if has_level else NAN
            lo, hi = phat - q * se, phat + q * se
        else:
            w = INF if phat > 0.5 else (-INF if phat < 0.5 else NAN)
            df = NAN
            lo = hi = phat if has_level else NAN
        return [w, _t_p(w, df, tail), df, NAN, phat, lo, hi, float(n), float(n1), float(n2), se, 0.0]
    ids = np.unique(sample)
    k = len(ids)
    arms = [v[sample == j] for j in ids]
    if k < 2 or min(len(a) for a in arms) < 2:
        return _failed(n, k, NAN)
    if test == BROWN_FORSYTHE:
        arms = [np.abs(a - np.median(a)) for a in arms]
    f, p, df, df2, ssb, ssw = _f_record(arms, n)
    if test == ANOVA and kind == WELCH_ANOVA:          # R's oneway.test(var.equal = FALSE)
        var = [_centred(a)[1] / (len(a) - 1.0) for a in arms]
        if min(var) > 0:
            w = np.array([len(a) / s for a, s in zip(arms, var)])
            means = np.array([a.mean() for a in arms])
            mt = (w * means).sum() / w.sum()
            tmp = sum((1.0 - wj / w.sum()) ** 2 / (len(a) - 1.0) for wj, a in zip(w, arms)) / (k * k - 1.0)
            f = float((w * (means - mt) ** 2).sum() / ((k - 1.0) * (1.0 + 2.0 * (k - 2.0) * tmp)))
            df2 = float(1.0 / (3.0 * tmp))
            p = float(sps.f.sf(f, df, df2))
        else:
            f = df2 = p = NAN
    return [f, p, df, df2, ssb, NAN, NAN, float(n), float(k), NAN, ssw, 0.0]


def as_row(rec):
    """The record's fields as a dict, or None where the status is not 0."""
    if rec[11] != 0:
        return None
    return dict(zip(RECORD_NAMES[:11], (float(t) for t in rec[:11])))


# ---- the tables of the reference's SQL tests: tests/golden/sample_tests/*.csv, rows of (table, value, second column) ----
def load_tables(directory):
    """-> {test name: {table name: (values, sample ids)}}; grouped_A / grouped_B: the keys of the GROUP BY table."""
    import csv
    import os
    out = {}
    for name in TESTS:
        tables = {}
        with open(os.path.join(directory, name + ".csv")) as f:
            for row in csv.DictReader(f):
                a, b = tables.setdefault(row["table"], ([], []))
                a.append(float(row["value"]))
                b.append(int(row["second"]))
        out[name] = tables
    return out


def check_known_answers(tables, get):
    """get(test name, table name, values, sample ids, **options) -> the record's fields as a dict (RECORD_NAMES), or None for a NULL: the
    statements of the reference's SQL tests."""
    def of(name, table, **kw):
        return get(name, table, *tables[name][table], **kw)
    r = of("t_test", "two_groups")
    assert r["p_value"] < 0.001 and r["statistic"] < -10 and (r["n1"], r["n2"]) == (10, 10) and r["ci_upper"] < 0 and 17 < r["df"] < 19
    r = of("t_test", "no_diff")
    assert r["p_value"] > 0.05 and r["ci_lower"] < 0 < r["ci_upper"]
    assert of("t_test", "two_groups", alternative="less")["p_value"] < 0.001
    assert of("t_test", "two_groups", alternative="greater")["p_value"] > 0.99
    width = {cl: (lambda d: d["ci_upper"] - d["ci_lower"])(of("t_test", "two_groups", confidence_level=cl)) for cl in (0.9, 0.95, 0.99)}
    assert width[0.9] < width[0.95] < width[0.99]
    assert of("t_test", "grouped_A")["p_value"] < 0.05 and not of("t_test", "grouped_B")["p_value"] < 0.05
    assert of("t_test", "insufficient") is None and of("t_test", "same_group") is None
    r = of("t_test", "nan_data")
    assert (r["n1"], r["n2"]) == (3, 3)

    r = of("yuen", "yuen_data")
    assert r["p_value"] < 0.001 and (r["n1"], r["n2"]) == (6, 6) and r["ci_upper"] < 0 and not np.isnan(r["df"])
    assert of("yuen", "no_diff")["p_value"] > 0.05
    for trim in (0.1, 0.25):
        assert not np.isnan(of("yuen", "yuen_data", trim=trim)["statistic"])
    assert of("yuen", "grouped_A")["p_value"] < 0.05 and not of("yuen", "grouped_B")["p_value"] < 0.05

    r = of("anova", "three_groups")
    assert r["p_value"] < 0.001 and r["statistic"] > 10 and (r["df"], r["df2"]) == (2, 9) and (r["n1"], r["n"]) == (3, 12)
    assert abs(r["estimate"] + r["aux"] - 215.0) < 1.0                     # SSB + SSW
    assert of("anova", "no_diff")["p_value"] > 0.05 and of("anova", "two_groups")["df"] == 1
    assert of("anova", "grouped_A")["p_value"] < 0.05 and not of("anova", "grouped_B")["p_value"] < 0.05
    assert of("anova", "single_group") is None

    r = of("brown_forsythe", "variance_data")
    assert r["p_value"] < 0.05 and r["df"] == 2 and r["n"] == 24
    assert of("brown_forsythe", "equal_var")["p_value"] > 0.05 and of("brown_forsythe", "two_groups")["df"] == 1
    assert of("brown_forsythe", "grouped_A")["p_value"] > 0.05 and not of("brown_forsythe", "grouped_B")["p_value"] > 0.05

    r = of("brunner_munzel", "bm_data")
    assert r["p_value"] < 0.05 and (r["n1"], r["n2"]) == (12, 11) and 0 <= r["estimate"] <= 1
    assert not any(np.isnan(r[f]) for f in ("statistic", "df", "ci_lower", "ci_upper"))
    assert of("brunner_munzel", "no_diff")["p_value"] > 0.05
    assert of("brunner_munzel", "grouped_A")["p_value"] < 0.05 and not of("brunner_munzel", "grouped_B")["p_value"] < 0.05


# ---- the shapes of the issue: groups of these many VALID rows in one call, for every content ----
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 129, 300)
_COMMON = ("noise", "nan_rows", "ties", "all_equal", "one_sample")
CONTENTS = {
    T_TEST: _COMMON + ("shift", "paired", "paired_nan"),
    YUEN: _COMMON + ("trim0", "trim10", "trim25"),
    ANOVA: _COMMON + ("separated", "k2", "k3", "k7", "sparse_ids"),
    BROWN_FORSYTHE: _COMMON + ("k2", "k3", "k7", "sparse_ids"),
    BRUNNER_MUNZEL: _COMMON + ("separated",),
}
CASES = [(name, content) for name, t in TESTS.items() for content in CONTENTS[t]]
_IDS = (-5, 3, 1000000, 0, -2147483648, 2147483647, 7)   # the k-sample tests' ids of k2, k3, k7: sparse, negative, unsorted
_TWO = (T_TEST, YUEN, BRUNNER_MUNZEL)


def _sample_ids(rng, test, content, n):
    if content == "one_sample":
        return np.full(n, 0 if test in _TWO else 42, np.int32)
    if test in _TWO:
        return rng.choice(np.array([0, 0, 1, -3], np.int32), n)    # every id but 0 is the second sample
    if content == "sparse_ids":                                    # the seven ids, every arm with rows enough at the larger sizes
        return rng.choice(np.array(_IDS, np.int32), n)
    if content in ("k2", "k3", "k7"):
        pool = np.array(_IDS[:int(content[1:])], np.int32)
        s = rng.choice(pool[:-1], n)
        if n:
            s[rng.integers(n)] = pool[-1]                        # one arm with a single row: status 6
        return s
    return rng.choice(np.array([2, 0, 1], np.int32), n)


def make_call(test, content, seed=0):
    """-> dict(off, v, y, sample, opts): one group per size of SIZES, the group's valid rows as many as its size; opts: the
    options the content asks for (kind, mu, trim)."""
    rng = np.random.default_rng(1000 * seed + 100 * test + CONTENTS[test].index(content))
    vs, ys, ss, off = [], [], [], [0]
    opts = {}
    if content.startswith("paired"):
        opts["kind"] = PAIRED
    if content.startswith("trim"):
        opts["trim"] = int(content[4:]) / 100.0
    for n in SIZES:
        s = _sample_ids(rng, test, content, n)
        second = s != 0 if test in _TWO else s == 2
        v = rng.standard_normal(n) + 0.3 * second            # arm means 0 and 0.3, unit variance
        y = 0.3 + rng.standard_normal(n)
        if content == "ties":
            v, y = rng.integers(0, 12, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
        elif content == "all_equal":
            v, y = np.full(n, 2.5), np.full(n, 1.0)
        elif content == "shift":      # quarter-valued data against mu = 0.75
            opts["mu"] = 0.75
            v = rng.integers(0, 24, n) / 4.0
        elif content == "separated":  # arms that do not overlap; ANOVA's are constant, so SSW = 0
            v = 10.0 * s if test == ANOVA else v + 100.0 * second
        if content in ("nan_rows", "paired_nan"):     # NaN rows scattered in: the valid rows stay n
            extra = n // 3 + 2
            total = n + extra
            mask = np.zeros(total, bool)
            mask[rng.permutation(total)[:extra]] = True
            fv, fy, fs = np.empty(total), np.empty(total), np.empty(total, np.int32)
            fv[~mask], fy[~mask], fs[~mask] = v, y, s
            fv[mask], fy[mask], fs[mask] = rng.standard_normal(extra), rng.standard_normal(extra), rng.integers(0, 3, extra)
            for j, i in enumerate(np.flatnonzero(mask)):
                if content == "nan_rows" or j % 3 != 1:
                    fv[i] = NAN
                if j % 3 != 0:
                    fy[i] = NAN
            v, y, s = fv, fy, fs
        vs.append(v)
        ys.append(y)
        ss.append(s)
        off.append(off[-1] + len(v))
    return dict(off=np.array(off, np.int64), v=np.concatenate(vs), y=np.concatenate(ys), sample=np.concatenate(ss).astype(np.int32),
                opts=opts)


def reference(test, call, **kw):
    off = call["off"]
    kw = dict(call.get("opts", {}), **kw)
    return np.array([record(test, call["v"][off[g]:off[g + 1]], y=call["y"][off[g]:off[g + 1]], sample=call["sample"][off[g]:off[g + 1]], **kw)
                     for g in range(len(off) - 1)], np.float64)


def _integer_df(test, kind):
    """Which of (df, df2) are counts, compared exactly."""
    if test == T_TEST:
        return (kind != WELCH, True)
    if test == ANOVA:
        return (True, kind == FISHER)
    return (test == BROWN_FORSYTHE, test == BROWN_FORSYTHE)


def check_records(test, got, ref, kind=0, errs=None):
    """The issue's bounds: the counts, the status and an integer df exactly; the statistic, a non-integer df, the interval's ends
    and the estimate of a two-sample test within 1e-9 max(1, |ref|); p within 1e-9 relative where p > 1e-300; SSB and SSW within
    1e-9 relative; NaN and +-inf exactly where the restatement has them."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 12), np.asarray(ref, np.float64).reshape(-1, 12)
    assert got.shape == ref.shape
    errs = {} if errs is None else errs
    exact_df = _integer_df(test, kind)
    k_sample = test in (ANOVA, BROWN_FORSYTHE)

    def near(name, a, b, relative=False):
        if np.isnan(b) or np.isinf(b):
            return
        e = abs(a - b) / (abs(b) if relative else max(1.0, abs(b))) if b != 0.0 else abs(a)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e <= 1e-9, (name, a, b)

    for g in range(len(ref)):
        a, b = got[g], ref[g]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (g, a, b)
        assert np.array_equal(np.isinf(a), np.isinf(b)) and np.array_equal(a[np.isinf(b)], b[np.isinf(b)]), (g, a, b)
        for j in (7, 8, 9, 11):
            assert a[j] == b[j] or (np.isnan(a[j]) and np.isnan(b[j])), (g, j, a, b)
        if b[11] != 0:
            continue
        near("statistic", a[0], b[0])
        for j, exact in zip((2, 3), exact_df):
            if exact:
                assert a[j] == b[j] or (np.isnan(a[j]) and np.isnan(b[j])), (g, j, a, b)
            else:
                near("df", a[j], b[j])
        near("estimate", a[4], b[4], relative=k_sample)
        near("aux", a[10], b[10], relative=k_sample)
        near("ci", a[5], b[5])
        near("ci", a[6], b[6])
        if np.isnan(b[1]):
            continue
        if b[1] > 1e-300:
            e = abs(a[1] - b[1]) / b[1]
            errs["p_value"] = max(errs.get("p_value", 0.0), e)
            assert e <= 1e-9, (g, a, b)
        else:
            assert a[1] <= 1e-299, (g, a, b)
    return errs
