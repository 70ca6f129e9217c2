"""A row-based restatement of the rank test contract ("Rank-based location tests") for the tests, in numpy and
scipy.stats' distribution functions; it does not import the package.  R's wilcox.test(exact = FALSE) and kruskal.test in closed
form, with midranks of its own from a stable sort.  Also the shapes and the known answers the CPU and GPU tiers share."""
import numpy as np
from scipy import stats as sps

MANN_WHITNEY, WILCOXON, KRUSKAL_WALLIS = 0, 1, 2
TESTS = {"mann_whitney": MANN_WHITNEY, "wilcoxon": WILCOXON, "kruskal_wallis": KRUSKAL_WALLIS}
TWO_SIDED, LESS, GREATER = 0, 1, 2
NAN = float("nan")


def midranks(v):
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    s = v[order]
    out = np.empty(len(v))
    i = 0
    while i < len(s):
        e = i + 1
        while e < len(s) and s[e] == s[i]:
            e += 1
        out[order[i:e]] = (i + e + 1) / 2.0
        i = e
    return out


def tie_sum(v):
    """sum(t^3 - t) over the runs of equal values, as a Python integer, and the number of distinct values"""
    _, counts = np.unique(v, return_counts=True)
    return sum(int(c) ** 3 - int(c) for c in counts), len(counts)


def _z_p(z, alt):
    if np.isnan(z):
        return NAN
    if alt == TWO_SIDED:
        return float(2.0 * min(sps.norm.cdf(z), sps.norm.sf(z)))
    return float(sps.norm.cdf(z) if alt == LESS else sps.norm.sf(z))


def _correction(num, alt, on):
    if not on:
        return 0.0
    if alt == TWO_SIDED:
        return 0.5 * float(np.sign(num))
    return 0.5 if alt == GREATER else -0.5


def _z(num, var, alt, on):
    return (num - _correction(num, alt, on)) / np.sqrt(var) if var > 0 else NAN


def record(test, v, y=None, sample=None, alternative=TWO_SIDED, correction=True, mu=0.0):
    """The 8 doubles of one group: {statistic, z, p_value, df, n, n1, n2, status}."""
    v = np.asarray(v, np.float64)
    if test == WILCOXON:
        with np.errstate(invalid="ignore"):
            d = v - np.asarray(y, np.float64) - mu
        d = d[~np.isnan(d)]
        valid = len(d)
        d = d[d != 0.0]
        m = len(d)
        if valid < 2:
            return [NAN, NAN, NAN, NAN, float(valid), float(m), float(valid - m), 6.0]
        r = midranks(np.abs(d))
        stat = float(r[d > 0].sum())
        ties, _ = tie_sum(np.abs(d))
        var = m * (m + 1) * (2 * m + 1) / 24.0 - ties / 48.0 if m > 0 else 0.0
        z = _z(stat - m * (m + 1) / 4.0, var, alternative, correction)
        return [stat, z, _z_p(z, alternative), NAN, float(valid), float(m), float(valid - m), 0.0]
    sample = np.asarray(sample, np.int64)
    keep = ~np.isnan(v)
    v, sample = v[keep], sample[keep]
    n = len(v)
    if test == MANN_WHITNEY:
        first = sample == 0
        n1, n2 = int(first.sum()), int(n - first.sum())
        if n1 < 1 or n2 < 1:
            return [NAN, NAN, NAN, NAN, float(n), float(n1), float(n2), 6.0]
        pooled = np.where(first, v - mu, v)
        r = midranks(pooled)
        stat = float(r[first].sum() - n1 * (n1 + 1) / 2.0)
        ties, distinct = tie_sum(pooled)
        var = n1 * n2 / 12.0 * ((n + 1.0) - ties / (n * (n - 1.0))) if distinct > 1 else 0.0
        z = _z(stat - n1 * n2 / 2.0, var, alternative, correction)
        return [stat, z, _z_p(z, alternative), NAN, float(n), float(n1), float(n2), 0.0]
    ids = np.unique(sample)
    k = len(ids)
    if n < 3 or k < 2:
        return [NAN, NAN, NAN, NAN, float(n), float(k), NAN, 6.0]
    ties, distinct = tie_sum(v)
    if distinct < 2:
        return [NAN, NAN, NAN, float(k - 1), float(n), float(k), NAN, 0.0]
    r = midranks(v)
    s = sum(float(r[sample == j].sum()) ** 2 / float((sample == j).sum()) for j in ids)
    h = (12.0 / (n * (n + 1.0)) * s - 3.0 * (n + 1.0)) / (1.0 - ties / (float(n) ** 3 - n))
    return [h, NAN, float(sps.chi2.sf(h, k - 1)), float(k - 1), float(n), float(k), NAN, 0.0]


# ---- the reference's SQL tables (test/sql/hypothesis_tests/test_{mann_whitney,wilcoxon,kruskal_wallis}_agg.test) ----
# Mann-Whitney and Kruskal-Wallis: (values, sample ids); Wilcoxon: (x, y).  grouped_A / grouped_B: the keys of the GROUP BY table.
TABLES = {
    MANN_WHITNEY: {
        "two_groups": ([5.0, 4.0, 5.0, 3.0, 4.0, 5.0, 4.0, 5.0, 3.0, 2.0, 3.0, 4.0, 2.0, 3.0, 2.0, 3.0], [0] * 8 + [1] * 8),
        "no_diff": ([5.0, 4.0, 5.0, 3.0, 4.0, 5.1, 4.1, 4.9, 3.1, 4.1], [0] * 5 + [1] * 5),
        "grouped_A": ([10.0, 12.0, 11.0, 13.0, 5.0, 6.0, 4.0, 7.0], [0] * 4 + [1] * 4),
        "grouped_B": ([5.0, 6.0, 5.5, 6.5, 5.1, 6.1, 5.6, 6.6], [0] * 4 + [1] * 4),
        "tied_data": ([1.0, 2.0, 2.0, 3.0, 3.0, 4.0, 4.0, 5.0], [0] * 4 + [1] * 4),
        "insufficient": ([10.0, 20.0], [0, 1]),
        "same_group": ([10.0, 11.0, 12.0, 13.0], [0, 0, 0, 0]),
    },
    WILCOXON: {
        "paired_data": ([68.5, 72.3, 69.1, 71.8, 67.2, 73.5, 70.2, 68.9], [70.2, 74.5, 71.3, 73.9, 69.4, 75.8, 72.1, 71.2]),
        "no_diff": ([10.0, 11.0, 10.5, 10.8, 10.2, 10.9, 10.4, 10.6], [10.1, 10.9, 10.6, 10.7, 10.3, 10.8, 10.5, 10.5]),
        "grouped_A": ([10.0, 11.0, 10.5, 10.8, 12.0, 13.0, 11.5, 11.8], [15.0, 16.0, 15.5, 15.8, 17.0, 18.0, 16.5, 16.8]),
        "grouped_B": ([10.0, 11.0, 10.5, 10.8, 12.0, 13.0, 11.5, 11.8], [10.1, 10.9, 10.6, 10.7, 12.1, 12.9, 11.6, 11.7]),
        "tied_data": ([1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 4.0, 4.0], [2.0, 2.0, 3.0, 3.0, 4.0, 4.0, 5.0, 5.0]),
        "zero_diff": ([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], [2.0, 3.0, 3.0, 4.0, 6.0, 7.0, 7.0, 8.0]),
    },
    KRUSKAL_WALLIS: {
        "three_groups": ([5.2, 4.8, 5.1, 4.9, 5.0, 3.1, 3.3, 3.0, 3.2, 3.4, 4.1, 4.3, 4.0, 4.2, 4.4], [0] * 5 + [1] * 5 + [2] * 5),
        "no_diff": ([4.0, 5.0, 4.5, 4.8, 4.1, 5.1, 4.6, 4.9, 4.0, 4.9, 4.4, 4.7], [0] * 4 + [1] * 4 + [2] * 4),
        "four_groups": ([10.0, 12.0, 11.0, 20.0, 22.0, 21.0, 15.0, 17.0, 16.0, 25.0, 27.0, 26.0], [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3),
        "grouped_A": ([10.0, 12.0, 11.0, 20.0, 22.0, 21.0, 15.0, 17.0, 16.0], [0] * 3 + [1] * 3 + [2] * 3),
        "grouped_B": ([5.0, 6.0, 5.5, 5.1, 6.1, 5.6, 5.0, 6.0, 5.5], [0] * 3 + [1] * 3 + [2] * 3),
        "tied_data": ([1.0, 2.0, 2.0, 3.0, 3.0, 4.0, 4.0, 5.0, 5.0, 6.0, 6.0, 7.0], [0] * 4 + [1] * 4 + [2] * 4),
        "single_group": ([10.0, 11.0, 12.0, 13.0], [0, 0, 0, 0]),
    },
}


def restated(test, table, **kw):
    """The restatement's answer for check_known_answers: a dict of the record's fields, or None where the status is not 0."""
    a, b = TABLES[test][table]
    rec = record(test, a, y=b, sample=b, **kw) if test == WILCOXON else record(test, a, sample=b, **kw)
    return as_row(rec)


def as_row(rec):
    if rec[7] != 0:
        return None
    return dict(zip(("statistic", "z", "p_value", "df", "n", "n1", "n2"), (float(t) for t in rec[:7])))


def check_known_answers(get):
    """get(test, table name, alternative=..., correction=...) -> the fields of the group's record as a dict (statistic, p_value,
    df, n, n1, n2), or None for a NULL: the statements of the reference's SQL tests, but the two about ci_lower / ci_upper."""
    M, W, K = MANN_WHITNEY, WILCOXON, KRUSKAL_WALLIS
    r = get(M, "two_groups")
    assert r["p_value"] < 0.05 and r["n1"] == 8 and r["n2"] == 8 and not np.isnan(r["statistic"])
    assert get(M, "no_diff")["p_value"] > 0.05
    assert get(M, "two_groups", alternative=LESS)["p_value"] > 0.9
    assert get(M, "two_groups", alternative=GREATER)["p_value"] < 0.05
    for on in (True, False):
        assert not np.isnan(get(M, "two_groups", correction=on)["p_value"])
    assert get(M, "grouped_A")["p_value"] < 0.05 and not get(M, "grouped_B")["p_value"] < 0.05
    assert not np.isnan(get(M, "tied_data")["statistic"]) and not np.isnan(get(M, "insufficient")["statistic"])
    assert get(M, "same_group") is None          # one sample only: NULL

    r = get(W, "paired_data")
    assert r["p_value"] < 0.05 and r["n"] == 8 and not np.isnan(r["statistic"])
    assert get(W, "no_diff")["p_value"] > 0.05
    assert get(W, "paired_data", alternative=LESS)["p_value"] < 0.05
    assert get(W, "paired_data", alternative=GREATER)["p_value"] > 0.9
    assert get(W, "grouped_A")["p_value"] < 0.05 and not get(W, "grouped_B")["p_value"] < 0.05
    assert not np.isnan(get(W, "tied_data")["statistic"]) and not np.isnan(get(W, "zero_diff")["statistic"])

    r = get(K, "three_groups")
    assert r["p_value"] < 0.05 and r["statistic"] > 5 and r["df"] == 2 and r["n"] == 15
    assert get(K, "no_diff")["p_value"] > 0.05
    assert get(K, "four_groups")["df"] == 3
    assert get(K, "grouped_A")["p_value"] < 0.05 and not get(K, "grouped_B")["p_value"] < 0.05
    assert not np.isnan(get(K, "tied_data")["statistic"])
    assert get(K, "single_group") is None        # one sample only: NULL


# ---- the shapes of the issue: groups of these many VALID rows in one call, for every content ----
SIZES = (0, 1, 2, 3, 4, 63, 64, 65, 129, 300)
_COMMON = ("noise", "nan_rows", "ties", "all_equal")
CONTENTS = {
    MANN_WHITNEY: _COMMON + ("one_sample", "shift"),
    WILCOXON: _COMMON + ("some_zero", "all_zero", "shift"),
    KRUSKAL_WALLIS: _COMMON + ("one_sample", "k2", "k3", "k7"),
}
CASES = [(name, content) for name, t in TESTS.items() for content in CONTENTS[t]]
_IDS = (-5, 3, 1000000, 0, -2147483648, 2147483647, 7)   # Kruskal-Wallis' ids of k2, k3, k7: sparse, negative, unsorted


def _sample_ids(rng, test, content, n):
    if content == "one_sample":
        return np.full(n, 0 if test == MANN_WHITNEY else 42, np.int32)
    if test == MANN_WHITNEY:
        return rng.choice(np.array([0, 0, 1, -3], np.int32), n)    # every id but 0 is the second sample
    if content in ("k2", "k3", "k7"):
        pool = np.array(_IDS[:int(content[1:])], np.int32)
        s = rng.choice(pool[:-1], n)
        if n:
            s[rng.integers(n)] = pool[-1]                        # one sample with a single row
        return s
    return rng.choice(np.array([2, 0, 1], np.int32), n)


def make_call(test, content, seed=0):
    """-> dict(off, v, y, sample, mu): one group per size of SIZES, the group's valid rows as many as its size."""
    rng = np.random.default_rng(1000 * seed + 100 * test + CONTENTS[test].index(content))
    vs, ys, ss, off = [], [], [], [0]
    mu = 0.0
    for n in SIZES:
        v = rng.standard_normal(n)
        y = 0.3 + rng.standard_normal(n)
        s = _sample_ids(rng, test, content, n)
        if content == "ties":
            v, y = rng.integers(0, 12, n).astype(np.float64), rng.integers(0, 12, n).astype(np.float64)
        elif content == "all_equal":
            v, y = np.full(n, 2.5), np.full(n, 1.0)
        elif content == "some_zero":
            v, y = rng.integers(0, 4, n).astype(np.float64), rng.integers(0, 4, n).astype(np.float64)
        elif content == "all_zero":
            y = v.copy()
        elif content == "shift":      # quarter-valued data: the shifted differences tie and vanish now and then
            mu = 0.75
            v, y = rng.integers(0, 24, n) / 4.0, rng.integers(0, 24, n) / 4.0
        if content == "nan_rows":     # NaN rows scattered in: the valid rows stay n
            extra = n // 3 + 2
            total = n + extra
            mask = np.zeros(total, bool)
            mask[rng.permutation(total)[:extra]] = True
            fv, fy, fs = np.empty(total), np.empty(total), np.empty(total, np.int32)
            fv[~mask], fy[~mask], fs[~mask] = v, y, s
            fv[mask], fy[mask], fs[mask] = rng.standard_normal(extra), rng.standard_normal(extra), rng.integers(0, 3, extra)
            for j, i in enumerate(np.flatnonzero(mask)):
                if test != WILCOXON or j % 3 != 1:
                    fv[i] = NAN
                if j % 3 != 0:
                    fy[i] = NAN
            v, y, s = fv, fy, fs
        vs.append(v)
        ys.append(y)
        ss.append(s)
        off.append(off[-1] + len(v))
    return dict(off=np.array(off, np.int64), v=np.concatenate(vs), y=np.concatenate(ys), sample=np.concatenate(ss).astype(np.int32), mu=mu)


def reference(test, call, **kw):
    off = call["off"]
    kw.setdefault("mu", call["mu"])
    return np.array([record(test, call["v"][off[g]:off[g + 1]], y=call["y"][off[g]:off[g + 1]], sample=call["sample"][off[g]:off[g + 1]], **kw)
                     for g in range(len(off) - 1)], np.float64)


def check_records(test, got, ref, errs=None):
    """The issue's bounds: the counts and status exactly; W and V bit-equal; z within 1e-9 relative; H within max(1e-9 relative,
    1e-12 (N + 1) absolute: the cancellation of two terms of size 3 (N + 1)); p-values within 1e-9 relative where p > 1e-300.
    NaN where the restatement has NaN."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 8), np.asarray(ref, np.float64).reshape(-1, 8)
    assert got.shape == ref.shape
    errs = {} if errs is None else errs
    for g in range(len(ref)):
        a, b = got[g], ref[g]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (g, a, b)
        assert a[7] == b[7], (g, a, b)
        for j in (4, 5, 6, 3):      # the counts and df
            assert a[j] == b[j] or (np.isnan(a[j]) and np.isnan(b[j])), (g, j, a, b)
        if b[7] != 0:
            continue
        if test != KRUSKAL_WALLIS:
            assert a[0] == b[0], (g, a, b)
            if not np.isnan(b[1]):
                e = abs(a[1] - b[1]) / abs(b[1]) if b[1] != 0.0 else abs(a[1])
                errs["z"] = max(errs.get("z", 0.0), e)
                assert e <= 1e-9, (g, a, b)
        elif not np.isnan(b[0]):
            e = abs(a[0] - b[0])
            errs["H"] = max(errs.get("H", 0.0), e)
            assert e <= max(1e-9 * abs(b[0]), 1e-12 * (b[4] + 1.0)), (g, a, b)
        if np.isnan(b[2]):
            continue
        if b[2] > 1e-300:
            e = abs(a[2] - b[2]) / b[2]
            errs["p_value"] = max(errs.get("p_value", 0.0), e)
            assert e <= 1e-9, (g, a, b)
        else:
            assert a[2] <= 1e-299, (g, a, b)
    return errs
