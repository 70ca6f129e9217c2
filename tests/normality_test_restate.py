"""numpy restatement of csrc/normality_tests.h: the Shapiro-Wilk test (Royston's AS R94 as R's swilk.c and scipy compute it),
D'Agostino's K2 (scipy.stats.normaltest: the D'Agostino 1970 skewness transform and the Anscombe-Glynn kurtosis transform) and the
Jarque-Bera test of one group of rows.  It does not import the package; scipy gives the normal quantile (ndtri) and the normal
tail (norm.sf) only.

    valid row: v not NaN (infinities stay in);  n = the valid rows
    record {statistic, p_value, skewness, kurtosis, z_skewness, z_kurtosis, n, status}; a field a test does not define is NaN
    status 6: too few rows (Shapiro-Wilk n < 3, K2 n < 8, Jarque-Bera n < 3);  status 1: Shapiro-Wilk n > 5000, K2 and
    Jarque-Bera with m2 <= 0;  every field but n and the status is NaN in both.

The case set: every n of SIZES_CPU as each content of CONTENTS.  `offset` is 1e6 + noise in units of 1/1024 whose sum is a
multiple of n: every partial sum of such values is exact in binary64 (33 bits before the point, 10 behind) and so is their mean,
whatever the order of the sum.  With an unrepresentable mean of 5000 values near 1e6 the rounding of the mean (up to 6e-11)
moves the skewness by 3 times as much over sd, and the yardsticks then differ among themselves: scipy.stats.jarque_bera centres
its data a second time, scipy.stats.normaltest does not, and the two disagree by 7e-9 relative on such data, so no one definition
of the moments could be within 1e-12 of both.  The exact mean takes nothing else from the case: the centred values still lose
the bits the offset costs them."""
import csv
import os

import numpy as np
from scipy.special import ndtri
from scipy.stats import norm

NAN = float("nan")
SHAPIRO_WILK, DAGOSTINO_K2, JARQUE_BERA = 0, 1, 2
TESTS = {"shapiro_wilk": SHAPIRO_WILK, "dagostino_k2": DAGOSTINO_K2, "jarque_bera": JARQUE_BERA}
RECORD_NAMES = ("statistic", "p_value", "skewness", "kurtosis", "z_skewness", "z_kurtosis", "n", "status")
STATUS_INVALID_INPUT, STATUS_INSUFFICIENT_DATA = 1, 6
MIN_ROWS = {SHAPIRO_WILK: 3, DAGOSTINO_K2: 8, JARQUE_BERA: 3}
SW_MAX_ROWS = 5000

# Royston (1995), Algorithm AS R94
_C1 = (0.0, 0.221157, -0.147981, -2.07119, 4.434685, -2.706056)
_C2 = (0.0, 0.042981, -0.293762, -1.752461, 5.682633, -3.582633)
_C3 = (0.544, -0.39978, 0.025054, -6.714e-4)
_C4 = (1.3822, -0.77857, 0.062767, -0.0020322)
_C5 = (-1.5861, -0.31082, -0.083751, 0.0038915)
_C6 = (-0.4803, -0.082676, 0.0030302)
_G = (-2.273, 0.459)


def _poly(c, x):
    r = 0.0
    for a in reversed(c):
        r = r * x + a
    return r


def _failed(n, status):
    return [NAN] * 6 + [float(n), float(status)]


def sw_coefficients(n):
    """a_1 .. a_(n // 2) > 0: the coefficient of x_(n + 1 - i) - x_(i)."""
    if n == 3:
        return np.array([np.sqrt(0.5)])
    half = n // 2
    u = -ndtri((np.arange(1, half + 1) - 0.375) / (n + 0.25))       # the upper quantiles, > 0
    summ2 = 2.0 * float(np.sum(u * u))
    ssumm2, rsn = np.sqrt(summ2), 1.0 / np.sqrt(n)
    a = np.empty(half)
    a1 = _poly(_C1, rsn) + u[0] / ssumm2
    if n > 5:
        a2 = u[1] / ssumm2 + _poly(_C2, rsn)
        fac = np.sqrt((summ2 - 2.0 * u[0] ** 2 - 2.0 * u[1] ** 2) / (1.0 - 2.0 * a1 ** 2 - 2.0 * a2 ** 2))
        a[1] = a2
        first = 2
    else:
        fac = np.sqrt((summ2 - 2.0 * u[0] ** 2) / (1.0 - 2.0 * a1 ** 2))
        first = 1
    a[0] = a1
    a[first:] = u[first:] / fac
    return a


def sw_p(w, w1, n):
    """The p-value of W = 1 - w1 at n rows."""
    if n == 3:
        if np.isnan(w):                        # (an infinity among the three rows; max() below would turn the NaN into 0)
            return NAN
        return max(0.0, 6.0 / np.pi * (np.arcsin(np.sqrt(min(w, 1.0))) - np.arcsin(np.sqrt(0.75))))
    if not w1 > 0.0:
        return 1.0 if w1 <= 0.0 else NAN       # (W at or, by rounding, past 1: the limit of the tail)
    y = np.log(w1)
    if n <= 11:
        gamma = _poly(_G, float(n))
        if y >= gamma:
            return 1e-99
        y = -np.log(gamma - y)
        m, s = _poly(_C3, float(n)), np.exp(_poly(_C4, float(n)))
    else:
        xx = np.log(float(n))
        m, s = _poly(_C5, xx), np.exp(_poly(_C6, xx))
    return float(norm.sf((y - m) / s))


def shapiro_wilk(x):
    n = len(x)
    if n < 3:
        return _failed(n, STATUS_INSUFFICIENT_DATA)
    if n > SW_MAX_ROWS:
        return _failed(n, STATUS_INVALID_INPUT)
    y = np.sort(x)
    rng = y[-1] - y[0]
    if rng == 0.0:
        return [1.0, 1.0, NAN, NAN, NAN, NAN, float(n), 0.0]
    with np.errstate(invalid="ignore"):
        xi = (y - y[n // 2]) / rng
        a = sw_coefficients(n)
        half = len(a)
        ssa = 2.0 * float(np.sum(a * a))
        sx = float(np.sum(xi)) / n
        ssx = float(np.sum((xi - sx) ** 2))
        sax = float(np.sum(a * (xi[::-1][:half] - xi[:half])))
        ssassx = np.sqrt(ssa * ssx)
        w1 = (ssassx - sax) * (ssassx + sax) / (ssa * ssx)
        w = 1.0 - w1
        return [w, sw_p(w, w1, n), NAN, NAN, NAN, NAN, float(n), 0.0]


def moments(x):
    """-> (m2, m3, m4), biased, about the mean, in two passes."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - np.sum(x) / len(x)
        d2 = d * d
        return float(np.sum(d2)) / len(x), float(np.sum(d2 * d)) / len(x), float(np.sum(d2 * d2)) / len(x)


def _shape(x):
    m2, m3, m4 = moments(x)
    if m2 <= 0.0:
        return None
    sd = np.sqrt(m2)
    return m3 / (sd * sd * sd), m4 / (m2 * m2) - 3.0


def jarque_bera(x):
    n = len(x)
    if n < 3:
        return _failed(n, STATUS_INSUFFICIENT_DATA)
    sk = _shape(x)
    if sk is None:
        return _failed(n, STATUS_INVALID_INPUT)
    s, k = sk
    with np.errstate(over="ignore", invalid="ignore"):
        jb = n / 6.0 * (s * s + k * k / 4.0)
        return [jb, float(np.exp(-jb / 2.0)), s, k, NAN, NAN, float(n), 0.0]


def skew_z(s, n):
    n = float(n)
    y = s * np.sqrt((n + 1.0) * (n + 3.0) / (6.0 * (n - 2.0)))
    beta2 = 3.0 * (n * n + 27.0 * n - 70.0) * (n + 1.0) * (n + 3.0) / ((n - 2.0) * (n + 5.0) * (n + 7.0) * (n + 9.0))
    w2 = -1.0 + np.sqrt(2.0 * (beta2 - 1.0))
    delta = 1.0 / np.sqrt(0.5 * np.log(w2))
    alpha = np.sqrt(2.0 / (w2 - 1.0))
    if y == 0.0:
        y = 1.0
    return float(delta * np.arcsinh(y / alpha))


def kurtosis_z(k, n):
    n = float(n)
    b2 = k + 3.0
    e = 3.0 * (n - 1.0) / (n + 1.0)
    var = 24.0 * n * (n - 2.0) * (n - 3.0) / ((n + 1.0) * (n + 1.0) * (n + 3.0) * (n + 5.0))
    x = (b2 - e) / np.sqrt(var)
    sb1 = 6.0 * (n * n - 5.0 * n + 2.0) / ((n + 7.0) * (n + 9.0)) * np.sqrt(6.0 * (n + 3.0) * (n + 5.0) / (n * (n - 2.0) * (n - 3.0)))
    a = 6.0 + 8.0 / sb1 * (2.0 / sb1 + np.sqrt(1.0 + 4.0 / (sb1 * sb1)))
    term1 = 1.0 - 2.0 / (9.0 * a)
    denom = 1.0 + x * np.sqrt(2.0 / (a - 4.0))
    if denom == 0.0:
        return NAN
    term2 = np.sign(denom) * np.cbrt((1.0 - 2.0 / a) / abs(denom))
    return float((term1 - term2) / np.sqrt(2.0 / (9.0 * a)))


def dagostino_k2(x):
    n = len(x)
    if n < 8:
        return _failed(n, STATUS_INSUFFICIENT_DATA)
    sk = _shape(x)
    if sk is None:
        return _failed(n, STATUS_INVALID_INPUT)
    s, k = sk
    with np.errstate(over="ignore", invalid="ignore"):
        zs, zk = skew_z(s, n), kurtosis_z(k, n)
        k2 = zs * zs + zk * zk
        return [k2, float(np.exp(-k2 / 2.0)), s, k, zs, zk, float(n), 0.0]


_RECORD = {SHAPIRO_WILK: shapiro_wilk, DAGOSTINO_K2: dagostino_k2, JARQUE_BERA: jarque_bera}


def record(test, v):
    """The record of one group: the rows v, NaN rows dropped."""
    v = np.asarray(v, np.float64)
    return _RECORD[test](v[~np.isnan(v)])


def as_row(rec):
    """The record as a dict, or None for a status that is not 0."""
    return None if rec[7] != 0 else dict(zip(RECORD_NAMES, rec))


# ---- the case set ----
SIZES_CPU = tuple(range(3, 14)) + (20, 63, 64, 65, 129, 300, 1462, 1463, 5000)
SIZES_GPU = (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 63, 64, 65, 129, 300)
CONTENTS = ("normal", "exponential", "ties", "nan_rows", "offset", "all_equal")


def make_group(content, n, seed=0):
    """One group with n VALID rows of the content."""
    rng = np.random.default_rng(100003 * seed + 1009 * CONTENTS.index(content) + n)
    if content == "exponential":
        return rng.exponential(1.0, n)
    if content == "ties":
        return rng.integers(0, 5, n).astype(np.float64)
    if content == "offset":
        k = np.round(rng.standard_normal(n) * 1024.0)
        if n:
            k[0] -= np.sum(k) % n             # the sum a multiple of n: the mean is exact
        return 1e6 + k / 1024.0
    if content == "all_equal":
        return np.full(n, 2.5)
    v = rng.standard_normal(n)
    if content == "nan_rows":
        extra = n // 3 + 2
        full = np.full(n + extra, NAN)
        keep = np.ones(n + extra, bool)
        keep[rng.permutation(n + extra)[:extra]] = False
        full[keep] = v
        return full
    return v


def make_call(content, sizes=SIZES_GPU, seed=0):
    """-> dict(off, v): one group per size, the group's valid rows as many as its size."""
    groups = [make_group(content, n, seed) for n in sizes]
    return dict(off=np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64),
                v=np.concatenate(groups) if groups else np.zeros(0))


def reference(test, call):
    off = call["off"]
    return np.array([record(test, call["v"][off[g]:off[g + 1]]) for g in range(len(off) - 1)], np.float64).reshape(-1, 8)


def check_records(test, got, ref, errs=None):
    """The bounds of the host program and of the GPU against this file: counts and statuses exactly; W, skewness and kurtosis within
    1e-12 absolute; the statistic and the two z within 1e-9 max(1, |ref|); p within 1e-9 relative where p > 1e-300; NaN exactly
    where this file has it.  The p of a Shapiro-Wilk group passes through log(1 - W): every compared group has 1 - W >= 1e-8 on
    this file's W, or is the W = 1, p = 1 that a range of 0 is given by rule (or the NaN of an infinity among the rows)."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 8), np.asarray(ref, np.float64).reshape(-1, 8)
    assert got.shape == ref.shape
    errs = {} if errs is None else errs

    def near(name, a, b, bound, scale):
        if np.isnan(b):
            return
        e = abs(a - b) / scale if np.isfinite(b) else (0.0 if a == b else np.inf)
        errs[name] = max(errs.get(name, 0.0), e)
        assert e <= bound, (name, a, b)

    for g in range(len(ref)):
        a, b = got[g], ref[g]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (g, a, b)
        assert a[6] == b[6] and a[7] == b[7], (g, a, b)
        if b[7] != 0:
            continue
        if test == SHAPIRO_WILK:
            assert np.isnan(b[0]) or 1.0 - b[0] >= 1e-8 or (b[0] == 1.0 and b[1] == 1.0), (g, b)      # (1, 1: the rule for a range of 0, no logarithm)
            near("W", a[0], b[0], 1e-12, 1.0)
        else:
            near("statistic", a[0], b[0], 1e-9, max(1.0, abs(b[0])))
            near("skewness", a[2], b[2], 1e-12, 1.0)
            near("kurtosis", a[3], b[3], 1e-12, 1.0)
            near("z", a[4], b[4], 1e-9, max(1.0, abs(b[4])))
            near("z", a[5], b[5], 1e-9, max(1.0, abs(b[5])))
        if np.isnan(b[1]):
            continue
        if b[1] > 1e-300:
            near("p_value", a[1], b[1], 1e-9, b[1])
        else:
            assert a[1] <= 1e-299, (g, a, b)
    return errs


# ---- the tables of the reference's SQL tests (tests/golden/normality_tests/*.csv: table, value) ----
def load_tables(folder):
    """-> {test name: {table: values}}"""
    out = {}
    for name in TESTS:
        tables = {}
        with open(os.path.join(folder, name + ".csv"), newline="") as f:
            for row in csv.DictReader(f):
                tables.setdefault(row["table"], []).append(float(row["value"]))
        out[name] = {t: np.array(v) for t, v in tables.items()}
    return out


def check_known_answers(tables, run):
    """Every inequality of test/sql/normality/test_{shapiro_wilk,jarque_bera,dagostino}_agg.test; run(name, table, values) -> the
    record as a dict (RECORD_NAMES), or None for a NULL."""
    def of(name, table):
        return run(name, table, tables[name][table])

    r = of("shapiro_wilk", "normal_data")
    assert r["p_value"] > 0.05 and r["statistic"] > 0.95 and r["n"] == 20
    assert of("shapiro_wilk", "skewed_data")["p_value"] < 0.05 and of("shapiro_wilk", "bimodal_data")["p_value"] < 0.05
    assert of("shapiro_wilk", "grouped_normal")["p_value"] > 0.05 and not of("shapiro_wilk", "grouped_skewed")["p_value"] > 0.05
    assert not np.isnan(of("shapiro_wilk", "min_sample")["statistic"])
    r = of("shapiro_wilk", "constant_data")
    assert r["statistic"] == 1.0 and r["p_value"] == 1.0

    r = of("jarque_bera", "normal_data")
    assert r["p_value"] > 0.05 and abs(r["skewness"]) < 1.0 and r["n"] == 20 and not np.isnan(r["statistic"]) and not np.isnan(r["kurtosis"])
    r = of("jarque_bera", "skewed_data")
    assert r["p_value"] < 0.05 and r["skewness"] > 1.0
    assert of("jarque_bera", "grouped_normal")["p_value"] > 0.05 and not of("jarque_bera", "grouped_skewed")["p_value"] > 0.05

    r = of("dagostino_k2", "normal_data")
    assert r["p_value"] > 0.05 and r["n"] == 20 and not np.isnan(r["statistic"])
    assert of("dagostino_k2", "skewed_data")["p_value"] < 0.05
    assert of("dagostino_k2", "grouped_normal")["p_value"] > 0.05 and not of("dagostino_k2", "grouped_skewed")["p_value"] > 0.05
