"""A row-based restatement of the correlation contract ("Rank and product-moment correlation") for the tests, in
numpy and scipy.stats; it does not import the package.  R's cor.test with exact = FALSE in closed form: Kendall's s by the
definition over all pairs (O(n^2)), midranks from a stable sort, p-values from scipy's Student-t and normal distributions.
Also the shapes and the known answers the CPU and GPU tiers share."""
import numpy as np
from scipy import stats as sps

PEARSON, SPEARMAN, KENDALL = 0, 1, 2
TWO_SIDED, LESS, GREATER = 0, 1, 2
TAU_A, TAU_B, TAU_C = 0, 1, 2
NAN = float("nan")


def midranks(v, dtype=np.float64):
    order = np.argsort(v, kind="stable")
    s = v[order]
    out = np.empty(len(v), dtype)
    i = 0
    while i < len(s):
        e = i + 1
        while e < len(s) and s[e] == s[i]:
            e += 1
        out[order[i:e]] = dtype(i + e + 1) / dtype(2)
        i = e
    return out


def _pearson_r(a, b, dtype=np.float64):
    a, b = a.astype(dtype), b.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        da, db = a - a.sum() / dtype(len(a)), b - b.sum() / dtype(len(b))
        saa, sbb, sab = (da * da).sum(), (db * db).sum(), (da * db).sum()
        if not (saa > 0 and sbb > 0):
            return dtype(NAN)
        return min(dtype(1), max(dtype(-1), sab / np.sqrt(saa * sbb)))


def _t_p(t, df, alt):
    if np.isnan(t):
        return NAN
    if alt == TWO_SIDED:
        return float(2.0 * sps.t.sf(abs(t), df))
    return float(sps.t.cdf(t, df) if alt == LESS else sps.t.sf(t, df))


def _z_p(z, alt):
    if np.isnan(z):
        return NAN
    if alt == TWO_SIDED:
        return float(2.0 * sps.norm.sf(abs(z)))
    return float(sps.norm.cdf(z) if alt == LESS else sps.norm.sf(z))


def ties(v):
    _, counts = np.unique(v, return_counts=True)
    t = [int(c) for c in counts]
    return (sum(c * (c - 1) for c in t), sum(c * (c - 1) * (2 * c + 5) for c in t), sum(c * (c - 1) * (c - 2) for c in t), len(t))


def kendall_s(x, y):
    sx = (x[:, None] > x[None, :]).astype(np.int64) - (x[:, None] < x[None, :]).astype(np.int64)
    sy = (y[:, None] > y[None, :]).astype(np.int64) - (y[:, None] < y[None, :]).astype(np.int64)
    return int(np.triu(sx * sy, 1).sum())


def record(x, y, method, alternative=TWO_SIDED, tau_type=TAU_B, confidence_level=0.95, dtype=np.float64):
    """The 8 doubles of one group: {estimate, statistic, p_value, ci_lower, ci_upper, n, s, status}.  dtype: the arithmetic of the
    estimate, the statistic and the interval (np.longdouble for the restatement's own spread); the p-values are scipy's."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    keep = ~(np.isnan(x) | np.isnan(y))
    x, y = x[keep], y[keep]
    n = len(x)
    if n < 3:
        return [NAN, NAN, NAN, NAN, NAN, float(n), NAN, 6.0]
    D = dtype
    if method in (PEARSON, SPEARMAN):
        r = _pearson_r(x, y, D) if method == PEARSON else _pearson_r(midranks(x, D), midranks(y, D), D)
        t, lo, hi = D(NAN), D(NAN), D(NAN)
        if not np.isnan(r):
            with np.errstate(divide="ignore"):
                t = D(np.inf) * np.sign(r) if abs(r) >= 1 else r * np.sqrt(D(n - 2) / (D(1) - r * r))
                if n > 3 and confidence_level is not None and not np.isnan(confidence_level):
                    zq = D(sps.norm.ppf(0.5 * (1.0 + confidence_level)))
                    z, h = np.arctanh(r), zq / np.sqrt(D(n - 3))
                    lo, hi = np.tanh(z - h), np.tanh(z + h)
        return [r, t, _t_p(float(t), n - 2, alternative), lo, hi, float(n), NAN, 0.0]
    s = kendall_s(x, y)
    tx, ty = ties(x), ties(y)
    tau, z = D(NAN), D(NAN)
    if tx[3] > 1 and ty[3] > 1:
        n0 = n * (n - 1) // 2
        if tau_type == TAU_A:
            tau = D(s) / D(n0)
        elif tau_type == TAU_B:
            tau = D(s) / np.sqrt(D(n0 - tx[0] // 2) * D(n0 - ty[0] // 2))
        else:
            m = D(min(tx[3], ty[3]))
            tau = D(2) * D(s) / (D(n) * D(n) * (m - 1) / m)
        dn = D(n)
        var = (dn * (dn - 1) * (2 * dn + 5) - D(tx[1]) - D(ty[1])) / 18 + D(tx[0]) * D(ty[0]) / (2 * dn * (dn - 1)) + \
            D(tx[2]) * D(ty[2]) / (9 * dn * (dn - 1) * (dn - 2))
        z = D(s) / np.sqrt(var)
    return [tau, z, _z_p(float(z), alternative), NAN, NAN, float(n), float(s), 0.0]


# ---- the reference's SQL tables (test/sql/correlation/test_{pearson,spearman,kendall}_agg.test) ----
_X10 = [float(i) for i in range(1, 11)]
TABLES = {
    "positive": (_X10, [2.0, 4.1, 5.9, 8.2, 9.8, 12.1, 13.9, 16.2, 18.0, 20.1]),
    "negative": (_X10, [10.0, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0]),
    "negative_pearson": (_X10, [10.0, 8.1, 6.0, 4.2, 2.1, 0.0, -1.9, -3.9, -6.0, -8.1]),
    "no_cor": (_X10, [5.0, 3.0, 8.0, 1.0, 10.0, 2.0, 7.0, 4.0, 9.0, 6.0]),
    "no_cor_pearson": (_X10, [5.2, 3.1, 7.4, 2.3, 8.9, 1.2, 6.5, 4.8, 9.1, 0.5]),
    "group_a": (_X10[:5], [2.0, 4.0, 6.0, 8.0, 10.0]),
    "group_b": (_X10[:5], [5.0, 3.0, 8.0, 1.0, 10.0]),
    "tied_data": (_X10, [2.0, 2.0, 4.0, 4.0, 6.0, 6.0, 8.0, 8.0, 10.0, 10.0]),
    "nonlinear": (_X10, [v * v for v in _X10]),
}


def check_known_answers(get):
    """get(table name, method) -> (estimate, p_value, n): the statements of the reference's SQL tests."""
    for m in (SPEARMAN, KENDALL):
        assert get("positive", m)[0] == 1.0 and get("positive", m)[1] < 0.001 and get("positive", m)[2] == 10
        assert get("negative", m)[0] == -1.0
        assert abs(get("no_cor", m)[0]) < 0.5
        assert get("group_a", m)[0] > 0.5 and not get("group_b", m)[0] > 0.5
    assert get("tied_data", KENDALL)[0] > 0.8 and get("tied_data", SPEARMAN)[0] > 0.9
    assert get("nonlinear", SPEARMAN)[0] == 1.0
    assert get("positive", PEARSON)[0] > 0.99 and get("positive", PEARSON)[1] < 0.001 and get("positive", PEARSON)[2] == 10
    assert get("negative_pearson", PEARSON)[0] < -0.99
    assert abs(get("no_cor_pearson", PEARSON)[0]) < 0.5 and get("no_cor_pearson", PEARSON)[1] > 0.05
    assert abs(get("group_a", PEARSON)[0] - 1.0) < 1e-4 and not get("group_b", PEARSON)[0] > 0.5


# ---- the shapes of the issue: groups of these many VALID rows in one call, with varied content ----
SIZES = (0, 2, 3, 4, 63, 64, 65, 129, 300)
CONTENTS = ("noise", "nan_rows", "constant_x", "ties", "monotone")


def make_call(content, seed=0):
    """-> (row_offsets, x, y) with one group per size of SIZES, the group's valid rows as many as its size."""
    rng = np.random.default_rng(1000 * seed + CONTENTS.index(content))
    xs, ys, off = [], [], [0]
    for n in SIZES:
        x = rng.standard_normal(n)
        y = 0.6 * x + rng.standard_normal(n)
        if content == "constant_x":
            x = np.full(n, 2.5)
        elif content == "ties":
            x, y = rng.integers(0, 5, n).astype(np.float64), rng.integers(0, 5, n).astype(np.float64)
        elif content == "monotone":
            x = rng.permutation(n).astype(np.float64)
            y = -np.exp(x / 50.0)
        if content == "nan_rows":   # NaN rows scattered in: the valid rows stay n
            extra = n // 3 + 2
            total = n + extra
            at = rng.permutation(total)[:extra]
            fx, fy = np.empty(total), np.empty(total)
            mask = np.zeros(total, bool)
            mask[at] = True
            fx[~mask], fy[~mask] = x, y
            fx[mask], fy[mask] = rng.standard_normal(extra), rng.standard_normal(extra)
            for j, i in enumerate(at):
                if j % 3 != 1:
                    fx[i] = NAN
                if j % 3 != 0:
                    fy[i] = NAN
            x, y = fx, fy
        xs.append(x)
        ys.append(y)
        off.append(off[-1] + len(x))
    return np.array(off, np.int64), np.concatenate(xs), np.concatenate(ys)


def reference(off, x, y, method, **kw):
    return np.array([record(x[off[g]:off[g + 1]], y[off[g]:off[g + 1]], method, **kw) for g in range(len(off) - 1)], np.float64)


def check_records(got, ref, errs=None):
    """The issue's bounds: n, s and status exactly; the estimate within 1e-12 absolute; statistic and interval within 1e-9
    relative; p-values within 1e-9 relative where p > 1e-300.  NaN where the restatement has NaN."""
    got, ref = np.asarray(got, np.float64).reshape(-1, 8), np.asarray(ref, np.float64).reshape(-1, 8)
    assert got.shape == ref.shape
    errs = {} if errs is None else errs
    for g in range(len(ref)):
        a, b = got[g], ref[g]
        assert a[7] == b[7] and a[5] == b[5], (g, a, b)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (g, a, b)
        if b[7] != 0:
            continue
        if not np.isnan(b[6]):
            assert a[6] == b[6], (g, a, b)
        if np.isnan(b[0]):
            continue
        e = abs(a[0] - b[0])
        errs["estimate"] = max(errs.get("estimate", 0.0), e)
        assert e <= 1e-12, (g, a, b)
        for j, name in ((1, "statistic"), (3, "ci"), (4, "ci")):
            if np.isnan(b[j]):
                continue
            if np.isinf(b[j]) or b[j] == 0.0:
                assert a[j] == b[j], (g, j, a, b)
                continue
            e = abs(a[j] - b[j]) / abs(b[j])
            errs[name] = max(errs.get(name, 0.0), e)
            assert e <= 1e-9, (g, j, a, b)
        if b[2] > 1e-300:
            e = abs(a[2] - b[2]) / b[2]
            errs["p_value"] = max(errs.get("p_value", 0.0), e)
            assert e <= 1e-9, (g, a, b)
        else:
            assert a[2] <= 1e-299, (g, a, b)
    return errs
