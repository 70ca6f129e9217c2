"""The seeded cases of the randomised sweep of the five grouped test families that run on the size-tiered launch driver
(csrc/rank_launch.h): correlation, rank tests, sample tests, normality tests, categorical tests.  Pure numpy; it does not import
the package.  The references are the five restatement modules, their record / reference / check_records unchanged.

    case(family, seed)            one call: the family's test, its options, 8 to 40 groups whose sizes and contents are drawn
                                  independently, in the family's existing call layout plus `kinds`, `sizes`, `family`, `test`
    tiled_call(family, ...)       a pool of drawn groups repeated cyclically to many groups, for the many-group tests
    reference / check             the family's restatement and its bounds on a case
    assert_input_conditions(case) the float64 restatement against a higher-precision form of itself, at a tenth of the bounds

Sizes are ROW counts (the driver tiers a group by its rows, valid or not): 0..9 and b - 1, b, b + 1 around the wavefront, the
tiers (256, 1462) and the powers of two a bitonic pad steps at; one group of 2049 rows at most, the first size at which the
large path's sort strides.  A seed is given three boundary sizes by its number (six consecutive seeds hold all eighteen) and the
kind of its first group, so that a dozen seeds cover every size and kind whatever the draws; the rest is drawn, weighted to small
sizes so that a call stays under about 6000 rows.

KINDS[family][kind] lists the tests of the family that take the kind.  A (test, kind) pair is absent where the float64
restatement does not agree with its higher-precision form within a tenth of check_records' bound: there the restatement cannot
referee the kernel.  Every absence carries the failing field and the size of the disagreement.  No group of a generated call is
left out of the comparison at run time."""
import os
from fractions import Fraction

import numpy as np
from scipy import stats as sps

import categorical_test_restate as CT
import cor_restate as COR
import normality_test_restate as NT
import rank_test_restate as RT
import sample_test_restate as ST

SCALE = max(1, int(os.environ.get("ANOFOX_FUZZ_SCALE", "1")))
FAMILIES = ("cor", "rank", "sample", "normality", "categorical")
MODULE = {"cor": COR, "rank": RT, "sample": ST, "normality": NT, "categorical": CT}
TESTS = {"cor": (COR.PEARSON, COR.SPEARMAN, COR.KENDALL), "rank": (RT.MANN_WHITNEY, RT.WILCOXON, RT.KRUSKAL_WALLIS),
         "sample": (ST.T_TEST, ST.YUEN, ST.ANOVA, ST.BROWN_FORSYTHE, ST.BRUNNER_MUNZEL),
         "normality": (NT.SHAPIRO_WILK, NT.DAGOSTINO_K2, NT.JARQUE_BERA),
         "categorical": (CT.CHI_SQUARE, CT.G_TEST, CT.FISHER_EXACT, CT.MCNEMAR)}
# the tests whose rows are staged in the work arrays (the others run every group on the first small instance)
STAGED = {"cor": (COR.SPEARMAN, COR.KENDALL), "rank": TESTS["rank"],
          "sample": (ST.YUEN, ST.ANOVA, ST.BROWN_FORSYTHE, ST.BRUNNER_MUNZEL), "normality": (NT.SHAPIRO_WILK,),
          "categorical": (CT.CHI_SQUARE, CT.G_TEST)}
WIDTH = {"cor": 8, "rank": 8, "sample": 12, "normality": 8, "categorical": 12}
STATUS = {"cor": 7, "rank": 7, "sample": 11, "normality": 7, "categorical": 11}
COUNT = {"cor": 5, "rank": 4, "sample": 7, "normality": 6, "categorical": 6}       # the record's count of valid rows
INSUFFICIENT = 6

SMALL_SIZES = (0, 1, 2, 3, 4, 5, 7, 8, 9)
BOUNDARY_SIZES = tuple(b + d for b in (64, 128, 256, 512, 1024, 1462) for d in (-1, 0, 1))
STRIDE_SIZE = 2049
CAPS = (1, 2, 63, 64, 65, 128, 255, 256, 257, 300, 1461)
ROW_BUDGET = 6000

FLOAT_KINDS = ("continuous", "ties", "all_equal", "ascending", "descending", "nan_scattered", "all_nan", "signed_zeros", "infinities",
               "subnormal", "offset")
LABEL_KINDS = ("table", "distinct", "constant", "extreme", "sentinel", "all_null")


def _all_but(family, **absent):
    """kind -> the tests of the family that take it; absent: kind -> the tests that do not."""
    kinds = LABEL_KINDS if family == "categorical" else FLOAT_KINDS
    return {k: tuple(t for t in TESTS[family] if t not in absent.get(k, ())) for k in kinds}


KINDS = {
    # subnormal, Pearson: the squares of multiples of 5e-324 are 0 in binary64, so r is NaN; in long double r is a number (7.6e-4
    #   where binary64 has NaN, 128 rows)
    "cor": _all_but("cor", subnormal=(COR.PEARSON,)),
    "rank": _all_but("rank"),
    # subnormal, t, Yuen, ANOVA, Brown-Forsythe: the centred squares are 0 in binary64 (se or SSW 0: a NaN statistic) and are not 0
    #   exactly (F = 0.131 where binary64 has NaN, 2049 rows)
    # offset, t, Yuen, ANOVA: the mean of 1e8 + z is rounded by about 1e-8, as large as the difference of two arm means over its
    #   standard error allows: the statistic moves by 2.7e-7 (t, 2049 rows), 1.6e-7 (Yuen, 129 rows), 1.8e-9 (F, 65 rows) against a
    #   tenth of 1e-9.  Brown-Forsythe (deviations from a median: exact differences) and Brunner-Munzel (ranks) keep the kind.
    "sample": _all_but("sample", subnormal=(ST.T_TEST, ST.YUEN, ST.ANOVA, ST.BROWN_FORSYTHE), offset=(ST.T_TEST, ST.YUEN, ST.ANOVA)),
    # offset, K2 and Jarque-Bera: the rounded mean moves the third moment: the statistic by 8.5e-8 (K2, 8 rows) and 1.2e-7
    #   (Jarque-Bera, 129 rows) against a tenth of 1e-9.  Shapiro-Wilk centres on an order statistic and keeps the kind.
    "normality": _all_but("normality", offset=(NT.DAGOSTINO_K2, NT.JARQUE_BERA)),
    "categorical": _all_but("categorical"),
}
# Brown-Forsythe's F of a group whose arms all have two rows is a ratio of rounding noise (the two deviations from the arms' median
# are equal, SSW is 0 exactly and 1e-33 in binary64: F = 8.6e31 against -7.7e32).  Groups of fewer than 10 rows of this test take
# their real-valued kinds as "ties", whose deviations and sums are exact.
_REAL_VALUED = ("continuous", "ascending", "descending", "nan_scattered", "infinities", "offset")


def kind_at(family, test, n, kind):
    """The kind a group of n rows takes where `kind` was drawn."""
    return "ties" if family == "sample" and test == ST.BROWN_FORSYTHE and n < 10 and kind in _REAL_VALUED else kind


def kinds_of(family, test):
    return tuple(k for k, tests in KINDS[family].items() if test in tests)


# ---- the contents ----
def values(rng, n, kind):
    """n rows of the kind."""
    if kind == "ties":
        return rng.integers(0, 4, n).astype(np.float64)
    if kind == "all_equal":
        return np.full(n, 2.5)
    if kind == "all_nan":
        return np.full(n, np.nan)
    if kind == "signed_zeros":
        return rng.choice(np.array([-0.0, 0.0, 1.0]), n)
    if kind == "subnormal":
        return rng.integers(-40, 41, n) * 5e-324
    v = rng.standard_normal(n)
    if kind == "ascending":
        return np.sort(v)
    if kind == "descending":
        return np.sort(v)[::-1].copy()
    if kind == "offset":
        return 1e8 + v
    if kind == "nan_scattered" and n:
        v[rng.random(n) < rng.uniform(0.1, 0.6)] = np.nan
    if kind == "infinities" and n:
        at = rng.permutation(n)[:min(n, int(rng.integers(1, 4)))]
        v[at] = rng.choice(np.array([np.inf, -np.inf]), len(at))
    return v


def _ids(rng, family, test, n):
    """The sample ids of a group: the two-sample tests split on 0; the k-sample tests take a pool of 2 to 7 of the restatements'
    ids (INT32_MIN and INT32_MAX among them), now and then with an arm of one row."""
    two = test in ((RT.MANN_WHITNEY,) if family == "rank" else ST._TWO)
    ids = (RT if family == "rank" else ST)._IDS
    if two:
        pool = np.array([0, 0, 1, -3] if rng.random() < 0.5 else [0, ids[4], ids[5], 0], np.int32)
        s = rng.choice(pool, n)
        if n > 2 and rng.random() < 0.15:          # a single-row arm
            s[:] = 0 if rng.random() < 0.5 else 7
            s[rng.integers(n)] = 7 if s[0] == 0 else 0
        return s
    k = int(rng.integers(2, 8))
    pool = np.array(ids[:k], np.int32)
    if n > k and rng.random() < 0.25:
        s = rng.choice(pool[:-1], n) if k > 2 else np.full(n, pool[0], np.int32)
        s[rng.integers(n)] = pool[-1]
        return s.astype(np.int32)
    return rng.choice(pool, n)


def _labels(rng, n, kind):
    """(a, b) int32 label pairs of n rows: a drawn r x c table (2 x 2 to 5 x 7) with association, or one of the alphabets of
    categorical_test_restate."""
    if kind == "distinct":
        a, b = rng.permutation(n) - n // 2, rng.permutation(n) * 3 - 5
    elif kind == "constant":
        a, b = rng.integers(0, 3, n), np.full(n, 1)
    elif kind == "extreme":
        a, b = CT.EXTREME[rng.integers(0, 5, n)], CT.EXTREME[rng.integers(0, 5, n)]
    elif kind == "all_null":
        a, b = np.full(n, CT.NULL), np.where(rng.random(n) < 0.5, CT.NULL, 1)
    else:
        r, c = int(rng.integers(2, 6)), int(rng.integers(2, 8))
        a = rng.integers(0, r, n)
        b = (a + rng.integers(0, c, n) * (rng.random(n) < 0.7)) % c
        if kind == "sentinel" and n:
            a, b = a.copy(), b.copy()
            gone = rng.random(n) < rng.uniform(0.1, 0.6)
            gone[[0, n - 1]] = True
            side = rng.integers(0, 3, n)
            a[gone & (side != 1)] = CT.NULL
            b[gone & (side != 0)] = CT.NULL
    return np.asarray(a, np.int32), np.asarray(b, np.int32)


def draw_group(family, test, rng, n, kind):
    """The columns of one group of n rows."""
    if family == "categorical":
        a, b = _labels(rng, n, kind)
        return dict(a=a, b=b)
    v = values(rng, n, kind)
    if family == "normality":
        return dict(v=v)
    if kind == "continuous":
        y = 0.6 * v + rng.standard_normal(n)
    else:
        y = values(rng, n, kind) if rng.random() < 0.5 and kind != "all_nan" else rng.standard_normal(n)
    if family == "cor":
        return dict(x=v, y=y)
    return dict(v=v, y=y, sample=_ids(rng, family, test, n))


_COLUMNS = {"cor": (("x", np.float64), ("y", np.float64)), "rank": (("v", np.float64), ("y", np.float64), ("sample", np.int32)),
            "sample": (("v", np.float64), ("y", np.float64), ("sample", np.int32)), "normality": (("v", np.float64),),
            "categorical": (("a", np.int32), ("b", np.int32))}


def build_call(family, test, opts, groups, kinds):
    """The call of the groups (each the dict draw_group returns)."""
    call = dict(family=family, test=test, opts=dict(opts), kinds=list(kinds))
    lead = _COLUMNS[family][0][0]
    call["sizes"] = [len(g[lead]) for g in groups]
    call["off"] = np.concatenate([[0], np.cumsum(call["sizes"])]).astype(np.int64)
    for name, dtype in _COLUMNS[family]:
        call[name] = np.concatenate([g[name] for g in groups]).astype(dtype) if groups else np.zeros(0, dtype)
    if family == "rank":
        call["mu"] = opts.get("mu", 0.0)
    return call


def draw_options(family, test, rng):
    """The options of a call, the absent forms of the confidence level (None, NaN) among them."""
    level = lambda: [0.95, 0.9, 0.99, None, float("nan")][int(rng.integers(0, 5))]   # noqa: E731
    alt = int(rng.integers(0, 3))
    if family == "cor":
        return dict(alternative=alt, tau_type=int(rng.integers(0, 3)), confidence_level=level())
    if family == "rank":
        mu = float(rng.choice([0.0, 0.0, 0.75, -0.5]))
        return dict(alternative=alt, correction=bool(rng.integers(0, 2)), mu=0.0 if test == RT.KRUSKAL_WALLIS else mu)   # (it takes none)
    if family == "sample":
        kind = int(rng.integers(0, 3)) if test == ST.T_TEST else int(rng.integers(0, 2)) if test == ST.ANOVA else 0
        mu = float(rng.choice([0.0, 0.75]))
        return dict(alternative=alt, kind=kind, mu=mu if test == ST.T_TEST else 0.0, trim=float(rng.choice([0.0, 0.1, 0.2, 0.25])),
                    confidence_level=level())                   # (only the t-test takes a mu)
    if family == "categorical":
        return dict(alternative=alt, correction=bool(rng.integers(0, 2)), exact=bool(rng.integers(0, 2)), confidence_level=level())
    return {}


def _rng(family, seed, salt=0):
    return np.random.default_rng([FAMILIES.index(family), seed, salt])


def case(family, seed):
    """The call of the seed.  The test cycles with the seed (every test of a family within any run of consecutive seeds)."""
    rng = _rng(family, seed)
    tests = TESTS[family]
    test = tests[seed % len(tests)]
    opts = draw_options(family, test, rng)
    kinds = kinds_of(family, test)
    n_groups = int(rng.integers(8, 41))
    forced = [BOUNDARY_SIZES[i] for i in range(len(BOUNDARY_SIZES)) if i % 6 == seed % 6]
    if seed % 2 == 0:
        forced.append(STRIDE_SIZE)
    sizes = [None] * n_groups
    for n, at in zip(forced, rng.permutation(n_groups)):
        sizes[at] = n
    left = ROW_BUDGET - sum(forced)
    weights = np.array([1.0 / b for b in BOUNDARY_SIZES])
    for g in range(n_groups):
        if sizes[g] is None:
            n = int(rng.choice(BOUNDARY_SIZES, p=weights / weights.sum())) if rng.random() < 0.55 else int(rng.choice(SMALL_SIZES))
            sizes[g] = n if n <= left else int(rng.choice(SMALL_SIZES))
            left -= sizes[g]
    all_kinds = LABEL_KINDS if family == "categorical" else FLOAT_KINDS
    first = all_kinds[seed % len(all_kinds)]
    drawn = [kinds[int(rng.integers(len(kinds)))] for _ in range(n_groups)]
    if first in kinds:
        drawn[0] = first
    drawn = [kind_at(family, test, n, k) for n, k in zip(sizes, drawn)]
    groups = [draw_group(family, test, rng, n, k) for n, k in zip(sizes, drawn)]
    return build_call(family, test, opts, groups, drawn)


def fixed_call(family, test, sizes, kinds, seed=0, opts=None):
    """A call of the given sizes and kinds (one kind for all, or one per group) with default options."""
    rng = _rng(family, seed, 1)
    kinds = [kinds] * len(sizes) if isinstance(kinds, str) else list(kinds)
    kinds = [kind_at(family, test, n, k) for n, k in zip(sizes, kinds)]
    return build_call(family, test, opts or {}, [draw_group(family, test, rng, n, k) for n, k in zip(sizes, kinds)], kinds)


def select(call, groups):
    """The call of the listed groups of `call`, in that order (a group may repeat)."""
    off = call["off"]
    parts = [{name: call[name][off[g]:off[g + 1]] for name, _ in _COLUMNS[call["family"]]} for g in groups]
    return build_call(call["family"], call["test"], call["opts"], parts, [call["kinds"][g] for g in groups])


def tiled_call(family, pool_seed, n_pool, n_groups, test=None, sizes=range(0, 41), shuffle=False):
    """-> (call of n_groups groups, the pool index of every group, the pool's own call of n_pool groups).  The pool: n_pool drawn
    groups, distinct, of every kind the test takes and of sizes spread over `sizes`; group g of the call is pool member g % n_pool."""
    rng = _rng(family, pool_seed, 2)
    test = TESTS[family][0] if test is None else test
    kinds = kinds_of(family, test)
    sizes = list(sizes)
    ns = [sizes[(i * 7) % len(sizes)] for i in range(n_pool)]
    ks = [kind_at(family, test, n, kinds[i % len(kinds)]) for i, n in enumerate(ns)]
    if shuffle:
        order = rng.permutation(n_pool)
        ns, ks = [ns[i] for i in order], [ks[i] for i in order]
    pool = build_call(family, test, {}, [draw_group(family, test, rng, n, k) for n, k in zip(ns, ks)], ks)
    index = np.arange(n_groups) % n_pool
    lens = np.asarray(pool["sizes"], np.int64)[index]
    call = dict(family=family, test=test, opts={}, kinds=[ks[i] for i in index], sizes=lens.tolist(),
                off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    reps, rest = divmod(n_groups, n_pool)
    for name, _ in _COLUMNS[family]:
        call[name] = np.concatenate([np.tile(pool[name], reps), pool[name][:pool["off"][rest]]])
    if family == "rank":
        call["mu"] = 0.0
    return call, index, pool


# ---- the stated calls of the GPU tier (its tests b to f), built here so that the CPU tier checks their input conditions ----
POOL_SEED = 1             # (a pool of seed 5 holds a 6-row signed-zero group whose r is 0 exactly and 2e-16 in binary64)
LADDER_TEST = {"cor": COR.SPEARMAN, "rank": RT.MANN_WHITNEY, "sample": ST.BRUNNER_MUNZEL, "normality": NT.SHAPIRO_WILK,
               "categorical": CT.CHI_SQUARE}
UNSTAGED_TEST = {"cor": COR.PEARSON, "sample": ST.T_TEST, "normality": NT.JARQUE_BERA, "categorical": CT.MCNEMAR}   # (rank has none)
SMALL_POOL, LARGE_POOL, LARGE_POOL_CAP = 97, 61, 16
SMALL_TILED = [(f, LADDER_TEST[f]) for f in FAMILIES] + list(UNSTAGED_TEST.items())
EVERY_STAGED = [(f, t) for f in FAMILIES for t in STAGED[f]]
EVERY_TEST = [(f, t) for f in FAMILIES for t in TESTS[f]]
STRIDE_SIZES = (2048, 2049, 4096, 4097)


def ladder_call(family, cap):
    """Groups of cap - 1, cap, cap + 1 and 2 cap + 1 valid rows and the tier boundaries, for the family's staged test."""
    kind = "table" if family == "categorical" else "continuous"          # every row valid
    return fixed_call(family, LADDER_TEST[family], [cap - 1, cap, cap + 1, 2 * cap + 1, 256, 257, 1462, 1463], kind, seed=cap)


def small_pool_call(family, test, n_groups=65536 * 2 + SMALL_POOL):
    return tiled_call(family, POOL_SEED, SMALL_POOL, n_groups, test=test, sizes=range(0, 41))


def large_pool_call(family, test, n_groups=1024 * 2 + LARGE_POOL):
    return tiled_call(family, POOL_SEED, LARGE_POOL, n_groups, test=test, sizes=range(0, 81), shuffle=True)


def stride_call(family, test):
    """Every size of STRIDE_SIZES as three kinds: group 0, 4 and 8 are the 2048-row ones."""
    kinds = ("table", "extreme", "sentinel") if family == "categorical" else ("continuous", "ties", "descending")
    return fixed_call(family, test, list(STRIDE_SIZES) * 3, [k for k in kinds for _ in STRIDE_SIZES], seed=11)


def special_call(family, test):
    """-> (call, the all-NaN groups): 65 and 257 rows of each special kind the test takes, then all-NaN (all-NULL) groups of 65 and
    257 rows, each between two full groups."""
    labels = family == "categorical"
    full, empty = ("table", "all_null") if labels else ("continuous", "all_nan")
    special = [k for k in (("extreme", "sentinel") if labels else ("signed_zeros", "infinities", "subnormal")) if k in kinds_of(family, test)]
    kinds = [full] + [k for k in special for _ in (65, 257)] + [full, empty, full, empty, full]
    sizes = [65] + [65, 257] * len(special) + [257, 65, 65, 257, 257]
    return fixed_call(family, test, sizes, kinds, seed=13), [g for g, k in enumerate(kinds) if k == empty]


def stated_calls():
    """(name, call) of every call of the GPU tier's tests b to f (the tiled ones as their pools)."""
    for f in FAMILIES:
        for cap in CAPS:
            yield "ladder %s cap %d" % (f, cap), ladder_call(f, cap)
    for f, t in SMALL_TILED:
        yield "small pool %s %d" % (f, t), small_pool_call(f, t, SMALL_POOL)[2]
    for f, t in EVERY_STAGED:
        yield "large pool %s %d" % (f, t), large_pool_call(f, t, LARGE_POOL)[2]
        yield "stride %s %d" % (f, t), stride_call(f, t)
    for f, t in EVERY_TEST:
        yield "special %s %d" % (f, t), special_call(f, t)[0]


# ---- the restatements on a case ----
def reference(call):
    f, t, o = call["family"], call["test"], call["opts"]
    if f == "cor":
        return COR.reference(call["off"], call["x"], call["y"], t, **o)
    if f == "rank":
        return RT.reference(t, call, **o)
    return MODULE[f].reference(t, call)       # sample, categorical: the call's opts; normality: none


def check(call, got, ref, errs=None):
    """The family's check_records; -> the worst error per field."""
    f, t = call["family"], call["test"]
    if f == "cor":
        return COR.check_records(got, ref, errs)
    if f == "sample":
        return ST.check_records(t, got, ref, call["opts"].get("kind", 0), errs)
    return MODULE[f].check_records(t, got, ref, errs)


# ---- the higher-precision forms ----
def _ld(fr):
    """A Fraction as a long double (two binary64 parts)."""
    hi = float(fr)
    return np.longdouble(hi) + np.longdouble(float(fr - Fraction(hi)))


def _fr(v):
    return [Fraction(float(t)) for t in v]


def _centred(fv):
    m = sum(fv) / len(fv)
    return m, sum((t - m) ** 2 for t in fv)


def _hp_rank(test, v, y, sample, o):
    """{field: value}: the rank sums and the variance in exact rationals (the midranks are exact in either form)."""
    alt, on, mu = o.get("alternative", 0), o.get("correction", True), o.get("mu", 0.0)
    half = Fraction(1, 2)
    if test == RT.WILCOXON:
        with np.errstate(invalid="ignore"):
            d = v - y - mu
        d = d[~np.isnan(d)]
        d = d[d != 0.0]
        m = len(d)
        r = _fr(RT.midranks(np.abs(d)))
        stat = sum((t for t, s in zip(r, d) if s > 0), Fraction(0))
        var = Fraction(m * (m + 1) * (2 * m + 1), 24) - Fraction(RT.tie_sum(np.abs(d))[0], 48) if m else Fraction(0)
        num = stat - Fraction(m * (m + 1), 4)
    elif test == RT.MANN_WHITNEY:
        keep = ~np.isnan(v)
        v, sample = v[keep], sample[keep]
        first = sample == 0
        n, n1 = len(v), int(first.sum())
        n2 = n - n1
        pooled = np.where(first, v - mu, v)
        r = _fr(RT.midranks(pooled))
        stat = sum((t for t, s in zip(r, first) if s), Fraction(0)) - Fraction(n1 * (n1 + 1), 2)
        ties, distinct = RT.tie_sum(pooled)
        var = Fraction(n1 * n2, 12) * ((n + 1) - Fraction(ties, n * (n - 1))) if distinct > 1 else Fraction(0)
        num = stat - Fraction(n1 * n2, 2)
    else:
        keep = ~np.isnan(v)
        v, sample = v[keep], sample[keep]
        n = len(v)
        ties, distinct = RT.tie_sum(v)
        if distinct < 2:
            return {}
        r = np.array(_fr(RT.midranks(v)), object)
        s = sum((sum(r[sample == j], Fraction(0)) ** 2 / int((sample == j).sum()) for j in np.unique(sample)), Fraction(0))
        return {0: _ld((Fraction(12, n * (n + 1)) * s - 3 * (n + 1)) / (1 - Fraction(ties, n ** 3 - n)))}
    if var <= 0:
        return {0: _ld(stat)}
    c = Fraction(0) if not on else (half * (1 if num > 0 else -1 if num < 0 else 0) if alt == 0 else half if alt == 2 else -half)
    return {0: _ld(stat), 1: _ld(num - c) / np.sqrt(_ld(var))}


def _hp_studentised(est, num, se2, df, o, out):
    se = np.sqrt(_ld(se2))
    out[4], out[10] = _ld(est), se
    if se2 > 0:
        out[0], out[2] = _ld(num) / se, _ld(df) if isinstance(df, Fraction) else df
        cl, alt = o.get("confidence_level", 0.95), o.get("alternative", 0)
        if cl is not None and not np.isnan(cl):
            q = np.longdouble(sps.t.isf(0.5 * (1.0 - cl) if alt == 0 else 1.0 - cl, float(out[2])))
            if alt != 1:
                out[5] = out[4] - q * se
            if alt != 2:
                out[6] = out[4] + q * se
    return out


def _hp_sample(test, v, y, sample, o):
    """{field: value}: the means, the centred sums and everything rational in them in exact rationals; square roots and the t
    quantile (scipy's, at the exact df) in long double."""
    kind, mu, trim = o.get("kind", 0), o.get("mu", 0.0), o.get("trim", 0.2)
    out = {}
    if test == ST.T_TEST and kind == ST.PAIRED:
        with np.errstate(invalid="ignore"):
            d = v - y
            d = d[~np.isnan(d - mu)]
        if not np.all(np.isfinite(d)):
            return {}
        n = len(d)
        m, s = _centred(_fr(d))
        return _hp_studentised(m, m - Fraction(mu), s / (n - 1) / n, np.longdouble(n - 1), o, out)
    keep = ~np.isnan(v)
    v, sample = v[keep], sample[keep]
    if not np.all(np.isfinite(v)):
        return {}
    n = len(v)
    a, b = v[sample == 0], v[sample != 0]
    n1, n2 = len(a), len(b)
    if test == ST.T_TEST:
        (m1, s1), (m2, s2) = _centred(_fr(a)), _centred(_fr(b))
        est = m1 - m2
        if kind == ST.STUDENT:
            return _hp_studentised(est, est - Fraction(mu), (s1 + s2) / (n1 + n2 - 2) * (Fraction(1, n1) + Fraction(1, n2)),
                                   np.longdouble(n1 + n2 - 2), o, out)
        e1, e2 = s1 / (n1 - 1) / n1, s2 / (n2 - 1) / n2
        den = e1 * e1 / (n1 - 1) + e2 * e2 / (n2 - 1)
        return _hp_studentised(est, est - Fraction(mu), e1 + e2, (e1 + e2) ** 2 / den if den > 0 else np.longdouble(np.nan), o, out)
    if test == ST.YUEN:
        parts = []
        for s in (np.sort(a), np.sort(b)):
            g = int(np.floor(trim * len(s)))
            h = len(s) - 2 * g
            w = _fr(np.clip(s, s[g], s[len(s) - g - 1]))
            parts.append((sum(_fr(s[g:len(s) - g])) / h, _centred(w)[1] / (h * (h - 1)), h))
        (t1, d1, h1), (t2, d2, h2) = parts
        den = d1 * d1 / (h1 - 1) + d2 * d2 / (h2 - 1)
        return _hp_studentised(t1 - t2, t1 - t2, d1 + d2, (d1 + d2) ** 2 / den if den > 0 else np.longdouble(np.nan), o, out)
    if test == ST.BRUNNER_MUNZEL:
        R = _fr(RT.midranks(np.concatenate([a, b])))
        R1, R2, r1, r2 = R[:n1], R[n1:], _fr(RT.midranks(a)), _fr(RT.midranks(b))
        m1, m2 = sum(R1) / n1, sum(R2) / n2
        v1 = sum((p - q + (Fraction(n1 + 1, 2) - m1)) ** 2 for p, q in zip(R1, r1)) / (n1 - 1)
        v2 = sum((p - q + (Fraction(n2 + 1, 2) - m2)) ** 2 for p, q in zip(R2, r2)) / (n2 - 1)
        phat = (m2 - Fraction(n2 + 1, 2)) / n1
        se = np.sqrt(_ld(v1 / (n1 * n2 * n2) + v2 / (n2 * n1 * n1)))
        s = n1 * v1 + n2 * v2
        out[4], out[10] = _ld(phat), se
        if s > 0:
            out[0] = _ld(Fraction(n1 * n2) * (m2 - m1) / (n1 + n2)) / np.sqrt(_ld(s))
            out[2] = _ld(s * s / ((n1 * v1) ** 2 / (n1 - 1) + (n2 * v2) ** 2 / (n2 - 1)))
            cl = o.get("confidence_level", 0.95)
            if cl is not None and not np.isnan(cl):
                q = np.longdouble(sps.t.isf(0.5 * (1.0 - cl), float(out[2])))
                out[5], out[6] = out[4] - q * se, out[4] + q * se
        return out
    arms = [v[sample == j] for j in np.unique(sample)]
    if test == ST.BROWN_FORSYTHE:
        arms = [np.abs(t - np.median(t)) for t in arms]     # (the absolute deviations are the data of the F test, in binary64)
    fa = [_fr(t) for t in arms]
    k = len(fa)
    grand = sum(sum(t) for t in fa) / n
    cs = [_centred(t) for t in fa]
    ssb = sum(len(t) * (m - grand) ** 2 for t, (m, _) in zip(fa, cs))
    ssw = sum(s for _, s in cs)
    out[4], out[10] = _ld(ssb), _ld(ssw)
    if ssw > 0:
        out[0] = _ld((ssb / (k - 1)) / (ssw / (n - k)))
    if test == ST.ANOVA and kind == ST.WELCH_ANOVA:
        out.pop(0, None)
        var = [s / (len(t) - 1) for t, (_, s) in zip(fa, cs)]
        if min(var) > 0:
            w = [len(t) / s for t, s in zip(fa, var)]
            mt = sum(wj * m for wj, (m, _) in zip(w, cs)) / sum(w)
            tmp = sum((1 - wj / sum(w)) ** 2 / (len(t) - 1) for wj, t in zip(w, fa)) / (k * k - 1)
            out[0] = _ld(sum(wj * (m - mt) ** 2 for wj, (m, _) in zip(w, cs)) / ((k - 1) * (1 + 2 * (k - 2) * tmp)))
            out[3] = _ld(1 / (3 * tmp))
    return out


def _hp_normality(test, v, o):
    """{field: value}: the central moments, and W = (sum a d)^2 / (sum a^2 sum (x - mean)^2), in exact rationals."""
    x = v[~np.isnan(v)]
    n = len(x)
    if not np.all(np.isfinite(x)):
        return {}
    if test == NT.SHAPIRO_WILK:
        y = np.sort(x)
        if y[-1] == y[0]:
            return {}
        fy = _fr(y)
        rng = fy[-1] - fy[0]
        xi = [(t - fy[n // 2]) / rng for t in fy]
        a = _fr(NT.sw_coefficients(n))
        ssa = 2 * sum(t * t for t in a)
        sax = sum(c * (xi[n - 1 - i] - xi[i]) for i, c in enumerate(a))
        return {0: _ld(sax * sax / (ssa * _centred(xi)[1]))}
    fx = _fr(x)
    m = sum(fx) / n
    m2, m3, m4 = (sum((t - m) ** p for t in fx) / n for p in (2, 3, 4))
    if m2 <= 0:
        return {}
    s, k = _ld(m3) / np.sqrt(_ld(m2)) ** 3, _ld(m4 / (m2 * m2) - 3)
    out = {2: s, 3: k}
    if test == NT.JARQUE_BERA:
        out[0] = n / np.longdouble(6) * (s * s + k * k / 4)
    else:
        out[4], out[5] = np.longdouble(NT.skew_z(float(s), n)), np.longdouble(NT.kurtosis_z(float(k), n))
        out[0] = out[4] ** 2 + out[5] ** 2
    return out


def _hp_categorical(test, a, b, o):
    """{field: value}: X2 and its measures from the table in exact rationals; G with long double logarithms."""
    if test not in (CT.CHI_SQUARE, CT.G_TEST):
        return {}                    # Fisher and McNemar take four counted cells: no sum depends on the rows' content
    a, b = a.astype(np.int64), b.astype(np.int64)
    ok = (a != CT.NULL) & (b != CT.NULL)
    t = CT.dense_table(a[ok], b[ok])
    n = int(t.sum())
    rows, cols = [int(s) for s in t.sum(axis=1)], [int(s) for s in t.sum(axis=0)]
    r, c = t.shape
    cells = [(int(t[i, j]), Fraction(rows[i] * cols[j], n)) for i in range(r) for j in range(c)]
    if test == CT.G_TEST:
        return {0: 2 * sum((np.longdouble(O) * np.log(np.longdouble(O) / _ld(E)) for O, E in cells if O), np.longdouble(0))}
    x2 = sum((O - E) ** 2 / E for O, E in cells)
    out = {0: _ld(x2), 3: np.sqrt(_ld(x2 / (n * min(r - 1, c - 1)))), 9: np.sqrt(_ld(x2 / (x2 + n)))}
    if r == 2 and c == 2:
        det = int(t[0, 0]) * int(t[1, 1]) - int(t[0, 1]) * int(t[1, 0])
        out[10] = np.longdouble(det) / np.sqrt(np.longdouble(rows[0] * rows[1] * cols[0] * cols[1]))
        if o.get("correction", False):
            out[0] = _ld(sum((abs(O - E) - min(Fraction(1, 2), abs(O - E))) ** 2 / E for O, E in cells))
    return out


def higher_precision(call, g):
    """{field: long double} of group g: the fields of its record that sums of the rows enter, recomputed in a wider arithmetic."""
    f, t, o = call["family"], call["test"], call["opts"]
    lo, hi = call["off"][g], call["off"][g + 1]
    if f == "cor":
        rec = COR.record(call["x"][lo:hi], call["y"][lo:hi], t, dtype=np.longdouble, **o)
        return {j: np.longdouble(rec[j]) for j in (0, 1, 3, 4)}
    if f == "rank":
        return _hp_rank(t, call["v"][lo:hi], call["y"][lo:hi], call["sample"][lo:hi], o)
    if f == "sample":
        return _hp_sample(t, call["v"][lo:hi], call["y"][lo:hi], call["sample"][lo:hi], o)
    if f == "normality":
        return _hp_normality(t, call["v"][lo:hi], o)
    return _hp_categorical(t, call["a"][lo:hi], call["b"][lo:hi], o)


def assert_input_conditions(call, ref=None, errs=None):
    """Every group of the call: the float64 restatement within a TENTH of check_records' bounds of its higher-precision form.  The
    family's own check is applied to ref + 10 (ref - hp), so the bounds are those of check_records, field by field; where one of
    the two is not finite both have to be the same.  -> the worst (ref - hp) per field, in check_records' units."""
    ref = reference(call) if ref is None else ref
    errs = {} if errs is None else errs
    status = STATUS[call["family"]]
    for g in range(len(ref)):
        if ref[g, status] != 0:
            continue
        what = (call["family"], call["test"], g, call["kinds"][g], call["sizes"][g])
        pseudo = ref[g].copy()
        for j, hp in higher_precision(call, g).items():
            r = ref[g, j]
            if np.isfinite(r) and np.isfinite(hp):
                pseudo[j] = np.float64(np.longdouble(r) + 10 * (np.longdouble(r) - hp))
            else:
                assert (np.isnan(r) and np.isnan(hp)) or r == hp, what + (j, r, hp)
        tenfold = {}
        try:
            check(call, pseudo[None, :], ref[g:g + 1], tenfold)
        except AssertionError as e:
            raise AssertionError("the restatement is not a referee for %r: %s" % (what, e)) from None
        for k, e in tenfold.items():
            errs[k] = max(errs.get(k, 0.0), e / 10.0)
    return errs
