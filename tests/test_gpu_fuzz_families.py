"""Randomised reference sweeps of the elastic net, bounded least squares and recursive least squares fits (run with -m gpu
on an MI355X): every group of every drawn batch against a row-based restatement that shares no code with the library —
tests/elasticnet_restate.py (extended precision), tests/bls_restate.py, tests/rls_restate.py (bit for bit).

A seed draws the width (every size class of the batch path: 1..8, 9..26, 27..42, 43..64, 65..128), a group count that is
never a multiple of 64 (several hundred at p <= 8: many wavefronts of the lane-per-group kernels, many workgroups), group
sizes (the SIZES of test_gpu_fuzz.py plus k + [intercept] - 1 (status 6), k + [intercept] (allowed), k + [intercept] + 1 and
5p), one of two regimes — more than 128 rows per group on average (the plain accumulate kernel) or at most 128 (the packed
small-group kernel) —, in one seed of eight a group of more than 8192 rows (row splitting), column scales and shifts, the
degenerate content of test_gpu_fuzz._case (without its weights) and an option set.  Tolerances are the project's
(conftest.assert_records_match / bls_restate.assert_record_matches): coefficients 1e-9 max(|ref_j|, 1e-3 max_k |ref_k|), the
intercept with its xbar allowance, diagnostics 1e-6 (1e-12 absolute for r2-like values), statuses, NaN patterns, counts and
flags exactly; groups without residual degrees of freedom on coefficients only.

Conditions on the INPUT are asserted on the restatement's output for every case (elasticnet_restate.input_conditions,
bls_restate.moment_conditions): no case is skipped, a seed that violates one fails.  The generator's ranges were tuned on
the CPU, where the restatements alone run, until every seed of the default run and of ANOFOX_FUZZ_SCALE=10 met them:
* a solver that sees only moments loses p kappa^2 2^-53, so designs are built well conditioned: groups with fewer than three
  rows per column get orthonormalised columns times a mild mixing matrix (a square Gaussian matrix has no bounded condition
  number), shifts shrink with sqrt(p), and an exactly aliased pair (kind 1 of _case: no unique minimiser, kappa infinite)
  is drawn as a strongly correlated pair instead;
* column scales are 10^U(a, a + 2) with a ~ U(-2, 1) per seed: the sweep covers 10^-2 .. 10^3, one design spans two decades —
  with five decades inside one design, ordinary shrinkage puts an active coefficient below 1e-6 of the largest one (the
  second input condition) in about one group in a hundred."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls_restate as br  # noqa: E402
import elasticnet_restate as er  # noqa: E402
import rls_restate as R  # noqa: E402
from conftest import assert_records_match, import_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SCALE = max(1, int(os.environ.get("ANOFOX_FUZZ_SCALE", "1")))

SIZES = [0, 1, 2, 3, 4, 5, 7, 9, 17, 50, 63, 64, 65, 127, 128, 129, 200, 256, 257, 400]      # test_gpu_fuzz.SIZES
CLASSES = [(1, 8), (9, 26), (27, 42), (43, 64), (65, 128)]
CLASS_OF_SEED = [0, 1, 0, 2, 0, 3, 0, 4, 0, 1]          # half the seeds at p <= 8, the rest over the wide classes
LONG_ROWS = 9000                                        # above the row-splitting threshold (8192)


@pytest.fixture(scope="module")
def pkg():
    return import_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


# ---- generator ---------------------------------------------------------------------------------------------------------

def _block(rng, n, k, icpt, rho, mu):
    """n x k columns of unit scale with means `mu`, well conditioned whatever n >= k + icpt is; with `rho` the later of two
    random columns becomes a strongly correlated companion of the other.  Groups with fewer than three rows per column get
    orthonormalised columns times a mild mixing matrix: centred ones plus the means with an intercept, the shifted columns
    themselves orthonormalised without one (a rank-one shift can make a square matrix singular)."""
    Z = rng.standard_normal((n, k))
    if rho and k >= 2:
        a, b = sorted(rng.choice(k, 2, replace=False))
        Z[:, b] = rho * Z[:, a] + np.sqrt(1.0 - rho * rho) * Z[:, b]
    if k and n >= k + icpt and n - icpt < 3 * k:
        Z = Z - Z.mean(axis=0) if icpt else Z + mu
        Z = np.sqrt(n) * np.linalg.qr(Z)[0] @ (np.eye(k) + 0.25 * rng.standard_normal((k, k)) / np.sqrt(k))
        return Z + mu if icpt else Z
    return Z + mu


def _shape(rng, cls, icpt, few_groups=False):
    lo, hi = CLASSES[cls]
    p = int(rng.integers(lo, hi + 1))
    plain = bool(rng.integers(0, 2))
    long_group = int(rng.integers(0, 8)) == 0 and p <= 42
    if p <= 8:
        G = int(rng.integers(65, 320))
    else:
        G = int(rng.integers(3, [0, 40, 14, 10, 6][cls]))
    if few_groups and p > 8:
        G = min(G, [0, 12, 6, 4, 2][cls])
    if long_group and not plain:           # the packed regime holds a long group only among many small ones
        long_group = p <= 8
        G = max(G, 90) if long_group else G
    G += 1 if G % 64 == 0 else 0
    sizes = SIZES + [p + icpt - 1, p + icpt, p + icpt + 1, 5 * p]
    ns = rng.choice(sizes, size=G)
    if plain:
        big = rng.random(G) < 0.6
        # (the BLS restatement refits its free set by lstsq every pass: its widest groups stay below 300 rows)
        ns = np.where(big, rng.choice([200, 250, 300] if few_groups and p > 42 else [300, 400, 500, 700, 1000], size=G), ns)
        if ns.mean() <= 128:
            ns[int(rng.integers(0, G))] += int(129 * G - ns.sum())
    g_long = int(rng.integers(0, G)) if long_group else -1
    if long_group:
        ns[g_long] = LONG_ROWS + int(rng.integers(0, 300))
    small = [3, 5, 9, 17, p + icpt + 1]
    while not plain and ns.mean() > 128:
        cand = np.where(np.arange(G) == g_long, -1, ns)
        ns[int(np.argmax(cand))] = int(rng.choice(small))
    assert (ns.mean() > 128) == plain and G % 64 != 0
    return p, G, ns.astype(np.int64), plain


def _rows(rng, p, ns, icpt):
    """(offsets, y, X) of a batch: per group the degenerate kind of test_gpu_fuzz._case, the invalid rows, then a well
    conditioned design on the valid rows."""
    G = len(ns)
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    N = int(offs[-1])
    a = rng.uniform(-2.0, 1.0)
    col_scale = 10.0 ** rng.uniform(a, a + 2.0, p)
    kmax = er.kappa_bound(p)
    smax = min(3.0, 0.04 * kmax / np.sqrt(p))
    mu = rng.choice([0.0, 0.0, min(1.0, 0.5 * smax), smax], p)          # the columns' shifts in units of their scales
    rho = 0.98 if p <= 42 else 0.9
    X = np.empty((N, p))
    y = np.empty(N)
    noise = 10.0 ** rng.uniform(-3, 0.5)
    for g in range(G):
        lo, hi = int(offs[g]), int(offs[g + 1])
        n = hi - lo
        if n == 0:
            continue
        kind = int(rng.integers(0, 10))
        invalid = np.zeros(n, dtype=bool)
        if kind == 2:
            invalid[rng.choice(n, size=max(1, n // 6), replace=False)] = True
        elif kind == 3:
            invalid[rng.choice(n, size=max(1, n // 8), replace=False)] = True
        const_col = int(rng.integers(0, p)) if kind == 0 else -1
        nv = int((~invalid).sum())
        keep = np.arange(p) != const_col
        Z = np.zeros((n, p))
        Z[np.ix_(~invalid, keep)] = _block(rng, nv, int(keep.sum()), icpt, rho if kind == 1 else 0.0, mu[keep])
        Z[invalid] = rng.standard_normal((n - nv, p)) + mu
        if const_col >= 0:
            Z[:, const_col] = rng.uniform(-3, 3)
        Xg = Z * col_scale
        u = rng.uniform(0.5, 3.0, p) * rng.choice([-1.0, 1.0], p)
        yg = rng.uniform(-5, 5) + Z @ u + noise * rng.standard_normal(n)
        if not icpt and nv <= 4:         # a y of two to four rows is nearly constant by chance: glmnet's sd_y would cancel
            yg += (2.0 * np.max(np.abs(yg)) + 1.0) * (-1.0) ** np.cumsum(~invalid)
        if kind == 2:
            yg[invalid] = np.nan
        elif kind == 3:
            Xg[invalid, int(rng.integers(0, p))] = rng.choice([np.nan, np.inf, -np.inf])
        X[lo:hi], y[lo:hi] = Xg, yg
    return offs, y, X


def _cols(X):
    return [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])]


def _xbar(res, Xg, p):
    if res["status"] != 0:
        return np.zeros(p)
    return np.abs(Xg[res["valid"]]).mean(axis=0)


def _worst_coef(core, rcore, p):
    """The largest coefficient error of a batch as a multiple of its tolerance (reported, not asserted here)."""
    ok = rcore[:, p + 5] == 0
    rc, c = rcore[ok, :p], core[ok, :p]
    if not rc.size or np.all(np.isnan(rc)):
        return 0.0
    with np.errstate(all="ignore"):
        scale = np.nanmax(np.abs(rcore[ok, :p + 1]), axis=1, keepdims=True)
        scale = np.where(np.isfinite(scale), scale, 0.0)
        ratio = np.abs(c - rc) / np.maximum(1e-9 * np.maximum(np.abs(rc), 1e-3 * scale), 1e-300)
    return float(np.nanmax(ratio)) if np.any(~np.isnan(ratio)) else 0.0


# ---- elastic net ---------------------------------------------------------------------------------------------------------

def _en_case(seed):
    rng = np.random.default_rng(seed)
    icpt = bool(rng.integers(0, 2))
    p, G, ns, plain = _shape(rng, CLASS_OF_SEED[seed % 10], int(icpt))
    offs, y, X = _rows(rng, p, ns, int(icpt))
    scaling = str(rng.choice(["raw", "glmnet"]))
    l1 = [0.0, float(rng.uniform(0.05, 0.95)), 1.0][int(rng.integers(0, 3))]
    # alpha as a multiple of the median group's lambda_max (in alpha's units): 0, inside, and beyond it — lambda_max grows with
    # the group's row count, so every alpha > 0 lies beyond the lambda_max of the batch's smallest groups
    lmax = []
    for g in range(G):
        s = slice(offs[g], offs[g + 1])
        ok = np.isfinite(y[s]) & np.isfinite(X[s]).all(axis=1)
        if ok.sum() < p + 2:
            continue
        yv, Xv = y[s][ok], X[s][ok]
        yc, Xc = (yv - yv.mean(), Xv - Xv.mean(axis=0)) if icpt else (yv, Xv)
        lm = float(np.max(np.abs(Xc.T @ yc))) / max(l1, 1e-3)
        if scaling == "glmnet":
            lm *= np.std(yv) / len(yv)
        lmax.append(lm)
    base = float(np.median(lmax)) if lmax else 1.0
    f = [0.0, 10.0 ** rng.uniform(-3, 0), rng.uniform(1.0, 2.0)][int(rng.choice(3, p=[0.15, 0.6, 0.25]))]
    kw = dict(alpha=float(f * base), l1_ratio=l1, fit_intercept=icpt, lambda_scaling=scaling)
    return p, offs, y, X, kw, plain


def _en_restate(p, offs, y, X, kw, what, rule_counts=None):
    """Restated records of every group, the input conditions asserted; (rcore, zero-df groups, xbar, restated fits)."""
    G = len(offs) - 1
    rcore, xbar, skip, fits = np.empty((G, p + 6)), np.zeros((G, p)), [], []
    for g in range(G):
        s = slice(offs[g], offs[g + 1])
        res = er.fit_en(y[s], X[s], rule_count=None if rule_counts is None else int(rule_counts[g]), **kw)
        assert er.input_conditions(res, y[s], X[s]) == [], f"{what} group {g} (n = {offs[g + 1] - offs[g]})"
        rcore[g], xbar[g] = er.record(res), _xbar(res, X[s], p)
        if res["status"] == 0 and res["df"] <= 0:
            skip.append(g)
        fits.append(res)
    return rcore, skip, xbar, fits


def _run_en(pkg, ctx, seed, record_property=None):
    p, offs, y, X, kw, plain = _en_case(seed)
    what = f"elastic net seed {seed} p={p} G={len(offs) - 1} {'plain' if plain else 'packed'} {kw}"
    rcore, skip, xbar, fits = _en_restate(p, offs, y, X, kw, what)
    o = pkg.ElasticNetOptions(tolerance=1e-14, max_iterations=2_000_000, **kw).batch_options()
    core, its = pkg.elasticnet_fit_batch_host(offs, y, _cols(X), o, ctx=ctx)
    if record_property is not None:
        record_property("worst_coef_x_tol", _worst_coef(core, rcore, p))
        record_property("groups", len(offs) - 1)
    assert_records_match(core, rcore, p, what=what, skip_diag_groups=skip, xbar=xbar)
    # converged: a positive sweep count for every status-0 group (the intercept-only shortcut runs no solve and reports 0)
    solved = [g for g, r in enumerate(fits) if r["status"] == 0 and not r["shortcut"]]
    assert np.all(its[solved] > 0), f"{what}: not converged at groups {[g for g in solved if its[g] <= 0][:10]}"
    assert np.all(its[[g for g, r in enumerate(fits) if r["status"] == 0 and r["shortcut"]]] == 0), what


@pytest.mark.parametrize("seed", range(40 * _SCALE))
def test_fuzz_elasticnet(pkg, ctx, seed, record_property):
    _run_en(pkg, ctx, 110_000 + seed, record_property)


# ---- bounded least squares -----------------------------------------------------------------------------------------------

def _bls_case(seed):
    rng = np.random.default_rng(seed)
    icpt = bool(rng.integers(0, 2))
    p, G, ns, plain = _shape(rng, CLASS_OF_SEED[seed % 10], int(icpt), few_groups=True)
    offs, y, X = _rows(rng, p, ns, int(icpt))
    cs = np.array([np.nanstd(np.where(np.isfinite(c), c, np.nan)) for c in X.T])        # the columns' scales: bounds that bind
    cs = np.where(cs > 0, cs, 1.0)
    m = float(np.median(1.0 / cs))
    variants = [("nnls", None, None), ("lower", -0.5 * m, None), ("upper", None, 0.25 * m), ("box", -1.0 * m, 1.5 * m),
                ("per_column", rng.uniform(-2.0, -0.1, size=p) / cs, rng.uniform(0.1, 2.0, size=p) / cs),
                ("per_column_mixed", np.where(rng.random(p) < 0.3, -np.inf, rng.uniform(-3.0, 1.0, size=p) / cs),
                 np.where(rng.random(p) < 0.3, np.inf, rng.uniform(1.5, 4.0, size=p) / cs))]
    name, lo, hi = variants[int(rng.integers(0, len(variants)))]
    return p, offs, y, X, dict(fit_intercept=icpt, lower_bound=lo, upper_bound=hi), plain, name


def _bls_restate(p, offs, y, X, kw, what, rule_counts=None):
    fits = []
    for g in range(len(offs) - 1):
        s = slice(offs[g], offs[g + 1])
        res = br.fit_bls(y[s], X[s], kw["fit_intercept"], kw["lower_bound"], kw["upper_bound"],
                         rule_count=None if rule_counts is None else int(rule_counts[g]))
        assert br.moment_conditions(res, y[s], X[s], kw["fit_intercept"]) == [], f"{what} group {g} (n = {offs[g + 1] - offs[g]})"
        fits.append(res)
    return fits


def _run_bls(pkg, ctx, seed, record_property=None):
    p, offs, y, X, kw, plain, name = _bls_case(seed)
    what = f"bls seed {seed} p={p} G={len(offs) - 1} {'plain' if plain else 'packed'} {name} intercept={kw['fit_intercept']}"
    fits = _bls_restate(p, offs, y, X, kw, what)
    rec, its = pkg.bls_fit_batch_host(offs, y, _cols(X), pkg.BlsOptions(**kw).batch_options(), ctx=ctx)
    rrec = np.array([br.record(r) for r in fits]).reshape(len(fits), 3 * p + 6)
    if record_property is not None:
        record_property("worst_coef_x_tol", _worst_coef(rec[:, :p + 6], rrec[:, :p + 6], p))
        record_property("groups", len(fits))
    for g, res in enumerate(fits):
        s = slice(offs[g], offs[g + 1])
        br.assert_record_matches(rec[g], rrec[g], p, xbar=_xbar(res, X[s], p) if res["status"] == 0 else None, what=f"{what} group {g}")
        if res["status"] == 0:
            assert its[g] >= 0, f"{what} group {g}: the iteration limit stopped the solve"


@pytest.mark.parametrize("seed", range(30 * _SCALE))
def test_fuzz_bls(pkg, ctx, seed, record_property):
    _run_bls(pkg, ctx, 120_000 + seed, record_property)


# ---- recursive least squares ---------------------------------------------------------------------------------------------

def _rls_case(seed):
    rng = np.random.default_rng(seed)
    narrow = seed % 4 != 3
    p = int(rng.integers(1, 9)) if narrow else int(rng.integers(9, 34))
    G = int(rng.integers(65, 300)) if narrow else int(rng.integers(3, 20))
    G += 1 if G % 64 == 0 else 0
    ns = rng.choice([0, 1, 2, 3, 4, 5, 7, 9, 17, p, p + 1, p + 2, 2 * p + 3, 40, 64, 65], size=G)
    budget = 5000 if narrow else 600                        # rows the Python restatement walks in seconds
    while ns.sum() > budget:
        ns[int(np.argmax(ns))] = int(rng.choice([1, 2, 3, 5]))
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    N = int(offs[-1])
    X = rng.standard_normal((N, p)) * 10.0 ** rng.uniform(-1, 1, p) + rng.choice([0.0, 1.0, 5.0], p)
    y = X @ rng.uniform(-2, 2, p) + rng.uniform(-3, 3) + 0.3 * rng.standard_normal(N)
    for g in range(G):
        lo, hi = int(offs[g]), int(offs[g + 1])
        if hi == lo:
            continue
        kind = int(rng.integers(0, 8))
        if kind == 0:
            X[lo:hi, rng.integers(0, p)] = rng.uniform(-3, 3)
        elif kind == 1:
            X[lo:hi, :] = rng.uniform(-3, 3, p)                                  # every column constant: the shortcut / status 6
        elif kind == 2:
            y[lo + rng.choice(hi - lo, size=max(1, (hi - lo) // 6), replace=False)] = rng.choice([np.nan, np.inf])
        elif kind == 3:
            X[lo + rng.choice(hi - lo, size=max(1, (hi - lo) // 8), replace=False), rng.integers(0, p)] = rng.choice([np.nan, np.inf, -np.inf])
        elif kind == 4:
            y[lo:hi] = np.nan                                                    # no valid row
    kw = dict(forgetting_factor=float(rng.choice([1.0, rng.uniform(0.9, 1.0)])), initial_p_diagonal=float(10.0 ** rng.uniform(-1, 3)),
              fit_intercept=bool(rng.integers(0, 2)))
    return p, offs, y, X, kw


@pytest.mark.parametrize("seed", range(24 * _SCALE))
def test_fuzz_rls(pkg, ctx, seed):
    p, offs, y, X, kw = _rls_case(130_000 + seed)
    core = pkg.rls_fit_batch_host(offs, y, _cols(X), pkg.RlsOptions(**kw).batch_options(), ctx=ctx)
    want = R.batch(offs, y, _cols(X), **kw)
    got = np.ascontiguousarray(core, dtype=np.float64)
    assert got.shape == want.shape
    bad = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[0]
    assert bad.size == 0, f"rls seed {seed} p={p} G={len(offs) - 1} {kw}: records differ at groups {bad[:10]}"


# ---- fit-predict ---------------------------------------------------------------------------------------------------------

def _fit_predict_case(seed):
    """Shapes of test_gpu_fuzz.test_fuzz_fit_predict: rows with a NULL y are predicted only, NULL features drop a row."""
    rng = np.random.default_rng(seed)
    icpt = bool(rng.integers(0, 2))
    p = int(rng.integers(1, 13))
    G = int(rng.integers(1, 30))
    ns = rng.choice([0, 1, 2, 3, 5, p + 1, p + 2, 2 * p + 3, 40, 127, 128, 129, 300], size=G)
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    N = int(offs[-1])
    col_scale = 10.0 ** rng.uniform(-1, 1, p)
    mu = rng.choice([0.0, 1.0, 3.0], p)
    hold = rng.random(N) < 0.2
    null_x = rng.random(N) < 0.01
    X, y = np.empty((N, p)), np.empty(N)
    for g in range(G):
        lo, hi = int(offs[g]), int(offs[g + 1])
        tr = ~(hold[lo:hi] | null_x[lo:hi])
        Z = rng.standard_normal((hi - lo, p)) + mu
        Z[tr] = _block(rng, int(tr.sum()), p, int(icpt), 0.0, mu)
        X[lo:hi] = Z * col_scale
        u = rng.uniform(0.5, 3.0, p) * rng.choice([-1.0, 1.0], p)
        y[lo:hi] = rng.uniform(-5, 5) + Z @ u + 0.3 * rng.standard_normal(hi - lo)
    y[hold] = np.nan
    X[null_x, int(rng.integers(0, p))] = np.nan
    counts = np.array([int(np.sum(~np.isnan(y[offs[g]:offs[g + 1]]))) for g in range(G)], dtype=np.int64)
    return rng, p, offs, y, X, icpt, counts, float(rng.choice([0.8, 0.95]))


def _interval(pkg, yhat, sigma, n, p, icpt, df, conf):
    """anofox_predict_with_interval's simplified interval: yhat -+ t(df) sigma sqrt(1 + 1/n), bounds = yhat without a sigma."""
    out = np.full((len(yhat), 3), np.nan)
    margin = 0.0
    if not (np.isnan(sigma) or sigma <= 0 or n <= p + 1) and df > 0:
        margin = pkg.t_critical(conf, int(df)) * sigma * np.sqrt(1.0 + 1.0 / n)
    fin = np.isfinite(yhat)
    out[fin] = np.stack([yhat[fin], yhat[fin] - margin, yhat[fin] + margin], axis=1)
    return out


def _assert_pred(pred, ref, what):
    assert np.array_equal(np.isnan(pred), np.isnan(ref)), f"{what}: NULL pattern"
    m = ~np.isnan(ref[:, 0])
    scale = np.maximum(np.abs(ref[m, 0]), 1.0)
    assert m.sum() == 0 or (np.abs(pred[m, 0] - ref[m, 0]) / scale).max() < 1e-8, f"{what}: yhat"
    for k in (1, 2):
        assert m.sum() == 0 or (np.abs(pred[m, k] - ref[m, k]) / scale).max() < 1e-6, f"{what}: bound {k}"


@pytest.mark.parametrize("seed", range(12 * _SCALE))
def test_fuzz_elasticnet_fit_predict(pkg, ctx, seed):
    rng, p, offs, y, X, icpt, counts, conf = _fit_predict_case(140_000 + seed)
    kw = dict(alpha=float(10.0 ** rng.uniform(-2, 1.5)), l1_ratio=float(rng.choice([0.0, rng.uniform(0.05, 0.95), 1.0])),
              fit_intercept=icpt, lambda_scaling=str(rng.choice(["raw", "glmnet"])))
    if kw["lambda_scaling"] == "glmnet":
        kw["alpha"] /= 100.0
    what = f"elastic net fit_predict seed {seed} p={p} {kw}"
    rcore, skip, xbar, fits = _en_restate(p, offs, y, X, kw, what, rule_counts=counts)
    o = pkg.ElasticNetOptions(tolerance=1e-14, max_iterations=2_000_000, **kw).batch_options()
    core, pred = pkg.elasticnet_fit_predict_batch_host(offs, y, _cols(X), o, conf, train_counts=counts, ctx=ctx)
    assert_records_match(core, rcore, p, what=what, skip_diag_groups=skip, xbar=xbar)
    for g, res in enumerate(fits):
        s = slice(offs[g], offs[g + 1])
        if res["status"] != 0:
            assert np.all(np.isnan(pred[s])), f"{what} group {g}: a failed fit predicts NULL"
            continue
        if g in skip:
            continue                                                        # zero residual df: sigma is 0/0
        b = np.where(np.isnan(res["coefficients"]), 0.0, res["coefficients"])
        yhat = (res["intercept"] if icpt else 0.0) + np.where(np.isnan(res["coefficients"])[None, :], 0.0, X[s]) @ b
        n = res["n_observations"]
        ref = _interval(pkg, yhat, res["residual_std_error"], n, p, icpt, n - (p + (1 if icpt else 0)), conf)
        _assert_pred(pred[s], ref, f"{what} group {g}")


@pytest.mark.parametrize("seed", range(12 * _SCALE))
def test_fuzz_bls_fit_predict(pkg, ctx, seed):
    rng, p, offs, y, X, icpt, counts, conf = _fit_predict_case(150_000 + seed)
    with np.errstate(all="ignore"):
        sd = np.nanstd(X, axis=0) if len(X) else np.ones(p)
    cs = 1.0 / np.where(sd > 0, sd, 1.0)
    lo, hi = [(None, None), (-0.5 * np.median(cs), 0.8 * np.median(cs)), (rng.uniform(-2.0, -0.1, p) * cs, rng.uniform(0.1, 2.0, p) * cs)][int(rng.integers(0, 3))]
    kw = dict(fit_intercept=icpt, lower_bound=lo, upper_bound=hi)
    what = f"bls fit_predict seed {seed} p={p} intercept={icpt}"
    fits = _bls_restate(p, offs, y, X, kw, what, rule_counts=counts)
    core, pred = pkg.bls_fit_predict_batch_host(offs, y, _cols(X), pkg.BlsOptions(**kw).batch_options(), conf, train_counts=counts, ctx=ctx)
    for g, res in enumerate(fits):
        s = slice(offs[g], offs[g + 1])
        assert core[g, p + 5] == res["status"], f"{what} group {g}: status"
        if res["status"] != 0:
            assert np.all(np.isnan(pred[s])), f"{what} group {g}: a failed fit predicts NULL"
            continue
        n = res["n_observations"]
        df = (n - p - (1 if icpt else 0)) % (1 << 64)                       # the reference's unsigned df over ALL columns
        if n - int((~res["const"]).sum()) - (1 if icpt else 0) <= 0 and not np.isnan(res["ssr"]):
            continue                                                        # an exact fit: ssr, hence sigma, is rounding noise
        b = np.where(np.isnan(res["coefficients"]), 0.0, res["coefficients"])
        yhat = (res["intercept"] if icpt else 0.0) + np.where(np.isnan(res["coefficients"])[None, :], 0.0, X[s]) @ b
        sigma = np.sqrt(res["ssr"] / df) if df > 0 and res["ssr"] >= 0 else np.nan
        _assert_pred(pred[s], _interval(pkg, yhat, sigma, n, p, icpt, df, conf), f"{what} group {g}")


# ---- the benchmark shape: p = 8, 1000 rows per group, the plain accumulate kernel with and without the fused solve --------

BENCH_G, BENCH_N, BENCH_P = 1003, 1000, 8


def _bench_batch():
    rng = np.random.default_rng(160_000)
    offs = (np.arange(BENCH_G + 1) * BENCH_N).astype(np.int64)
    X = rng.standard_normal((BENCH_G * BENCH_N, BENCH_P)) * 10.0 ** rng.uniform(-1, 1, BENCH_P) + rng.uniform(-2, 2, BENCH_P)
    gid = np.repeat(np.arange(BENCH_G), BENCH_N)
    beta = rng.uniform(0.5, 3.0, (BENCH_G, BENCH_P)) * rng.choice([-1.0, 1.0], (BENCH_G, BENCH_P))
    y = rng.uniform(-5, 5, BENCH_G)[gid] + np.einsum("ij,ij->i", X, beta[gid]) + rng.standard_normal(len(gid))
    return offs, y, X


def _bench_options(icpt):
    return (dict(alpha=150.0, l1_ratio=0.5, fit_intercept=icpt, lambda_scaling="raw"),
            dict(fit_intercept=icpt, lower_bound=-1.0, upper_bound=2.0))


def _bench_child(out_path):
    sys.path.insert(0, ROOT)
    pkg = import_pkg()
    offs, y, X = _bench_batch()
    c = pkg.Context()
    res = {}
    try:
        for icpt in (True, False):
            en, bls = _bench_options(icpt)
            o = pkg.ElasticNetOptions(tolerance=1e-14, max_iterations=2_000_000, **en).batch_options()
            res[f"en{int(icpt)}"], res[f"en_its{int(icpt)}"] = pkg.elasticnet_fit_batch_host(offs, y, _cols(X), o, ctx=c)
            res[f"bls{int(icpt)}"], res[f"bls_its{int(icpt)}"] = pkg.bls_fit_batch_host(offs, y, _cols(X), pkg.BlsOptions(**bls).batch_options(), ctx=c)
    finally:
        c.close()
    np.savez(out_path, **res)


def test_benchmark_shape_against_restatements(tmp_path):
    """1003 groups x 1000 rows x 8 columns, elastic net and BLS, with and without an intercept: every group against its
    restatement, and the same bits with ANOFOX_NARROW_FUSED=0 (read once per process: each side in a child of its own)."""
    runs = {}
    for name, fused in (("fused", "1"), ("separate", "0")):
        out = tmp_path / f"{name}.npz"
        subprocess.run([sys.executable, os.path.abspath(__file__), str(out)], env=dict(os.environ, ANOFOX_NARROW_FUSED=fused),
                       check=True, timeout=600)
        runs[name] = np.load(out)
    a, b = runs["fused"], runs["separate"]
    for k in a.files:
        assert a[k].tobytes() == b[k].tobytes(), f"{k}: ANOFOX_NARROW_FUSED=0 changes the records"
    offs, y, X = _bench_batch()
    p = BENCH_P
    for icpt in (True, False):
        en, bls = _bench_options(icpt)
        what = f"benchmark shape elastic net intercept={icpt}"
        rcore, skip, xbar, fits = _en_restate(p, offs, y, X, en, what)
        assert_records_match(a[f"en{int(icpt)}"], rcore, p, what=what, skip_diag_groups=skip, xbar=xbar)
        assert np.all(a[f"en_its{int(icpt)}"] > 0)
        what = f"benchmark shape bls intercept={icpt}"
        for g, res in enumerate(_bls_restate(p, offs, y, X, bls, what)):
            s = slice(offs[g], offs[g + 1])
            br.assert_record_matches(a[f"bls{int(icpt)}"][g], br.record(res), p, xbar=_xbar(res, X[s], p), what=f"{what} group {g}")
            assert a[f"bls_its{int(icpt)}"][g] >= 0


# ---- beyond the glmnet boundary -------------------------------------------------------------------------------------------

def test_glmnet_without_intercept_beyond_the_cancellation_boundary(pkg, ctx):
    """lambda_scaling = glmnet without an intercept and q_yy >= 1e4 c_yy (a y nearly constant far from zero): DESIGN.md
    promises no more than that lambda = n alpha / sd_y carries the digits  c_yy = q_yy - s_y^2 / n  loses.  Sums of n doubles
    carry a few ulps each, so c_yy is off by at most 32 ulps of q_yy, sd_y and lambda by half that relatively:
    delta = 16 * 2^-53 q_yy / c_yy.  The record must lie within the ordinary 1e-9 of the interval the restatement spans
    between lambda (1 - delta) and lambda (1 + delta); statuses and n exactly."""
    rng = np.random.default_rng(170_000)
    p, n, G = 4, 200, 70
    offs = (np.arange(G + 1) * n).astype(np.int64)
    X = rng.standard_normal((G * n, p)) + 1.0
    y = 5000.0 + X @ np.array([1.5, -2.0, 0.7, 1.1]) + 0.5 * rng.standard_normal(G * n)
    kw = dict(alpha=0.02, l1_ratio=0.5, fit_intercept=False, lambda_scaling="glmnet")
    o = pkg.ElasticNetOptions(tolerance=1e-14, max_iterations=2_000_000, **kw).batch_options()
    core, its = pkg.elasticnet_fit_batch_host(offs, y, _cols(X), o, ctx=ctx)
    for g in range(G):
        s = slice(offs[g], offs[g + 1])
        mid = er.fit_en(y[s], X[s], **kw)
        assert mid["q_yy"] >= 1e4 * mid["c_yy"]
        assert er.input_conditions(mid, y[s], X[s]) == ["glmnet scaling without an intercept with q_yy >= 1e4 c_yy"]
        delta = 16.0 * 2.0 ** -53 * mid["q_yy"] / mid["c_yy"]
        lo_b = er.fit_en(y[s], X[s], lambda_factor=1.0 - delta, **kw)["coefficients"]
        hi_b = er.fit_en(y[s], X[s], lambda_factor=1.0 + delta, **kw)["coefficients"]
        ref = mid["coefficients"]
        tol = 1e-9 * np.maximum(np.abs(ref), 1e-3 * np.max(np.abs(ref))) + np.abs(hi_b - lo_b)
        assert core[g, p + 5] == 0 and core[g, p + 4] == n and its[g] > 0
        assert np.all(np.abs(core[g, :p] - ref) <= tol), (g, np.max(np.abs(core[g, :p] - ref) / tol), delta)


if __name__ == "__main__":
    _bench_child(sys.argv[1])
