"""The inputs of tests/test_gpu_state_models.py (and of the CPU check that they meet the restatements' input conditions):
rows of a streaming state's slots in shuffled arrival order, the same rows grouped for the batch entry points, the option
sets, and the restated records.  No GPU here.

Shapes: p in {1, 3, 8} (moment states) and {9, 33} (log-only states); 65 or 130 slots (never a multiple of 64); 0, 1, 2,
k + [intercept], k + [intercept] + 1 and up to 40 rows per slot plus one slot of 9000 rows (above the 8192-row split); the
designs, NaN y / NaN x rows and constant columns of test_gpu_fuzz_families._rows (well conditioned: a solver of moments is
held to 1e-9), and rows with valid = 0."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls_restate as br  # noqa: E402
import elasticnet_restate as er  # noqa: E402
import test_gpu_fuzz_families as F  # noqa: E402  (the generator and the restatement drivers; nothing in it runs on import)

MOMENT_P = [1, 3, 8]
LOG_ONLY_P = [9, 33]
LONG_ROWS = 9000
CHUNKS = [2048, 1, 7, 64]
EXACT_X = 8                                              # exact-fit slots: whole-number features in [-8, 8]

# state vs restatement: what test_gpu_fuzz_families applies to the batch entry points (conftest.COEF_RTOL / DIAG_RTOL, the
# defaults of assert_records_match and bls_restate.assert_record_matches)
# state vs batch call: what test_gpu_streaming applies between a regression state and its batch call
# (test_retained_rows_refit_queued_groups: coef_rtol=1e-10, diag_rtol=1e-8)
STATE_VS_BATCH = dict(coef_rtol=1e-10, diag_rtol=1e-8)


def n_slots_for(p):
    return 130 if p == 3 else 65


def seed_for(family, p, icpt, exact=False):
    return 7_000_000 + 1000 * ["elasticnet", "bls"].index(family) + 10 * p + int(icpt) + (500 if exact else 0)


class Case:
    pass


def make_case(family, p, icpt, exact=False):
    """exact: every third slot with residual degrees of freedom gets y = b0 + X b exactly (b inside the bounds), so that the
    moment-form ssr cancels and the family's solve flags it.  Exactly means in whole numbers (|x| <= EXACT_X, b in 1..3, b0 in
    1..5): every product and every sum of up to 9000 of them is a whole number far below 2^53, so the slot's moments are the
    same bits in whatever order a kernel sums them.  The residual of an exact fit is nothing but rounding: with real-valued
    rows its sigma follows the last bits of the coefficients, and those follow the summation order of the moments, which the
    batch call itself chooses by the mean group size of the batch it is handed (packed small-group kernel or one wavefront
    per group).  A state's refit of the flagged slots and the batch call on all slots are batches of different composition,
    so sigma of such a slot is comparable between them only where the order cannot matter."""
    rng = np.random.default_rng(seed_for(family, p, icpt, exact))
    S = n_slots_for(p)
    k = p + int(icpt)
    sizes = [0, 1, 2, k, k + 1, 5, 9, 17, 30, 40]
    ns = rng.choice(sizes + [k + 2, 17, 30, 35, 40, 40], size=S)       # (most slots have residual degrees of freedom)
    ns[:len(sizes)] = sizes
    ns[S - 3] = LONG_ROWS
    ns = ns.astype(np.int64)
    offs, y, X = F._rows(rng, p, ns, int(icpt))
    slot_of = np.repeat(np.arange(S, dtype=np.uint32), ns)
    X[offs[8], 0] = np.nan                               # the special slots: a NaN x element (slot 8, 30 rows) ...
    y[offs[9]] = np.nan                                  # ... and a NaN y (slot 9, 40 rows)
    exact_slots = []
    if exact:
        for g in range(0, S, 3):
            if ns[g] < k + 2:
                continue
            s = slice(offs[g], offs[g + 1])
            X[s] = np.where(np.isnan(X[s]), np.nan, rng.integers(-EXACT_X, EXACT_X + 1, X[s].shape))
            b = rng.integers(1, 4, p).astype(np.float64)
            yy = (float(rng.integers(1, 6)) if icpt else 0.0) + X[s] @ b
            y[s] = np.where(np.isnan(y[s]), np.nan, yy)
            exact_slots.append(g)
    valid = (rng.random(len(y)) > 0.02).astype(np.uint8)
    valid[offs[S - 5]:offs[S - 4]] = 0                  # one slot whose rows are all skipped by Update
    valid[offs[8]] = valid[offs[9]] = 1                  # (the two NaN rows reach the state)
    perm = rng.permutation(len(y))                       # arrival order: shuffled across slots
    c = Case()
    c.family, c.p, c.icpt, c.S = family, p, icpt, S
    c.slot, c.y, c.X, c.valid = slot_of[perm], y[perm], np.ascontiguousarray(X[perm]), valid[perm]
    # the same rows as the batch entry points take them: Update's skipped rows left out, slots contiguous, arrival order inside
    keep = np.nonzero(c.valid != 0)[0]
    order = keep[np.argsort(c.slot[keep], kind="stable")]
    c.gy, c.gX = c.y[order], np.ascontiguousarray(c.X[order])
    cnt = np.bincount(c.slot[order], minlength=S)
    c.goffs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    c.exact_slots = np.array(exact_slots, dtype=np.int64)
    c.kw = options(c)
    return c


def options(c):
    """Keyword arguments of ElasticNetOptions / BlsOptions for a case."""
    if c.family == "elasticnet":
        if len(c.exact_slots):
            # lambda = 0+: a penalty whose shrinkage (lambda / C_jj ~ 1e-15) leaves the moment-form rss far below 1e-7 tss
            return dict(alpha=1e-12, l1_ratio=0.5, fit_intercept=c.icpt, lambda_scaling="raw")
        return dict(alpha=alpha_grid(c)[0], l1_ratio=0.5, fit_intercept=c.icpt, lambda_scaling="raw")
    if c.icpt and not len(c.exact_slots):                 # a box that binds; NNLS without an intercept
        sd = np.array([np.nanstd(np.where(np.isfinite(col), col, np.nan)) for col in c.gX.T])
        m = float(np.median(1.0 / np.where(sd > 0, sd, 1.0)))
        return dict(fit_intercept=True, lower_bound=-1.0 * m, upper_bound=1.5 * m)
    return dict(fit_intercept=c.icpt, lower_bound=None, upper_bound=None)


def alpha_grid(c):
    """Two penalties inside the median slot's lambda_max (test_gpu_fuzz_families._en_case's scale)."""
    lmax = []
    for g in range(c.S):
        s = slice(c.goffs[g], c.goffs[g + 1])
        ok = np.isfinite(c.gy[s]) & np.isfinite(c.gX[s]).all(axis=1)
        if ok.sum() < c.p + 2:
            continue
        yv, Xv = c.gy[s][ok], c.gX[s][ok]
        yc, Xc = (yv - yv.mean(), Xv - Xv.mean(axis=0)) if c.icpt else (yv, Xv)
        lmax.append(float(np.max(np.abs(Xc.T @ yc))) / 0.5)
    base = float(np.median(lmax)) if lmax else 1.0
    return [0.05 * base, 0.3 * base]


def restate(c):
    """The restated records of the grouped rows, with the input conditions asserted (a violated one fails, it never skips):
    elastic net -> (rcore, zero-df groups, xbar); bls -> (rrec, fits)."""
    what = f"{c.family} p={c.p} intercept={c.icpt}"
    if c.family == "elasticnet":
        rcore, skip, xbar, _ = F._en_restate(c.p, c.goffs, c.gy, c.gX, c.kw, what)
        return rcore, skip, xbar
    fits = F._bls_restate(c.p, c.goffs, c.gy, c.gX, c.kw, what)
    return np.array([br.record(r) for r in fits]).reshape(c.S, 3 * c.p + 6), fits


_CACHE = {}


def cached(family, p, icpt, exact=False, restated=False):
    """A case (and its restatement) computed once per process and shared by the tests that need it; never modified."""
    key = (family, p, bool(icpt), bool(exact))
    if key not in _CACHE:
        _CACHE[key] = [make_case(family, p, icpt, exact), None]
    ent = _CACHE[key]
    if restated and ent[1] is None:
        ent[1] = restate(ent[0])
    return (ent[0], ent[1]) if restated else ent[0]
