"""The randomised cases of the quantile regression sweeps (tests/test_quantile_fuzz_cpu.py on the host build of
csrc/quantile_solve.h, tests/test_gpu_fuzz_quantile.py on the MI355X) and the assertions both make on a record.  A plain
module: the reference of every group comes from tests/quantile_restate.py::solve (interior point + crossover, numpy only)
and is cached per seed, so that the tests of one module share one solve; the arrays of a case are read-only.

A seed draws
  width       p in the classes 1-8, 9-16, 17-32 (half the seeds at p <= 8); p = 31 and p = 32 with an intercept and p = 32
              without one (k = 32 and 33, the most the work memory holds) are forced in seeds 3, 7 and 11;
  tau         one of 0.01 0.05 0.1 0.25 0.5 0.75 0.9 0.95 0.99 or U(0.02, 0.98); a path draws T in {1, 2, 7, 19, 64} of them,
              unsorted, in some seeds with duplicates and with one to three invalid entries (0, 1, NaN, -0.1);
  group sizes from 0 1 k-1 k k+1 2k 63 64 65 127 128 129 5k 300 1000 (each once where the call has that many groups, the rest
              weighted towards the small ones: the numpy reference is the cost of a test); 65-200 groups at p <= 8, 3-20
              above; one seed in eight at p <= 8 has a group of about 5000 rows;
  content     column scales 10^U(a, a+2), a ~ U(-2, 1), shifts of 0, 0.5 or 2 column scales, Student-t(3) or heteroscedastic
              noise of scale 10^U(-3, 0.5), a y offset of 0 (half the seeds) or U(0, 100) noise scales;
  per group   one KIND: plain / invalid rows (NaN y, NaN or +-inf in an x) / all y NaN / duplicated rows / a constant column
              (aliased with an intercept) / an exactly aliased pair / lattice (small integer x and y: ties, more than k zero
              residuals at the optimum, rank deficiency at small n).

What a record has to meet is check_sweep_record's docstring.  Conditions on the INPUT are asserted on the reference alone by
assert_input_conditions, for every case: none is skipped, a seed that breaks one fails.  The generator's ranges were set on the
CPU until every seed of the default runs and of ANOFOX_FUZZ_SCALE=10 met them; nothing of the issue's ranges had to shrink:
with a y offset of up to 100 noise scales and 5000 rows the smallest residual off the basis stays above 1e-8 max|y| (the
expected smallest of n residuals is about sigma / n, i.e. 2e-6 max|y| there), and the uncompared share of the continuous groups
(mostly square-ish wide groups whose A_Z has kappa > 1e4) stays below the 5 % cap.

The refined-vertex condition (double solve and its extended-precision refinement within 1e-11, in column units) is asserted
on every unique group with kappa <= 1e4, whatever its rmin: there the double solve errs by about kappa 2^-53 <= 1e-12 in
practice.  A unique group with a larger kappa is outside the coefficient comparison, a k x k solve in double cannot agree with
its refinement to 1e-11 there and nothing rests on it: such groups are held to the loss and the certificate."""
import functools
import os

import numpy as np

import quantile_restate as qr

SCALE = max(1, int(os.environ.get("ANOFOX_FUZZ_SCALE", "1")))

TAU_SET = [0.01, 0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95, 0.99]
CLASSES = [(1, 8), (9, 16), (17, 32)]
CLASS_OF_SEED = [0, 1, 0, 2]
FORCED = {3: (31, True), 7: (32, True), 11: (32, False)}     # seed -> (p, intercept): k = 32, 33, 32
PATH_T = [7, 1, 19, 2, 64]
LONG_ROWS = 5000
KINDS = ("plain", "invalid", "all_nan", "duplicates", "constant", "aliased", "lattice")
KIND_P = (0.40, 0.15, 0.04, 0.10, 0.08, 0.08, 0.15)
CONTINUOUS = ("plain", "invalid")
RANK_KINDS = ("constant", "aliased")

KAPPA_MAX = 1e4
RMIN_MIN = 1e-8
COEF_TOL = 1e-9
UNCOMPARED_CAP = 0.05


def _tau(rng):
    return float(rng.choice(TAU_SET)) if rng.random() < 0.6 else float(rng.uniform(0.02, 0.98))


def _shape(rng, seed, few_rows=False, max_groups=200):
    """-> (p, intercept, group sizes)."""
    if seed in FORCED:
        p, icpt = FORCED[seed]
    else:
        lo, hi = CLASSES[CLASS_OF_SEED[seed % 4]]
        p, icpt = int(rng.integers(lo, hi + 1)), bool(rng.integers(0, 2))
    k = p + icpt
    sizes = [0, 1, k - 1, k, k + 1, 2 * k, 63, 64, 65, 127, 128, 129, 5 * k, 300, 1000]
    G = int(rng.integers(65, max_groups + 1)) if p <= 8 else int(rng.integers(3, 21))
    if few_rows:                                  # the 64-tau grid: 64 references per group
        G = 65 if p <= 8 else G
        weight = np.array([1.0 if n <= 2 * k else 0.15 if n <= 65 else 0.0 for n in sizes])
    else:
        weight = np.array([1.0 if n <= 129 else 0.5 if n <= 300 else 0.25 for n in sizes])
    ns = rng.choice(sizes, size=G, p=weight / weight.sum())
    visit = [n for n, w in zip(sizes, weight) if w > 0]
    if G >= len(visit):                           # every size class once, at random positions
        ns[rng.choice(G, size=len(visit), replace=False)] = visit
    if p <= 8 and seed % 8 == 2 and not few_rows:
        ns[int(rng.integers(0, G))] = LONG_ROWS + int(rng.integers(0, 200))
    return p, icpt, ns.astype(np.int64)


def _rows(rng, p, icpt, ns, predict_rows):
    """-> (offsets, y, X, kinds, train_counts or None).  With predict_rows about a fifth of the rows of every group are
    prediction rows (y NaN, scattered), some of them with a NaN feature; train_counts counts the rows whose y is not NaN."""
    G = len(ns)
    off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    N = int(off[-1])
    a = rng.uniform(-2.0, 1.0)
    col_scale = 10.0 ** rng.uniform(a, a + 2.0, p)
    mu = rng.choice([0.0, 0.0, 0.5, 2.0], p)                            # shifts in units of the column's scale
    sigma = 10.0 ** rng.uniform(-3.0, 0.5)
    offset = sigma * (0.0 if rng.random() < 0.5 else rng.uniform(0.0, 100.0))
    hetero = bool(rng.integers(0, 2))
    beta = rng.standard_normal(p) / col_scale
    X = np.empty((N, p))
    y = np.empty(N)
    kinds = []
    for g in range(G):
        lo, hi = int(off[g]), int(off[g + 1])
        n = hi - lo
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_P))]
        if kind == "aliased" and p < 2:
            kind = "constant"
        kinds.append(kind)
        if n == 0:
            continue
        if kind == "lattice":
            Xg = rng.integers(-3, 4, size=(n, p)).astype(np.float64)
            yg = Xg @ rng.integers(-2, 3, size=p).astype(np.float64) + float(rng.integers(-5, 6)) + rng.integers(-2, 3, size=n)
        else:
            Z = rng.standard_normal((n, p))
            Xg = (Z + mu) * col_scale
            if kind == "constant":
                j = int(rng.integers(0, p))
                Xg[:, j] = col_scale[j] * (1.0 + mu[j])
            elif kind == "aliased":
                i, j = rng.choice(p, 2, replace=False)
                Xg[:, j] = Xg[:, i] * 0.5                                 # exact in binary: an exactly aliased pair
            e = rng.standard_t(3, size=n) if not hetero else rng.standard_normal(n) * (0.2 + np.abs(Z[:, 0]))
            yg = offset + Xg @ beta + sigma * e
            if kind == "duplicates" and n >= 2:
                m = max(1, n // 4)
                src, dst = rng.choice(n, m), rng.choice(n, m, replace=False)
                keep = ~np.isin(src, dst)                                 # (a copied row is not itself overwritten)
                Xg[dst[keep]], yg[dst[keep]] = Xg[src[keep]], yg[src[keep]]
            elif kind == "invalid":
                bad = rng.choice(n, size=max(1, n // 6), replace=False)
                for i in bad:
                    c = int(rng.integers(0, 4))
                    if c == 0:
                        yg[i] = np.nan
                    else:
                        Xg[i, int(rng.integers(0, p))] = (np.nan, np.inf, -np.inf)[c - 1]
            elif kind == "all_nan":
                yg[:] = np.nan
        X[lo:hi], y[lo:hi] = Xg, yg
    tc = None
    if predict_rows:
        pr = rng.random(N) < 0.2
        y[pr] = np.nan
        idx = np.nonzero(pr)[0]
        if len(idx):
            nanx = rng.choice(idx, size=max(1, len(idx) // 10), replace=False)
            X[nanx, rng.integers(0, p, size=len(nanx))] = np.nan
        tc = np.array([int(np.sum(~np.isnan(y[off[g]:off[g + 1]]))) for g in range(G)], dtype=np.int64)
    return off, y, X, kinds, tc


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _group(c, g):
    lo, hi = int(c["off"][g]), int(c["off"][g + 1])
    return c["X"][lo:hi], c["y"][lo:hi], (None if c["train_counts"] is None else int(c["train_counts"][g]))


@functools.lru_cache(maxsize=None)
def case(seed, predict_rows=False):
    """One single-tau call: dict(p, fit_intercept, tau, off, y, X, cols, kinds, train_counts, ref); ref[g] is solve()'s result,
    None for a group the row rules refuse."""
    rng = np.random.default_rng([20261018, int(predict_rows), seed])
    p, icpt, ns = _shape(rng, seed)
    tau = _tau(rng)
    off, y, X, kinds, tc = _rows(rng, p, icpt, ns, predict_rows)
    c = dict(seed=seed, p=p, fit_intercept=icpt, tau=tau, off=off, y=y, X=X, kinds=kinds, train_counts=tc)
    c["cols"] = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    c["ref"] = []
    for g in range(len(ns)):
        Xg, yg, rule = _group(c, g)
        c["ref"].append(qr.solve(Xg, yg, tau, icpt) if qr.rule_status(Xg, yg, tau, icpt, rule) == 0 else None)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def path_case(seed):
    """One call of the tau path with prediction rows: case()'s dict with taus (the caller's grid: unsorted, in some seeds with
    duplicates and invalid entries) in place of tau, and ref[g][t] per position (None at an invalid tau or a refused group)."""
    rng = np.random.default_rng([20261018, 2, seed])
    T = PATH_T[seed % len(PATH_T)]
    # (4 seed: the class p <= 8, never forced wide; 19 references per group: at most 100 groups, every size class still once)
    p, icpt, ns = _shape(rng, seed if T < 64 else 4 * seed, few_rows=T == 64, max_groups=100 if T == 19 else 200)
    taus = [_tau(rng) for _ in range(T)]
    if T >= 7 and seed % 2 == 0:                                                 # duplicates
        for _ in range(2):
            taus[int(rng.integers(0, T))] = taus[int(rng.integers(0, T))]
    if T >= 2 and seed % 3 != 1:                                                 # one to three invalid entries
        for j in rng.choice(T, size=min(T - 1, int(rng.integers(1, 4))), replace=False):
            taus[int(j)] = float(rng.choice([0.0, 1.0, np.nan, -0.1]))
    off, y, X, kinds, tc = _rows(rng, p, icpt, ns, True)
    c = dict(seed=seed, p=p, fit_intercept=icpt, taus=np.array(taus), off=off, y=y, X=X, kinds=kinds, train_counts=tc)
    c["cols"] = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    order = sorted({t for t in taus if 0.0 < t < 1.0})
    c["ref"] = []
    for g in range(len(ns)):
        Xg, yg, rule = _group(c, g)
        by_tau, warm = {}, None
        if order and qr.rule_status(Xg, yg, order[0], icpt, rule) == 0:
            for t in order:                       # the neighbour's vertex is tried first; solve() accepts it only certified at t
                by_tau[t] = qr.solve(Xg, yg, t, icpt, warm=warm)
                warm = (by_tau[t]["b"], by_tau[t]["b0"]) if by_tau[t]["unique"] else None
        c["ref"].append([by_tau.get(t) for t in taus])
    return _freeze(c)


def column_units(X, y, fit_intercept):
    """s_j = max_i |x_ij| over the valid rows (the intercept's is 1), in the order (b, b0)."""
    ok = qr.valid_rows(X, y)
    s = np.max(np.abs(np.asarray(X, dtype=np.float64)[ok]), axis=0)
    return np.concatenate([s, [1.0]]) if fit_intercept else s


def in_comparison(ref):
    return bool(ref["unique"] and ref["kappa"] <= KAPPA_MAX and ref["rmin"] >= RMIN_MIN)


class Tally:
    """What a run saw: the worst coefficient error in units of its tolerance, the continuous groups fitted and outside the
    coefficient comparison, the lattice and the aliased (constant column / aliased pair) groups fitted."""

    def __init__(self):
        self.worst, self.groups, self.continuous, self.outside, self.lattice, self.aliased = 0.0, 0, 0, 0, 0, 0

    def add(self, kind, ref, ratio):
        self.groups += 1
        if ref is None:
            return
        if kind in CONTINUOUS:
            self.continuous += 1
            self.outside += not in_comparison(ref)
        self.lattice += kind == "lattice"
        self.aliased += kind in RANK_KINDS
        if ratio is not None:
            self.worst = max(self.worst, ratio)

    def line(self, what):
        share = self.outside / max(self.continuous, 1)
        return (f"{what}: worst_coef_x_tol {self.worst:.3g}, continuous groups outside the comparison {self.outside}/{self.continuous}"
                f" ({100 * share:.2f} %), lattice {self.lattice}, aliased {self.aliased}, groups {self.groups}")


def assert_input_conditions(refs, kinds, X_y_icpt, what):
    """The conditions on the input, on the reference alone.  refs / kinds: the groups (or group-tau pairs) of one run;
    X_y_icpt[i] = (X, y, fit_intercept) of refs[i]."""
    n_cont = n_out = 0
    for ref, kind, (X, y, icpt) in zip(refs, kinds, X_y_icpt):
        if ref is None:
            continue
        if not ref["unique"]:
            assert ref["gap"] <= 1e-10, f"{what}: interior-point gap {ref['gap']:.3g} of a non-unique {kind} group"
        if kind in CONTINUOUS:
            n_cont += 1
            n_out += not in_comparison(ref)
        if ref["unique"] and ref["kappa"] <= KAPPA_MAX:
            s = column_units(X, y, icpt)
            full = np.concatenate([ref["b"], [ref["b0"]]]) if icpt else ref["b"]
            dbl = np.concatenate([ref["b_double"], [ref["b0_double"]]]) if icpt else ref["b_double"]
            err, size = np.max(np.abs(full - dbl) * s), np.max(np.abs(full) * s)
            assert err <= 1e-11 * size, f"{what}: the double and the refined vertex differ by {err:.3g} of {size:.3g} ({kind}, kappa {ref['kappa']:.3g})"
    # a call of fewer than 20 continuous groups (the wide seeds have 3 to 20 groups) cannot express 5 % in whole groups: there
    # one group may fall outside, and assert_run_share holds the 5 % over the seeds of the run
    assert n_out <= max(1, int(UNCOMPARED_CAP * n_cont)), f"{what}: {n_out} of {n_cont} continuous groups are outside the coefficient comparison"


def assert_run_share(cases, what):
    """At most 5 % of the continuous fitted groups of a run (all its seeds) are outside the coefficient comparison; -> Tally."""
    tally = Tally()
    for c in cases:
        for g, ref in enumerate(c["ref"]):
            for r in (ref if isinstance(ref, list) else [ref]):
                tally.add(c["kinds"][g], r, None)
    assert tally.outside <= UNCOMPARED_CAP * tally.continuous, f"{what}: {tally.outside} of {tally.continuous}"
    return tally


def check_sweep_record(ref, rec, its, X, y, tau, fit_intercept, kind, what, rule_count=None):
    """The assertions a record (host build or GPU) has to meet; -> the coefficient error as a multiple of its tolerance, or
    None where the coefficients were not compared.

    every group    status, n_observations, tau, the NaN pattern and the sign of the pivot count exactly;
                   the record's loss = the pinball loss of its coefficients (test_quantile_cpu.check_record's tolerance);
                   loss <= reference loss (1 + 1e-9) — where the reference interpolates (loss <= 1e-12 max|y|) plus the rounding of
                   evaluating residuals in binary64, as check_record allows it;
                   the certificate optimal wherever it is decided.
    unique, kappa <= 1e4, rmin >= 1e-8
                   |b_j - ref_j| s_j <= 1e-9 max_k |ref_k| s_k, s_j = max_i |x_ij| over the valid rows, s_0 = 1.  A backward
                   stable k x k solve errs by about k kappa 2^-53 <= 33 * 1e4 * 1.1e-16 = 4e-11 of |beta| in these units: 27
                   times inside 1e-9, the project's sweep tolerance.
    every fitted group
                   numpy's matrix_rank of the valid design (columns scaled to unit max-abs) is the reference's rank;
                   n_basis_rows equals it and exactly k - rank coefficient slots are exactly 0.0.  On a lattice the two are
                   one-sided, n_basis_rows <= rank and at least k - n_basis_rows >= k - rank zero slots: the optimum of integer
                   data can have a coefficient that is exactly 0, and then its artificial stays in the basis with a zero
                   multiplier — an optimum all the same, held by the loss and the certificate.  Seen on the GPU sweep: seed 20
                   group 28 (n = 2, p = 1, no intercept: beta = 0, no row in the basis, rank 1) and fit-predict seed 0 group
                   68 (n = 3, p = 1, intercept: one row, rank 2)."""
    p = X.shape[1]
    status = qr.rule_status(X, y, tau, fit_intercept, rule_count)
    assert rec[p + 5] == status, f"{what}: status {rec[p + 5]} != {status}"
    if status != 0:
        assert np.isnan(rec[:p + 5]).all() and its == 0, what
        assert ref is None, what
        return None
    assert its >= 0, f"{what}: the iteration bound stopped the fit ({its})"
    b, b0 = rec[:p], rec[p]
    assert np.isfinite(b).all() and np.isnan(b0) == (not fit_intercept), what
    ok = qr.valid_rows(X, y)
    assert rec[p + 1] == tau and rec[p + 4] == int(ok.sum()), what
    ymax = float(np.max(np.abs(y[ok])))
    loss = qr.pinball_loss(X, y, tau, b, b0)
    assert abs(rec[p + 2] - loss) <= 1e-9 * max(loss, 1e-300) + 1e-12 * ymax, f"{what}: record loss {rec[p + 2]!r} vs {loss!r}"
    A = qr.design(X[ok], fit_intercept)
    k = A.shape[1]
    beta = np.concatenate([[b0], b]) if fit_intercept else b
    noise = 0.0
    if ref["loss"] <= 1e-12 * ymax:
        noise = (k + 2) * 2.0 ** -52 * float(np.sum(np.abs(y[ok]) + np.abs(A) @ np.abs(beta)))
    assert loss <= ref["loss"] * (1 + 1e-9) + noise, f"{what}: loss {loss!r} > reference {ref['loss']!r} ({kind})"
    cert = qr.certify(X, y, tau, fit_intercept, b, b0)
    if cert["decided"]:
        assert cert["optimal"], f"{what}: not optimal {cert} ({kind})"
    s = np.max(np.abs(A), axis=0)
    rank = int(np.linalg.matrix_rank(A / np.where(s > 0, s, 1.0)))
    zeros = int((beta == 0.0).sum())
    assert rank == ref["rank"], f"{what}: the reference's rank {ref['rank']} != {rank}"
    if kind == "lattice":
        assert 0 <= rec[p + 3] <= rank, f"{what}: n_basis_rows {rec[p + 3]} > rank {rank} ({kind})"
        assert zeros >= k - rec[p + 3], f"{what}: {zeros} zero slots, {k - rec[p + 3]} artificials in the basis ({kind})"
    else:
        assert rec[p + 3] == rank, f"{what}: n_basis_rows {rec[p + 3]} != rank {rank} ({kind})"
        assert zeros == k - rank, f"{what}: {zeros} zero slots, k - rank = {k - rank} ({kind})"
    if not in_comparison(ref):
        return None
    assert cert["decided"] and cert["optimal"], f"{what}: {cert}"
    s = column_units(X, y, fit_intercept)
    got = np.concatenate([b, [b0]]) if fit_intercept else b
    want = np.concatenate([ref["b"], [ref["b0"]]]) if fit_intercept else ref["b"]
    err, tol = float(np.max(np.abs(got - want) * s)), COEF_TOL * float(np.max(np.abs(want) * s))
    ratio = err / tol if tol > 0.0 else (0.0 if err == 0.0 else float("inf"))      # (integer data can have the vertex beta = 0)
    assert ratio <= 1.0, f"{what}: coefficients off by {ratio:.3g} x tolerance ({kind}, kappa {ref['kappa']:.3g}, rmin {ref['rmin']:.3g})"
    return ratio
