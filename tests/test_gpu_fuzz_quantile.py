"""Randomised reference sweep of grouped quantile regression and its tau path on the MI355X (run with -m gpu): every group of
every drawn call against tests/quantile_restate.py::solve, a numpy interior-point solver with a crossover that shares neither a
pivot rule nor a tolerance with csrc/quantile_solve.h.  The generator, what a seed draws, the assertions on a record
(check_sweep_record) and the conditions on the input (assert_input_conditions, on the reference alone, no case skipped) are
tests/quantile_fuzz_cases.py's; tests/test_quantile_fuzz_cpu.py runs the first seeds of the same generator through the host
build.  ANOFOX_FUZZ_SCALE multiplies the number of seeds.  Nothing here asserts a pivot count or a time."""
import numpy as np
import pytest

import quantile_fuzz_cases as fc
import quantile_restate as qr
from conftest import import_pkg

pytestmark = pytest.mark.gpu

FIT_SEEDS = list(range(30 * fc.SCALE))
PATH_SEEDS = list(range(16 * fc.SCALE))
PREDICT_SEEDS = list(range(8 * fc.SCALE))


@pytest.fixture(scope="module")
def pkg():
    return import_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _what(c, g, extra=""):
    n = int(c["off"][g + 1] - c["off"][g])
    return f"seed {c['seed']} group {g}{extra} (p={c['p']} icpt={int(c['fit_intercept'])} n={n} {c['kinds'][g]})"


def _fit(pkg, ctx, c, tau=None):
    o = pkg.QuantileOptions(tau=c["tau"] if tau is None else tau, fit_intercept=c["fit_intercept"]).batch_options()
    return pkg.quantile_fit_batch_host(c["off"], c["y"], c["cols"], o, ctx=ctx)


def _check_fit(c, rec, its):
    """check_sweep_record on every group of a single-tau call (the rule count is the group's row count) -> Tally."""
    tally = fc.Tally()
    for g in range(len(c["kinds"])):
        X, y, _ = fc._group(c, g)
        ratio = fc.check_sweep_record(_plain_fit_ref(c, g), rec[g], int(its[g]), X, y, c["tau"], c["fit_intercept"], c["kinds"][g], _what(c, g))
        tally.add(c["kinds"][g], c["ref"][g], ratio)
    return tally


def _plain_fit_ref(c, g):
    """The reference of group g under the plain fit's rule, which counts rows.  A case with prediction rows holds the
    references of the fit-predict rule, which counts training rows (those with a y): the two differ only on a group of two or
    more rows of which fewer than two have a y, which fit-predict refuses (status 100, no reference) and the plain fit does not
    — that group is solved here."""
    X, y, _ = fc._group(c, g)
    if c["train_counts"] is None or c["train_counts"][g] >= 2 or len(y) < 2:
        return c["ref"][g]
    return qr.solve(X, y, c["tau"], c["fit_intercept"]) if qr.rule_status(X, y, c["tau"], c["fit_intercept"]) == 0 else None


def _conditions(c, what):
    G = len(c["kinds"])
    xy = [(*fc._group(c, g)[:2], c["fit_intercept"]) for g in range(G)]
    if "taus" in c:
        T = len(c["taus"])
        fc.assert_input_conditions([r for g in range(G) for r in c["ref"][g]], [k for k in c["kinds"] for _ in range(T)],
                                   [v for v in xy for _ in range(T)], what)
    else:
        fc.assert_input_conditions(c["ref"], c["kinds"], xy, what)


@pytest.mark.parametrize("seed", FIT_SEEDS)
def test_fuzz_quantile(pkg, ctx, seed, record_property):
    """One quantile_fit_batch_host call per seed, check_sweep_record on every group.

    Seed 0, group 78 (lattice, n = 300, p = 6, intercept, tau = 0.25) is the case that found the degenerate-vertex defect of
    the single exchange: the MI355X returned loss 128.5 "converged", the optimum is 128.082265019521 (DESIGN.md §1;
    tests/test_quantile_fuzz_cpu.py::test_lattice_optimum_behind_a_degenerate_vertex is its reduced form)."""
    c = fc.case(seed)
    rec, its = _fit(pkg, ctx, c)
    tally = _check_fit(c, rec, its)
    _conditions(c, f"seed {seed}")
    record_property("worst_coef_x_tol", tally.worst)
    record_property("groups", tally.groups)
    print(tally.line(f"gpu fit seed {seed}"))


def _path_calls(pkg, ctx, c):
    o = pkg.QuantileOptions(tau=float("nan"), fit_intercept=c["fit_intercept"]).batch_options()
    return pkg.quantile_fit_predict_path_batch_host(c["off"], c["y"], c["cols"], o, c["taus"], train_counts=c["train_counts"], ctx=ctx)


@pytest.mark.parametrize("seed", PATH_SEEDS)
def test_fuzz_quantile_path(pkg, ctx, seed, record_property):
    """Every (group, tau) record of quantile_fit_predict_path_batch_host against the reference at that tau; invalid positions
    have status 1; the fused predictions are the record's own coefficients applied to the row within 1e-12 max(1, |yhat|), NaN
    where a feature is not finite or the fit failed; quantile_fit_path_batch_host gives the same bytes and every loss agrees
    with a cold single-tau call — on the groups whose rule count (rows there, training rows here) does not decide."""
    c = fc.path_case(seed)
    G, taus, p, icpt, off = len(c["kinds"]), c["taus"], c["p"], c["fit_intercept"], c["off"]
    rec, its, pred = _path_calls(pkg, ctx, c)
    tally = fc.Tally()
    for g in range(G):
        X, y, rule = fc._group(c, g)
        A = qr.design(X, icpt)
        finite = np.isfinite(X).all(axis=1)
        pg = pred[off[g]:off[g + 1]]
        for t, tau in enumerate(taus):
            what = _what(c, g, f" tau[{t}]={tau}")
            if not 0.0 < tau < 1.0:
                assert rec[g, t, p + 5] == 1 and np.isnan(rec[g, t, :p + 5]).all() and its[g, t] == 0 and np.isnan(pg[:, t]).all(), what
                continue
            ratio = fc.check_sweep_record(c["ref"][g][t], rec[g, t], int(its[g, t]), X, y, float(tau), icpt, c["kinds"][g], what, rule)
            tally.add(c["kinds"][g], c["ref"][g][t], ratio)
            if rec[g, t, p + 5] != 0:
                assert np.isnan(pg[:, t]).all(), what
                continue
            beta = np.concatenate([[rec[g, t, p]], rec[g, t, :p]]) if icpt else rec[g, t, :p]
            yhat = np.where(finite[:, None], A, 0.0) @ beta
            assert np.isnan(pg[~finite, t]).all(), what
            assert (np.abs(pg[finite, t] - yhat[finite]) <= 1e-12 * np.maximum(1.0, np.abs(yhat[finite]))).all(), what
    _conditions(c, f"path seed {seed}")
    # the entry without a prediction and the cold fits count rows, not training rows: the groups both rules treat alike
    same_rule = np.array([c["train_counts"][g] >= 2 or off[g + 1] - off[g] < 2 for g in range(G)])
    o = pkg.QuantileOptions(fit_intercept=icpt).batch_options()
    rec2, its2 = pkg.quantile_fit_path_batch_host(off, c["y"], c["cols"], o, taus, ctx=ctx)
    assert rec2[same_rule].tobytes() == rec[same_rule].tobytes() and its2[same_rule].tobytes() == its[same_rule].tobytes()
    ymax = np.array([np.max(np.abs(np.nan_to_num(c["y"][off[g]:off[g + 1]], posinf=0.0, neginf=0.0)), initial=0.0) for g in range(G)])
    for tau in sorted({float(t) for t in taus if 0.0 < t < 1.0}):
        cold, _ = _fit(pkg, ctx, c, tau)
        for t in np.nonzero(taus == tau)[0]:
            assert (rec[same_rule, t, p + 5] == cold[same_rule, p + 5]).all(), tau
            m = same_rule & (cold[:, p + 5] == 0)
            lp, lc = rec[m, t, p + 2], cold[m, p + 2]
            assert (np.abs(lp - lc) <= 1e-9 * np.maximum(lc, 1e-300) + 1e-12 * ymax[m]).all(), f"path seed {seed} tau {tau}: loss against the cold fit"
    record_property("worst_coef_x_tol", tally.worst)
    record_property("groups", tally.groups)
    print(tally.line(f"gpu path seed {seed} T={len(taus)}"))


@pytest.mark.parametrize("seed", PREDICT_SEEDS)
def test_fuzz_quantile_fit_predict(pkg, ctx, seed, record_property):
    """quantile_fit_predict_batch_host on a batch with scattered prediction rows.  The core is the fit of the training rows:
    the plain fit of the same arrays (rows without a y are masked there as well) meets check_sweep_record, and the core holds
    its coefficient bytes, NaN for r2 / ssr / sigma, the count and the status of the training-count rule.  yhat against the
    REFERENCE coefficients on the compared groups: coefficients within 1e-9 M of the reference in column units
    (M = max_k |ref_k| s_k) move a_i'beta by at most 1e-9 M sum_j |a_ij| / s_j.  The bounds are NaN; a failed group is all NaN;
    a row with a feature that is not finite has a NaN yhat."""
    c = fc.case(seed, True)
    G, p, icpt, off, tc = len(c["kinds"]), c["p"], c["fit_intercept"], c["off"], c["train_counts"]
    o = pkg.QuantileOptions(tau=c["tau"], fit_intercept=icpt).batch_options()
    core, pred = pkg.quantile_fit_predict_batch_host(off, c["y"], c["cols"], o, train_counts=tc, ctx=ctx)
    rec, its = _fit(pkg, ctx, c)
    tally = _check_fit(c, rec, its)
    _conditions(c, f"fit-predict seed {seed}")
    assert np.isnan(pred[:, 1:]).all()
    for g in range(G):
        X, y, rule = fc._group(c, g)
        what = _what(c, g)
        pg = pred[off[g]:off[g + 1], 0]
        status = qr.rule_status(X, y, c["tau"], icpt, rule)
        assert core[g, p + 5] == status, what
        if status != 0:
            assert np.isnan(core[g, :p + 5]).all() and np.isnan(pg).all(), what
            continue
        assert core[g, :p + 1].tobytes() == rec[g, :p + 1].tobytes() and np.isnan(core[g, p + 1:p + 4]).all() and core[g, p + 4] == rec[g, p + 4], what
        finite = np.isfinite(X).all(axis=1)
        assert np.isnan(pg[~finite]).all() and np.isfinite(pg[finite]).all(), what
        ref = c["ref"][g]
        if fc.in_comparison(ref):
            s = fc.column_units(X, y, icpt)
            want = np.concatenate([ref["b"], [ref["b0"]]]) if icpt else ref["b"]
            Af = np.column_stack([X[finite], np.ones(int(finite.sum()))]) if icpt else X[finite]
            tol = fc.COEF_TOL * np.max(np.abs(want) * s) * (np.abs(Af) / s).sum(axis=1)
            assert (np.abs(pg[finite] - Af @ want) <= tol).all(), f"{what}: yhat against the reference coefficients"
    record_property("worst_coef_x_tol", tally.worst)
    record_property("groups", tally.groups)
    print(tally.line(f"gpu fit-predict seed {seed}"))


def _shuffled_table(c, rng):
    """The rows of a case in random order under keys that are neither contiguous nor sorted; groups without rows have no key.
    -> (keys, y list with None for NULL, X, the batch layout the aggregate sorts them into: off, y, cols, train_counts)."""
    G = len(c["kinds"])
    gid = np.repeat(np.arange(G), np.diff(c["off"]))
    key_of = rng.permutation(G) * 7 + 3
    order = rng.permutation(len(gid))
    keys, y, X = key_of[gid][order], c["y"][order], c["X"][order]
    srt = np.argsort(keys, kind="stable")                                  # what finalize() does with them
    ks, ys, Xs = keys[srt], y[srt], X[srt]
    off = np.concatenate([[0], np.cumsum(np.unique(ks, return_counts=True)[1])]).astype(np.int64)
    tc = np.array([int(np.sum(~np.isnan(ys[off[i]:off[i + 1]]))) for i in range(len(off) - 1)], dtype=np.int64)
    return keys, [None if np.isnan(v) else float(v) for v in y], X, (off, ys, [np.ascontiguousarray(Xs[:, j]) for j in range(c["p"])], tc)


def test_python_aggregates_on_shuffled_keys(pkg, ctx):
    """quantile_fit_predict_agg and quantile_path_fit_predict_agg on a seeded batch whose rows arrive shuffled, under keys that
    are not contiguous, with NULL y: every key's rows are the batch call's on the sorted layout, byte for byte."""
    rng = np.random.default_rng(77)
    c = fc.case(1, True)                                                   # a wide seed: a dozen groups, a few hundred rows
    keys, ylist, X, (off, ys, cols, tc) = _shuffled_table(c, rng)
    r = pkg.quantile_fit_predict_agg(keys, ylist, X, {"tau": c["tau"], "intercept": c["fit_intercept"]}, context=ctx)
    o = pkg.QuantileOptions(tau=c["tau"], fit_intercept=c["fit_intercept"]).batch_options()
    core, pred = pkg.quantile_fit_predict_batch_host(off, ys, cols, o, train_counts=tc, ctx=ctx)
    assert list(r.keys) == sorted(set(keys.tolist())) and r.row_offsets.tobytes() == off.tobytes()
    assert r.core.tobytes() == core.tobytes() and r.yhat.tobytes() == pred[:, 0].tobytes()
    assert np.isnan(r.yhat_lower).all() and np.isnan(r.yhat_upper).all()
    assert (r.is_null == (core[:, -1] != 0)).all() and (core[:, -1] == 0).any() and r.y_is_null.sum() == np.isnan(ys).sum()
    for i in np.nonzero(core[:, -1] == 0)[0][:3]:
        rows = r.rows(int(i))
        assert len(rows) == off[i + 1] - off[i] and sum(x["is_training"] for x in rows) == tc[i]

    c = fc.path_case(5)
    keys, ylist, X, (off, ys, cols, tc) = _shuffled_table(c, rng)
    taus = [float(t) for t in c["taus"] if 0.0 < t < 1.0]
    rp = pkg.quantile_path_fit_predict_agg(keys, ylist, X, {"taus": taus, "intercept": c["fit_intercept"]}, context=ctx)
    o = pkg.QuantileOptions(fit_intercept=c["fit_intercept"]).batch_options()
    rec, its, pred = pkg.quantile_fit_predict_path_batch_host(off, ys, cols, o, taus, train_counts=tc, ctx=ctx)
    assert rp.records.tobytes() == rec.tobytes() and rp.iterations.tobytes() == its.tobytes() and rp.yhat.tobytes() == pred.tobytes()
    assert (rp.is_null == (rec[:, :, -1] != 0)).all() and (rec[:, :, -1] == 0).any() and rp.yhat_of(0).shape == (off[1], len(taus))


def test_two_calls_give_the_same_bytes(pkg, ctx):
    """One sweep seed of each kind, called twice (the seed with the 5000-row group among them)."""
    c = fc.case(2)
    a, b = _fit(pkg, ctx, c), _fit(pkg, ctx, c)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = fc.path_case(2)
    a, b = _path_calls(pkg, ctx, c), _path_calls(pkg, ctx, c)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))
    c = fc.case(0, True)
    o = pkg.QuantileOptions(tau=c["tau"], fit_intercept=c["fit_intercept"]).batch_options()
    a = pkg.quantile_fit_predict_batch_host(c["off"], c["y"], c["cols"], o, train_counts=c["train_counts"], ctx=ctx)
    b = pkg.quantile_fit_predict_batch_host(c["off"], c["y"], c["cols"], o, train_counts=c["train_counts"], ctx=ctx)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_uncompared_share_of_the_run():
    """Over all seeds of this module (the reference alone; the cases are cached): at most 5 % of the continuous fitted groups
    are outside the coefficient comparison."""
    for what, cases in (("fit", [fc.case(s) for s in FIT_SEEDS]), ("path", [fc.path_case(s) for s in PATH_SEEDS]),
                        ("fit-predict", [fc.case(s, True) for s in PREDICT_SEEDS])):
        print(fc.assert_run_share(cases, what).line(what))
