"""The randomised quantile regression sweep without a GPU.  First the reference solver of the sweep
(tests/quantile_restate.py::solve: interior point on the dual, crossover, certificate; numpy only) against everything that is
known: all golden cases and the path fixture (scipy's HiGHS, recorded) under test_quantile_cpu.check_record, and HiGHS itself
on groups of the sweep's own seeds where scipy imports.  Then the cases of tests/quantile_fuzz_cases.py through the host build of
csrc/quantile_solve.h (tests/tools/quantile_solve_host.cpp and quantile_path_host.cpp under ASan / UBSan: programs of their
own, never loaded into python) with quantile_fuzz_cases.check_sweep_record on every group: fewer seeds than
tests/test_gpu_fuzz_quantile.py runs (the one-lane build is slow on the long groups), the same generator, the same assertions,
and the generator's input conditions on the reference alone.  Nothing here asserts a pivot count or a time."""
import json
import os
import subprocess

import numpy as np
import pytest

import quantile_fuzz_cases as fc
import quantile_restate as qr
from conftest import ROOT
from test_quantile_cpu import _case_text, check_record, host_solver  # noqa: F401  (host_solver, path_solver: fixtures)
from test_quantile_path_cpu import load_path_sets, path_solver  # noqa: F401

FIT_SEEDS = list(range(12))            # the forced widths p = 31 / 32 (seeds 3, 7, 11) and the 5000-row group (seeds 2, 10) included
PATH_SEEDS = list(range(6))            # T = 7, 1, 19, 2, 64, 7; seed 3 is p = 31 with an intercept


def _as_record(c, r):
    p = c["X"].shape[1]
    k = p + c["fit_intercept"]
    return np.concatenate([r["b"], [r["b0"], c["tau"], r["loss"], k, len(c["y"]), 0.0]])


def test_reference_solver_reproduces_the_golden_cases():
    """b, b0 and loss of every golden case and of the path fixture within check_record's tolerances; every case the fixtures
    mark unique comes out of the crossover certified, with the double and the refined vertex 1e-11 apart at most."""
    cases = qr.load_cases() + [c for s in load_path_sets()[1] for c in s["cases"]]
    gauss = compared = 0
    for c in cases:
        if qr.rule_status(c["X"], c["y"], c["tau"], c["fit_intercept"]) != 0:
            continue
        r = qr.solve(c["X"], c["y"], c["tau"], c["fit_intercept"])
        assert r["unique"] == c["unique"], c["name"]
        assert r["unique"] or r["gap"] <= 1e-10, f"{c['name']}: gap {r['gap']:.3g}"
        assert abs(r["loss"] - c["loss"]) <= 1e-9 * c["loss"] + 1e-12 * np.max(np.abs(c["y"])), c["name"]
        done = check_record(c, _as_record(c, r), 0, "solve " + c["name"])
        compared += done
        gauss += c["name"].startswith("gauss")
        if done:                                         # in column units, as the sweep measures it
            s = fc.column_units(c["X"], c["y"], c["fit_intercept"])
            full = np.concatenate([r["b"], [r["b0"]]]) if c["fit_intercept"] else r["b"]
            dbl = np.concatenate([r["b_double"], [r["b0_double"]]]) if c["fit_intercept"] else r["b_double"]
            assert np.max(np.abs(full - dbl) * s) <= 1e-11 * np.max(np.abs(full) * s), c["name"]
    assert gauss >= 180 and compared == sum(c["unique"] and qr.rule_status(c["X"], c["y"], c["tau"], c["fit_intercept"]) == 0 for c in cases)


def test_reference_solver_against_highs_on_sweep_groups():
    opt = pytest.importorskip("scipy.optimize")
    checked = 0
    for seed in (0, 3, 5):
        c = fc.case(seed)
        fitted = [g for g, r in enumerate(c["ref"]) if r is not None and c["off"][g + 1] - c["off"][g] <= 400]
        for g in fitted[::max(1, len(fitted) // 12)]:
            X, y, _ = fc._group(c, g)
            ok = qr.valid_rows(X, y)
            A = qr.design(X[ok], c["fit_intercept"])
            s = np.max(np.abs(A), axis=0)
            A = A / np.where(s > 0, s, 1.0)                                # (the loss does not depend on the columns' units)
            n, k = A.shape
            cost = np.concatenate([np.zeros(k), np.full(n, c["tau"]), np.full(n, 1.0 - c["tau"])])
            res = opt.linprog(cost, A_eq=np.hstack([A, np.eye(n), -np.eye(n)]), b_eq=y[ok],
                              bounds=[(None, None)] * k + [(0, None)] * (2 * n), method="highs-ds")
            assert res.status == 0
            ref = c["ref"][g]
            assert abs(res.fun - ref["loss"]) <= 1e-8 * max(1.0, abs(ref["loss"])), f"seed {seed} group {g} ({c['kinds'][g]})"
            checked += 1
    assert checked >= 20


def _run_fit_seed(seed, host_solver, tally):
    c = fc.case(seed)
    G = len(c["kinds"])
    groups = [fc._group(c, g) for g in range(G)]
    rows = host_solver("".join(_case_text(X, y, c["tau"], c["fit_intercept"]) for X, y, _ in groups))
    assert len(rows) == G
    p = c["p"]
    for g, ((X, y, _), v) in enumerate(zip(groups, rows)):
        ratio = fc.check_sweep_record(c["ref"][g], v[:p + 6], int(v[p + 6]), X, y, c["tau"], c["fit_intercept"], c["kinds"][g],
                                      f"seed {seed} group {g} (p={p} icpt={int(c['fit_intercept'])} n={len(y)} tau={c['tau']})")
        tally.add(c["kinds"][g], c["ref"][g], ratio)
    fc.assert_input_conditions(c["ref"], c["kinds"], [(X, y, c["fit_intercept"]) for X, y, _ in groups], f"seed {seed}")


@pytest.mark.parametrize("seed", FIT_SEEDS)
def test_fuzz_quantile_host(seed, host_solver, record_property):
    tally = fc.Tally()
    _run_fit_seed(seed, host_solver, tally)
    record_property("worst_coef_x_tol", tally.worst)
    record_property("groups", tally.groups)
    print(tally.line(f"host fit seed {seed}"))


@pytest.mark.parametrize("seed", PATH_SEEDS)
def test_fuzz_quantile_path_host(seed, path_solver, record_property):
    """Every (group, tau) record of the path against the reference at that tau; invalid positions have status 1; the fused
    prediction is the record's own coefficients applied to the row, NaN where a feature is not finite or the fit failed.
    (Seed 2, group 62 at tau = 0.75 — lattice, n = 128, p = 2 — ended at loss 47.5 instead of 47.4 under the single exchange.)"""
    c = fc.path_case(seed)
    G, taus, p, icpt = len(c["kinds"]), c["taus"], c["p"], c["fit_intercept"]
    groups = [fc._group(c, g) for g in range(G)]
    runs = path_solver([(X, y, taus, icpt, 1000, rule) for X, y, rule in groups])
    tally = fc.Tally()
    refs, kinds, xy = [], [], []
    for g, ((X, y, rule), (rec, its, pred)) in enumerate(zip(groups, runs)):
        A = qr.design(X, icpt)
        finite = np.isfinite(X).all(axis=1)
        for t, tau in enumerate(taus):
            what = f"path seed {seed} group {g} tau[{t}]={tau} (p={p} icpt={int(icpt)} n={len(y)})"
            if not 0.0 < tau < 1.0:
                assert rec[t, p + 5] == 1 and np.isnan(rec[t, :p + 5]).all() and its[t] == 0 and np.isnan(pred[:, t]).all(), what
                continue
            ratio = fc.check_sweep_record(c["ref"][g][t], rec[t], int(its[t]), X, y, float(tau), icpt, c["kinds"][g], what, rule)
            tally.add(c["kinds"][g], c["ref"][g][t], ratio)
            refs.append(c["ref"][g][t]), kinds.append(c["kinds"][g]), xy.append((X, y, icpt))
            if rec[t, p + 5] != 0:
                assert np.isnan(pred[:, t]).all(), what
                continue
            beta = np.concatenate([[rec[t, p]], rec[t, :p]]) if icpt else rec[t, :p]
            yhat = np.where(finite[:, None], A, 0.0) @ beta
            assert np.isnan(pred[~finite, t]).all() and (np.abs(pred[finite, t] - yhat[finite]) <= 1e-12 * np.maximum(1.0, np.abs(yhat[finite]))).all(), what
    fc.assert_input_conditions(refs, kinds, xy, f"path seed {seed}")
    record_property("worst_coef_x_tol", tally.worst)
    record_property("groups", tally.groups)
    print(tally.line(f"host path seed {seed} T={len(taus)}"))


def test_uncompared_share_of_the_run():
    """Over all seeds of this module (the reference alone; the cases are cached): at most 5 % of the continuous fitted groups are
    outside the coefficient comparison, and the run has met lattice and aliased groups."""
    for what, cases in (("fit", [fc.case(s) for s in FIT_SEEDS]), ("path", [fc.path_case(s) for s in PATH_SEEDS])):
        tally = fc.assert_run_share(cases, what)
        assert tally.continuous >= 100 and tally.lattice >= 20 and tally.aliased >= 20, tally.line(what)
        print(tally.line(what))


def _lattice_behind_a_degenerate_vertex():
    """tests/golden/quantile/lattice_degenerate.json: n = 129, p = 3, intercept, tau = 0.25, drawn by the sweep's lattice recipe."""
    with open(os.path.join(os.path.dirname(qr.GOLDEN), "lattice_degenerate.json")) as f:
        doc = json.load(f)
    return np.array(doc["X"], dtype=np.float64), np.array(doc["y"], dtype=np.float64), doc["tau"], doc["optimal_loss"]


def test_lattice_optimum_behind_a_degenerate_vertex(host_solver):
    """The defect this sweep found, reduced.  With one zero-length exchange per trial the solve ended "converged" (3 pivots) at a
    degenerate vertex of loss 63.54166666666667; the optimum (the reference here, HiGHS agrees) is 63.3359375.  No edge of that
    basis descends and no single exchange finds one that does: leaving the vertex takes several pivots of length zero in a
    row, which the sided kink rows of quantile_solve.h now make.  Of 600 random lattice groups (n = 129 / 300 / 1000,
    p = 3 .. 8) the host build missed the optimum in 11, and in 49 of 200 row orders of the group the MI355X missed
    (tests/test_gpu_fuzz_quantile.py::test_fuzz_quantile[0], group 78); none of the 800 since."""
    X, y, tau, optimum = _lattice_behind_a_degenerate_vertex()
    assert X.shape == (129, 3) and tau == 0.25 and optimum == 63.3359375
    ref = qr.solve(X, y, tau, True)
    assert ref["gap"] <= 1e-10 and abs(ref["loss"] - optimum) <= 1e-9
    v, = host_solver(_case_text(X, y, tau, True))
    fc.check_sweep_record(ref, v[:9], int(v[9]), X, y, tau, True, "lattice", "the reduced lattice case")


def test_lattice_that_ends_under_blands_rule(host_solver, tmp_path):
    """tests/golden/quantile/lattice_bland.json (n = 300, p = 7, intercept, tau = 0.25): the fit makes 272 pivots of length zero
    at one degenerate vertex, so its last 16 follow Bland's rule (kQsBlandAfter = 256).  It converges to the optimum; and built
    with the cap at 256 (QS_MAX_EXCHANGES) the same program reports the fit as stopped (count negated), which shows that the
    pivots under Bland's rule are needed and made.  (With Bland's rule from the first zero-length pivot on, groups of 1000 rows
    exhaust the cap of 1024: the rule ends a stall, it is no substitute for the side-changing pivots before it.)"""
    with open(os.path.join(os.path.dirname(qr.GOLDEN), "lattice_bland.json")) as f:
        doc = json.load(f)
    X, y, tau = np.array(doc["X"], dtype=np.float64), np.array(doc["y"], dtype=np.float64), doc["tau"]
    ref = qr.solve(X, y, tau, True)
    assert abs(ref["loss"] - doc["optimal_loss"]) <= 1e-9 * doc["optimal_loss"] and (ref["unique"] or ref["gap"] <= 1e-10)
    v, = host_solver(_case_text(X, y, tau, True))
    fc.check_sweep_record(ref, v[:13], int(v[13]), X, y, tau, True, "lattice", "the Bland case")
    exe = str(tmp_path / "quantile_solve_host_256")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-DQS_MAX_EXCHANGES=256", os.path.join(ROOT, "tests", "tools", "quantile_solve_host.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], input=_case_text(X, y, tau, True), capture_output=True, text=True,
                         env={k: e for k, e in os.environ.items() if k != "LD_PRELOAD"})
    assert out.returncode == 0 and int(out.stdout.split()[-1]) < 0, out.stdout[-200:] + out.stderr[-500:]
