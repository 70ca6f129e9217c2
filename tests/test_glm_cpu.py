"""CPU tier of the GLM family: csrc/glm_irls.h in its host build (tests/tools/glm_host.cpp, a program of its own compiled
under ASan / UBSan, never loaded into python) on every case of tests/glm_cases.py, checked against tests/glm_restate.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import glm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = GC.calls()
IDS = ["%s-p%d-%s-lam%g-%s" % ("poisson" if c[0] == GC.POISSON else "binomial", c[1], "icpt" if c[2] else "noicpt", c[3],
                               "off" if c[4] else "nooff") for c in CALLS]


@pytest.fixture(scope="module")
def host_glm(tmp_path_factory):
    """tests/tools/glm_host.cpp as a program of its own, under ASan / UBSan.  The child inherits the environment unchanged.  Where
    a process-wide LD_PRELOAD is set, a sanitizer's runtime could not be the first one loaded, so there the same program is built
    without the sanitizers and the cases still run (the sanitised run is the one on a plain environment)."""
    exe = str(tmp_path_factory.mktemp("glm") / "glm_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "glm_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(data):
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return [np.array([float(t) for t in ln.split()]) for ln in out.stdout.decode().strip().split("\n")]
    return run


def split(line, p, n=None):
    rec, inf = line[:p + 11], line[p + 11:6 * p + 11]
    pred = line[6 * p + 11:] if n is not None else None
    assert pred is None or len(pred) == n
    return rec, inf, pred


def test_input_conditions_cap():
    """At most 5 % of the non-degenerate groups of a call (|eta| <= 3 by construction, at least 12 k rows) are separated or
    beyond the kappa bound: asserted on the restatement alone, for every seed."""
    for c in CALLS:
        call = GC.make_call(*c)
        refs = GC.reference(call)
        k = call["p"] + int(call["icpt"])
        rows = np.diff(call["offsets"])  # (the two rules of the generator hold for the groups of at least 12 k rows)
        pool = [r for r, kind, n in zip(refs, call["kinds"], rows) if r["status"] == 0 and kind not in ("degenerate", "dup") and n >= 12 * k]
        out = [r for r in pool if not GC.in_conditions(r, call["p"])]
        print("seed %d: %d of %d groups outside the input conditions" % (c[5], len(out), len(pool)))
        assert len(out) <= 0.05 * len(pool), (c, len(out), len(pool))


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_tight_tolerance(host_glm, c):
    """tolerance = 1e-12, with inference and fit-predict: coefficients, deviances, AIC, standard errors and mu to the bounds."""
    call = GC.make_call(*c)
    refs = GC.reference(call)
    lines = host_glm(GC.host_input(call, 1e-12, predict=True))
    o, p, errs, compared = call["offsets"], call["p"], {}, 0
    for g, (line, ref) in enumerate(zip(lines, refs)):
        n = int(o[g + 1] - o[g])
        rec, inf, pred = split(line, p, n)
        if n < 2:  # the fit-predict rule
            assert rec[p + 10] == 100 and np.all(np.isnan(rec[:p + 10])) and np.all(np.isnan(pred))
            continue
        compared += GC.check_record(rec, inf, ref, p, True, errs, pred, "group %d (%s)" % (g, call["kinds"][g]), call["kinds"][g], call["lam"])
    print(IDS[CALLS.index(c)], "compared", compared, {k: "%.2e" % v for k, v in errs.items()})
    assert compared >= 50


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_default_tolerance(host_glm, c):
    """tolerance = 1e-8 (the default), the plain fit: converged, 0 <= deviance - optimum <= 2e-8 (0.1 + deviance)."""
    call = GC.make_call(*c)
    refs = GC.reference(call)
    lines = host_glm(GC.host_input(call, 1e-8))
    p, errs, compared = call["p"], {}, 0
    for g, (line, ref) in enumerate(zip(lines, refs)):
        rec, inf, _ = split(line, p)
        compared += GC.check_record(rec, inf, ref, p, False, errs, None, "group %d (%s)" % (g, call["kinds"][g]), call["kinds"][g], call["lam"])
    print(IDS[CALLS.index(c)], "compared", compared, {k: "%.2e" % v for k, v in errs.items()})
    assert compared >= 50


@pytest.mark.parametrize("bad", [dict(tolerance=float("nan")), dict(tolerance=0.0), dict(tolerance=float("inf")), dict(lam=-1.0),
                                 dict(lam=float("nan")), dict(max_iterations=0), dict(family=7)])
def test_invalid_options(host_glm, bad):
    call = GC.make_call(GC.POISSON, 2, True, 0.0, False, 77)
    call["offsets"] = call["offsets"][:12]
    call["lam"] = bad.get("lam", 0.0)
    call["family"] = bad.get("family", GC.POISSON)
    for line in host_glm(GC.host_input(call, bad.get("tolerance", 1e-8), bad.get("max_iterations", 100))):
        assert line[2 + 10] == 1 and np.all(np.isnan(line[:12])) and np.all(np.isnan(line[13:]))


def test_no_convergence_status(host_glm):
    """max_iterations = 1 cannot converge from mustart: the convergence-failure status, every other field NaN."""
    call = GC.make_call(GC.BINOMIAL, 2, True, 0.0, False, 78)
    lines = host_glm(GC.host_input(call, 1e-12, 1))
    assert any(line[12] == 3 for line in lines)
    for line in lines:
        if line[12] == 3:
            assert np.all(np.isnan(line[:12])) and np.all(np.isnan(line[13:]))


GOLDEN = os.path.join(ROOT, "tests", "golden", "glm")


@pytest.mark.parametrize("name", ["poisson_offset", "binomial_ridge", "poisson_constant_column", "poisson_large_counts"])
def test_golden_fixture(host_glm, name):
    """Reduced cases committed as data: inputs and the restatement's outputs.  poisson_large_counts (n = 30, p = 1, an
    intercept, mean count 54286) is the defect of halving the first step against the deviance at mustart: ten halvings took
    beta from the near-optimal first solve to beta / 1024, the restart from mu = 1 overflowed, and the fit ended with status 3."""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        fx = json.load(f)
    y, x = np.array(fx["y"], float), np.array(fx["x"], float)
    call = dict(family=fx["family"], p=x.shape[1], icpt=fx["fit_intercept"], lam=fx["lambda"], offsets=np.array([0, len(y)]), y=y, x=x,
                off=np.array(fx["offset"], float) if fx["offset"] is not None else None, kinds=["golden"], seed=-1)
    rec, inf, _ = split(host_glm(GC.host_input(call, 1e-12))[0], x.shape[1])
    want = fx["expected"]
    p = x.shape[1]
    coef = np.array([np.nan if v is None else v for v in want["coef"]])
    assert np.array_equal(np.isnan(rec[:p]), np.isnan(coef))
    m = ~np.isnan(coef)
    assert np.max(np.abs(rec[:p][m] - coef[m])) <= 1e-9 * max(1.0, np.max(np.abs(coef[m])))
    if want["intercept"] is not None:
        assert abs(rec[p] - want["intercept"]) <= 1e-9 * max(1.0, abs(want["intercept"]))
    assert GC.rel(rec[p + 1], want["deviance"]) <= 1e-9 and GC.rel(rec[p + 4], want["aic"]) <= 1e-9
    assert rec[p + 6] == want["n_obs"] and rec[p + 7] == want["n_params"]
    se = np.array([np.nan if v is None else v for v in want["se"]])
    assert np.max(np.abs(inf[:p][m] / se[m] - 1.0)) <= 1e-6
