"""CPU tier of the GLM extras: the Poisson interval and the binomial accuracy of csrc/glm_irls.h in its host build
(tests/tools/glm_extras_host.cpp, a program of its own compiled under ASan / UBSan, never loaded into python) on the cases of
tests/glm_extras_cases.py.  The bounds and the reasoning behind them: the docstring of that module."""
import os
import subprocess

import numpy as np
import pytest

import glm_cases as GC
import glm_extras_cases as XC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = XC.calls()
IDS = [XC.ident(c) for c in CALLS]
POISSON_CALLS = [c for c in CALLS if c[0] == XC.POISSON]
BINOMIAL_CALLS = [c for c in CALLS if c[0] == XC.BINOMIAL]


def _build(tmp, name):
    exe = str(tmp / name)
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(data):
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return [ln.split() for ln in out.stdout.decode().strip().split("\n")]
    return run


@pytest.fixture(scope="module")
def extras(tmp_path_factory):
    """glm_extras_host.cpp as a program of its own, under ASan / UBSan where no process-wide LD_PRELOAD is set (as
    test_glm_cpu.py builds glm_host.cpp)."""
    return _build(tmp_path_factory.mktemp("glm_extras"), "glm_extras_host")


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """glm_host.cpp: the program that never sets the new fields."""
    return _build(tmp_path_factory.mktemp("glm_plain"), "glm_host")


def split(tokens, p, n):
    v = np.array([float(t) for t in tokens])
    assert len(v) == p + 12 + 3 * n
    return v[:p + 11], v[p + 11], v[p + 12:].reshape(n, 3)


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_interval_zero_is_the_plain_fit_predict(extras, plain, c):
    """interval_z = 0: the record and mu print to the same text (%.17g round-trips a double) as the program that leaves the new
    fields alone, and both bounds stay NaN."""
    call = XC.make_call(*c)
    o, p = call["offsets"], call["p"]
    got = extras(XC.host_input(call, 1e-12, True, 0.0, XC.THRESHOLD, False))
    want = plain(GC.host_input(call, 1e-12, predict=True))
    for g, (a, b) in enumerate(zip(got, want)):
        n = int(o[g + 1] - o[g])
        assert a[:p + 11] == b[:p + 11], g
        assert a[p + 12::3] == b[6 * p + 11:], g
        rec, acc, pred = split(a, p, n)
        assert np.isnan(acc) and np.all(np.isnan(pred[:, 1:])), g


@pytest.mark.parametrize("c", POISSON_CALLS, ids=[XC.ident(c) for c in POISSON_CALLS])
def test_interval(extras, c):
    call = XC.make_call(*c)
    refs, o, p, errs = GC.reference(call), call["offsets"], call["p"], {}
    base = extras(XC.host_input(call, 1e-12, True, 0.0, XC.THRESHOLD, False))
    lines = extras(XC.host_input(call, 1e-12, True, XC.Z, XC.THRESHOLD, False))
    compared = fitted = 0
    for g, (tok, ref) in enumerate(zip(lines, refs)):
        n = int(o[g + 1] - o[g])
        rec, _, pred = split(tok, p, n)
        assert tok[:p + 11] == base[g][:p + 11] and tok[p + 12::3] == base[g][p + 12::3], g   # the interval changes nothing else
        if n < 2:
            assert rec[p + 10] == 100 and np.all(np.isnan(pred)), g
            continue
        GC.check_record(rec, None, ref, p, True, None, pred[:, 0], "group %d" % g)
        if rec[p + 10] != 0:
            assert np.all(np.isnan(pred)), g
            continue
        fitted += 1
        compared += XC.check_interval(rec, pred, ref, p, XC.Z, "group %d" % g, errs)
        if call["kinds"][g] == "nanrow":
            assert np.all(np.isnan(pred[3])) and np.all(np.isfinite(pred[5])), g
    print(XC.ident(c), "fitted", fitted, "compared", compared, {k: "%.2e of the bound" % v for k, v in errs.items()})
    assert compared >= 3 and fitted >= 5


def test_no_compared_row_near_the_threshold():
    """On the restatement alone: no row of a compared group has a mu within 1e-6 of the threshold (cap 0)."""
    for c in BINOMIAL_CALLS:
        call = XC.make_call(*c)
        assert XC.band_rows(call, GC.reference(call)) == 0, c


@pytest.mark.parametrize("c", BINOMIAL_CALLS, ids=[XC.ident(c) for c in BINOMIAL_CALLS])
def test_accuracy(extras, c):
    """With fit-predict (the count over the same run's mu) and as a plain fit (the same record, the same accuracy)."""
    call = XC.make_call(*c)
    refs, o, p = GC.reference(call), call["offsets"], call["p"]
    lines = extras(XC.host_input(call, 1e-12, True, 0.0, XC.THRESHOLD, True))
    fits = extras(XC.host_input(call, 1e-12, False, 0.0, XC.THRESHOLD, True))
    compared = fitted = 0
    for g, (tok, ref) in enumerate(zip(lines, refs)):
        n = int(o[g + 1] - o[g])
        y = call["y"][o[g]:o[g + 1]]
        rec, acc, pred = split(tok, p, n)
        frec, facc, _ = split(fits[g], p, 0)
        if n < 2:
            assert rec[p + 10] == 100 and np.isnan(acc) and np.all(np.isnan(pred)), g
            # without the fit-predict rule one row is a fit of one parameter (every column is constant over it and is dropped), and
            # a separated one: it may not converge
            assert frec[p + 10] in (0, 3), g
            assert np.isnan(facc) == (frec[p + 10] != 0), g
            continue
        assert tok[:p + 12] == fits[g][:p + 12], g
        GC.check_record(rec, None, ref, p, True, None, pred[:, 0], "group %d" % g)
        done = XC.check_accuracy(acc, int(rec[p + 10]), y, pred[:, 0], ref, p, XC.THRESHOLD, "group %d" % g)
        fitted += rec[p + 10] == 0
        compared += done
    print(XC.ident(c), "fitted", fitted, "compared", compared)
    assert compared >= 3 and fitted >= 5


def test_accuracy_at_another_threshold(extras):
    call = XC.make_call(*BINOMIAL_CALLS[1])
    o, p = call["offsets"], call["p"]
    for thr in (0.0, 0.35, 1.0):
        for g, tok in enumerate(extras(XC.host_input(call, 1e-12, True, 0.0, thr, True))):
            n = int(o[g + 1] - o[g])
            rec, acc, pred = split(tok, p, n)
            if rec[p + 10] == 0:
                assert acc == XC.count_accuracy(call["y"][o[g]:o[g + 1]], pred[:, 0], thr), (thr, g)
