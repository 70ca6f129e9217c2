"""CPU tier of the AFT prediction pass: csrc/aft_newton.h in its host build with an_predict (tests/tools/aft_predict_host.cpp, a
program of its own compiled under ASan / UBSan, never loaded into python) on the seeded cases of tests/aft_cases.py extended with
rows to score only (tests/aft_predict_cases.py), with the rules and bounds of the GPU tier (tests/test_gpu_aft_predict.py)."""
import os
import subprocess

import numpy as np
import pytest

import aft_cases as AC
import aft_predict_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = PC.calls()
IDS = [AC.call_id(c) for c in CALLS]


@pytest.fixture(scope="module")
def host_predict(tmp_path_factory):
    """tests/tools/aft_predict_host.cpp as a program of its own, under ASan / UBSan.  The child inherits the environment unchanged;
    where a process-wide LD_PRELOAD is set a sanitizer's runtime could not be the first one loaded, so there the same program is
    built without the sanitizers and the cases still run (as tests/test_aft_cpu.py does)."""
    exe = str(tmp_path_factory.mktemp("aft_predict") / "aft_predict_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "aft_predict_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(data):
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return [np.array([float(t) for t in ln.split()]) for ln in out.stdout.decode().strip().split("\n")]
    return run


def split(line, p):
    """-> (rec, inf, rec of the run without the pass, inf of that run, pred[n, 4])"""
    a, b = p + 13, 5 * p + 2
    return line[:a], line[a:a + b], line[a + b:2 * a + b], line[2 * a + b:2 * (a + b)], line[2 * (a + b):].reshape(-1, 4)


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_prediction_pass(host_predict, c):
    """Every rule of check_pred on every group; the record and the inference are those of the run without the pass; and the rows to
    score left the record what the training rows alone give."""
    call = PC.make_call(*c)
    p, h = call["p"], PC.horizon_of(call)
    lines = host_predict(PC.host_input(call, 0.3, h))
    alone = host_predict(PC.host_input(call["base"], 0.3, h))
    errs, n_tight, n_rows = {}, 0, 0
    for g, line in enumerate(lines):
        rec, inf, rec0, inf0, pred = split(line, p)
        assert PC.same_values(rec, rec0) and PC.same_values(inf, inf0), "group %d: the pass changed the record" % g
        assert PC.same_values(rec, split(alone[g], p)[0]), "group %d: rows to score changed the record" % g
        n_tight += PC.check_pred(pred, rec, call, g, 0.3, h, errs)
        n_rows += len(pred) if rec[p + 12] == 0 else 0
        if call["kinds"][g] in AC.EXPECTED_STATUS:
            assert rec[p + 12] == AC.EXPECTED_STATUS[call["kinds"][g]] and np.all(np.isnan(pred))
    print(IDS[CALLS.index(c)], "rows of fitted groups %d, under the tight bound %d" % (n_rows, n_tight), {k: "%.2e" % v for k, v in errs.items()})
    # (the rest: rows that are not scored in full, and the groups of k + 1 and k + 2 rows, which the fit all but interpolates)
    assert n_tight >= 0.5 * n_rows


@pytest.mark.parametrize("c", [(d, 8, True) for d in AC.DISTS], ids=[AC.R.NAMES[d] for d in AC.DISTS])
def test_known_answers(host_predict, c):
    """No horizon: risk all NaN, the rest unchanged.  Horizon 0: risk exactly +0.  The median of a lognormal time is exp(eta)."""
    call = PC.make_call(*c)
    p = call["p"]
    with_h = host_predict(PC.host_input(call, 0.5, PC.horizon_of(call)))
    none = host_predict(PC.host_input(call, 0.5, None))
    zero = host_predict(PC.host_input(call, 0.5, 0.0))
    for g in range(len(with_h)):
        rec, _, _, _, pred = split(with_h[g], p)
        pn, pz = split(none[g], p)[4], split(zero[g], p)[4]
        assert PC.same_values(pred[:, :3], pn[:, :3]) and PC.same_values(pred[:, :3], pz[:, :3])
        assert np.all(np.isnan(pn[:, 3]))
        PC.check_pred(pn, rec, call, g, 0.5, None)
        PC.check_pred(pz, rec, call, g, 0.5, 0.0)
        if rec[p + 12] == 0 and c[0] == AC.R.LOGNORMAL:
            ok = np.isfinite(pred[:, 0])
            want = np.exp(pred[ok, 0])
            assert np.all(np.abs(pred[ok, 1] - want) <= np.spacing(want))


def test_invalid_options_score_nothing(host_predict):
    call = PC.make_call(AC.R.WEIBULL, 1, True)
    for line in host_predict(PC.host_input(call, 0.5, 1.0, tolerance=float("nan"))):
        rec, inf, rec0, inf0, pred = split(line, 1)
        assert rec[13] == 1 and np.all(np.isnan(pred)) and PC.same_values(rec, rec0)
