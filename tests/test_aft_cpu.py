"""CPU tier of the AFT family: csrc/aft_newton.h in its host build (tests/tools/aft_host.cpp, a program of its own compiled under
ASan / UBSan, never loaded into python) on every case of tests/aft_cases.py, checked against tests/aft_restate.py with the bounds
of the GPU tier (tests/test_gpu_aft.py)."""
import os
import subprocess

import numpy as np
import pytest

import aft_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = AC.calls()
IDS = [AC.call_id(c) for c in CALLS]


@pytest.fixture(scope="module")
def host_aft(tmp_path_factory):
    """tests/tools/aft_host.cpp as a program of its own, under ASan / UBSan.  The child inherits the environment unchanged.  Where
    a process-wide LD_PRELOAD is set, a sanitizer's runtime could not be the first one loaded, so there the same program is built
    without the sanitizers and the cases still run (the sanitised run is the one on a plain environment)."""
    exe = str(tmp_path_factory.mktemp("aft") / "aft_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "aft_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(data):
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return [np.array([float(t) for t in ln.split()]) for ln in out.stdout.decode().strip().split("\n")]
    return run


def split(line, p):
    return line[:p + 13], line[p + 13:6 * p + 15], int(line[6 * p + 15])


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_default_and_tight_tolerance(host_aft, c):
    """Both runs of the GPU tier on the host build: tolerance 1e-9 (the default) and 1e-14, every bound of check_record."""
    call = AC.make_call(*c)
    refs, p = AC.reference(call), call["p"]
    for tolerance, tight in ((1e-9, False), (1e-14, True)):
        lines = host_aft(AC.host_input(call, tolerance))
        errs, n_compared, iters, ladder = {}, 0, 0, 0
        for g, (line, ref) in enumerate(zip(lines, refs)):
            rec, inf, lad = split(line, p)
            n_compared += AC.check_record(rec, inf, ref, call, g, tolerance, tight, errs)
            if rec[p + 12] == 0:
                iters, ladder = max(iters, int(rec[p + 10])), ladder + (lad > 0)
        print(IDS[CALLS.index(c)], "tolerance %g: compared %d of %d, max iterations %d, groups on the ladder %d" %
              (tolerance, n_compared, len(refs), iters, ladder), {k: "%.2e" % v for k, v in errs.items()})
        assert n_compared >= 6   # (half of the 12 groups of 63 rows or more; the share over all calls is asserted on its own)


def test_invalid_options_and_no_convergence(host_aft):
    call = AC.make_call(AC.R.WEIBULL, 2, True)
    p = call["p"]
    for data in (AC.host_input(call, float("nan")), AC.host_input(call, 1e-9, max_iterations=0), AC.host_input(call, -1.0)):
        for line in host_aft(data):
            rec, inf, _ = split(line, p)
            assert rec[p + 12] == 1 and np.all(np.isnan(rec[:p + 12])) and np.all(np.isnan(inf))
    lines = host_aft(AC.host_input(call, 1e-14, max_iterations=1))
    st = np.array([split(ln, p)[0][p + 12] for ln in lines])
    assert np.sum(st == 3) >= 10
    for ln in lines:
        rec, inf, _ = split(ln, p)
        assert rec[p + 12] == 0 or np.all(np.isnan(rec[:p + 12]))
