"""CPU tier of the mixed-model family: csrc/lmm_profile.h in its host build (tests/tools/glmm_host.cpp, a program of its own
compiled under ASan / UBSan, never loaded into python) on every case of tests/glmm_cases.py, with the library's wavefront count
and with each of 1, 4 and 16 forced, checked against tests/glmm_restate.py."""
import os
import subprocess

import numpy as np
import pytest

import glmm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = GC.calls()


@pytest.fixture(scope="module")
def host_glmm(tmp_path_factory):
    """The child inherits the environment unchanged.  Where a process-wide LD_PRELOAD is set, a sanitizer's runtime could not be
    the first one loaded, so there the same program is built without the sanitizers and the cases still run."""
    exe = str(tmp_path_factory.mktemp("glmm") / "glmm_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "glmm_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("glmm_host built", "with ASan / UBSan" if sanitize else "WITHOUT sanitizers (LD_PRELOAD is set)")

    def run(call, waves=0, **kw):
        out = subprocess.run([exe], input=GC.host_input(call, waves, **kw), capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        lines = out.stdout.decode().split("\n")
        return [np.array([float(t) for t in lines[i].split()]) for i in range(3)] + [np.array([int(t) for t in lines[3].split()])]
    return run


@pytest.mark.parametrize("name", list(CALLS))
def test_cases_against_the_restatement(host_glmm, name):
    call = CALLS[name]
    refs = GC.reference(name, call)
    for waves in (0, 1, 4, 16):
        errs = {}
        n, left = GC.check(call, refs, *host_glmm(call, waves), errs, GC.CPU_BOUNDS)
        print(name, "waves %d: compared %d, left out %d" % (waves, n, left), {k: "%.2e" % v for k, v in errs.items()})
        assert left == 0 and n == len(refs)


def test_statuses_and_their_neighbours(host_glmm):
    good = [GC.panel((5, 6, 7, 8), 2, s) for s in (1, 2)]
    none = GC.panel((3, 3), 2, 7)
    none[1][:] = np.nan
    call = GC.make_call([good[0], GC.panel((9,), 2, 4), GC.panel((1, 1, 1, 1, 1, 1), 2, 5), GC.panel((2, 2), 2, 6), good[1], none])
    rec, inf, ranef, ln = host_glmm(call)
    assert list(rec.reshape(-1, 15)[:, 14]) == [0, 1, 1, 6, 0, 10]
    alone = host_glmm(GC.make_call(good))
    assert np.array_equal(rec.reshape(-1, 15)[[0, 4]], alone[0].reshape(-1, 15))
    bad = host_glmm(call, tolerance=float("nan"))
    assert np.all(bad[0].reshape(-1, 15)[:, 14] == 1) and np.all(np.isnan(bad[2]))


def test_an_aliased_column_is_dropped(host_glmm):
    sizes, y, X = GC.panel((6, 7, 8, 9), 2, 9)
    X = np.column_stack([X, np.full(len(y), 3.0), X[:, 0] - 2.0 * X[:, 1]])   # a constant column and a combination of the first two
    rec, inf, ranef, ln = host_glmm(GC.make_call([(sizes, y, X)]))
    ref = GC.reference("aliased", GC.make_call([(sizes, y, X[:, :2])]))[0]
    assert rec[4 + 12] == 0 and np.isnan(rec[2]) and np.isnan(rec[3]) and np.isnan(inf[2]) and np.isnan(inf[3])
    assert np.allclose(rec[:2], ref["beta"][1:], rtol=1e-9) and abs(rec[4 + 4] - ref["ell"]) <= 1e-9 * abs(ref["ell"])


def test_the_iteration_cap_returns_the_last_iterate(host_glmm):
    call = CALLS["fixtures-reml"]
    rec = host_glmm(call, max_iterations=2)[0].reshape(-1, 14)
    assert rec[0, 13] == 0 and rec[0, 12] == 0 and rec[0, 11] == 2 and np.isfinite(rec[0, 2])
