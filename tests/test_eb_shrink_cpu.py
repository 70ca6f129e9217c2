"""CPU tier of eb_shrink: csrc/eb_shrink.h in its host build (tests/tools/eb_shrink_host.cpp, a program of its own compiled under
ASan / UBSan, never loaded into python) on every case of tests/eb_shrink_cases.py, both paths, checked against
tests/eb_shrink_restate.py with the bounds of the GPU tier."""
import os
import subprocess

import numpy as np
import pytest

import eb_shrink_cases as EC
import eb_shrink_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = EC.calls()
IDS = [EC.call_id(c) for c in CALLS]


def build_host(tmp_path_factory):
    """tests/tools/eb_shrink_host.cpp as a program of its own, under ASan / UBSan.  The child inherits the environment unchanged.
    Where a process-wide LD_PRELOAD is set, a sanitizer's runtime could not be the first one loaded, so there the same program is
    built without the sanitizers and the cases still run (the sanitised run is the one on a plain environment)."""
    exe = str(tmp_path_factory.mktemp("eb") / "eb_shrink_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "eb_shrink_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("eb_shrink_host built", "with ASan / UBSan" if sanitize else "WITHOUT sanitizers (LD_PRELOAD is set)")

    def run(call, path=1, chunk=0):
        out = subprocess.run([exe], input=EC.host_input(call, path, chunk), capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        lines = out.stdout.decode().split("\n")
        return np.array([float(t) for t in lines[1].split()]), np.array([float(t) for t in lines[0].split()])
    return run


@pytest.fixture(scope="module")
def host_eb(tmp_path_factory):
    return build_host(tmp_path_factory)


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_both_paths_against_the_restatement(host_eb, c):
    call = EC.make_call(*c)
    ref = EC.reference(call, c)
    for path, chunk in ((1, 0), (2, 0), (2, 7)):
        errs = {}
        n, left = EC.check(call, *host_eb(call, path, chunk), ref, errs)
        print(EC.call_id(c), "path %d chunk %d: compared %d, left out %d" % (path, chunk, n, left), {k: "%.2e" % v for k, v in errs.items()})
        assert n >= 8 * c[1]


@pytest.mark.parametrize("c", EC.wide_calls(), ids=[EC.call_id(c) for c in EC.wide_calls()])
def test_raw_wide_se_draw(host_eb, c):
    """se log-uniform over 1e-3 .. 1e3 per pair, a set's weights up to 12 decades apart: the lanes and seams with such weights;
    what does not pass through C by plain bounds, what does by the bound times Sw / C (eb_shrink_cases.check_wide)."""
    call = EC.make_call(*c)
    ref = EC.reference(call, c)
    for path, chunk in ((1, 0), (2, 0), (2, 7)):
        errs = {}
        n = EC.check_wide(call, *host_eb(call, path, chunk), ref, errs)
        print(EC.call_id(c), "path %d chunk %d: compared %d" % (path, chunk, n), {k: "%.2e" % v for k, v in errs.items()})
        assert n >= 8 * c[1]


@pytest.mark.parametrize("n_cols", [1, 9])
@pytest.mark.parametrize("chunk", [64, 100])
def test_chunk_seams(host_eb, n_cols, chunk):
    call = EC.chunk_call(n_cols, 7)
    errs = {}
    assert EC.check(call, *host_eb(call, 2, chunk), EC.reference(call, ("chunk", n_cols)), errs)[0] == n_cols


def test_wide_calls_go_by_column_blocks(host_eb):
    call = EC.make_call("heterogeneous", 70, "loose", 11, sizes=(3, 40, 0, 65), sparse=False)
    ref = EC.reference(call)
    for path, chunk in ((1, 0), (2, 16)):
        EC.check(call, *host_eb(call, path, chunk), ref, {})


@pytest.mark.parametrize("kw", [dict(method=R.NONE), dict(tau_squared=0.04), dict(tau_squared=0.0), dict(tau_squared=-1.0),
                                dict(tau_squared=float("inf")), dict(method=5)])
def test_options(host_eb, kw):
    call = EC.make_call("heterogeneous", 2, "glm", 5, **kw)
    ref = EC.reference(call)
    invalid = R.options_invalid(call["method"], call["tau_squared"])
    for path, chunk in ((1, 0), (2, 50)):
        out, summary = host_eb(call, path, chunk)
        EC.check(call, out, summary, ref, {})
        if invalid:
            assert np.all(summary.reshape(-1, 8)[:, 7] == 1) and np.all(np.isnan(out))
