"""CPU tier of the correlation family: csrc/rank_cor.h in its host build (tests/tools/cor_host.cpp, a program of its own compiled
under ASan / UBSan, never loaded into python) held to tests/cor_restate.py with the bounds of the GPU tier, on both size paths,
and to the tables of the reference's SQL tests as known answers."""
import os
import subprocess

import numpy as np
import pytest

import cor_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = {"pearson": R.PEARSON, "spearman": R.SPEARMAN, "kendall": R.KENDALL}


@pytest.fixture(scope="module")
def host_cor(tmp_path_factory):
    """tests/tools/cor_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a sanitizer's
    runtime could not be the first one loaded, so there the same program is built without them and the cases still run."""
    exe = str(tmp_path_factory.mktemp("cor") / "cor_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "cor_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(off, x, y, method, cap=1462, alternative=0, tau_type=1, confidence_level=0.95):
        head = [method, alternative, tau_type, confidence_level, cap, len(off) - 1, len(x)]
        data = np.concatenate([np.array(head, np.float64), np.asarray(off, np.float64), x, y]).tobytes()
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, 8)
    return run


def test_restatement_known_values():
    """The restatement itself, on hand-checked values: three concordant pairs and one tie in y."""
    rec = R.record([1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 2.0, 5.0], R.KENDALL)
    assert rec[6] == 5.0 and rec[5] == 4.0 and abs(rec[0] - 5.0 / np.sqrt(6.0 * 5.0)) < 1e-15
    assert list(R.midranks(np.array([3.0, 1.0, 3.0, 2.0]))) == [3.5, 1.0, 3.5, 2.0]
    short = R.record([1.0, np.nan, 3.0], [1.0, 2.0, np.nan], R.PEARSON)
    assert short[5] == 1.0 and short[7] == 6.0 and all(np.isnan(short[:5]))


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("method", list(METHODS))
def test_both_paths_against_the_restatement(host_cor, method, content):
    off, x, y = R.make_call(content)
    ref = R.reference(off, x, y, METHODS[method])
    small, large = host_cor(off, x, y, METHODS[method]), host_cor(off, x, y, METHODS[method], cap=128)
    for name, got in (("small", small), ("cap 128", large)):
        print(method, content, name, {k: "%.2e" % v for k, v in R.check_records(got, ref).items()})
    # the two paths: n, s, status and the estimate to the bit
    assert small[:, [0, 5, 6, 7]].tobytes() == large[:, [0, 5, 6, 7]].tobytes()


@pytest.mark.parametrize("kw", [dict(alternative=1), dict(alternative=2), dict(tau_type=0), dict(tau_type=2), dict(confidence_level=0.99),
                                dict(confidence_level=float("nan"))])
@pytest.mark.parametrize("method", list(METHODS))
def test_options(host_cor, method, kw):
    off, x, y = R.make_call("ties" if "tau_type" in kw else "noise", seed=1)
    R.check_records(host_cor(off, x, y, METHODS[method], cap=128, **kw), R.reference(off, x, y, METHODS[method], **kw))


def test_infinities_stay_in(host_cor):
    x = np.array([1.0, np.inf, 3.0, -np.inf, 5.0, np.inf, 2.0])
    y = np.array([2.0, 9.0, np.inf, -4.0, 1.0, 9.5, np.inf])
    off = np.array([0, 7], np.int64)
    for m in (R.SPEARMAN, R.KENDALL):
        R.check_records(host_cor(off, x, y, m), R.reference(off, x, y, m))
        R.check_records(host_cor(off, x, y, m, cap=4), R.reference(off, x, y, m))


def test_sql_tables_known_answers(host_cor):
    def get(table, method):
        x, y = (np.array(v) for v in R.TABLES[table])
        for cap in (1462, 4):
            rec = host_cor(np.array([0, len(x)], np.int64), x, y, method, cap=cap)[0]
            assert rec[7] == 0
        return rec[0], rec[2], rec[5]
    R.check_known_answers(get)
    R.check_known_answers(lambda table, method: [R.record(*R.TABLES[table], method)[j] for j in (0, 2, 5)])
