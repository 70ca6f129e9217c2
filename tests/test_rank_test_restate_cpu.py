"""CPU tier of the rank tests: tests/rank_test_restate.py held to scipy.stats and to hand-checked values, then csrc/rank_tests.h in
its host build (tests/tools/rank_test_host.cpp, a program of its own compiled under ASan / UBSan, never loaded into python) held to
the restatement with the bounds of the GPU tier, on both size paths, and to the tables of the reference's SQL tests."""
import os
import subprocess

import numpy as np
import pytest
from scipy import stats as sps

import rank_test_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALT = {R.TWO_SIDED: "two-sided", R.LESS: "less", R.GREATER: "greater"}


@pytest.fixture(scope="module")
def host_rank_test(tmp_path_factory):
    """tests/tools/rank_test_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a
    sanitizer's runtime could not be the first one loaded, so there the same program is built without them and the cases still
    run."""
    exe = str(tmp_path_factory.mktemp("rank_test") / "rank_test_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "rank_test_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(test, call, cap=1462, alternative=0, correction=True, mu=None):
        head = [test, alternative, int(correction), call["mu"] if mu is None else mu, cap, len(call["off"]) - 1, len(call["v"])]
        data = np.concatenate([np.array(head, np.float64), np.asarray(call["off"], np.float64), call["v"], call["y"],
                               np.asarray(call["sample"], np.float64)]).tobytes()
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, 8)
    return run


def _one(v, y=None, sample=None, mu=0.0):
    v = np.asarray(v, np.float64)
    return dict(off=np.array([0, len(v)], np.int64), v=v, y=np.zeros(len(v)) if y is None else np.asarray(y, np.float64),
                sample=np.zeros(len(v), np.int32) if sample is None else np.asarray(sample, np.int32), mu=mu)


def test_restatement_against_scipy():
    """Random tied cases: W, V and H exactly (V where scipy reports the sum of the positive ranks), p to 1e-12 relative."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for case in range(120):
        n1, n2 = int(rng.integers(2, 40)), int(rng.integers(2, 40))
        a, b = rng.integers(0, 15, n1).astype(np.float64), rng.integers(0, 15, n2).astype(np.float64)
        alt, on = case % 3, bool(case // 3 % 2)
        rec = R.record(R.MANN_WHITNEY, np.concatenate([a, b]), sample=[0] * n1 + [1] * n2, alternative=alt, correction=on)
        if len(set(a) | set(b)) > 1:
            s = sps.mannwhitneyu(a, b, use_continuity=on, alternative=ALT[alt], method="asymptotic")
            assert rec[0] == s.statistic
            worst = max(worst, abs(rec[2] - s.pvalue) / s.pvalue)
        x, y = rng.integers(0, 9, n1).astype(np.float64), rng.integers(0, 9, n1).astype(np.float64)
        if np.count_nonzero(x - y) > 0:
            rec = R.record(R.WILCOXON, x, y=y, alternative=alt, correction=on)
            s = sps.wilcoxon(x, y, zero_method="wilcox", correction=on, alternative=ALT[alt], method="approx")
            if alt != R.TWO_SIDED:
                assert rec[0] == s.statistic
            worst = max(worst, abs(rec[2] - s.pvalue) / s.pvalue)
        k = int(rng.integers(2, 6))
        ids = rng.integers(0, k, n1 + n2)
        v = rng.integers(0, 15, n1 + n2).astype(np.float64)
        rec = R.record(R.KRUSKAL_WALLIS, v, sample=ids)
        if rec[7] == 0 and not np.isnan(rec[0]):
            s = sps.kruskal(*[v[ids == j] for j in np.unique(ids)])
            assert abs(rec[0] - s.statistic) <= 1e-12 * max(1.0, abs(s.statistic))
            worst = max(worst, abs(rec[2] - s.pvalue) / s.pvalue)
    print("restatement against scipy, worst relative p difference %.2e" % worst)
    assert worst <= 1e-12


def test_restatement_known_values():
    """Hand-checked: ranks of c(1, 2 | 2, 3) are 1, 2.5, 2.5, 4, so W = 3.5 - 3 = 0.5; |d| = 1, 2, 3 with signs +, -, +: V = 4."""
    rec = R.record(R.MANN_WHITNEY, [1.0, 2.0, 2.0, 3.0], sample=[0, 0, 5, -1], correction=False)
    assert rec[0] == 0.5 and rec[4:] == [4.0, 2.0, 2.0, 0.0]
    assert abs(rec[1] - (0.5 - 2.0) / np.sqrt(4.0 / 12.0 * (5.0 - 6.0 / 12.0))) < 1e-15
    rec = R.record(R.WILCOXON, [2.0, 1.0, 5.0, 4.0, np.nan], y=[1.0, 3.0, 2.0, 4.0, 1.0], correction=False)
    assert rec[0] == 4.0 and rec[4:] == [4.0, 3.0, 1.0, 0.0] and abs(rec[1] - (4.0 - 3.0) / np.sqrt(3.5)) < 1e-15
    rec = R.record(R.KRUSKAL_WALLIS, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0], sample=[7, 7, -1, -1, 9, 9])
    assert abs(rec[0] - (12.0 / 42.0 * (9.0 + 49.0 + 121.0) / 2.0 - 21.0)) < 1e-13 and rec[3:6] == [2.0, 6.0, 3.0] and np.isnan(rec[6])
    assert abs(rec[2] - np.exp(-rec[0] / 2.0)) < 1e-15      # chi-square with 2 degrees of freedom
    assert list(R.midranks([3.0, 1.0, 3.0, 2.0])) == [3.5, 1.0, 3.5, 2.0]
    assert R.record(R.MANN_WHITNEY, [1.0, 2.0], sample=[1, 2])[4:] == [2.0, 0.0, 2.0, 6.0]
    assert R.record(R.WILCOXON, [1.0, np.nan], y=[1.0, 2.0])[4:] == [1.0, 0.0, 1.0, 6.0]
    assert R.record(R.KRUSKAL_WALLIS, [1.0, 2.0], sample=[1, 2])[7] == 6.0 and R.record(R.KRUSKAL_WALLIS, [1.0, 2.0, 3.0], sample=[1, 1, 1])[7] == 6.0
    flat = R.record(R.MANN_WHITNEY, [2.0, 2.0, 2.0], sample=[0, 1, 1])
    assert flat[0] == 1.0 and np.isnan(flat[1]) and np.isnan(flat[2]) and flat[7] == 0.0


@pytest.mark.parametrize("name, content", R.CASES)
def test_both_paths_against_the_restatement(host_rank_test, name, content):
    test = R.TESTS[name]
    call = R.make_call(test, content)
    ref = R.reference(test, call)
    small, large = host_rank_test(test, call), host_rank_test(test, call, cap=128)
    for path, got in (("small", small), ("cap 128", large)):
        print(name, content, path, {k: "%.2e" % v for k, v in R.check_records(test, got, ref).items()})
    cols = [4, 5, 6, 7] if test == R.KRUSKAL_WALLIS else [0, 4, 5, 6, 7]   # the two paths: counts, status, W and V to the bit
    assert small[:, cols].tobytes() == large[:, cols].tobytes()


@pytest.mark.parametrize("correction", [True, False])
@pytest.mark.parametrize("alternative", [R.TWO_SIDED, R.LESS, R.GREATER])
@pytest.mark.parametrize("name", ["mann_whitney", "wilcoxon"])
def test_alternatives_and_correction(host_rank_test, name, alternative, correction):
    test = R.TESTS[name]
    for content in ("ties", "shift"):
        call = R.make_call(test, content, seed=1)
        kw = dict(alternative=alternative, correction=correction)
        R.check_records(test, host_rank_test(test, call, cap=128, **kw), R.reference(test, call, **kw))


def test_infinities_stay_in(host_rank_test):
    v = np.array([1.0, np.inf, 3.0, -np.inf, 5.0, np.inf, 2.0, np.inf])
    y = np.array([2.0, 9.0, np.inf, -4.0, 1.0, 9.5, -np.inf, np.inf])     # the last pair's difference is NaN: not valid
    call = _one(v, y, [0, 1, 0, 1, 2, 0, 1, 2])
    for test in R.TESTS.values():
        for cap in (1462, 4):
            R.check_records(test, host_rank_test(test, call, cap=cap), R.reference(test, call))
    assert R.reference(R.WILCOXON, call)[0][4] == 7.0


def test_sql_tables_known_answers(host_rank_test):
    def get(test, table, alternative=R.TWO_SIDED, correction=True):
        a, b = R.TABLES[test][table]
        call = _one(a, y=b) if test == R.WILCOXON else _one(a, sample=b)
        recs = [host_rank_test(test, call, cap=cap, alternative=alternative, correction=correction)[0] for cap in (1462, 3)]
        assert test == R.KRUSKAL_WALLIS or np.array_equal(recs[0], recs[1], equal_nan=True)
        return R.as_row(recs[0])
    R.check_known_answers(get)
    R.check_known_answers(R.restated)
