"""CPU tier of the sample tests: tests/sample_test_restate.py held to scipy.stats and to its identities, then csrc/sample_tests.h in
its host build (tests/tools/sample_test_host.cpp, a program of its own compiled under ASan / UBSan, never loaded into python) held
to the restatement with the bounds of the GPU tier, on both size paths, its t quantile to scipy's, and both to the tables of the
reference's SQL tests."""
import os
import subprocess

import numpy as np
import pytest
from scipy import stats as sps

import sample_test_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALT = {R.TWO_SIDED: "two-sided", R.LESS: "less", R.GREATER: "greater"}
ALT_CODE = {"two_sided": R.TWO_SIDED, "less": R.LESS, "greater": R.GREATER}


# (scipy warns about its own cancellation on the tied, all-equal cases; those cases are skipped below by their NaN)
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """tests/tools/sample_test_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a
    sanitizer's runtime could not be the first one loaded, so there the same program is built without them and the cases still
    run."""
    exe = str(tmp_path_factory.mktemp("sample_test") / "sample_test_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "sample_test_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, doubles, width):
    out = subprocess.run([exe], input=np.asarray(doubles, np.float64).tobytes(), capture_output=True)
    err = out.stderr.decode()
    assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
    return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, width)


@pytest.fixture(scope="module")
def host_sample_test(host_exe):
    def run(test, call, cap=1462, alternative=0, kind=None, mu=None, trim=None, confidence_level=0.95):
        o = call.get("opts", {})
        head = [test, alternative, o.get("kind", 0) if kind is None else kind, o.get("mu", 0.0) if mu is None else mu,
                o.get("trim", 0.2) if trim is None else trim, confidence_level, cap, len(call["off"]) - 1, len(call["v"])]
        return _run(host_exe, np.concatenate([np.array(head, np.float64), np.asarray(call["off"], np.float64), call["v"], call["y"],
                                              np.asarray(call["sample"], np.float64)]), 12)
    return run


def _one(v, sample=None, y=None, **opts):
    v = np.asarray(v, np.float64)
    return dict(off=np.array([0, len(v)], np.int64), v=v, y=np.zeros(len(v)) if y is None else np.asarray(y, np.float64),
                sample=np.zeros(len(v), np.int32) if sample is None else np.asarray(sample, np.int32), opts=opts)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def test_restatement_against_scipy():
    """Random cases with and without ties, every alternative: statistic, df, p and the t-test's interval to 1e-12 relative."""
    rng = np.random.default_rng(5)
    worst = 0.0
    sizes = [(2, 2), (2, 5), (4, 4), (5, 9), (17, 30), (64, 65), (300, 7)]
    for case in range(84):
        n1, n2 = sizes[case % len(sizes)]
        tied = case // len(sizes) % 2 == 1
        a = rng.integers(0, 9, n1).astype(np.float64) if tied else rng.standard_normal(n1)
        b = rng.integers(0, 9, n2).astype(np.float64) if tied else 0.3 + 1.5 * rng.standard_normal(n2)
        alt = case % 3
        v, s = np.concatenate([a, b]), [0] * n1 + [7] * n2
        for kind in (R.WELCH, R.STUDENT):
            rec = R.record(R.T_TEST, v, sample=s, alternative=alt, kind=kind)
            ref = sps.ttest_ind(a, b, equal_var=kind == R.STUDENT, alternative=ALT[alt])
            if np.isnan(ref.statistic) or rec[10] == 0:
                assert np.isnan(rec[0])
                continue
            ci = ref.confidence_interval(0.95)
            for got, want in ((rec[0], ref.statistic), (rec[1], ref.pvalue), (rec[2], ref.df), (rec[5], ci.low), (rec[6], ci.high)):
                if np.isinf(want):
                    assert got == want
                else:
                    worst = max(worst, _rel(got, want))
        if n1 == n2:
            rec = R.record(R.T_TEST, a, y=b, alternative=alt, kind=R.PAIRED)
            ref = sps.ttest_rel(a, b, alternative=ALT[alt])
            if not np.isnan(ref.statistic) and rec[10] > 0:
                worst = max(worst, _rel(rec[0], ref.statistic), _rel(rec[1], ref.pvalue))
        for trim in (0.0, 0.1, 0.2, 0.25):
            rec = R.record(R.YUEN, v, sample=s, alternative=alt, trim=trim)
            if rec[11] == 0 and rec[10] > 0:
                ref = sps.ttest_ind(a, b, equal_var=False, trim=trim, alternative=ALT[alt])
                worst = max(worst, _rel(rec[0], ref.statistic), _rel(rec[1], ref.pvalue))
        rec = R.record(R.BRUNNER_MUNZEL, v, sample=s, alternative=alt)
        if rec[11] == 0 and np.isfinite(rec[0]):
            ref = sps.brunnermunzel(a, b, alternative=ALT[alt], distribution="t")
            worst = max(worst, _rel(rec[0], ref.statistic), _rel(rec[1], ref.pvalue))
            assert abs(rec[0] - (rec[4] - 0.5) / rec[10]) <= 1e-12 * abs(rec[0])      # W = (phat - 1/2) / se
        c = rng.integers(0, 9, n2).astype(np.float64) if tied else rng.standard_normal(n2)
        if min(n1, n2) >= 2:
            arms = [a, b, c]
            v3, s3 = np.concatenate(arms), [4] * n1 + [-2] * n2 + [9] * n2
            rec = R.record(R.ANOVA, v3, sample=s3)
            ref = sps.f_oneway(*arms)
            if np.isfinite(ref.statistic) and rec[10] > 0:
                worst = max(worst, _rel(rec[0], ref.statistic), _rel(rec[1], ref.pvalue))
            rec = R.record(R.BROWN_FORSYTHE, v3, sample=s3)
            ref = sps.levene(*arms, center="median")
            if np.isfinite(ref.statistic) and rec[10] > 0:
                worst = max(worst, _rel(rec[0], ref.statistic), _rel(rec[1], ref.pvalue))
            # Welch ANOVA has no scipy counterpart: at k = 2 it is the Welch t-test squared, with its df
            w2, t2 = R.record(R.ANOVA, v, sample=s, kind=R.WELCH_ANOVA), R.record(R.T_TEST, v, sample=s)
            if t2[10] > 0 and not np.isnan(w2[0]):
                worst = max(worst, _rel(w2[0], t2[0] ** 2), _rel(w2[3], t2[2]))
                assert w2[2] == 1.0
    print("restatement against scipy, worst relative difference %.2e" % worst)
    assert worst <= 1e-12


def test_restatement_known_values():
    """Hand-checked: arms (1, 2, 3) and (2, 4, 6): means 2 and 4, S = 2 and 8."""
    v, s = [1.0, 2.0, 3.0, 2.0, 4.0, 6.0], [0, 0, 0, 5, -1, 5]
    rec = R.record(R.T_TEST, v, sample=s, kind=R.STUDENT)
    assert rec[4] == -2.0 and rec[2] == 4.0 and abs(rec[0] + 2.0 / np.sqrt(2.5 * 2.0 / 3.0)) < 1e-15 and rec[7:10] == [6.0, 3.0, 3.0]
    rec = R.record(R.T_TEST, v, sample=s)
    assert abs(rec[10] - np.sqrt(1.0 / 3.0 + 4.0 / 3.0)) < 1e-15 and abs(rec[2] - (5.0 / 3.0) ** 2 / ((1.0 / 9.0 + 16.0 / 9.0) / 2.0)) < 1e-14
    rec = R.record(R.T_TEST, [1.0, 2.0, 3.0, 9.0], y=[2.0, 4.0, 6.0, np.nan], kind=R.PAIRED)
    assert rec[4] == -2.0 and rec[7:10] == [3.0, 3.0, 3.0] and abs(rec[0] + 2.0 / np.sqrt(1.0 / 3.0)) < 1e-15
    rec = R.record(R.ANOVA, v, sample=[7, 7, 7, -1, -1, -1])
    assert rec[4] == 6.0 and rec[10] == 10.0 and rec[0] == 6.0 / 2.5 and rec[2:4] == [1.0, 4.0] and rec[8] == 2.0
    rec = R.record(R.BROWN_FORSYTHE, v, sample=[7, 7, 7, -1, -1, -1])      # z = (1, 0, 1) and (2, 0, 2)
    assert abs(rec[4] - 2.0 / 3.0) < 1e-15 and abs(rec[10] - (2.0 / 3.0 + 8.0 / 3.0)) < 1e-15
    rec = R.record(R.BRUNNER_MUNZEL, [1.0, 2.0, 3.0, 4.0], sample=[0, 0, 1, 1])        # complete separation
    assert rec[0] == np.inf and rec[1] == 0.0 and np.isnan(rec[2]) and rec[4:7] == [1.0, 1.0, 1.0]
    assert R.record(R.BRUNNER_MUNZEL, [1.0, 2.0, 3.0, 4.0], sample=[0, 0, 1, 1], alternative=R.LESS)[1] == 0.0
    assert R.record(R.BRUNNER_MUNZEL, [1.0, 2.0, 3.0, 4.0], sample=[0, 0, 1, 1], alternative=R.GREATER)[1] == 1.0
    rec = R.record(R.BRUNNER_MUNZEL, [2.0] * 5, sample=[0, 0, 1, 1, 1])
    assert rec[4] == 0.5 and np.isnan(rec[0]) and np.isnan(rec[1]) and rec[11] == 0.0
    rec = R.record(R.YUEN, [1.0, 2.0, 3.0, 4.0, 100.0, 1.0, 2.0, 3.0, 4.0, 5.0], sample=[0] * 5 + [1] * 5)   # g = 1: 100 is trimmed
    assert rec[4] == 0.0 and rec[0] == 0.0
    assert R.record(R.YUEN, [1.0, 2.0, 3.0, 1.0, 2.0, 3.0, 4.0], sample=[0] * 3 + [1] * 4)[11] == 6.0
    assert R.record(R.T_TEST, [1.0, 2.0, 3.0], sample=[0, 0, 1])[7:10] == [3.0, 2.0, 1.0]
    assert R.record(R.ANOVA, [1.0, 2.0, 3.0], sample=[0, 0, 1])[11] == 6.0 and R.record(R.ANOVA, [1.0, 2.0], sample=[3, 3])[11] == 6.0
    sep = R.record(R.ANOVA, [1.0, 1.0, 2.0, 2.0], sample=[0, 0, 1, 1])
    assert sep[0] == np.inf and sep[1] == 0.0 and sep[10] == 0.0


def test_t_quantile_against_scipy(host_exe):
    dfs, probs = (1.01, 1.5, 2, 3.7, 10, 100, 1e4), (0.9, 0.95, 0.975, 0.995, 0.9995)
    pairs = [(1.0 - p, df) for df in dfs for p in probs] + [(0.5, 3.0), (0.9, 2.5), (0.025, 2e5), (0.0005, 1e7)]
    got = _run(host_exe, [-1, len(pairs)] + [t for pair in pairs for t in pair], 1)[:, 0]
    worst = 0.0
    for (tail, df), q in zip(pairs, got):
        want = sps.t.isf(tail, df)
        worst = max(worst, abs(q - want) / abs(want) if tail != 0.5 else abs(q))     # (the median is 0 exactly)
    print("t quantile, worst relative difference %.2e" % worst)
    assert worst <= 1e-10


def test_t_quantile_ends_on_a_newton_step_only(host_exe):
    """Regression (found by tests/test_gpu_fuzz_stat_tests.py, Yuen and Brunner-Munzel intervals 3e-9 off): at the root the Newton
    step rounds to 0, the iterate sits on the end of its bracket, and the search took the bracket's middle instead, which it then
    returned, up to 1e-8 relative off, when the start had been within 2e-8.  6000 quantiles on a dense grid of df: 99 of 12000
    such points were more than 1e-10 off (worst 9.98e-9 at df = 22.653, tail 0.05); also df = 32 at 0.025, the paired t-test of 33
    rows."""
    dfs = np.concatenate([np.linspace(1.5, 60.0, 2000), [22.65303825956489, 32.0]])
    pairs = [(tail, df) for df in dfs for tail in (0.05, 0.025, 0.005)]
    got = _run(host_exe, [-1, len(pairs)] + [t for pair in pairs for t in pair], 1)[:, 0]
    want = np.array([sps.t.isf(tail, df) for tail, df in pairs])
    worst = np.max(np.abs(got - want) / want)
    print("t quantile on the grid, worst relative difference %.2e" % worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("name, content", R.CASES)
def test_both_paths_against_the_restatement(host_sample_test, name, content):
    test = R.TESTS[name]
    call = R.make_call(test, content)
    ref = R.reference(test, call)
    kind = call["opts"].get("kind", 0)
    small, large = host_sample_test(test, call), host_sample_test(test, call, cap=128)
    for path, got in (("small", small), ("cap 128", large)):
        print(name, content, path, {k: "%.2e" % v for k, v in R.check_records(test, got, ref, kind).items()})
    assert small.tobytes() == large.tobytes()      # the lead wavefront runs the same code on either path
    assert np.any(ref[:, 11] == 0) != (content in ("one_sample", "k2", "k3", "k7"))     # (a single-row arm: status 6)


@pytest.mark.parametrize("kw", [dict(alternative=R.LESS), dict(alternative=R.GREATER), dict(kind=R.STUDENT), dict(confidence_level=0.8),
                                dict(alternative=R.LESS, confidence_level=0.3), dict(confidence_level=float("nan"))])
def test_options_of_the_studentised_tests(host_sample_test, kw):
    for test, content in ((R.T_TEST, "shift"), (R.T_TEST, "noise"), (R.YUEN, "trim10"), (R.BRUNNER_MUNZEL, "ties")):
        if test != R.T_TEST and "kind" in kw:
            continue
        call = R.make_call(test, content, seed=1)
        R.check_records(test, host_sample_test(test, call, cap=128, **kw), R.reference(test, call, **kw), kw.get("kind", 0))


def test_welch_anova(host_sample_test):
    for content in ("noise", "ties", "all_equal", "k3", "separated"):
        call = R.make_call(R.ANOVA, content, seed=2)
        R.check_records(R.ANOVA, host_sample_test(R.ANOVA, call, cap=128, kind=R.WELCH_ANOVA), R.reference(R.ANOVA, call, kind=R.WELCH_ANOVA),
                        R.WELCH_ANOVA)


def test_identities_between_the_tests(host_sample_test):
    """Yuen at trim = 0 is the Welch t-test; two-arm Fisher ANOVA is the Student t squared; two-arm Welch ANOVA the Welch t squared."""
    call = R.make_call(R.T_TEST, "noise", seed=3)
    welch, student = host_sample_test(R.T_TEST, call), host_sample_test(R.T_TEST, call, kind=R.STUDENT)
    yuen = host_sample_test(R.YUEN, call, trim=0.0)
    fisher, welch_f = host_sample_test(R.ANOVA, call), host_sample_test(R.ANOVA, call, kind=R.WELCH_ANOVA)
    seen = 0
    for g in range(len(welch)):
        if yuen[g, 11] == 0:
            seen += 1
            for j in (0, 1, 2, 4, 5, 6):
                assert _rel(yuen[g, j], welch[g, j]) <= 1e-12
    assert seen >= 5
    # (ANOVA's arms are the ids: sample 2 of the t-test has the two ids 1 and -3, so the identity is checked on a two-id call)
    two = dict(call, sample=np.where(call["sample"] == 0, 0, 1).astype(np.int32))
    fisher, welch_f = host_sample_test(R.ANOVA, two), host_sample_test(R.ANOVA, two, kind=R.WELCH_ANOVA)
    for g in range(len(welch)):
        if fisher[g, 11] == 0:
            assert _rel(fisher[g, 0], student[g, 0] ** 2) <= 1e-12 and _rel(fisher[g, 1], student[g, 1]) <= 1e-10
            assert _rel(welch_f[g, 0], welch[g, 0] ** 2) <= 1e-12 and _rel(welch_f[g, 3], welch[g, 2]) <= 1e-12


@pytest.mark.parametrize("n1", [64, 65])
def test_second_sub_view_on_and_off_a_wavefront_boundary(host_sample_test, n1):
    rng = np.random.default_rng(n1)
    n = n1 + 71
    s = np.ones(n, np.int32)
    s[rng.permutation(n)[:n1]] = 0
    call = _one(np.round(rng.standard_normal(n), 1), s)
    for test in (R.YUEN, R.BRUNNER_MUNZEL):
        ref = R.reference(test, call)
        assert ref[0, 8] == n1
        for cap in (1462, 100):
            R.check_records(test, host_sample_test(test, call, cap=cap), ref)


def test_sql_tables_known_answers(host_sample_test):
    tables = R.load_tables(os.path.join(ROOT, "tests", "golden", "sample_tests"))

    def by_host(name, _, v, s, alternative="two_sided", **kw):
        test = R.TESTS[name]
        recs = [host_sample_test(test, _one(v, s), cap=cap, alternative=ALT_CODE[alternative], **kw)[0] for cap in (1462, 3)]
        assert np.array_equal(recs[0], recs[1], equal_nan=True)
        return R.as_row(recs[0])

    def by_restatement(name, _, v, s, alternative="two_sided", **kw):
        return R.as_row(R.record(R.TESTS[name], v, sample=s, alternative=ALT_CODE[alternative], **kw))
    R.check_known_answers(tables, by_host)
    R.check_known_answers(tables, by_restatement)
