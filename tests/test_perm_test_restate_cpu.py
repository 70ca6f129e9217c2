"""CPU tier of the permutation tests: tests/perm_test_restate.py held to scipy, to dense formulas and to hand values; the sampler's
uniformity; the property tables of the reference's SQL test; then csrc/perm_tests.h in its host build (tests/tools/
perm_test_host.cpp, a program of its own compiled under ASan / UBSan, never loaded into python) held to the restatement on both
size paths."""
import csv
import itertools
import os
import subprocess

import numpy as np
import pytest
from scipy import stats as sps

import perm_test_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "perm_tests")
TABLE_SEED = 20261021   # recorded: the restatement satisfies every property of the tables with it
# the host build's MMD statistic against the restatement, relative: measured 0 on the machine this was written on (glibc's exp
# and numpy's agreed on every input); ten times nothing is no bound for another libm, so the bound is the GPU tier's
MMD_HOST_BOUND = 1e-14
NAN = float("nan")


def _observed(v, s, test, sigma=NAN):
    return R.group_record(v, s, test, 0, 0, 0, sigma)


def _labels(g1, g2):
    return np.concatenate([g1, g2]), np.concatenate([np.zeros(len(g1), np.int32), np.ones(len(g2), np.int32)])


@pytest.mark.parametrize("ties", [False, True])
def test_energy_distance_against_scipy(ties):
    rng = np.random.default_rng(1)
    for n1, n2 in ((2, 2), (3, 7), (40, 25), (150, 151)):
        g1, g2 = rng.normal(size=n1), rng.normal(0.4, 1.3, size=n2)
        if ties:
            g1, g2 = np.round(g1 * 3), np.round(g2 * 3)
        want = sps.energy_distance(g1, g2) ** 2 * n1 * n2 / (n1 + n2)
        got = _observed(*_labels(g1, g2), R.ENERGY)[0]
        assert got == pytest.approx(want, rel=1e-12, abs=1e-13)
        assert _observed(*_labels(g2, g1), R.ENERGY)[0].tobytes() == got.tobytes()   # the samples swapped: the same bits


def test_energy_distance_by_hand():
    """(1, 2 | 2, 3): z = 1, 2, 2, 3 with the labels x x y y (the tie keeps its order), gaps 1, 0, 1.
    k = 0: a = 1, b = 0: sxx = 1 * 1 * 1 = 1, sxy = 1 * (1 * 2 + 0) = 2.   k = 1: the gap is 0.
    k = 2: a = 2, b = 1: sxx += 0, syy = 1 * 1 * 1 = 1, sxy += 2 * 1 + 1 * 0 = 2 -> sxx = 1, syy = 1, sxy = 4.
    E = 2 * 2 / 4 * (2 * 4 / 4 - 2 * 1 / 4 - 2 * 1 / 4) = 1.  (Directly: E|X - Y| = (1 + 2 + 0 + 1) / 4 = 1, E|X - X'| = E|Y - Y'| =
    1 / 2, 2 * 1 - 1 / 2 - 1 / 2 = 1.)"""
    assert _observed(*_labels(np.array([1.0, 2.0]), np.array([2.0, 3.0])), R.ENERGY)[0] == 1.0


def test_welch_t_against_scipy():
    rng = np.random.default_rng(2)
    for n1, n2, shift in ((2, 2, 0.0), (5, 9, 1.0), (60, 33, -0.5), (400, 390, 1e3)):
        g1, g2 = rng.normal(shift, 1.0, size=n1) + 50.0, rng.normal(0.0, 2.0, size=n2) + 50.0
        rec = _observed(*_labels(g1, g2), R.T_TEST)
        want = sps.ttest_ind(g1, g2, equal_var=False)
        # (sums of squares about the median element: the cancellation left is that of the spread, not of the level)
        assert rec[0] == pytest.approx(want.statistic, rel=1e-10)
        assert rec[2] == pytest.approx(want.df, rel=1e-10)
    const = _observed(*_labels(np.full(3, 2.0), np.full(4, 2.0)), R.T_TEST)
    assert const[7] == 0 and np.isnan(const[0]) and np.isnan(const[1])


def test_mmd_and_sigma_against_dense_formulas():
    rng = np.random.default_rng(3)
    for n1, n2, sigma in ((2, 2, NAN), (7, 12, NAN), (70, 61, 0.8), (64, 65, NAN)):
        g1, g2 = rng.normal(size=n1), rng.normal(0.5, 1.0, size=n2)
        rec = _observed(*_labels(g1, g2), R.MMD, sigma)
        x = np.concatenate([g1, g2])
        d = np.abs(x[:, None] - x[None, :])[np.triu_indices(len(x), 1)]
        want_sigma = np.partition(d, (len(d) + 1) // 2 - 1)[(len(d) + 1) // 2 - 1] if sigma != sigma else sigma
        assert rec[2] == pytest.approx(want_sigma, rel=1e-15)
        k = lambda a, b: np.exp(-(a[:, None] - b[None, :]) ** 2 / (2.0 * rec[2] ** 2))   # noqa: E731
        want = k(g1, g1).mean() + k(g2, g2).mean() - 2.0 * k(g1, g2).mean()
        assert rec[0] == pytest.approx(want, rel=1e-11, abs=1e-15)
        assert _observed(*_labels(g2, g1), R.MMD, sigma)[0].tobytes() == rec[0].tobytes()
    tied = _observed(*_labels(np.array([1.0, 1.0, 1.0]), np.array([1.0, 1.0, 2.0])), R.MMD)
    assert tied[7] == 0 and tied[2] == 0.0 and np.isnan(tied[0])


def test_pair_order():
    assert R.pair_order(0, 3).tolist() == [2, 1]
    assert R.pair_order(62, 130).tolist() == [63] + list(range(127, 63, -1)) + [129, 128]
    assert R.pair_order(64, 67).tolist() == [66, 65]


def test_the_sampler_is_uniform():
    """N = 6, n1 = 3, B = 20000: the 20 subsets' frequencies under a chi-square test.  The seed is fixed, so this is deterministic."""
    labels = R.draw_labels(12345, 20000, 6, 3)
    assert (labels.sum(axis=0) == 3).all()
    codes = (labels * (1 << np.arange(6))[:, None]).sum(axis=0)
    subsets = [sum(1 << i for i in c) for c in itertools.combinations(range(6), 3)]
    counts = np.array([(codes == c).sum() for c in subsets])
    assert counts.sum() == 20000
    p = sps.chisquare(counts).pvalue
    print("chi-square p of the 20 subsets:", p)
    assert p > 1e-4


def test_the_stream_depends_on_seed_permutation_and_row_alone():
    a, b = R.draw_labels(9, 100, 10, 4), R.draw_labels(9, 70, 10, 4)
    assert np.array_equal(a[:, :70], b) and not np.array_equal(a, R.draw_labels(10, 100, 10, 4))


def _table(name):
    with open(os.path.join(GOLDEN, name)) as f:
        rows = list(csv.DictReader(f))
    out = {}
    for r in rows:
        out.setdefault(r["table"], ([], []))
        out[r["table"]][0].append(float(r["value"]))
        out[r["table"]][1].append(int(r["grp"]))
    return {k: (np.array(v), np.array(s, np.int32)) for k, (v, s) in out.items()}


def test_property_tables_of_the_reference():
    """test/sql/distribution/test_distribution_tests.test: n1 = n2 = 10, a statistic >= 0, p < 0.05 on the tables that differ and
    p > 0.05 on those that do not, at B = 1000."""
    tables = _table("distribution_tables.csv")
    for test in (R.ENERGY, R.MMD):
        diff, same = (R.group_record(*tables[t], test, 0, 1000, TABLE_SEED) for t in ("different", "same"))
        assert (diff[5], diff[6]) == (10, 10) and diff[0] >= 0 and same[0] >= 0
        assert diff[1] < 0.05 < same[1]
    assert R.group_record(*tables["different"], R.MMD, 0, 1000, TABLE_SEED, 1.0)[0] > 0     # a given bandwidth
    grouped = _table("grouped_tables.csv")
    assert R.group_record(*grouped["diff"], R.ENERGY, 0, 1000, TABLE_SEED)[1] < 0.05
    assert not R.group_record(*grouped["same"], R.ENERGY, 0, 1000, TABLE_SEED)[1] < 0.05


# ---- csrc/perm_tests.h in its host build ----

@pytest.fixture(scope="module")
def host_perm_test(tmp_path_factory):
    """tests/tools/perm_test_host.cpp as a program of its own, under ASan / UBSan.  Where a process-wide LD_PRELOAD is set a
    sanitizer's runtime could not be the first one loaded, so there the same program is built without them and the cases still
    run."""
    exe = str(tmp_path_factory.mktemp("perm_test") / "perm_test_host")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        os.path.join(ROOT, "tests", "tools", "perm_test_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(call, test, alternative=0, n_perm=1000, seed=0, sigma=NAN, cap=R.CAP):
        off, v, s = call
        head = [test, alternative, n_perm, seed >> 32, seed & 0xFFFFFFFF, sigma, cap, len(off) - 1, len(v)]
        data = np.concatenate([np.array(head, np.float64), off.astype(np.float64), v, s.astype(np.float64)]).tobytes()
        out = subprocess.run([exe], input=data, capture_output=True)
        err = out.stderr.decode()
        assert out.returncode == 0, out.stdout.decode()[-2000:] + err[-4000:]
        assert "ERROR" not in err and "runtime error" not in err, err[-4000:]
        return np.array([float(t) for t in out.stdout.decode().split()]).reshape(-1, 8)
    return run


@pytest.fixture(scope="module")
def call():
    rng = np.random.default_rng(11)
    i32 = lambda a: np.asarray(a, np.int32)   # noqa: E731
    groups = [R.make_group(rng, n, ties=t, nan_share=ns) for n, t, ns in ((4, 0, 0), (5, 0, 0.2), (63, 0.5, 0), (64, 0, 0), (65, 0, 0.1),
                                                                          (130, 0.3, 0), (200, 0, 0), (257, 0, 0))]
    groups += [(np.array([1.0, np.inf, 2.0, 3.0, 4.0]), i32([0, 0, 1, 1, 0])), (np.array([1.0, 2.0, 3.0]), i32([0, 0, 1])),
               (np.zeros(0), i32([])), (np.array([1.0, 1.0, 1.0, 1.0, 1.0, 2.0]), i32([0, 0, 0, 1, 1, 1])),
               (np.full(6, 1.0), i32([0, 0, 0, 1, 1, 1]))]
    return R.pack(groups)


SEED = 0x123456789ABCDEF1


@pytest.mark.parametrize("n_perm", [0, 1, 65, 1000])
@pytest.mark.parametrize("test, alternative", [(R.ENERGY, 0), (R.T_TEST, 0), (R.T_TEST, 1), (R.T_TEST, 2)])
def test_host_build_equals_the_restatement_to_the_bit(host_perm_test, call, test, alternative, n_perm):
    for cap in (R.CAP, 16):   # 16: the groups of 17 rows and more take the large path
        ref = R.reference(*call, test, alternative, n_perm, SEED, cap=cap)
        got = host_perm_test(call, test, alternative, n_perm, SEED, cap=cap)
        assert np.array_equal(got, ref, equal_nan=True), (cap, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref)))).tolist())


@pytest.mark.parametrize("n_perm, sigma", [(0, NAN), (1, NAN), (65, NAN), (200, NAN), (65, 0.9)])
def test_host_build_mmd(host_perm_test, call, n_perm, sigma):
    for cap in (R.CAP, 16):
        ref = R.reference(*call, R.MMD, 0, n_perm, SEED, sigma, cap)
        got = host_perm_test(call, R.MMD, 0, n_perm, SEED, sigma, cap)
        assert np.array_equal(got[:, 1:], ref[:, 1:], equal_nan=True)     # sigma to the bit, n_extreme, p, the counts, the status
        assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref[:, 0]))
        if not np.isnan(ref[:, 0]).all():
            err = np.nanmax(np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-3))
            print("MMD host build, B", n_perm, "cap", cap, "statistic error %.3e" % err)
            assert err <= MMD_HOST_BOUND
    assert (got[:8, 7] == [0, 0, 7, 7, 7, 7, 7, 7]).all()                  # cap 16: MMD's status 7 above it
