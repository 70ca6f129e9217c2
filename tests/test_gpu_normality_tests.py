"""GPU tier of the normality tests: anofox_hip_normality_test_batch_{host,device} on the shapes of tests/normality_test_restate.py
(groups of 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 63, 64, 65, 129 and 300 valid rows in one call, for every content), with the cap
hooked to 128 (129 and 300 on the large path) and at the default cap, against the restatement within the host program's bounds;
the two paths against each other; the tier boundaries; the row limit of Shapiro-Wilk; several large groups in one call; calls of
other families in between; the four families' hooks; the scalars and the aggregates on the tables of the reference's SQL tests."""
import os

import numpy as np
import pytest

import cor_restate
import normality_test_restate as R
import rank_test_restate
import sample_test_restate
from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu
_EXACT = [0, 6, 7]      # W, n and the status: the same bits on both size paths


@pytest.fixture(scope="module")
def calls():
    """content -> (call, {test: reference records}); computed once, read by every test."""
    out = {}
    for content in R.CONTENTS:
        call = R.make_call(content)
        out[content] = (call, {t: R.reference(t, call) for t in R.TESTS.values()})
    return out


@pytest.fixture()
def pkg():
    p = import_pkg()
    yield p
    p.normality_test_hooks(0)


def _random_call(seed, sizes):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(off=off, v=np.round(rng.standard_normal(off[-1]), 2))


def _every_test(pkg, call, cap):
    """-> {test: records} of the call at the cap, each held to the restatement."""
    pkg.normality_test_hooks(cap)
    out = {}
    for test in R.TESTS.values():
        out[test] = pkg.normality_test_batch_host(call["off"], call["v"], test)
        R.check_records(test, out[test], R.reference(test, call))
    return out


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("name", list(R.TESTS))
def test_both_paths_against_the_restatement_and_each_other(pkg, calls, name, content):
    import torch
    test = R.TESTS[name]
    call, refs = calls[content]
    dev = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    ctx = pkg.Context(0)
    got = {}
    for cap in (128, 0):
        pkg.normality_test_hooks(cap)
        host = pkg.normality_test_batch_host(call["off"], call["v"], test, ctx=ctx)
        rec = ctx.normality_test_batch_device(dev(call["off"]), dev(call["v"]), test)
        torch.cuda.synchronize()
        assert rec.cpu().numpy().tobytes() == host.tobytes()        # host and device entries: the same bytes
        errs = R.check_records(test, host, refs[test])
        print(name, content, "cap", cap or "default", {k: "%.2e" % e for k, e in errs.items()})
        got[cap] = host
    ctx.close()
    assert got[128][:, _EXACT].tobytes() == got[0][:, _EXACT].tobytes()


def test_tier_boundaries_at_the_default_cap(pkg):
    """Groups of 256, 257, 1462 and 1463 rows: at the default cap both small instances and the large path."""
    _every_test(pkg, _random_call(17, [256, 257, 1462, 1463]), 0)


def test_row_limit_of_shapiro_wilk(pkg):
    """One group of 5000 rows and one of 5001: the second has status invalid input with n = 5001."""
    call = _random_call(23, [5000, 5001])
    out = _every_test(pkg, call, 0)
    sw = out[R.SHAPIRO_WILK]
    assert list(sw[:, 6]) == [5000.0, 5001.0] and list(sw[:, 7]) == [0.0, 1.0] and np.all(np.isnan(sw[1, :6]))
    assert np.all(out[R.JARQUE_BERA][:, 7] == 0) and np.all(out[R.DAGOSTINO_K2][:, 7] == 0)


def test_several_large_groups_in_one_call(pkg):
    """Five groups above the hooked cap and one below it in one call."""
    call = _random_call(7, [130, 257, 40, 700, 129, 300])
    large, small = _every_test(pkg, call, 128), _every_test(pkg, call, 0)
    for test in R.TESTS.values():
        assert small[test][:, _EXACT].tobytes() == large[test][:, _EXACT].tobytes()


def test_calls_of_other_families_in_between(pkg, calls):
    """A sample-test call and a rank-test call between two identical normality calls: identical bytes."""
    call, _ = calls["normal"]
    other = sample_test_restate.make_call(sample_test_restate.BRUNNER_MUNZEL, "noise")
    pkg.normality_test_hooks(128)
    for test in R.TESTS.values():
        first = pkg.normality_test_batch_host(call["off"], call["v"], test)
        pkg.sample_test_batch_host(other["off"], other["v"], None, other["sample"], sample_test_restate.BRUNNER_MUNZEL)
        pkg.rank_test_batch_host(other["off"], other["v"], None, other["sample"], rank_test_restate.MANN_WHITNEY)
        assert pkg.normality_test_batch_host(call["off"], call["v"], test).tobytes() == first.tobytes()


def test_the_hook_leaves_the_other_families_caps_alone(pkg):
    """One 300-row group through a Shapiro-Wilk, a Brunner-Munzel, a Mann-Whitney and a Spearman call, with this family's cap hooked
    to 128 and then each of the other three's: every record within its bounds, and the exact columns as with none hooked."""
    rng = np.random.default_rng(19)
    call = dict(off=np.array([0, 300], np.int64), v=np.round(rng.standard_normal(300), 1), y=np.round(rng.standard_normal(300), 1),
                sample=rng.choice(np.array([0, 1], np.int32), 300), opts={}, mu=0.0)
    S, K = sample_test_restate, rank_test_restate
    refs = (R.reference(R.SHAPIRO_WILK, call), S.reference(S.BRUNNER_MUNZEL, call), K.reference(K.MANN_WHITNEY, call),
            cor_restate.reference(call["off"], call["v"], call["y"], cor_restate.SPEARMAN))

    def all_four(normality_cap, sample_cap, rank_cap, cor_cap):
        pkg.normality_test_hooks(normality_cap)
        pkg.sample_test_hooks(sample_cap)
        pkg.rank_test_hooks(rank_cap)
        pkg.cor_test_hooks(cor_cap)
        return (pkg.normality_test_batch_host(call["off"], call["v"], R.SHAPIRO_WILK),
                pkg.sample_test_batch_host(call["off"], call["v"], None, call["sample"], S.BRUNNER_MUNZEL),
                pkg.rank_test_batch_host(call["off"], call["v"], None, call["sample"], K.MANN_WHITNEY),
                pkg.cor_batch_host(call["off"], call["v"], call["y"], cor_restate.SPEARMAN))
    try:
        plain = all_four(0, 0, 0, 0)
        for caps in ((128, 0, 0, 0), (0, 128, 0, 0), (0, 0, 128, 0), (0, 0, 0, 128)):
            sw, bm, mw, rho = all_four(*caps)
            R.check_records(R.SHAPIRO_WILK, sw, refs[0])
            S.check_records(S.BRUNNER_MUNZEL, bm, refs[1])
            K.check_records(K.MANN_WHITNEY, mw, refs[2])
            cor_restate.check_records(rho, refs[3])
            assert sw[:, _EXACT].tobytes() == plain[0][:, _EXACT].tobytes()
            assert bm[:, [4, 7, 8, 9, 11]].tobytes() == plain[1][:, [4, 7, 8, 9, 11]].tobytes()
            assert mw[:, [0, 4, 5, 6, 7]].tobytes() == plain[2][:, [0, 4, 5, 6, 7]].tobytes()
            assert rho[:, [0, 5, 6, 7]].tobytes() == plain[3][:, [0, 5, 6, 7]].tobytes()
    finally:
        pkg.cor_test_hooks(0)
        pkg.rank_test_hooks(0)
        pkg.sample_test_hooks(0)
        pkg.normality_test_hooks(0)


def test_empty_call_and_empty_groups(pkg):
    none = np.zeros(0)
    assert pkg.normality_test_batch_host(np.zeros(1, np.int64), none, R.SHAPIRO_WILK).shape == (0, 8)
    for test in R.TESTS.values():
        rec = pkg.normality_test_batch_host(np.array([0, 0, 0], np.int64), none, test)
        assert np.all(rec[:, 7] == 6) and np.all(rec[:, 6] == 0) and np.all(np.isnan(rec[:, :6]))


def test_scalars_and_aggregates_reproduce_the_sql_tables(pkg):
    tables = R.load_tables(os.path.join(ROOT, "tests", "golden", "normality_tests"))
    scalar = {"shapiro_wilk": pkg.shapiro_wilk, "dagostino_k2": pkg.dagostino_k2, "jarque_bera": pkg.jarque_bera}
    agg = {"shapiro_wilk": pkg.shapiro_wilk_agg, "dagostino_k2": pkg.dagostino_k2_agg, "jarque_bera": pkg.jarque_bera_agg}
    text = {"shapiro_wilk": "Shapiro-Wilk test", "dagostino_k2": "D'Agostino K-squared test", "jarque_bera": "Jarque-Bera test"}

    def by_scalar(name, _, v):
        d = scalar[name](v)
        ref = R.record(R.TESTS[name], v)
        assert d["n"] == len(v) and abs(d["statistic"] - ref[0]) <= 1e-9 * max(1.0, abs(ref[0]))
        if name == "jarque_bera":
            assert set(d) == {"statistic", "p_value", "skewness", "kurtosis", "n"}
            return d
        assert d["method"] == text[name] and (d["n1"], d["n2"], d["alternative"]) == (0, 0, 0)
        assert (d["df"] == 2.0 if name == "dagostino_k2" else np.isnan(d["df"]))
        assert all(np.isnan(d[f]) for f in ("effect_size", "ci_lower", "ci_upper", "confidence_level"))
        return d
    R.check_known_answers(tables, by_scalar)

    def by_agg(name, table, _):
        names = list(tables[name])
        keys = np.concatenate([[t] * len(tables[name][t]) for t in names])
        d = agg[name](keys, np.concatenate([tables[name][t] for t in names])).by_key()[table]
        assert d["method"] == text[name]
        return d
    R.check_known_answers(tables, by_agg)
    # a None is a NULL: the row is not valid; a key with too few rows, or (K2, Jarque-Bera) without spread, is NULL
    res = pkg.shapiro_wilk_agg(["a"] * 4 + ["b"] * 3, [1.0, 2.0, None, 4.0, 1.0, None, 3.0])
    assert res.row(1) is None and res.row(0)["n"] == 3 and abs(res.row(0)["statistic"] - 27.0 / 28.0) <= 1e-14
    assert pkg.jarque_bera_agg(["a"] * 4, [2.0] * 4).row(0) is None and pkg.shapiro_wilk_agg(["a"] * 4, [2.0] * 4).row(0)["p_value"] == 1.0
    row = pkg.dagostino_k2_agg(["a"] * 9, np.arange(9.0) ** 2).row(0)
    assert set(row) == {"statistic", "p_value", "skewness", "kurtosis", "z_skewness", "z_kurtosis", "n", "method"} and row["n"] == 9
    with pytest.raises(pkg.InvalidInputException, match="Data has zero variance") as failed:
        pkg.jarque_bera([3.0] * 5)
    assert failed.value.code == 1
    with pytest.raises(pkg.InvalidInputException, match="Data has zero variance"):
        pkg.dagostino_k2([3.0] * 9)
    assert pkg.shapiro_wilk([5.0] * 10)["statistic"] == 1.0
