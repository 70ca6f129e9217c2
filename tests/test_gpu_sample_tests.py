"""GPU tier of the sample tests: anofox_hip_sample_test_batch_{host,device} on the shapes of tests/sample_test_restate.py (groups of
0, 1, 2, 3, 4, 63, 64, 65, 129 and 300 valid rows in one call, for every content of every test), with the cap hooked to 128 (129
and 300 on the large path) and at the default cap (both on the small path), against the restatement; the two paths against each
other; the options on the large path; several large groups in one call; one group above the true cap; the last row of each size
tier and the first of the next in one call; the three families' test hooks, each leaving the other two caps alone; the identities
between the tests; a second sub-view that starts on and off a wavefront boundary; the scalars and the aggregates on the tables of
the reference's SQL tests."""
import os

import numpy as np
import pytest

import cor_restate
import rank_test_restate
import sample_test_restate as R
from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu
_BITWISE = [7, 8, 9, 11]      # the counts and the status


@pytest.fixture(scope="module")
def calls():
    """(test, content) -> (call, reference records); computed once, read by every test."""
    out = {}
    for name, content in R.CASES:
        call = R.make_call(R.TESTS[name], content)
        out[name, content] = (call, R.reference(R.TESTS[name], call))
    return out


@pytest.fixture()
def pkg():
    p = import_pkg()
    yield p
    p.sample_test_hooks(0)


def _exact_columns(test):
    return _BITWISE + [4] if test == R.BRUNNER_MUNZEL else _BITWISE       # Brunner-Munzel's estimate: sums of multiples of 1/2


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@pytest.mark.parametrize("name, content", R.CASES)
def test_both_paths_against_the_restatement_and_each_other(pkg, calls, name, content):
    import torch
    test = R.TESTS[name]
    call, ref = calls[name, content]
    opts = call["opts"]
    v, y, s = (call["v"], call["y"], None) if opts.get("kind") == R.PAIRED else (call["v"], None, call["sample"])
    o = pkg.SampleTestOptions(kind=opts.get("kind", 0), mu=opts.get("mu", 0.0), trim=opts.get("trim", 0.2))
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()   # noqa: E731
    ctx = pkg.Context(0)
    got = {}
    for cap in (128, 0):
        pkg.sample_test_hooks(cap)
        host = pkg.sample_test_batch_host(call["off"], v, y, s, test, o, ctx=ctx)
        rec = ctx.sample_test_batch_device(dev(call["off"]), dev(v), dev(y), dev(s), test, o)
        torch.cuda.synchronize()
        assert rec.cpu().numpy().tobytes() == host.tobytes()        # host and device entries: the same bytes
        errs = R.check_records(test, host, ref, o.kind)
        print(name, content, "cap", cap or "default", {k: "%.2e" % e for k, e in errs.items()})
        got[cap] = host
    ctx.close()
    cols = _exact_columns(test)
    assert got[128][:, cols].tobytes() == got[0][:, cols].tobytes()


@pytest.mark.parametrize("name, kw", [("t_test", dict(alternative=R.LESS)), ("t_test", dict(alternative=R.GREATER)), ("t_test", dict(kind=R.STUDENT)),
                                      ("yuen", dict(alternative=R.LESS, trim=0.1)), ("yuen", dict(alternative=R.GREATER)), ("yuen", dict(trim=0.1)),
                                      ("brunner_munzel", dict(alternative=R.LESS)), ("brunner_munzel", dict(alternative=R.GREATER)),
                                      ("anova", dict(kind=R.WELCH_ANOVA))])
def test_options_on_the_large_path(pkg, name, kw):
    test = R.TESTS[name]
    o = pkg.SampleTestOptions(**kw)
    pkg.sample_test_hooks(128)
    for content in ("noise", "ties"):
        call = R.make_call(test, content, seed=1)
        ref = R.reference(test, call, **kw)
        R.check_records(test, pkg.sample_test_batch_host(call["off"], call["v"], None, call["sample"], test, o), ref, o.kind)


def _random_call(seed, sizes, ids=(0, 9, -4, 100000), rounded=False):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = off[-1]
    v = np.round(rng.standard_normal(n), 1) if rounded else rng.integers(0, 40, n).astype(np.float64)
    y = np.round(rng.standard_normal(n), 1) if rounded else rng.integers(0, 40, n).astype(np.float64)
    return dict(off=off, v=v, y=y, sample=rng.choice(np.array(ids, np.int32), n), opts={})


def _every_test(pkg, call, cap):
    """-> {test: records} of the call at the cap, each held to the restatement (the t-test as Welch and as paired)."""
    out = {}
    pkg.sample_test_hooks(cap)
    for test in R.TESTS.values():
        out[test] = pkg.sample_test_batch_host(call["off"], call["v"], None, call["sample"], test)
        R.check_records(test, out[test], R.reference(test, call))
    out["paired"] = pkg.sample_test_batch_host(call["off"], call["v"], call["y"], None, R.T_TEST, {"kind": "paired"})
    R.check_records(R.T_TEST, out["paired"], R.reference(R.T_TEST, call, kind=R.PAIRED), R.PAIRED)
    return out


def test_several_large_groups_in_one_call(pkg):
    """Five groups above the hooked cap and one below it in one call."""
    call = _random_call(7, [130, 257, 40, 700, 129, 300])
    large, small = _every_test(pkg, call, 128), _every_test(pkg, call, 0)
    for test in R.TESTS.values():
        cols = _exact_columns(test)
        assert small[test][:, cols].tobytes() == large[test][:, cols].tobytes()


def test_one_group_above_the_true_cap(pkg):
    _every_test(pkg, _random_call(11, [1463], ids=(0, 5, -1), rounded=True), 0)


def test_tier_boundaries_at_the_default_cap(pkg):
    """Groups of 256, 257, 1462 and 1463 rows: at the default cap both small instances and the large path."""
    _every_test(pkg, _random_call(17, [256, 257, 1462, 1463], ids=(0, 5, -1), rounded=True), 0)


def test_each_family_has_its_own_hook(pkg):
    """A Brunner-Munzel, a Mann-Whitney and a Spearman call of one 300-row group each, with one family's cap hooked to 128 and the
    other two not, every way round: within bounds of the restatements, and the exact columns as with none hooked."""
    call = _random_call(19, [300], ids=(0, 1), rounded=True)
    call["mu"] = 0.0
    refs = (R.reference(R.BRUNNER_MUNZEL, call), rank_test_restate.reference(rank_test_restate.MANN_WHITNEY, call),
            cor_restate.reference(call["off"], call["v"], call["y"], cor_restate.SPEARMAN))

    def all_three(sample_cap, rank_cap, cor_cap):
        pkg.sample_test_hooks(sample_cap)
        pkg.rank_test_hooks(rank_cap)
        pkg.cor_test_hooks(cor_cap)
        return (pkg.sample_test_batch_host(call["off"], call["v"], None, call["sample"], R.BRUNNER_MUNZEL),
                pkg.rank_test_batch_host(call["off"], call["v"], None, call["sample"], rank_test_restate.MANN_WHITNEY),
                pkg.cor_batch_host(call["off"], call["v"], call["y"], cor_restate.SPEARMAN))
    try:
        plain = all_three(0, 0, 0)
        for caps in ((128, 0, 0), (0, 128, 0), (0, 0, 128)):
            bm, mw, rho = all_three(*caps)
            R.check_records(R.BRUNNER_MUNZEL, bm, refs[0])
            rank_test_restate.check_records(rank_test_restate.MANN_WHITNEY, mw, refs[1])
            cor_restate.check_records(rho, refs[2])
            cols = _exact_columns(R.BRUNNER_MUNZEL)
            assert bm[:, cols].tobytes() == plain[0][:, cols].tobytes()
            assert mw[:, [0, 4, 5, 6, 7]].tobytes() == plain[1][:, [0, 4, 5, 6, 7]].tobytes()
            assert rho[:, [0, 5, 6, 7]].tobytes() == plain[2][:, [0, 5, 6, 7]].tobytes()
    finally:
        pkg.cor_test_hooks(0)
        pkg.rank_test_hooks(0)
        pkg.sample_test_hooks(0)


def test_identities_between_the_tests(pkg):
    """Yuen at trim = 0 against the Welch t-test of the same call, and two-arm Fisher ANOVA against the Student t squared, within
    1e-12 relative, on both size paths."""
    call = R.make_call(R.T_TEST, "noise", seed=3)
    two = np.where(call["sample"] == 0, 0, 1).astype(np.int32)       # ANOVA's arms are the ids: two of them
    for cap in (128, 0):
        pkg.sample_test_hooks(cap)
        run = lambda test, o=None, s=call["sample"]: pkg.sample_test_batch_host(call["off"], call["v"], None, s, test, o)   # noqa: E731
        welch, student = run(R.T_TEST), run(R.T_TEST, {"kind": "student"})
        yuen, fisher = run(R.YUEN, {"trim": 0.0}), run(R.ANOVA, None, two)
        seen = 0
        for g in range(len(welch)):
            if yuen[g, 11] == 0:
                seen += 1
                for j in (0, 1, 2, 4, 5, 6):
                    assert _rel(yuen[g, j], welch[g, j]) <= 1e-12, (g, j)
            if fisher[g, 11] == 0:
                assert _rel(fisher[g, 0], student[g, 0] ** 2) <= 1e-12, g
        assert seen >= 5


@pytest.mark.parametrize("n1", [64, 65])
def test_second_sub_view_on_and_off_a_wavefront_boundary(pkg, n1):
    rng = np.random.default_rng(n1)
    n = n1 + 71
    s = np.ones(n, np.int32)
    s[rng.permutation(n)[:n1]] = 0
    call = dict(off=np.array([0, n], np.int64), v=np.round(rng.standard_normal(n), 1), y=np.zeros(n), sample=s, opts={})
    for test in (R.YUEN, R.BRUNNER_MUNZEL):
        ref = R.reference(test, call)
        assert ref[0, 8] == n1
        for cap in (0, 100):
            pkg.sample_test_hooks(cap)
            R.check_records(test, pkg.sample_test_batch_host(call["off"], call["v"], None, s, test), ref)


def test_interval_ends_over_many_degrees_of_freedom(pkg):
    """Regression (found by tests/test_gpu_fuzz_stat_tests.py): the t quantile returned the middle of its bracket, up to 1e-8
    relative off, where the Newton step at the root rounded to 0; it happened at about one df in 120.  600 Welch groups of 6 to 40
    rows at three levels: 1800 quantiles at as many real-valued df, every interval end within the bounds."""
    rng = np.random.default_rng(41)
    call = _random_call(41, rng.integers(6, 41, 600), ids=(0, 0, 1, -3), rounded=True)
    for level in (0.9, 0.95, 0.99):
        got = pkg.sample_test_batch_host(call["off"], call["v"], None, call["sample"], R.T_TEST, pkg.SampleTestOptions(confidence_level=level))
        ref = R.reference(R.T_TEST, call, confidence_level=level)
        assert np.sum(ref[:, 11] == 0) >= 550
        R.check_records(R.T_TEST, got, ref)


def test_empty_call_and_empty_groups(pkg):
    none, ids = np.zeros(0), np.zeros(0, np.int32)
    assert pkg.sample_test_batch_host(np.zeros(1, np.int64), none, None, ids, R.ANOVA).shape == (0, 12)
    for test in R.TESTS.values():
        rec = pkg.sample_test_batch_host(np.array([0, 0, 0], np.int64), none, None, ids, test)
        assert np.all(rec[:, 11] == 6) and np.all(rec[:, 7] == 0) and np.all(np.isnan(rec[:, :7]))
    rec = pkg.sample_test_batch_host(np.array([0, 0], np.int64), none, none, None, R.T_TEST, {"kind": "paired"})
    assert rec[0, 11] == 6 and rec[0, 7] == 0


def test_scalars_and_aggregates_reproduce_the_sql_tables(pkg):
    tables = R.load_tables(os.path.join(ROOT, "tests", "golden", "sample_tests"))
    text = {"t_test": "Welch t-test", "yuen": "Yuen test (trim=%.2f)", "anova": "Fisher One-way ANOVA", "brown_forsythe": "Brown-Forsythe test",
            "brunner_munzel": "Brunner-Munzel test"}

    def by_scalar(name, _, v, s, **opts):
        v, s = np.array(v), np.array(s)
        try:
            if name in ("anova", "brown_forsythe"):
                d = (pkg.one_way_anova if name == "anova" else pkg.brown_forsythe)(v, s.astype(np.float64))
            else:
                d = {"t_test": pkg.t_test, "yuen": pkg.yuen, "brunner_munzel": pkg.brunner_munzel}[name](v[s == 0], v[s != 0], opts)
        except pkg.InvalidInputException as e:
            assert "requires at least" in str(e)
            return None
        assert d["method"] == (text[name] % opts.get("trim", 0.2) if name == "yuen" else text[name])
        if name == "anova":
            return dict(statistic=d["f_statistic"], p_value=d["p_value"], df=d["df_between"], df2=d["df_within"], estimate=d["ss_between"],
                        aux=d["ss_within"], n1=d["n_groups"], n=d["n"])
        assert np.isnan(d["effect_size"]) == (name != "brunner_munzel")
        return dict(d, estimate=d["effect_size"])
    R.check_known_answers(tables, by_scalar)

    def by_agg(name, table, v, s, **opts):
        names = list(tables[name])
        keys = np.concatenate([[t] * len(tables[name][t][0]) for t in names])
        a = np.concatenate([tables[name][t][0] for t in names])
        b = np.concatenate([tables[name][t][1] for t in names]).astype(np.int32)
        agg = {"t_test": pkg.t_test_agg, "yuen": pkg.yuen_agg, "anova": pkg.one_way_anova_agg, "brunner_munzel": pkg.brunner_munzel_agg}
        res = pkg.brown_forsythe_agg(keys, a, b) if name == "brown_forsythe" else agg[name](keys, a, b, opts)
        d = res.by_key()[table]
        if d is None:
            return None
        assert d["method"] == (text[name] % opts.get("trim", 0.2) if name == "yuen" else text[name])
        if name == "anova":
            return dict(statistic=d["f_statistic"], p_value=d["p_value"], df=d["df_between"], df2=d["df_within"], estimate=d["ss_between"],
                        aux=d["ss_within"], n1=d["n_groups"], n=d["n"])
        return dict(d, estimate=d.get("effect_size"))
    R.check_known_answers(tables, by_agg)
    # a None is a NULL: the row is not valid; a key with one arm only is NULL
    res = pkg.t_test_agg(["a"] * 4 + ["b"] * 6, [1.0, 2.0, 3.0, 4.0, 1.0, None, 3.0, 4.0, 9.0, 5.0], [0, 0, 0, None, 0, 1, 1, None, 0, 1],
                         {"kind": "student"})
    assert res.row(0) is None and res.row(1)["n1"] == 2 and res.row(1)["n2"] == 2 and res.row(1)["method"] == "Student t-test"
    d = pkg.paired_t_test([1.0, 2.0, 3.0, 9.0], [2.0, 4.0, 6.0, None])
    assert d["n"] == 3 and d["estimate"] == -2.0 and abs(d["statistic"] + 2.0 / np.sqrt(1.0 / 3.0)) < 1e-14 and d["method"] == "Paired t-test"
    res = pkg.paired_t_test_agg(["a"] * 4 + ["b"], [1.0, 2.0, 3.0, 9.0, 1.0], [2.0, 4.0, 6.0, None, 0.0])
    assert res.row(1) is None and abs(res.row(0)["statistic"] - d["statistic"]) < 1e-14
    assert pkg.one_way_anova_agg(["a"] * 6, [1.0, 2.0, 3.0, 2.0, 4.0, 6.0], [7, 7, 7, -1, -1, -1], {"kind": "welch"}).row(0)["method"] == "Welch One-way ANOVA"
