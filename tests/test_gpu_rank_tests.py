"""GPU tier of the rank tests: anofox_hip_rank_test_batch_{host,device} on the shapes of tests/rank_test_restate.py (groups of 0, 1,
2, 3, 4, 63, 64, 65, 129 and 300 valid rows in one call, for every content of every test), with the cap hooked to 128 (129 and 300
on the large path) and at the default cap (both on the small path), against the restatement; the two paths against each other;
one group above the true cap; the last row of each size tier and the first of the next in one call; the test hooks of this family
and of the correlation family, each leaving the other's cap alone; the scalars and the aggregates on the tables of the reference's
SQL tests."""
import numpy as np
import pytest

import cor_restate
import rank_test_restate as R
from conftest import import_pkg

pytestmark = pytest.mark.gpu


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
    p.rank_test_hooks(0)


def _columns(test, call):
    return (call["v"], call["y"], None) if test == R.WILCOXON else (call["v"], None, call["sample"])


def _exact_columns(test):
    return [4, 5, 6, 7] if test == R.KRUSKAL_WALLIS else [0, 4, 5, 6, 7]   # counts and status; W and V


@pytest.mark.parametrize("name, content", R.CASES)
def test_both_paths_against_the_restatement_and_each_other(pkg, calls, name, content):
    import torch
    test = R.TESTS[name]
    call, ref = calls[name, content]
    v, y, s = _columns(test, call)
    opts = {"mu": call["mu"]}
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()   # noqa: E731
    ctx = pkg.Context(0)
    got = {}
    for cap in (128, 0):
        pkg.rank_test_hooks(cap)
        host = pkg.rank_test_batch_host(call["off"], v, y, s, test, opts, ctx=ctx)
        rec = ctx.rank_test_batch_device(dev(call["off"]), dev(v), dev(y), dev(s), test, opts)
        torch.cuda.synchronize()
        assert rec.cpu().numpy().tobytes() == host.tobytes()        # host and device entries: the same bytes
        errs = R.check_records(test, host, ref)
        print(name, content, "cap", cap or "default", {k: "%.2e" % e for k, e in errs.items()})
        got[cap] = host
    ctx.close()
    cols = _exact_columns(test)
    assert got[128][:, cols].tobytes() == got[0][:, cols].tobytes()


@pytest.mark.parametrize("kw", [dict(alternative="less"), dict(alternative="greater", correction=False), dict(continuity_correction=False)])
def test_options_on_the_large_path(pkg, kw):
    o = pkg.parse_rank_test_options(kw)
    pkg.rank_test_hooks(128)
    for test in (R.MANN_WHITNEY, R.WILCOXON):
        call = R.make_call(test, "shift", seed=1)
        v, y, s = _columns(test, call)
        ref = R.reference(test, call, alternative=o.alternative, correction=o.continuity_correction)
        R.check_records(test, pkg.rank_test_batch_host(call["off"], v, y, s, test, dict(kw, mu=call["mu"])), ref)


def test_several_large_groups_in_one_call(pkg):
    """Five groups above the hooked cap and one below it in one call."""
    rng = np.random.default_rng(7)
    sizes = [130, 257, 40, 700, 129, 300]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    call = dict(off=off, v=rng.integers(0, 40, off[-1]).astype(np.float64), y=rng.integers(0, 40, off[-1]).astype(np.float64),
                sample=rng.choice(np.array([0, 9, -4, 100000], np.int32), off[-1]), mu=0.0)
    for test in R.TESTS.values():
        v, y, s = _columns(test, call)
        pkg.rank_test_hooks(128)
        large = pkg.rank_test_batch_host(off, v, y, s, test)
        R.check_records(test, large, R.reference(test, call))
        pkg.rank_test_hooks(0)
        cols = _exact_columns(test)
        assert pkg.rank_test_batch_host(off, v, y, s, test)[:, cols].tobytes() == large[:, cols].tobytes()


def test_one_group_above_the_true_cap(pkg):
    rng = np.random.default_rng(11)
    n = 1463
    call = dict(off=np.array([0, n], np.int64), v=np.round(rng.standard_normal(n), 1), y=np.round(rng.standard_normal(n), 1),
                sample=rng.choice(np.array([0, 5, -1], np.int32), n), mu=0.0)
    for test in R.TESTS.values():
        v, y, s = _columns(test, call)
        R.check_records(test, pkg.rank_test_batch_host(call["off"], v, y, s, test), R.reference(test, call))


def boundary_call():
    """Groups of 256, 257, 1462 and 1463 rows of rounded normals: at the default cap both small instances and the large path."""
    rng = np.random.default_rng(17)
    off = np.concatenate([[0], np.cumsum([256, 257, 1462, 1463])]).astype(np.int64)
    n = off[-1]
    return dict(off=off, v=np.round(rng.standard_normal(n), 1), y=np.round(rng.standard_normal(n), 1),
                sample=rng.choice(np.array([0, 5, -1], np.int32), n), mu=0.0)


def test_tier_boundaries_at_the_default_cap(pkg):
    call = boundary_call()
    for test in R.TESTS.values():
        v, y, s = _columns(test, call)
        R.check_records(test, pkg.rank_test_batch_host(call["off"], v, y, s, test), R.reference(test, call))


def test_each_family_has_its_own_hook(pkg):
    """A Mann-Whitney and a Spearman call of one 300-row group each, with one family's cap hooked to 128 and the other's not, both
    ways round: within bounds of the restatement, and the exact columns as with neither hooked."""
    rng = np.random.default_rng(19)
    n = 300
    call = dict(off=np.array([0, n], np.int64), v=np.round(rng.standard_normal(n), 1), y=np.round(rng.standard_normal(n), 1),
                sample=rng.choice(np.array([0, 1], np.int32), n), mu=0.0)
    refs = R.reference(R.MANN_WHITNEY, call), cor_restate.reference(call["off"], call["v"], call["y"], cor_restate.SPEARMAN)

    def both(cor_cap, rank_cap):
        pkg.cor_test_hooks(cor_cap)
        pkg.rank_test_hooks(rank_cap)
        return (pkg.rank_test_batch_host(call["off"], call["v"], None, call["sample"], R.MANN_WHITNEY),
                pkg.cor_batch_host(call["off"], call["v"], call["y"], cor_restate.SPEARMAN))
    try:
        plain = both(0, 0)
        for caps in ((128, 0), (0, 128)):
            mw, rho = both(*caps)
            R.check_records(R.MANN_WHITNEY, mw, refs[0])
            cor_restate.check_records(rho, refs[1])
            cols = _exact_columns(R.MANN_WHITNEY)
            assert mw[:, cols].tobytes() == plain[0][:, cols].tobytes()
            assert rho[:, [0, 5, 6, 7]].tobytes() == plain[1][:, [0, 5, 6, 7]].tobytes()
    finally:
        pkg.cor_test_hooks(0)
        pkg.rank_test_hooks(0)


def test_empty_call_and_empty_groups(pkg):
    none, ids = np.zeros(0), np.zeros(0, np.int32)
    assert pkg.rank_test_batch_host(np.zeros(1, np.int64), none, None, ids, R.KRUSKAL_WALLIS).shape == (0, 8)
    for test in R.TESTS.values():
        rec = pkg.rank_test_batch_host(np.array([0, 0, 0], np.int64), none, none, ids, test)
        assert np.all(rec[:, 7] == 6) and np.all(rec[:, 4] == 0) and np.all(np.isnan(rec[:, :4]))


def test_scalars_and_aggregates_reproduce_the_sql_tables(pkg):
    text = {R.MANN_WHITNEY: "Mann-Whitney U test", R.WILCOXON: "Wilcoxon signed-rank test", R.KRUSKAL_WALLIS: "Kruskal-Wallis H test"}
    alt = {R.TWO_SIDED: "two_sided", R.LESS: "less", R.GREATER: "greater"}

    def by_scalar(test, table, alternative=R.TWO_SIDED, correction=True):
        a, b = R.TABLES[test][table]
        opts = {"alternative": alt[alternative], "continuity_correction": correction}
        try:
            if test == R.MANN_WHITNEY:
                a, b = np.array(a), np.array(b)
                d = pkg.mann_whitney_u(a[b == 0], a[b != 0], opts)
            elif test == R.WILCOXON:
                d = pkg.wilcoxon_signed_rank(a, b, opts)
            else:
                d = pkg.kruskal_wallis(a, [float(t) for t in b])
        except pkg.InvalidInputException as e:
            assert "requires at least" in str(e)
            return None
        assert d["method"] == text[test] and np.isnan(d["ci_lower"]) and np.isnan(d["ci_upper"]) and np.isnan(d["effect_size"])
        return d
    R.check_known_answers(by_scalar)

    def by_agg(test, table, alternative=R.TWO_SIDED, correction=True):
        names = list(R.TABLES[test])
        keys = np.concatenate([[t] * len(R.TABLES[test][t][0]) for t in names])
        a = np.concatenate([R.TABLES[test][t][0] for t in names])
        b = np.concatenate([R.TABLES[test][t][1] for t in names])
        opts = {"alternative": alt[alternative], "correction": correction}
        if test == R.MANN_WHITNEY:
            res = pkg.mann_whitney_u_agg(keys, a, b.astype(np.int32), opts)
        elif test == R.WILCOXON:
            res = pkg.wilcoxon_signed_rank_agg(keys, a, b, opts)
        else:
            res = pkg.kruskal_wallis_agg(keys, a, b.astype(np.int32))
        d = res.by_key()[table]
        assert d is None or d["method"] == text[test]
        return d
    R.check_known_answers(by_agg)
    # a None is a NULL: the row is not valid; a key with one sample only is NULL
    res = pkg.mann_whitney_u_agg(["a"] * 4 + ["b"] * 5, [1.0, 2.0, 3.0, 4.0, 1.0, None, 3.0, 4.0, 9.0], [0, 0, 0, None, 0, 1, 1, None, 0],
                                 {"correction": False})
    assert res.row(0) is None and res.row(1)["n1"] == 2 and res.row(1)["n2"] == 1 and res.row(1)["statistic"] == 1.0
    assert pkg.wilcoxon_signed_rank([2.0, 1.0, 5.0, 4.0, None], [1.0, 3.0, 2.0, 4.0, 1.0])["statistic"] == 4.0
    assert pkg.kruskal_wallis([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [7.0, 7.0, -1.0, -1.0, 9.5, 9.0])["df"] == 2.0
