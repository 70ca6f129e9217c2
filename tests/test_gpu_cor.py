"""GPU tier of the correlation family: anofox_hip_cor_batch_{host,device} on the shapes of tests/cor_restate.py (groups of 0, 2, 3,
4, 63, 64, 65, 129 and 300 valid rows in one call; noise, scattered NaN rows, a constant x, heavy ties, an exact monotone group),
with the cap hooked to 128 (129 and 300 on the large path) and at the default cap (both on the small path), against the
restatement; the two paths against each other; the last row of each size tier and the first of the next in one call; the scalars
and the aggregates on the tables of the reference's SQL tests."""
import numpy as np
import pytest

import cor_restate as R
from conftest import import_pkg

pytestmark = pytest.mark.gpu
METHODS = {"pearson": R.PEARSON, "spearman": R.SPEARMAN, "kendall": R.KENDALL}


@pytest.fixture(scope="module")
def calls():
    """content -> (offsets, x, y, {method: reference records}); computed once, read by every test."""
    out = {}
    for content in R.CONTENTS:
        off, x, y = R.make_call(content)
        out[content] = (off, x, y, {m: R.reference(off, x, y, m) for m in METHODS.values()})
    return out


@pytest.fixture()
def pkg():
    p = import_pkg()
    yield p
    p.cor_test_hooks(0)


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("method", list(METHODS))
def test_both_paths_against_the_restatement_and_each_other(pkg, calls, method, content):
    import torch
    off, x, y, refs = calls[content]
    m = METHODS[method]
    ctx = pkg.Context(0)
    got = {}
    for cap in (128, 0):
        pkg.cor_test_hooks(cap)
        host = pkg.cor_batch_host(off, x, y, m, ctx=ctx)
        dev = ctx.cor_batch_device(torch.from_numpy(off).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), m)
        torch.cuda.synchronize()
        assert dev.cpu().numpy().tobytes() == host.tobytes()        # host and device entries: the same bytes
        errs = R.check_records(host, refs[m])
        print(method, content, "cap", cap or "default", {k: "%.2e" % v for k, v in errs.items()})
        got[cap] = host
    ctx.close()
    # the two paths: n, s, status and the estimate (the midrank-based rho) bit for bit
    assert got[128][:, [0, 5, 6, 7]].tobytes() == got[0][:, [0, 5, 6, 7]].tobytes()


@pytest.mark.parametrize("kw", [dict(alternative="less"), dict(alternative="greater", tau_type="a"), dict(variant="c", confidence_level=0.99)])
def test_options_on_the_large_path(pkg, calls, kw):
    off, x, y, _ = calls["ties"]
    o = pkg.parse_correlation_options(kw)
    pkg.cor_test_hooks(128)
    for m in METHODS.values():
        ref = R.reference(off, x, y, m, alternative=o.alternative, tau_type=o.tau_type, confidence_level=o.confidence_level)
        R.check_records(pkg.cor_batch_host(off, x, y, m, kw), ref)


def test_several_large_groups_share_the_pair_kernel(pkg):
    """Five groups above the hooked cap in one call, none a multiple of the pair tile, one of them larger than two tiles."""
    rng = np.random.default_rng(7)
    sizes = [130, 257, 40, 700, 129, 300]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x = rng.integers(0, 40, off[-1]).astype(np.float64)
    y = x + rng.integers(-15, 15, off[-1])
    pkg.cor_test_hooks(128)
    for m in (R.SPEARMAN, R.KENDALL):
        large = pkg.cor_batch_host(off, x, y, m)
        R.check_records(large, R.reference(off, x, y, m))
        pkg.cor_test_hooks(0)
        assert pkg.cor_batch_host(off, x, y, m)[:, [0, 5, 6, 7]].tobytes() == large[:, [0, 5, 6, 7]].tobytes()
        pkg.cor_test_hooks(128)


def boundary_call():
    """Groups of 256, 257, 1462 and 1463 rows of rounded normals: at the default cap both small instances and the large path."""
    rng = np.random.default_rng(17)
    off = np.concatenate([[0], np.cumsum([256, 257, 1462, 1463])]).astype(np.int64)
    return off, np.round(rng.standard_normal(off[-1]), 1), np.round(rng.standard_normal(off[-1]), 1)


def test_tier_boundaries_at_the_default_cap(pkg):
    off, x, y = boundary_call()
    for m in METHODS.values():
        R.check_records(pkg.cor_batch_host(off, x, y, m), R.reference(off, x, y, m))


def test_empty_call_and_empty_groups(pkg):
    rec = pkg.cor_batch_host(np.zeros(1, np.int64), np.zeros(0), np.zeros(0), R.KENDALL)
    assert rec.shape == (0, 8)
    rec = pkg.cor_batch_host(np.array([0, 0, 0], np.int64), np.zeros(0), np.zeros(0), R.SPEARMAN)
    assert np.all(rec[:, 7] == 6) and np.all(rec[:, 5] == 0) and np.all(np.isnan(rec[:, :5]))


def test_scalars_and_aggregates_reproduce_the_sql_tables(pkg):
    scalar = {R.PEARSON: pkg.pearson, R.SPEARMAN: pkg.spearman, R.KENDALL: pkg.kendall}
    agg = {R.PEARSON: pkg.pearson_agg, R.SPEARMAN: pkg.spearman_agg, R.KENDALL: pkg.kendall_agg}
    text = {R.PEARSON: "Pearson correlation", R.SPEARMAN: "Spearman rank correlation", R.KENDALL: "Kendall's TauB"}

    def by_scalar(table, m):
        d = scalar[m](*R.TABLES[table])
        assert d["method"] == text[m]
        return d["tau" if m == R.KENDALL else "r"], d["p_value"], d["n"]
    R.check_known_answers(by_scalar)

    names = list(R.TABLES)
    keys = np.concatenate([[t] * len(R.TABLES[t][0]) for t in names])
    x = np.concatenate([R.TABLES[t][0] for t in names])
    y = np.concatenate([R.TABLES[t][1] for t in names])
    rows = {m: agg[m](keys, x, y).by_key() for m in agg}

    def by_agg(table, m):
        d = rows[m][table]
        assert d["method"] == text[m]
        return d["tau" if m == R.KENDALL else "r"], d["p_value"], d["n"]
    R.check_known_answers(by_agg)
    # a group with fewer than 3 valid pairs is NULL; None is a NULL
    res = pkg.kendall_agg(["a", "a", "a", "b", "b", "b", "b"], [1.0, None, 3.0, 1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0, 3.0, 2.0, 1.0],
                          {"tau_type": "a"})
    assert res.row(0) is None and res.row(1)["tau"] == -1.0 and res.row(1)["method"] == "Kendall's TauA" and res.row(1)["n"] == 4
    assert pkg.kendall([1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 2.0, 5.0], {"tau_type": "b"})["tau"] == pytest.approx(5.0 / np.sqrt(30.0), abs=1e-15)
    with pytest.raises(pkg.InvalidInputException, match="at least 3 valid pairs"):
        pkg.pearson([1.0, 2.0], [2.0, 1.0])
