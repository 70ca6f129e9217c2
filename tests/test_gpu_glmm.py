"""GPU tier of the mixed-model family (csrc/glmm.hip): every case of tests/glmm_cases.py through both entry forms against the dense
restatement, status isolation, the theta^ = 0 and upper-bracket rules, the properties, identical bytes, and the Python layer."""
import importlib

import numpy as np
import pytest

import glmm_cases as GC
import glmm_restate as R

pytestmark = pytest.mark.gpu

CALLS = GC.calls()


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("anofox-statistics_amd")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def opts(call, **kw):
    return dict(fit_intercept=call["fit_intercept"], reml=call["reml"], compute_inference=True, **kw)


def host_fit(ctx, call, **kw):
    return ctx.glmm_fit_batch_host(call["plo"], call["lro"], call["y"], call["x_cols"], opts(call, **kw))


def device_fit(ctx, call, **kw):
    import torch
    t = lambda a: torch.as_tensor(a).cuda()   # noqa: E731
    out = ctx.glmm_fit_batch_device(t(call["plo"]), t(call["lro"]), t(call["y"]), [t(c) for c in call["x_cols"]], opts(call, **kw))
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(CALLS))
def test_cases_against_the_restatement_and_bytes(ctx, name):
    call = CALLS[name]
    refs = GC.reference(name, call)
    host, dev = host_fit(ctx, call), device_fit(ctx, call)
    errs = {}
    n, left = GC.check(call, refs, *host, errs, GC.GPU_BOUNDS)
    print(name, "compared %d, left out %d" % (n, left), {k: "%.2e" % v for k, v in errs.items()})
    assert left == 0 and n == sum(isinstance(r, dict) for r in refs)
    assert same_bytes(host, dev), "the host form and the device form differ"
    assert same_bytes(host, host_fit(ctx, call)), "a call and its repeat differ"


def test_fixture_values(ctx):
    rec = host_fit(ctx, CALLS["fixtures-reml"])[0]
    e = GC.FIXTURES["sql_panel"]["expect"]
    assert round(rec[0, 1], 4) == e["intercept"] and round(rec[0, 0], 4) == e["slope"]
    assert rec[0, 10] == e["n_groups"] and rec[0, 9] == e["n_observations"] and rec[0, 4] > e["icc_above"]
    assert rec[1, 4] < GC.FIXTURES["flat_panel"]["expect"]["icc_below"]
    lo, hi = GC.FIXTURES["doubling"]["var_group_ratio"]
    assert lo <= rec[3, 2] / rec[0, 2] <= hi and abs(rec[3, 0] / rec[0, 0] - 2.0) < 1e-9 and abs(rec[3, 1] / rec[0, 1] - 2.0) < 1e-9


def test_a_panel_alone_and_inside_a_larger_call(ctx):
    """for every workgroup size: the level counts of the call cover 1, 4 and 16 wavefronts"""
    call = CALLS["level-counts"]
    whole = host_fit(ctx, call)
    for g in range(len(call["plo"]) - 1):
        l0, l1 = call["plo"][g], call["plo"][g + 1]
        r0, r1 = call["lro"][l0], call["lro"][l1]
        one = dict(call, plo=np.array([0, l1 - l0]), lro=call["lro"][l0:l1 + 1] - r0, y=call["y"][r0:r1], x_cols=[c[r0:r1] for c in call["x_cols"]])
        rec, inf, ranef, ln = host_fit(ctx, one)
        assert same_bytes((rec[0], inf[0], ranef, ln), (whole[0][g], whole[1][g], whole[2][l0:l1], whole[3][l0:l1])), g


def test_status_isolation(ctx):
    good = [GC.panel((5, 6, 7, 8), 2, s) for s in (1, 2, 3)]
    single = GC.panel((9,), 2, 4)
    singletons = GC.panel((1, 1, 1, 1, 1, 1), 2, 5)
    few = GC.panel((2, 2), 2, 6)
    none = GC.panel((3, 3), 2, 7)
    none[1][:] = np.nan
    call = GC.make_call([good[0], single, good[1], singletons, few, good[2], none])
    rec, inf, ranef, ln = host_fit(ctx, call)
    assert list(rec[:, 2 + 12]) == [0, 1, 0, 1, 6, 0, 10]
    for g in (1, 3, 4, 6):
        assert np.all(np.isnan(rec[g, :14])) and np.all(np.isnan(inf[g])) and np.all(np.isnan(ranef[call["plo"][g]:call["plo"][g + 1]]))
    alone = host_fit(ctx, GC.make_call(good))
    assert rec[[0, 2, 5]].tobytes() == alone[0].tobytes() and inf[[0, 2, 5]].tobytes() == alone[1].tobytes()
    empty = ctx.glmm_fit_batch_host(np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(0), [np.zeros(0)], None)
    assert empty[0].shape == (0, 14)
    bad = host_fit(ctx, GC.make_call(good), tolerance=0.0)
    assert np.all(bad[0][:, 14] == 1) and np.all(np.isnan(bad[2]))


def test_theta_zero_is_the_pooled_fit(ctx, pkg):
    rng = np.random.default_rng(3)
    sizes = np.full(6, 8)
    x = np.tile(np.arange(8.0), 6)
    e = np.tile(rng.normal(size=8), 6)   # every level has the same rows: the level means coincide
    call = GC.make_call([(sizes, 2.0 + 0.3 * x + e, x[:, None])])
    rec, inf, ranef, ln = host_fit(ctx, call)
    assert rec[0, 2] == 0.0 and rec[0, 4] == 0.0 and np.all(ranef == 0.0) and rec[0, 12] == 1 and rec[0, 13] == 0
    runtime = importlib.import_module("anofox-statistics_amd.runtime")
    core, _ = runtime.fit_batch_host(np.array([0, 48], np.int64), call["y"], call["x_cols"], None, pkg.RegressionOptions().batch_options("ols"), ctx)
    assert abs(rec[0, 0] - core[0, 0]) <= 1e-12 * abs(core[0, 0]) and abs(rec[0, 1] - core[0, 1]) <= 1e-12 * abs(core[0, 1])


def test_zero_residual_ends_on_the_upper_bracket(ctx):
    sizes = np.full(5, 4)
    x = np.tile(np.arange(4.0), 5)
    b = np.repeat([-2.0, -1.0, 0.5, 1.0, 3.0], 4)
    call = GC.make_call([(sizes, 1.0 + 0.5 * x + b, x[:, None])])
    rec = host_fit(ctx, call)[0]
    assert rec[0, 13] == 0 and rec[0, 12] == 0 and abs(rec[0, 2] / rec[0, 3] / R.THETA_HI - 1.0) <= 1e-12, rec


def test_blups_shrink_and_levels_permute(ctx):
    sizes, y, X = GC.fixture_panel("shrink_panel")
    call = GC.make_call([(sizes, y, X)])
    rec, inf, ranef, ln = host_fit(ctx, call)
    means = np.array([y[6 * j:6 * j + 6].mean() for j in range(15)])
    assert np.all(np.abs(ranef) <= np.abs(means - y.mean()) + 1e-9)
    ref = GC.reference("shrink", call)[0]
    curv = max(ref["curvature"], 1.0)
    moved = {k: 0.0 for k in GC.PERMUTE_BOUNDS}
    for seed in range(5):
        perm = np.random.default_rng(seed).permutation(15)
        rows = np.concatenate([np.arange(6 * j, 6 * j + 6) for j in perm])
        rec2, inf2, ranef2, _ = host_fit(ctx, GC.make_call([(sizes, y[rows], X[rows])]))
        m = {"beta": np.max(np.abs(rec2[0, :2] - rec[0, :2])) / np.max(np.abs(rec[0, :2])) / ref["cond"],
             "var_group": abs(rec2[0, 2] / rec[0, 2] - 1.0) * curv, "var_residual": abs(rec2[0, 3] / rec[0, 3] - 1.0) * curv,
             "blup": np.max(np.abs(ranef2 - ranef[perm])) / np.max(np.abs(ranef)) * curv}
        moved = {k: max(moved[k], float(v)) for k, v in m.items()}
    print("permuted levels, largest movement:", {k: "%.2e" % v for k, v in moved.items()})
    for k, v in moved.items():
        assert v <= GC.PERMUTE_BOUNDS[k], "%s moves by %.3e, above %.1e" % (k, v, GC.PERMUTE_BOUNDS[k])
    # l at the returned theta^, recomputed densely, is not below the restatement's maximum
    d = R.Dense(y, np.column_stack([np.ones(len(y)), X]), np.repeat(np.arange(15), 6), True)
    assert d.ell_score(rec[0, 2] / rec[0, 3])[0] >= ref["ell"] - GC.GPU_BOUNDS["ell"] * abs(ref["ell"])


def test_python_layer(pkg):
    sizes, y, X = GC.fixture_panel("sql_panel")
    labels = np.array(["sku_%d" % g for g in GC.FIXTURES["sql_panel"]["group"]], dtype=object)
    perm = np.random.default_rng(5).permutation(len(y))
    res = pkg.glmm_fit_agg(None, y[perm], [X[perm, 0]], labels[perm], {"compute_inference": True})
    row = res.row(0)
    assert round(row["intercept"], 4) == 1.0052 and round(row["coefficients"][0], 4) == 0.4974 and row["n_groups"] == 20
    seen = list(dict.fromkeys(labels[perm]))
    assert [r["group"] for r in row["ranef"]] == seen and all(r["n"] == 15 and np.isnan(r["se"]) for r in row["ranef"])
    scalar = pkg.glmm_fit(list(y[perm]), [list(X[perm, 0])], list(labels[perm]), {"compute_inference": True})
    assert scalar["intercept"] == row["intercept"] and scalar["var_group"] == row["var_group"]
    assert [r["group"] for r in scalar["ranef"]] == seen and [r["intercept"] for r in scalar["ranef"]] == [r["intercept"] for r in row["ranef"]]
    keys = np.where(np.arange(len(y)) < 150, "b", "a")
    two = pkg.glmm_fit_agg(keys[perm], y[perm], [X[perm, 0]], list(labels[perm[:-1]]) + [None])
    assert two.keys == ["a", "b"] and two.row(0)["n_groups"] == 10 and two.row(0)["n_observations"] + two.row(1)["n_observations"] == 299
    with pytest.raises(ValueError, match="is not built"):
        pkg.glmm_fit_agg(None, y, [X[:, 0]], labels, {"family": "poisson"})
    with pytest.raises(ValueError, match="Unknown GLMM family"):
        pkg.glmm_fit_agg(None, y, [X[:, 0]], labels, {"family": "cauchy"})
