"""GPU tier of the categorical tests: anofox_hip_categorical_test_batch_{host,device} on the shapes of
tests/categorical_test_restate.py (groups of 0, 1, 3, 4, 63, 64, 65, 255, 256, 257, 1462 and 1463 valid rows in one call, for every
content), at the default cap (the 1463-row group alone on the large path; with scattered NULL rows the 1462-row group too) and with
the cap hooked to 128 (255 to 1462 rows on the large path as well): the two calls byte-equal, both within check_records' bounds of
the restatement.  Fisher's and McNemar's tables, the device entry, and the aggregates and scalars on the reference's SQL tables."""
import os

import numpy as np
import pytest

import categorical_test_restate as R
from conftest import ROOT, import_pkg
from test_categorical_test_restate_cpu import restated_aggregate

pytestmark = pytest.mark.gpu


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
    try:
        yield p
    finally:
        p.categorical_test_hooks(0)


@pytest.mark.parametrize("content", R.CONTENTS)
@pytest.mark.parametrize("name", list(R.TESTS))
def test_both_paths_against_the_restatement_and_each_other(pkg, calls, name, content):
    test = R.TESTS[name]
    call, refs = calls[content]
    got = {}
    try:
        for cap in (0, 128):
            pkg.categorical_test_hooks(small_cap=cap)
            got[cap] = pkg.categorical_test_batch_host(call["off"], call["a"], call["b"], test, {"correction": False})   # the restatement's default
            errs = R.check_records(test, got[cap], refs[test])
            print(name, content, "cap", cap or "default", {k: "%.2e" % e for k, e in errs.items()})
    finally:
        pkg.categorical_test_hooks(0)
    assert got[0].tobytes() == got[128].tobytes()          # the lead wavefront runs the same code on either path


def test_yates_correction_on_both_paths(pkg, calls):
    call, _ = calls["2x2"]
    ref = R.reference(R.CHI_SQUARE, dict(call, opts=dict(correction=True)))
    try:
        got = []
        for cap in (0, 128):
            pkg.categorical_test_hooks(small_cap=cap)
            got.append(pkg.categorical_test_batch_host(call["off"], call["a"], call["b"], R.CHI_SQUARE, {"correction": True}))
            R.check_records(R.CHI_SQUARE, got[-1], ref)
    finally:
        pkg.categorical_test_hooks(0)
    assert got[0].tobytes() == got[1].tobytes() and np.any(got[0][:, 0] != calls["2x2"][1][R.CHI_SQUARE][:, 0])


@pytest.mark.parametrize("alternative", (R.TWO_SIDED, R.LESS, R.GREATER))
def test_fisher_tables(pkg, alternative):
    """Margins of 1000 with the observed cell at both ends of the support and in the middle, a zero cell, every alternative."""
    for level in (0.95, None):
        call = R.cells_call(R.FISHER_TABLES, dict(alternative=alternative, confidence_level=level))
        opts = pkg.CategoricalTestOptions(alternative=alternative, confidence_level=level)
        got = pkg.categorical_test_batch_host(call["off"], call["a"], call["b"], R.FISHER_EXACT, opts)
        errs = R.check_records(R.FISHER_EXACT, got, R.reference(R.FISHER_EXACT, call))
        print("fisher", alternative, level, {k: "%.2e" % e for k, e in errs.items()})


def test_mcnemar_tables(pkg):
    """b + c = 0, b = c, exact and asymptotic with and without the correction."""
    for opts in (dict(correction=True), dict(correction=False), dict(exact=True)):
        call = R.cells_call(R.MCNEMAR_TABLES, opts)
        got = pkg.categorical_test_batch_host(call["off"], call["a"] * 5, call["b"] * -2, R.MCNEMAR, opts)
        R.check_records(R.MCNEMAR, got, R.reference(R.MCNEMAR, call))
        assert np.isnan(got[0, 0]) and np.isnan(got[0, 1]) and got[0, 11] == 0 and got[1, 9] == got[1, 10]


def test_device_entry_on_the_current_stream(pkg, calls):
    import torch
    call, refs = calls["5x7"]
    dev = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
    ctx = pkg.Context(0)
    off, a, b = dev(call["off"]), dev(call["a"]), dev(call["b"])
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        rec = ctx.categorical_test_batch_device(off, a, b, R.CHI_SQUARE)
        none = ctx.categorical_test_batch_device(off[:1], a[:0], b[:0], R.G_TEST)          # zero groups
    stream.synchronize()
    assert none.shape == (0, 12)
    assert rec.cpu().numpy().tobytes() == pkg.categorical_test_batch_host(call["off"], call["a"], call["b"], R.CHI_SQUARE, ctx=ctx).tobytes()
    # offsets outside [0, n_rows] are clipped as group_rows clips them: the device form does not read them on the host
    wild = call["off"].copy()
    wild[0], wild[-1] = -5, wild[-1] + 1000
    clipped = ctx.categorical_test_batch_device(dev(wild), a, b, R.CHI_SQUARE)
    torch.cuda.synchronize()
    R.check_records(R.CHI_SQUARE, clipped.cpu().numpy(), refs[R.CHI_SQUARE])
    ctx.close()


def test_aggregates_and_scalars_reproduce_the_sql_tables(pkg):
    fixtures = R.load_tables(os.path.join(ROOT, "tests", "golden", "categorical_tests"))

    def by_agg(function, a, b):
        keys = np.array(["k"] * len(a) + ["other"] * 3)
        got = getattr(pkg, function + "_agg")(keys, np.concatenate([a, [0, 1, None]]), np.concatenate([b, [1, None, 0]])).by_key()
        assert got["other"] is None                              # one valid row: a NULL label makes its row invalid
        ref = restated_aggregate(function, a, b)
        if isinstance(ref, dict):
            for key, value in ref.items():
                assert abs(got["k"][key] - value) <= 1e-9 * max(1.0, abs(value)), (function, key)
        return got["k"]
    R.check_known_answers(fixtures, by_agg)

    def by_scalar(function, a, b):
        if function != "chisq_test":
            return restated_aggregate(function, a, b)            # the other scalars touch no device: test_categorical_test_abi_cpu.py
        d = pkg.chisq_test(a.astype(np.float64), b.astype(np.float64))
        assert d["method"] == "Pearson's Chi-squared test"
        return d
    R.check_known_answers(fixtures, by_scalar)
    # NaN rows are dropped, labels are cast toward zero, negative ones to 0; Yates' correction through the options
    d = pkg.chisq_test([0.0, 0.9, 1.2, np.nan, 1.0, -3.0, 0.0, 1.5], [0.0, 1.0, 1.0, 1.0, 0.0, 1.0, None, 0.2], {"correction": True})
    ref = R.table_record(R.CHI_SQUARE, np.array([[1, 2], [2, 1]]), True)
    assert abs(d["statistic"] - ref[0]) <= 1e-12 and abs(d["p_value"] - ref[1]) <= 1e-12 and d["df"] == 1
    with pytest.raises(pkg.InvalidInputException, match="at least 2 rows and 2 columns"):
        pkg.chisq_test([1.0, 1.0, 1.0], [0.0, 1.0, 2.0])
    # the aggregates' NULL rules: row minimums, fewer than two levels, phi off a 2 x 2 table
    keys = ["three"] * 3 + ["flat"] * 5 + ["wide"] * 6
    a = [0, 1, 1, 0, 1, 0, 1, 0, 0, 1, 2, 0, 1, 2]
    b = [0, 1, 0, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 0]
    assert pkg.chisq_test_agg(keys, a, b).by_key()["three"]["df"] == 1 and pkg.cramers_v_agg(keys, a, b).by_key()["three"] is not None
    for agg in (pkg.g_test_agg, pkg.mcnemar_agg, pkg.phi_coefficient_agg, pkg.contingency_coef_agg, pkg.fisher_exact_agg):
        assert agg(keys, a, b).by_key()["three"] is None
    assert pkg.chisq_test_agg(keys, a, b).by_key()["flat"] is None and pkg.cramers_v_agg(keys, a, b).by_key()["flat"] is None
    assert pkg.phi_coefficient_agg(keys, a, b).by_key()["wide"] is None and pkg.contingency_coef_agg(keys, a, b).by_key()["wide"] > 0
    assert pkg.mcnemar_agg(keys, a, b, {"correction": False}).by_key()["wide"]["method"] == "McNemar's Chi-squared test"
