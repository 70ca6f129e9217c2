"""A drawn sweep of the permutation tests against the restatement: sizes, tie density, NaN share, test, alternative, permutations,
seed and small-path cap are all drawn (tests/perm_fuzz_cases.py).  Energy distance and the t-test: the whole record equal.  MMD:
sigma, the counts and the status equal, the statistic within the GPU tier's bound, and n_extreme equal for every group whose
restated statistics are separated from the observed one (tied data can put a permuted statistic within rounding of it)."""
import numpy as np
import pytest

import perm_fuzz_cases as F
import perm_test_restate as R
from conftest import import_pkg
from test_gpu_perm_tests import MMD_STAT_BOUND, separated

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("index", range(F.CALLS))
def test_drawn_call(index):
    pkg = import_pkg()
    case = F.draw_case(index)
    off, v, s = R.pack(case["groups"])
    test, cap = case["test"], case["cap"]
    ref = R.reference(off, v, s, test, case["alternative"], case["n_perm"], case["seed"], case["sigma"], cap or R.CAP)
    opts = pkg.PermTestOptions(case["n_perm"], case["seed"], None if case["sigma"] != case["sigma"] else case["sigma"], case["alternative"])
    try:
        pkg.perm_test_hooks(cap)
        got = pkg.perm_test_batch_host(off, v, s, test, opts)
    finally:
        pkg.perm_test_hooks(0)
    print({k: case[k] for k in ("test", "alternative", "n_perm", "cap", "sigma")}, "groups", len(off) - 1)
    if test != R.MMD:
        assert np.array_equal(got, ref, equal_nan=True), np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref)))).tolist()[:8]
        return
    assert np.array_equal(got[:, [2, 4, 5, 6, 7]], ref[:, [2, 4, 5, 6, 7]], equal_nan=True)
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref[:, 0]))
    if not np.isnan(ref[:, 0]).all():
        assert np.nanmax(np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-3)) <= MMD_STAT_BOUND
    for g in range(len(off) - 1):
        if ref[g, 7] == 0 and ref[g, 0] == ref[g, 0]:
            stats = R.group_stats(v[off[g]:off[g + 1]], s[off[g]:off[g + 1]], test, case["n_perm"], case["seed"], case["sigma"], cap or R.CAP)[3]
            if separated(stats):
                assert got[g, 3] == ref[g, 3] and (got[g, 1] == ref[g, 1] or case["n_perm"] == 0)
