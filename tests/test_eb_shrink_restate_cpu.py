"""The restatement of eb_shrink (tests/eb_shrink_restate.py) against the reference's own unit fixtures (data only:
tests/golden/eb_shrink/fixtures.json) and hand-computed cases, and the cap on the sets the clamp rule leaves out of the value
comparison (tests/eb_shrink_cases.py), which is a property of the cases and the restatement alone."""
import json
import math
import os

import numpy as np
import pytest

import eb_shrink_cases as EC
import eb_shrink_restate as R

FIX = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eb_shrink", "fixtures.json")))


def arr(v):
    return np.array([np.nan if x is None else x for x in v], dtype=np.float64)


def fixture():
    return arr(FIX["fixture"]["estimate"]), arr(FIX["fixture"]["se"])


def test_matches_the_dersimonian_laird_formulas_in_plain_float64():
    est, se = fixture()
    s, out, _ = R.shrink_set(est, se)
    w = 1 / se ** 2
    fixed = math.fsum(w * est) / math.fsum(w)
    q = math.fsum(w * (est - fixed) ** 2)
    c = math.fsum(w) - math.fsum(w * w) / math.fsum(w)
    tau2 = max(0.0, (q - 4.0) / c)
    wr = 1 / (se ** 2 + tau2)
    mu = math.fsum(wr * est) / math.fsum(wr)
    tol = FIX["formula_tolerance"]
    assert abs(s[4] - q) < tol and abs(s[2] - tau2) < tol and abs(s[0] - mu) < tol and abs(s[1] - math.sqrt(1 / math.fsum(wr))) < tol
    assert s[5] == 5 and s[6] == 5 and s[7] == 0 and tau2 > 0


def test_properties_of_the_reference_fixture():
    est, se = fixture()
    s, out, _ = R.shrink_set(est, se)
    lo, hi = np.minimum(est, s[0]), np.maximum(est, s[0])
    assert np.all(out[:, 0] >= lo - 1e-12) and np.all(out[:, 0] <= hi + 1e-12)       # between the estimate and the mean
    order = np.argsort(se)
    assert np.all(np.diff(out[order, 2]) <= 0)                                       # noisier groups are pulled harder
    assert np.all(out[:, 1] <= se + 1e-12)                                           # shrinkage reduces the standard error
    assert est.min() < s[0] < est.max()


def test_identical_estimates_pool_completely():
    h = FIX["homogeneous"]
    s, out, _ = R.shrink_set(arr(h["estimate"]), arr(h["se"]))
    assert s[2] == 0.0 and s[3] == 0.0 and np.all(out[:, 2] == 0.0)
    assert np.all(np.abs(out[:, 0] - s[0]) < 1e-12) and abs(s[0] - 0.5) < 1e-15
    assert np.all(out[:, 1] == s[1]) and abs(s[1] - 1 / math.sqrt(sum(1 / v ** 2 for v in h["se"]))) < 1e-15


def test_a_fixed_tau_squared_by_hand():
    # two pairs, se 1 and 2, tau^2 = 3: wr = 1/4, 1/7; mu = (1/4 * 2 + 1/7 * 9) / (11/28) = 50/11; mu_se = sqrt(28/11)
    s, out, _ = R.shrink_set([2.0, 9.0], [1.0, 2.0], tau_squared=3.0)
    assert s[2] == 3.0 and abs(s[0] - 50 / 11) < 1e-15 and abs(s[1] - math.sqrt(28 / 11)) < 1e-15
    # weight = 1 / (1 + 1/3) = 3/4 and (1/4) / (1/4 + 1/3) = 3/7; shrunken_se = sqrt(1 / (1 + 1/3)), sqrt(1 / (1/4 + 1/3))
    assert np.allclose(out[:, 2], [0.75, 3 / 7], rtol=0, atol=1e-15)
    assert np.allclose(out[:, 0], [0.75 * 2 + 0.25 * 50 / 11, 3 / 7 * 9 + 4 / 7 * 50 / 11], rtol=0, atol=1e-14)
    assert np.allclose(out[:, 1], [math.sqrt(0.75), math.sqrt(12 / 7)], rtol=0, atol=1e-15)
    # Q = 1 * (2 - 3.4)^2 + (1/4) (9 - 3.4)^2 = 9.8 about fixed = (2 + 9/4) / (5/4) = 3.4; I^2 = (9.8 - 1) / 9.8
    assert abs(s[4] - 9.8) < 1e-14 and abs(s[3] - 8.8 / 9.8) < 1e-15
    big = FIX["large_tau"]
    est, se = fixture()
    s, out, _ = R.shrink_set(est, se, tau_squared=big["tau_squared"])
    assert np.all(np.abs(out[:, 0] - est) < big["max_move"]) and np.all(out[:, 2] > big["min_weight"])


def test_method_none_and_heterogeneity():
    est, se = fixture()
    s, out, _ = R.shrink_set(est, se, method=R.NONE)
    w = 1 / se ** 2
    assert s[2] == 0.0 and np.all(out[:, 0] == s[0]) and abs(s[0] - math.fsum(w * est) / math.fsum(w)) < 1e-15
    assert s[3] > 0      # I^2 does not depend on the method
    h = FIX["heterogeneous"]
    s, _, _ = R.shrink_set(arr(h["estimate"]), arr(h["se"]))
    assert s[3] > h["min_i_squared"] and s[2] > h["min_tau_squared"]


def test_unusable_rows_and_failures():
    u = FIX["unusable"]
    s, out, _ = R.shrink_set(arr(u["estimate"]), arr(u["se"]))
    assert s[5] == u["n_groups"] and s[6] == 4 and len(out) == 4
    assert np.all(np.isnan(out[u["nan_rows"]])) and np.all(np.isfinite(out[u["finite_rows"]]))
    s, out, _ = R.shrink_set(arr(FIX["single"]["estimate"]), arr(FIX["single"]["se"]))
    assert s[7] == FIX["single"]["status"] and np.all(np.isnan(s[:7])) and np.all(np.isnan(out))
    assert R.shrink_set([], [])[0][7] == 10
    est, se = fixture()
    for bad in (FIX["negative_tau"]["tau_squared"], float("inf")):
        s, out, _ = R.shrink_set(est, se, tau_squared=bad)
        assert s[7] == FIX["negative_tau"]["status"] and np.all(np.isnan(out))
    assert R.shrink_set(est, se, method=7)[0][7] == 1


@pytest.mark.parametrize("seed_shift", [0, 1000, 2000])
def test_few_sets_are_left_out_by_the_clamp_rule(seed_shift):
    """At most 5 % of the generated sets of a seed may sit within the margin of Q = df; about half the homogeneous sets clamp."""
    for c in EC.calls():
        call = EC.make_call(c[0], c[1], c[2], c[3] + seed_shift)
        _, summary, qd = EC.reference(call)
        left = EC.decided_by_clamp(summary, qd)
        assert left.sum() <= 0.05 * left.size
        if c[0] == "homogeneous" and c[1] >= 9:
            good = summary[..., 7] == 0
            share = np.mean(summary[..., 2][good] == 0.0)
            assert 0.25 < share < 0.85, share
