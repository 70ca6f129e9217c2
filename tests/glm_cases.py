"""Seeded cases of the GLM tests and `check_record`, shared by the CPU tier (tests/tools/glm_host.cpp) and the GPU tier.

A CALL is one batch: a family, p, fit_intercept, lambda, offset on / off and 70 groups.  Group sizes: 0, 1, k - 1, k, k + 1, 63,
64, 65, ~200, one of 5000 rows, the rest max(12 k, 40) .. + 40 rows.  Patterns: NaN / +-inf rows in y, x and the offset, a
constant column, a duplicated column, a y outside the support, an all-zero Poisson group / an all-ones binomial group.  True
coefficients keep |eta| <= 3 (x in [-1, 1], sum |b| <= 2.2, |intercept| <= 0.5, |offset| <= 0.3).

What is compared (ISSUE / DESIGN.md §1): every group's status, NaN pattern, n_observations and n_params; and, for the groups
inside the input conditions (not separated, p kappa^2 2^-53 <= 1e-10, |eta| <= 30 so that no clamp is active), the values
against tests/glm_restate.py.

Outside the input conditions a fit has no well-defined answer to compare: a separated group has no finite optimum (the loop may
stop on its relative-change test, status 0, or run out of iterations, status 3), and the rank of a design whose kappa is beyond the
bound depends on the tolerance it is taken at.  So there the statuses of the row rules (1, 6, 10) are exact, a status of the fit is
in {0, 3}, n_observations is exact, and n_params is asserted only where the deficiency is structural (a constant or an exactly
duplicated column).
The restatement stops at a score below 1e-12 max(1, ||X'y||), which a fit that diverges (the all-zero Poisson group, the all-ones
binomial group, a perfectly fitted group of k rows) reaches at |eta| between 25 and 29, before its `separated` flag (|eta| > 30)
can rise: between 20 and 30 the restatement cannot tell an optimum from a divergence.  The generator keeps |eta| <= 3.3 at the
truth, so the compared set is further narrowed to max|eta| <= 20 (ETA_RESOLVED); that only removes groups, it widens no bound.
A deviance is a sum of n unit deviances, each carrying an absolute rounding error of a few eps (y + mu): a relative bound on it
carries the absolute floor 1e-13 (n + sum y) (about 450 eps per unit of y + 1), which matters only for a saturated fit (deviance = 0 up to rounding).
With lambda > 0 the minimised quantity is deviance + lambda sum b^2, so the default-tolerance bound is taken on that objective
(for lambda = 0 it is the deviance itself)."""
from statistics import NormalDist

import numpy as np

import glm_restate as R

POISSON, BINOMIAL = R.POISSON, R.BINOMIAL
N_GROUPS = 70
WIDTHS = (1, 2, 8, 9, 31, 32)


def calls():
    """(family, p, fit_intercept, lambda, with_offset, seed) of every call."""
    out = []
    i = 0
    for family in (POISSON, BINOMIAL):
        for p in WIDTHS:
            for icpt in (True, False):
                out.append((family, p, icpt, 0.5 if ((i >> 1) ^ i) & 1 else 0.0, bool((i >> 1) & 1), 1000 + i))
                i += 1
    return out


def make_call(family, p, icpt, lam, with_offset, seed):
    """-> dict(family, p, icpt, lam, offsets[G + 1], y, x [N, p], off (or None), kinds[G])."""
    rng = np.random.default_rng(seed)
    k = p + (1 if icpt else 0)
    big = max(12 * k, 40)
    sizes = [0, 1, max(k - 1, 0), k, k + 1, 63, 64, 65, 200 + int(rng.integers(0, 9)), 5000]
    kinds = ["plain"] * len(sizes)
    special = ["nanrows", "const", "dup", "badsupport", "degenerate", "nanrows"]
    while len(sizes) < N_GROUPS:
        sizes.append(big + int(rng.integers(0, 41)))
        kinds.append(special.pop(0) if special else "plain")
    ys, xs, offs = [], [], []
    for n, kind in zip(sizes, kinds):
        x = rng.uniform(-1.0, 1.0, size=(n, p))
        b = rng.normal(size=p)
        b *= rng.uniform(0.3, 2.2) / max(np.sum(np.abs(b)), 1e-9)
        b0 = rng.uniform(-0.5, 0.5) if icpt else 0.0
        o = rng.uniform(-0.3, 0.3, size=n) if with_offset else np.zeros(n)
        if kind == "const":
            x[:, p // 2] = 0.75
        if kind == "dup" and p >= 2:
            x[:, p - 1] = x[:, 0]
        eta = x @ b + b0 + o
        if family == POISSON:
            y = rng.poisson(np.exp(eta + 1.0)).astype(float)  # (means around e: few all-zero groups by chance)
        else:
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
        if kind == "badsupport" and n:
            y[n // 3] = -1.0 if family == POISSON else 1.5
        if kind == "degenerate":
            y[:] = 0.0 if family == POISSON else 1.0
        if kind == "nanrows" and n >= 8:
            y[1] = np.nan
            y[2] = np.inf
            x[3, 0] = np.nan
            x[4, p - 1] = -np.inf
            if with_offset:
                o[5] = np.nan
                o[6] = np.inf
        ys.append(y)
        xs.append(x)
        offs.append(o)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(family=family, p=p, icpt=icpt, lam=lam, offsets=offsets, y=np.concatenate(ys), x=np.vstack(xs),
                off=np.concatenate(offs) if with_offset else None, kinds=kinds, seed=seed)


_REF = {}


def reference(call):
    """The restatement of every group of a call, computed once."""
    key = call["seed"]
    if key not in _REF:
        out = []
        o = call["offsets"]
        for g in range(len(o) - 1):
            s = slice(o[g], o[g + 1])
            out.append(R.fit(call["family"], call["y"][s], call["x"][s], None if call["off"] is None else call["off"][s],
                             call["icpt"], call["lam"]))
        _REF[key] = out
    return _REF[key]


ETA_RESOLVED = 20.0


def in_conditions(ref, p):
    return (ref["status"] == 0 and not ref["separated"] and p * ref["kappa"] ** 2 * 2.0 ** -53 <= 1e-10 and
            ref["max_abs_eta"] <= ETA_RESOLVED)


def zq(confidence_level=0.95):
    return NormalDist().inv_cdf(0.5 + confidence_level / 2.0)


def host_input(call, tolerance, max_iterations=100, predict=False, confidence_level=0.95):
    """The bytes tests/tools/glm_host.cpp reads for a call."""
    o, p = call["offsets"], call["p"]
    parts = [np.array([len(o) - 1], float)]
    for g in range(len(o) - 1):
        s = slice(o[g], o[g + 1])
        n = o[g + 1] - o[g]
        parts.append(np.array([call["family"], call["icpt"], max_iterations, tolerance, call["lam"], 1, zq(confidence_level), p, n,
                               call["off"] is not None, predict, n if predict else -1], float))
        cols = [call["y"][s, None], call["x"][s]] + ([call["off"][s, None]] if call["off"] is not None else [])
        parts.append(np.hstack(cols).ravel())
    return np.concatenate(parts).tobytes()


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def check_record(rec, inf, ref, p, tight, errs=None, pred=None, label="", kind="plain", lam=0.0):
    """One group's record (p + 11), inference (5 p or None) and predictions (or None) against the restatement `ref`.
    tight: the run had tolerance = 1e-12 (values to 1e-9); else the default 1e-8 (converged, deviance within 2e-8 (0.1 + dev)).
    errs: a dict that collects the maxima of the measured errors."""
    status = int(rec[p + 10])
    inside = in_conditions(ref, p)
    if ref["status"] != 0:
        assert status == ref["status"], (label, status, ref["status"])
    elif inside:
        assert status == 0, (label, status)
    else:
        assert status in (0, 3), (label, status)
    if status != 0:
        assert np.all(np.isnan(rec[:p + 10])), label
        assert inf is None or np.all(np.isnan(inf)), label
        assert pred is None or np.all(np.isnan(pred)), label
        return False
    assert rec[p + 6] == ref["n_obs"], (label, rec[p + 6], ref["n_obs"])
    assert rec[p + 9] == 1.0, label
    nan_coef = np.isnan(rec[:p])
    assert np.all(nan_coef[ref["dropped"]]), label
    if inside or (kind in ("dup", "const") and not ref["separated"]):
        assert rec[p + 7] == ref["n_params"], (label, rec[p + 7], ref["n_params"])
        assert int(nan_coef.sum()) + int(np.isnan(rec[p]) and not np.isnan(ref["intercept"])) == ref["k"] - ref["n_params"] + int(ref["dropped"].sum()), label
    if not inside:
        return False
    e = errs if errs is not None else {}

    def note(name, v):
        e[name] = max(e.get(name, 0.0), float(v))
    dev, rdev = rec[p + 1], ref["deviance"]
    if not tight:
        obj = dev + lam * float(np.nansum(rec[:p] ** 2))
        robj = rdev + lam * float(np.nansum(ref["coef"] ** 2))
        note("default_obj_excess", (obj - robj) / (0.1 + obj))
        assert -1e-12 * (0.1 + obj) <= obj - robj <= 2e-8 * (0.1 + obj), (label, obj, robj)
        return True
    b = np.append(rec[:p], rec[p])
    rb = np.append(ref["coef"], ref["intercept"])
    m = ~np.isnan(rb)
    assert np.array_equal(np.isnan(b), np.isnan(rb)), label
    scale = max(1.0, float(np.max(np.abs(rb[m]))))
    note("coef", np.max(np.abs(b[m] - rb[m])) / scale)
    assert np.max(np.abs(b[m] - rb[m])) <= 1e-9 * scale, (label, b, rb)
    for name, got, want in (("deviance", dev, rdev), ("null_deviance", rec[p + 2], ref["null_deviance"]), ("aic", rec[p + 4], ref["aic"])):
        floor = 1e-13 * (ref["n_obs"] + ref["sum_y"])
        note(name, max(0.0, abs(got - want) - floor) / max(abs(want), 1e-300))
        assert abs(got - want) <= max(1e-9 * abs(want), floor), (label, name, got, want)
    note("dispersion", rel(rec[p + 5], ref["dispersion"]))
    assert rel(rec[p + 5], ref["dispersion"]) <= 1e-6, (label, rec[p + 5], ref["dispersion"])
    want_r2 = 1.0 - rdev / ref["null_deviance"] if ref["null_deviance"] > 0 else 0.0
    assert abs(rec[p + 3] - want_r2) <= 1e-9, (label, rec[p + 3], want_r2)
    if inf is not None:
        se, z, pv, lo, hi = (inf[i * p:(i + 1) * p] for i in range(5))
        ms = ~np.isnan(ref["se"])
        assert np.array_equal(np.isnan(se), ~ms), label
        if ms.any():
            note("se", np.max(np.abs(se[ms] / ref["se"][ms] - 1.0)))
            assert np.max(np.abs(se[ms] / ref["se"][ms] - 1.0)) <= 1e-6, (label, se, ref["se"])
            q = zq()
            assert np.allclose(z[ms], rec[:p][ms] / se[ms], rtol=1e-12, atol=0)
            assert np.allclose(lo[ms], rec[:p][ms] - q * se[ms], rtol=1e-9, atol=1e-12)
            assert np.allclose(hi[ms], rec[:p][ms] + q * se[ms], rtol=1e-9, atol=1e-12)
            want_p = np.array([2.0 * (1.0 - NormalDist().cdf(abs(v))) for v in z[ms]])
            assert np.allclose(pv[ms], want_p, rtol=1e-6, atol=1e-14), (label, pv, want_p)
    if pred is not None:
        want = ref["mu_all"]
        assert np.array_equal(np.isnan(pred), np.isnan(want)), label
        mm = ~np.isnan(want)
        if mm.any():
            d = np.abs(pred[mm] - want[mm]) / np.maximum(1.0, np.abs(want[mm]))
            note("pred", np.max(d))
            assert np.max(d) <= 1e-9, (label, np.max(d))
    return True
