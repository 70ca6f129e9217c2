"""Seeded cases and the checks of the GLM extras (the Poisson interval of fit-predict, the binomial training accuracy), shared by
the CPU tier (tests/tools/glm_extras_host.cpp) and the GPU tier (tests/test_gpu_glm_extras.py).

A CALL is one batch of 9 groups of a family at one width.  Widths: p = 1 without an intercept (k = 1), and with an intercept
k = 9 and 10, 21 and 22 (the edges of the kernel's entry classes), and 33.  Group sizes: 1 (fails: the fit-predict rule, or fewer
rows than parameters), 2, 63, 64, 65, 129 (the edges of the 64-row tile), two of max(12 k, 40) + 7 rows (the second with a NaN in x
on one row and a row without y), and one of 12 k + 40 rows.  Every second width carries an offset.

The narrow groups of a wide call (63 .. 129 rows at k = 21 .. 33) are often separated or ill-conditioned; they are still fitted, and
the checks that need no yardstick (the bounds from the same run's mu and dispersion, the accuracy as a count over the same run's mu)
hold for them.  The comparisons with tests/glm_restate.py are made for the groups inside glm_cases.in_conditions.

Bounds of the comparison with the restatement (mu to 1e-9, dispersion to 1e-6: the tolerances of glm_cases.check_record): with
h = z s, s = sqrt(dispersion) / max(mu, 0.001), a bound is exp(eta -+ h), so to first order its relative error is that of mu
(1e-9) plus the absolute error of h, h (1e-9 + 0.5e-6); twice that is allowed: 1e-9 + 2 h (1e-9 + 0.5e-6), on rows with h <= 10.
The accuracy is an exact count, compared with the restatement's count where no restated mu lies within 1e-6 of the threshold (a mu
known to 1e-9 cannot change sides there); the seeds are chosen so that no compared group has such a row (asserted, cap 0)."""
import numpy as np

import glm_cases as GC

POISSON, BINOMIAL = GC.POISSON, GC.BINOMIAL
Z = 1.96
THRESHOLD = 0.5
BAND = 1e-6
WIDTHS = ((1, False), (8, True), (9, True), (20, True), (21, True), (32, True))


def calls():
    """(family, p, fit_intercept, with_offset, seed) of every call."""
    out = []
    for f, family in enumerate((POISSON, BINOMIAL)):
        for i, (p, icpt) in enumerate(WIDTHS):
            out.append((family, p, icpt, bool(i & 1), 4100 + 10 * f + i))
    return out


def ident(c):
    return "%s-p%d-%s-%s" % ("poisson" if c[0] == POISSON else "binomial", c[1], "icpt" if c[2] else "noicpt", "off" if c[3] else "nooff")


_CALLS = {}


def make_call(family, p, icpt, with_offset, seed):
    """-> the dict of glm_cases.make_call (lam = 0)."""
    if seed in _CALLS:
        return _CALLS[seed]
    rng = np.random.default_rng(seed)
    k = p + (1 if icpt else 0)
    big = max(12 * k, 40) + 7
    sizes = [1, 2, 63, 64, 65, 129, big, big, 12 * k + 40]
    kinds = ["one", "plain", "plain", "plain", "plain", "plain", "plain", "nanrow", "plain"]
    ys, xs, offs = [], [], []
    for n, kind in zip(sizes, kinds):
        x = rng.uniform(-1.0, 1.0, size=(n, p))
        b = rng.normal(size=p)
        b *= rng.uniform(0.3, 2.2) / max(np.sum(np.abs(b)), 1e-9)
        b0 = rng.uniform(-0.5, 0.5) if icpt else 0.0
        o = rng.uniform(-0.3, 0.3, size=n) if with_offset else np.zeros(n)
        eta = x @ b + b0 + o
        if family == POISSON:
            y = rng.poisson(np.exp(eta + 1.0)).astype(float)
        else:
            y = (rng.uniform(size=n) < 1.0 / (1.0 + np.exp(-eta))).astype(float)
        if kind == "nanrow":
            x[3, p - 1] = np.nan   # no mu, no bounds, not counted
            y[5] = np.nan          # a row to predict only: mu and bounds, not counted
        ys.append(y)
        xs.append(x)
        offs.append(o)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    call = dict(family=family, p=p, icpt=icpt, lam=0.0, offsets=offsets, y=np.concatenate(ys), x=np.vstack(xs),
                off=np.concatenate(offs) if with_offset else None, kinds=kinds, seed=seed)
    _CALLS[seed] = call
    return call


def host_input(call, tolerance, predict, interval_z, threshold, want_accuracy, max_iterations=100):
    """The bytes tests/tools/glm_extras_host.cpp reads for a call."""
    o, p = call["offsets"], call["p"]
    parts = [np.array([len(o) - 1], float)]
    for g in range(len(o) - 1):
        s = slice(o[g], o[g + 1])
        n = o[g + 1] - o[g]
        parts.append(np.array([call["family"], call["icpt"], max_iterations, tolerance, call["lam"], p, n, call["off"] is not None,
                               predict, n if predict else -1, interval_z, threshold, want_accuracy], float))
        cols = [call["y"][s, None], call["x"][s]] + ([call["off"][s, None]] if call["off"] is not None else [])
        parts.append(np.hstack(cols).ravel())
    return np.concatenate(parts).tobytes()


def formula(mu, dispersion, z):
    """The reference's bounds from mu (Poisson: eta = log mu) and the dispersion; NaN where mu is."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        h = z * np.sqrt(dispersion) / np.maximum(mu, 0.001)
        eta = np.log(mu)
        return np.maximum(0.0, np.exp(eta - h)), np.exp(eta + h), h


def check_interval(rec, pred, ref, p, z, label, errs=None):
    """One fitted Poisson group: pred[n, 3] of a run with interval_z = z against the formula on the run's own mu and dispersion
    (rtol 1e-9) and, inside the input conditions, on the restatement's.  -> whether the restatement was compared."""
    mu, lo, hi = pred[:, 0], pred[:, 1], pred[:, 2]
    fin = np.isfinite(mu)
    assert np.all(np.isnan(lo[~fin])) and np.all(np.isnan(hi[~fin])), label
    assert np.all(np.isfinite(lo[fin])) and np.all(hi[fin] >= mu[fin]) and np.all(lo[fin] <= mu[fin]) and np.all(lo[fin] >= 0), label
    wl, wh, _ = formula(mu[fin], rec[p + 5], z)
    assert np.allclose(lo[fin], wl, rtol=1e-9, atol=0) and np.allclose(hi[fin], wh, rtol=1e-9, atol=0), label
    if not GC.in_conditions(ref, p):
        return False
    rmu = ref["mu_all"]
    assert np.array_equal(np.isnan(rmu), ~fin), label
    rl, rh, h = formula(rmu[fin], ref["dispersion"], z)
    m = h <= 10.0
    assert m.any(), label
    bound = 1e-9 + 2.0 * h[m] * (1e-9 + 0.5e-6)
    for name, got, want in (("lower", lo[fin][m], rl[m]), ("upper", hi[fin][m], rh[m])):
        d = np.abs(got - want) / np.abs(want)
        if errs is not None:
            errs[name] = max(errs.get(name, 0.0), float(np.max(d / bound)))
        assert np.all(d <= bound), (label, name, float(np.max(d / bound)))
    return True


def count_accuracy(y, mu, threshold):
    """The share of the rows with a finite y and a finite mu for which (mu >= threshold) == y (the scalar entry's count)."""
    m = np.isfinite(y) & np.isfinite(mu)
    return float(np.sum((mu[m] >= threshold).astype(float) == y[m])) / max(int(m.sum()), 1)


def band_rows(call, refs, threshold=THRESHOLD):
    """The rows of the compared groups whose restated mu lies within BAND of the threshold (must be none)."""
    o, out = call["offsets"], 0
    for g, ref in enumerate(refs):
        if GC.in_conditions(ref, call["p"]):
            mu = ref["mu_all"]
            out += int(np.sum(np.abs(mu[np.isfinite(mu)] - threshold) <= BAND))
    return out


def check_accuracy(acc, status, y, mu, ref, p, threshold, label):
    """One binomial group: acc against the count over the same entry's mu (or None), and against the restatement's count inside
    the input conditions.  -> whether the restatement was compared."""
    if status != 0:
        assert np.isnan(acc), label
        return False
    if mu is not None:
        assert acc == count_accuracy(y, mu, threshold), (label, acc, count_accuracy(y, mu, threshold))
    if not GC.in_conditions(ref, p):
        return False
    assert acc == count_accuracy(y, ref["mu_all"], threshold), (label, acc)
    return True
