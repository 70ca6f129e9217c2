"""The randomised cases of the GLM sweeps (tests/test_glm_fuzz_cpu.py on the host build of csrc/glm_irls.h,
tests/test_gpu_fuzz_glm.py on the MI355X) and the default-tolerance comparison both make.  A plain module: the reference of
every group is tests/glm_restate.py::fit, computed once per seed (glm_cases.reference); the arrays of a case are read-only.

A seed draws
  width       k = 1 + seed % 33, family = (seed // 33) % 2: one base pass of 66 seeds meets every k = 1 .. 33 (every slice width
              T' = 4 .. 64 of the Gram mapping, every entry class EM, T = 253 of 256 owned entries at k = 21) in both families;
              fit_intercept is drawn and p = k - [intercept], with the intercept forced where p would leave 1 .. 32 (k = 1: none,
              k = 33: one);
  lambda      one of 0, 0, 1e-3, 0.5, 10;
  offset      on or off; a Poisson call without an intercept always has one (the `counts` shift has nowhere else to go);
  24 groups   of k, k + 1, 2 k + 1, 63, 64, 65, 127, 128, 129, 191, 193 rows and 13 of max(12 k, 40) + U{0 .. 40} (436 at most);
  per group   one REGIME, dealt round-robin in a shuffled order so that every regime the call allows occurs:
                plain       glm_cases.make_call's draw: x in [-1, 1], sum |b| in [0.3, 2.2], |intercept| <= 0.5, offset +-0.3;
                counts      Poisson: the predictor shifted by U(6, 12) (means of e^6 .. e^15) through the intercept, or through an
                            offset of that size without one;
                fractional  binomial: y = Binomial(m, mu) / m, m drawn per row from 2 .. 19 (the x log x terms of the deviance);
                noninteger  Poisson: y + U(0, 1) where y > 0;
                bigoffset   the offset U(-3, 3) (calls with an offset);
                steep       sum |b| in [3, 6];
              and, on five of the long groups, glm_cases' patterns nanrows, const, dup, badsupport and degenerate (plain draws).

The tight comparison (tolerance 1e-12) is glm_cases.check_record, its bounds and its in_conditions filter unchanged.  The
default-tolerance comparison is check_default_record below: glm_cases.check_record takes the kernel's reported deviance as the
objective, and at counts around 1e5 a deviance summed in double carries a rounding of about eps y log y per row, more than the
-1e-12 (0.1 + obj) the lower bound allows; so here the objective deviance + lambda sum b^2 is evaluated in np.longdouble at the
record's coefficients and at the restatement's, and the reported deviance is held separately to the long-double deviance at the
record's own coefficients.

Conditions on the INPUT are asserted on the restatement alone (assert_seed_compares, pooled_share): no case is skipped, a seed
that breaks one fails."""
import os

import numpy as np

import glm_cases as GC

POISSON, BINOMIAL = GC.POISSON, GC.BINOMIAL
SCALE = max(1, int(os.environ.get("ANOFOX_FUZZ_SCALE", "1")))
BASE_SEEDS = 66                                   # every k = 1 .. 33 in both families
SEEDS = list(range(BASE_SEEDS * SCALE))
N_GROUPS = 24
LAMBDAS = (0.0, 0.0, 1e-3, 0.5, 10.0)
SPECIAL = ("nanrows", "const", "dup", "badsupport", "degenerate")
OUTSIDE_CAP = 0.05
MIN_COMPARED = 12


def regimes_of(family, icpt, with_offset):
    out = ["plain", "steep"]
    out += ["counts", "noninteger"] if family == POISSON else ["fractional"]
    if with_offset:
        out.append("bigoffset")
    return out


def shape(seed):
    """-> (family, p, fit_intercept, lambda, with_offset, rng) of a seed; rng goes on to draw the rows."""
    rng = np.random.default_rng([20261019, seed])
    k = 1 + seed % 33
    family = (seed // 33) % 2
    icpt = bool(rng.integers(0, 2))
    if not 1 <= k - icpt <= 32:
        icpt = not icpt
    lam = float(LAMBDAS[int(rng.integers(0, len(LAMBDAS)))])
    with_offset = bool(rng.integers(0, 2)) or (family == POISSON and not icpt)
    return family, k - icpt, icpt, lam, with_offset, rng


_CASES = {}


def case(seed):
    """glm_cases.make_call's dict (family, p, icpt, lam, offsets, y, x, off, kinds, seed) of a sweep seed; kinds[g] is the
    group's regime or pattern.  The seed key is offset so that glm_cases.reference caches it apart from the seeded calls."""
    if seed in _CASES:
        return _CASES[seed]
    family, p, icpt, lam, with_offset, rng = shape(seed)
    k = p + int(icpt)
    big = max(12 * k, 40)
    sizes = [k, k + 1, 2 * k + 1, 63, 64, 65, 127, 128, 129, 191, 193]
    sizes += [big + int(rng.integers(0, 41)) for _ in range(N_GROUPS - len(sizes))]
    allowed = regimes_of(family, icpt, with_offset)
    deal = [allowed[i] for i in rng.permutation(len(allowed))]
    kinds = [deal[g % len(deal)] for g in range(N_GROUPS)]
    for j, s in enumerate(SPECIAL):                # the patterns sit on long groups
        kinds[N_GROUPS - 1 - j] = s
    ys, xs, offs = [], [], []
    for n, kind in zip(sizes, kinds):
        x = rng.uniform(-1.0, 1.0, size=(n, p))
        b = rng.normal(size=p)
        b *= (rng.uniform(3.0, 6.0) if kind == "steep" else rng.uniform(0.3, 2.2)) / max(np.sum(np.abs(b)), 1e-9)
        b0 = rng.uniform(-0.5, 0.5) if icpt else 0.0
        o = np.zeros(n)
        if with_offset:
            o = rng.uniform(-3.0, 3.0, size=n) if kind == "bigoffset" else rng.uniform(-0.3, 0.3, size=n)
        if kind == "counts":
            shift = rng.uniform(6.0, 12.0)
            if icpt:
                b0 += shift
            else:
                o = o + shift
        if kind == "const":
            x[:, p // 2] = 0.75
        if kind == "dup" and p >= 2:
            x[:, p - 1] = x[:, 0]
        eta = x @ b + b0 + o
        if family == POISSON:
            y = rng.poisson(np.exp(eta if kind == "counts" else eta + 1.0)).astype(float)
            if kind == "noninteger":
                y = np.where(y > 0, y + rng.uniform(0.0, 1.0, size=n), y)
        else:
            mu = 1.0 / (1.0 + np.exp(-eta))
            if kind == "fractional":
                m = rng.integers(2, 20, size=n)
                y = rng.binomial(m, mu) / m
            else:
                y = (rng.uniform(size=n) < mu).astype(float)
        if kind == "badsupport":
            y[n // 3] = -1.0 if family == POISSON else 1.5
        if kind == "degenerate":
            y[:] = 0.0 if family == POISSON else 1.0
        if kind == "nanrows":
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
    c = dict(family=family, p=p, icpt=icpt, lam=lam, offsets=offsets, y=np.concatenate(ys), x=np.vstack(xs),
             off=np.concatenate(offs) if with_offset else None, kinds=kinds, seed=("fuzz", seed))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASES[seed] = c
    return c


def case_id(seed):
    family, p, icpt, lam, with_offset, _ = shape(seed)
    return "%d-%s-k%d-%s-lam%g-%s" % (seed, "poisson" if family == POISSON else "binomial", p + int(icpt), "icpt" if icpt else "noicpt", lam,
                                      "off" if with_offset else "nooff")


def label(call, g):
    return "seed %s group %d (%s, n=%d)" % (call["seed"][1], g, call["kinds"][g], call["offsets"][g + 1] - call["offsets"][g])


def group(call, g):
    """-> (y, x, offset or None) of group g, every row."""
    s = slice(call["offsets"][g], call["offsets"][g + 1])
    return call["y"][s], call["x"][s], None if call["off"] is None else call["off"][s]


def assert_seed_compares(call, refs):
    """Every seed compares at least MIN_COMPARED of its 24 groups; -> that count."""
    n = sum(GC.in_conditions(r, call["p"]) for r in refs)
    assert n >= MIN_COMPARED, "seed %s: only %d of %d groups are inside the input conditions" % (call["seed"][1], n, len(refs))
    return n


def pooled_share(seeds):
    """-> (outside, pool): over the seeds, the fitted groups of at least 12 k rows (dup and degenerate excluded) and those of
    them outside the input conditions."""
    outside = pool = 0
    for seed in seeds:
        call = case(seed)
        k = call["p"] + int(call["icpt"])
        for ref, kind, n in zip(GC.reference(call), call["kinds"], np.diff(call["offsets"])):
            if ref["status"] == 0 and kind not in ("dup", "degenerate") and n >= 12 * k:
                pool += 1
                outside += not GC.in_conditions(ref, call["p"])
    return outside, pool


def objective_longdouble(family, y, x, off, icpt, lam, coef, intercept):
    """-> (deviance, deviance + lambda sum b^2) in np.longdouble over the valid rows at the given coefficients (a NaN
    coefficient is a dropped column: 0)."""
    L = np.longdouble
    ok = np.isfinite(y) & np.isfinite(x).all(axis=1) & (True if off is None else np.isfinite(off))
    yl, xl = y[ok].astype(L), x[ok].astype(L)
    b = np.where(np.isnan(coef), 0.0, coef).astype(L)
    eta = xl @ b + (L(intercept) if icpt else L(0)) + (L(0) if off is None else off[ok].astype(L))
    pos = yl > 0
    if family == POISSON:
        ylog = np.zeros_like(yl)
        ylog[pos] = yl[pos] * (np.log(yl[pos]) - eta[pos])
        dev = 2 * np.sum(ylog - (yl - np.exp(eta)))
    else:
        lmu, lq = -np.log1p(np.exp(-eta)), -np.log1p(np.exp(eta))
        one = 1 - yl
        t = np.zeros_like(yl)
        t[pos] += yl[pos] * np.log(yl[pos])
        t[one > 0] += one[one > 0] * np.log(one[one > 0])
        dev = 2 * np.sum(t - yl * lmu - one * lq)
    return dev, dev + L(lam) * np.sum(b * b)


def check_default_record(rec, call, g, ref, errs=None):
    """One group's record of a run at the default tolerance 1e-8 against the restatement `ref`: the status and NaN rules of
    glm_cases.check_record; then, inside the input conditions, with obj = deviance + lambda sum b^2 in np.longdouble,
        -1e-12 (0.1 + obj) <= obj(record's coefficients) - obj(restatement's) <= 2e-8 (0.1 + obj),
    and the reported deviance within max(1e-9 |dev|, 1e-13 (n + sum y)) of the long-double deviance at the record's own
    coefficients.  -> whether the values were compared."""
    p, what = call["p"], label(call, g)
    status = int(rec[p + 10])
    inside = GC.in_conditions(ref, p)
    if ref["status"] != 0:
        assert status == ref["status"], (what, status, ref["status"])
    elif inside:
        assert status == 0, (what, status)
    else:
        assert status in (0, 3), (what, status)
    if status != 0:
        assert np.all(np.isnan(rec[:p + 10])), what
        return False
    assert rec[p + 6] == ref["n_obs"] and rec[p + 9] == 1.0, what
    assert np.all(np.isnan(rec[:p])[ref["dropped"]]), what
    if not inside:
        return False
    assert np.array_equal(np.isnan(rec[:p]), np.isnan(ref["coef"])), what
    y, x, off = group(call, g)
    dev, obj = objective_longdouble(call["family"], y, x, off, call["icpt"], call["lam"], rec[:p], rec[p])
    _, robj = objective_longdouble(call["family"], y, x, off, call["icpt"], call["lam"], ref["coef"], ref["intercept"])
    excess = float((obj - robj) / (0.1 + obj))
    floor = 1e-13 * (ref["n_obs"] + ref["sum_y"])
    dev_err = max(0.0, abs(float(rec[p + 1] - dev)) - floor) / max(abs(float(dev)), 1e-300)
    if errs is not None:
        errs["default_obj_excess"] = max(errs.get("default_obj_excess", 0.0), excess)
        errs["default_obj_excess_min"] = min(errs.get("default_obj_excess_min", 0.0), excess)
        errs["default_deviance"] = max(errs.get("default_deviance", 0.0), dev_err)
    assert -1e-12 <= excess <= 2e-8, (what, float(obj), float(robj), excess)
    assert abs(float(rec[p + 1] - dev)) <= max(1e-9 * abs(float(dev)), floor), (what, rec[p + 1], float(dev))
    return True
