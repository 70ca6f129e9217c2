"""The cases of the eb_shrink tests (seeded) and the comparison against tests/eb_shrink_restate.py, shared by the CPU tier
(tests/test_eb_shrink_cpu.py: csrc/eb_shrink.h in its host build) and the GPU tier (tests/test_gpu_eb_shrink.py).

A call is the matrix form of anofox_hip_eb_shrink_batch_*: 13 item ranges x n_cols columns.  The ranges hold m in SIZES items (the
smallest sizes at which the lane mapping can go wrong: empty, below, at and above one and two wavefronts' worth of lanes) and
three ranges of 6 items that unusable pairs leave with k = 0, 1 and 2.  About 5 % of the other pairs are made unusable (NaN / +-inf
estimates, se in {0, -1, NaN, inf}).  The doubles of the strided arrays that belong to no column hold POISON.

Regimes: homogeneous (true tau = 0: about half the sets clamp tau^2 to 0), heterogeneous (true tau = 0.3), wide-se (se spanning
1e-3 .. 1e3) and offset (estimates near 1e6 with spread 1: the case a one-pass Q gets wrong)."""
import numpy as np

import eb_shrink_restate as R

SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 129, 200)
COLS = (1, 2, 9, 32)
REGIMES = ("homogeneous", "heterogeneous", "wide-se", "offset")
STRIDES = ("tight", "glm", "loose")   # n_cols / n_cols;  p + 11 / 5 p (a GLM record and inference batch);  n_cols + 3 / n_cols + 1
POISON = 777.25
MARGIN = 1e-6   # the clamp decides where |Q - df| <= MARGIN max(Q, df): such a set is left out of the value comparison

# Asserted bounds: 100 x the largest error of the host build against the restatement over all calls() (docs/PARITY.md,
# "eb_shrink"), none looser than 1e-9.  Errors are relative to max(|reference|, 1e-12 scale), scale = the set's largest usable
# |estimate| for mu, its smallest usable se^2 for tau_squared, 1 for i_squared and weight, the value otherwise.  One deviation
# from a plain relative error: shrunken = weight est + (1 - weight) mu is a sum of terms of either sign and comes arbitrarily
# close to 0 in the generated data (plain relative error 3.6e-11 on the host build at a value 1e-5 of its terms), so it is
# relative to max(|reference|, 1e-3 of the set's largest usable |estimate|), the floor of the other families' coefficient
# comparisons: its rounding is that of its terms, not of its value.
# Measured maxima (host build, one wavefront per set): mu 3.9e-14, mu_se 1.1e-14, q 1.6e-15, tau_squared 4.8e-14, i_squared 4.8e-14,
# shrunken 8.7e-14, shrunken_se 2.4e-14, weight 4.8e-14.
BOUNDS = {"mu": 3.9e-12, "mu_se": 1.1e-12, "q": 1.6e-13, "tau_squared": 4.8e-12, "i_squared": 4.8e-12, "shrunken": 8.7e-12,
          "shrunken_se": 2.4e-12, "weight": 4.8e-12}


def strides(kind, n_cols):
    return {"tight": (n_cols, n_cols), "glm": (n_cols + 11, 5 * n_cols), "loose": (n_cols + 3, n_cols + 1)}[kind]


def calls():
    """(regime, n_cols, stride kind, seed): every regime at every width, the stride kinds dealt round."""
    out = []
    for r, regime in enumerate(REGIMES):
        for c, n_cols in enumerate(COLS):
            out.append((regime, n_cols, STRIDES[(r + c) % 3], 100 * r + c))
    return out


def call_id(c):
    return "%s-c%d-%s" % c[:3]


def _pairs(rng, regime, m):
    if regime == "wide-se-raw":
        # every pair's se log-uniform over 1e-3 .. 1e3: a set's weights up to 12 decades apart (check_wide compares it)
        se = 10.0 ** rng.uniform(-3, 3, m)
        theta = 3.0 + rng.normal(0, 1, m)
    elif regime == "wide-se":
        # a set's centre over four decades and its own pairs over two more: the call spans 1e-3 .. 1e3, and within a set
        # w = 1/se^2 spans 1e4 at most.  (C = Sw - sum w^2 / Sw cancels by the ratio of the two largest w of a set, in the
        # reference as here: a set of two pairs six decades apart has no digits of tau^2 left in binary64 by the formula
        # itself, which is a property of the estimator and not of the code under test.)
        se = 10.0 ** (rng.uniform(-2, 2) + rng.uniform(-1, 1, m))
        theta = 3.0 + (se.min() if m else 0.0) * 5 * rng.normal(0, 1, m)
    else:
        se = rng.uniform(0.1, 0.5, m)
        theta = {"homogeneous": np.full(m, 0.5), "heterogeneous": 0.5 + rng.normal(0, 0.3, m), "offset": 1e6 + rng.normal(0, 1, m)}[regime]
    return theta + se * rng.normal(0, 1, m), se


def _spoil(rng, est, se, i):
    kind = rng.integers(0, 7)
    if kind < 3:
        est[i] = (np.nan, np.inf, -np.inf)[kind]
    else:
        se[i] = (0.0, -1.0, np.nan, np.inf)[kind - 3]


def make_call(regime, n_cols, stride_kind, seed, sizes=SIZES, sparse=True, method=R.DL, tau_squared=None):
    rng = np.random.default_rng(seed)
    sizes = list(sizes) + ([6, 6, 6] if sparse else [])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_items, (es, ss) = int(off[-1]), strides(stride_kind, n_cols)
    est, se = np.full(max(n_items, 1) * es, POISON), np.full(max(n_items, 1) * ss, POISON)
    for s, m in enumerate(sizes):
        for c in range(n_cols):
            e, v = _pairs(rng, regime, m)
            left = len(sizes) - 1 - s if sparse else 99   # the last three ranges keep k = 2, 1, 0 usable pairs
            if left < 3:
                for i in range(left, m):
                    _spoil(rng, e, v, i)
            else:
                for i in np.flatnonzero(rng.uniform(size=m) < 0.05):
                    _spoil(rng, e, v, i)
            g = np.arange(off[s], off[s + 1])
            est[g * es + c], se[g * ss + c] = e, v
    return {"regime": regime, "n_cols": n_cols, "offsets": off, "n_items": n_items, "est": est, "se": se, "est_stride": es, "se_stride": ss,
            "method": method, "tau_squared": tau_squared}


def chunk_call(n_cols, seed, m=1000, regime="heterogeneous"):
    """One set of m items: with chunk_items forced to 64 and to 100 the seams fall inside the set and at its end."""
    return make_call(regime, n_cols, "glm" if n_cols > 1 else "tight", seed, sizes=(m,), sparse=False)


def stride_loop_call(seed):
    """7 sets for max_workgroups = 2: the grid-stride loop of both paths."""
    return make_call("heterogeneous", 2, "loose", seed, sizes=(5, 70, 0, 130, 64, 3, 33), sparse=False)


_REFERENCES = {}


def reference(call, key=None):
    """(out, summary, (q - df)) of the restatement, computed once per key and never changed."""
    if key is None or key not in _REFERENCES:
        ref = R.shrink_batch(call["offsets"], call["n_cols"], call["est"], call["est_stride"], call["se"], call["se_stride"],
                             call["method"], call["tau_squared"])
        for a in ref:
            a.setflags(write=False)
        if key is None:
            return ref
        _REFERENCES[key] = ref
    return _REFERENCES[key]


def decided_by_clamp(summary, qd):
    """The sets whose Q - df is within MARGIN max(Q, df) of 0."""
    q = summary[..., 4]
    with np.errstate(invalid="ignore"):
        return (summary[..., 7] == 0) & (np.abs(qd) <= MARGIN * np.maximum(q, q - qd))


def _rel(a, b, floor):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.maximum(np.abs(b), floor)


def check(call, out, summary, ref, errs, bounds=BOUNDS):
    """Compares one call's outputs with the reference: statuses, counts and the NaN pattern exactly, the values within `bounds`
    (None: measure only).  Adds the largest error per field to `errs`; returns (sets compared, sets left out by the clamp rule)."""
    rout, rsum, qd = ref
    n_cols, off = call["n_cols"], call["offsets"]
    out, summary = np.asarray(out).reshape(rout.shape), np.asarray(summary).reshape(rsum.shape)
    assert np.array_equal(summary[..., 7], rsum[..., 7]), "status"
    assert np.array_equal(np.isnan(summary), np.isnan(rsum)), "NaN pattern of the summary"
    assert np.array_equal(np.isnan(out), np.isnan(rout)), "NaN pattern of the outputs"
    good = rsum[..., 7] == 0
    assert np.array_equal(summary[..., 5:7][good], rsum[..., 5:7][good]), "n_groups / n_input"
    failed = ~good
    assert np.all(np.isnan(summary[failed][:, :7])), "a failed set's summary is NaN"
    left_out = decided_by_clamp(rsum, qd)
    n_compared = 0
    worst = {}
    for s in range(len(off) - 1):
        g = np.arange(off[s], off[s + 1])
        for c in range(n_cols):
            if not good[s, c]:
                assert np.all(np.isnan(out[g, c])), "a failed set's outputs are NaN"
                continue
            e, v = call["est"][g * call["est_stride"] + c], call["se"][g * call["se_stride"] + c]
            ok = np.isfinite(e) & np.isfinite(v) & (v > 0)
            scale, v2 = np.max(np.abs(e[ok])), np.min(v[ok]) ** 2
            a, b = summary[s, c], rsum[s, c]
            found = {"q": _rel(a[4], b[4], 1e-12 * (b[5] - 1))}
            if left_out[s, c]:
                # the weaker property: on both sides tau^2 and I^2 are what a Q - df within the margin gives at most
                for t in (a, b):
                    assert t[3] <= 2 * MARGIN, "i_squared of a set the clamp decides"
            else:
                n_compared += 1
                found.update({"mu": _rel(a[0], b[0], 1e-12 * scale), "mu_se": _rel(a[1], b[1], 0.0),
                              "tau_squared": _rel(a[2], b[2], 1e-12 * v2), "i_squared": _rel(a[3], b[3], 1e-12),
                              "shrunken": np.max(_rel(out[g, c, 0][ok], rout[g, c, 0][ok], 1e-3 * scale)),
                              "shrunken_se": np.max(_rel(out[g, c, 1][ok], rout[g, c, 1][ok], 0.0)),
                              "weight": np.max(_rel(out[g, c, 2][ok], rout[g, c, 2][ok], 1e-12))})
            for k, x in found.items():
                worst[k] = max(worst.get(k, 0.0), float(x))
    for k, x in worst.items():
        errs[k] = max(errs.get(k, 0.0), x)
        if bounds is not None:
            assert x <= bounds[k], "%s: %.3e over the bound %.1e" % (k, x, bounds[k])
    return n_compared, int(left_out.sum())


# Bounds of check_wide: 100 x the host build's maxima over wide_calls() on the wavefront-per-set path (q 6.5e-16, i_squared 1.4e-15;
# tau_squared and mu_se divided by the set's Sw / C: 7.6e-16, 4.6e-16 — docs/PARITY.md, "eb_shrink").
WIDE_BOUNDS = {"q": 6.5e-14, "i_squared": 1.4e-13, "tau_squared/cond": 7.6e-14, "mu_se/cond": 4.6e-14}


def wide_calls():
    return [("wide-se-raw", n_cols, STRIDES[c % 3], 500 + c) for c, n_cols in enumerate(COLS)]


def check_wide(call, out, summary, ref, errs, bounds=WIDE_BOUNDS):
    """The comparison of a `wide-se-raw` call: statuses, counts and the NaN pattern exactly; q and i_squared, which do not pass
    through C, within their bounds; tau_squared and mu_se, which do, within their bound times the condition number Sw / C of
    C = Sw - sum w^2 / Sw (from the inputs, in long double).  mu and the per-pair values inherit tau_squared's conditioning
    through sums of either sign and are not compared here by value."""
    rout, rsum, qd = ref
    out, summary = np.asarray(out).reshape(rout.shape), np.asarray(summary).reshape(rsum.shape)
    assert np.array_equal(summary[..., 7], rsum[..., 7]), "status"
    assert np.array_equal(np.isnan(summary), np.isnan(rsum)), "NaN pattern of the summary"
    assert np.array_equal(np.isnan(out), np.isnan(rout)), "NaN pattern of the outputs"
    good = rsum[..., 7] == 0
    assert np.array_equal(summary[..., 5:7][good], rsum[..., 5:7][good]), "n_groups / n_input"
    left_out = decided_by_clamp(rsum, qd)
    off, n = call["offsets"], 0
    for s in range(len(off) - 1):
        g = np.arange(off[s], off[s + 1])
        for c in range(call["n_cols"]):
            if not good[s, c]:
                continue
            e, v = call["est"][g * call["est_stride"] + c], call["se"][g * call["se_stride"] + c]
            ok = np.isfinite(e) & np.isfinite(v) & (v > 0)
            w = 1 / v[ok].astype(R.LD) ** 2
            cond = float(w.sum() / (w.sum() - (w * w).sum() / w.sum()))
            a, b = summary[s, c], rsum[s, c]
            found = {"q": _rel(a[4], b[4], 1e-12 * (b[5] - 1))}
            if not left_out[s, c]:
                n += 1
                found.update({"i_squared": _rel(a[3], b[3], 1e-12), "tau_squared/cond": _rel(a[2], b[2], 1e-12 * np.min(v[ok]) ** 2) / cond,
                              "mu_se/cond": _rel(a[1], b[1], 0.0) / cond})
            for k, x in found.items():
                errs[k] = max(errs.get(k, 0.0), float(x))
                if bounds is not None:
                    assert x <= bounds[k], "%s: %.3e over the bound %.1e (Sw / C = %.1e)" % (k, x, bounds[k], cond)
    return n


def host_input(call, path=1, chunk=0):
    """The bytes tests/tools/eb_shrink_host.cpp reads: raw doubles."""
    t = call["tau_squared"]
    head = [path, chunk, call["method"], np.nan if t is None else t, len(call["offsets"]) - 1, call["n_items"], call["n_cols"],
            call["est_stride"], call["se_stride"], len(call["est"]), len(call["se"])]
    return np.concatenate([np.array(head, np.float64), call["offsets"].astype(np.float64), call["est"], call["se"]]).tobytes()
