"""Seeded cases of the AFT tests and `check_record`, shared by the CPU tier (tests/tools/aft_host.cpp) and the GPU tier.

A call is one (dist, p, intercept): 18 groups drawn from the model itself, n in {k + 1, k + 2, 63, 64, 65, 130} x a censored share
of 0, about 30 % and about 70 %; two groups of 80 rows, 15 of them not valid (NaN / infinite entries); and one group per row-rule status.
The generator keeps the restatement inside the tests' condition (max|z| <= 8, k kappa 2^-53 <= 1e-10): features uniform on
[-1, 1], coefficients of size 0.5 / sqrt(p), an intercept in [0.5, 1.5], sigma in [0.5, 1.2], W by inversion of a uniform on
[0.01, 0.99]; a censored row's time is the event time shortened by a uniform factor.  test_aft_restate_cpu.py asserts the share."""
import math

import numpy as np

import aft_restate as R

DISTS = (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC, R.EXPONENTIAL)
WIDTHS = (1, 2, 7, 8, 9, 32)
SHARES = (0.0, 0.3, 0.7)
Q975 = 1.959963984540054  # the normal quantile of 0.975
STATUS_KINDS = ("bad_time", "bad_event", "all_censored", "no_valid_row", "too_few_rows")


def calls():
    return [(d, p, icpt) for d in DISTS for p in WIDTHS for icpt in (True, False)]


def call_id(c):
    return "%s-p%d-%s" % (R.NAMES[c[0]], c[1], "icpt" if c[2] else "noicpt")


def n_params(dist, p, icpt):
    return p + int(icpt) + int(not R.scale_is_fixed(dist))


def sizes(k):
    return (k + 1, k + 2, 63, 64, 65, 130)


def draw_group(rng, dist, p, icpt, n, share):
    """n rows from the model: -> (time, event, x[n, p])."""
    x = rng.uniform(-1.0, 1.0, (n, p))
    beta = rng.uniform(-0.5, 0.5, p) / math.sqrt(p)
    b0 = rng.uniform(0.5, 1.5) if icpt else 0.0
    sigma = 1.0 if R.scale_is_fixed(dist) else rng.uniform(0.5, 1.2)
    w = np.array([R.kernel_quantile(dist, u) for u in rng.uniform(0.01, 0.99, n)])
    t = np.exp(b0 + x @ beta + sigma * w)
    event = np.ones(n)
    cens = rng.uniform(size=n) < share
    t = np.where(cens, t * rng.uniform(0.5, 1.0, n), t)
    event[cens] = 0.0
    return t, event, x


_CALLS = {}


def make_call(dist, p, icpt):
    """-> dict(dist, p, icpt, k, offsets[G + 1], time[N], event[N], x[N, p], kinds[G]); built once per process."""
    key = (dist, p, icpt)
    if key in _CALLS:
        return _CALLS[key]
    rng = np.random.default_rng(1000 * dist + 10 * p + int(icpt) + 20240)
    k = n_params(dist, p, icpt)
    T, E, X, kinds = [], [], [], []

    def add(t, e, x, kind):
        T.append(t), E.append(e), X.append(x), kinds.append(kind)
    for n in sizes(k):
        for share in SHARES:
            add(*draw_group(rng, dist, p, icpt, n, share), "n%d-c%g" % (n, share))
    for j in range(2):  # rows that are not valid, scattered over both tiles: a NaN time, event or x, an infinite x
        t, e, x = draw_group(rng, dist, p, icpt, 80, 0.3)
        bad = rng.choice(80, 15, replace=False)
        t[bad[:5]] = np.nan
        e[bad[5:9]] = np.nan
        x[bad[9:13], rng.integers(0, p, 4)] = np.nan
        x[bad[13:], 0] = np.inf
        t[bad[0]] = -1.0 if j else np.nan   # (a NaN event hides this row's bad time: it is not "otherwise finite")
        e[bad[0]] = np.nan
        add(t, e, x, "nan_rows")
    for kind in STATUS_KINDS:
        t, e, x = draw_group(rng, dist, p, icpt, k + 6, 0.3)
        if kind == "bad_time":
            t[3] = 0.0
        elif kind == "bad_event":
            e[2] = 0.5
        elif kind == "all_censored":
            e[:] = 0.0
        elif kind == "no_valid_row":
            t[:] = np.nan
        else:
            x[k:, 0] = np.nan     # k valid rows: one fewer than k + 1
            e[0] = 1.0
        add(t, e, x, kind)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int64)
    call = dict(dist=dist, p=p, icpt=icpt, k=k, offsets=offsets, time=np.concatenate(T), event=np.concatenate(E), x=np.vstack(X),
                kinds=kinds)
    _CALLS[key] = call
    return call


_REFS = {}


def reference(call):
    """The restatement's fit of every group of a call, computed once per process and shared."""
    key = (call["dist"], call["p"], call["icpt"])
    if key not in _REFS:
        o = call["offsets"]
        _REFS[key] = [R.fit(call["dist"], call["time"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]], call["event"][o[g]:o[g + 1]], call["icpt"])
                      for g in range(len(o) - 1)]
    return _REFS[key]


EXPECTED_STATUS = {"bad_time": 1, "bad_event": 1, "all_censored": 1, "no_valid_row": 10, "too_few_rows": 6}


def compared(ref):
    """The tests' condition on a group: the restatement has it at status 0, max|z| <= 8 and k kappa 2^-53 <= 1e-10."""
    return ref["status"] == 0 and ref["max_abs_z"] <= 8.0 and ref["n_params"] * ref["kappa"] * 2.0 ** -53 <= 1e-10


def columns(call):
    return [np.ascontiguousarray(call["x"][:, j]) for j in range(call["p"])]


def host_input(call, tolerance, inference=True, max_iterations=100):
    """The bytes tests/tools/aft_host.cpp reads for a call."""
    o, p = call["offsets"], call["p"]
    out = [float(len(o) - 1)]
    for g in range(len(o) - 1):
        n = int(o[g + 1] - o[g])
        out += [float(call["dist"]), float(call["icpt"]), float(max_iterations), tolerance, float(inference), Q975, float(p), float(n)]
        rows = np.column_stack([call["time"][o[g]:o[g + 1]], call["event"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]]])
        out += rows.ravel().tolist()
    return np.asarray(out, dtype=np.float64).tobytes()


def _note(errs, name, value, bound):
    if errs is not None and bound > 0:
        errs[name] = max(errs.get(name, 0.0), value / bound)


def check_record(rec, inf, ref, call, g, tolerance, tight, errs=None):
    """The record (and, in the tight run, the inference) of group g against the restatement's fit `ref`.  -> 1 when the group is
    one of the compared ones, else 0 (then only the status rules are checked).  errs: name -> the largest error seen, in units
    of its bound."""
    p, icpt, dist, k = call["p"], call["icpt"], call["dist"], call["k"]
    kind, what = call["kinds"][g], "%s group %d (%s)" % (call_id((dist, p, icpt)), g, call["kinds"][g])
    status = int(rec[p + 12])
    if kind in EXPECTED_STATUS:
        assert ref["status"] == EXPECTED_STATUS[kind], what
    if ref["status"] in (1, 6, 10):
        assert status == ref["status"], "%s: status %d, the row rules say %d" % (what, status, ref["status"])
    if status != 0:
        assert np.all(np.isnan(rec[:p + 12])), what
        assert inf is None or np.all(np.isnan(inf)), what
    if not compared(ref):
        return 0
    assert status == 0, "%s: status %d on a group inside the tests' condition" % (what, status)
    o = call["offsets"]
    t, e, x = call["time"][o[g]:o[g + 1]], call["event"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]]
    ic, fs = int(icpt), int(not R.scale_is_fixed(dist))
    kb = p + ic
    theta = np.concatenate([[rec[p]] if ic else [], rec[:p], [math.log(rec[p + 1])] if fs else []])
    ll, lls = float(rec[p + 2]), ref["ll"]
    # 1 the certificate: the stopping rule recomputed by the restatement at the returned theta
    l_at, g_at, info_at = R.evaluate(dist, t, x, e, icpt, theta)
    dec = 0.5 * float(g_at @ np.linalg.solve(info_at, g_at))
    bound = 2.0 * tolerance * (1.0 + abs(ll))
    _note(errs, "certificate", dec, bound)
    assert dec <= bound, "%s: certificate %.3e > %.3e" % (what, dec, bound)
    # 2 the log-likelihood
    floor = 1e-13 * ref["n_obs"] * (1.0 + ref["max_abs_logt"])
    gap = lls - ll
    _note(errs, "ll_gap", max(gap, 0.0), 2.0 * tolerance * (1.0 + abs(lls)) + floor)
    _note(errs, "ll_above", max(-gap, 0.0), floor)
    assert -floor <= gap <= 2.0 * tolerance * (1.0 + abs(lls)) + floor, "%s: l* - l = %.3e" % (what, gap)
    # 3 the parameters
    tb = ref["se"] * math.sqrt(4.0 * tolerance * (1.0 + abs(lls))) + 1e-12 * np.maximum(1.0, np.abs(ref["theta"]))
    terr = np.abs(theta - ref["theta"])
    _note(errs, "theta", float(np.max(terr / tb)), 1.0)
    assert np.all(terr <= tb), "%s: theta off by %.3g x its bound" % (what, float(np.max(terr / tb)))
    # 4 the other record fields
    assert (rec[p + 6], rec[p + 7], rec[p + 8], rec[p + 9]) == (ref["n_obs"], ref["n_events"], ref["n_censored"], k), what
    assert rec[p + 11] == 1.0 and 1 <= rec[p + 10] <= 100, what
    assert (np.isnan(rec[p]) if not ic else np.isfinite(rec[p])), what
    assert rec[p + 1] == 1.0 if not fs else rec[p + 1] > 0.0, what
    aic, bic = 2.0 * k - 2.0 * ll, k * math.log(ref["n_obs"]) - 2.0 * ll
    assert abs(rec[p + 4] - aic) <= 1e-12 * abs(aic) and abs(rec[p + 5] - bic) <= 1e-12 * abs(bic), what
    if not ic:
        assert np.isnan(rec[p + 3]), what
    elif np.isfinite(ref["null_ll"]):
        ngap = ref["null_ll"] - rec[p + 3]
        assert -floor <= ngap <= 2.0 * tolerance * (1.0 + abs(ref["null_ll"])) + floor, "%s: null l* - l = %.3e" % (what, ngap)
    # 5 the inference
    if tight and inf is not None:
        se = np.concatenate([[inf[5 * p]] if ic else [], inf[:p], [inf[5 * p + 1]] if fs else []])
        serr = np.abs(se / ref["se"] - 1.0)
        _note(errs, "se", float(np.max(serr)), 1e-6)
        assert np.all(serr <= 1e-6), "%s: standard errors off by %.3e" % (what, float(np.max(serr)))
        assert (np.isnan(inf[5 * p]) if not ic else True) and (np.isnan(inf[5 * p + 1]) if not fs else True), what
        b, sf, z = rec[:p], inf[:p], inf[p:2 * p]
        assert np.all(np.abs(z - b / sf) <= 1e-12 * np.abs(b / sf)), what
        assert np.all(np.abs(inf[3 * p:4 * p] - (b - Q975 * sf)) <= 1e-9 * np.maximum(1.0, np.abs(b) + Q975 * sf)), what
        assert np.all(np.abs(inf[4 * p:5 * p] - (b + Q975 * sf)) <= 1e-9 * np.maximum(1.0, np.abs(b) + Q975 * sf)), what
        from scipy.special import erfc
        pref = erfc(np.abs(ref["coef"] / ref["se"][ic:kb]) / math.sqrt(2.0))
        assert np.allclose(inf[2 * p:3 * p], pref, rtol=1e-6, atol=1e-14), what
    return 1
