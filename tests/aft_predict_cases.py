"""Cases and checks of the AFT prediction pass, shared by its CPU tier (tests/tools/aft_predict_host.cpp) and its GPU tier.

A call of tests/aft_cases.py is extended with rows to score only, appended to every group (so the training rows keep their places
in the 64-row tiles and the fit's sums keep their order): two rows with event = NaN and a time drawn like the group's, one with
event = NaN and time 0, one with event = NaN and a negative time, one with time = NaN, one with a NaN x.

`check_pred` holds the rules of DESIGN.md §1 "Fit-predict".  The three probability slots are compared with tests/aft_restate.py
evaluated at the eta and the scale the code under test returned, so the only difference left is the math library:
  cdf, risk       1e-14 + 1e-13 want   (the host bound of tests/test_aft_abi_cpu.py), on the rows with |z| <= 4 at t and t + h
  time_quantile   1e-11 want           (0.01 <= quantile <= 0.99)
  eta             2 (k + 1) 2^-53 sum_j |a_ij beta_j| against numpy's dot: the rounding of a k-term sum in any order."""
import math

import numpy as np

import aft_cases as AC
import aft_restate as R

WIDTHS = (1, 8, 9, 32)
N_EXTRA = 6
Z_MAX = 4.0


def calls():
    return [(d, p, icpt) for d in AC.DISTS for p in WIDTHS for icpt in (True, False)]


_CALLS = {}


def _extra_rows(rng, t, p):
    """N_EXTRA rows to score only, with times of the size of the group's `t`: -> (time, event, x)."""
    good = t[np.isfinite(t) & (t > 0)]
    typical = float(np.median(good)) if len(good) else 1.0
    xt = rng.uniform(-1.0, 1.0, (N_EXTRA, p))
    tt = typical * rng.uniform(0.5, 2.0, N_EXTRA)
    et = np.full(N_EXTRA, np.nan)
    tt[2], tt[3] = 0.0, -1.5
    tt[4], et[4] = np.nan, 1.0
    xt[5, rng.integers(0, p)] = np.nan
    return tt, et, xt


def small_sizes(k):
    """The GPU tier's handful of groups: rows in all (None: k + 1 training rows and none to score)."""
    return (None, 63, 64, 65, 129)


def _small_base(dist, p, icpt):
    """A call in the layout of aft_cases.make_call: one group of k + 1 rows, four whose size WITH the rows to score is 63, 64, 65
    and 129 (the 64-row tile's edges), and one group per status of aft_cases.STATUS_KINDS[:2] + all_censored."""
    rng = np.random.default_rng(4242 + 1000 * dist + 10 * p + int(icpt))
    k = AC.n_params(dist, p, icpt)
    T, E, X, kinds, extra = [], [], [], [], []
    for n in small_sizes(k):
        t, e, x = AC.draw_group(rng, dist, p, icpt, k + 1 if n is None else n - N_EXTRA, 0.3)
        e[0] = 1.0
        T.append(t), E.append(e), X.append(x), kinds.append("n%s" % n), extra.append(n is not None)
    for kind in ("bad_time", "all_censored"):
        t, e, x = AC.draw_group(rng, dist, p, icpt, k + 6, 0.3)
        if kind == "bad_time":
            t[3] = 0.0
        else:
            e[:] = 0.0
        T.append(t), E.append(e), X.append(x), kinds.append(kind), extra.append(True)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int64)
    return dict(dist=dist, p=p, icpt=icpt, k=k, offsets=offsets, time=np.concatenate(T), event=np.concatenate(E), x=np.vstack(X),
                kinds=kinds), extra


def make_call(dist, p, icpt, small=False):
    """The call of aft_cases.make_call (small: the GPU tier's handful of groups) with N_EXTRA rows to score appended to its groups.
    -> dict(base, offsets, time, event, x, train: the mask of the base call's rows)."""
    key = (dist, p, icpt, small)
    if key in _CALLS:
        return _CALLS[key]
    base, extra = _small_base(dist, p, icpt) if small else (AC.make_call(dist, p, icpt), None)
    rng = np.random.default_rng(777 + 1000 * dist + 10 * p + int(icpt))
    o = base["offsets"]
    T, E, X, M, sizes = [], [], [], [], []
    for g in range(len(o) - 1):
        t, e, x = base["time"][o[g]:o[g + 1]], base["event"][o[g]:o[g + 1]], base["x"][o[g]:o[g + 1]]
        n_extra = N_EXTRA if extra is None or extra[g] else 0
        tt, et, xt = _extra_rows(rng, t, p)
        T += [t, tt[:n_extra]]
        E += [e, et[:n_extra]]
        X += [x, xt[:n_extra]]
        M += [np.ones(len(t), bool), np.zeros(n_extra, bool)]
        sizes.append(len(t) + n_extra)
    call = dict(base=base, dist=dist, p=p, icpt=icpt, k=base["k"], kinds=base["kinds"],
                offsets=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), time=np.concatenate(T), event=np.concatenate(E),
                x=np.vstack(X), train=np.concatenate(M))
    _CALLS[key] = call
    return call


def horizon_of(call):
    """One horizon per call, of the size of the times themselves."""
    t = call["time"]
    return float(np.round(np.median(t[np.isfinite(t) & (t > 0)]), 2))


def host_input(call, quantile, horizon, tolerance=1e-9, inference=True):
    """The bytes tests/tools/aft_predict_host.cpp reads for a call (horizon None: NaN)."""
    o, p = call["offsets"], call["p"]
    wq = R.kernel_quantile(call["dist"], quantile)
    out = [float(len(o) - 1)]
    for g in range(len(o) - 1):
        n = int(o[g + 1] - o[g])
        out += [float(call["dist"]), float(call["icpt"]), 100.0, tolerance, float(inference), AC.Q975, wq,
                float("nan") if horizon is None else horizon, float(p), float(n)]
        out += np.column_stack([call["time"][o[g]:o[g + 1]], call["event"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]]]).ravel().tolist()
    return np.asarray(out, dtype=np.float64).tobytes()


def log_survival(dist, z):
    """log S_W(z): the term of a censored row."""
    return float(R.terms(dist, False, np.array([z]))[0][0])


def risk_time(dist, t, h, eta, scale):
    """P(T <= t + h | T > t) restated: -expm1 of the difference of the two log-survival terms; t <= 0: the cdf at t + h."""
    if t <= 0.0:
        return R.cdf_time(dist, t + h, eta, scale)
    return -math.expm1(log_survival(dist, (math.log(t + h) - eta) / scale) - log_survival(dist, (math.log(t) - eta) / scale))


def bytes_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


def same_values(a, b):
    """Equal as numbers, NaN where NaN (what a text round trip keeps)."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def _note(errs, name, value, bound):
    if errs is not None and bound > 0:
        errs[name] = max(errs.get(name, 0.0), value / bound)


def check_pred(pred, rec, call, g, quantile, horizon, errs=None):
    """pred[n, 4] of group g's rows against its record `rec`.  -> the number of rows whose cdf and risk met the tight bound's
    condition (|z| <= 4 at t and at t + h)."""
    p, icpt, dist = call["p"], call["icpt"], call["dist"]
    o = call["offsets"]
    t, x = call["time"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]]
    what = "%s group %d (%s)" % (AC.call_id((dist, p, icpt)), g, call["kinds"][g])
    assert pred.shape == (len(t), 4), what
    if int(rec[p + 12]) != 0:
        assert np.all(np.isnan(pred)), "%s: a failed group's rows are not all NaN" % what
        return 0
    beta, b0, scale = rec[:p], (rec[p] if icpt else 0.0), float(rec[p + 1])
    k = p + int(icpt)
    n_tight = 0
    for i in range(len(t)):
        eta, tq, cdf, risk = (float(v) for v in pred[i])
        row = "%s row %d" % (what, i)
        if not np.all(np.isfinite(x[i])):
            assert np.all(np.isnan(pred[i])), "%s: a NaN x has to give four NaN" % row
            continue
        # eta
        terms = np.concatenate([[b0] if icpt else [], x[i] * beta])
        bound = 2.0 * (k + 1) * 2.0 ** -53 * float(np.sum(np.abs(terms)))
        err = abs(eta - (float(np.dot(x[i], beta)) + b0))
        _note(errs, "eta", err, bound)
        assert err <= bound, "%s: eta off by %.3e > %.3e" % (row, err, bound)
        # time_quantile
        want = R.quantile_time(dist, quantile, eta, scale)
        _note(errs, "time_quantile", abs(tq - want), 1e-11 * want)
        assert abs(tq - want) <= 1e-11 * want, "%s: time_quantile %.17g, restated %.17g" % (row, tq, want)
        # cdf and risk
        if not np.isfinite(t[i]):
            assert math.isnan(cdf) and math.isnan(risk), "%s: a time that is not finite has to give NaN" % row
            continue
        if horizon is None:
            assert math.isnan(risk), "%s: no horizon, but a risk" % row
        if t[i] <= 0.0:
            assert cdf == 0.0, "%s: cdf at a time <= 0 is %r" % (row, cdf)
        if horizon == 0.0:
            assert risk == 0.0 and not math.copysign(1.0, risk) < 0, "%s: horizon 0 gives %r" % (row, risk)
        tight = all(abs((math.log(v) - eta) / scale) <= Z_MAX for v in (t[i], t[i] + (horizon or 0.0)) if v > 0.0)
        want = R.cdf_time(dist, t[i], eta, scale)
        assert 0.0 <= cdf <= 1.0, row
        if tight:
            n_tight += 1
            _note(errs, "cdf", abs(cdf - want), 1e-14 + 1e-13 * want)
            assert abs(cdf - want) <= 1e-14 + 1e-13 * want, "%s: cdf %.17g, restated %.17g" % (row, cdf, want)
        if horizon is not None:
            want = risk_time(dist, t[i], horizon, eta, scale)
            assert 0.0 <= risk <= 1.0, row
            if tight:
                _note(errs, "risk", abs(risk - want), 1e-14 + 1e-13 * want)
                assert abs(risk - want) <= 1e-14 + 1e-13 * want, "%s: risk %.17g, restated %.17g" % (row, risk, want)
                if dist == R.EXPONENTIAL and t[i] > 0:  # memoryless: the risk does not depend on t
                    known = -math.expm1(-horizon / math.exp(eta))
                    _note(errs, "risk_memoryless", abs(risk - known), 1e-14 + 1e-13 * known)
                    assert abs(risk - known) <= 1e-14 + 1e-13 * known, "%s: risk %.17g, memoryless %.17g" % (row, risk, known)
    return n_tight
