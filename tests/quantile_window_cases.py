"""The cases and the assertions of the quantile regression window function's tests (tests/test_quantile_window_cpu.py on the
host build of csrc/quantile_solve.h::qs_fit_window, tests/test_gpu_quantile_window.py on the MI355X).  A plain module: the
reference of every frame comes from tests/quantile_restate.py::solve and is cached, so the CPU and the GPU tests of one
process share one solve per frame; arrays are read-only.

What a frame's record has to meet (check_frame):
  status, the NaN pattern, n_observations, tau and the sign of the pivot count exactly (the row rules of the fit-predict
  aggregate on the frame's rows; rule count = the frame's rows whose y is not NaN);
  the loss against the restatement's within the tolerance of test_quantile_cpu.check_record, which is called, not restated;
  the k x k certificate optimal wherever it is decided, rank and aliased slots (quantile_fuzz_cases.check_sweep_record);
  coefficients within quantile_fuzz_cases.COEF_TOL in column units, and yhat within what those coefficient tolerances allow
  on the prediction row, only where quantile_fuzz_cases.in_comparison(ref) holds."""
import functools

import numpy as np

import quantile_fuzz_cases as qf
import quantile_restate as qr
from test_quantile_cpu import check_record

UNBOUNDED = None


def rows_frames(off, start, end):
    """ROWS BETWEEN start PRECEDING AND end PRECEDING per row, clipped to the partition (None: UNBOUNDED); an empty frame is
    (r, r).  -> (lo, hi) int64."""
    n = int(off[-1])
    lo, hi = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    for g in range(len(off) - 1):
        plo, phi = int(off[g]), int(off[g + 1])
        for r in range(plo, phi):
            first = plo if start is None else max(r - start, plo)
            last = phi - 1 if end is None else min(r - end, phi - 1)
            lo[r], hi[r] = (r, r) if last < first else (first, last + 1)
    return lo, hi


def window_text(X, y, lo, hi, tau, icpt, run_length=0, max_it=1000):
    """One case of tests/tools/quantile_window_host.cpp."""
    n, p = X.shape
    lines = [f"{p} {int(icpt)} {tau!r} {n} {max_it} {run_length}"]
    lines += [" ".join([str(int(lo[i])), str(int(hi[i]))] + [repr(float(v)) for v in (y[i], *X[i])]) for i in range(n)]
    return "\n".join(lines) + "\n"


def parse_window_output(text, jobs):
    """-> per job dict(rec[n, p+6], its[n], cold[n], restarts (summed over the runs), yhat[n], cold_rec[n, p+6], cold_its[n])."""
    lines = text.strip().split("\n") if text.strip() else []
    out, at = [], 0
    for X, *_ in jobs:
        n, p = X.shape
        v = np.array([[float(t) for t in ln.split()] for ln in lines[at:at + n]]).reshape(n, 2 * (p + 6) + 4)
        at += n
        flag = v[:, p + 7].astype(np.int64)                # bit 0: began afresh; the rest: the run's restarts, on its first row
        out.append(dict(rec=v[:, :p + 6], its=v[:, p + 6].astype(np.int64), cold=flag & 1, restarts=int((flag >> 1).sum()), yhat=v[:, p + 8],
                        cold_rec=v[:, p + 9:2 * p + 15], cold_its=v[:, 2 * p + 15].astype(np.int64)))
    assert at == len(lines)
    return out


# ---- data ------------------------------------------------------------------------------------------------------------------
KINDS_A = ("plain", "invalid", "duplicates", "constant", "aliased", "lattice")
A_SEED, A_P, A_N, A_FRAME, A_TAU = 2, 3, 48, 14, 0.5


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def kinds_case(seed=A_SEED, p=A_P, n=A_N, icpt=True):
    """One partition of n rows per data kind of quantile_fuzz_cases._rows (the first group of each kind of one call of 60
    groups).  -> (off, y, X, kinds)."""
    rng = np.random.default_rng([20261018, 7, seed])
    off0, y0, X0, kinds0, _ = qf._rows(rng, p, icpt, np.full(60, n, dtype=np.int64), False)
    ys, Xs = [], []
    for kind in KINDS_A:
        g = kinds0.index(kind)
        ys.append(y0[off0[g]:off0[g + 1]])
        Xs.append(X0[off0[g]:off0[g + 1]])
    off = np.arange(len(KINDS_A) + 1, dtype=np.int64) * n
    y, X = np.concatenate(ys), np.concatenate(Xs)
    _freeze(off, y, X)
    return off, y, X, KINDS_A


@functools.lru_cache(maxsize=None)
def small_partition(seed=0, n=40, p=2):
    """The partition of the frame-shape tests: continuous, one row with a NaN y and one with an infinite x."""
    rng = np.random.default_rng([20261018, 8, seed])
    X = rng.normal(size=(n, p)) * [1.0, 3.0][:p] + [0.0, 2.0][:p]
    y = 1.5 + X @ np.array([2.0, -1.0])[:p] + rng.standard_t(3, size=n)
    y[11] = np.nan
    X[23, p - 1] = np.inf
    _freeze(X, y)
    return X, y


_REFS = {}


def frame_ref(X, y, lo, hi, tau, icpt):
    """The restatement's solve of the frame's rows, None where the row rules refuse it; cached per (array, frame, tau)."""
    key = (id(X), id(y), int(lo), int(hi), float(tau), bool(icpt))
    if key not in _REFS:
        Xf, yf = X[lo:hi], y[lo:hi]
        rule = int(np.sum(~np.isnan(yf)))
        ok = hi > lo and qr.rule_status(Xf, yf, tau, icpt, rule) == 0
        _REFS[key] = (X, y, qr.solve(Xf, yf, tau, icpt) if ok else None)     # (the arrays are kept alive: their ids are the key)
    return _REFS[key][2]


def check_frame(X, y, lo, hi, tau, icpt, rec, its, yhat, kind, what, tally=None):
    """The assertions on one output row (module docstring); -> whether the coefficients were compared."""
    p = X.shape[1]
    if hi <= lo:
        assert rec[p + 5] == qr.STATUS_TOO_FEW_ROWS and np.isnan(rec[:p + 5]).all() and its == 0 and np.isnan(yhat), what
        return False
    Xf, yf = X[lo:hi], y[lo:hi]
    rule = int(np.sum(~np.isnan(yf)))
    ref = frame_ref(X, y, lo, hi, tau, icpt)
    ratio = qf.check_sweep_record(ref, rec, its, Xf, yf, tau, icpt, kind, what, rule_count=rule)
    if tally is not None:
        tally.add(kind, ref, ratio)
    if ref is None:
        assert np.isnan(yhat), what
        return False
    ok = qr.valid_rows(Xf, yf)
    if ok.sum() >= 2:                          # check_record's own rule reads the row count of what it is given
        c = dict(name=what, X=Xf[ok], y=yf[ok], tau=tau, fit_intercept=icpt, loss=ref["loss"], unique=False, b=ref["b"], b0=ref["b0"])
        check_record(c, rec, its, what)
    q = hi - 1
    if not np.isfinite(X[q]).all():
        assert np.isnan(yhat), what
        return ratio is not None
    a = np.concatenate([[1.0], X[q]]) if icpt else X[q]
    beta = np.concatenate([[rec[p]], rec[:p]]) if icpt else rec[:p]
    mine = float(a @ beta)
    assert abs(yhat - mine) <= 2 * (len(a) + 1) * 2.0 ** -53 * float(np.abs(a) @ np.abs(beta)) + 1e-300, f"{what}: yhat {yhat!r} vs {mine!r}"
    if ratio is not None:                      # inside the comparison: yhat within what the coefficient tolerances allow on row q
        s = qf.column_units(Xf, yf, icpt)
        s = np.concatenate([[s[-1]], s[:-1]]) if icpt else s
        want = np.concatenate([[ref["b0"]], ref["b"]]) if icpt else ref["b"]
        tol = qf.COEF_TOL * float(np.max(np.abs(want) * s)) * float(np.sum(np.abs(a) / s))
        assert abs(yhat - float(a @ want)) <= tol + 2 * (len(a) + 1) * 2.0 ** -53 * float(np.abs(a) @ np.abs(want)), f"{what}: yhat off"
    return ratio is not None


def check_partition(X, y, lo, hi, tau, icpt, rec, its, yhat, kind, what, rows=None, tally=None):
    compared = 0
    for e in (range(len(y)) if rows is None else rows):
        compared += check_frame(X, y, int(lo[e]), int(hi[e]), tau, icpt, rec[e], int(its[e]), float(yhat[e]), kind, f"{what} row {e}", tally)
    return compared


def frame_losses(rec, p):
    return rec[:, p + 2]
