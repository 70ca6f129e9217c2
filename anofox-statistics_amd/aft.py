"""Accelerated failure time (AFT) survival regression with right censoring on the fused Newton kernel (csrc/aft.hip): aft_fit_agg,
aft_fit_predict_agg (the fit and a score per row), the scalar aft_fit, aft_cdf / aft_quantile, and the numpy / tensor drivers of
anofox_hip_aft_fit_batch_{host,device} and anofox_hip_aft_fit_predict_batch_{host,device}.
The contract: DESIGN.md §1 "Accelerated failure time models".  Results mirror the fields of the reference's AnofoxAftFitResultCore
and AnofoxAftInference; a group whose status is not 0 is None (SQL NULL)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Any, Mapping, Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import DeviceBatch, HostBatch, call, column, group_rows
from .options import InvalidInputException, _extract_bool, _extract_double, _extract_uint32

# the names a distribution goes by (the reference's AftDistribution::from_name), case-insensitive
AFT_DIST = {"weibull": 0, "lognormal": 1, "log_normal": 1, "log-normal": 1, "loglogistic": 2, "log_logistic": 2, "log-logistic": 2,
            "exponential": 3, "exp": 3}


@dataclass
class AftOptions:
    """Resolved options of aft_fit_agg (the reference's defaults: Weibull, an intercept, 100 iterations, tolerance 1e-9, no
    inference, confidence 0.95)."""
    dist: int = 0
    fit_intercept: bool = True
    max_iterations: int = 100
    tolerance: float = 1e-9
    compute_inference: bool = False
    confidence_level: float = 0.95
    quantile: float = 0.5              # aft_fit_predict_agg: the quantile of T that time_quantile is
    horizon: Optional[float] = None    # aft_fit_predict_agg: risk = P(T <= time + horizon | T > time); None: not asked for

    def predict_options(self) -> "_abi.AnofoxHipAftPredictOptions":
        return _abi.AnofoxHipAftPredictOptions(self.quantile, float("nan") if self.horizon is None else self.horizon)

    def batch_options(self) -> "_abi.AnofoxHipAftBatchOptions":
        return _abi.AnofoxHipAftBatchOptions(self.dist, int(self.fit_intercept), self.max_iterations, self.tolerance,
                                             int(self.compute_inference), self.confidence_level)

    def ffi_options(self) -> "_abi.AnofoxAftOptions":
        return _abi.AnofoxAftOptions(self.dist, self.fit_intercept, self.max_iterations, self.tolerance, self.compute_inference,
                                     self.confidence_level, None, 0, 0)


def aft_dist_code(name) -> int:
    """The ANOFOX_AFT_* code of a distribution's name (or of a code)."""
    if isinstance(name, (int, np.integer)) and not isinstance(name, bool):
        if 0 <= int(name) <= 3:
            return int(name)
    elif str(name).lower() in AFT_DIST:
        return AFT_DIST[str(name).lower()]
    raise InvalidInputException("Unknown AFT distribution '%s'. Expected 'weibull', 'lognormal', 'loglogistic' or 'exponential'" % (name,))


def parse_aft_options(opts: Optional[Mapping[str, Any]]) -> AftOptions:
    """aft_fit_agg's MAP options: dist (a name of AFT_DIST), fit_intercept / intercept, max_iterations / max_iter, tolerance /
    tol, compute_inference, confidence_level, and for aft_fit_predict_agg quantile and horizon (checked by the library: a quantile
    outside (0, 1) or a negative or infinite horizon fails the call).  Keys are case-insensitive; other keys are ignored, except that priors fail with
    "aft: priors are not built"; every vcov is accepted (without priors they coincide).  The values are not range-checked here:
    the fit reports them (status 1 / InvalidInput)."""
    out = AftOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("dist", "distribution") and val is not None:
            out.dist = aft_dist_code(val)
        elif key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("max_iterations", "max_iter"):
            v = _extract_uint32(val)
            if v is not None:
                out.max_iterations = v
        elif key in ("tolerance", "tol"):
            v = _extract_double(val)
            if v is not None:
                out.tolerance = v
        elif key == "compute_inference":
            v = _extract_bool(val)
            if v is not None:
                out.compute_inference = v
        elif key == "confidence_level":
            v = _extract_double(val)
            if v is not None:
                out.confidence_level = v
        elif key == "quantile":
            v = _extract_double(val)
            if v is not None:
                out.quantile = v
        elif key == "horizon":
            out.horizon = _extract_double(val)
        elif key in ("priors", "prior") and val is not None:
            raise InvalidInputException("aft: priors are not built")
    return out


def _aft_fit(b, event, options, inference):
    """records[G, p + 13] and, on request, inference[G, 5 p + 2]."""
    rec = b.out((b.G, b.p + 13))
    inf = b.out((b.G, 5 * b.p + 2)) if inference else None
    b.call("anofox_hip_aft_fit_batch", *b.head, b.rows(event, "event"), options, rec, inf)
    return (rec, inf) if inference else rec


def aft_fit_batch_host(row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions, inference: bool = False,
                       ctx=None):
    """Grouped AFT fits, numpy in / out: records[G, p + 13] (and inference[G, 5 p + 2] with inference=True); the layouts are
    anofox_hip_aft_fit_batch_host's (include/anofox_stats_hip.h)."""
    if event is None:
        raise ValueError("event is needed: one 0 / 1 per row")
    return _aft_fit(HostBatch(ctx, row_offsets, time, x_cols), event, options, inference)


def aft_fit_batch_device(ctx, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions, inference: bool = False,
                         use_current_torch_stream: bool = True):
    """Grouped AFT fits on CUDA tensors (row_offsets int64[G + 1], time / x_cols[j] / event float64[N]).  Asynchronous.
    Returns records[G, p + 13], or (records, inference[G, 5 p + 2]) with inference=True."""
    if event is None:
        raise ValueError("event is needed: one 0 / 1 per row")
    return _aft_fit(DeviceBatch(ctx, row_offsets, time, x_cols, use_current_torch_stream), event, options, inference)


def _aft_fit_predict(b, event, options, predict, inference, pred_out=None):
    """(records[G, p + 13], inference[G, 5 p + 2] or None, pred[N, 4])."""
    rec = b.out((b.G, b.p + 13))
    inf = b.out((b.G, 5 * b.p + 2)) if inference else None
    pred = b.out((b.N, 4), given=pred_out)
    b.call("anofox_hip_aft_fit_predict_batch", *b.head, b.rows(event, "event"), options, predict, rec, inf, pred)
    return rec, inf, pred


def aft_fit_predict_batch_host(row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                               predict: _abi.AnofoxHipAftPredictOptions, inference: bool = False, ctx=None):
    """Grouped AFT fits and a score per row, numpy in / out: (records[G, p + 13], inference[G, 5 p + 2] or None, pred[N, 4] =
    {eta, time_quantile, cdf, risk} per row); anofox_hip_aft_fit_predict_batch_host's layouts.  A row with event = NaN is scored
    and not fitted."""
    if event is None:
        raise ValueError("event is needed: 0 / 1 per row, NaN for a row to score only")
    return _aft_fit_predict(HostBatch(ctx, row_offsets, time, x_cols), event, options, predict, inference)


def aft_fit_predict_batch_device(ctx, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                                 predict: _abi.AnofoxHipAftPredictOptions, inference: bool = False, use_current_torch_stream: bool = True,
                                 pred_out=None):
    """aft_fit_predict_batch_host on CUDA tensors.  Asynchronous.  pred_out: a float64 tensor of 4 N elements to write into; rows
    outside [row_offsets[0], row_offsets[G]) keep what it held."""
    if event is None:
        raise ValueError("event is needed: 0 / 1 per row, NaN for a row to score only")
    return _aft_fit_predict(DeviceBatch(ctx, row_offsets, time, x_cols, use_current_torch_stream), event, options, predict, inference,
                            pred_out)


def aft_test_hooks(max_blocks: int = 0):
    """For tests: the most workgroups a later AFT launch starts (0: the library's rule), so a small batch strides over its groups."""
    _abi.load().anofox_hip_aft_test_hooks(int(max_blocks))


_INFERENCE_NAMES = ("std_errors", "z_values", "p_values", "ci_lower", "ci_upper")


@dataclass
class AftFitAggResult:
    """Per group (sorted keys): the record and, with compute_inference, the inference block.  row(i) is None for a NULL group."""
    keys: np.ndarray
    records: np.ndarray               # [G, p + 13]
    inference: Optional[np.ndarray]   # [G, 5 p + 2] or None
    n_features: int

    @property
    def status(self) -> np.ndarray:
        return self.records[:, self.n_features + 12].astype(np.int64)

    def row(self, i: int) -> Optional[dict]:
        p, r = self.n_features, self.records[i]
        if int(r[p + 12]) != 0:
            return None
        d = {"coefficients": r[:p].tolist(), "intercept": float(r[p]), "scale": float(r[p + 1]), "log_likelihood": float(r[p + 2]),
             "null_log_likelihood": float(r[p + 3]), "aic": float(r[p + 4]), "bic": float(r[p + 5]), "n_observations": int(r[p + 6]),
             "n_events": int(r[p + 7]), "n_censored": int(r[p + 8]), "n_features": p, "iterations": int(r[p + 10]),
             "converged": bool(r[p + 11])}
        if self.inference is not None:
            f = self.inference[i]
            for j, name in enumerate(_INFERENCE_NAMES):
                d[name] = f[j * p:(j + 1) * p].tolist()
            d["intercept_std_error"], d["log_scale_std_error"] = float(f[5 * p]), float(f[5 * p + 1])
        return d

    def as_dict(self) -> dict:
        return {k: self.row(i) for i, k in enumerate(self.keys.tolist())}


@dataclass
class AftFitPredictAggResult(AftFitAggResult):
    """aft_fit_predict_agg: the fit per group (as AftFitAggResult) and pred[N, 4] = {eta, time_quantile, cdf, risk} per input row,
    in the input's row order; NaN where a value is not defined ("Fit-predict")."""
    pred: np.ndarray = None

    @property
    def eta(self) -> np.ndarray:
        return self.pred[:, 0]

    @property
    def time_quantile(self) -> np.ndarray:
        return self.pred[:, 1]

    @property
    def cdf(self) -> np.ndarray:
        return self.pred[:, 2]

    @property
    def risk(self) -> np.ndarray:
        return self.pred[:, 3]


def _grouped(group_keys, time, x, event):
    """The rows sorted by key (stably): -> (sorted keys, the permutation, offsets[G + 1], time, columns, event)."""
    keys = np.asarray(group_keys)
    tv, ev = column(time), column(event)
    X = np.asarray(x, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if len(keys) != len(tv) or X.shape[0] != len(tv) or len(ev) != len(tv):
        raise InvalidInputException("group keys, time, x and event must have the same number of rows")
    uniq, perm, offsets = group_rows(keys)
    cols = [np.ascontiguousarray(X[perm, j]) for j in range(X.shape[1])]
    return uniq, perm, offsets, tv[perm], cols, ev[perm]


def aft_fit_agg(group_keys, time, x, event, options=None, context=None) -> AftFitAggResult:
    """aft_fit_agg(time, x, event, options) GROUP BY group_keys: x is [N, p], event 1 = observed, 0 = right-censored; None / NaN in a
    row leaves the row out.  Options: parse_aft_options."""
    opts = parse_aft_options(options)
    uniq, perm, offsets, tv, cols, ev = _grouped(group_keys, time, x, event)
    out = aft_fit_batch_host(offsets, tv, cols, ev, opts.batch_options(), inference=opts.compute_inference, ctx=context)
    rec, inf = out if opts.compute_inference else (out, None)
    return AftFitAggResult(uniq, rec, inf, len(cols))


def aft_fit_predict_agg(group_keys, time, x, event, options=None, context=None) -> AftFitPredictAggResult:
    """aft_fit_predict_agg(time, x, event, options) GROUP BY group_keys: aft_fit_agg's fit per group and, for every input row, its
    linear predictor, the `quantile`-quantile of its time (default 0.5: the median), P(T <= time) and, with a `horizon`, the chance
    of failing within it given survival to `time`.  A row whose event (or time) is None / NaN is scored and not fitted."""
    opts = parse_aft_options(options)
    uniq, perm, offsets, tv, cols, ev = _grouped(group_keys, time, x, event)
    rec, inf, sorted_pred = aft_fit_predict_batch_host(offsets, tv, cols, ev, opts.batch_options(), opts.predict_options(),
                                                       inference=opts.compute_inference, ctx=context)
    pred = np.empty_like(sorted_pred)
    pred[perm] = sorted_pred
    return AftFitPredictAggResult(uniq, rec, inf, len(cols), pred)


def aft_fit(time, x, event, options=None) -> dict:
    """anofox_stats_aft_fit([time...], [[x1...], ...], [event...], {...}) through anofox_aft_fit (a batch of one group)."""
    from .scalar import _data_array
    o = parse_aft_options(options)
    lib = _abi.load()
    ta, k0 = _data_array(time)
    ea, k1 = _data_array(event)
    xs = (_abi.AnofoxDataArray * max(len(x), 1))()
    keep = [k0, k1]
    for j, col in enumerate(x):
        a, k = _data_array(col)
        xs[j] = a
        keep.append(k)
    core, inf = _abi.AnofoxAftFitResultCore(), _abi.AnofoxAftInference()
    try:
        call(lib, "anofox_aft_fit", ta, xs, len(x), ea, o.ffi_options(), C.byref(core), C.byref(inf) if o.compute_inference else None)
    except AnofoxStatsError as failed:
        e = InvalidInputException(f"AFT fit failed: {failed}")
        e.code = failed.code
        raise e from None
    try:
        p = core.coefficients_len
        d = {"coefficients": [core.coefficients[i] for i in range(p)], "intercept": core.intercept, "scale": core.scale,
             "log_likelihood": core.log_likelihood, "null_log_likelihood": core.null_log_likelihood, "aic": core.aic, "bic": core.bic,
             "n_observations": core.n_observations, "n_events": core.n_events, "n_censored": core.n_censored,
             "n_features": core.n_features, "iterations": core.iterations, "converged": bool(core.converged)}
        if o.compute_inference:
            for name in _INFERENCE_NAMES:
                arr = getattr(inf, name)
                d[name] = [arr[i] for i in range(inf.len)]
            d["intercept_std_error"], d["log_scale_std_error"] = inf.intercept_std_error, inf.log_scale_std_error
        return d
    finally:
        lib.anofox_free_aft_result(C.byref(core))
        lib.anofox_free_aft_inference(C.byref(inf))


def aft_cdf(t: float, eta: float, scale: float, dist="weibull") -> float:
    """P(T <= t) of a fitted AFT model at the linear predictor eta (anofox_aft_cdf); 0 for t <= 0."""
    return float(_abi.load().anofox_aft_cdf(float(t), float(eta), float(scale), aft_dist_code(dist)))


def aft_quantile(p: float, eta: float, scale: float, dist="weibull") -> float:
    """The p-quantile of T of a fitted AFT model (anofox_aft_quantile); p is clamped to [1e-12, 1 - 1e-12]."""
    return float(_abi.load().anofox_aft_quantile(float(p), float(eta), float(scale), aft_dist_code(dist)))
