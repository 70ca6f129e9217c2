"""Generalised linear models on the fused IRLS kernel (csrc/glm.hip): poisson_fit_agg, binomial_fit_agg, logistic_fit_agg,
poisson_fit_predict_agg, the scalar poisson_fit / logistic_fit, and the numpy drivers of anofox_hip_glm_fit_batch_host /
anofox_hip_glm_fit_predict_batch_host and of their interval / accuracy forms; and the window functions poisson_fit_predict /
logistic_fit_predict / binomial_fit_predict with the drivers of anofox_hip_glm_fit_predict_{window,frames}_* (csrc/glm_window.hip).
The contract: DESIGN.md §1 "Generalised linear models".  Results mirror the fields of the reference's AnofoxGlmFitResultCore; a group whose status is not 0 is None (SQL NULL)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import I64, DeviceBatch, HostBatch, call, group_rows, handle, host_array
from .options import GlmOptions, InvalidInputException, parse_binomial_options, parse_poisson_options

def _glm_fit(b, options, offset, inference, threshold):
    """records[G, p + 11], inference[G, 5 p] on request and, with a threshold (binomial, the accuracy entry), accuracy[G]."""
    rec = b.out((b.G, b.p + 11))
    inf = b.out((b.G, 5 * b.p)) if inference else None
    head = (*b.head, b.rows(offset, "offset"), options)
    if threshold is None:
        b.call("anofox_hip_glm_fit_batch", *head, rec, inf)
    else:
        acc = b.out((b.G,))
        b.call("anofox_hip_glm_fit_accuracy_batch", *head, float(threshold), rec, inf, acc)
    res = (rec, inf) if inference else (rec,)
    if threshold is not None:
        res += (acc,)
    return res if len(res) > 1 else rec


def _glm_fit_predict(b, options, offset, train_counts, interval_z):
    """(core[G, p + 11], pred[N, 3]); with interval_z through the interval entry."""
    core, pred = b.out((b.G, b.p + 11)), b.out((b.N, 3))
    head = (*b.head, b.rows(offset, "offset"), b.groups(train_counts, "train_counts"), options)
    if interval_z is None:
        b.call("anofox_hip_glm_fit_predict_batch", *head, core, pred)
    else:
        b.call("anofox_hip_glm_fit_predict_interval_batch", *head, float(interval_z), core, pred)
    return core, pred


def glm_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None, inference: bool = False,
                       ctx=None, threshold=None):
    """Grouped GLM fits, numpy in / out: records[G, p + 11] (and inference[G, 5 p] with inference=True); the layouts are
    anofox_hip_glm_fit_batch_host's (include/anofox_stats_hip.h).  With a threshold (binomial) the call goes through
    anofox_hip_glm_fit_accuracy_batch_host and accuracy[G] is appended to what is returned."""
    return _glm_fit(HostBatch(ctx, row_offsets, y, x_cols), options, offset, inference, threshold)


def glm_fit_accuracy_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, threshold: float = 0.5,
                                offset=None, inference: bool = False, ctx=None):
    """anofox_hip_glm_fit_accuracy_batch_host: (records, [inference,] accuracy[G]); binomial family only."""
    return glm_fit_batch_host(row_offsets, y, x_cols, options, offset, inference, ctx, threshold=threshold)


def glm_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None, train_counts=None,
                               ctx=None, interval_z=None):
    """GLM fit + predict, numpy in / out: (core[G, p + 11], pred[N, 3] = mu, NaN, NaN; a NaN mu = NULL).  With interval_z the
    call goes through anofox_hip_glm_fit_predict_interval_batch_host: pred = mu, lower, upper for interval_z > 0 (Poisson)."""
    return _glm_fit_predict(HostBatch(ctx, row_offsets, y, x_cols), options, offset, train_counts, interval_z)


def glm_fit_predict_interval_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, interval_z: float,
                                        offset=None, train_counts=None, ctx=None):
    """anofox_hip_glm_fit_predict_interval_batch_host: (core[G, p + 11], pred[N, 3] = mu, lower, upper)."""
    return glm_fit_predict_batch_host(row_offsets, y, x_cols, options, offset, train_counts, ctx, interval_z=interval_z)


def glm_fit_batch_device(ctx, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                         inference: bool = False, use_current_torch_stream: bool = True, threshold=None):
    """Grouped GLM fits on CUDA tensors (row_offsets int64[G + 1], y / x_cols[j] / offset float64[N]).  Asynchronous.
    Returns records[G, p + 11], or (records, inference[G, 5 p]) with inference=True; with a threshold (binomial, through
    anofox_hip_glm_fit_accuracy_batch_device) accuracy[G] is appended."""
    return _glm_fit(DeviceBatch(ctx, row_offsets, y, x_cols, use_current_torch_stream), options, offset, inference, threshold)


def glm_fit_predict_batch_device(ctx, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                                 train_counts=None, use_current_torch_stream: bool = True, interval_z=None):
    """GLM fit + predict on CUDA tensors (inputs as glm_fit_batch_device; train_counts int64[G] or None).  Asynchronous.
    Returns (core[G, p + 11], pred[N, 3]); rows outside [row_offsets[0], row_offsets[G]) are not written.  With interval_z the
    call goes through anofox_hip_glm_fit_predict_interval_batch_device."""
    return _glm_fit_predict(DeviceBatch(ctx, row_offsets, y, x_cols, use_current_torch_stream), options, offset, train_counts, interval_z)


def _glm_window(b, options, offset, interval_z, want_records, frame=None, bounds=None):
    """pred[N, 3] (and records[N, p + 11] with want_records) of the window function: ROWS frames (`frame`) or explicit `bounds`."""
    from .runtime import _frame
    pred = b.out((b.N, 3))
    rec = b.out((b.N, b.p + 11)) if want_records else None
    z = 0.0 if interval_z is None else float(interval_z)
    if bounds is None:
        b.call("anofox_hip_glm_fit_predict_window", *b.head, b.rows(offset, "offset"), _frame(frame), options, z, pred, rec)
    else:
        b.call("anofox_hip_glm_fit_predict_frames", *b.rows_head, b.rows(offset, "offset"), *b.frames(*bounds), options, z, pred, rec)
    return (pred, rec) if want_records else pred


def glm_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, frame=(None, 0), offset=None,
                                interval_z=None, want_records: bool = False, ctx=None):
    """The GLM window function over ROWS frames, numpy in / out: pred[N, 3] = (mu, lower, upper) at the frame's last row per
    output row (a NaN mu = NULL), or (pred, records[N, p + 11]) with want_records.  frame = (start, end) in rows PRECEDING the
    current row (negative = FOLLOWING; None = UNBOUNDED)."""
    return _glm_window(HostBatch(ctx, row_offsets, y, x_cols), options, offset, interval_z, want_records, frame=frame)


def glm_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                                interval_z=None, want_records: bool = False, ctx=None):
    """The GLM window function over explicit frames [frame_lo[e], frame_hi[e]) of any shape (hi <= lo: an empty frame)."""
    return _glm_window(HostBatch(ctx, None, y, x_cols), options, offset, interval_z, want_records, bounds=(frame_lo, frame_hi))


def glm_fit_predict_window_device(ctx, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, frame=(None, 0),
                                  offset=None, interval_z=None, want_records: bool = False, use_current_torch_stream: bool = True):
    """glm_fit_predict_window_host on CUDA tensors.  The offsets are copied to the host for the planner (one synchronising copy);
    the walk itself is asynchronous."""
    return _glm_window(DeviceBatch(ctx, row_offsets, y, x_cols, use_current_torch_stream), options, offset, interval_z, want_records,
                       frame=frame)


def glm_fit_predict_frames_device(ctx, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                                  interval_z=None, want_records: bool = False, use_current_torch_stream: bool = True):
    """glm_fit_predict_frames_host on CUDA tensors (frame_lo / frame_hi int64[N])."""
    return _glm_window(DeviceBatch(ctx, None, y, x_cols, use_current_torch_stream), options, offset, interval_z, want_records,
                       bounds=(frame_lo, frame_hi))


def glm_window_plan(row_offsets, frame_lo, frame_hi):
    """The planner of the GLM window function alone (host arrays, no device), under the test hooks in force: -> (run_begin
    int64[walkers + 1], scratch rows per wavefront = the longest frame, launched wavefronts)."""
    off = host_array(row_offsets, I64, None, "row_offsets")
    lo = host_array(frame_lo, I64, None, "frame_lo")
    hi = host_array(frame_hi, I64, lo.size, "frame_hi")
    runs = np.empty(lo.size + 2, dtype=np.int64)
    n_runs, span, waves = C.c_int64(), C.c_int64(), C.c_int64()
    call(_abi.load(), "anofox_hip_glm_window_plan", off.size - 1, off, lo.size, lo, hi, runs, runs.size, C.byref(n_runs), C.byref(span),
         C.byref(waves))
    return runs[:n_runs.value + 1].copy(), int(span.value), int(waves.value)


def glm_window_test_hooks(run_length: int = 0, scratch_cap_bytes: int = 0, warm: bool = True):
    """For tests and measurements: the run length and the scratch cap of every later GLM window call (0: the library's rule), and
    whether a frame may start from its predecessor's coefficients (False: every frame starts cold)."""
    _abi.load().anofox_hip_glm_window_test_hooks(int(run_length), int(scratch_cap_bytes), 1 if warm else 0)


def glm_window_stats(ctx=None):
    """The most recent GLM window call on the context: dict(frames, cold_starts, warm_starts, refits (warm frames fitted again
    cold), iterations (IRLS iterations summed over the frames), walkers, waves, span_rows)."""
    out = (C.c_int64 * 8)()
    call(_abi.load(), "anofox_hip_glm_window_stats", handle(ctx), out)
    return dict(zip(("frames", "cold_starts", "warm_starts", "refits", "iterations", "walkers", "waves", "span_rows"), (int(v) for v in out)))


@dataclass
class GlmFitPredictResult:
    """The window functions' result: pred[N, 3] = (mu, yhat_lower, yhat_upper) in the order of the input rows (NaN = NULL)."""
    pred: np.ndarray

    @property
    def yhat(self) -> np.ndarray:
        return self.pred[:, 0]


def _fit_predict(partition_keys, order, y, x, opts: GlmOptions, options, frame, context) -> GlmFitPredictResult:
    from .aggregate import _parse_frame
    start, end = _parse_frame(frame, 0)
    keys = np.asarray(partition_keys)
    yv = np.array([np.nan if v is None else v for v in y], dtype=np.float64) if np.asarray(y).dtype == object else np.asarray(y, np.float64)
    X = np.asarray(x, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if len(keys) != len(yv) or X.shape[0] != len(yv) or len(np.asarray(order)) != len(yv):
        raise InvalidInputException("partition keys, order, y and x must have the same number of rows")
    if opts.offset < 0 or opts.offset > X.shape[1]:
        raise InvalidInputException("offset must be a 1-based index into x (1..=%d), got %d" % (X.shape[1], opts.offset))
    ukeys, gid = np.unique(keys, return_inverse=True)
    perm = np.lexsort((np.asarray(order), gid))
    offsets = np.concatenate([[0], np.cumsum(np.bincount(gid, minlength=len(ukeys)))]).astype(np.int64)
    cols = [np.ascontiguousarray(X[perm, j]) for j in range(X.shape[1]) if j != opts.offset - 1]
    off = np.ascontiguousarray(X[perm, opts.offset - 1]) if opts.offset else None
    z = interval_z(opts.confidence_level) if bool(_option(options, ("interval",), False)) else None
    pred_sorted = glm_fit_predict_window_host(offsets, yv[perm], cols, opts.batch_options(), (start, end), offset=off, interval_z=z,
                                              ctx=context)
    pred = np.empty_like(pred_sorted)
    pred[perm] = pred_sorted
    return GlmFitPredictResult(pred)


def poisson_fit_predict(partition_keys, order, y, x, options=None, frame=(None, 0), context=None) -> GlmFitPredictResult:
    """poisson_fit_predict(y, x [, options]) OVER (PARTITION BY partition_keys ORDER BY order ROWS frame): the Poisson fit of every
    row's frame, predicting at the x (and offset) of the frame's last row.  Options as poisson_fit_predict_agg (offset, interval /
    confidence_level, lambda, tolerance, max_iterations, fit_intercept); frame = (start, end) as ols_fit_predict's.  result.pred
    is [n_rows, 3] in input row order; the bounds are NaN without options['interval']."""
    return _fit_predict(partition_keys, order, y, x, parse_poisson_options(options), options, frame, context)


def binomial_fit_predict(partition_keys, order, y, x, options=None, frame=(None, 0), context=None) -> GlmFitPredictResult:
    """The binomial / logit window function; an interval is not built for this family (the library refuses it)."""
    return _fit_predict(partition_keys, order, y, x, parse_binomial_options(options), options, frame, context)


def logistic_fit_predict(partition_keys, order, y, x, options=None, frame=(None, 0), context=None) -> GlmFitPredictResult:
    """binomial_fit_predict under the reference's name for a 0 / 1 response: rolling logistic scores."""
    return binomial_fit_predict(partition_keys, order, y, x, options, frame, context)


@dataclass
class GlmFitAggResult:
    """Per group (sorted keys): the record and, with compute_inference, the inference block.  row(i) is None for a NULL group."""
    keys: np.ndarray
    records: np.ndarray               # [G, p + 11]
    inference: Optional[np.ndarray]   # [G, 5 p] or None
    n_features: int
    pred: Optional[np.ndarray] = None         # fit-predict: [N, 3] in the order of the input rows
    row_group: Optional[np.ndarray] = None
    accuracy: Optional[np.ndarray] = None     # logistic_fit_agg: [G], NaN for a NULL group
    threshold: Optional[float] = None

    @property
    def status(self) -> np.ndarray:
        return self.records[:, self.n_features + 10].astype(np.int64)

    def row(self, i: int) -> Optional[dict]:
        p, r = self.n_features, self.records[i]
        if int(r[p + 10]) != 0:
            return None
        d = {"coefficients": r[:p].tolist(), "intercept": float(r[p]), "deviance": float(r[p + 1]), "null_deviance": float(r[p + 2]),
             "pseudo_r_squared": float(r[p + 3]), "aic": float(r[p + 4]), "dispersion": float(r[p + 5]),
             "n_observations": int(r[p + 6]), "n_features": p, "iterations": int(r[p + 8]), "converged": bool(r[p + 9])}
        if self.inference is not None:
            f = self.inference[i]
            for j, name in enumerate(("std_errors", "z_values", "p_values", "ci_lower", "ci_upper")):
                d[name] = f[j * p:(j + 1) * p].tolist()
        if self.accuracy is not None:
            d["accuracy"], d["threshold"] = float(self.accuracy[i]), self.threshold
        return d

    def as_dict(self) -> dict:
        return {k: self.row(i) for i, k in enumerate(self.keys.tolist())}


def _grouped(group_keys, y, x, opts: GlmOptions):
    keys = np.asarray(group_keys)
    yv = np.array([np.nan if v is None else v for v in y], dtype=np.float64) if np.asarray(y).dtype == object else np.asarray(y, np.float64)
    X = np.asarray(x, dtype=np.float64)
    if X.ndim == 1:
        X = X[:, None]
    if len(keys) != len(yv) or X.shape[0] != len(yv):
        raise InvalidInputException("group keys, y and x must have the same number of rows")
    if opts.offset < 0 or opts.offset > X.shape[1]:
        raise InvalidInputException("offset must be a 1-based index into x (1..=%d), got %d" % (X.shape[1], opts.offset))
    uniq, perm, offsets = group_rows(keys)
    feat = [j for j in range(X.shape[1]) if j != opts.offset - 1]
    cols = [np.ascontiguousarray(X[perm, j]) for j in feat]
    off = np.ascontiguousarray(X[perm, opts.offset - 1]) if opts.offset else None
    return uniq, np.searchsorted(uniq, keys), perm, offsets, yv[perm], cols, off


def _fit_agg(group_keys, y, x, opts: GlmOptions, context) -> GlmFitAggResult:
    uniq, _, _, offsets, ys, cols, off = _grouped(group_keys, y, x, opts)
    out = glm_fit_batch_host(offsets, ys, cols, opts.batch_options(), offset=off, inference=opts.compute_inference, ctx=context)
    rec, inf = out if opts.compute_inference else (out, None)
    return GlmFitAggResult(uniq, rec, inf, len(cols))


def poisson_fit_agg(group_keys, y, x, options=None, context=None) -> GlmFitAggResult:
    """poisson_fit_agg(y, x, options) GROUP BY group_keys: x is [N, p] (with options['offset'] = j, column j is the offset)."""
    return _fit_agg(group_keys, y, x, parse_poisson_options(options), context)


def binomial_fit_agg(group_keys, y, x, options=None, context=None) -> GlmFitAggResult:
    return _fit_agg(group_keys, y, x, parse_binomial_options(options), context)


def _option(options, names, default):
    for k, v in (options or {}).items():
        if str(k).lower() in names and v is not None:
            return v
    return default


def interval_z(confidence_level: float) -> float:
    """The reference's GetTCritical table: 0.95 -> 1.96, 0.99 -> 2.576, 0.90 -> 1.645 (each within 0.001), anything else 1.96."""
    for level, z in ((0.95, 1.96), (0.99, 2.576), (0.90, 1.645)):
        if abs(confidence_level - level) < 0.001:
            return z
    return 1.96


def logistic_fit_agg(group_keys, y, x, options=None, context=None) -> GlmFitAggResult:
    """The logit fit of binomial_fit_agg plus, per group, the training accuracy at options['threshold'] (default 0.5), counted by
    the wavefront that fitted the group (anofox_hip_glm_fit_accuracy_batch_host)."""
    opts = parse_binomial_options(options)
    thr = float(_option(options, ("threshold",), 0.5))
    uniq, _, _, offsets, ys, cols, off = _grouped(group_keys, y, x, opts)
    out = glm_fit_batch_host(offsets, ys, cols, opts.batch_options(), offset=off, inference=opts.compute_inference, ctx=context, threshold=thr)
    rec, inf, acc = out if opts.compute_inference else (out[0], None, out[1])
    return GlmFitAggResult(uniq, rec, inf, len(cols), accuracy=acc, threshold=thr)


def poisson_fit_predict_agg(group_keys, y, x, options=None, context=None) -> GlmFitAggResult:
    """poisson_fit_predict_agg: the fit on each group's rows with a y (None / NaN = a row to predict only), then mu for every row.
    result.pred[i] = (mu, NaN, NaN) of input row i; with options['interval'] = True it is (mu, yhat_lower, yhat_upper), the
    reference's interval at interval_z(confidence_level)."""
    opts = parse_poisson_options(options)
    z = interval_z(opts.confidence_level) if bool(_option(options, ("interval",), False)) else None
    uniq, inv, perm, offsets, ys, cols, off = _grouped(group_keys, y, x, opts)
    train = np.add.reduceat(np.isfinite(ys).astype(np.int64), offsets[:-1]) if len(ys) else np.zeros(len(uniq), np.int64)
    train = np.where(np.diff(offsets) > 0, train, 0)
    core, pred_sorted = glm_fit_predict_batch_host(offsets, ys, cols, opts.batch_options(), offset=off, train_counts=train, ctx=context,
                                                   interval_z=z)
    pred = np.empty_like(pred_sorted)
    pred[perm] = pred_sorted
    return GlmFitAggResult(uniq, core, None, len(cols), pred=pred, row_group=inv)


def _scalar(fn_name, opt_struct, y, x, extras=False):
    from .scalar import _data_array
    lib = _abi.load()
    ya, k0 = _data_array(y)
    xs = (_abi.AnofoxDataArray * max(len(x), 1))()
    keep = [k0]
    for j, col in enumerate(x):
        a, k = _data_array(col)
        xs[j] = a
        keep.append(k)
    core, inf, ex = _abi.AnofoxGlmFitResultCore(), _abi.AnofoxFitResultInference(), _abi.AnofoxLogisticFitExtras()
    args = [ya, xs, len(x), opt_struct, C.byref(core), C.byref(inf) if opt_struct.compute_inference else None]
    if extras:
        args.append(C.byref(ex))
    try:
        call(lib, fn_name, *args)
    except AnofoxStatsError as failed:
        e = InvalidInputException(f"GLM fit failed: {failed}")
        e.code = failed.code
        raise e from None
    try:
        p = core.coefficients_len
        d = {"coefficients": [core.coefficients[i] for i in range(p)], "intercept": core.intercept, "deviance": core.deviance,
             "null_deviance": core.null_deviance, "pseudo_r_squared": core.pseudo_r_squared, "aic": core.aic,
             "dispersion": core.dispersion, "n_observations": core.n_observations, "n_features": core.n_features,
             "iterations": core.iterations, "converged": bool(core.converged)}
        if opt_struct.compute_inference:
            for name, arr in (("std_errors", inf.std_errors), ("z_values", inf.t_values), ("p_values", inf.p_values),
                              ("ci_lower", inf.ci_lower), ("ci_upper", inf.ci_upper)):
                d[name] = [arr[i] for i in range(inf.len)]
        if extras:
            d["accuracy"], d["threshold"] = ex.accuracy, ex.threshold
        return d
    finally:
        lib.anofox_free_glm_result(C.byref(core))
        lib.anofox_free_result_inference(C.byref(inf))


def poisson_fit(y, x, options=None) -> dict:
    """anofox_stats_poisson_fit([y...], [[x1...], ...], {...}) through anofox_poisson_fit (a batch of one group)."""
    o = parse_poisson_options(options)
    s = _abi.AnofoxPoissonOptions(o.fit_intercept, 0, o.max_iterations, o.tolerance, o.compute_inference, o.confidence_level, o.lambda_,
                                  None, 0, 0, o.offset)
    return _scalar("anofox_poisson_fit", s, y, x)


def logistic_fit(y, x, options=None) -> dict:
    """anofox_stats_logistic_fit through anofox_logistic_fit: the binomial / logit fit of a 0 / 1 response plus the training
    accuracy at options['threshold'] (default 0.5)."""
    o = parse_binomial_options(options)
    thr = 0.5
    for k, v in (options or {}).items():
        if str(k).lower() == "threshold" and v is not None:
            thr = float(v)
    s = _abi.AnofoxLogisticOptions(o.fit_intercept, o.compute_inference, o.confidence_level, o.lambda_, thr, o.max_iterations,
                                   o.tolerance, None, 0, 0, o.offset)
    return _scalar("anofox_logistic_fit", s, y, x, extras=True)
