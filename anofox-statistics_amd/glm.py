"""Generalised linear models on the fused IRLS kernel (csrc/glm.hip): poisson_fit_agg, binomial_fit_agg, logistic_fit_agg,
poisson_fit_predict_agg, the scalar poisson_fit / logistic_fit, and the numpy drivers of anofox_hip_glm_fit_batch_host /
anofox_hip_glm_fit_predict_batch_host and of their interval / accuracy forms.  The contract: DESIGN.md §1 "Generalised linear
models".  Results mirror the fields of the reference's AnofoxGlmFitResultCore; a group whose status is not 0 is None (SQL NULL)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from .options import GlmOptions, InvalidInputException, parse_binomial_options, parse_poisson_options

_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)


def _prepare(row_offsets, y, x_cols, offset):
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    ov = None if offset is None else np.ascontiguousarray(offset, dtype=np.float64)
    N = len(yv)
    if any(len(c) != N for c in cols) or (ov is not None and len(ov) != N):
        raise ValueError("every column must have y's length")
    colp = (_DP * max(len(cols), 1))(*[c.ctypes.data_as(_DP) for c in cols])
    return off, yv, cols, ov, colp


def glm_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None, inference: bool = False,
                       ctx=None, threshold=None):
    """Grouped GLM fits, numpy in / out: records[G, p + 11] (and inference[G, 5 p] with inference=True); the layouts are
    anofox_hip_glm_fit_batch_host's (include/anofox_stats_hip.h).  With a threshold (binomial) the call goes through
    anofox_hip_glm_fit_accuracy_batch_host and accuracy[G] is appended to what is returned."""
    lib = _abi.load()
    off, yv, cols, ov, colp = _prepare(row_offsets, y, x_cols, offset)
    p, G, N = len(cols), len(off) - 1, len(yv)
    rec = np.empty((G, p + 11), dtype=np.float64)
    inf = np.empty((G, 5 * p), dtype=np.float64) if inference else None
    err = _abi.AnofoxError()
    head = (ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(_I64P), yv.ctypes.data_as(_DP), colp,
            None if ov is None else ov.ctypes.data_as(_DP), options)
    out = (rec.ctypes.data_as(_DP), None if inf is None else inf.ctypes.data_as(_DP))
    if threshold is None:
        ok = lib.anofox_hip_glm_fit_batch_host(*head, *out, C.byref(err))
    else:
        acc = np.empty(G, dtype=np.float64)
        ok = lib.anofox_hip_glm_fit_accuracy_batch_host(*head, float(threshold), *out, acc.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    res = (rec, inf) if inference else (rec,)
    if threshold is not None:
        res += (acc,)
    return res if len(res) > 1 else rec


def glm_fit_accuracy_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, threshold: float = 0.5,
                                offset=None, inference: bool = False, ctx=None):
    """anofox_hip_glm_fit_accuracy_batch_host: (records, [inference,] accuracy[G]); binomial family only."""
    return glm_fit_batch_host(row_offsets, y, x_cols, options, offset, inference, ctx, threshold=threshold)


def glm_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None, train_counts=None,
                               ctx=None, interval_z=None):
    """GLM fit + predict, numpy in / out: (core[G, p + 11], pred[N, 3] = mu, NaN, NaN; a NaN mu = NULL).  With interval_z the
    call goes through anofox_hip_glm_fit_predict_interval_batch_host: pred = mu, lower, upper for interval_z > 0 (Poisson)."""
    lib = _abi.load()
    off, yv, cols, ov, colp = _prepare(row_offsets, y, x_cols, offset)
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    core = np.empty((G, p + 11), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    err = _abi.AnofoxError()
    fn = lib.anofox_hip_glm_fit_predict_batch_host if interval_z is None else lib.anofox_hip_glm_fit_predict_interval_batch_host
    ok = fn(ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(_I64P), yv.ctypes.data_as(_DP), colp,
            None if ov is None else ov.ctypes.data_as(_DP), None if tc is None else tc.ctypes.data_as(_I64P), options,
            *(() if interval_z is None else (float(interval_z),)), core.ctypes.data_as(_DP), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def glm_fit_predict_interval_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, interval_z: float,
                                        offset=None, train_counts=None, ctx=None):
    """anofox_hip_glm_fit_predict_interval_batch_host: (core[G, p + 11], pred[N, 3] = mu, lower, upper)."""
    return glm_fit_predict_batch_host(row_offsets, y, x_cols, options, offset, train_counts, ctx, interval_z=interval_z)


def glm_fit_batch_device(ctx, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                         inference: bool = False, use_current_torch_stream: bool = True, threshold=None):
    """Grouped GLM fits on CUDA tensors (row_offsets int64[G + 1], y / x_cols[j] / offset float64[N]).  Asynchronous.
    Returns records[G, p + 11], or (records, inference[G, 5 p]) with inference=True; with a threshold (binomial, through
    anofox_hip_glm_fit_accuracy_batch_device) accuracy[G] is appended."""
    import torch

    p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
    tensors = (row_offsets, y, *x_cols) + (() if offset is None else (offset,))
    for t in tensors:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device batch needs contiguous CUDA tensors")
    if row_offsets.dtype != torch.int64 or any(t.dtype != torch.float64 for t in tensors[1:]):
        raise ValueError("row_offsets must be int64 and data float64")
    if any(int(t.numel()) != N for t in tensors[1:]):
        raise ValueError("every column must have y's length")
    rec = torch.empty((G, p + 11), dtype=torch.float64, device=y.device)
    inf = torch.empty((G, 5 * p), dtype=torch.float64, device=y.device) if inference else None
    if use_current_torch_stream:
        ctx.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
    cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
    err = _abi.AnofoxError()
    head = (ctx._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(offset.data_ptr()) if offset is not None else None, options)
    out = (C.c_void_p(rec.data_ptr()), C.c_void_p(inf.data_ptr()) if inf is not None else None)
    if threshold is None:
        ok = ctx._lib.anofox_hip_glm_fit_batch_device(*head, *out, C.byref(err))
    else:
        acc = torch.empty((G,), dtype=torch.float64, device=y.device)
        ok = ctx._lib.anofox_hip_glm_fit_accuracy_batch_device(*head, float(threshold), *out, C.c_void_p(acc.data_ptr()), C.byref(err))
    ctx._check(ok, err)
    res = (rec, inf) if inference else (rec,)
    if threshold is not None:
        res += (acc,)
    return res if len(res) > 1 else rec


def glm_fit_predict_batch_device(ctx, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                                 train_counts=None, use_current_torch_stream: bool = True, interval_z=None):
    """GLM fit + predict on CUDA tensors (inputs as glm_fit_batch_device; train_counts int64[G] or None).  Asynchronous.
    Returns (core[G, p + 11], pred[N, 3]); rows outside [row_offsets[0], row_offsets[G]) are not written.  With interval_z the
    call goes through anofox_hip_glm_fit_predict_interval_batch_device."""
    import torch

    p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
    data = (y, *x_cols) + (() if offset is None else (offset,))
    ints = (row_offsets,) + (() if train_counts is None else (train_counts,))
    for t in data + ints:
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("device batch needs contiguous CUDA tensors")
    if any(t.dtype != torch.int64 for t in ints) or any(t.dtype != torch.float64 for t in data):
        raise ValueError("row_offsets / train_counts must be int64 and data float64")
    if any(int(t.numel()) != N for t in data) or (train_counts is not None and int(train_counts.numel()) != G):
        raise ValueError("every column must have y's length and train_counts one entry per group")
    core = torch.empty((G, p + 11), dtype=torch.float64, device=y.device)
    pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
    if use_current_torch_stream:
        ctx.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
    cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
    err = _abi.AnofoxError()
    fn = ctx._lib.anofox_hip_glm_fit_predict_batch_device if interval_z is None else ctx._lib.anofox_hip_glm_fit_predict_interval_batch_device
    ok = fn(ctx._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(offset.data_ptr()) if offset is not None else None,
            C.c_void_p(train_counts.data_ptr()) if train_counts is not None else None, options,
            *(() if interval_z is None else (float(interval_z),)), C.c_void_p(core.data_ptr()), C.c_void_p(pred.data_ptr()), C.byref(err))
    ctx._check(ok, err)
    return core, pred


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
    uniq, inv = np.unique(keys, return_inverse=True)
    perm = np.argsort(inv, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))]).astype(np.int64)
    feat = [j for j in range(X.shape[1]) if j != opts.offset - 1]
    cols = [np.ascontiguousarray(X[perm, j]) for j in feat]
    off = np.ascontiguousarray(X[perm, opts.offset - 1]) if opts.offset else None
    return uniq, inv, perm, offsets, yv[perm], cols, off


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
    core, inf, ex, err = _abi.AnofoxGlmFitResultCore(), _abi.AnofoxFitResultInference(), _abi.AnofoxLogisticFitExtras(), _abi.AnofoxError()
    args = [ya, xs, len(x), opt_struct, C.byref(core), C.byref(inf) if opt_struct.compute_inference else None]
    if extras:
        args.append(C.byref(ex))
    if not getattr(lib, fn_name)(*args, C.byref(err)):
        e = InvalidInputException(f"GLM fit failed: {err.text()}")
        e.code = err.code
        raise e
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
