"""Grouped Gaussian linear mixed models with one random intercept (csrc/glmm.hip): the aggregates glmm_fit_agg and
glmm_fit_predict_agg, the scalar glmm_fit and the numpy / tensor drivers of anofox_hip_glmm_fit_batch_{host,device} and
anofox_hip_glmm_fit_predict_batch_{host,device}.  The contract: DESIGN.md §1 "Linear mixed models".  A
panel whose status is not 0 is None (SQL NULL) in the aggregate and NaN in the arrays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Mapping, Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import F64, I64, DeviceBatch, HostBatch
from .options import InvalidInputException, _extract_double

GAUSSIAN_NAMES = ("gaussian", "normal", "lmm")
NOT_BUILT_FAMILIES = {"poisson": 1, "binomial": 2, "logistic": 2, "negbinomial": 3, "gamma": 4, "tweedie": 5}
PRED_NAMES = ("yhat", "yhat_fixed", "se", "lower", "upper")
INTERVALS = {"none": 0, "confidence": 1, "prediction": 2}
RECORD_NAMES = ("intercept", "var_group", "var_residual", "icc", "log_likelihood", "aic", "bic", "deviance", "n_observations", "n_groups",
                "iterations", "converged", "status")


@dataclass
class GlmmOptions:
    family: int = 0
    fit_intercept: bool = True
    reml: bool = True
    max_iterations: int = 100
    tolerance: float = 1e-8
    compute_inference: bool = False
    confidence_level: float = 0.95
    interval: int = 0                  # fit-predict only: 0 none, 1 confidence, 2 prediction
    level: Optional[float] = None      # fit-predict only; None: confidence_level

    def predict_options(self) -> "_abi.AnofoxHipGlmmPredictOptions":
        return _abi.AnofoxHipGlmmPredictOptions(int(self.interval), float(self.confidence_level if self.level is None else self.level))

    def batch_options(self) -> "_abi.AnofoxHipGlmmOptions":
        return _abi.AnofoxHipGlmmOptions(self.family, int(self.fit_intercept), int(self.reml), int(self.max_iterations), float(self.tolerance),
                                         int(self.compute_inference), float(self.confidence_level))

    def ffi_options(self) -> "_abi.AnofoxGlmmOptions":
        return _abi.AnofoxGlmmOptions(self.family, bool(self.fit_intercept), int(self.max_iterations), float(self.tolerance),
                                      bool(self.compute_inference), float(self.confidence_level), bool(self.reml), 1.0, 1.5, 0, None, 0)


def _flag(v) -> bool:
    return str(v).lower() in ("true", "1", "t", "yes") if isinstance(v, str) else bool(v)


def parse_interval(val) -> int:
    """False, None or 'none' -> 0; 'confidence' -> 1; 'prediction' or True -> 2"""
    if val is None or val is False:
        return 0
    if val is True:
        return 2
    name = str(val).lower()
    if name not in INTERVALS:
        raise InvalidInputException("Unknown interval '%s'. Expected 'none', 'confidence' or 'prediction'." % (val,))
    return INTERVALS[name]


def parse_glmm_options(opts, predict: bool = False) -> GlmmOptions:
    """glmm_fit_agg's MAP options: family (gaussian | normal | lmm), fit_intercept | intercept, reml, max_iterations | max_iter,
    tolerance | tol, compute_inference, confidence_level, and for a fit-predict interval (False | None | 'none' | 'confidence' |
    'prediction'; True: 'prediction') and level (default: confidence_level).  Keys and values are case-insensitive; other keys are ignored, except
    those that ask for what is not built (an offset, random_slopes, a family other than Gaussian), which raise."""
    if isinstance(opts, GlmmOptions):
        return opts
    out = GlmmOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "family" and val is not None:
            name = str(val).lower()
            if name in NOT_BUILT_FAMILIES:
                raise InvalidInputException("glmm: the %s family is not built" % name)
            if name not in GAUSSIAN_NAMES:
                raise InvalidInputException("Unknown GLMM family '%s'. Expected 'gaussian'." % (val,))
        elif key in ("offset", "offset_column") and val is not None:
            raise InvalidInputException("glmm: an offset is not built")
        elif key == "random_slopes" and val is not None and len(val) > 0:
            raise InvalidInputException("glmm: random slopes are not built")
        elif key in ("fit_intercept", "intercept"):
            out.fit_intercept = _flag(val)
        elif key == "reml":
            out.reml = _flag(val)
        elif key in ("max_iterations", "max_iter"):
            out.max_iterations = int(_extract_double(val))
        elif key in ("tolerance", "tol"):
            out.tolerance = _extract_double(val)
        elif key == "compute_inference":
            out.compute_inference = _flag(val)
        elif key == "confidence_level":
            out.confidence_level = _extract_double(val)
        elif predict and key == "interval":   # (a fit ignores the two keys of a fit-predict, like every key it does not know)
            out.interval = parse_interval(val)
        elif predict and key == "level" and val is not None:
            out.level = _extract_double(val)
    return out


def _batch(b, plo, lro, options, inference, predict=False):
    o = parse_glmm_options(options, predict)
    plo, lro = b.array(plo, I64, None, "panel_level_offsets"), b.array(lro, I64, None, "level_row_offsets")
    G, L = b._size(plo) - 1, b._size(lro) - 1
    if G < 0 or L < 0:
        raise ValueError("the offsets need one entry more than there are panels and levels")
    if not 1 <= b.p <= 32:
        raise ValueError("glmm: 1 <= n_features <= 32")
    rec, ranef, ln = b.out((G, b.p + 13)), b.out((L,)), b.out((L,), I64)
    inf = b.out((G, 5 * b.p + 1)) if inference or o.compute_inference else None
    batch = o.batch_options()
    batch.compute_inference = int(inf is not None)
    if predict:
        pred = b.out((b.N, 5))
        b.call("anofox_hip_glmm_fit_predict_batch", G, L, b.p, b.N, plo, lro, b.y, b.cols, batch, o.predict_options(), rec, inf, ranef, ln, pred)
        return rec, inf, ranef, ln, pred
    b.call("anofox_hip_glmm_fit_batch", G, L, b.p, b.N, plo, lro, b.y, b.cols, batch, rec, inf, ranef, ln)
    return rec, inf, ranef, ln


def glmm_fit_batch_host(panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False, ctx=None):
    """numpy in / out: (records[n_panels, p + 13], inference[n_panels, 5 p + 1] or None, ranef[n_levels], level_n[n_levels]);
    anofox_hip_glmm_fit_batch_host's layouts."""
    return _batch(HostBatch(ctx, None, y, x_cols), panel_level_offsets, level_row_offsets, options, inference)


def glmm_fit_batch_device(ctx, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False,
                          use_current_torch_stream: bool = True):
    """glmm_fit_batch_host on CUDA tensors (offsets int64, y / columns float64).  Asynchronous."""
    return _batch(DeviceBatch(ctx, None, y, x_cols, use_current_torch_stream), panel_level_offsets, level_row_offsets, options, inference)


def glmm_fit_predict_batch_host(panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False, ctx=None):
    """glmm_fit_batch_host's four arrays (the same bytes) and pred[n_rows, 5] = (yhat, yhat_fixed, se, lower, upper);
    anofox_hip_glmm_fit_predict_batch_host's layouts.  Rows outside the level offsets are not written."""
    return _batch(HostBatch(ctx, None, y, x_cols), panel_level_offsets, level_row_offsets, options, inference, True)


def glmm_fit_predict_batch_device(ctx, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False,
                                  use_current_torch_stream: bool = True):
    """glmm_fit_predict_batch_host on CUDA tensors.  Asynchronous."""
    return _batch(DeviceBatch(ctx, None, y, x_cols, use_current_torch_stream), panel_level_offsets, level_row_offsets, options, inference, True)


def glmm_test_hooks(stats_only: int = 0, wave_mask: int = 0):
    """For measurements and tests: stats_only != 0 makes a call stop after the level statistics (the outputs are not written);
    wave_mask (bits 0, 1, 2: the search launch of 1, 4, 16 wavefronts) keeps the device form to those launches.  0 restores the
    library's rule."""
    _abi.load().anofox_hip_glmm_test_hooks(int(stats_only), int(wave_mask))


def record_dict(rec, inf, p: int) -> Optional[dict]:
    if int(rec[p + 12]) != 0:
        return None
    d = {"coefficients": [float(v) for v in rec[:p]]}
    for j, name in enumerate(RECORD_NAMES[:-1]):
        v = float(rec[p + j])
        d[name] = int(v) if name in ("n_observations", "n_groups", "iterations") else (bool(v) if name == "converged" else v)
    if inf is not None:
        for j, name in enumerate(("std_errors", "z_values", "p_values", "ci_lower", "ci_upper")):
            d[name] = [float(v) for v in inf[j * p:(j + 1) * p]]
        d["intercept_std_error"] = float(inf[5 * p])
    return d


@dataclass
class GlmmFitAggResult:
    """glmm_fit_agg's result: per panel (sorted keys) the record, the inference, and the levels in first-seen order."""
    keys: list
    n_features: int
    records: np.ndarray
    inference: Optional[np.ndarray]
    panel_level_offsets: np.ndarray
    level_labels: list          # per level: the caller's group value
    ranef_values: np.ndarray    # per level
    level_n: np.ndarray

    def row(self, i: int) -> Optional[dict]:
        d = record_dict(self.records[i], None if self.inference is None else self.inference[i], self.n_features)
        if d is not None:
            d["ranef"] = self.ranef(i)
        return d

    def ranef(self, i: int) -> list:
        l0, l1 = int(self.panel_level_offsets[i]), int(self.panel_level_offsets[i + 1])
        return [{"group": self.level_labels[l], "intercept": float(self.ranef_values[l]), "se": float("nan"), "n": int(self.level_n[l])}
                for l in range(l0, l1) if self.level_n[l] > 0]


def _column(values):
    a = np.asarray(values)
    return np.array([np.nan if v is None else v for v in values], dtype=np.float64) if a.dtype == object else np.asarray(a, np.float64)


def _first_seen(values):
    """-> (codes in first-seen order, the labels)"""
    seen, labels, codes = {}, [], np.empty(len(values), np.int64)
    for i, v in enumerate(values):
        v = v.item() if hasattr(v, "item") else v
        c = seen.get(v)
        if c is None:
            c = seen[v] = len(labels)
            labels.append(v)
        codes[i] = c
    return codes, labels


@dataclass
class GlmmFitPredictAggResult(GlmmFitAggResult):
    """glmm_fit_predict_agg's result: the fit's, and pred[n_input_rows, 5] in input row order (NaN for a row whose group is None)."""
    pred: Optional[np.ndarray] = None

    def __getattr__(self, name):   # the named views yhat, yhat_fixed, se, lower, upper
        pred = self.__dict__.get("pred")
        if name in PRED_NAMES and pred is not None:
            return pred[:, PRED_NAMES.index(name)]
        raise AttributeError(name)


def glmm_fit_agg(keys, y, x: Sequence, group, options=None, context=None) -> GlmmFitAggResult:
    """glmm_fit_agg(y, [x...], group, options) GROUP BY keys (None: one panel).  Rows may come in any order: they are sorted by
    (key, group), a key's levels in first-seen order; a row whose group is None is dropped, as the aggregate's Update drops it."""
    return _agg(keys, y, x, group, options, context, False)


def glmm_fit_predict_agg(keys, y, x: Sequence, group, options=None, context=None) -> GlmmFitPredictAggResult:
    """glmm_fit_predict_agg(y, [x...], group, options) GROUP BY keys: glmm_fit_agg's result and a score of every input row (a row
    with y None / NaN is a prediction row: the fit drops it and it is scored all the same)."""
    return _agg(keys, y, x, group, options, context, True)


def _agg(keys, y, x, group, options, context, predict):
    yv = _column(y)
    n = len(yv)
    cols = [_column(c) for c in x]
    groups = list(group)
    if len(groups) != n or any(len(c) != n for c in cols) or (keys is not None and len(keys) != n):
        raise InvalidInputException("y, every x, the group and the keys must have the same number of rows")
    keep = np.array([g is not None for g in groups], dtype=bool) if n else np.zeros(0, bool)
    idx = np.nonzero(keep)[0]
    key_codes_all, key_labels = _first_seen(list(keys)) if keys is not None else (np.zeros(n, np.int64), [None])
    order_keys = sorted(range(len(key_labels)), key=lambda i: key_labels[i]) if keys is not None else [0]
    rank = np.empty(len(key_labels), np.int64)
    rank[order_keys] = np.arange(len(key_labels))
    panel_of = rank[key_codes_all[idx]] if len(idx) else np.zeros(0, np.int64)
    pair_codes, pair_labels = _first_seen([(int(pk), groups[i]) for pk, i in zip(panel_of, idx)])
    # the levels of panel 0 first, each panel's in first-seen order
    level_panel = np.array([pl[0] for pl in pair_labels], np.int64)
    level_order = np.argsort(level_panel, kind="stable")
    level_rank = np.empty(len(pair_labels), np.int64)
    level_rank[level_order] = np.arange(len(pair_labels))
    row_level = level_rank[pair_codes] if len(idx) else np.zeros(0, np.int64)
    perm = idx[np.argsort(row_level, kind="stable")]
    L, G = len(pair_labels), len(key_labels)
    lro = np.concatenate([[0], np.cumsum(np.bincount(row_level, minlength=L))]).astype(np.int64)
    plo = np.concatenate([[0], np.cumsum(np.bincount(level_panel, minlength=G))]).astype(np.int64)
    labels = [pair_labels[i][1] for i in level_order]
    if predict:
        rec, inf, ranef, ln, sorted_pred = glmm_fit_predict_batch_host(plo, lro, yv[perm], [c[perm] for c in cols], options, ctx=context)
        pred = np.full((n, 5), np.nan)
        pred[perm] = sorted_pred
        return GlmmFitPredictAggResult([key_labels[i] for i in order_keys], len(cols), rec, inf, plo, labels, ranef, ln, pred)
    rec, inf, ranef, ln = glmm_fit_batch_host(plo, lro, yv[perm], [c[perm] for c in cols], options, ctx=context)
    return GlmmFitAggResult([key_labels[i] for i in order_keys], len(cols), rec, inf, plo, [pair_labels[i][1] for i in level_order], ranef, ln)


def glmm_fit(y, x: Sequence, group, options=None) -> dict:
    """anofox_stats_glmm_fit(y, [x...], group, {...}) through anofox_glmm_fit (a batch of one panel): glmm_fit_agg's row.  group:
    integer ids (ids < 0 and None are dropped) or any labels, which are numbered in first-seen order."""
    from .scalar import _data_array
    o = parse_glmm_options(options)
    groups = list(group)
    if all(g is None or isinstance(g, (int, np.integer)) for g in groups):
        ids, labels = np.array([-1 if g is None else int(g) for g in groups], np.int32), None
    else:
        codes, labels = _first_seen([g for g in groups if g is not None])
        ids, it = np.full(len(groups), -1, np.int32), iter(codes)
        for i, g in enumerate(groups):
            if g is not None:
                ids[i] = next(it)
    lib = _abi.load()
    ya, k0 = _data_array(y)
    held = [_data_array(c) for c in x]
    xa = (_abi.AnofoxDataArray * max(len(held), 1))(*[h[0] for h in held])
    res = _abi.AnofoxGlmmResult()
    err = _abi.AnofoxError()
    ok = lib.anofox_glmm_fit(ya, xa, len(held), ids.ctypes.data_as(C.POINTER(C.c_int32)), len(ids), None, 0, o.ffi_options(), C.byref(res),
                             C.byref(err))
    if not ok:
        e = InvalidInputException(f"glmm_fit failed: {AnofoxStatsError(err.code, err.text())}")
        e.code = err.code
        raise e
    try:
        p = res.coefficients_len
        d = {"coefficients": [res.coefficients[j] for j in range(p)], "intercept": res.intercept, "var_group": res.var_group,
             "var_residual": res.var_residual, "icc": res.icc, "log_likelihood": res.log_likelihood, "aic": res.aic, "bic": res.bic,
             "deviance": res.deviance, "n_observations": res.n_observations, "n_groups": res.n_groups, "iterations": res.iterations,
             "converged": bool(res.converged)}
        if res.inference_len:
            for name in ("std_errors", "z_values", "p_values", "ci_lower", "ci_upper"):
                d[name] = [getattr(res, name)[j] for j in range(p)]
            d["intercept_std_error"] = res.intercept_std_error
        d["ranef"] = [{"group": res.ranef_group[i] if labels is None else labels[res.ranef_group[i]], "intercept": res.ranef_value[i],
                       "se": res.ranef_se[i], "n": res.ranef_n[i]} for i in range(res.ranef_len)]
        return d
    finally:
        lib.anofox_free_glmm_result(C.byref(res))
