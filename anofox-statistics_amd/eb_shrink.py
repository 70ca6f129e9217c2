"""Empirical-Bayes shrinkage of per-group estimates toward their precision-weighted mean (csrc/eb_shrink.hip): the scalar
eb_shrink, the aggregate eb_shrink_agg, shrink_coefficients on a GLM or AFT fit result, and the numpy / tensor drivers of
anofox_hip_eb_shrink_batch_{host,device}.  The contract: DESIGN.md §1 "Empirical-Bayes shrinkage".  A set whose status is not 0
is None (SQL NULL) in the aggregate and NaN in the arrays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import F64, I64, call, column, device_tensor, group_rows, handle, host_array, _invoke
from .options import InvalidInputException, _extract_double

TAU_METHOD = {"dl": 0, "dersimonian_laird": 0, "dersimonian-laird": 0, "none": 1, "pooled": 1, "complete": 1}
SUMMARY_NAMES = ("mu", "mu_se", "tau_squared", "i_squared", "q", "n_groups", "n_input", "status")


@dataclass
class EbShrinkOptions:
    """Resolved options: the DerSimonian-Laird estimate of tau^2 unless method is 1 (none: complete pooling) or tau_squared is
    given (it overrides the method)."""
    method: int = 0
    tau_squared: Optional[float] = None

    def batch_options(self) -> "_abi.AnofoxHipEbShrinkOptions":
        return _abi.AnofoxHipEbShrinkOptions(self.method, float("nan") if self.tau_squared is None else float(self.tau_squared))

    def ffi_options(self) -> "_abi.AnofoxEbShrinkOptions":
        return _abi.AnofoxEbShrinkOptions(self.method, float("nan") if self.tau_squared is None else float(self.tau_squared))


def parse_eb_shrink_options(opts) -> EbShrinkOptions:
    """eb_shrink's MAP options: tau_squared | tau2, tau_method | shrinkage (dl | dersimonian_laird | dersimonian-laird, none | pooled |
    complete).  Keys and values are case-insensitive; other keys are ignored.  The value of tau_squared is not range-checked
    here: the library reports it (status 1 / InvalidInput)."""
    if isinstance(opts, EbShrinkOptions):
        return opts
    out = EbShrinkOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("tau_squared", "tau2"):
            out.tau_squared = _extract_double(val)
        elif key in ("tau_method", "shrinkage") and val is not None:
            name = str(val).lower()
            if name not in TAU_METHOD:
                raise InvalidInputException("Unknown tau_method '%s'. Expected 'dl' or 'none'." % (val,))
            out.method = TAU_METHOD[name]
    return out


def _shape(set_offsets_len, n_items, n_cols, est_stride, se_stride):
    n_cols = int(n_cols)
    est_stride, se_stride = int(n_cols if est_stride is None else est_stride), int(n_cols if se_stride is None else se_stride)
    if set_offsets_len < 1:
        raise ValueError("set_offsets needs one entry more than there are sets")
    if n_cols < 1 or est_stride < n_cols or se_stride < n_cols:
        raise ValueError("n_cols must be at least 1 and no stride smaller than n_cols")
    need = lambda stride: (n_items - 1) * stride + n_cols if n_items > 0 else 0   # noqa: E731
    return n_cols, est_stride, se_stride, need(est_stride), need(se_stride)


def eb_shrink_batch_host(set_offsets, est, se, n_cols: int = 1, est_stride: Optional[int] = None, se_stride: Optional[int] = None,
                         options=None, n_items: Optional[int] = None, ctx=None):
    """The matrix form, numpy in / out: est[g est_stride + c], se[g se_stride + c] for item g and column c, set_offsets[n_sets + 1]
    contiguous item ranges.  Returns (out[n_items, n_cols, 3] = {shrunken, shrunken_se, weight}, summary[n_sets, n_cols, 8] =
    SUMMARY_NAMES); anofox_hip_eb_shrink_batch_host's layouts.  Items outside every set are NaN."""
    off = host_array(set_offsets, I64, None, "set_offsets")
    n_items = int(off[-1]) if n_items is None and off.size else int(n_items or 0)
    n_cols, es, ss, need_e, need_s = _shape(off.size, n_items, n_cols, est_stride, se_stride)
    e, s = host_array(est, F64, None, "estimate"), host_array(se, F64, None, "se")
    if e.size < need_e or s.size < need_s:
        raise ValueError("estimate or se is shorter than n_items, the stride and n_cols need")
    out, summary = np.full((n_items, n_cols, 3), np.nan), np.empty((off.size - 1, n_cols, 8))
    call(_abi.load(), "anofox_hip_eb_shrink_batch_host", handle(ctx), off.size - 1, n_items, off, n_cols, e, es, s, ss,
         parse_eb_shrink_options(options).batch_options(), out, summary)
    return out, summary


def eb_shrink_batch_device(ctx, set_offsets, est, se, n_cols: int = 1, est_stride: Optional[int] = None, se_stride: Optional[int] = None,
                           options=None, n_items: Optional[int] = None, use_current_torch_stream: bool = True):
    """eb_shrink_batch_host on CUDA tensors (set_offsets int64, est / se float64).  Asynchronous.  n_items: the items the arrays
    hold (None: as many as the tensors hold at these strides).  Items outside every set keep NaN."""
    import torch

    off = device_tensor(set_offsets, I64, None, "set_offsets")
    e = device_tensor(est, F64, None, "estimate", off.device)
    s = device_tensor(se, F64, None, "se", off.device)
    nc = int(n_cols)
    if n_items is None:
        es0, ss0 = int(nc if est_stride is None else est_stride), int(nc if se_stride is None else se_stride)
        n_items = max(0, min((e.numel() - nc) // es0 + 1 if e.numel() >= nc else 0, (s.numel() - nc) // ss0 + 1 if s.numel() >= nc else 0))
    n_cols, es, ss, need_e, need_s = _shape(off.numel(), int(n_items), n_cols, est_stride, se_stride)
    if e.numel() < need_e or s.numel() < need_s:
        raise ValueError("estimate or se is shorter than n_items, the stride and n_cols need")
    out = torch.full((int(n_items), n_cols, 3), float("nan"), dtype=torch.float64, device=off.device)
    summary = torch.empty((off.numel() - 1, n_cols, 8), dtype=torch.float64, device=off.device)
    if use_current_torch_stream:
        ctx.set_stream(torch.cuda.current_stream(off.device).cuda_stream)
    ok, err = _invoke(ctx._lib, "anofox_hip_eb_shrink_batch_device", (ctx._h, off.numel() - 1, int(n_items), off, n_cols, e, es, s, ss,
                                                                      parse_eb_shrink_options(options).batch_options(), out, summary))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return out, summary


def eb_shrink_test_hooks(force_path: int = 0, chunk_items: int = 0, max_workgroups: int = 0):
    """For tests: force_path 1 = one wavefront per set, 2 = the chunk path; chunk_items = the items of a chunk; max_workgroups =
    the most workgroups a launch starts.  0 restores the library's rule."""
    _abi.load().anofox_hip_eb_shrink_test_hooks(int(force_path), int(chunk_items), int(max_workgroups))


def _summary_dict(row) -> Optional[dict]:
    if int(row[7]) != 0:
        return None
    return {"mu": float(row[0]), "mu_se": float(row[1]), "tau_squared": float(row[2]), "i_squared": float(row[3]), "q": float(row[4]),
            "n_groups": int(row[5])}


def eb_shrink(estimate, se, options=None) -> dict:
    """anofox_stats_eb_shrink([estimate...], [se...], {...}) through anofox_eb_shrink (a batch of one set): the reference's result,
    {mu, mu_se, tau_squared, i_squared, q, n_groups, shrunken: [{estimate, se, shrunken, shrunken_se, weight}, ...]}.  None entries are
    NULLs: pairs that are not usable."""
    from .scalar import _data_array
    o = parse_eb_shrink_options(options)
    lib = _abi.load()
    ea, k0 = _data_array(estimate)
    sa, k1 = _data_array(se)
    res = _abi.AnofoxEbShrinkResult()
    try:
        call(lib, "anofox_eb_shrink", ea, sa, o.ffi_options(), C.byref(res))
    except AnofoxStatsError as failed:
        e = InvalidInputException(f"eb_shrink failed: {failed}")
        e.code = failed.code
        raise e from None
    try:
        rows = [{"estimate": res.estimate[i], "se": res.se[i], "shrunken": res.shrunken[i], "shrunken_se": res.shrunken_se[i],
                 "weight": res.weight[i]} for i in range(res.len)]
        return {"mu": res.mu, "mu_se": res.mu_se, "tau_squared": res.tau_squared, "i_squared": res.i_squared, "q": res.q,
                "n_groups": res.n_groups, "shrunken": rows}
    finally:
        lib.anofox_free_eb_shrink_result(C.byref(res))


def _sets(keys, n):
    """The items sorted by key (stably): -> (sorted unique keys, the permutation, offsets)."""
    keys = np.asarray(keys)
    if len(keys) != n:
        raise InvalidInputException("the keys and the estimates must have the same number of rows")
    return group_rows(keys)


def eb_shrink_agg(set_keys, estimate, se, options=None, context=None) -> dict:
    """eb_shrink_agg(estimate, se, options) GROUP BY set_keys: per key the reference's result (eb_shrink's dict, the rows in input
    order), or None for a set with fewer than 2 usable pairs.  A row whose estimate or se is None is skipped, as the aggregate's
    Update skips a NULL."""
    e, s = column(estimate), column(se)
    if len(e) != len(s):
        raise InvalidInputException("estimate and se must have the same number of rows")
    raw_e, raw_s = np.asarray(estimate, dtype=object), np.asarray(se, dtype=object)
    keep = np.array([a is not None and b is not None for a, b in zip(raw_e, raw_s)], dtype=bool) if len(e) else np.zeros(0, bool)
    keys = np.asarray(set_keys)
    if len(keys) != len(e):
        raise InvalidInputException("the keys and the estimates must have the same number of rows")
    all_keys = np.unique(keys)
    uniq, perm, off = _sets(keys[keep], int(keep.sum()))
    e, s = e[keep][perm], s[keep][perm]
    out, summary = eb_shrink_batch_host(off, e, s, options=options, ctx=context)
    result = {k: None for k in all_keys.tolist()}
    for i, k in enumerate(uniq.tolist()):
        d = _summary_dict(summary[i, 0])
        if d is not None:
            d["shrunken"] = [{"estimate": float(e[g]), "se": float(s[g]), "shrunken": float(out[g, 0, 0]), "shrunken_se": float(out[g, 0, 1]),
                              "weight": float(out[g, 0, 2])} for g in range(off[i], off[i + 1])]
        result[k] = d
    return result


@dataclass
class ShrunkCoefficients:
    """shrink_coefficients' result: per set (sorted keys of `by`; one set without it) and coefficient column the summary, and per
    group of the fit, in the fit's order, the shrunken coefficients."""
    set_keys: np.ndarray
    summary: np.ndarray       # [n_sets, p, 8]: SUMMARY_NAMES
    shrunken: np.ndarray      # [n_groups, p]
    shrunken_se: np.ndarray   # [n_groups, p]
    weight: np.ndarray        # [n_groups, p]

    def set_summary(self, i: int, column: int) -> Optional[dict]:
        return _summary_dict(self.summary[i, column])


def shrink_coefficients(fit, by=None, options=None, context=None) -> ShrunkCoefficients:
    """Shrinks every coefficient column of a GlmFitAggResult or an AftFitAggResult computed with inference toward the column's
    pooled mean: one launch on the result's own record and inference arrays (the strided form; no column is copied out).  by: a
    key per group; groups with equal keys form one set (default: all groups one set).  A failed group (NaN coefficients) is a pair
    that is not usable: it keeps its place with NaN outputs."""
    rec, inf, p = getattr(fit, "records", None), getattr(fit, "inference", None), getattr(fit, "n_features", None)
    if rec is None or p is None:
        raise InvalidInputException("shrink_coefficients takes the result of a GLM or AFT fit aggregate")
    if inf is None:
        raise InvalidInputException("shrink_coefficients needs standard errors: fit with compute_inference")
    rec, inf = np.asarray(rec, np.float64), np.asarray(inf, np.float64)
    n = rec.shape[0]
    if by is None:
        keys, perm, off = np.zeros(1, np.int64), None, np.array([0, n], np.int64)
    else:
        keys, perm, off = _sets(by, n)
        rec, inf = rec[perm], inf[perm]   # (equal keys become neighbours; the records stay whole)
    out, summary = eb_shrink_batch_host(off, rec, inf, n_cols=p, est_stride=rec.shape[1], se_stride=inf.shape[1], options=options,
                                        n_items=n, ctx=context)
    if perm is not None:
        back = np.empty_like(out)
        back[perm] = out
        out = back
    return ShrunkCoefficients(keys, summary, out[:, :, 0].copy(), out[:, :, 1].copy(), out[:, :, 2].copy())
