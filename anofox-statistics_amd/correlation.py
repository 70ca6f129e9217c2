"""Grouped Pearson, Spearman and Kendall correlation with the test of no association (csrc/rank_cor.hip): the aggregates
pearson_agg / spearman_agg / kendall_agg, the scalars pearson / spearman / kendall through the reference-compatible symbols, and
the numpy / tensor drivers of anofox_hip_cor_batch_{host,device}.  The contract: DESIGN.md §1 "Rank and product-moment
correlation".  A group whose status is not 0 (fewer than 3 valid pairs) is None (SQL NULL) in the aggregates."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._marshal import F64, DeviceBatch, HostBatch, column, group_rows, scalar_call
from .options import InvalidInputException, _extract_alternative, _extract_double

PEARSON, SPEARMAN, KENDALL = 0, 1, 2
RECORD_NAMES = ("estimate", "statistic", "p_value", "ci_lower", "ci_upper", "n", "s", "status")
TAU_TYPE = {"a": 0, "tau_a": 0, "taua": 0, "b": 1, "tau_b": 1, "taub": 1, "c": 2, "tau_c": 2, "tauc": 2}
METHOD_TEXT = {PEARSON: "Pearson correlation", SPEARMAN: "Spearman rank correlation"}
TAU_TEXT = ("Kendall's TauA", "Kendall's TauB", "Kendall's TauC")


@dataclass
class CorrelationOptions:
    """Resolved options: alternative 0 two-sided, 1 less, 2 greater; tau_type 0 a, 1 b, 2 c (Kendall only); confidence_level None:
    no interval."""
    alternative: int = 0
    confidence_level: Optional[float] = 0.95
    tau_type: int = 1

    def _level(self) -> float:
        return float("nan") if self.confidence_level is None else float(self.confidence_level)

    def batch_options(self, method: int) -> "_abi.AnofoxHipCorBatchOptions":
        return _abi.AnofoxHipCorBatchOptions(int(method), self.alternative, self.tau_type, self._level())

    def ffi_options(self) -> "_abi.AnofoxCorrelationOptions":
        return _abi.AnofoxCorrelationOptions(self.alternative, self._level())

    def kendall_ffi_options(self) -> "_abi.AnofoxKendallOptions":
        return _abi.AnofoxKendallOptions(self.alternative, self.tau_type, self._level())

    def method_text(self, method: int) -> str:
        return TAU_TEXT[self.tau_type] if method == KENDALL else METHOD_TEXT[method]


def parse_correlation_options(opts) -> CorrelationOptions:
    """The MAP options of the three aggregates: alternative (two_sided | less | greater), confidence_level, tau_type | variant
    (a | b | c, also tau_a ...).  Keys and values are case-insensitive; other keys are ignored.  The confidence level is not
    range-checked here: the library reports it."""
    if isinstance(opts, CorrelationOptions):
        return opts
    out = CorrelationOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "alternative" and val is not None:
            out.alternative = _extract_alternative(val)
        elif key == "confidence_level":
            out.confidence_level = _extract_double(val)
        elif key in ("tau_type", "variant") and val is not None:
            name = str(val).lower()
            if name not in TAU_TYPE:
                raise InvalidInputException("Unknown tau_type '%s'. Expected 'a', 'b' or 'c'." % (val,))
            out.tau_type = TAU_TYPE[name]
    return out


def _cor_batch(b, y, method, options):
    """records[G, 8] of the batch b, whose leading column is x."""
    rec = b.out((b.G, 8))
    b.call("anofox_hip_cor_batch", b.G, b.N, b.off, b.y, b.array(y, F64, b.N, "y"), parse_correlation_options(options).batch_options(method), rec)
    return rec


def cor_batch_host(row_offsets, x, y, method: int, options=None, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of x and y.  Returns records[n_groups, 8] =
    RECORD_NAMES; anofox_hip_cor_batch_host's layout."""
    return _cor_batch(HostBatch(ctx, row_offsets, x, [], lead="x"), y, method, options)


def cor_batch_device(ctx, row_offsets, x, y, method: int, options=None, use_current_torch_stream: bool = True):
    """cor_batch_host on CUDA tensors (row_offsets int64, x / y float64).  Asynchronous.  Returns the records tensor."""
    return _cor_batch(DeviceBatch(ctx, row_offsets, x, [], use_current_torch_stream, lead="x"), y, method, options)


def cor_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group may have on the small path (one wavefront, rows in LDS); 0 restores the library's cap."""
    _abi.load().anofox_hip_cor_test_hooks(int(small_cap))


@dataclass
class CorrelationAggResult:
    """Per sorted key the record of its group."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 8]: RECORD_NAMES
    method: int
    method_text: str

    def row(self, g: int) -> Optional[dict]:
        """{r | tau, statistic, p_value, ci_lower, ci_upper, n, method}, or None for a failed group."""
        rec = self.records[g]
        if int(rec[7]) != 0:
            return None
        return {"tau" if self.method == KENDALL else "r": float(rec[0]), "statistic": float(rec[1]), "p_value": float(rec[2]),
                "ci_lower": float(rec[3]), "ci_upper": float(rec[4]), "n": int(rec[5]), "method": self.method_text}

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _agg(method, keys, x, y, options, context) -> CorrelationAggResult:
    o = parse_correlation_options(options)
    xv, yv = column(x), column(y)
    if not (len(xv) == len(yv) == len(keys)):
        raise InvalidInputException("the keys, x and y must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    rec = cor_batch_host(off, xv[perm], yv[perm], method, o, ctx=context)
    return CorrelationAggResult(uniq, rec, method, o.method_text(method))


def pearson_agg(keys, x, y, options=None, context=None) -> CorrelationAggResult:
    """pearson_agg(x, y, options) GROUP BY keys.  A None in x or y is a NULL: the row is not valid."""
    return _agg(PEARSON, keys, x, y, options, context)


def spearman_agg(keys, x, y, options=None, context=None) -> CorrelationAggResult:
    """spearman_agg(x, y, options) GROUP BY keys."""
    return _agg(SPEARMAN, keys, x, y, options, context)


def kendall_agg(keys, x, y, options=None, context=None) -> CorrelationAggResult:
    """kendall_agg(x, y, options) GROUP BY keys; options tau_type | variant a, b (default) or c."""
    return _agg(KENDALL, keys, x, y, options, context)


def _scalar(symbol, x, y, ffi_options, estimate) -> dict:
    fields = [(estimate, "r")] + [(f, f) for f in ("statistic", "p_value", "ci_lower", "ci_upper", "n", "method")]
    return scalar_call(symbol, (x, y), ffi_options, _abi.AnofoxCorrelationResult, "anofox_free_correlation_result", fields)


def pearson(x, y, options=None) -> dict:
    """anofox_stats_pearson(x, y, {...}) through anofox_pearson_cor (a batch of one group)."""
    return _scalar("anofox_pearson_cor", x, y, parse_correlation_options(options).ffi_options(), "r")


def spearman(x, y, options=None) -> dict:
    """anofox_stats_spearman(x, y, {...}) through anofox_spearman_cor."""
    return _scalar("anofox_spearman_cor", x, y, parse_correlation_options(options).ffi_options(), "r")


def kendall(x, y, options=None) -> dict:
    """anofox_stats_kendall(x, y, {'tau_type': 'b'}) through anofox_kendall_cor."""
    return _scalar("anofox_kendall_cor", x, y, parse_correlation_options(options).kendall_ffi_options(), "tau")
