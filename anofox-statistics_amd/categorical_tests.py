"""Grouped categorical tests (csrc/categorical_tests.hip): the aggregates chisq_test_agg / g_test_agg / fisher_exact_agg / mcnemar_agg /
cramers_v_agg / phi_coefficient_agg / contingency_coef_agg, the scalars chisq_test / g_test / fisher_exact / mcnemar_test / cramers_v /
phi_coefficient / contingency_coef through the reference-compatible symbols, and the numpy / tensor drivers of
anofox_hip_categorical_test_batch_{host,device}.  The contract: DESIGN.md §1 "Categorical tests".  A group is None (SQL NULL) in an
aggregate where the reference's finalize returns NULL: below its minimum of rows (1 for chi-square, 2 for Cramer's V, 4 for G,
Fisher, McNemar, phi and C), with fewer than two levels on a side, and for phi when the table is not 2 x 2."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import I32, DeviceBatch, HostBatch, call, group_rows, scalar_call
from .options import InvalidInputException, _extract_alternative, _extract_double
from .rank_tests import _extract_bool

CHI_SQUARE, G_TEST, FISHER_EXACT, MCNEMAR = 0, 1, 2, 3
RECORD_NAMES = ("statistic", "p_value", "df", "estimate", "ci_lower", "ci_upper", "n", "n_row_levels", "n_col_levels", "aux", "aux2", "status")
NULL_LABEL = -2 ** 31   # INT32_MIN: the NULL of a label column
NAN = float("nan")


@dataclass
class CategoricalTestOptions:
    """Resolved options: correction (None: the aggregate's default, off for chi-square and on for McNemar); alternative 0 two-sided,
    1 less, 2 greater (Fisher); exact (McNemar's binomial p); confidence_level of Fisher's interval (None: no interval)."""
    correction: Optional[bool] = None
    alternative: int = 0
    exact: bool = False
    confidence_level: Optional[float] = 0.95

    def resolved_correction(self, test: int) -> bool:
        return (test == MCNEMAR) if self.correction is None else bool(self.correction)

    def batch_options(self, test: int) -> "_abi.AnofoxHipCategoricalTestBatchOptions":
        level = NAN if self.confidence_level is None else float(self.confidence_level)
        return _abi.AnofoxHipCategoricalTestBatchOptions(int(test), int(self.alternative), int(self.resolved_correction(test)),
                                                         int(bool(self.exact)), level)


def parse_categorical_test_options(opts) -> CategoricalTestOptions:
    """The MAP options of the aggregates: correction | continuity_correction, alternative, exact, confidence_level.  Keys and values
    are case-insensitive; other keys are ignored."""
    if isinstance(opts, CategoricalTestOptions):
        return opts
    out = CategoricalTestOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("correction", "continuity_correction") and val is not None:
            out.correction = _extract_bool(val)
        elif key == "alternative" and val is not None:
            out.alternative = _extract_alternative(val)
        elif key == "exact" and val is not None:
            out.exact = _extract_bool(val)
        elif key == "confidence_level":
            out.confidence_level = _extract_double(val)
    return out


def _categorical_test_batch(b, a, b_col, test, options):
    """records[G, 12] of the batch b (its offsets alone) over the int32 columns a and b_col."""
    a = b.array(a, I32, None, "a")
    n = b._size(a)
    b_col = b.array(b_col, I32, n, "b")
    rec = b.out((b.G, 12))
    b.call("anofox_hip_categorical_test_batch", b.G, n, b.off, a, b_col, parse_categorical_test_options(options).batch_options(test), rec)
    return rec


def categorical_test_batch_host(row_offsets, a, b, test: int, options=None, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of the int32 label columns a and b; a row with
    NULL_LABEL on either side is not valid.  Returns records[n_groups, 12] = RECORD_NAMES; anofox_hip_categorical_test_batch_host's
    layout."""
    return _categorical_test_batch(HostBatch(ctx, row_offsets, None, []), a, b, test, options)


def categorical_test_batch_device(ctx, row_offsets, a, b, test: int, options=None, use_current_torch_stream: bool = True):
    """categorical_test_batch_host on CUDA tensors (row_offsets int64, a / b int32).  Asynchronous.  Returns the records tensor."""
    return _categorical_test_batch(DeviceBatch(ctx, row_offsets, None, [], use_current_torch_stream), a, b, test, options)


def categorical_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group of this family may have on the small path (one wavefront, rows in LDS); 0 restores the
    library's cap."""
    _abi.load().anofox_hip_categorical_test_hooks(int(small_cap))


# ---- the aggregates ----
CHISQ_METHOD, G_METHOD, FISHER_METHOD = "Pearson's Chi-squared test", "G-test (log-likelihood ratio)", "Fisher's exact test"
VIEWS = ("chisq_test", "g_test", "fisher_exact", "mcnemar", "cramers_v", "phi_coefficient", "contingency_coef")
_MIN_ROWS = {"chisq_test": 1, "cramers_v": 2, "g_test": 4, "fisher_exact": 4, "mcnemar": 4, "phi_coefficient": 4, "contingency_coef": 4}


def mcnemar_method(correction: bool, exact: bool) -> str:
    if exact:
        return "McNemar's exact test"
    return "McNemar's Chi-squared test" + (" with continuity correction" if correction else "")


def label_column(values) -> np.ndarray:
    """A label column of an aggregate as int32; a None or a masked entry (SQL NULL) becomes NULL_LABEL."""
    if isinstance(values, np.ma.MaskedArray):
        return np.asarray(np.ma.filled(values.astype(np.int64), NULL_LABEL), np.int32)
    a = np.asarray(values)
    if a.dtype == object:
        a = np.array([NULL_LABEL if v is None else int(v) for v in values], np.int64)
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise InvalidInputException("a label does not fit a 32-bit integer")
    return np.asarray(a, np.int32)


@dataclass
class CategoricalTestAggResult:
    """Per sorted key the record of its group, read as the aggregate `view`."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 12]: RECORD_NAMES
    view: str
    options: CategoricalTestOptions

    def row(self, g: int):
        """The reference's result of the aggregate (a STRUCT as a dict, a DOUBLE for the association measures), or None."""
        rec = self.records[g]
        if int(rec[11]) != 0 or int(rec[6]) < _MIN_ROWS[self.view]:
            return None
        if self.view == "fisher_exact":
            return {"statistic": float(rec[0]), "p_value": float(rec[1]), "odds_ratio": float(rec[0]), "conditional_odds_ratio": float(rec[3]),
                    "ci_lower": float(rec[4]), "ci_upper": float(rec[5]), "n": int(rec[6]), "method": FISHER_METHOD}
        if self.view == "mcnemar":
            o = self.options
            return {"statistic": float(rec[0]), "p_value": float(rec[1]), "df": 0 if np.isnan(rec[2]) else int(rec[2]),
                    "method": mcnemar_method(o.resolved_correction(MCNEMAR), o.exact)}
        if self.view == "cramers_v":
            return float(rec[3])
        if self.view == "contingency_coef":
            return float(rec[9])
        if self.view == "phi_coefficient":
            return None if np.isnan(rec[10]) else float(rec[10])
        return {"statistic": float(rec[0]), "p_value": float(rec[1]), "df": int(rec[2]), "method": CHISQ_METHOD if self.view == "chisq_test" else G_METHOD}

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _agg(view, test, keys, first, second, options, context) -> CategoricalTestAggResult:
    o = parse_categorical_test_options(options)
    a, b = label_column(first), label_column(second)
    if not (len(a) == len(b) == len(keys)):
        raise InvalidInputException("the keys and the two columns must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    return CategoricalTestAggResult(uniq, categorical_test_batch_host(off, a[perm], b[perm], test, o, ctx=context), view, o)


def chisq_test_agg(keys, row_var, col_var, options=None, context=None) -> CategoricalTestAggResult:
    """chisq_test_agg(row_var, col_var, options) GROUP BY keys: the chi-square test of independence of the table of the labels that
    occur; {'correction': true} applies Yates' correction to a 2 x 2 table.  A None label is a NULL: the row is not valid."""
    return _agg("chisq_test", CHI_SQUARE, keys, row_var, col_var, options, context)


def g_test_agg(keys, row_var, col_var, context=None) -> CategoricalTestAggResult:
    """g_test_agg(row_var, col_var) GROUP BY keys: the log-likelihood ratio test of independence."""
    return _agg("g_test", G_TEST, keys, row_var, col_var, None, context)


def fisher_exact_agg(keys, row_var, col_var, options=None, context=None) -> CategoricalTestAggResult:
    """fisher_exact_agg(row_var, col_var, options) GROUP BY keys: Fisher's exact test of the rows whose labels are both 0 or 1.
    `odds_ratio` is the sample odds ratio (as `statistic`), `conditional_odds_ratio` the conditional maximum-likelihood estimate
    that the interval surrounds."""
    return _agg("fisher_exact", FISHER_EXACT, keys, row_var, col_var, options, context)


def mcnemar_agg(keys, before, after, options=None, context=None) -> CategoricalTestAggResult:
    """mcnemar_agg(before, after, options) GROUP BY keys: a label of 0 against every other label; the correction is on unless
    {'correction': false}."""
    return _agg("mcnemar", MCNEMAR, keys, before, after, options, context)


def _association(view, keys, row_var, col_var, context) -> CategoricalTestAggResult:
    return _agg(view, CHI_SQUARE, keys, row_var, col_var, CategoricalTestOptions(correction=False), context)


def cramers_v_agg(keys, row_var, col_var, context=None) -> CategoricalTestAggResult:
    """cramers_v_agg(row_var, col_var) GROUP BY keys: a view of the uncorrected chi-square call."""
    return _association("cramers_v", keys, row_var, col_var, context)


def phi_coefficient_agg(keys, row_var, col_var, context=None) -> CategoricalTestAggResult:
    """phi_coefficient_agg(row_var, col_var) GROUP BY keys: the signed phi of a 2 x 2 table, by ascending label order; NULL for any
    other table."""
    return _association("phi_coefficient", keys, row_var, col_var, context)


def contingency_coef_agg(keys, row_var, col_var, context=None) -> CategoricalTestAggResult:
    """contingency_coef_agg(row_var, col_var) GROUP BY keys: Pearson's C."""
    return _association("contingency_coef", keys, row_var, col_var, context)


# ---- the scalars ----
_CHISQ_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "method")]
_RESULT_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "effect_size", "ci_lower", "ci_upper", "confidence_level", "n", "n1", "n2",
                                    "alternative", "method")]


def _counts_call(symbol, args, result, free, fields):
    """lib.<symbol>(*args, &result) of an entry that takes counts; a failure raises InvalidInputException with the library's code."""
    lib = _abi.load()
    res = result()
    try:
        call(lib, symbol, *args, C.byref(res))
    except AnofoxStatsError as failed:
        e = InvalidInputException(f"{symbol.replace('anofox_', '')} failed: {failed}")
        e.code = failed.code
        raise e from None
    if fields is None:
        return float(res.value)
    try:
        values = [(name, getattr(res, field)) for name, field in fields]
        return {name: v.decode() if isinstance(v, bytes) else v for name, v in values}
    finally:
        getattr(lib, free)(C.byref(res))


def _flat_table(table):
    """A table (rows of counts, possibly ragged) flattened row by row -> (cells, row_lengths, n_rows) as the C entries take them."""
    rows = [[int(v) for v in row] for row in table]
    if any(v < 0 for row in rows for v in row):
        raise InvalidInputException("a count is negative")
    cells = np.array([v for row in rows for v in row] or [0], np.uint64)
    lengths = np.array([len(row) for row in rows] or [0], np.uint64)
    return cells, lengths, len(rows)


def chisq_test(row_var, col_var, options=None) -> dict:
    """anofox_stats_chisq_test(row_var, col_var, {...}) through anofox_chisq_test (a batch of one group)."""
    o = parse_categorical_test_options(options)
    return scalar_call("anofox_chisq_test", (row_var, col_var), _abi.AnofoxChiSquareOptions(o.resolved_correction(CHI_SQUARE)),
                       _abi.AnofoxChiSquareResult, "anofox_free_chisq_result", _CHISQ_FIELDS)


def g_test(table) -> dict:
    """The G-test of a table of counts through anofox_g_test; no device is touched."""
    return _counts_call("anofox_g_test", _flat_table(table), _abi.AnofoxChiSquareResult, "anofox_free_chisq_result", _CHISQ_FIELDS)


def cramers_v(table) -> float:
    return _counts_call("anofox_cramers_v", _flat_table(table), C.c_double, None, None)


def contingency_coef(table) -> float:
    return _counts_call("anofox_contingency_coef", _flat_table(table), C.c_double, None, None)


def phi_coefficient(a: int, b: int, c: int, d: int) -> float:
    """phi of the table [[a, b], [c, d]] through anofox_phi_coefficient."""
    return _counts_call("anofox_phi_coefficient", (int(a), int(b), int(c), int(d)), C.c_double, None, None)


def fisher_exact(a: int, b: int, c: int, d: int, options=None) -> dict:
    """Fisher's exact test of [[a, b], [c, d]] through anofox_fisher_exact: statistic = the sample odds ratio, effect_size = the
    conditional maximum-likelihood odds ratio with its exact interval."""
    o = parse_categorical_test_options(options)
    level = NAN if o.confidence_level is None else float(o.confidence_level)
    return _counts_call("anofox_fisher_exact", (int(a), int(b), int(c), int(d), _abi.AnofoxFisherExactOptions(o.alternative, level)),
                        _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)


def mcnemar_test(a: int, b: int, c: int, d: int, options=None) -> dict:
    """McNemar's test of [[a, b], [c, d]] (b and c the discordant cells) through anofox_mcnemar_test."""
    o = parse_categorical_test_options(options)
    return _counts_call("anofox_mcnemar_test", (int(a), int(b), int(c), int(d), o.resolved_correction(MCNEMAR), bool(o.exact)),
                        _abi.AnofoxChiSquareResult, "anofox_free_chisq_result", _CHISQ_FIELDS)
