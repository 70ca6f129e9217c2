"""Grouped normality tests (csrc/normality_tests.hip): the aggregates shapiro_wilk_agg / dagostino_k2_agg / jarque_bera_agg, the
scalars shapiro_wilk / dagostino_k2 / jarque_bera through the reference-compatible symbols, and the numpy / tensor drivers of
anofox_hip_normality_test_batch_{host,device}.  The contract: DESIGN.md §1 "Normality tests".  A group whose status is not 0 (too
few rows, more than 5000 rows for Shapiro-Wilk, values that are all equal for K2 and Jarque-Bera) is None (SQL NULL) in the
aggregates."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _abi
from ._marshal import DeviceBatch, HostBatch, column, group_rows, scalar_call
from .options import InvalidInputException

SHAPIRO_WILK, DAGOSTINO_K2, JARQUE_BERA = 0, 1, 2
RECORD_NAMES = ("statistic", "p_value", "skewness", "kurtosis", "z_skewness", "z_kurtosis", "n", "status")
METHODS = ("Shapiro-Wilk test", "D'Agostino K-squared test", "Jarque-Bera test")


def _normality_test_batch(b, test):
    """records[G, 8] of the batch b, whose leading column is v."""
    rec = b.out((b.G, 8))
    b.call("anofox_hip_normality_test_batch", b.G, b.N, b.off, b.y, _abi.AnofoxHipNormalityTestBatchOptions(int(test), 0), rec)
    return rec


def normality_test_batch_host(row_offsets, v, test: int, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of v.  Returns records[n_groups, 8] = RECORD_NAMES;
    anofox_hip_normality_test_batch_host's layout."""
    return _normality_test_batch(HostBatch(ctx, row_offsets, v, [], lead="v"), test)


def normality_test_batch_device(ctx, row_offsets, v, test: int, use_current_torch_stream: bool = True):
    """normality_test_batch_host on CUDA tensors (row_offsets int64, v float64).  Asynchronous.  Returns the records tensor."""
    return _normality_test_batch(DeviceBatch(ctx, row_offsets, v, [], use_current_torch_stream, lead="v"), test)


def normality_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group of this family may have on the small path (one wavefront, rows in LDS); 0 restores the
    library's cap."""
    _abi.load().anofox_hip_normality_test_hooks(int(small_cap))


def _row(rec, test: int) -> Optional[dict]:
    """The reference's result STRUCT of the aggregate from one record, or None for a failed group."""
    if int(rec[7]) != 0:
        return None
    out = {"statistic": float(rec[0]), "p_value": float(rec[1])}
    if test != SHAPIRO_WILK:
        out.update(skewness=float(rec[2]), kurtosis=float(rec[3]))
    if test == DAGOSTINO_K2:
        out.update(z_skewness=float(rec[4]), z_kurtosis=float(rec[5]))
    out.update(n=int(rec[6]), method=METHODS[test])
    return out


@dataclass
class NormalityTestAggResult:
    """Per sorted key the record of its group."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 8]: RECORD_NAMES
    test: int

    def row(self, g: int) -> Optional[dict]:
        return _row(self.records[g], self.test)

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _agg(test, keys, value, context) -> NormalityTestAggResult:
    v = column(value)
    if len(v) != len(keys):
        raise InvalidInputException("the keys and the value column must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    return NormalityTestAggResult(uniq, normality_test_batch_host(off, v[perm], test, ctx=context), test)


def shapiro_wilk_agg(keys, value, context=None) -> NormalityTestAggResult:
    """shapiro_wilk_agg(value) GROUP BY keys: W and its p-value; a None value is a NULL, the row is not valid.  Keys of fewer than
    3 or more than 5000 valid rows are NULL; values that are all equal give W = 1, p = 1."""
    return _agg(SHAPIRO_WILK, keys, value, context)


def dagostino_k2_agg(keys, value, context=None) -> NormalityTestAggResult:
    """dagostino_k2_agg(value) GROUP BY keys: K2 with the skewness, the excess kurtosis and their z.  Keys of fewer than 8 valid
    rows, or of values that are all equal, are NULL."""
    return _agg(DAGOSTINO_K2, keys, value, context)


def jarque_bera_agg(keys, value, context=None) -> NormalityTestAggResult:
    """jarque_bera_agg(value) GROUP BY keys: JB with the skewness and the excess kurtosis.  Keys of fewer than 3 valid rows, or
    of values that are all equal, are NULL."""
    return _agg(JARQUE_BERA, keys, value, context)


_RESULT_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "effect_size", "ci_lower", "ci_upper", "confidence_level", "n", "n1", "n2",
                                    "alternative", "method")]
_JB_FIELDS = [(f, f) for f in ("statistic", "p_value", "skewness", "kurtosis", "n")]


def shapiro_wilk(data) -> dict:
    """anofox_stats_shapiro_wilk(data) through anofox_shapiro_wilk (a batch of one group)."""
    return scalar_call("anofox_shapiro_wilk", (data,), None, _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)


def dagostino_k2(data) -> dict:
    """anofox_stats_dagostino_k2(data) through anofox_dagostino_k2; df is 2."""
    return scalar_call("anofox_dagostino_k2", (data,), None, _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)


def jarque_bera(data) -> dict:
    """anofox_stats_jarque_bera(data) through anofox_jarque_bera."""
    return scalar_call("anofox_jarque_bera", (data,), None, _abi.AnofoxJarqueBeraResult, None, _JB_FIELDS)
