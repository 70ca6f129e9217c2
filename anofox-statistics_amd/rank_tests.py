"""Grouped rank-based location tests (csrc/rank_tests.hip): the aggregates mann_whitney_u_agg / wilcoxon_signed_rank_agg /
kruskal_wallis_agg, the scalars mann_whitney_u / wilcoxon_signed_rank / kruskal_wallis through the reference-compatible symbols,
and the numpy / tensor drivers of anofox_hip_rank_test_batch_{host,device}.  The contract: DESIGN.md §1 "Rank-based location
tests".  A group whose status is not 0 (an empty sample, fewer than 2 valid pairs, fewer than 3 rows or 2 samples) is None (SQL
NULL) in the aggregates.  Exact p-values and the Hodges-Lehmann interval are not built: ci_lower / ci_upper are NaN."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._marshal import I32, DeviceBatch, HostBatch, column, group_rows, scalar_call
from .options import InvalidInputException, _extract_alternative, _extract_double

MANN_WHITNEY, WILCOXON, KRUSKAL_WALLIS = 0, 1, 2
RECORD_NAMES = ("statistic", "z", "p_value", "df", "n", "n1", "n2", "status")
METHOD_TEXT = ("Mann-Whitney U test", "Wilcoxon signed-rank test", "Kruskal-Wallis H test")
NAN = float("nan")


@dataclass
class RankTestOptions:
    """Resolved options: alternative 0 two-sided, 1 less, 2 greater; continuity_correction (the reference's default: on); mu the
    hypothesised shift; confidence_level is accepted and echoed by the scalars (no interval is built)."""
    alternative: int = 0
    continuity_correction: bool = True
    mu: float = 0.0
    confidence_level: Optional[float] = 0.95

    def batch_options(self, test: int) -> "_abi.AnofoxHipRankTestBatchOptions":
        return _abi.AnofoxHipRankTestBatchOptions(int(test), self.alternative, int(bool(self.continuity_correction)), float(self.mu))

    def ffi_options(self, exact: bool = False):
        level = NAN if self.confidence_level is None else float(self.confidence_level)
        return _abi.AnofoxMannWhitneyOptions(self.alternative, bool(exact), bool(self.continuity_correction), level, float(self.mu))


def _extract_bool(val) -> bool:
    if isinstance(val, str):
        name = val.strip().lower()
        if name in ("true", "t", "1", "yes"):
            return True
        if name in ("false", "f", "0", "no"):
            return False
        raise InvalidInputException("Unknown boolean '%s'" % (val,))
    return bool(val)


def parse_rank_test_options(opts) -> RankTestOptions:
    """The MAP options of the aggregates: alternative (the spellings correlation accepts), continuity_correction | correction,
    mu, confidence_level.  Keys and values are case-insensitive; other keys are ignored."""
    if isinstance(opts, RankTestOptions):
        return opts
    out = RankTestOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "alternative" and val is not None:
            out.alternative = _extract_alternative(val)
        elif key in ("continuity_correction", "correction") and val is not None:
            out.continuity_correction = _extract_bool(val)
        elif key == "mu" and val is not None:
            out.mu = _extract_double(val)
        elif key == "confidence_level":
            out.confidence_level = _extract_double(val)
    return out


def _rank_test_batch(b, y, sample, test, options):
    """records[G, 8] of the batch b, whose leading column is v."""
    rec = b.out((b.G, 8))
    b.call("anofox_hip_rank_test_batch", b.G, b.N, b.off, b.y, b.rows(y, "y"), b.rows(sample, "sample", I32),
           parse_rank_test_options(options).batch_options(test), rec)
    return rec


def rank_test_batch_host(row_offsets, v, y, sample, test: int, options=None, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of v, of y (Wilcoxon, else None) and of the int32
    sample ids (Mann-Whitney and Kruskal-Wallis, else None).  Returns records[n_groups, 8] = RECORD_NAMES;
    anofox_hip_rank_test_batch_host's layout."""
    return _rank_test_batch(HostBatch(ctx, row_offsets, v, [], lead="v"), y, sample, test, options)


def rank_test_batch_device(ctx, row_offsets, v, y, sample, test: int, options=None, use_current_torch_stream: bool = True):
    """rank_test_batch_host on CUDA tensors (row_offsets int64, v / y float64, sample int32).  Asynchronous.  Returns the records
    tensor."""
    return _rank_test_batch(DeviceBatch(ctx, row_offsets, v, [], use_current_torch_stream, lead="v"), y, sample, test, options)


def rank_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group may have on the small path (one wavefront, rows in LDS); 0 restores the library's cap."""
    _abi.load().anofox_hip_rank_test_hooks(int(small_cap))


@dataclass
class RankTestAggResult:
    """Per sorted key the record of its group."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 8]: RECORD_NAMES
    test: int

    def row(self, g: int) -> Optional[dict]:
        """The reference's result STRUCT of the aggregate, or None for a failed group."""
        rec = self.records[g]
        if int(rec[7]) != 0:
            return None
        out = {"statistic": float(rec[0]), "p_value": float(rec[2])}
        if self.test == MANN_WHITNEY:
            out.update(effect_size=NAN, ci_lower=NAN, ci_upper=NAN, n1=int(rec[5]), n2=int(rec[6]))
        elif self.test == WILCOXON:
            out.update(ci_lower=NAN, ci_upper=NAN, n=int(rec[4]))
        else:
            out.update(df=float(rec[3]), n=int(rec[4]))
        out["method"] = METHOD_TEXT[self.test]
        return out

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _sample_column(sample, v):
    """The int32 sample ids; a None (NULL) id makes its row invalid: the value becomes NaN."""
    a = np.asarray(sample)
    if a.dtype == object:
        null = np.array([s is None for s in sample], bool)
        v = np.where(null, np.nan, v)
        a = np.array([0 if s is None else s for s in sample])
    return np.asarray(a, np.int32), v


def _agg(test, keys, v, y, sample, options, context) -> RankTestAggResult:
    o = parse_rank_test_options(options)
    vv = column(v)
    yv = sv = None
    if test == WILCOXON:
        yv = column(y)
    else:
        sv, vv = _sample_column(sample, vv)
    second = yv if sv is None else sv
    if not (len(vv) == len(second) == len(keys)):
        raise InvalidInputException("the keys and the two columns must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    rec = rank_test_batch_host(off, vv[perm], None if yv is None else yv[perm], None if sv is None else sv[perm], test, o, ctx=context)
    return RankTestAggResult(uniq, rec, test)


def mann_whitney_u_agg(keys, value, sample, options=None, context=None) -> RankTestAggResult:
    """mann_whitney_u_agg(value, sample, options) GROUP BY keys: sample 0 against every other id.  A None value or id is a NULL:
    the row is not valid."""
    return _agg(MANN_WHITNEY, keys, value, None, sample, options, context)


def wilcoxon_signed_rank_agg(keys, x, y, options=None, context=None) -> RankTestAggResult:
    """wilcoxon_signed_rank_agg(x, y, options) GROUP BY keys, on the paired differences x - y."""
    return _agg(WILCOXON, keys, x, y, None, options, context)


def kruskal_wallis_agg(keys, value, sample, context=None) -> RankTestAggResult:
    """kruskal_wallis_agg(value, sample) GROUP BY keys; the sample ids are any int32."""
    return _agg(KRUSKAL_WALLIS, keys, value, None, sample, None, context)


_RESULT_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "effect_size", "ci_lower", "ci_upper", "confidence_level", "n", "n1", "n2",
                                    "alternative", "method")]


def _scalar(symbol, a, b, ffi_options) -> dict:
    return scalar_call(symbol, (a, b), ffi_options, _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)


def _exact(options) -> bool:
    return isinstance(options, Mapping) and any(str(k).lower() == "exact" and v is not None and _extract_bool(v) for k, v in options.items())


def mann_whitney_u(group1, group2, options=None) -> dict:
    """anofox_stats_mann_whitney_u(group1, group2, {...}) through anofox_mann_whitney_u (a batch of one group)."""
    return _scalar("anofox_mann_whitney_u", group1, group2, parse_rank_test_options(options).ffi_options(_exact(options)))


def wilcoxon_signed_rank(x, y, options=None) -> dict:
    """anofox_stats_wilcoxon_signed_rank(x, y, {...}) through anofox_wilcoxon_signed_rank."""
    o = parse_rank_test_options(options).ffi_options(_exact(options))
    return _scalar("anofox_wilcoxon_signed_rank", x, y, _abi.AnofoxWilcoxonOptions(o.alternative, o.exact, o.continuity_correction,
                                                                                    o.confidence_level, o.mu))


def kruskal_wallis(values, groups) -> dict:
    """anofox_stats_kruskal_wallis(values, groups) through anofox_kruskal_wallis; the group ids go as doubles, as in the reference."""
    return _scalar("anofox_kruskal_wallis", values, groups, None)
