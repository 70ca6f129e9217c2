"""Grouped parametric and studentised-rank tests (csrc/sample_tests.hip): the aggregates t_test_agg / paired_t_test_agg / yuen_agg /
one_way_anova_agg / brown_forsythe_agg / brunner_munzel_agg, the scalars t_test / yuen / brunner_munzel / one_way_anova /
brown_forsythe through the reference-compatible symbols (paired_t_test: a batch of one group), and the numpy / tensor drivers of
anofox_hip_sample_test_batch_{host,device}.  The contract: DESIGN.md §1 "Parametric and studentised-rank tests".  A group whose
status is not 0 (an arm with too few rows, fewer than 2 valid pairs, fewer than 2 arms) is None (SQL NULL) in the aggregates."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._marshal import I32, DeviceBatch, HostBatch, column, group_rows, scalar_call
from .options import InvalidInputException, _extract_alternative, _extract_double
from .rank_tests import _extract_bool, _sample_column

T_TEST, YUEN, ANOVA, BROWN_FORSYTHE, BRUNNER_MUNZEL = 0, 1, 2, 3, 4
WELCH, STUDENT, PAIRED = 0, 1, 2       # the t-test's kinds
FISHER, WELCH_ANOVA = 0, 1             # ANOVA's kinds
RECORD_NAMES = ("statistic", "p_value", "df", "df2", "estimate", "ci_lower", "ci_upper", "n", "n1", "n2", "aux", "status")
T_KINDS = {"welch": WELCH, "student": STUDENT, "paired": PAIRED}
ANOVA_KINDS = {"fisher": FISHER, "welch": WELCH_ANOVA}
NAN = float("nan")


@dataclass
class SampleTestOptions:
    """Resolved options: alternative 0 two-sided, 1 less, 2 greater; kind (the t-test: 0 Welch, 1 Student, 2 paired; ANOVA: 0 Fisher,
    1 Welch); mu the t-test's hypothesised difference; trim Yuen's proportion; confidence_level (None: no interval)."""
    alternative: int = 0
    kind: int = 0
    mu: float = 0.0
    trim: float = 0.2
    confidence_level: Optional[float] = 0.95

    def batch_options(self, test: int) -> "_abi.AnofoxHipSampleTestBatchOptions":
        level = NAN if self.confidence_level is None else float(self.confidence_level)
        return _abi.AnofoxHipSampleTestBatchOptions(int(test), self.alternative, self.kind, float(self.mu), float(self.trim), level)

    def method(self, test: int) -> str:
        if test == T_TEST:
            return ("Welch t-test", "Student t-test", "Paired t-test")[self.kind]
        if test == YUEN:
            return "Yuen test (trim=%.2f)" % self.trim
        if test == ANOVA:
            return ("Fisher One-way ANOVA", "Welch One-way ANOVA")[self.kind]
        return "Brown-Forsythe test" if test == BROWN_FORSYTHE else "Brunner-Munzel test"


def parse_sample_test_options(opts, test: int = T_TEST) -> SampleTestOptions:
    """The MAP options of the aggregates: alternative (the spellings correlation accepts), kind (`welch | student | paired` for
    the t-test, `fisher | welch` for ANOVA), var_equal (true: student), mu, trim, confidence_level.  Keys and values are
    case-insensitive; other keys are ignored."""
    if isinstance(opts, SampleTestOptions):
        return opts
    out = SampleTestOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    kinds = ANOVA_KINDS if test == ANOVA else T_KINDS
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "alternative" and val is not None:
            out.alternative = _extract_alternative(val)
        elif key == "kind" and val is not None:
            name = str(val).strip().lower()
            if name not in kinds:
                raise InvalidInputException("Unknown kind '%s'. Expected %s." % (val, " or ".join("'%s'" % k for k in kinds)))
            out.kind = kinds[name]
        elif key == "var_equal" and val is not None:
            out.kind = STUDENT if _extract_bool(val) else WELCH
        elif key == "mu" and val is not None:
            out.mu = _extract_double(val)
        elif key == "trim" and val is not None:
            out.trim = _extract_double(val)
        elif key == "confidence_level":
            out.confidence_level = _extract_double(val)
    return out


def _sample_test_batch(b, y, sample, test, options):
    """records[G, 12] of the batch b, whose leading column is v."""
    rec = b.out((b.G, 12))
    b.call("anofox_hip_sample_test_batch", b.G, b.N, b.off, b.y, b.rows(y, "y"), b.rows(sample, "sample", I32),
           parse_sample_test_options(options, test).batch_options(test), rec)
    return rec


def sample_test_batch_host(row_offsets, v, y, sample, test: int, options=None, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of v, of y (the paired t-test, else None) and of the
    int32 sample ids (every other test, else None).  Returns records[n_groups, 12] = RECORD_NAMES;
    anofox_hip_sample_test_batch_host's layout."""
    return _sample_test_batch(HostBatch(ctx, row_offsets, v, [], lead="v"), y, sample, test, options)


def sample_test_batch_device(ctx, row_offsets, v, y, sample, test: int, options=None, use_current_torch_stream: bool = True):
    """sample_test_batch_host on CUDA tensors (row_offsets int64, v / y float64, sample int32).  Asynchronous.  Returns the records
    tensor."""
    return _sample_test_batch(DeviceBatch(ctx, row_offsets, v, [], use_current_torch_stream, lead="v"), y, sample, test, options)


def sample_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group of this family may have on the small path (one wavefront, rows in LDS); 0 restores the
    library's cap."""
    _abi.load().anofox_hip_sample_test_hooks(int(small_cap))


def _row(rec, test: int, method: str) -> Optional[dict]:
    """The reference's result STRUCT of the aggregate from one record, or None for a failed group."""
    if int(rec[11]) != 0:
        return None
    if test == ANOVA:
        return {"f_statistic": float(rec[0]), "p_value": float(rec[1]), "df_between": int(rec[2]),
                "df_within": int(rec[3]) if float(rec[3]).is_integer() else float(rec[3]),   # (Welch's is not a count)
                "ss_between": float(rec[4]), "ss_within": float(rec[10]), "n_groups": int(rec[8]), "n": int(rec[7]), "method": method}
    out = {"statistic": float(rec[0]), "p_value": float(rec[1]), "df": float(rec[2])}
    if test == BROWN_FORSYTHE:
        out.update(n=int(rec[7]))
    else:
        out.update(effect_size=float(rec[4]) if test == BRUNNER_MUNZEL else NAN, ci_lower=float(rec[5]), ci_upper=float(rec[6]),
                   n1=int(rec[8]), n2=int(rec[9]))
    out["method"] = method
    return out


@dataclass
class SampleTestAggResult:
    """Per sorted key the record of its group."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 12]: RECORD_NAMES
    test: int
    method: str

    def row(self, g: int) -> Optional[dict]:
        return _row(self.records[g], self.test, self.method)

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _agg(test, keys, v, y, sample, options, context) -> SampleTestAggResult:
    o = parse_sample_test_options(options, test)
    vv = column(v)
    yv = sv = None
    if y is not None:
        yv = column(y)
    else:
        sv, vv = _sample_column(sample, vv)
    second = yv if sv is None else sv
    if not (len(vv) == len(second) == len(keys)):
        raise InvalidInputException("the keys and the two columns must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    rec = sample_test_batch_host(off, vv[perm], None if yv is None else yv[perm], None if sv is None else sv[perm], test, o, ctx=context)
    return SampleTestAggResult(uniq, rec, test, o.method(test))


def _not_paired(o: SampleTestOptions) -> SampleTestOptions:
    if o.kind == PAIRED:
        raise InvalidInputException("the paired t-test takes two value columns: paired_t_test_agg / paired_t_test")
    return o


def t_test_agg(keys, value, arm, options=None, context=None) -> SampleTestAggResult:
    """t_test_agg(value, group_id, options) GROUP BY keys: arm 0 against every other id; Welch unless kind / var_equal says
    Student.  A None value or id is a NULL: the row is not valid."""
    return _agg(T_TEST, keys, value, None, arm, _not_paired(parse_sample_test_options(options)), context)


def paired_t_test_agg(keys, before, after, options=None, context=None) -> SampleTestAggResult:
    """The paired t-test of the differences before - after GROUP BY keys."""
    o = parse_sample_test_options(options)
    return _agg(T_TEST, keys, before, after, None, SampleTestOptions(o.alternative, PAIRED, o.mu, o.trim, o.confidence_level), context)


def yuen_agg(keys, value, arm, options=None, context=None) -> SampleTestAggResult:
    """yuen_agg(value, group_id, options) GROUP BY keys: Yuen's trimmed-mean test (trim 0.2 unless given)."""
    return _agg(YUEN, keys, value, None, arm, options, context)


def one_way_anova_agg(keys, value, arm, options=None, context=None) -> SampleTestAggResult:
    """one_way_anova_agg(value, group_id) GROUP BY keys; the ids are any int32; kind `welch` for unequal variances."""
    return _agg(ANOVA, keys, value, None, arm, options, context)


def brown_forsythe_agg(keys, value, arm, context=None) -> SampleTestAggResult:
    """brown_forsythe_agg(value, group_id) GROUP BY keys: the median-centred Levene test."""
    return _agg(BROWN_FORSYTHE, keys, value, None, arm, None, context)


def brunner_munzel_agg(keys, value, arm, options=None, context=None) -> SampleTestAggResult:
    """brunner_munzel_agg(value, group_id, options) GROUP BY keys; effect_size is phat."""
    return _agg(BRUNNER_MUNZEL, keys, value, None, arm, options, context)


_RESULT_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "effect_size", "ci_lower", "ci_upper", "confidence_level", "n", "n1", "n2",
                                    "alternative", "method")]
_ANOVA_FIELDS = [(f, f) for f in ("f_statistic", "p_value", "df_between", "df_within", "ss_between", "ss_within", "n_groups", "n", "method")]


def _level(o: SampleTestOptions) -> float:
    return NAN if o.confidence_level is None else float(o.confidence_level)


def _scalar(symbol, a, b, ffi_options) -> dict:
    return scalar_call(symbol, (a, b), ffi_options, _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)


def t_test(group1, group2, options=None) -> dict:
    """anofox_stats_t_test(group1, group2, {...}) through anofox_t_test (a batch of one group)."""
    o = _not_paired(parse_sample_test_options(options))
    return _scalar("anofox_t_test", group1, group2, _abi.AnofoxTTestOptions(o.alternative, _level(o), o.kind == STUDENT, float(o.mu)))


def paired_t_test(before, after, options=None) -> dict:
    """The paired t-test of before - after: one group through the host batch entry; the record's fields, or an
    InvalidInputException below 2 valid pairs."""
    b, a = column(before), column(after)
    if len(b) != len(a):
        raise InvalidInputException("paired t-test requires equal length samples")
    o = parse_sample_test_options(options)
    o = SampleTestOptions(o.alternative, PAIRED, o.mu, o.trim, o.confidence_level)
    rec = sample_test_batch_host(np.array([0, len(b)], np.int64), b, a, None, T_TEST, o)[0]
    if int(rec[11]) != 0:
        raise InvalidInputException("paired t-test requires at least 2 valid pairs")
    out = _row(rec, T_TEST, o.method(T_TEST))
    out.update(n=int(rec[7]), confidence_level=_level(o), alternative=o.alternative, estimate=float(rec[4]))
    return out


def yuen(group1, group2, options=None) -> dict:
    """anofox_stats_yuen(group1, group2, {...}) through anofox_yuen_test."""
    o = parse_sample_test_options(options, YUEN)
    return _scalar("anofox_yuen_test", group1, group2, (float(o.trim), o.alternative, _level(o)))


def brunner_munzel(group1, group2, options=None) -> dict:
    """anofox_stats_brunner_munzel(group1, group2, {...}) through anofox_brunner_munzel; effect_size is phat."""
    o = parse_sample_test_options(options, BRUNNER_MUNZEL)
    return _scalar("anofox_brunner_munzel", group1, group2, _abi.AnofoxBrunnerMunzelOptions(o.alternative, _level(o)))


def one_way_anova(values, groups) -> dict:
    """anofox_stats_one_way_anova(values, groups) through anofox_one_way_anova; the group ids go as doubles, as in the reference."""
    return scalar_call("anofox_one_way_anova", (values, groups), None, _abi.AnofoxAnovaResult, "anofox_free_anova_result", _ANOVA_FIELDS)


def brown_forsythe(values, groups) -> dict:
    """anofox_stats_brown_forsythe(values, groups) through anofox_brown_forsythe."""
    return _scalar("anofox_brown_forsythe", values, groups, None)
