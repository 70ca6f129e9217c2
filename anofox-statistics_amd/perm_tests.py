"""Grouped permutation tests (csrc/perm_tests.hip): the aggregates energy_distance_agg / mmd_agg / permutation_t_test_agg, the
scalars energy_distance / mmd / permutation_t_test through the reference-compatible symbols, and the numpy / tensor drivers of
anofox_hip_perm_test_batch_{host,device}.  The contract, the permutation stream and what differs from the reference: DESIGN.md §1
"Permutation tests".  A group whose status is not 0 (fewer than 2 rows in a sample, an infinity, an MMD group above 1462 rows) is
None (SQL NULL) in the aggregates.  A seed of None is drawn here and reported, so that a result can be reproduced."""
from __future__ import annotations

import secrets
from dataclasses import dataclass
from typing import Mapping, Optional

import numpy as np

from . import _abi
from ._marshal import I32, DeviceBatch, HostBatch, column, group_rows, scalar_call
from .options import InvalidInputException, _extract_alternative, _extract_double
from .rank_tests import _sample_column

ENERGY_DISTANCE, PERMUTATION_T_TEST, MMD = 0, 1, 2
RECORD_NAMES = ("statistic", "p_value", "aux", "n_extreme", "n", "n1", "n2", "status")
METHOD_TEXT = ("Energy distance test (%d permutations)", "Permutation t-test (%d permutations)",
               "MMD test (Gaussian kernel, %d permutations)")
DEFAULT_PERMUTATIONS = (1000, 10000, 1000)   # the reference's documented defaults
MAX_PERMUTATIONS = 1000000
NAN = float("nan")


@dataclass
class PermTestOptions:
    """Resolved options: n_permutations (None: 1000, for the t-test 10000); seed (None: drawn per call and reported); sigma, MMD's
    kernel width (None: the median heuristic); alternative 0 two-sided, 1 less, 2 greater (the t-test alone)."""
    n_permutations: Optional[int] = None
    seed: Optional[int] = None
    sigma: Optional[float] = None
    alternative: int = 0

    def permutations(self, test: int) -> int:
        return DEFAULT_PERMUTATIONS[test] if self.n_permutations is None else int(self.n_permutations)

    def resolved(self) -> "PermTestOptions":
        """These options with a seed."""
        seed = secrets.randbits(64) if self.seed is None else int(self.seed) & 0xFFFFFFFFFFFFFFFF
        return PermTestOptions(self.n_permutations, seed, self.sigma, self.alternative)

    def batch_options(self, test: int) -> "_abi.AnofoxHipPermTestBatchOptions":
        if self.seed is None:
            raise InvalidInputException("permutation test: the batch entries need a seed")
        n = self.permutations(test)
        if n < 0 or n > MAX_PERMUTATIONS:
            raise InvalidInputException("permutation test: n_permutations must be within [0, 1000000]")
        return _abi.AnofoxHipPermTestBatchOptions(int(test), self.alternative, n, int(self.seed) & 0xFFFFFFFFFFFFFFFF,
                                                  NAN if self.sigma is None else float(self.sigma))


def parse_perm_test_options(opts) -> PermTestOptions:
    """The MAP options of the aggregates: n_permutations, seed, sigma, alternative.  Keys and values are case-insensitive; other
    keys are ignored."""
    if isinstance(opts, PermTestOptions):
        return opts
    out = PermTestOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if val is None:
            continue
        if key == "alternative":
            out.alternative = _extract_alternative(val)
        elif key == "n_permutations":
            out.n_permutations = int(val)
        elif key == "seed":
            out.seed = int(val)
        elif key == "sigma":
            out.sigma = _extract_double(val)
    return out


def _perm_test_batch(b, sample, test, options):
    """records[G, 8] of the batch b, whose leading column is v."""
    rec = b.out((b.G, 8))
    b.call("anofox_hip_perm_test_batch", b.G, b.N, b.off, b.y, b.rows(sample, "sample", I32),
           parse_perm_test_options(options).batch_options(test), rec)
    return rec


def perm_test_batch_host(row_offsets, v, sample, test: int, options=None, ctx=None) -> np.ndarray:
    """numpy in / out: group g owns rows [row_offsets[g], row_offsets[g + 1]) of v and of the int32 sample ids (0: sample 1).
    The options need a seed.  Returns records[n_groups, 8] = RECORD_NAMES; anofox_hip_perm_test_batch_host's layout."""
    return _perm_test_batch(HostBatch(ctx, row_offsets, v, [], lead="v"), sample, test, options)


def perm_test_batch_device(ctx, row_offsets, v, sample, test: int, options=None, use_current_torch_stream: bool = True):
    """perm_test_batch_host on CUDA tensors (row_offsets int64, v float64, sample int32).  Asynchronous.  Returns the records
    tensor."""
    return _perm_test_batch(DeviceBatch(ctx, row_offsets, v, [], use_current_torch_stream, lead="v"), sample, test, options)


def perm_test_hooks(small_cap: int = 0):
    """For tests: the most rows a group may have on the small path (one wavefront, rows in LDS); 0 restores the library's cap."""
    _abi.load().anofox_hip_perm_test_hooks(int(small_cap))


@dataclass
class PermTestAggResult:
    """Per sorted key the record of its group; `options` carry the seed the call ran with."""
    keys: np.ndarray
    records: np.ndarray   # [n_groups, 8]: RECORD_NAMES
    test: int
    options: PermTestOptions

    def row(self, g: int) -> Optional[dict]:
        """The result STRUCT of the aggregate, or None for a failed group."""
        rec = self.records[g]
        if int(rec[7]) != 0:
            return None
        out = {"statistic": float(rec[0]), "p_value": float(rec[1]), "n_extreme": int(rec[3]), "n1": int(rec[5]), "n2": int(rec[6]),
               "n": int(rec[4]), "seed": self.options.seed, "method": METHOD_TEXT[self.test] % self.options.permutations(self.test)}
        if self.test == MMD:
            out["sigma"] = float(rec[2])
        elif self.test == PERMUTATION_T_TEST:
            out["df"] = float(rec[2])
        return out

    def by_key(self) -> dict:
        return {k: self.row(g) for g, k in enumerate(self.keys.tolist())}


def _agg(test, keys, value, arm, options, context) -> PermTestAggResult:
    o = parse_perm_test_options(options).resolved()
    sv, vv = _sample_column(arm, column(value))
    if not (len(vv) == len(sv) == len(keys)):
        raise InvalidInputException("the keys and the two columns must have the same number of rows")
    uniq, perm, off = group_rows(keys)
    return PermTestAggResult(uniq, perm_test_batch_host(off, vv[perm], sv[perm], test, o, ctx=context), test, o)


def energy_distance_agg(keys, value, arm, options=None, context=None) -> PermTestAggResult:
    """energy_distance_agg(value, arm, options) GROUP BY keys: arm 0 against every other id.  A None value or id is a NULL: the row
    is not valid."""
    return _agg(ENERGY_DISTANCE, keys, value, arm, options, context)


def mmd_agg(keys, value, arm, options=None, context=None) -> PermTestAggResult:
    """mmd_agg(value, arm, options) GROUP BY keys, the Gaussian kernel; a group of more than 1462 rows is None."""
    return _agg(MMD, keys, value, arm, options, context)


def permutation_t_test_agg(keys, value, arm, options=None, context=None) -> PermTestAggResult:
    """permutation_t_test_agg(value, arm, options) GROUP BY keys: Welch's t with a permutation p-value."""
    return _agg(PERMUTATION_T_TEST, keys, value, arm, options, context)


_RESULT_FIELDS = [(f, f) for f in ("statistic", "p_value", "df", "effect_size", "n", "n1", "n2", "alternative", "method")]


def _scalar(test, symbol, g1, g2, options) -> dict:
    o = parse_perm_test_options(options).resolved()
    n = o.permutations(test)
    if n < 0:
        raise InvalidInputException("permutation test: n_permutations must be within [0, 1000000]")
    if test == PERMUTATION_T_TEST:
        ffi = (o.alternative, n, o.seed, True)
    else:
        ffi = (_abi.AnofoxEnergyDistanceOptions if test == ENERGY_DISTANCE else _abi.AnofoxMmdOptions)(n, o.seed, True)
    out = scalar_call(symbol, (g1, g2), ffi, _abi.AnofoxTestResult, "anofox_free_test_result", _RESULT_FIELDS)
    p = out["p_value"]
    out["n_extreme"] = int(round(p * (n + 1))) - 1 if p == p else 0
    out["seed"] = o.seed
    return out


def energy_distance(group1, group2, options=None) -> dict:
    """anofox_stats_energy_distance(group1, group2, {...}) through anofox_energy_distance (a batch of one group)."""
    return _scalar(ENERGY_DISTANCE, "anofox_energy_distance", group1, group2, options)


def mmd(group1, group2, options=None) -> dict:
    """anofox_stats_mmd(group1, group2, {...}) through anofox_mmd: the median heuristic's sigma (the symbol takes none)."""
    return _scalar(MMD, "anofox_mmd", group1, group2, options)


def permutation_t_test(group1, group2, options=None) -> dict:
    """anofox_stats_permutation_t_test(group1, group2, {...}) through anofox_permutation_t_test; df is Welch's."""
    return _scalar(PERMUTATION_T_TEST, "anofox_permutation_t_test", group1, group2, options)
