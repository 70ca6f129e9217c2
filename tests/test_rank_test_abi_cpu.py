"""CPU-side checks of the rank test surface: the header compiles as C, the struct layouts (the reference's ABI), the exported
symbols, the option spellings, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

SYMBOLS = ("anofox_hip_rank_test_record_len", "anofox_hip_rank_test_batch_device", "anofox_hip_rank_test_batch_host",
           "anofox_hip_rank_test_hooks", "anofox_mann_whitney_u", "anofox_wilcoxon_signed_rank", "anofox_kruskal_wallis",
           "anofox_free_test_result")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)
_SP = C.POINTER(C.c_int32)
NAN = float("nan")


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_rank_test_record_len() == 8
    pkg = import_pkg()
    for name in ("mann_whitney_u", "wilcoxon_signed_rank", "kruskal_wallis", "mann_whitney_u_agg", "wilcoxon_signed_rank_agg",
                 "kruskal_wallis_agg"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.SQL_FUNCTIONS["anofox_stats_" + name] is getattr(pkg, name) and name in pkg.__all__
    for name in ("rank_test_batch_host", "rank_test_batch_device", "rank_test_hooks", "parse_rank_test_options"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.rank_test_batch_host) and callable(pkg.Context.rank_test_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(AnofoxTestResult), sizeof(AnofoxMannWhitneyOptions), sizeof(AnofoxWilcoxonOptions),
         sizeof(AnofoxHipRankTestBatchOptions));
  O(AnofoxTestResult, statistic); O(AnofoxTestResult, p_value); O(AnofoxTestResult, df); O(AnofoxTestResult, effect_size);
  O(AnofoxTestResult, ci_lower); O(AnofoxTestResult, ci_upper); O(AnofoxTestResult, confidence_level); O(AnofoxTestResult, n);
  O(AnofoxTestResult, n1); O(AnofoxTestResult, n2); O(AnofoxTestResult, alternative); O(AnofoxTestResult, method);
  printf("\n");
  O(AnofoxMannWhitneyOptions, alternative); O(AnofoxMannWhitneyOptions, exact); O(AnofoxMannWhitneyOptions, continuity_correction);
  O(AnofoxMannWhitneyOptions, confidence_level); O(AnofoxMannWhitneyOptions, mu);
  O(AnofoxWilcoxonOptions, alternative); O(AnofoxWilcoxonOptions, exact); O(AnofoxWilcoxonOptions, continuity_correction);
  O(AnofoxWilcoxonOptions, confidence_level); O(AnofoxWilcoxonOptions, mu);
  printf("\n");
  O(AnofoxHipRankTestBatchOptions, test); O(AnofoxHipRankTestBatchOptions, alternative);
  O(AnofoxHipRankTestBatchOptions, continuity_correction); O(AnofoxHipRankTestBatchOptions, mu);
  printf("\n");
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    # the layouts of src/include/anofox_stats_ffi.h:1555-1583, 1696-1707, 1920-1931 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [96, 24, 24, 24]
    assert [int(v) for v in out[1].split()] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88]
    assert [int(v) for v in out[2].split()] == [0, 4, 5, 8, 16] * 2
    assert [int(v) for v in out[3].split()] == [0, 4, 8, 16]
    abi = import_pkg("_abi")
    assert [C.sizeof(t) for t in (abi.AnofoxTestResult, abi.AnofoxMannWhitneyOptions, abi.AnofoxWilcoxonOptions,
                                  abi.AnofoxHipRankTestBatchOptions)] == [96, 24, 24, 24]
    assert [getattr(abi.AnofoxTestResult, f).offset for f, _ in abi.AnofoxTestResult._fields_] == list(range(0, 96, 8))
    for t in (abi.AnofoxMannWhitneyOptions, abi.AnofoxWilcoxonOptions):
        assert [getattr(t, f).offset for f, _ in t._fields_] == [0, 4, 5, 8, 16]
    assert [getattr(abi.AnofoxHipRankTestBatchOptions, f).offset for f, _ in abi.AnofoxHipRankTestBatchOptions._fields_] == [0, 4, 8, 16]


def test_option_spellings():
    pkg = import_pkg()
    P = pkg.parse_rank_test_options
    d = P(None)
    assert (d.alternative, d.continuity_correction, d.mu, d.confidence_level) == (0, True, 0.0, 0.95)
    for name, code in (("two_sided", 0), ("Two-Sided", 0), ("two.sided", 0), ("LESS", 1), ("greater", 2)):
        assert P({"alternative": name}).alternative == code and P({"ALTERNATIVE": name}).alternative == code
    for key in ("continuity_correction", "correction", "Correction"):
        assert P({key: False}).continuity_correction is False and P({key: "true"}).continuity_correction is True
    assert P({"mu": 0.5, "confidence_level": 0.9, "something_else": 3}).mu == 0.5 and P({"confidence_level": 0.9}).confidence_level == 0.9
    o = P({"alternative": "less", "correction": False, "mu": -1.5})
    b, f = o.batch_options(1), o.ffi_options()
    assert (b.test, b.alternative, b.continuity_correction, b.mu) == (1, 1, 0, -1.5)
    assert (f.alternative, f.exact, f.continuity_correction, f.confidence_level, f.mu) == (1, False, False, 0.95, -1.5)
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown alternative 'sideways'"):
        P({"alternative": "sideways"})


def _batch(lib, abi, n_groups=1, n_rows=4, off=(0, 4), v=True, y=True, sample=True, records=True, offsets=True, options=(0, 0, 1, 0.0)):
    o = np.array(off, np.int64)
    vv, yv, sv, rec = np.ones(64), np.ones(64), np.zeros(64, np.int32), np.zeros(64)
    err = abi.AnofoxError()
    p = lambda a, on: a.ctypes.data_as(_DP) if on else None   # noqa: E731
    ok = lib.anofox_hip_rank_test_batch_host(None, n_groups, n_rows, o.ctypes.data_as(_IP) if offsets else None, p(vv, v), p(yv, y),
                                             sv.ctypes.data_as(_SP) if sample else None, abi.AnofoxHipRankTestBatchOptions(*options),
                                             p(rec, records), C.byref(err))
    return ok, err.code, err.text()


@pytest.mark.parametrize("kw, text", [
    (dict(v=False), "rank test: row_offsets, v or records is NULL"), (dict(records=False), "rank test: row_offsets, v or records is NULL"),
    (dict(offsets=False), "rank test: row_offsets, v or records is NULL"),
    (dict(y=False, options=(1, 0, 1, 0.0)), "rank test: the Wilcoxon signed-rank test needs the y column"),
    (dict(sample=False), "rank test: the Mann-Whitney and Kruskal-Wallis tests need the sample column"),
    (dict(sample=False, options=(2, 0, 0, 0.0)), "rank test: the Mann-Whitney and Kruskal-Wallis tests need the sample column"),
    (dict(off=(0, 3, 2), n_groups=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"), (dict(off=(-1, 4)), "non-decreasing"),
    (dict(n_groups=-1), "negative"), (dict(n_rows=-1), "negative"),
    (dict(options=(3, 0, 1, 0.0)), "rank test: unknown test"), (dict(options=(-1, 0, 1, 0.0)), "rank test: unknown test"),
    (dict(options=(0, 3, 1, 0.0)), "rank test: unknown alternative"), (dict(options=(1, -1, 1, 0.0)), "rank test: unknown alternative"),
    (dict(options=(0, 0, 1, NAN)), "rank test: mu must be finite"), (dict(options=(1, 0, 1, float("inf"))), "rank test: mu must be finite"),
    (dict(options=(2, 0, 0, 0.5)), "rank test: the Kruskal-Wallis test takes no mu")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first_and_an_empty_call_succeeds():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    good, bad = abi.AnofoxHipRankTestBatchOptions(0, 0, 1, 0.0), abi.AnofoxHipRankTestBatchOptions(5, 0, 1, 0.0)
    assert not lib.anofox_hip_rank_test_batch_device(None, 1, 4, None, None, None, None, good, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_rank_test_batch_device(None, 1, 4, 8, 8, 8, 8, bad, 8, C.byref(err)) and "rank test: unknown test" in err.text()
    assert not lib.anofox_hip_rank_test_batch_device(None, 1, 4, 8, 8, None, None, good, 8, C.byref(err)) and "sample column" in err.text()
    assert not lib.anofox_hip_rank_test_batch_device(None, 1, 4, 8, 8, None, 8, good, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_rank_test_batch_host(None, 0, 0, None, None, None, None, good, None, C.byref(err)) and err.code == 0   # nothing to do
    lib.anofox_hip_rank_test_hooks(128)
    lib.anofox_hip_rank_test_hooks(0)


def _array(abi, values):
    a = np.asarray(values, np.float64)
    return abi.AnofoxDataArray(a.ctypes.data_as(_DP), None, len(a)), a


def _scalar(abi, symbol, a, b, options):
    res, err = abi.AnofoxTestResult(), abi.AnofoxError()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    (aa, k0), (ba, k1) = _array(abi, a), _array(abi, b)
    args = (aa, ba, C.byref(res), C.byref(err)) if options is None else (aa, ba, options, C.byref(res), C.byref(err))
    return getattr(abi.load(), symbol)(*args), res, err


def test_scalar_failures_leave_the_result_zeroed():
    abi = import_pkg("_abi")
    mw = lambda alt=0, exact=False, mu=0.0: abi.AnofoxMannWhitneyOptions(alt, exact, True, 0.95, mu)   # noqa: E731
    wx = lambda alt=0, exact=False, mu=0.0: abi.AnofoxWilcoxonOptions(alt, exact, True, 0.95, mu)      # noqa: E731
    cases = [("anofox_mann_whitney_u", [1.0, 2.0], [], mw(), "Mann-Whitney U test requires at least 1 observation per group"),
             ("anofox_mann_whitney_u", [NAN], [1.0, 2.0], mw(), "Mann-Whitney U test requires at least 1 observation per group"),
             ("anofox_mann_whitney_u", [1.0, 2.0], [3.0], mw(exact=True), "Mann-Whitney U test: exact p-values are not built"),
             ("anofox_mann_whitney_u", [1.0, 2.0], [3.0], mw(alt=7), "rank test: unknown alternative"),
             ("anofox_mann_whitney_u", [1.0, 2.0], [3.0], mw(mu=float("inf")), "rank test: mu must be finite"),
             ("anofox_wilcoxon_signed_rank", [1.0, 2.0, 3.0], [1.0, 2.0], wx(), "Wilcoxon signed-rank test requires equal length samples"),
             ("anofox_wilcoxon_signed_rank", [1.0, NAN, 3.0], [1.0, 2.0, NAN], wx(), "Wilcoxon signed-rank test requires at least 2 valid pairs"),
             ("anofox_wilcoxon_signed_rank", [1.0, 2.0, 3.0], [2.0, 1.0, 5.0], wx(exact=True), "Wilcoxon signed-rank test: exact p-values are not built"),
             ("anofox_wilcoxon_signed_rank", [1.0, 2.0, 3.0], [2.0, 1.0, 5.0], wx(alt=-2), "rank test: unknown alternative"),
             ("anofox_kruskal_wallis", [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.9, -0.9], None, "Kruskal-Wallis test requires at least 2 groups"),
             ("anofox_kruskal_wallis", [1.0, NAN, 3.0, 4.0], [0.0, 1.0, NAN, 0.0], None, "Kruskal-Wallis test requires at least 2 groups"),
             ("anofox_kruskal_wallis", [1.0, 2.0], [0.0, 1.0], None, "Kruskal-Wallis test requires at least 3 observations")]
    for symbol, a, b, options, text in cases:
        ok, res, err = _scalar(abi, symbol, a, b, options)
        assert not ok and err.code == 1 and text in err.text(), err.text()
        assert bytes(res) == bytes(C.sizeof(res))          # every field 0, the pointer NULL: nothing to free
        abi.load().anofox_free_test_result(C.byref(res))   # and freeing it is harmless
    err, empty = abi.AnofoxError(), abi.AnofoxDataArray(None, None, 0)
    assert not abi.load().anofox_mann_whitney_u(empty, empty, mw(), None, C.byref(err)) and "out_result is NULL" in err.text()
    assert not abi.load().anofox_kruskal_wallis(empty, empty, None, C.byref(err)) and "out_result is NULL" in err.text()


def test_python_refuses_exact_and_unequal_lengths_before_any_device():
    pkg = import_pkg()
    with pytest.raises(pkg.InvalidInputException, match="exact p-values are not built"):
        pkg.mann_whitney_u([1.0, 2.0], [3.0, 4.0], {"exact": True})
    with pytest.raises(pkg.InvalidInputException, match="exact p-values are not built"):
        pkg.wilcoxon_signed_rank([1.0, 2.0], [3.0, 4.5], {"Exact": "true"})
    with pytest.raises(pkg.InvalidInputException, match="requires equal length samples"):
        pkg.wilcoxon_signed_rank([1.0, 2.0, 3.0], [3.0, 4.5])
    with pytest.raises(pkg.InvalidInputException, match="same number of rows"):
        pkg.mann_whitney_u_agg(["a", "a"], [1.0, 2.0], [0])
