"""CPU-side checks of the eb_shrink surface: the header compiles as C, the struct layouts (the reference's ABI), the exported
symbols, the option spellings, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

EB_SYMBOLS = ("anofox_hip_eb_shrink_summary_len", "anofox_hip_eb_shrink_batch_device", "anofox_hip_eb_shrink_batch_host",
              "anofox_hip_eb_shrink_test_hooks", "anofox_eb_shrink", "anofox_free_eb_shrink_result")
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int64)


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in EB_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_eb_shrink_summary_len() == 8
    pkg = import_pkg()
    for name in ("eb_shrink", "eb_shrink_agg"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.SQL_FUNCTIONS["anofox_stats_" + name] is getattr(pkg, name)
    for name in ("eb_shrink_batch_host", "eb_shrink_batch_device", "shrink_coefficients", "eb_shrink_test_hooks"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(AnofoxEbShrinkOptions), sizeof(AnofoxEbShrinkResult), sizeof(AnofoxTauMethod),
         sizeof(AnofoxHipEbShrinkOptions), offsetof(AnofoxHipEbShrinkOptions, tau_squared));
  O(AnofoxEbShrinkOptions, method); O(AnofoxEbShrinkOptions, tau_squared);
  O(AnofoxEbShrinkResult, mu); O(AnofoxEbShrinkResult, mu_se); O(AnofoxEbShrinkResult, tau_squared); O(AnofoxEbShrinkResult, i_squared);
  O(AnofoxEbShrinkResult, q); O(AnofoxEbShrinkResult, n_groups); O(AnofoxEbShrinkResult, estimate); O(AnofoxEbShrinkResult, se);
  O(AnofoxEbShrinkResult, shrunken); O(AnofoxEbShrinkResult, shrunken_se); O(AnofoxEbShrinkResult, weight); O(AnofoxEbShrinkResult, len);
  printf("\n%d %d\n", ANOFOX_TAU_DERSIMONIAN_LAIRD, ANOFOX_TAU_NONE);
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    # the layouts of src/include/anofox_stats_ffi.h:2390-2418 under gcc, x86-64 SysV
    assert [int(v) for v in out[0].split()] == [16, 96, 4, 16, 8]
    assert [int(v) for v in out[1].split()] == [0, 8, 0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88]
    assert [int(v) for v in out[2].split()] == [0, 1]
    abi = import_pkg("_abi")
    assert C.sizeof(abi.AnofoxEbShrinkOptions) == 16 and C.sizeof(abi.AnofoxHipEbShrinkOptions) == 16 and C.sizeof(abi.AnofoxEbShrinkResult) == 96
    assert abi.AnofoxEbShrinkOptions.tau_squared.offset == 8
    assert [getattr(abi.AnofoxEbShrinkResult, f).offset for f, _ in abi.AnofoxEbShrinkResult._fields_] == list(range(0, 96, 8))


def test_option_spellings():
    pkg = import_pkg()
    P = pkg.parse_eb_shrink_options
    assert P(None).method == 0 and P(None).tau_squared is None and np.isnan(P(None).ffi_options().tau_squared)
    for name in ("dl", "dersimonian_laird", "dersimonian-laird", "DL"):
        assert P({"tau_method": name}).method == 0 and P({"shrinkage": name}).method == 0
    for name in ("none", "pooled", "complete", "Pooled"):
        assert P({"tau_method": name}).method == 1 and P({"SHRINKAGE": name}).method == 1
    assert P({"tau_squared": 0.25}).tau_squared == 0.25 and P({"tau2": 2}).tau_squared == 2.0
    assert P({"something_else": 3, "tau2": 0.5}).tau_squared == 0.5
    with pytest.raises(pkg.InvalidInputException, match=r"Unknown tau_method 'reml'\. Expected 'dl' or 'none'\."):
        P({"tau_method": "reml"})


def _batch(lib, abi, n_sets=1, n_items=4, off=(0, 4), n_cols=1, est_stride=1, se_stride=1, est=True, se=True, out=True, summary=True,
           offsets=True):
    o = np.array(off, np.int64)
    e, s = np.ones(64), np.ones(64)
    res, summ = np.zeros(64 * 3), np.zeros(64)
    err = abi.AnofoxError()
    p = lambda a, on: a.ctypes.data_as(_DP) if on else None
    ok = lib.anofox_hip_eb_shrink_batch_host(None, n_sets, n_items, o.ctypes.data_as(_IP) if offsets else None, n_cols, p(e, est), est_stride,
                                             p(s, se), se_stride, abi.AnofoxHipEbShrinkOptions(0, float("nan")), p(res, out), p(summ, summary),
                                             C.byref(err))
    return ok, err.code, err.text()


@pytest.mark.parametrize("kw, text", [
    (dict(est=False), "NULL"), (dict(se=False), "NULL"), (dict(out=False), "NULL"), (dict(summary=False), "NULL"),
    (dict(offsets=False), "NULL"), (dict(off=(0, 3, 2), n_sets=2), "non-decreasing"), (dict(off=(0, 5)), "non-decreasing"),
    (dict(off=(-1, 4)), "non-decreasing"), (dict(n_cols=0), "n_cols is 0"), (dict(n_cols=2, est_stride=1, se_stride=2), "stride"),
    (dict(n_cols=2, est_stride=2, se_stride=1), "stride"), (dict(n_sets=-1), "negative"), (dict(n_items=-1), "negative")])
def test_batch_argument_errors_come_before_any_device(kw, text):
    abi = import_pkg("_abi")
    ok, code, msg = _batch(abi.load(), abi, **kw)
    assert not ok and code == 1 and text in msg, msg


def test_device_form_checks_its_arguments_first():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    opts = abi.AnofoxHipEbShrinkOptions(0, float("nan"))
    assert not lib.anofox_hip_eb_shrink_batch_device(None, 1, 4, None, 1, None, 1, None, 1, opts, None, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_hip_eb_shrink_batch_device(None, 1, 4, 8, 0, 8, 1, 8, 1, opts, 8, 8, C.byref(err)) and "n_cols is 0" in err.text()
    assert not lib.anofox_hip_eb_shrink_batch_device(None, 1, 4, 8, 3, 8, 2, 8, 3, opts, 8, 8, C.byref(err)) and "stride" in err.text()
    assert not lib.anofox_hip_eb_shrink_batch_device(None, 1, 4, 8, 1, 8, 1, 8, 1, opts, 8, 8, C.byref(err)) and "context is NULL" in err.text()
    assert lib.anofox_hip_eb_shrink_batch_host(None, 0, 0, None, 1, None, 1, None, 1, opts, None, None, C.byref(err))   # nothing to do


def _scalar(abi, est, se, method=0, tau=float("nan"), validity=None):
    e, s = np.asarray(est, np.float64), np.asarray(se, np.float64)
    res, err = abi.AnofoxEbShrinkResult(), abi.AnofoxError()
    C.memset(C.byref(res), 0xAB, C.sizeof(res))
    ok = abi.load().anofox_eb_shrink(abi.AnofoxDataArray(e.ctypes.data_as(_DP), validity, len(e)),
                                     abi.AnofoxDataArray(s.ctypes.data_as(_DP), None, len(s)), abi.AnofoxEbShrinkOptions(method, tau),
                                     C.byref(res), C.byref(err))
    return ok, res, err


@pytest.mark.parametrize("est, se, kw, code, text", [
    ([], [], {}, 1, "Empty input"), ([0.1, 0.2], [0.1], {}, 9, "Dimension mismatch"), ([0.1, 0.2], [0.1, 0.1], dict(tau=-1.0), 1, "tau_squared"),
    ([0.1, 0.2], [0.1, 0.1], dict(tau=float("inf")), 1, "tau_squared"), ([0.1, 0.2], [0.1, 0.1], dict(method=3), 1, "method")])
def test_scalar_failures_leave_the_result_zeroed(est, se, kw, code, text):
    abi = import_pkg("_abi")
    ok, res, err = _scalar(abi, est, se, **kw)
    assert not ok and err.code == code and text in err.text(), err.text()
    assert bytes(res) == bytes(C.sizeof(res))          # every field 0, every pointer NULL: nothing to free
    abi.load().anofox_free_eb_shrink_result(C.byref(res))   # and freeing it is harmless
    assert not abi.load().anofox_eb_shrink(abi.AnofoxDataArray(None, None, 0), abi.AnofoxDataArray(None, None, 0),
                                           abi.AnofoxEbShrinkOptions(0, float("nan")), None, C.byref(err)) and "out_result is NULL" in err.text()
