"""CPU-side checks of the AFT fit-predict surface: the layout of AnofoxHipAftPredictOptions as C compiles it and as _abi.py mirrors
it, the exported symbols, the argument and option errors that are answered before any device is touched, and the Python option
parser's two new keys."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

_DP = C.POINTER(C.c_double)
SYMBOLS = ("anofox_hip_aft_pred_len", "anofox_hip_aft_fit_predict_batch_device", "anofox_hip_aft_fit_predict_batch_host")


def test_symbols_and_layout():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_aft_pred_len() == 4
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(AnofoxHipAftPredictOptions), offsetof(AnofoxHipAftPredictOptions, quantile),
         offsetof(AnofoxHipAftPredictOptions, horizon), sizeof(AnofoxHipAftBatchOptions));
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        assert [int(v) for v in subprocess.check_output([exe]).decode().split()] == [16, 0, 8, 40]
    assert C.sizeof(abi.AnofoxHipAftPredictOptions) == 16
    assert (abi.AnofoxHipAftPredictOptions.quantile.offset, abi.AnofoxHipAftPredictOptions.horizon.offset) == (0, 8)


def _host_call(lib, abi, p=2, n=8, quantile=0.5, horizon=float("nan"), pred=True, event=True, err=None):
    y = np.ones(n)
    off = np.array([0, n], dtype=np.int64)
    c = y.ctypes.data_as(_DP)
    recs, out = np.empty(p + 13), np.empty(4 * n)
    return lib.anofox_hip_aft_fit_predict_batch_host(
        None, 1, p, n, off.ctypes.data_as(C.POINTER(C.c_int64)), c, (_DP * max(p, 1))(*[c] * p), c if event else None,
        abi.AnofoxHipAftBatchOptions(0, 1, 100, 1e-9, 0, 0.95), abi.AnofoxHipAftPredictOptions(quantile, horizon),
        recs.ctypes.data_as(_DP), None, out.ctypes.data_as(_DP) if pred else None, C.byref(err))


def test_errors_answered_without_a_device():
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    for q in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert not _host_call(lib, abi, quantile=q, err=err)
        assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "aft: quantile must be in (0, 1)"
    for h in (-1e-300, -1.0, float("inf"), float("-inf")):
        assert not _host_call(lib, abi, horizon=h, err=err)
        assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "aft: horizon must be finite and >= 0"
    assert not _host_call(lib, abi, pred=False, err=err) and err.code == 1 and err.text() == "pred is NULL"
    assert not _host_call(lib, abi, event=False, err=err) and err.code == 1 and err.text() == "event is NULL"
    assert not _host_call(lib, abi, p=33, err=err) and err.code == 1 and err.text() == "aft: n_features > 32 is not built"
    # the device form: the same order, then the context
    fake = C.c_void_p(np.ones(8).ctypes.data)
    vcols = (C.c_void_p * 2)(fake, fake)
    dev = lib.anofox_hip_aft_fit_predict_batch_device
    opts = abi.AnofoxHipAftBatchOptions(0, 1, 100, 1e-9, 0, 0.95)
    ok = abi.AnofoxHipAftPredictOptions(0.5, 2.0)
    assert not dev(None, 1, 2, 8, fake, fake, vcols, fake, opts, abi.AnofoxHipAftPredictOptions(1.0, 2.0), fake, None, fake, C.byref(err))
    assert err.text() == "aft: quantile must be in (0, 1)"
    assert not dev(None, 1, 2, 8, fake, fake, vcols, fake, opts, abi.AnofoxHipAftPredictOptions(0.5, -2.0), fake, None, fake, C.byref(err))
    assert err.text() == "aft: horizon must be finite and >= 0"
    assert not dev(None, 1, 2, 8, fake, fake, vcols, fake, opts, ok, fake, None, None, C.byref(err)) and err.text() == "pred is NULL"
    assert not dev(None, 1, 2, 8, fake, fake, vcols, fake, opts, ok, fake, None, fake, C.byref(err)) and err.text() == "context is NULL"
    # no groups: nothing to do, no device needed
    assert lib.anofox_hip_aft_fit_predict_batch_host(None, 0, 2, 0, None, None, (_DP * 2)(), None, opts, ok, None, None, None, C.byref(err))


def test_option_parser_quantile_and_horizon():
    aft = import_pkg("aft")
    d = aft.parse_aft_options(None)
    assert d.quantile == 0.5 and d.horizon is None
    b = d.predict_options()
    assert b.quantile == 0.5 and np.isnan(b.horizon)
    o = aft.parse_aft_options({"Quantile": 0.9, "HORIZON": 30, "dist": "exp"})
    assert (o.quantile, o.horizon, o.dist) == (0.9, 30.0, 3)
    assert (o.predict_options().quantile, o.predict_options().horizon) == (0.9, 30.0)
    assert aft.parse_aft_options({"horizon": None}).horizon is None
    # the fit's options are what they were
    assert aft.parse_aft_options({"quantile": 0.9}).batch_options().tolerance == 1e-9
    pkg = import_pkg()
    assert callable(pkg.aft_fit_predict_agg) and "aft_fit_predict_agg" in pkg.__all__
    with pytest.raises(import_pkg("options").InvalidInputException, match="same number of rows"):
        pkg.aft_fit_predict_agg([1, 1], [1.0, 2.0], [[0.1], [0.2]], [1.0])
