"""CPU-side checks of the AFT surface: the header compiles as C, the struct layouts (the reference's ABI), the exported symbols,
the host functions anofox_aft_cdf / anofox_aft_quantile against the restatement, and the argument errors that are answered
before any GPU work."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import aft_restate as R
from conftest import ROOT, import_pkg

AFT_SYMBOLS = ("anofox_hip_aft_record_len", "anofox_hip_aft_fit_batch_device", "anofox_hip_aft_fit_batch_host", "anofox_hip_aft_test_hooks",
               "anofox_aft_fit", "anofox_free_aft_result", "anofox_free_aft_inference", "anofox_aft_cdf", "anofox_aft_quantile")
_DP = C.POINTER(C.c_double)


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in AFT_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_aft_record_len(5) == 18 and lib.anofox_hip_aft_record_len(32) == 45


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu %zu\n", sizeof(AnofoxAftOptions), sizeof(AnofoxAftFitResultCore), sizeof(AnofoxAftInference),
         sizeof(AnofoxAftDistribution), sizeof(AnofoxHipAftBatchOptions));
  O(AnofoxAftOptions, fit_intercept); O(AnofoxAftOptions, max_iterations); O(AnofoxAftOptions, tolerance);
  O(AnofoxAftOptions, compute_inference); O(AnofoxAftOptions, confidence_level); O(AnofoxAftOptions, priors);
  O(AnofoxAftOptions, priors_len); O(AnofoxAftOptions, vcov);
  O(AnofoxAftFitResultCore, scale); O(AnofoxAftFitResultCore, null_log_likelihood); O(AnofoxAftFitResultCore, bic);
  O(AnofoxAftFitResultCore, n_events); O(AnofoxAftFitResultCore, n_features); O(AnofoxAftFitResultCore, iterations);
  O(AnofoxAftFitResultCore, converged);
  O(AnofoxAftInference, len); O(AnofoxAftInference, confidence_level); O(AnofoxAftInference, intercept_std_error);
  O(AnofoxAftInference, log_scale_std_error);
  O(AnofoxHipAftBatchOptions, fit_intercept); O(AnofoxHipAftBatchOptions, max_iterations); O(AnofoxHipAftBatchOptions, tolerance);
  O(AnofoxHipAftBatchOptions, compute_inference); O(AnofoxHipAftBatchOptions, confidence_level);
  printf("\n%d %d %d %d\n", ANOFOX_AFT_WEIBULL, ANOFOX_AFT_LOGNORMAL, ANOFOX_AFT_LOGLOGISTIC, ANOFOX_AFT_EXPONENTIAL);
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    sizes = [int(v) for v in out[0].split()]
    offs = [int(v) for v in out[1].split()]
    # the layouts of src/include/anofox_stats_ffi.h:2293-2354 under gcc, x86-64 SysV
    assert sizes[:4] == [64, 104, 72, 4]
    assert offs[:19] == [4, 8, 16, 24, 32, 40, 48, 56, 24, 40, 56, 72, 88, 96, 100, 40, 48, 56, 64]
    assert sizes[4] == 40 and offs[19:] == [4, 8, 16, 24, 32]
    assert [int(v) for v in out[2].split()] == [0, 1, 2, 3]
    abi = import_pkg("_abi")
    assert [C.sizeof(t) for t in (abi.AnofoxAftOptions, abi.AnofoxAftFitResultCore, abi.AnofoxAftInference)] == sizes[:3]
    assert C.sizeof(abi.AnofoxHipAftBatchOptions) == 40
    assert abi.AnofoxAftOptions.vcov.offset == 56 and abi.AnofoxAftFitResultCore.converged.offset == 100
    assert abi.AnofoxAftInference.log_scale_std_error.offset == 64 and abi.AnofoxHipAftBatchOptions.confidence_level.offset == 32


def test_cdf_and_quantile_agree_with_the_restatement():
    lib = import_pkg("_abi").load()
    for dist in (R.WEIBULL, R.LOGNORMAL, R.LOGLOGISTIC, R.EXPONENTIAL):
        for eta, scale in ((0.0, 1.0), (1.3, 0.6), (-0.7, 2.5)):
            for t in (1e-6, 0.05, 0.5, 1.0, 2.0, 7.5, 40.0, 1e4):
                got, want = lib.anofox_aft_cdf(t, eta, scale, dist), R.cdf_time(dist, t, eta, scale)
                assert abs(got - want) <= 1e-14 + 1e-13 * want, (dist, t, eta, scale, got, want)
            for p in (1e-9, 0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0 - 1e-9):
                got, want = lib.anofox_aft_quantile(p, eta, scale, dist), R.quantile_time(dist, p, eta, scale)
                # (in the tails the quantile is ill conditioned in p: an error of 1e-16 in F moves z by 1e-16 / f(z); the inversion
                # below is the check there)
                assert abs(got - want) <= (1e-11 if 0.01 <= p <= 0.99 else 1e-6) * want, (dist, p, eta, scale, got, want)
                assert abs(lib.anofox_aft_cdf(got, eta, scale, dist) - p) <= 1e-12
            # the rules at the edges: t <= 0 is 0; p is clamped to [1e-12, 1 - 1e-12]
            assert lib.anofox_aft_cdf(0.0, eta, scale, dist) == 0.0 and lib.anofox_aft_cdf(-3.0, eta, scale, dist) == 0.0
            assert lib.anofox_aft_quantile(0.0, eta, scale, dist) == lib.anofox_aft_quantile(1e-12, eta, scale, dist)
            assert lib.anofox_aft_quantile(-1.0, eta, scale, dist) == lib.anofox_aft_quantile(1e-12, eta, scale, dist)
            assert lib.anofox_aft_quantile(1.0, eta, scale, dist) == lib.anofox_aft_quantile(1.0 - 1e-12, eta, scale, dist)
            assert lib.anofox_aft_quantile(2.0, eta, scale, dist) == lib.anofox_aft_quantile(1.0 - 1e-12, eta, scale, dist)
            assert math.isfinite(lib.anofox_aft_quantile(1.0, eta, scale, dist))
    assert math.isnan(lib.anofox_aft_cdf(1.0, 0.0, 1.0, 9)) and math.isnan(lib.anofox_aft_quantile(0.5, 0.0, 1.0, 9))
    pkg = import_pkg()
    assert pkg.aft_cdf(2.0, 0.5, 0.7, "log_normal") == lib.anofox_aft_cdf(2.0, 0.5, 0.7, 1)
    assert pkg.aft_quantile(0.3, 0.5, 0.7, "EXP") == lib.anofox_aft_quantile(0.3, 0.5, 0.7, 3)


def _arrays(n=8, p=2):
    abi = import_pkg("_abi")
    rng = np.random.default_rng(1)
    t = rng.uniform(0.5, 3.0, n)
    e = (rng.uniform(size=n) < 0.7).astype(float)
    cols = [rng.uniform(-1, 1, n) for _ in range(p)]
    keep = [t, e] + cols
    arr = lambda v: abi.AnofoxDataArray(v.ctypes.data_as(_DP), None, n)
    xs = (abi.AnofoxDataArray * p)(*[arr(c) for c in cols])
    return abi, arr(t), xs, arr(e), keep


def _options(abi, **kw):
    o = abi.AnofoxAftOptions(0, True, 100, 1e-9, False, 0.95, None, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("kw", [dict(max_iterations=0), dict(tolerance=float("nan")), dict(tolerance=0.0), dict(tolerance=float("inf")),
                                dict(dist=4), dict(compute_inference=True, confidence_level=1.0)])
def test_scalar_invalid_options(kw):
    abi, ta, xs, ea, keep = _arrays()
    lib = abi.load()
    core, inf, err = abi.AnofoxAftFitResultCore(), abi.AnofoxAftInference(), abi.AnofoxError()
    assert not lib.anofox_aft_fit(ta, xs, 2, ea, _options(abi, **kw), C.byref(core), C.byref(inf), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "aft: invalid options"
    assert not core.coefficients and core.coefficients_len == 0 and math.isnan(core.log_likelihood)


def test_scalar_priors_width_and_argument_errors():
    abi, ta, xs, ea, keep = _arrays()
    lib = abi.load()
    core, inf, err = abi.AnofoxAftFitResultCore(), abi.AnofoxAftInference(), abi.AnofoxError()
    junk = np.ones(2)
    core.coefficients, core.coefficients_len, inf.std_errors, inf.len = junk.ctypes.data_as(_DP), 2, junk.ctypes.data_as(_DP), 2
    prior = abi.AnofoxPriorSpec(1, 0.0, 1.0)
    o = _options(abi)
    o.priors, o.priors_len = C.pointer(prior), 1
    assert not lib.anofox_aft_fit(ta, xs, 2, ea, o, C.byref(core), C.byref(inf), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "aft: priors are not built"
    assert not core.coefficients and not inf.std_errors and inf.len == 0 and math.isnan(inf.log_scale_std_error)
    abi33, t33, xs33, e33, keep33 = _arrays(40, 33)
    assert not lib.anofox_aft_fit(t33, xs33, 33, e33, _options(abi), C.byref(core), None, C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "aft: n_features > 32 is not built"
    assert not lib.anofox_aft_fit(ta, xs, 2, ea, _options(abi), None, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_aft_fit(ta, None, 0, ea, _options(abi), C.byref(core), None, C.byref(err)) and err.code == 1
    short = abi.AnofoxDataArray(keep[1].ctypes.data_as(_DP), None, 5)
    assert not lib.anofox_aft_fit(ta, xs, 2, short, _options(abi), C.byref(core), None, C.byref(err))
    assert err.code == abi.ERROR_DIMENSION_MISMATCH
    for vcov in (1, 2):   # without priors every vcov is the same covariance: accepted (what fails next is the missing device, not vcov)
        ok = lib.anofox_aft_fit(ta, xs, 2, ea, _options(abi, vcov=vcov), C.byref(core), None, C.byref(err))
        assert ok or "vcov" not in err.text()
        lib.anofox_free_aft_result(C.byref(core))
    lib.anofox_free_aft_result(None)
    lib.anofox_free_aft_inference(None)
    lib.anofox_free_aft_inference(C.byref(abi.AnofoxAftInference()))


def test_batch_argument_errors():
    abi = import_pkg("_abi")
    lib = abi.load()
    n, err = 8, abi.AnofoxError()
    y = np.ones(n)
    off = np.array([0, n], dtype=np.int64)
    opts = abi.AnofoxHipAftBatchOptions(0, 1, 100, 1e-9, 0, 0.95)
    I64P = C.POINTER(C.c_int64)
    c = y.ctypes.data_as(_DP)

    def call(p, cols, tp=c, ep=c, offp=off.ctypes.data_as(I64P)):
        recs = np.empty(p + 13)
        colp = (_DP * max(p, 1))(*cols) if cols is not None else None
        return lib.anofox_hip_aft_fit_batch_host(None, 1, p, n, offp, tp, colp, ep, opts, recs.ctypes.data_as(_DP), None, C.byref(err))
    assert not call(33, [c] * 33) and err.code == 1 and err.text() == "aft: n_features > 32 is not built"
    assert not call(0, None) and err.code == 1
    assert not call(2, [c, c], tp=None) and err.code == 1 and "NULL" in err.text()
    assert not call(2, [c, c], ep=None) and err.code == 1 and err.text() == "event is NULL"
    assert not call(2, [c, None]) and err.code == 1 and "NULL" in err.text()
    bad = np.array([3, 1], dtype=np.int64)
    assert not call(2, [c, c], offp=bad.ctypes.data_as(I64P)) and err.code == 1 and "row_offsets" in err.text()
    fake = C.c_void_p(y.ctypes.data)
    vcols = (C.c_void_p * 2)(fake, fake)
    dev = lib.anofox_hip_aft_fit_batch_device
    assert not dev(None, 1, 2, n, fake, fake, vcols, fake, opts, fake, None, C.byref(err))
    assert err.code == 1 and err.text() == "context is NULL"
    assert not dev(None, 1, 33, n, fake, fake, (C.c_void_p * 33)(*[fake] * 33), fake, opts, fake, None, C.byref(err))
    assert err.code == 1 and "n_features > 32 is not built" in err.text()
    assert not dev(None, -1, 2, n, fake, fake, vcols, fake, opts, fake, None, C.byref(err)) and err.code == 1
    # no groups: nothing to do, no device needed
    assert lib.anofox_hip_aft_fit_batch_host(None, 0, 2, 0, None, None, (_DP * 2)(), None, opts, None, None, C.byref(err))


def test_option_parser_and_dist_names():
    aft = import_pkg("aft")
    o = aft.parse_aft_options({"DIST": "Log_Normal", "intercept": False, "max_iter": 7, "tol": 1e-5, "compute_inference": True,
                               "confidence_level": 0.9, "vcov": "sandwich", "something_else": 1})
    assert (o.dist, o.fit_intercept, o.max_iterations, o.tolerance, o.compute_inference, o.confidence_level) == (1, False, 7, 1e-5, True, 0.9)
    d = aft.parse_aft_options(None)
    assert (d.dist, d.fit_intercept, d.max_iterations, d.tolerance, d.compute_inference, d.confidence_level) == (0, True, 100, 1e-9, False, 0.95)
    b = d.batch_options()
    assert (b.dist, b.fit_intercept, b.max_iterations, b.tolerance, b.compute_inference) == (0, 1, 100, 1e-9, 0)
    names = {"weibull": 0, "lognormal": 1, "log_normal": 1, "log-normal": 1, "loglogistic": 2, "log_logistic": 2, "log-logistic": 2,
             "exponential": 3, "exp": 3, "WEIBULL": 0}
    for name, code in names.items():
        assert aft.parse_aft_options({"dist": name}).dist == code
    exc = import_pkg("options").InvalidInputException
    with pytest.raises(exc, match="Unknown AFT distribution"):
        aft.parse_aft_options({"dist": "cauchy"})
    with pytest.raises(exc, match="aft: priors are not built"):
        aft.parse_aft_options({"priors": [{"kind": "normal"}]})
    with pytest.raises(exc):
        aft.parse_aft_options([1, 2])
