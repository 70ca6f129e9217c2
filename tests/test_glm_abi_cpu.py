"""CPU-side checks of the GLM surface: the symbols, the struct layouts (the reference's ABI), the argument errors that are
answered before any GPU work, and the option parsers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

GLM_SYMBOLS = ("anofox_hip_glm_record_len", "anofox_hip_glm_fit_batch_device", "anofox_hip_glm_fit_batch_host",
               "anofox_hip_glm_fit_predict_batch_device", "anofox_hip_glm_fit_predict_batch_host", "anofox_poisson_fit",
               "anofox_binomial_fit", "anofox_logistic_fit", "anofox_free_glm_result")
_DP = C.POINTER(C.c_double)


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in GLM_SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_glm_record_len(5) == 16 and lib.anofox_hip_glm_record_len(32) == 43


def test_struct_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(AnofoxGlmFitResultCore), sizeof(AnofoxPoissonOptions), sizeof(AnofoxBinomialOptions),
         sizeof(AnofoxLogisticOptions), sizeof(AnofoxLogisticFitExtras), sizeof(AnofoxPriorSpec), sizeof(AnofoxHipGlmBatchOptions));
  O(AnofoxGlmFitResultCore, iterations); O(AnofoxGlmFitResultCore, converged); O(AnofoxPoissonOptions, link);
  O(AnofoxPoissonOptions, tolerance); O(AnofoxPoissonOptions, lambda); O(AnofoxPoissonOptions, priors); O(AnofoxPoissonOptions, vcov);
  O(AnofoxPoissonOptions, offset_column); O(AnofoxBinomialOptions, offset_column); O(AnofoxLogisticOptions, threshold);
  O(AnofoxLogisticOptions, max_iterations); O(AnofoxLogisticOptions, tolerance); O(AnofoxLogisticOptions, priors);
  O(AnofoxLogisticOptions, offset_column);
  O(AnofoxHipGlmBatchOptions, fit_intercept); O(AnofoxHipGlmBatchOptions, tolerance); O(AnofoxHipGlmBatchOptions, confidence_level);
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
    sizes = [int(v) for v in out[0].split()]
    offs = [int(v) for v in out[1].split()]
    # measured against src/include/anofox_stats_ffi.h with gcc, x86-64 SysV
    assert sizes[:6] == [88, 80, 80, 80, 16, 24]
    assert offs[:14] == [80, 84, 4, 16, 40, 48, 64, 72, 72, 24, 32, 40, 48, 72]
    abi = import_pkg("_abi")
    assert [C.sizeof(t) for t in (abi.AnofoxGlmFitResultCore, abi.AnofoxPoissonOptions, abi.AnofoxBinomialOptions,
                                  abi.AnofoxLogisticOptions, abi.AnofoxLogisticFitExtras, abi.AnofoxPriorSpec,
                                  abi.AnofoxHipGlmBatchOptions)] == sizes
    assert abi.AnofoxGlmFitResultCore.converged.offset == 84 and abi.AnofoxPoissonOptions.offset_column.offset == 72
    assert abi.AnofoxLogisticOptions.threshold.offset == 24 and abi.AnofoxLogisticOptions.offset_column.offset == 72
    assert [abi.AnofoxHipGlmBatchOptions.fit_intercept.offset, abi.AnofoxHipGlmBatchOptions.tolerance.offset,
            abi.AnofoxHipGlmBatchOptions.confidence_level.offset] == offs[14:]


def _arrays(n=6, p=2):
    abi = import_pkg("_abi")
    rng = np.random.default_rng(1)
    y = rng.poisson(2.0, n).astype(float)
    cols = [rng.uniform(-1, 1, n) for _ in range(p)]
    keep = [y] + cols
    ya = abi.AnofoxDataArray(y.ctypes.data_as(_DP), None, n)
    xs = (abi.AnofoxDataArray * p)(*[abi.AnofoxDataArray(c.ctypes.data_as(_DP), None, n) for c in cols])
    return abi, ya, xs, keep


def _poisson_options(abi, **kw):
    o = abi.AnofoxPoissonOptions(True, 0, 100, 1e-8, False, 0.95, 0.0, None, 0, 0, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("kw, text", [(dict(link=2), "glm: link 2 of poisson is not built"), (dict(vcov=1), "not built"),
                                      (dict(max_iterations=0), "invalid options"), (dict(tolerance=float("nan")), "invalid options"),
                                      (dict(lambda_=-1.0), "invalid options"), (dict(offset_column=3), "offset")])
def test_scalar_argument_errors(kw, text):
    abi, ya, xs, keep = _arrays()
    lib = abi.load()
    core, err = abi.AnofoxGlmFitResultCore(), abi.AnofoxError()
    assert not lib.anofox_poisson_fit(ya, xs, 2, _poisson_options(abi, **kw), C.byref(core), None, C.byref(err))
    assert err.code == 1 and text in err.text(), err.text()
    assert not core.coefficients


def test_scalar_priors_probit_and_width_errors():
    abi, ya, xs, keep = _arrays()
    lib = abi.load()
    core, err = abi.AnofoxGlmFitResultCore(), abi.AnofoxError()
    prior = abi.AnofoxPriorSpec(1, 0.0, 1.0)
    o = _poisson_options(abi)
    o.priors, o.priors_len = C.pointer(prior), 1
    assert not lib.anofox_poisson_fit(ya, xs, 2, o, C.byref(core), None, C.byref(err))
    assert err.code == 1 and "priors are not built" in err.text()
    b = abi.AnofoxBinomialOptions(True, 1, 100, 1e-8, False, 0.95, 0.0, None, 0, 0, 0)   # probit
    assert not lib.anofox_binomial_fit(ya, xs, 2, b, C.byref(core), None, C.byref(err))
    assert err.code == 1 and "glm: link 1 of binomial is not built" in err.text()
    lo = abi.AnofoxLogisticOptions(True, False, 0.95, 0.0, 0.5, 100, 1e-8, None, 0, 0, 0)
    assert not lib.anofox_logistic_fit(ya, xs, 2, lo, C.byref(core), None, None, C.byref(err))     # y is not 0 / 1
    assert err.code == 1 and "binary response" in err.text()
    assert not lib.anofox_poisson_fit(ya, xs, 2, _poisson_options(abi), None, None, C.byref(err)) and err.code == 1
    assert not lib.anofox_poisson_fit(ya, None, 0, _poisson_options(abi), C.byref(core), None, C.byref(err)) and err.code == 1
    abi33, ya33, xs33, keep33 = _arrays(40, 33)
    assert not lib.anofox_poisson_fit(ya33, xs33, 33, _poisson_options(abi), C.byref(core), None, C.byref(err))
    assert err.code == 1 and "n_features > 32 is not built" in err.text()
    lib.anofox_free_glm_result(None)
    lib.anofox_free_glm_result(C.byref(core))


def test_batch_argument_errors():
    abi = import_pkg("_abi")
    lib = abi.load()
    n, err = 8, abi.AnofoxError()
    y = np.ones(n)
    off = np.array([0, n], dtype=np.int64)
    opts = abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    I64P = C.POINTER(C.c_int64)

    def call(p, cols, yp=y.ctypes.data_as(_DP), rec=None, offp=off.ctypes.data_as(I64P)):
        recs = np.empty(p + 11) if rec is None else rec
        colp = (_DP * max(p, 1))(*cols) if cols is not None else None
        return lib.anofox_hip_glm_fit_batch_host(None, 1, p, n, offp, yp, colp, None, opts, recs.ctypes.data_as(_DP), None, C.byref(err))
    c = y.ctypes.data_as(_DP)
    assert not call(33, [c] * 33) and err.code == 1 and "glm: n_features > 32 is not built" in err.text()
    assert not call(0, None) and err.code == 1
    assert not call(2, [c, c], yp=None) and err.code == 1 and "NULL" in err.text()
    assert not call(2, [c, None]) and err.code == 1 and "NULL" in err.text()
    bad = np.array([3, 1], dtype=np.int64)
    assert not call(2, [c, c], offp=bad.ctypes.data_as(I64P)) and err.code == 1 and "row_offsets" in err.text()
    assert not lib.anofox_hip_glm_fit_predict_batch_host(None, 1, 2, n, off.ctypes.data_as(I64P), c, (_DP * 2)(c, c), None, None, opts,
                                                         np.empty(13).ctypes.data_as(_DP), None, C.byref(err))
    assert err.code == 1 and "pred is NULL" in err.text()
    assert not lib.anofox_hip_glm_fit_batch_device(None, 1, 2, n, None, None, (C.c_void_p * 2)(), None, opts, None, None, C.byref(err))
    assert err.code == 1
    # the device fit-predict entry: its own checks, answered before any GPU work (the pointers are never dereferenced)
    fake = C.c_void_p(y.ctypes.data)
    vcols = (C.c_void_p * 2)(fake, fake)
    fpd = lib.anofox_hip_glm_fit_predict_batch_device
    assert not fpd(None, 1, 2, n, fake, fake, vcols, None, None, opts, fake, None, C.byref(err))
    assert err.code == 1 and "pred is NULL" in err.text()
    assert not fpd(None, 1, 2, n, fake, fake, vcols, None, None, opts, None, fake, C.byref(err))
    assert err.code == 1 and "NULL" in err.text()
    assert not fpd(None, 1, 2, n, fake, fake, vcols, None, None, opts, fake, fake, C.byref(err))
    assert err.code == 1 and "context is NULL" in err.text()
    assert not fpd(None, 1, 33, n, fake, fake, (C.c_void_p * 33)(*[fake] * 33), None, None, opts, fake, fake, C.byref(err))
    assert err.code == 1 and "n_features > 32 is not built" in err.text()
    assert not fpd(None, -1, 2, n, fake, fake, vcols, None, None, opts, fake, fake, C.byref(err)) and err.code == 1


def test_failed_scalar_call_resets_its_outputs():
    abi, ya, xs, keep = _arrays()
    lib = abi.load()
    core, inf, ex, err = abi.AnofoxGlmFitResultCore(), abi.AnofoxFitResultInference(), abi.AnofoxLogisticFitExtras(), abi.AnofoxError()
    junk = np.ones(2)
    core.coefficients, core.coefficients_len, core.deviance = junk.ctypes.data_as(_DP), 2, 5.0
    inf.std_errors, inf.len, ex.accuracy = junk.ctypes.data_as(_DP), 2, 0.5
    lo = abi.AnofoxLogisticOptions(True, True, 0.95, 0.0, 0.5, 100, 1e-8, None, 0, 0, 0)
    assert not lib.anofox_logistic_fit(ya, xs, 2, lo, C.byref(core), C.byref(inf), C.byref(ex), C.byref(err))   # y is not 0 / 1
    assert not core.coefficients and core.coefficients_len == 0 and np.isnan(core.deviance)
    assert not inf.std_errors and inf.len == 0 and np.isnan(inf.f_statistic) and np.isnan(ex.accuracy)
    o = _poisson_options(abi, compute_inference=True, confidence_level=1.5)
    assert not lib.anofox_poisson_fit(ya, xs, 2, o, C.byref(core), C.byref(inf), C.byref(err))
    assert err.code == 1 and "invalid options" in err.text()


def test_option_parsers():
    pkg = import_pkg("options")
    o = pkg.parse_poisson_options({"INTERCEPT": False, "max_iter": 7, "TOL": 1e-5, "Lambda": 0.25, "compute_inference": True,
                                   "confidence_level": 0.9, "offset": 2, "link": "LOG", "something_else": 1})
    assert (o.family, o.fit_intercept, o.max_iterations, o.tolerance, o.lambda_, o.compute_inference, o.confidence_level, o.offset) == \
        ("poisson", False, 7, 1e-5, 0.25, True, 0.9, 2)
    d = pkg.parse_binomial_options(None)
    assert (d.family, d.fit_intercept, d.max_iterations, d.tolerance, d.lambda_, d.link) == ("binomial", True, 100, 1e-8, 0.0, "logit")
    b = d.batch_options()
    assert b.family == 1 and b.max_iterations == 100 and b.tolerance == 1e-8
    assert pkg.parse_poisson_options({"fit_intercept": True, "max_iterations": 3, "tolerance": 0.5}).max_iterations == 3
    with pytest.raises(pkg.InvalidInputException, match="glm: link probit is not built"):
        pkg.parse_binomial_options({"link": "probit"})
    with pytest.raises(pkg.InvalidInputException, match="glm: link sqrt is not built"):
        pkg.parse_poisson_options({"link": "sqrt"})
    with pytest.raises(pkg.InvalidInputException):
        pkg.parse_poisson_options([1, 2])
    with pytest.raises(pkg.InvalidInputException, match="glm: vcov sandwich is not built"):
        pkg.parse_poisson_options({"VCOV": "sandwich"})
    with pytest.raises(pkg.InvalidInputException, match="glm: priors are not built"):
        pkg.parse_binomial_options({"priors": [{"kind": "normal"}]})
    assert pkg.parse_poisson_options({"vcov": "Laplace", "priors": None}).fit_intercept
