"""The DuckDB glue of the mixed-model family (duckdb_shim/glmm_family_hip.cpp) without a GPU: what binds through the real glue
library (tests/tools/glmm_family_capi.cpp): the four names, every overload, the result types with and without inference, the
bind-time errors and the options that do not fold; and the glue with its driver on a mock of the C ABI under ASan / UBSan as a
stand-alone program (tests/tools/glmm_glue_sanitize.cpp): Update's NULL rules for both aggregates and the three group types,
Combine's renumbering of the levels, Finalize."""
import ctypes as C
import os
import subprocess

import pytest

import glmm_glue_driver as D
from conftest import ROOT

NAMES = ("anofox_stats_glmm_fit_agg", "glmm_fit_agg", "anofox_stats_glmm_fit_predict_agg", "glmm_fit_predict_agg")
DOUBLE, BOOLEAN, BIGINT, INTEGER, LIST, FACTORS, RANEF = 0, 1, 2, 3, 4, 5, 6
CORE = ("coefficients,intercept,var_group,var_residual,icc,log_likelihood,aic,bic,deviance,n_observations,n_groups,n_features,iterations,"
        "converged,random_cov,random_dim,factors")
INFERENCE = ",std_errors,z_values,p_values,ci_lower,ci_upper,intercept_std_error"


@pytest.fixture(scope="module")
def lib():
    return D.load()


def test_the_glue_library_has_a_makefile_target():
    with open(os.path.join(D.SHIM, "Makefile")) as f:
        text = f.read()
    assert "libanofox_glmm_family_capi.so" in text and "glmm_family_hip.cpp" in text and "glmm_family_capi.cpp" in text


def test_names_overloads_and_aliases(lib):
    q, msg = D.open_query(lib, NAMES[0])
    assert q, msg
    assert lib.ag_registered_count(q) == 4
    for name in NAMES:
        counts = (C.c_int * 8)()
        assert lib.ag_registered(q, name.encode()) == 1
        k = lib.ag_overloads(q, name.encode(), counts)
        # (y, x, group), (.., options) and for the fit-predict aggregate (.., split_col), (.., split_col, options)
        assert list(counts[:k]) == ([3, 4] if "predict" not in name else [3, 4, 104, 105])
    assert lib.ag_registered(q, b"glmm_fit") == 0
    lib.ag_close(q)
    assert D.open_query(lib, "glmm_fit")[0] is None
    assert D.open_query(lib, "glmm_fit_agg", split=True)[0] is None   # the fit aggregate has no split column


@pytest.mark.parametrize("fn", NAMES[:2])
def test_fit_result_type_with_and_without_inference(lib, fn):
    core = [LIST] + [DOUBLE] * 8 + [BIGINT] * 3 + [INTEGER, BOOLEAN, LIST, INTEGER, FACTORS]
    for spec, as_map, inference in ((None, False, False), ("reml=false", False, False), ("compute_inference=false", False, False),
                                    ("compute_inference=true", False, True), ("COMPUTE_INFERENCE=1", True, True), ("family=LMM;compute_inference=true", False, True)):
        q, msg = D.open_query(lib, fn, spec, as_map)
        assert q, msg
        is_list, kinds, names = D.fields(lib, q)
        lib.ag_close(q)
        assert is_list == 0 and names == CORE + (INFERENCE if inference else "") + ",ranef"
        assert kinds == core + ([LIST] * 5 + [DOUBLE] if inference else []) + [RANEF]
    # options that are not a constant keep the defaults: no inference fields, and nothing to refuse
    q, msg = D.open_query(lib, fn, "compute_inference=true;family=poisson", foldable=False)
    assert q, msg
    assert len(D.fields(lib, q)[1]) == 18
    lib.ag_close(q)


@pytest.mark.parametrize("fn", NAMES[2:])
@pytest.mark.parametrize("split", [False, True])
def test_fit_predict_result_type(lib, fn, split):
    for spec in (None, "interval=prediction;level=0.9", "compute_inference=true", "interval=true"):
        q, msg = D.open_query(lib, fn, spec, split=split)
        assert q, msg
        is_list, kinds, names = D.fields(lib, q)
        lib.ag_close(q)
        assert is_list == 1 and names == "y,yhat,yhat_fixed,yhat_lower,yhat_upper,is_training" and kinds == [DOUBLE] * 5 + [BOOLEAN]


@pytest.mark.parametrize("fn", NAMES)
def test_what_is_not_built_raises_at_bind(lib, fn):
    for spec, as_map, text in (("family=poisson", False, "glmm: the poisson family is not built"), ("FAMILY=Binomial", False, "glmm: the binomial family is not built"),
                               ("family=tweedie", True, "glmm: the tweedie family is not built"), ("offset=2", False, "glmm: an offset is not built"),
                               ("offset_column=1", True, "glmm: an offset is not built"), ("random_slopes=1", False, "glmm: random slopes are not built"),
                               ("family=cauchy", False, "Unknown GLMM family 'cauchy'. Expected 'gaussian'.")):
        q, msg = D.open_query(lib, fn, spec, as_map)
        assert q is None and msg == text
    for spec in ("family=gaussian", "family=normal", "offset=null", "vcov=sandwich", "<null>"):
        q, msg = D.open_query(lib, fn, spec)
        assert q, msg
        lib.ag_close(q)
    q, msg = D.open_query(lib, fn, "<scalar>")   # (the shared option visitor's rule, hip_options.hpp)
    assert q is None and msg == "Options must be a MAP or STRUCT, got DOUBLE"
    q, msg = D.open_query(lib, fn, "interval=both")   # read by the fit-predict aggregate alone
    if "predict" in fn:
        assert q is None and msg == "Unknown interval 'both'. Expected 'none', 'confidence' or 'prediction'."
    else:
        assert q, msg
        lib.ag_close(q)


def test_glue_under_sanitizers_on_a_mock_abi(tmp_path):
    """glmm_family_hip.cpp + its driver with a mock of the C ABI under ASan / UBSan, -Wall -Wextra -Werror, as a stand-alone
    program (tests/tools/glmm_glue_sanitize.cpp).  The child inherits the environment unchanged; where a process-wide LD_PRELOAD is
    set a sanitizer's runtime could not be the first one loaded, so there the same program is built without the sanitizers and the
    scenarios still run (as tests/test_aft_glue_cpu.py does)."""
    exe = str(tmp_path / "glmm_glue_sanitize")
    sanitize = [] if os.environ.get("LD_PRELOAD") else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *sanitize, "-fno-omit-frame-pointer", "-g", "-O1",
                        "-I" + os.path.join(D.TOOLS, "duckdb_stub"), "-I" + os.path.join(ROOT, "include"), "-I" + D.SHIM,
                        os.path.join(D.TOOLS, "glmm_glue_sanitize.cpp"), os.path.join(D.TOOLS, "glmm_family_capi.cpp"),
                        os.path.join(D.SHIM, "glmm_family_hip.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "glmm_glue_sanitize: ok" in r.stdout, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
