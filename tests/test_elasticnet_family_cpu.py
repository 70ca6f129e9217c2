"""Elastic net fit-predict family without a GPU: SQL names, option parsing (the alpha / lambda quirk of the aggregate),
the ctypes prototypes against the header, and the entry points' errors (argument errors first, then no device)."""
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import import_pkg

ROOT = Path(__file__).resolve().parents[1]
NAMES = ["anofox_stats_elasticnet_fit_predict_agg", "elasticnet_fit_predict_agg", "elasticnet_predict_agg",
         "anofox_stats_elasticnet_predict_agg", "anofox_stats_elasticnet_fit_predict", "elasticnet_fit_predict"]
ENTRY = ["anofox_hip_elasticnet_fit_predict_batch_device", "anofox_hip_elasticnet_fit_predict_batch_host",
         "anofox_hip_elasticnet_fit_predict_window_device", "anofox_hip_elasticnet_fit_predict_window_host",
         "anofox_hip_elasticnet_fit_predict_frames_device", "anofox_hip_elasticnet_fit_predict_frames_host"]


def _has_device():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_sql_names_resolve():
    pkg = import_pkg()
    for n in NAMES[:4]:
        assert pkg.SQL_FUNCTIONS[n] is pkg.elasticnet_fit_predict_agg
    for n in NAMES[4:]:
        assert pkg.SQL_FUNCTIONS[n] is pkg.elasticnet_fit_predict


def test_predict_options_and_the_alpha_lambda_quirk():
    pkg = import_pkg()
    o = pkg.parse_elasticnet_predict_options(None)
    assert (o.alpha, o.l1_ratio, o.max_iterations, o.tolerance, o.confidence_level, o.null_policy) == (1.0, 0.5, 1000, 1e-6, 0.95, "drop")
    # window bind (GetRegularizationStrength): alpha wins, lambda used without alpha
    assert pkg.parse_elasticnet_predict_options({"lambda": 0.3}).alpha == 0.3
    assert pkg.parse_elasticnet_predict_options({"lambda": 0.3, "alpha": 0.2}).alpha == 0.2
    # aggregate bind: opts.alpha only, lambda ignored
    assert pkg.parse_elasticnet_predict_options({"lambda": 0.3}, use_lambda=False).alpha == 1.0
    assert pkg.parse_elasticnet_predict_options({"Alpha": 0.2, "lambda": 0.3}, use_lambda=False).alpha == 0.2
    o = pkg.parse_elasticnet_predict_options({"confidence": 0.8, "null_policy": "DROP_Y_ZERO_X", "l1_ratio": 0.1})
    assert (o.confidence_level, o.null_policy, o.l1_ratio) == (0.8, "drop_y_zero_x", 0.1)
    with pytest.raises(pkg.InvalidInputException, match="Invalid null_policy: 'bogus'"):
        pkg.parse_elasticnet_predict_options({"null_policy": "bogus"})
    with pytest.raises(pkg.InvalidInputException, match="Invalid lambda_scaling"):
        pkg.parse_elasticnet_predict_options({"lambda_scaling": "nope"})
    # the fit aggregate's parser keeps ignoring the fit-predict keys
    e = pkg.parse_elasticnet_options({"confidence_level": 0.5, "null_policy": "bogus"})
    assert e == pkg.ElasticNetOptions()


def _ctype_choices(abi, decl):
    """The ctypes types a header parameter may be declared as in _abi.py: host pointers as typed POINTERs, device pointers
    (the d_ names of the _device forms) as c_void_p."""
    import ctypes as C
    decl = " ".join(decl.split())
    name = re.findall(r"\w+$", decl)[0]
    t = decl[: -len(name)].replace("const ", "").replace(" ", "")
    device = name.startswith("d_")
    scalars = {"int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}
    if t in scalars:
        return {scalars[t]}
    if t in ("AnofoxHipElasticNetBatchOptions", "AnofoxHipWindowFrame"):
        return {getattr(abi, t)}
    if t == "AnofoxHipContext*":
        return {abi._CTX}
    if t == "AnofoxError*":
        return {abi._ERRP}
    if t == "double*":
        return {C.c_void_p} if device else {C.POINTER(C.c_double)}
    if t == "int64_t*":
        return {C.c_void_p} if device else {C.POINTER(C.c_int64)}
    if t == "double**":   # const double *const *x_cols: the column table itself is a host array
        return {C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_double))}
    raise AssertionError(f"unmapped parameter type {decl!r}")


def test_prototypes_match_the_header():
    pkg = import_pkg()
    from importlib import import_module
    abi = import_module("anofox-statistics_amd._abi")
    hdr = (ROOT / "include" / "anofox_stats_hip.h").read_text()
    for name in ENTRY:
        m = re.search(r"ANOFOX_HIP_API bool " + name + r"\((.*?)\);", hdr, re.S)
        assert m, name
        params = [a.strip() for a in m.group(1).split(",") if a.strip()]
        restype, argtypes = _find_proto(abi, name)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (decl, got) in enumerate(zip(params, argtypes)):
            assert got in _ctype_choices(abi, decl), (name, k, decl, got)
        assert getattr(pkg._abi.load(), name) is not None


def _find_proto(abi, name):
    for v in vars(abi).values():
        if isinstance(v, dict) and name in v:
            return v[name]
    raise AssertionError(f"no prototype for {name}")


@pytest.mark.skipif(_has_device(), reason="checks the library's no-device error path")
def test_entry_points_fail_without_a_device_after_argument_checks():
    pkg = import_pkg()
    off = np.array([0, 4], dtype=np.int64)
    y = np.arange(4.0)
    x = [np.arange(4.0) ** 2]
    o = pkg.ElasticNetOptions().batch_options()
    with pytest.raises(pkg.AnofoxStatsError, match="no HIP device"):
        pkg.elasticnet_fit_predict_batch_host(off, y, x, o)
    with pytest.raises(pkg.AnofoxStatsError, match="no HIP device"):
        pkg.elasticnet_fit_predict_window_host(off, y, x, o)
    with pytest.raises(pkg.AnofoxStatsError, match="no HIP device"):
        pkg.elasticnet_fit_predict_frames_host(y, x, np.zeros(4), np.full(4, 4), o)
    # argument errors come before any device use (the _device forms, with a placeholder context handle that their checks
    # reject the call before touching)
    import ctypes as C
    lib = pkg._abi.load()
    dummy = C.c_void_p(1)
    cols = (C.c_void_p * 129)()
    frame = pkg._abi.AnofoxHipWindowFrame(0, 0)

    def expect(match, call):
        err = pkg._abi.AnofoxError()
        assert not call(C.byref(err))
        assert re.search(match, err.text()), err.text()

    bad = pkg.ElasticNetOptions(tolerance=-1.0).batch_options()
    expect("exceeds the supported maximum", lambda e: lib.anofox_hip_elasticnet_fit_predict_batch_device(
        dummy, 0, 129, 0, None, None, cols, None, o, 0.95, None, None, e))
    expect("tolerance must be >= 0", lambda e: lib.anofox_hip_elasticnet_fit_predict_window_device(
        dummy, 0, 1, 0, None, None, cols, frame, bad, 0.95, None, e))
    expect("window frame must start at or before its end", lambda e: lib.anofox_hip_elasticnet_fit_predict_window_device(
        dummy, 0, 1, 0, None, None, cols, pkg._abi.AnofoxHipWindowFrame(0, 3), o, 0.95, None, e))
    expect("unknown lambda_scaling", lambda e: lib.anofox_hip_elasticnet_fit_predict_frames_device(
        dummy, 0, 1, None, cols, None, None, pkg._abi.AnofoxHipElasticNetBatchOptions(True, 1.0, 0.5, 10, 1e-6, 7), 0.95, None, e))
    expect("context is NULL", lambda e: lib.anofox_hip_elasticnet_fit_predict_batch_device(
        None, 0, 1, 0, None, None, cols, None, o, 0.95, None, None, e))


# ---- the DuckDB glue (duckdb_shim/elasticnet_family_hip.cpp) through its test driver: binding needs no device ----
GLUE = ROOT / "anofox-statistics_amd" / "duckdb_shim" / "libanofox_elasticnet_family_capi.so"


def _glue():
    import ctypes as C
    import_pkg()
    lib = C.CDLL(str(GLUE))
    lib.enf_open.restype = C.c_void_p
    lib.enf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.enf_close.argtypes = [C.c_void_p]
    lib.enf_registered.argtypes = [C.c_void_p, C.c_char_p]
    lib.enf_overloads.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.enf_result_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    return lib


def test_glue_names_overloads_and_result_types_bind():
    import ctypes as C
    lib = _glue()
    msg = C.create_string_buffer(512)
    for fn in NAMES[:4]:
        for spec, split in ((None, 0), ("alpha=0.5", 0), (None, 1), ("alpha=0.5;l1_ratio=1", 1)):
            q = lib.enf_open(fn.encode(), None if spec is None else spec.encode(), 0, split, msg)
            assert q, (fn, spec, split, msg.value.decode())
            fields = C.c_int()
            assert lib.enf_result_shape(q, C.byref(fields)) == 0 and fields.value == 5   # LIST(STRUCT(y, yhat, lower, upper, is_training))
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.enf_overloads(q, fn.encode(), ov)]) == [2, 3, 3, 4]
            for name in NAMES[:4]:
                assert lib.enf_registered(q, name.encode()) == 1
            lib.enf_close(q)
    for fn in NAMES[4:]:
        for spec in (None, "lambda=0.5"):
            q = lib.enf_open(fn.encode(), None if spec is None else spec.encode(), 1, 0, msg)
            assert q, (fn, spec, msg.value.decode())
            fields = C.c_int()
            assert lib.enf_result_shape(q, C.byref(fields)) == 1 and fields.value == 3   # STRUCT(yhat, yhat_lower, yhat_upper)
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.enf_overloads(q, fn.encode(), ov)]) == [2, 3]
            lib.enf_close(q)
    # the window function takes no split column
    assert not lib.enf_open(b"elasticnet_fit_predict", None, 0, 1, msg)


@pytest.mark.parametrize("fn", ["elasticnet_fit_predict_agg", "elasticnet_fit_predict"])
def test_glue_bad_options_fail_at_bind(fn):
    import ctypes as C
    lib = _glue()
    msg = C.create_string_buffer(512)
    for spec, text in (("lambda_scaling=foo", "Invalid lambda_scaling: 'foo'. Valid values are 'raw', 'glmnet'"),
                       ("null_policy=bogus", "Invalid null_policy: 'bogus'. Valid values are 'drop', 'drop_y_zero_x'"),
                       ("max_iterations=-1", "out of range for UINTEGER")):
        assert not lib.enf_open(fn.encode(), spec.encode(), 0, 0, msg)
        assert text in msg.value.decode(), msg.value.decode()


@pytest.mark.parametrize("fn", ["elasticnet_fit_predict_agg", "elasticnet_fit_predict"])
def test_glue_feature_count_errors_carry_no_counts(fn):
    """One state given a 2-feature row and then a 3-feature row, and a 2-feature state combined into a 3-feature state: the
    bare texts of elasticnet_predict_aggregate.cpp / elasticnet_fit_predict.cpp.  Both are thrown before Finalize: no device."""
    import ctypes as C
    lib = _glue()
    lib.enf_feature_count_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    msg, update, combine = (C.create_string_buffer(512) for _ in range(3))
    q = lib.enf_open(fn.encode(), None, 0, 0, msg)
    assert q, msg.value.decode()
    lib.enf_feature_count_errors(q, update, combine)
    lib.enf_close(q)
    assert update.value.decode() == "Inconsistent feature count"
    assert combine.value.decode() == "Cannot combine states with different feature counts"


def test_glue_compiles_warning_free(tmp_path):
    import subprocess
    shim = ROOT / "anofox-statistics_amd" / "duckdb_shim"
    tools = ROOT / "tests" / "tools"
    for src in (shim / "elasticnet_family_hip.cpp", tools / "elasticnet_family_capi.cpp"):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", f"-I{tools / 'duckdb_stub'}",
                            f"-I{ROOT / 'include'}", f"-I{shim}", str(src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
