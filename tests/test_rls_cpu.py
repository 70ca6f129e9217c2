"""CPU tier of recursive least squares: the NumPy restatement of the reference's filter (tests/rls_restate.py) against the
reference's own expectations and against textbook RLS; csrc/rls_filter.h compiled for the host, bit for bit against the
restatement; the options parser, the ABI surface and the entry points' argument checks without a device."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, import_pkg

sys.path.insert(0, os.path.dirname(__file__))
import rls_restate as R  # noqa: E402

CSRC = os.path.join(ROOT, "anofox-statistics_amd", "csrc")
HEADER_DIR = os.path.join(ROOT, "include")
CXX = "/opt/rocm/llvm/bin/clang++" if os.path.exists("/opt/rocm/llvm/bin/clang++") else (shutil.which("clang++") or shutil.which("g++"))


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_restatement_reference_unit_tests():
    xs = np.arange(1.0, 21.0)
    rec = R.rls_fit(2 * xs + 1, xs[:, None])                   # rls.rs test_rls_batch_fit
    assert rec[1 + 4] == 20 and rec[1 + 5] == 0
    assert 1.9 < rec[0] < 2.1
    assert abs(R.predict(rec, [25.0]) - 51.0) < 1.0
    for n in (10, 50):                                          # n_observations of the SQL tests
        x = np.arange(1.0, n + 1)
        assert R.rls_fit(3 * x - 1 + np.sin(x), x[:, None])[1 + 4] == n
    rec = R.rls_fit(2 * xs, xs[:, None], fit_intercept=False)   # rls.rs test_rls_no_intercept
    assert np.isnan(rec[1]) and abs(rec[0] - 2.0) < 0.1


def test_restatement_differs_from_textbook_rls():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(200, 3))
    y = X @ np.array([1.0, -2.0, 0.5]) + 0.1 * rng.normal(size=200)
    quirk = R.rls_fit(y, X, forgetting_factor=0.99)
    textbook = R.rls_fit(y, X, forgetting_factor=0.99, textbook=True)
    assert np.max(np.abs(quirk[:4] - textbook[:4])) > 1e-6     # the in-place P update is really reproduced


# ---- rls_filter.h on the host ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_filter(tmp_path_factory):
    if CXX is None:
        pytest.skip("needs a C++ compiler")
    exe = str(tmp_path_factory.mktemp("rls") / "rls_filter_host")
    subprocess.check_call([CXX, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-pass-failed", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "tools", "rls_filter_host.cpp"), "-o", exe])
    return exe


def _run_host(exe, tmp_path, cases):
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        for y, X, lam, delta, icpt in cases:
            n, p = X.shape
            f.write(np.array([p, int(icpt)], dtype=np.int32).tobytes() + np.array([n], dtype=np.int64).tobytes())
            f.write(np.array([lam, delta], dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(y, dtype=np.float64).tobytes() + np.ascontiguousarray(X.T, dtype=np.float64).tobytes())
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    recs = np.fromfile(out, dtype=np.float64)
    res, k = [], 0
    for _, X, *_ in cases:
        p = X.shape[1]
        res.append(recs[k:k + p + 6])
        k += p + 6
    return res


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def _case(rng, n, p, lam, icpt=True, const=(), bad_rows=0):
    X = rng.normal(size=(n, p))
    for j in const:
        X[:, j] = -1.5
    y = X @ rng.normal(size=p) + 0.7 + 0.2 * rng.normal(size=n)
    for k in range(bad_rows):
        r = rng.integers(0, n)
        if k % 2:
            y[r] = np.nan
        else:
            X[r, rng.integers(0, p)] = np.inf
    return y, X, lam, 100.0, icpt


def test_host_filter_bit_identical(host_filter, tmp_path):
    rng = np.random.default_rng(2024)
    cases = []
    for p in list(range(1, 9)) + [12, 33]:
        for lam in (1.0, 0.99, 0.95):
            n = 60 if p > 8 else 120
            cases.append(_case(rng, n, p, lam, icpt=bool(p % 2), const=(0,) if p > 3 else (), bad_rows=4))
    cases.append(_case(rng, 1000, 3, 0.99))                   # the divergent case: coefficients ~1e11, chaotic
    for got, (y, X, lam, delta, icpt) in zip(_run_host(host_filter, tmp_path, cases), cases):
        want = R.rls_fit(y, X, forgetting_factor=lam, initial_p_diagonal=delta, fit_intercept=icpt)
        assert _same_bits(got, want), (X.shape, lam, icpt, got, want)


def test_host_filter_shortcut_statuses_and_option_quirk(host_filter, tmp_path):
    X1 = np.full((5, 2), 2.0)
    y1 = np.array([1.0, 2.0, 3.0, np.nan, 5.0])
    X2 = np.array([[1.0], [2.0], [3.0]])
    y2 = np.array([1.0, 2.0, 4.0])
    Xn = np.array([[np.nan], [1.0]])
    yn = np.array([1.0, np.nan])
    cases = [(y1, X1, 1.0, 100.0, True),     # intercept-only: mean of y
             (y1, X1, 0.0, -1.0, True),      # ... whose options are never checked
             (y1, X1, 1.0, 100.0, False),    # all constant, no intercept: 6
             (y2, X2, 0.0, 100.0, True),     # forgetting factor outside (0, 1]: 1
             (y2, X2, 1.0001, 100.0, True),
             (y2, X2, 0.5, 0.0, True),       # P diagonal <= 0: 1
             (y2, X2, np.nan, 100.0, True),  # NaN passes the reference's comparisons
             (yn, Xn, 1.0, 100.0, True)]     # no valid row: 10
    got = _run_host(host_filter, tmp_path, cases)
    for g, (y, X, lam, delta, icpt) in zip(got, cases):
        assert _same_bits(g, R.rls_fit(y, X, forgetting_factor=lam, initial_p_diagonal=delta, fit_intercept=icpt))
    assert [int(g[-1]) for g in got] == [0, 0, 6, 1, 1, 1, 0, 10]
    assert got[0][2] == (1.0 + 2.0 + 3.0 + 5.0) / 4 and np.all(np.isnan(got[0][:2]))


# ---- surface --------------------------------------------------------------------------------------------------------
def test_options_parser():
    o = import_pkg("options")
    r = o.parse_rls_options(None)
    assert (r.forgetting_factor, r.initial_p_diagonal, r.fit_intercept) == (1.0, 100.0, True)
    r = o.parse_rls_options({"Forgetting_Factor": 0.9, "p_diagonal": 5, "intercept": False, "confidence": 0.9})
    assert (r.forgetting_factor, r.initial_p_diagonal, r.fit_intercept, r.confidence_level) == (0.9, 5.0, False, 0.9)
    assert o.parse_rls_options({"initial_p_diagonal": 7.0}).initial_p_diagonal == 7.0
    assert o.parse_rls_options({"lambda": 0.99}).forgetting_factor == 1.0   # test_scalar_functions.test's quirk
    assert o.parse_rls_options({"unknown": "x", "alpha": 3}).forgetting_factor == 1.0
    for bad in ({"intercept": "yes"}, {"null_policy": "keep"}, {"max_iterations": -1}, {"max_iter": 1 << 33}):
        with pytest.raises(o.InvalidInputException):
            o.parse_rls_options(bad)
    with pytest.raises(ValueError):
        o.parse_rls_options({"lambda": "abc"})


def test_rls_options_layout_and_header_guard(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(AnofoxRlsOptions), offsetof(AnofoxRlsOptions, fit_intercept),
         offsetof(AnofoxRlsOptions, initial_p_diagonal), sizeof(AnofoxHipRlsBatchOptions));
  return 0;
}
'''
    src, exe = tmp_path / "t.c", str(tmp_path / "t")
    src.write_text(prog)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", HEADER_DIR, str(src), "-o", exe])
    assert subprocess.check_output([exe]).decode().split() == ["24", "8", "16", "24"]
    abi = import_pkg("_abi")
    assert C.sizeof(abi.AnofoxRlsOptions) == 24 and abi.AnofoxRlsOptions.initial_p_diagonal.offset == 16
    # after the reference's own header (ANOFOX_STATS_FFI_H defined, AnofoxRlsOptions from there), the batched RLS surface
    # still compiles: the reference's types come from a stand-in that declares exactly what this header then skips
    ref = tmp_path / "anofox_stats_ffi.h"
    ref.write_text("#ifndef ANOFOX_STATS_FFI_H\n#define ANOFOX_STATS_FFI_H\n#include <stdbool.h>\n#include <stddef.h>\n#include <stdint.h>\n"
                   + _reference_guarded_block() + "#endif\n")
    guard = tmp_path / "g.c"
    guard.write_text('#include "anofox_stats_ffi.h"\n#include "anofox_stats_hip.h"\n'
                     'int main(void) { AnofoxRlsOptions r = {0.99, true, 10.0}; AnofoxHipRlsBatchOptions o = {true, 0.99, 10.0};\n'
                     '  void *f[2] = {(void *)anofox_hip_rls_fit_batch_host, (void *)anofox_rls_fit}; (void)r; (void)o; return f[0] == f[1]; }\n')
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", str(tmp_path), "-I", HEADER_DIR, str(guard)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _reference_guarded_block():
    """The declarations of include/anofox_stats_hip.h's (1) block, lifted out of the header, as the reference's header would
    provide them (same types and prototypes, here without the export macro)."""
    src = open(os.path.join(HEADER_DIR, "anofox_stats_hip.h")).read()
    block = src[src.index("#ifndef ANOFOX_STATS_FFI_H") + len("#ifndef ANOFOX_STATS_FFI_H"):src.index("#endif /* ANOFOX_STATS_FFI_H */")]
    return block.replace("ANOFOX_HIP_API ", "")


def test_prototypes_match_the_header():
    abi = import_pkg("_abi")
    for name in ("anofox_rls_fit", "anofox_hip_rls_fit_batch_device", "anofox_hip_rls_fit_batch_host",
                 "anofox_hip_rls_fit_predict_batch_device", "anofox_hip_rls_fit_predict_batch_host",
                 "anofox_hip_rls_fit_predict_window_device", "anofox_hip_rls_fit_predict_window_host",
                 "anofox_hip_rls_fit_predict_frames_device", "anofox_hip_rls_fit_predict_frames_host"):
        assert name in abi.SYMBOLS
        assert name in open(os.path.join(HEADER_DIR, "anofox_stats_hip.h")).read()


def test_sql_names_resolve():
    pkg = import_pkg()
    for name in ("anofox_stats_rls_fit_agg", "rls_fit_agg", "anofox_stats_rls_fit_predict_agg", "rls_fit_predict_agg",
                 "rls_predict_agg", "anofox_stats_rls_predict_agg", "anofox_stats_rls_fit_predict", "rls_fit_predict",
                 "anofox_stats_rls_fit", "rls_fit"):
        assert name in pkg.SQL_FUNCTIONS


def test_entry_points_fail_without_a_device_after_argument_checks():
    import torch
    abi = import_pkg("_abi")
    lib = abi.load()
    err = abi.AnofoxError()
    core = abi.AnofoxFitResultCore()
    opt = abi.AnofoxRlsOptions(1.0, True, 100.0)
    y = abi.AnofoxDataArray()
    assert not lib.anofox_rls_fit(y, None, 0, opt, C.byref(core), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "x is NULL or empty"
    bo = abi.AnofoxHipRlsBatchOptions(True, 1.0, 100.0)
    off = (C.c_int64 * 2)(0, 3)
    ys = (C.c_double * 3)(1.0, 2.0, 3.0)
    xcol = (C.c_double * 3)(1.0, 2.0, 4.0)
    cols = (C.POINTER(C.c_double) * 1)(C.cast(xcol, C.POINTER(C.c_double)))
    out = (C.c_double * 7)()
    dp = C.POINTER(C.c_double)
    # argument errors come first, with or without a device
    assert not lib.anofox_hip_rls_fit_batch_host(None, 1, 0, 3, off, C.cast(ys, dp), cols, bo, C.cast(out, dp), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT
    assert not lib.anofox_hip_rls_fit_batch_host(None, 1, 200, 3, off, C.cast(ys, dp), cols, bo, C.cast(out, dp), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT
    bad_off = (C.c_int64 * 2)(0, 9)
    assert not lib.anofox_hip_rls_fit_batch_host(None, 1, 1, 3, bad_off, C.cast(ys, dp), cols, bo, C.cast(out, dp), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT
    frame = abi.AnofoxHipWindowFrame(0, 3)                      # starts after its end
    assert not lib.anofox_hip_rls_fit_predict_window_host(None, 1, 1, 3, off, C.cast(ys, dp), cols, frame, bo, 0.95,
                                                          C.cast(out, dp), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT
    if torch.cuda.is_available():
        return
    # valid arguments reach the device, and there is none
    assert not lib.anofox_hip_rls_fit_batch_host(None, 1, 1, 3, off, C.cast(ys, dp), cols, bo, C.cast(out, dp), C.byref(err))
    assert err.code == abi.ERROR_INTERNAL and "no HIP device" in err.text()
    xs = (abi.AnofoxDataArray * 1)(abi.AnofoxDataArray(C.cast(xcol, dp), None, 3))
    assert not lib.anofox_rls_fit(abi.AnofoxDataArray(C.cast(ys, dp), None, 3), xs, 1, opt, C.byref(core), C.byref(err))
    assert err.code == abi.ERROR_INTERNAL


# ---- the DuckDB glue (duckdb_shim/rls_family_hip.cpp) through its test driver: binding needs no device ----
GLUE = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_rls_family_capi.so")
GLUE_NAMES = ["anofox_stats_rls_fit_predict_agg", "rls_fit_predict_agg", "rls_predict_agg", "anofox_stats_rls_predict_agg",
              "anofox_stats_rls_fit_predict", "rls_fit_predict"]


def _glue():
    import_pkg()
    lib = C.CDLL(GLUE)
    lib.enf_open.restype = C.c_void_p
    lib.enf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.enf_close.argtypes = [C.c_void_p]
    lib.enf_registered.argtypes = [C.c_void_p, C.c_char_p]
    lib.enf_overloads.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
    lib.enf_result_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    return lib


def test_glue_names_overloads_and_result_types_bind():
    lib = _glue()
    msg = C.create_string_buffer(512)
    for fn in GLUE_NAMES[:4]:
        for spec, split in ((None, 0), ("forgetting_factor=0.9", 0), (None, 1), ("p_diagonal=10;lambda=0.99", 1)):
            q = lib.enf_open(fn.encode(), None if spec is None else spec.encode(), 0, split, msg)
            assert q, (fn, spec, split, msg.value.decode())
            fields = C.c_int()
            assert lib.enf_result_shape(q, C.byref(fields)) == 0 and fields.value == 5
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.enf_overloads(q, fn.encode(), ov)]) == [2, 3, 3, 4]
            for name in GLUE_NAMES + ["anofox_stats_rls_fit_agg", "rls_fit_agg"]:
                assert lib.enf_registered(q, name.encode()) == 1, name
            for name in ("anofox_stats_rls_fit_agg", "rls_fit_agg"):
                assert sorted(ov[:lib.enf_overloads(q, name.encode(), ov)]) == [2, 3]
            lib.enf_close(q)
    for fn in GLUE_NAMES[4:]:
        for spec in (None, "forgetting_factor=0.95"):
            q = lib.enf_open(fn.encode(), None if spec is None else spec.encode(), 1, 0, msg)
            assert q, (fn, spec, msg.value.decode())
            fields = C.c_int()
            assert lib.enf_result_shape(q, C.byref(fields)) == 1 and fields.value == 3
            ov = (C.c_int * 8)()
            assert sorted(ov[:lib.enf_overloads(q, fn.encode(), ov)]) == [2, 3]
            lib.enf_close(q)
    assert not lib.enf_open(b"rls_fit_predict", None, 0, 1, msg)        # the window function takes no split column


@pytest.mark.parametrize("fn", ["rls_fit_predict_agg", "rls_fit_predict"])
def test_glue_bad_options_fail_at_bind(fn):
    lib = _glue()
    msg = C.create_string_buffer(512)
    for spec, text in (("null_policy=bogus", "Invalid null_policy: 'bogus'"),
                       ("max_iterations=-1", "out of range for UINTEGER"),      # a key RLS ignores, still converted
                       ("lambda_scaling=foo", "Invalid lambda_scaling: 'foo'")):
        assert not lib.enf_open(fn.encode(), spec.encode(), 0, 0, msg)
        assert text in msg.value.decode(), msg.value.decode()


@pytest.mark.parametrize("fn", ["rls_fit_predict_agg", "rls_fit_predict"])
def test_glue_feature_count_errors_carry_no_counts(fn):
    """One state given a 2-feature row and then a 3-feature row, and a 2-feature state combined into a 3-feature state: the
    bare texts of rls_predict_aggregate.cpp / rls_fit_predict.cpp.  Both are thrown before Finalize: no device."""
    lib = _glue()
    lib.enf_feature_count_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    msg, update, combine = (C.create_string_buffer(512) for _ in range(3))
    q = lib.enf_open(fn.encode(), None, 0, 0, msg)
    assert q, msg.value.decode()
    lib.enf_feature_count_errors(q, update, combine)
    lib.enf_close(q)
    assert update.value.decode() == "Inconsistent feature count"
    assert combine.value.decode() == "Cannot combine states with different feature counts"


def test_glue_compiles_warning_free():
    shim = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
    tools = os.path.join(ROOT, "tests", "tools")
    for src in (os.path.join(shim, "rls_family_hip.cpp"), os.path.join(tools, "rls_family_capi.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(tools, "duckdb_stub"),
                            "-I" + HEADER_DIR, "-I" + shim, src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
