"""CPU-side checks of the permutation test surface: the header compiles as C, the struct layouts (the reference's ABI), the
exported symbols, the option spellings, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, import_pkg

SYMBOLS = ("anofox_hip_perm_test_record_len", "anofox_hip_perm_test_batch_device", "anofox_hip_perm_test_batch_host",
           "anofox_hip_perm_test_hooks", "anofox_energy_distance", "anofox_mmd", "anofox_permutation_t_test")
NAN = float("nan")


def test_symbols_present():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in SYMBOLS:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
    assert lib.anofox_hip_perm_test_record_len() == 8
    pkg = import_pkg()
    for name in ("energy_distance", "mmd", "permutation_t_test", "energy_distance_agg", "mmd_agg", "permutation_t_test_agg"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.SQL_FUNCTIONS["anofox_stats_" + name] is getattr(pkg, name) and name in pkg.__all__
    for name in ("perm_test_batch_host", "perm_test_batch_device", "perm_test_hooks", "parse_perm_test_options"):
        assert callable(getattr(pkg, name)) and name in pkg.__all__
    assert callable(pkg.Context.perm_test_batch_host) and callable(pkg.Context.perm_test_batch_device)


def test_header_compiles_as_c_and_layouts_match_reference_abi():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "anofox_stats_hip.h"
#define O(T, f) printf("%zu ", offsetof(T, f))
int main(void) {
  printf("%zu %zu %zu\n", sizeof(AnofoxEnergyDistanceOptions), sizeof(AnofoxMmdOptions), sizeof(AnofoxHipPermTestBatchOptions));
  O(AnofoxEnergyDistanceOptions, n_permutations); O(AnofoxEnergyDistanceOptions, seed); O(AnofoxEnergyDistanceOptions, has_seed);
  O(AnofoxMmdOptions, n_permutations); O(AnofoxMmdOptions, seed); O(AnofoxMmdOptions, has_seed);
  printf("\n");
  O(AnofoxHipPermTestBatchOptions, test); O(AnofoxHipPermTestBatchOptions, alternative);
  O(AnofoxHipPermTestBatchOptions, n_permutations); O(AnofoxHipPermTestBatchOptions, seed); O(AnofoxHipPermTestBatchOptions, sigma);
  printf("\n");
  return 0;
}
'''
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        with open(src, "w") as f:
            f.write(prog)
        r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = subprocess.run([exe], capture_output=True, text=True).stdout.split("\n")
    assert lines[0].split() == ["24", "24", "32"]
    assert lines[1].split() == ["0", "8", "16"] * 2
    assert lines[2].split() == ["0", "4", "8", "16", "24"]
    abi = import_pkg("_abi")
    assert C.sizeof(abi.AnofoxEnergyDistanceOptions) == C.sizeof(abi.AnofoxMmdOptions) == 24
    assert C.sizeof(abi.AnofoxHipPermTestBatchOptions) == 32
    assert [getattr(abi.AnofoxHipPermTestBatchOptions, f).offset for f in ("test", "alternative", "n_permutations", "seed", "sigma")] == \
        [0, 4, 8, 16, 24]


def test_option_spellings_and_defaults():
    pkg = import_pkg()
    o = pkg.parse_perm_test_options({"N_Permutations": 50, "SEED": 7, "sigma": "1.5", "Alternative": "LESS", "other": 1})
    assert (o.n_permutations, o.seed, o.sigma, o.alternative) == (50, 7, 1.5, 1)
    d = pkg.parse_perm_test_options(None)
    assert d.permutations(0) == 1000 and d.permutations(1) == 10000 and d.permutations(2) == 1000 and d.seed is None
    r = d.resolved()
    assert isinstance(r.seed, int) and 0 <= r.seed < 2 ** 64 and d.seed is None
    b = o.batch_options(2)
    assert (b.test, b.alternative, b.n_permutations, b.seed, b.sigma) == (2, 1, 50, 7, 1.5)
    assert pkg.PermTestOptions(seed=1).batch_options(0).sigma != pkg.PermTestOptions(seed=1).batch_options(0).sigma   # NaN
    with pytest.raises(pkg.InvalidInputException, match="need a seed"):
        d.batch_options(0)
    with pytest.raises(pkg.InvalidInputException, match="n_permutations"):
        pkg.PermTestOptions(2000000, 1).batch_options(0)
    with pytest.raises(pkg.InvalidInputException):
        pkg.parse_perm_test_options("seed=1")


def _batch(lib, abi, n_groups, n_rows, off, v, s, rec, o):
    err = abi.AnofoxError()
    P = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))   # noqa: E731
    ok = lib.anofox_hip_perm_test_batch_host(None, n_groups, n_rows, P(off, C.c_int64), P(v, C.c_double), P(s, C.c_int32), o,
                                             P(rec, C.c_double), C.byref(err))
    return ok, err.text()


def test_batch_argument_errors_before_any_device():
    abi = import_pkg("_abi")
    lib = abi.load()
    off, v, s, rec = np.array([0, 4], np.int64), np.arange(4.0), np.array([0, 0, 1, 1], np.int32), np.zeros(8)
    O = abi.AnofoxHipPermTestBatchOptions
    good = O(0, 0, 10, 1, NAN)
    for o, text in ((O(3, 0, 10, 1, NAN), "unknown test"), (O(-1, 0, 10, 1, NAN), "unknown test"), (O(0, 3, 10, 1, NAN), "unknown alternative"),
                    (O(0, 0, -1, 1, NAN), "n_permutations"), (O(0, 0, 1000001, 1, NAN), "n_permutations"),
                    (O(2, 0, 10, 1, float("inf")), "sigma must be finite"), (O(2, 0, 10, 1, float("-inf")), "sigma must be finite")):
        ok, msg = _batch(lib, abi, 1, 4, off, v, s, rec, o)
        assert not ok and msg.startswith("permutation test:") and text in msg, msg
    for args, text in (((-1, 4, off, v, s, rec), "negative"), ((1, -4, off, v, s, rec), "negative"), ((1, 4, None, v, s, rec), "NULL"),
                       ((1, 4, off, None, s, rec), "NULL"), ((1, 4, off, v, None, rec), "NULL"), ((1, 4, off, v, s, None), "NULL"),
                       ((1, 4, np.array([0, 5], np.int64), v, s, rec), ""), ((1, 4, np.array([3, 1], np.int64), v, s, rec), "")):
        ok, msg = _batch(lib, abi, *args, good)
        assert not ok and text in msg, msg
    err = abi.AnofoxError()
    assert lib.anofox_hip_perm_test_batch_device(None, 1, 4, 1, 1, 1, O(5, 0, 1, 1, NAN), 1, C.byref(err)) is False
    assert "unknown test" in err.text()
    ok, msg = _batch(lib, abi, 0, 0, None, None, None, None, good)   # no groups: nothing to do, nothing touched
    assert ok, msg


def test_scalar_argument_errors_before_any_device():
    pkg = import_pkg()
    two, one = [1.0, 2.0, NAN], [3.0, NAN, NAN]
    for fn, name in ((pkg.energy_distance, "Energy distance test"), (pkg.mmd, "MMD test"), (pkg.permutation_t_test, "Permutation t-test")):
        with pytest.raises(pkg.InvalidInputException, match=name + " requires at least 2 observations in group 1"):
            fn(one, two, {"seed": 1})
        with pytest.raises(pkg.InvalidInputException, match=name + " requires at least 2 observations in group 2"):
            fn(two, one, {"seed": 1})
        with pytest.raises(pkg.InvalidInputException, match="not defined on infinite values"):
            fn(two, [1.0, float("inf")], {"seed": 1})
        with pytest.raises(pkg.InvalidInputException, match="n_permutations"):
            fn(two, two, {"seed": 1, "n_permutations": 1000001})
    with pytest.raises(pkg.InvalidInputException, match="mmd: group too large"):
        pkg.mmd(np.arange(1000.0), np.arange(463.0), {"seed": 1})
    abi = import_pkg("_abi")
    lib, err = abi.load(), abi.AnofoxError()
    arr = abi.AnofoxDataArray()
    assert lib.anofox_energy_distance(arr, arr, abi.AnofoxEnergyDistanceOptions(10, 1, True), None, C.byref(err)) is False
    assert "out_result is NULL" in err.text()
    res = abi.AnofoxTestResult()
    assert lib.anofox_permutation_t_test(arr, arr, 7, 10, 1, True, C.byref(res), C.byref(err)) is False
    assert "unknown alternative" in err.text() and not res.method
