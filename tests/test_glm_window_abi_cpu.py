"""The GLM window function's C ABI and Python plumbing without a GPU: the ctypes signatures against the header, every argument
error and its text (all answered before a device is needed), and the planner's runs under the test hooks
(anofox_hip_glm_window_plan works on host arrays)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import glm_window_cases as WC
from conftest import ROOT, import_pkg

SYMBOLS = {"anofox_hip_glm_fit_predict_window_device": 14, "anofox_hip_glm_fit_predict_window_host": 14,
           "anofox_hip_glm_fit_predict_frames_device": 13, "anofox_hip_glm_fit_predict_frames_host": 13,
           "anofox_hip_glm_window_plan": 11, "anofox_hip_glm_window_test_hooks": 3, "anofox_hip_glm_window_stats": 3}
_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)


@pytest.fixture(autouse=True)
def _reset_hooks():
    yield
    import_pkg().glm_window_test_hooks(0, 0, True)


def test_symbols_and_signatures_against_the_header():
    abi = import_pkg("_abi")
    with open(os.path.join(ROOT, "include", "anofox_stats_hip.h")) as f:
        h = f.read()
    lib = abi.load()
    for sym, n in SYMBOLS.items():
        res, args = abi.SYMBOLS[sym]
        decl = re.search(r"\b" + sym + r"\(([^;]*)\);", h)
        assert decl and len(decl.group(1).split(",")) == n == len(args), sym
        assert getattr(lib, sym).argtypes == args
    err = abi._ERRP
    host, q = abi.SYMBOLS["anofox_hip_glm_fit_predict_window_host"][1], abi.SYMBOLS["anofox_hip_quantile_fit_predict_window_host"][1]
    assert host[:7] == q[:7] and host[7] == _DP and host[8] is abi.AnofoxHipWindowFrame and host[9] is abi.AnofoxHipGlmBatchOptions
    assert host[10:] == [C.c_double, _DP, _DP, err]
    fr = abi.SYMBOLS["anofox_hip_glm_fit_predict_frames_host"][1]
    assert fr[:5] == [abi._CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP)] and fr[5:8] == [_DP, _I64P, _I64P] and fr[8:] == host[9:]
    for sym in ("anofox_hip_glm_fit_predict_window_device", "anofox_hip_glm_fit_predict_frames_device"):
        assert abi.SYMBOLS[sym][0] is C.c_bool and abi.SYMBOLS[sym][1][-4:] == [C.c_double, C.c_void_p, C.c_void_p, err]
    pkg = import_pkg()
    for name in ("poisson_fit_predict", "logistic_fit_predict", "binomial_fit_predict", "glm_fit_predict_window_host",
                 "glm_fit_predict_frames_host", "glm_fit_predict_window_device", "glm_fit_predict_frames_device", "glm_window_stats",
                 "glm_window_plan", "glm_window_test_hooks"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("poisson_fit_predict", "logistic_fit_predict", "binomial_fit_predict"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.SQL_FUNCTIONS["anofox_stats_" + name] is getattr(pkg, name)
    assert callable(pkg.Context.glm_fit_predict_window_device) and callable(pkg.Context.glm_fit_predict_frames_device)


def _host_args():
    abi = import_pkg("_abi")
    n = 8
    y = np.ones(n)
    off = np.array([0, n], dtype=np.int64)
    c = y.ctypes.data_as(_DP)
    return abi, abi.load(), n, y, off, c


def test_every_argument_error_and_its_text():
    abi, lib, n, y, off, c = _host_args()
    err = abi.AnofoxError()
    po = abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    bo = abi.AnofoxHipGlmBatchOptions(1, True, 100, 1e-8, 0.0, False, 0.95)
    fr = abi.AnofoxHipWindowFrame(5, 0)
    offp, cols = off.ctypes.data_as(_I64P), (_DP * 2)(c, c)
    pred = np.full((n, 3), 7.0)
    pp = pred.ctypes.data_as(_DP)
    lo, hi = np.zeros(n, dtype=np.int64), np.arange(1, n + 1, dtype=np.int64)
    lop, hip = lo.ctypes.data_as(_I64P), hi.ctypes.data_as(_I64P)

    def window(G=1, p=2, N=n, o=offp, yy=c, xc=cols, frame=fr, opts=po, z=0.0, pr=pp):
        assert not lib.anofox_hip_glm_fit_predict_window_host(None, G, p, N, o, yy, xc, None, frame, opts, z, pr, None, C.byref(err))
        assert err.code == 1
        return err.text()

    def frames(p=2, N=n, yy=c, xc=cols, a=lop, b=hip, opts=po, z=0.0, pr=pp):
        assert not lib.anofox_hip_glm_fit_predict_frames_host(None, N, p, yy, xc, None, a, b, opts, z, pr, None, C.byref(err))
        assert err.code == 1
        return err.text()

    assert "negative n_groups or n_rows" in window(G=-1) and "negative n_groups or n_rows" in window(N=-1)
    assert "negative n_groups or n_rows" in frames(N=-1)
    for f in (window, frames):
        assert "glm: interval_z must be finite and not negative" in f(z=-1.0)
        assert "glm: interval_z must be finite and not negative" in f(z=float("nan"))
        assert "glm: the prediction interval of the binomial family is not built" in f(opts=bo, z=1.96)
        assert "x is NULL or empty" in f(p=0) and "x is NULL or empty" in f(xc=None)
        assert "glm: n_features > 32 is not built" in f(p=33, xc=(_DP * 33)(*[c] * 33))
        assert "y or pred is NULL" in f(yy=None) and "y or pred is NULL" in f(pr=None)
        assert "x column pointer is NULL" in f(xc=(_DP * 2)(c, None))
    assert "window frame must start at or before its end" in window(frame=abi.AnofoxHipWindowFrame(1, 2))
    assert "row_offsets is NULL" in window(o=None)
    assert "row_offsets must start at 0 and end at n_rows" in window(o=np.array([0, n - 1], dtype=np.int64).ctypes.data_as(_I64P))
    assert "row_offsets must be non-decreasing" in window(G=2, o=np.array([0, n, n - 1], dtype=np.int64).ctypes.data_as(_I64P))
    assert "frame_lo or frame_hi is NULL" in frames(a=None) and "frame_lo or frame_hi is NULL" in frames(b=None)
    assert "frame bounds must lie within [0, n_rows]" in frames(b=(hi + 1).ctypes.data_as(_I64P))
    assert np.all(pred == 7.0)
    # the device forms: the same checks, then the context
    fake = C.c_void_p(y.ctypes.data)
    vcols = (C.c_void_p * 2)(fake, fake)
    assert not lib.anofox_hip_glm_fit_predict_window_device(None, 1, 2, n, fake, fake, vcols, None, fr, bo, 1.96, fake, None, C.byref(err))
    assert err.code == 1 and "glm: the prediction interval of the binomial" in err.text()
    assert not lib.anofox_hip_glm_fit_predict_window_device(None, 1, 2, n, fake, fake, vcols, None, fr, po, 0.0, fake, None, C.byref(err))
    assert err.code == 1 and "context is NULL" in err.text()
    assert not lib.anofox_hip_glm_fit_predict_frames_device(None, n, 2, fake, vcols, None, fake, fake, po, 0.0, fake, None, C.byref(err))
    assert err.code == 1 and "context is NULL" in err.text()
    assert not lib.anofox_hip_glm_fit_predict_frames_device(None, n, 33, fake, (C.c_void_p * 33)(*[fake] * 33), None, fake, fake, po, 0.0,
                                                            fake, None, C.byref(err))
    assert "glm: n_features > 32 is not built" in err.text()
    # nothing to do: no rows or no groups, nothing touched, no device needed
    assert lib.anofox_hip_glm_fit_predict_window_host(None, 0, 2, 0, None, None, cols, None, fr, po, 0.0, None, None, C.byref(err))
    assert lib.anofox_hip_glm_fit_predict_frames_host(None, 0, 2, None, cols, None, None, None, po, 0.0, None, None, C.byref(err))
    assert not lib.anofox_hip_glm_window_stats(None, None, C.byref(err)) and "out is NULL" in err.text()
    assert not lib.anofox_hip_glm_window_plan(1, offp, n, None, hip, None, 0, None, None, None, C.byref(err))
    assert "glm window plan: a NULL or negative argument" in err.text()


def test_python_argument_errors():
    pkg = import_pkg()
    rng = np.random.default_rng(5)
    n = 12
    keys, order, y, x = np.zeros(n, dtype=np.int64), np.arange(n), rng.poisson(2.0, n).astype(float), rng.normal(size=(n, 2))
    for fn in (pkg.poisson_fit_predict, pkg.logistic_fit_predict, pkg.binomial_fit_predict):
        with pytest.raises(pkg.InvalidInputException):
            fn(keys, order, y, x, frame=(1, 3))
        with pytest.raises(pkg.InvalidInputException):
            fn(keys[:-1], order, y, x)
        with pytest.raises(pkg.InvalidInputException):
            fn(keys, order, y, x, {"offset": 3})
        with pytest.raises(pkg.AnofoxStatsError, match="n_features > 32 is not built"):
            fn(keys, order, y, rng.normal(size=(n, 33)))
    with pytest.raises(pkg.AnofoxStatsError, match="prediction interval of the binomial family"):
        pkg.logistic_fit_predict(keys, order, (y > 1).astype(float), x, {"interval": True})
    o = pkg.parse_poisson_options(None).batch_options()
    with pytest.raises(ValueError):
        pkg.glm_fit_predict_frames_host(np.zeros(4), [np.zeros(4)], [0, 0, 0], [1, 2, 3], o)
    with pytest.raises(ValueError):
        pkg.glm_fit_predict_window_host([0, 4], np.zeros(4), [np.zeros(4)], o, offset=np.zeros(3))


def _check_cover(runs, off):
    assert runs[0] == off[0] and runs[-1] == off[-1] and (np.diff(runs) > 0).all()
    assert set(int(v) for v in off[1:-1] if off[0] < v < off[-1]) <= set(int(v) for v in runs), "a run crosses a partition"


def test_planner_runs_under_the_hooks():
    pkg = import_pkg()
    plan, hooks = pkg.glm_window_plan, pkg.glm_window_test_hooks
    # the library's rule: the quantile window's cut (shared code); the span is the longest FRAME, not the longest chain
    sizes = np.array([100, 0, 37, 1, 0, 127, 64, 65] * 50)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lo, hi = WC.rows_frames(off, 30, 0)
    runs, span, waves = plan(off, lo, hi)
    _check_cover(runs, off)
    assert list(runs) == sorted(set(int(v) for v in off)) and waves == len(runs) - 1 and span == 31
    qruns, qspan, _ = pkg.quantile_window_plan(off, lo, hi)
    assert np.array_equal(runs, qruns) and qspan == 127
    off = np.array([0, 250, 300], dtype=np.int64)
    lo, hi = WC.rows_frames(off, 30, 0)
    assert [list(plan(off, lo, hi)[0]), plan(off, lo, hi)[1:]] == [[0, 84, 168, 250, 300], (31, 4)]
    lo_u, hi_u = WC.rows_frames(off, None, 0)
    assert list(plan(off, lo_u, hi_u)[0]) == [0, 250, 300] and plan(off, lo_u, hi_u)[1:] == (250, 2)
    # the run-length hook: runs of exactly that many rows in every partition
    for L in (1, 7):
        hooks(L, 0, True)
        runs_l, span_l, waves_l = plan(off, lo, hi)
        _check_cover(runs_l, off)
        assert np.array_equal(runs_l, WC.cut_runs(dict(offsets=off), L)) and span_l == 31 and waves_l == len(runs_l) - 1
    # the cap lowers the launched wavefronts, never the walkers; 16 bytes per row of the longest frame
    hooks(7, 16 * 31 * 3 + 15, True)
    runs_c, span_c, waves_c = plan(off, lo, hi)
    assert np.array_equal(runs_c, runs_l) and span_c == 31 and waves_c == 3
    hooks(0, 16 * 250, True)
    assert plan(off, lo_u, hi_u)[2] == 1
    hooks(0, 16 * 250 - 1, True)
    with pytest.raises(pkg.AnofoxStatsError, match=r"glm window: frame of 250 rows exceeds the scratch budget") as ei:
        plan(off, lo_u, hi_u)
    assert ei.value.code == 1
    hooks(0, 0, True)
    # explicit frames: empty ones (any bounds) own no scratch; far-apart frames cost one frame
    lo_e = np.array([0, 5, 5, 2, 9, 0, -4, 7, 7, 7], dtype=np.int64)
    hi_e = np.array([3, 5, 4, 6, 10, 0, -9, 9, 9, 10], dtype=np.int64)
    assert plan(np.array([0, 10]), lo_e, hi_e)[1] == 4 and plan(np.array([0, 0]), [], [])[0].tolist() == [0]
    n = 100_000
    far_lo = np.where(np.arange(n) % 2 == 0, 0, n - 50).astype(np.int64)
    runs_f, span_f, waves_f = plan(np.array([0, n], dtype=np.int64), far_lo, far_lo + 50)
    assert span_f == 50 and waves_f == len(runs_f) - 1 > 1000
