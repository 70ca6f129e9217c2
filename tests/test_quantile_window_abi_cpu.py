"""The quantile window function's C ABI, options and Python plumbing without a GPU: the ctypes signatures against the header,
the argument errors of quantile_fit_predict next to elasticnet_fit_predict's, and the planner as a pure function (no device
is touched: anofox_hip_quantile_window_plan works on host arrays)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import quantile_window_cases as qw
from conftest import ROOT, import_pkg

WINDOW_SYMBOLS = {"anofox_hip_quantile_fit_predict_window_device": 13, "anofox_hip_quantile_fit_predict_window_host": 13,
                  "anofox_hip_quantile_fit_predict_frames_device": 12, "anofox_hip_quantile_fit_predict_frames_host": 12,
                  "anofox_hip_quantile_window_plan": 13, "anofox_hip_quantile_window_test_hooks": 2, "anofox_hip_quantile_window_stats": 3}


def test_symbols_and_struct_layouts_against_the_header():
    abi = import_pkg("_abi")
    with open(os.path.join(ROOT, "include", "anofox_stats_hip.h")) as f:
        h = f.read()
    lib = abi.load()
    for sym, n in WINDOW_SYMBOLS.items():
        res, args = abi.SYMBOLS[sym]
        decl = re.search(r"\b" + sym + r"\(([^;]*)\);", h)
        assert decl and len(decl.group(1).split(",")) == n == len(args), sym
        assert getattr(lib, sym).argtypes == args
    err = abi.SYMBOLS["anofox_quantile_fit"][1][-1]
    host, en = abi.SYMBOLS["anofox_hip_quantile_fit_predict_window_host"][1], abi.SYMBOLS["anofox_hip_elasticnet_fit_predict_window_host"][1]
    assert host[:8] == en[:8] and host[7] is abi.AnofoxHipWindowFrame and host[8] is abi.AnofoxHipQuantileBatchOptions     # ctx .. frame as the elastic net's
    assert host[9:] == [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), err]
    fr, enf = abi.SYMBOLS["anofox_hip_quantile_fit_predict_frames_host"][1], abi.SYMBOLS["anofox_hip_elasticnet_fit_predict_frames_host"][1]
    assert fr[:7] == enf[:7] and fr[7] is abi.AnofoxHipQuantileBatchOptions and fr[8:] == host[9:]
    for sym in ("anofox_hip_quantile_fit_predict_window_device", "anofox_hip_quantile_fit_predict_frames_device"):
        assert abi.SYMBOLS[sym][0] is C.c_bool and abi.SYMBOLS[sym][1][-4:] == [C.c_void_p, C.c_void_p, C.c_void_p, err]
    # the structs the calls pass by value: AnofoxHipWindowFrame {int64 @0, int64 @8} = 16 bytes, the options 24 (double @0, bool @8,
    # uint32 @12, double @16), field names as the header declares them
    f, o = abi.AnofoxHipWindowFrame, abi.AnofoxHipQuantileBatchOptions
    assert C.sizeof(f) == 16 and [getattr(f, n).offset for n, _ in f._fields_] == [0, 8]
    assert C.sizeof(o) == 24 and [getattr(o, n).offset for n, _ in o._fields_] == [0, 8, 12, 16]
    for name, cls in (("AnofoxHipWindowFrame", f), ("AnofoxHipQuantileBatchOptions", o)):
        body = re.search(r"typedef struct \{([^}]*)\} " + name + ";", h).group(1)
        assert re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in cls._fields_], name
    pkg = import_pkg()
    for name in ("quantile_fit_predict", "quantile_fit_predict_window_host", "quantile_fit_predict_frames_host", "quantile_window_plan"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("anofox_stats_quantile_fit_predict", "quantile_fit_predict"):
        assert pkg.SQL_FUNCTIONS[name] is pkg.quantile_fit_predict
    import inspect
    assert inspect.signature(pkg.quantile_fit_predict) == inspect.signature(pkg.elasticnet_fit_predict)


def _raised(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except Exception as e:  # noqa: BLE001  (the type is what is compared)
        return type(e)
    return None


def test_argument_errors_are_elasticnet_fit_predict_s():
    """Every error below is raised before a device is needed."""
    pkg = import_pkg()
    rng = np.random.default_rng(3)
    n = 12
    keys, order, y = np.zeros(n, dtype=np.int64), np.arange(n), rng.normal(size=n)
    x = [list(r) for r in rng.normal(size=(n, 2))]
    q, en = pkg.quantile_fit_predict, pkg.elasticnet_fit_predict
    # options that are no MAP, a non-numeric value, a negative count: the options parser's exception, as the elastic net's
    for bad in ([("tau", 0.5)], {"max_iterations": -1}):
        assert _raised(q, keys, order, y, x, bad) is pkg.InvalidInputException
    t = _raised(en, keys, order, y, x, {"alpha": "median"})
    assert t is not None and _raised(q, keys, order, y, x, {"tau": "median"}) is t
    assert _raised(en, keys, order, y, x, [("alpha", 0.5)]) is pkg.InvalidInputException
    # frames and ragged x rows: the shared frame parser and row check
    for kw in (dict(frame=(1, 3)), dict(frame_end="next row")):
        assert _raised(q, keys, order, y, x, **kw) is _raised(en, keys, order, y, x, **kw) is pkg.InvalidInputException
    ragged = [r if i != 4 else r[:1] for i, r in enumerate(x)]
    assert _raised(q, keys, order, y, ragged) is _raised(en, keys, order, y, ragged) is pkg.InvalidInputException
    # mismatched lengths: whatever the elastic net's function raises
    for args in ((keys, order, y, x + [[0.0, 0.0]]), (keys[:-1], order, y, x), (keys, order[:-2], y, x)):
        t = _raised(en, *args)
        assert t is not None and _raised(q, *args) is t, args
    # p > 32: the library refuses the call with its existing message, before any context exists
    wide = [list(r) for r in rng.normal(size=(n, 33))]
    with pytest.raises(pkg.AnofoxStatsError, match="n_features > 32 is not built") as ei:
        q(keys, order, y, wide)
    assert ei.value.code == 1
    o = pkg.QuantileOptions().batch_options()
    cols = [np.zeros(4)]
    with pytest.raises(pkg.AnofoxStatsError, match="window frame must start at or before its end"):
        pkg.quantile_fit_predict_window_host([0, 4], np.zeros(4), cols, o, frame=(1, 2))
    with pytest.raises(pkg.AnofoxStatsError, match="row_offsets must start at 0 and end at n_rows"):
        pkg.quantile_fit_predict_window_host([0, 3], np.zeros(4), cols, o)
    with pytest.raises(pkg.AnofoxStatsError, match="frame bounds must lie within"):
        pkg.quantile_fit_predict_frames_host(np.zeros(4), cols, [0, 0, 0, 0], [1, 2, 3, 5], o)
    with pytest.raises(ValueError):
        pkg.quantile_fit_predict_frames_host(np.zeros(4), cols, [0, 0, 0], [1, 2, 3], o)
    # a bad tau is no argument error: the fit reports status 1 on every row (tests/test_gpu_quantile_window.py)
    assert pkg.parse_quantile_options({"tau": 1.5}).tau == 1.5


def _check_cover(runs, off):
    """Runs are consecutive, cover every row of every partition once and never cross a partition."""
    assert runs[0] == off[0] and runs[-1] == off[-1] and (np.diff(runs) > 0).all()
    inner = set(int(v) for v in off[1:-1] if off[0] < v < off[-1])
    assert inner <= set(int(v) for v in runs), "a run crosses a partition"


def test_planner_is_a_pure_function_of_offsets_and_frames():
    pkg = import_pkg()
    plan = pkg.quantile_window_plan
    # many short partitions (some empty): a run is a whole partition
    sizes = np.array([100, 0, 37, 1, 0, 127, 64, 65] * 50)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    lo, hi = qw.rows_frames(off, 30, 0)
    runs, span, waves = plan(off, lo, hi)
    _check_cover(runs, off)
    assert list(runs) == sorted(set(int(v) for v in off)) and waves == len(runs) - 1
    assert span == 127 == max(int(hi[b - 1] - lo[a]) for a, b in zip(runs[:-1], runs[1:]))
    # a partition long enough is cut, but never into runs below 64 rows
    off = np.array([0, 250, 300], dtype=np.int64)
    lo, hi = qw.rows_frames(off, 30, 0)
    runs, span, waves = plan(off, lo, hi)
    assert list(runs) == [0, 84, 168, 250, 300] and span == 84 + 30 and waves == 4
    # few long partitions: about 8192 walkers, every run's span within the bound
    off = np.array([0, 300_000, 300_000, 1_000_000], dtype=np.int64)
    lo, hi = qw.rows_frames(off, 100, 0)
    runs, span, waves = plan(off, lo, hi)
    _check_cover(runs, off)
    L = -(-1_000_000 // 8192)
    assert L == 123 and 8192 * 0.9 <= len(runs) - 1 <= 8192 + 2 and np.diff(runs).max() <= L
    assert span == max(int(hi[b - 1] - lo[a]) for a, b in zip(runs[:-1], runs[1:])) == L + 100 and waves == len(runs) - 1
    # an explicit run length; the scratch cap lowers the launched wavefronts, never the walkers
    runs7, span7, waves7 = plan(off, lo, hi, run_length=70_000)
    _check_cover(runs7, off)
    assert len(runs7) - 1 == 5 + 10 and span7 == 70_000 + 100
    _, span_c, waves_c = plan(off, lo, hi, scratch_cap_bytes=24 * (L + 100) * 10 + 23)
    assert span_c == span and waves_c == 10
    # frames that start UNBOUNDED PRECEDING span their partition: one walker per partition
    lo_u, hi_u = qw.rows_frames(off, None, 0)
    runs_u, span_u, waves_u = plan(off, lo_u, hi_u)
    assert list(runs_u) == [0, 300_000, 1_000_000] and span_u == 700_000 and waves_u == 2
    # a span that does not fit once fails the call with a plain message
    with pytest.raises(pkg.AnofoxStatsError, match=r"quantile window: frame span 700000 exceeds the scratch budget") as ei:
        plan(off, lo_u, hi_u, scratch_cap_bytes=24 * 700_000 - 1)
    assert ei.value.code == 1
    assert plan(off, lo_u, hi_u, scratch_cap_bytes=24 * 700_000)[2] == 1
    # explicit frames of any shape: empty frames own no scratch, and the span is the longest CHAIN of a run — consecutive frames
    # with non-decreasing, overlapping bounds, the walk's own rule — since the walk moves its origin wherever it begins afresh
    off1 = np.array([0, 10], dtype=np.int64)
    lo_e = np.array([0, 5, 5, 2, 9, 0, 0, 7, 7, 7], dtype=np.int64)
    hi_e = np.array([3, 5, 4, 6, 10, 0, 1, 9, 9, 10], dtype=np.int64)
    runs_e, span_e, _ = plan(off1, lo_e, hi_e, run_length=5)
    assert list(runs_e) == [0, 5, 10] and span_e == 4                     # [2, 6) alone; [7, 9) [7, 9) [7, 10) chain to 3
    assert plan(off1, lo_e, hi_e, run_length=3)[1] == 4 and plan(np.array([0, 0]), [], [])[0].tolist() == [0]
    # far-apart and unsorted small frames cost the scratch of one frame, however many rows lie between them
    n = 1_000_000
    far_lo = np.where(np.arange(n) % 2 == 0, 0, n - 50).astype(np.int64)
    runs_f, span_f, waves_f = plan(np.array([0, n], dtype=np.int64), far_lo, far_lo + 50)
    assert span_f == 50 and waves_f == len(runs_f) - 1 > 1000
    assert plan(np.array([0, n], dtype=np.int64), far_lo, far_lo + 50, scratch_cap_bytes=24 * 50)[2] == 1
