"""What the Python `*_host` functions of runtime.py and glm.py hand to the library, with a recording object in the library's place:
no GPU, no device touched.  The batch, the options and the inventory of the host entries are those of test_gpu_host_staging.py
(group sizes [0, 1, 32, 31], p = 1 and p = 3, the optional arrays once present and once absent); HOST below only says which
Python function reaches an entry and what it returns.

Per call: the symbol, the argument count of _abi.SYMBOLS, every argument acceptable to its argtype, the counts, every input
pointer the address of the array the inventory names (the arrays are contiguous and of the slot's dtype, so the address proves
both the slot and the absence of a copy), NULL for an absent optional, the p column addresses in the table, and behind every
output pointer a returned array of at least the inventory's size.  Then the error of a failed call and the returned shapes.

The "new checks" (test_short_input_is_refused): an input one element short raises ValueError and the library is not called."""
import ctypes as C

import numpy as np
import pytest

from conftest import import_pkg
from test_gpu_host_staging import ENTRIES, Cols, In, Out, batch, options

F, I = np.float64, np.int32


def _wls(opt):
    return "wls" if opt else "ols"


# name of the inventory -> (the call through the binding, the (shape, dtype) of what it returns, the batch keys it takes that can
# be short).  R is the package, d the batch, o the options, opt whether the optional arrays are present.
HOST = {
    "anofox_hip_fit_batch": (
        lambda R, d, o, opt: R.fit_batch_host(d["off"], d["y"], d["cols"], d["w"] if opt else None, o["reg"](_wls(opt), opt)),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["G"], 5 * d["p"] + 2), F) if opt else None], ("cols", "w")),
    "anofox_hip_fit_batch/ridge": (
        lambda R, d, o, opt: R.fit_batch_host(d["off"], d["y"], d["cols"], None, o["reg"]("ridge")),
        lambda d, opt: [((d["G"], d["p"] + 6), F), None], ()),
    "anofox_hip_residuals_batch": (
        lambda R, d, o, opt: R.residuals_batch_host(d["off"], d["y"], d["y_hat"], d["cols"], d["rse"] if opt else None, True, False),
        lambda d, opt: [((d["N"], 4), F), ((d["G"], 2), F)], ("cols", "y_hat", "rse")),
    "anofox_hip_vif_batch": (
        lambda R, d, o, opt: R.vif_batch_host(d["off"], d["cols"]),
        lambda d, opt: [((d["G"], d["p"] + 1), F)], ("cols",)),
    "anofox_hip_fit_predict_batch": (
        lambda R, d, o, opt: R.fit_predict_batch_host(d["off"], d["y"], d["cols"], d["w"] if opt else None, o["reg"](_wls(opt)),
                                                      d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["N"], 3), F)], ("cols", "w", "tc")),
    # (the binding reaches the expanding frame through the window entry: ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)
    "anofox_hip_fit_predict_expanding": (
        lambda R, d, o, opt: R.fit_predict_expanding_host(d["off"], d["y"], d["cols"], d["w"] if opt else None, o["reg"](_wls(opt))),
        lambda d, opt: [((d["N"], 3), F)], ("cols", "w")),
    "anofox_hip_fit_predict_window": (
        lambda R, d, o, opt: R.fit_predict_window_host(d["off"], d["y"], d["cols"], d["w"] if opt else None, o["reg"](_wls(opt)), (8, 1)),
        lambda d, opt: [((d["N"], 3), F)], ("cols", "w")),
    "anofox_hip_fit_predict_frames": (
        lambda R, d, o, opt: R.fit_predict_frames_host(d["y"], d["cols"], d["w"] if opt else None, d["lo"], d["hi"], o["reg"](_wls(opt))),
        lambda d, opt: [((d["N"], 3), F)], ("cols", "w", "lo", "hi")),
    "anofox_hip_information_criteria_batch": (
        lambda R, d, o, opt: R.information_criteria_host(d["core"], o["reg"]("ols")),
        lambda d, opt: [((d["G"], 3), F)], ()),
    "anofox_hip_elasticnet_fit_batch": (
        lambda R, d, o, opt: R.elasticnet_fit_batch_host(d["off"], d["y"], d["cols"], o["en"]),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["G"],), I)], ("cols",)),
    "anofox_hip_elasticnet_fit_predict_batch": (
        lambda R, d, o, opt: R.elasticnet_fit_predict_batch_host(d["off"], d["y"], d["cols"], o["en"], 0.95, d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["N"], 3), F)], ("cols", "tc")),
    "anofox_hip_elasticnet_fit_predict_window": (
        lambda R, d, o, opt: R.elasticnet_fit_predict_window_host(d["off"], d["y"], d["cols"], o["en"], (8, 1), 0.95),
        lambda d, opt: [((d["N"], 3), F)], ("cols",)),
    "anofox_hip_elasticnet_fit_predict_frames": (
        lambda R, d, o, opt: R.elasticnet_fit_predict_frames_host(d["y"], d["cols"], d["lo"], d["hi"], o["en"], 0.95),
        lambda d, opt: [((d["N"], 3), F)], ("cols", "lo", "hi")),
    "anofox_hip_rls_fit_batch": (
        lambda R, d, o, opt: R.rls_fit_batch_host(d["off"], d["y"], d["cols"], o["rls"]),
        lambda d, opt: [((d["G"], d["p"] + 6), F)], ("cols",)),
    "anofox_hip_rls_fit_predict_batch": (
        lambda R, d, o, opt: R.rls_fit_predict_batch_host(d["off"], d["y"], d["cols"], o["rls"], 0.95, d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["N"], 3), F)], ("cols", "tc")),
    "anofox_hip_rls_fit_predict_window": (
        lambda R, d, o, opt: R.rls_fit_predict_window_host(d["off"], d["y"], d["cols"], o["rls"], (8, 1), 0.95),
        lambda d, opt: [((d["N"], 3), F)], ("cols",)),
    "anofox_hip_rls_fit_predict_frames": (
        lambda R, d, o, opt: R.rls_fit_predict_frames_host(d["y"], d["cols"], d["lo"], d["hi"], o["rls"], 0.95),
        lambda d, opt: [((d["N"], 3), F)], ("cols", "lo", "hi")),
    "anofox_hip_bls_fit_batch": (
        lambda R, d, o, opt: R.bls_fit_batch_host(d["off"], d["y"], d["cols"], o["bls"]),
        lambda d, opt: [((d["G"], 3 * d["p"] + 6), F), ((d["G"],), I)], ("cols",)),
    "anofox_hip_bls_fit_predict_batch": (
        lambda R, d, o, opt: R.bls_fit_predict_batch_host(d["off"], d["y"], d["cols"], o["bls"], 0.95, d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["N"], 3), F)], ("cols", "tc")),
    "anofox_hip_quantile_fit_batch": (
        lambda R, d, o, opt: R.quantile_fit_batch_host(d["off"], d["y"], d["cols"], o["q"]),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["G"],), I)], ("cols",)),
    "anofox_hip_quantile_fit_predict_batch": (
        lambda R, d, o, opt: R.quantile_fit_predict_batch_host(d["off"], d["y"], d["cols"], o["q"], d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 6), F), ((d["N"], 3), F)], ("cols", "tc")),
    "anofox_hip_quantile_fit_path_batch": (
        lambda R, d, o, opt: R.quantile_fit_path_batch_host(d["off"], d["y"], d["cols"], o["q"], d["taus"]),
        lambda d, opt: [((d["G"], 3, d["p"] + 6), F), ((d["G"], 3), I)], ("cols",)),
    "anofox_hip_quantile_fit_predict_path_batch": (
        lambda R, d, o, opt: R.quantile_fit_predict_path_batch_host(d["off"], d["y"], d["cols"], o["q"], d["taus"], d["tc"] if opt else None),
        lambda d, opt: [((d["G"], 3, d["p"] + 6), F), ((d["G"], 3), I), ((d["N"], 3), F)], ("cols", "tc")),
    "anofox_hip_quantile_fit_predict_window": (
        lambda R, d, o, opt: R.quantile_fit_predict_window_host(d["off"], d["y"], d["cols"], o["q"], (8, 1), opt),
        lambda d, opt: [((d["N"], 3), F)] + ([((d["N"], d["p"] + 6), F), ((d["N"],), I)] if opt else []), ("cols",)),
    "anofox_hip_quantile_fit_predict_frames": (
        lambda R, d, o, opt: R.quantile_fit_predict_frames_host(d["y"], d["cols"], d["lo"], d["hi"], o["q"], opt),
        lambda d, opt: [((d["N"], 3), F)] + ([((d["N"], d["p"] + 6), F), ((d["N"],), I)] if opt else []), ("cols", "lo", "hi")),
    "anofox_hip_glm_fit_batch": (
        lambda R, d, o, opt: R.glm_fit_batch_host(d["off"], d["y_pois"], d["cols"], o["glm"]("poisson", opt), d["offset"] if opt else None, opt),
        lambda d, opt: [((d["G"], d["p"] + 11), F)] + ([((d["G"], 5 * d["p"]), F)] if opt else []), ("cols", "offset")),
    "anofox_hip_glm_fit_batch/binomial": (
        lambda R, d, o, opt: R.glm_fit_batch_host(d["off"], d["y_bin"], d["cols"], o["glm"]("binomial")),
        lambda d, opt: [((d["G"], d["p"] + 11), F)], ()),
    "anofox_hip_glm_fit_predict_batch": (
        lambda R, d, o, opt: R.glm_fit_predict_batch_host(d["off"], d["y_pois"], d["cols"], o["glm"]("poisson"), d["offset"] if opt else None,
                                                          d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 11), F), ((d["N"], 3), F)], ("cols", "offset", "tc")),
    "anofox_hip_glm_fit_predict_interval_batch": (
        lambda R, d, o, opt: R.glm.glm_fit_predict_interval_batch_host(d["off"], d["y_pois"], d["cols"], o["glm"]("poisson"), 1.96,
                                                                       d["offset"] if opt else None, d["tc"] if opt else None),
        lambda d, opt: [((d["G"], d["p"] + 11), F), ((d["N"], 3), F)], ("cols", "offset", "tc")),
    "anofox_hip_glm_fit_accuracy_batch": (
        lambda R, d, o, opt: R.glm.glm_fit_accuracy_batch_host(d["off"], d["y_bin"], d["cols"], o["glm"]("binomial", opt), 0.5,
                                                               d["offset"] if opt else None, opt),
        lambda d, opt: [((d["G"], d["p"] + 11), F)] + ([((d["G"], 5 * d["p"]), F)] if opt else []) + [((d["G"],), F)], ("cols", "offset")),
}
CASES = [(name, p, opt) for name, (has_opt, _) in ENTRIES.items() for p in (1, 3) for opt in ((True, False) if has_opt else (True,))]
IDS = ["%s-p%d-%s" % (n.replace("anofox_hip_", ""), p, "opt" if o else "null") for n, p, o in CASES]


class Recorder:
    """Stands in for the loaded library: every declared symbol is a function that records its arguments and answers `ok`
    (with `code` and `text` in the AnofoxError when that is False)."""

    def __init__(self, abi, ok=True, code=0, text=b""):
        self.abi, self.ok, self.code, self.text, self.calls = abi, ok, code, text, []

    def __getattr__(self, name):
        if name not in self.abi.SYMBOLS:
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            if not self.ok:
                err = args[-1]._obj
                err.code, err.message = self.code, self.text
            return self.ok
        fn.argtypes = self.abi.SYMBOLS[name][1]
        return fn


@pytest.fixture(scope="module")
def env():
    pkg = import_pkg()
    import_pkg("glm")
    return dict(pkg=pkg, o=options(pkg), d={p: batch(p) for p in (1, 3)})


@pytest.fixture
def recorder(env, monkeypatch):
    rec = Recorder(env["pkg"]._abi)
    monkeypatch.setattr(env["pkg"]._abi, "_lib", rec)
    return rec


def addr(a):
    if a is None or isinstance(a, int):
        return a or 0
    return C.cast(a, C.c_void_p).value or 0


def flat(result):
    return list(result) if isinstance(result, (tuple, list)) else [result]


def expected_items(pkg, name, d, o, opt):
    """The inventory's arguments after ctx; the expanding function goes through the window entry with the expanding frame."""
    if name != "anofox_hip_fit_predict_expanding":
        return name.split("/")[0] + "_host", ENTRIES[name][1](d, o, opt)
    items = ENTRIES["anofox_hip_fit_predict_window"][1](d, o, opt)
    k = [isinstance(it, pkg._abi.AnofoxHipWindowFrame) for it in items].index(True)
    items[k] = pkg._abi.AnofoxHipWindowFrame(2 ** 63 - 1, 0)
    return "anofox_hip_fit_predict_window_host", items


@pytest.mark.parametrize("name,p,opt", CASES, ids=IDS)
def test_host_function_marshals_its_entry(env, recorder, name, p, opt):
    pkg, d, o = env["pkg"], env["d"][p], env["o"]
    symbol, items = expected_items(pkg, name, d, o, opt)
    result = flat(HOST[name][0](pkg, d, o, opt))
    assert len(recorder.calls) == 1
    got_name, args = recorder.calls[0]
    argtypes = pkg._abi.SYMBOLS[symbol][1]
    assert got_name == symbol
    assert len(args) == len(argtypes) == len(items) + 2
    for a, t in zip(args, argtypes):
        if isinstance(t, type) and issubclass(t, C.Structure):
            assert isinstance(a, t)
        else:
            t.from_param(a)   # raises if ctypes would not take it
    assert addr(args[0]) == 0   # no context: the thread's default one
    outs = {r.ctypes.data: r for r in result if r is not None}
    for k, (it, a) in enumerate(zip(items, args[1:-1]), start=1):
        what = "%s argument %d" % (symbol, k)
        if isinstance(it, In):
            assert addr(a) == (0 if it.a is None else it.a.ctypes.data), what
        elif isinstance(it, Cols):
            assert len(a) >= max(len(it.cols), 1), what
            assert [addr(a[j]) for j in range(len(it.cols))] == [c.ctypes.data for c in it.cols], what
        elif isinstance(it, Out):
            if it.n is None:   # an output the entry may go without: NULL, or one the function returns anyway
                assert addr(a) == 0 or addr(a) in outs, what
            else:
                assert addr(a) in outs and outs[addr(a)].size >= it.n and outs[addr(a)].dtype == it.dtype, what
        elif isinstance(it, C.Structure):
            assert bytes(a) == bytes(it), what
        elif isinstance(it, C._Pointer):
            assert addr(a) == addr(it), what
        else:
            assert type(a) is type(it) and a == it, what   # G, p, N, T, the flags, the levels
    want = HOST[name][1](d, opt)
    assert len(result) == len(want)
    for r, w in zip(result, want):
        assert (r is None) == (w is None)
        if r is not None:
            assert (r.shape, r.dtype) == (w[0], np.dtype(w[1])) and r.flags.c_contiguous


@pytest.mark.parametrize("name", list(HOST), ids=[n.replace("anofox_hip_", "") for n in HOST])
def test_failed_call_raises_the_librarys_error(env, monkeypatch, name):
    pkg = env["pkg"]
    rec = Recorder(pkg._abi, ok=False, code=7, text=b"no room on the device")
    monkeypatch.setattr(pkg._abi, "_lib", rec)
    with pytest.raises(pkg.AnofoxStatsError) as e:
        HOST[name][0](pkg, env["d"][1], env["o"], True)
    assert e.value.code == 7 and str(e.value) == "no room on the device"
    assert len(rec.calls) == 1


def test_inventory_is_complete():
    assert set(HOST) == set(ENTRIES)


SHORT = [(name, key) for name, (_, _, keys) in HOST.items() for key in keys]


@pytest.mark.parametrize("name,key", SHORT, ids=["%s-%s" % (n.replace("anofox_hip_", ""), k) for n, k in SHORT])
def test_short_input_is_refused(env, recorder, name, key):
    """New checks: a column, or a per-row / per-group optional array or frame bound, that is one element short raises ValueError
    before the library is called (it cannot know a numpy array's length: a short one is a read past the buffer)."""
    d = dict(env["d"][3])
    d[key] = d["cols"][:-1] + [d["cols"][-1][:-1]] if key == "cols" else d[key][:-1]
    with pytest.raises(ValueError):
        HOST[name][0](env["pkg"], d, env["o"], True)
    assert recorder.calls == []
