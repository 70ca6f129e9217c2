"""The staging of the host-pointer entry points (csrc/host_stage.h): every `*_host` entry that the ctypes bindings reach, on one
small batch, against its `*_device` entry on the same data, BIT FOR BIT (NaNs included).  The table ENTRIES is the inventory of
the host entries; an entry that is added to the library belongs in it.

The batch is the smallest at which the staging can go wrong: group sizes [0, 1, 32, 31] — an empty group first, a one-row group,
and 64 rows in all, so that every column is exactly 512 bytes and a lost pad would make two columns adjacent — at p = 1 and
p = 3, every optional array (w, train_counts, offset, iterations, inference, the GLM accuracy) once present and once NULL, and
one n_groups = 0 call per entry, which returns true and touches nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import import_pkg

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 32, 31]
F64_FILL, INT_FILL = -777.25, -7  # what an output holds before the call


class In:
    """an input array (None: a NULL pointer on both sides)"""
    def __init__(self, a):
        self.a = None if a is None else np.ascontiguousarray(a)


class Cols:
    """the table of column pointers"""
    def __init__(self, cols):
        self.cols = [np.ascontiguousarray(c) for c in cols]


class Out:
    """an output of n elements (n None: a NULL pointer on both sides)"""
    def __init__(self, n, dtype=np.float64):
        self.n, self.dtype = n, dtype


def batch(p):
    """The data of every entry at width p, from one seed."""
    rng = np.random.default_rng(1000 + p)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    G, N = len(SIZES), int(off[-1])
    X = rng.normal(size=(N, p))
    eta = X @ rng.uniform(0.2, 0.6, size=p) + 0.3
    lo, hi = np.empty(N, np.int64), np.empty(N, np.int64)
    for g in range(G):
        for r in range(off[g], off[g + 1]):  # ROWS BETWEEN 8 PRECEDING AND 1 PRECEDING within the group
            lo[r], hi[r] = max(off[g], r - 8), r
    return dict(G=G, N=N, p=p, off=off, cols=[X[:, j].copy() for j in range(p)], y=eta + 0.3 * rng.normal(size=N),
                w=rng.uniform(0.5, 2.0, size=N), tc=np.array([0, 1, 20, 25], np.int64), offset=0.1 * rng.normal(size=N),
                y_pois=rng.poisson(np.exp(eta)).astype(np.float64), y_bin=(rng.random(N) < 1 / (1 + np.exp(-eta))).astype(np.float64),
                y_hat=eta, rse=rng.uniform(0.2, 0.4, size=G), lo=lo, hi=hi, taus=np.array([0.25, 0.5, 0.9]),
                core=np.abs(rng.normal(size=(G, p + 6))) + 1.0)


def options(pkg):
    A = pkg._abi
    return dict(
        reg=lambda model, inf=False: A.AnofoxHipBatchOptions(A.MODEL[model], True, inf, 0.95, 0.0, 0, 0, 0),
        en=A.AnofoxHipElasticNetBatchOptions(True, 0.1, 0.5, 1000, 1e-8, 0),
        rls=A.AnofoxHipRlsBatchOptions(True, 0.99, 100.0),
        bls=A.AnofoxHipBlsBatchOptions(True, None, 0, None, 0, 1000, 1e-10),
        q=A.AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-8),
        glm=lambda family, inf=False: A.AnofoxHipGlmBatchOptions(A.GLM_FAMILY[family], True, 25, 1e-8, 0.0, inf, 0.95),
        frame=A.AnofoxHipWindowFrame(8, 1))


# ---- the inventory: name without _host / _device -> (has optional arrays, arguments after ctx) --------------------------------
# `d` is batch(p), `o` is options(pkg), `opt` says whether the entry's optional arrays are present.  An entry whose first count
# is the number of rows (the explicit-frames entries) lists "rows" as its leading argument.

def _wls(opt):
    return "wls" if opt else "ols"


def _head(d, y="y"):
    return [d["G"], d["p"], d["N"], In(d["off"]), In(d[y]), Cols(d["cols"])]


def _frames_head(d):
    return [d["N"], d["p"], In(d["y"]), Cols(d["cols"])]


ENTRIES = {
    "anofox_hip_fit_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["w"] if opt else None), o["reg"](_wls(opt), opt), Out(d["G"] * (d["p"] + 6)), Out(d["G"] * (5 * d["p"] + 2) if opt else None)]),
    "anofox_hip_fit_batch/ridge": (False, lambda d, o, opt: _head(d) + [
        In(None), o["reg"]("ridge"), Out(d["G"] * (d["p"] + 6)), Out(None)]),
    "anofox_hip_residuals_batch": (True, lambda d, o, opt: [
        d["G"], d["p"], d["N"], In(d["off"]), In(d["y"]), In(d["y_hat"]), Cols(d["cols"]), In(d["rse"] if opt else None), True, False,
        Out(d["N"] * 4), Out(d["G"] * 2)]),
    "anofox_hip_vif_batch": (False, lambda d, o, opt: [
        d["G"], d["p"], d["N"], In(d["off"]), Cols(d["cols"]), Out(d["G"] * (d["p"] + 1))]),
    "anofox_hip_fit_predict_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["w"] if opt else None), In(d["tc"] if opt else None), o["reg"](_wls(opt)), Out(d["G"] * (d["p"] + 6)), Out(3 * d["N"])]),
    "anofox_hip_fit_predict_expanding": (True, lambda d, o, opt: _head(d) + [
        In(d["w"] if opt else None), o["reg"](_wls(opt)), Out(3 * d["N"])]),
    "anofox_hip_fit_predict_window": (True, lambda d, o, opt: _head(d) + [
        In(d["w"] if opt else None), o["frame"], o["reg"](_wls(opt)), Out(3 * d["N"])]),
    "anofox_hip_fit_predict_frames": (True, lambda d, o, opt: _frames_head(d) + [
        In(d["w"] if opt else None), In(d["lo"]), In(d["hi"]), o["reg"](_wls(opt)), Out(3 * d["N"])]),
    "anofox_hip_information_criteria_batch": (False, lambda d, o, opt: [
        d["G"], d["p"], In(d["core"]), o["reg"]("ols"), Out(3 * d["G"])]),
    "anofox_hip_elasticnet_fit_batch": (True, lambda d, o, opt: _head(d) + [
        o["en"], Out(d["G"] * (d["p"] + 6)), Out(d["G"] if opt else None, np.int32)]),
    "anofox_hip_elasticnet_fit_predict_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["tc"] if opt else None), o["en"], 0.95, Out(d["G"] * (d["p"] + 6)), Out(3 * d["N"])]),
    "anofox_hip_elasticnet_fit_predict_window": (False, lambda d, o, opt: _head(d) + [o["frame"], o["en"], 0.95, Out(3 * d["N"])]),
    "anofox_hip_elasticnet_fit_predict_frames": (False, lambda d, o, opt: _frames_head(d) + [
        In(d["lo"]), In(d["hi"]), o["en"], 0.95, Out(3 * d["N"])]),
    "anofox_hip_rls_fit_batch": (False, lambda d, o, opt: _head(d) + [o["rls"], Out(d["G"] * (d["p"] + 6))]),
    "anofox_hip_rls_fit_predict_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["tc"] if opt else None), o["rls"], 0.95, Out(d["G"] * (d["p"] + 6)), Out(3 * d["N"])]),
    "anofox_hip_rls_fit_predict_window": (False, lambda d, o, opt: _head(d) + [o["frame"], o["rls"], 0.95, Out(3 * d["N"])]),
    "anofox_hip_rls_fit_predict_frames": (False, lambda d, o, opt: _frames_head(d) + [
        In(d["lo"]), In(d["hi"]), o["rls"], 0.95, Out(3 * d["N"])]),
    "anofox_hip_bls_fit_batch": (True, lambda d, o, opt: _head(d) + [
        o["bls"], Out(d["G"] * (3 * d["p"] + 6)), Out(d["G"] if opt else None, np.int32)]),
    "anofox_hip_bls_fit_predict_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["tc"] if opt else None), o["bls"], 0.95, Out(d["G"] * (d["p"] + 6)), Out(3 * d["N"])]),
    "anofox_hip_quantile_fit_batch": (True, lambda d, o, opt: _head(d) + [
        o["q"], Out(d["G"] * (d["p"] + 6)), Out(d["G"] if opt else None, np.int32)]),
    "anofox_hip_quantile_fit_predict_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["tc"] if opt else None), o["q"], Out(d["G"] * (d["p"] + 6)), Out(3 * d["N"])]),
    "anofox_hip_quantile_fit_path_batch": (True, lambda d, o, opt: _head(d) + [
        o["q"], d["taus"].ctypes.data_as(C.POINTER(C.c_double)), len(d["taus"]), Out(d["G"] * len(d["taus"]) * (d["p"] + 6)),
        Out(d["G"] * len(d["taus"]) if opt else None, np.int32)]),
    "anofox_hip_quantile_fit_predict_path_batch": (True, lambda d, o, opt: _head(d) + [
        In(d["tc"] if opt else None), o["q"], d["taus"].ctypes.data_as(C.POINTER(C.c_double)), len(d["taus"]),
        Out(d["G"] * len(d["taus"]) * (d["p"] + 6)), Out(d["G"] * len(d["taus"]) if opt else None, np.int32), Out(d["N"] * len(d["taus"]))]),
    "anofox_hip_quantile_fit_predict_window": (True, lambda d, o, opt: _head(d) + [
        o["frame"], o["q"], Out(3 * d["N"]), Out(d["N"] * (d["p"] + 6) if opt else None), Out(d["N"] if opt else None, np.int32)]),
    "anofox_hip_quantile_fit_predict_frames": (True, lambda d, o, opt: _frames_head(d) + [
        In(d["lo"]), In(d["hi"]), o["q"], Out(3 * d["N"]), Out(d["N"] * (d["p"] + 6) if opt else None),
        Out(d["N"] if opt else None, np.int32)]),
    "anofox_hip_glm_fit_batch": (True, lambda d, o, opt: _head(d, "y_pois") + [
        In(d["offset"] if opt else None), o["glm"]("poisson", opt), Out(d["G"] * (d["p"] + 11)), Out(d["G"] * 5 * d["p"] if opt else None)]),
    "anofox_hip_glm_fit_batch/binomial": (False, lambda d, o, opt: _head(d, "y_bin") + [
        In(None), o["glm"]("binomial"), Out(d["G"] * (d["p"] + 11)), Out(None)]),
    "anofox_hip_glm_fit_predict_batch": (True, lambda d, o, opt: _head(d, "y_pois") + [
        In(d["offset"] if opt else None), In(d["tc"] if opt else None), o["glm"]("poisson"), Out(d["G"] * (d["p"] + 11)), Out(3 * d["N"])]),
    "anofox_hip_glm_fit_predict_interval_batch": (True, lambda d, o, opt: _head(d, "y_pois") + [
        In(d["offset"] if opt else None), In(d["tc"] if opt else None), o["glm"]("poisson"), 1.96, Out(d["G"] * (d["p"] + 11)),
        Out(3 * d["N"])]),
    # (the accuracy array is what this entry is for and may not be NULL; the fit entries above are the same staging without it)
    "anofox_hip_glm_fit_accuracy_batch": (True, lambda d, o, opt: _head(d, "y_bin") + [
        In(d["offset"] if opt else None), o["glm"]("binomial", opt), 0.5, Out(d["G"] * (d["p"] + 11)),
        Out(d["G"] * 5 * d["p"] if opt else None), Out(d["G"])]),
}
CASES = [(name, p, opt) for name, (has_opt, _) in ENTRIES.items() for p in (1, 3) for opt in ((True, False) if has_opt else (True,))]


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = import_pkg()
    ctx = pkg.Context(0)
    yield dict(pkg=pkg, lib=pkg._abi.load(), ctx=ctx, torch=torch, o=options(pkg), d={p: batch(p) for p in (1, 3)})
    ctx.close()


def run(env, name, items, device, counts=None):
    """One call of the entry's host or device form; returns its outputs as host arrays (None for a NULL one)."""
    torch, lib = env["torch"], env["lib"]
    fn = getattr(lib, name.split("/")[0] + ("_device" if device else "_host"))
    err = env["pkg"]._abi.AnofoxError()
    args, outs, keep = [env["ctx"]._h], [], []

    def dev(a):
        t = torch.from_numpy(a).to("cuda:0")
        keep.append(t)
        return t

    for i, it in enumerate(items, start=1):
        if counts is not None and isinstance(it, int) and i in (1, 3):
            it = counts  # the n_groups = 0 call: no groups (or frames) and no rows, the width and every pointer as before
        if isinstance(it, (In, Out)):
            a = it.a if isinstance(it, In) else None if it.n is None else np.full(it.n, F64_FILL if it.dtype == np.float64 else INT_FILL, it.dtype)
            if isinstance(it, Out):
                outs.append(a if a is None or not device else dev(a))
            if a is None:
                args.append(None)
            elif device:
                args.append(C.c_void_p((outs[-1] if isinstance(it, Out) else dev(a)).data_ptr()))
            else:
                args.append(a.ctypes.data_as(fn.argtypes[i]))
        elif isinstance(it, Cols):
            if device:
                args.append((C.c_void_p * len(it.cols))(*[dev(c).data_ptr() for c in it.cols]))
            else:
                args.append((C.POINTER(C.c_double) * len(it.cols))(*[c.ctypes.data_as(C.POINTER(C.c_double)) for c in it.cols]))
        else:
            args.append(it)
    ok = fn(*args, C.byref(err))
    assert ok, "%s: %s" % (fn.__name__, err.text())
    if device:
        assert lib.anofox_hip_context_synchronize(env["ctx"]._h, C.byref(err)), err.text()
    return [None if a is None else a.cpu().numpy() if device else a for a in outs]


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    if a.dtype == np.float64:
        a, b = a.view(np.uint64), b.view(np.uint64)
    return np.array_equal(a, b)


@pytest.mark.parametrize("name,p,opt", CASES, ids=["%s-p%d-%s" % (n.replace("anofox_hip_", ""), p, "opt" if o else "null") for n, p, o in CASES])
def test_host_equals_device(env, name, p, opt):
    items = ENTRIES[name][1](env["d"][p], env["o"], opt)
    host, device = run(env, name, items, False), run(env, name, items, True)
    assert len(host) == len(device) and len(host) > 0
    for k, (h, v) in enumerate(zip(host, device)):
        if h is not None and h.dtype == np.float64:
            print("%s p=%d output %d: %d of %d doubles differ" % (name, p, k, int(np.sum(h.view(np.uint64) != v.view(np.uint64))), h.size))
        assert same_bits(h, v), "%s p=%d: output %d of the host entry differs from the device entry's" % (name, p, k)
    assert any(h is not None and np.any(h != (F64_FILL if h.dtype == np.float64 else INT_FILL)) for h in host), "the call wrote nothing"


@pytest.mark.parametrize("name", list(ENTRIES), ids=[n.replace("anofox_hip_", "") for n in ENTRIES])
def test_no_groups_touches_nothing(env, name):
    items = ENTRIES[name][1](env["d"][3], env["o"], True)
    outs = [a for a in run(env, name, items, False, counts=0) if a is not None]
    assert outs
    for a in outs:
        assert np.all(a == (F64_FILL if a.dtype == np.float64 else INT_FILL))
