"""The Python wrappers of the batch entries, through the binding: every `*_host` function against its `Context.*_device` method bit
for bit (NaNs as bytes), the outputs a caller may supply, and the refusal of tensors a kernel must never see.
test_gpu_host_staging.py compares the same entries through raw ctypes and bypasses the wrappers on purpose; this file pins them.
The batch, the options and the inventory are that file's (64 rows, four groups, p = 1 and p = 3, the optional arrays once
present and once absent), the host calls are test_runtime_marshal_cpu.HOST; DEVICE below adds the device method of each entry.

Four host functions have no device method in the binding (fit_predict_frames, bls_fit_predict_batch,
quantile_fit_predict_batch, quantile_fit_predict_path_batch): test_gpu_host_staging.py alone covers their entries.

The refusals are new with the marshalling layer (_marshal.py) and are skipped on a tree without it.  While a bad call is tried
a Guard stands in the library's place: it refuses every batch entry, so a missing check fails the test and launches nothing."""
import os

import numpy as np
import pytest

from conftest import ROOT, import_pkg
from test_gpu_host_staging import ENTRIES, batch, options, same_bits
from test_runtime_marshal_cpu import HOST, _wls, flat

pytestmark = pytest.mark.gpu

HAS_MARSHAL = os.path.exists(os.path.join(ROOT, "anofox-statistics_amd", "_marshal.py"))
new_check = pytest.mark.skipif(not HAS_MARSHAL, reason="the binding has no marshalling layer: this check is new with it")

# name of the inventory -> (the device method on tensors t, {keyword of a caller-supplied output: (shape, dtype)})
DEVICE = {
    "anofox_hip_fit_batch": (
        lambda c, t, o, opt, **kw: c.fit_batch_device(t["off"], t["y"], t["cols"], t["w"] if opt else None, o["reg"](_wls(opt), opt), **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"), inference=lambda d: ((d["G"], 5 * d["p"] + 2), "float64"))),
    "anofox_hip_fit_batch/ridge": (
        lambda c, t, o, opt, **kw: c.fit_batch_device(t["off"], t["y"], t["cols"], None, o["reg"]("ridge"), **kw), {}),
    "anofox_hip_residuals_batch": (
        lambda c, t, o, opt, **kw: c.residuals_batch_device(t["off"], t["y"], t["y_hat"], t["cols"], t["rse"] if opt else None, True, False, **kw),
        dict(out=lambda d: ((d["N"], 4), "float64"), group=lambda d: ((d["G"], 2), "float64"))),
    "anofox_hip_vif_batch": (
        lambda c, t, o, opt, **kw: c.vif_batch_device(t["off"], t["cols"], **kw),
        dict(out=lambda d: ((d["G"], d["p"] + 1), "float64"))),
    "anofox_hip_fit_predict_batch": (
        lambda c, t, o, opt, **kw: c.fit_predict_batch_device(t["off"], t["y"], t["cols"], t["w"] if opt else None, o["reg"](_wls(opt)),
                                                              t["tc"] if opt else None, **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"), pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_fit_predict_expanding": (
        lambda c, t, o, opt, **kw: c.fit_predict_expanding_device(t["off"], t["y"], t["cols"], t["w"] if opt else None, o["reg"](_wls(opt)), **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_fit_predict_window": (
        lambda c, t, o, opt, **kw: c.fit_predict_window_device(t["off"], t["y"], t["cols"], t["w"] if opt else None, o["reg"](_wls(opt)),
                                                               (8, 1), **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_information_criteria_batch": (
        lambda c, t, o, opt, **kw: c.information_criteria_device(t["core"], o["reg"]("ols"), **kw),
        dict(out=lambda d: ((d["G"], 3), "float64"))),
    "anofox_hip_elasticnet_fit_batch": (
        lambda c, t, o, opt, **kw: c.elasticnet_fit_batch_device(t["off"], t["y"], t["cols"], o["en"], **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"), iterations=lambda d: ((d["G"],), "int32"))),
    "anofox_hip_elasticnet_fit_predict_batch": (
        lambda c, t, o, opt, **kw: c.elasticnet_fit_predict_batch_device(t["off"], t["y"], t["cols"], o["en"], 0.95, t["tc"] if opt else None, **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"), pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_elasticnet_fit_predict_window": (
        lambda c, t, o, opt, **kw: c.elasticnet_fit_predict_window_device(t["off"], t["y"], t["cols"], o["en"], (8, 1), 0.95, **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_elasticnet_fit_predict_frames": (
        lambda c, t, o, opt, **kw: c.elasticnet_fit_predict_frames_device(t["y"], t["cols"], t["lo"], t["hi"], o["en"], 0.95, **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_rls_fit_batch": (
        lambda c, t, o, opt, **kw: c.rls_fit_batch_device(t["off"], t["y"], t["cols"], o["rls"], **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"))),
    "anofox_hip_rls_fit_predict_batch": (
        lambda c, t, o, opt, **kw: c.rls_fit_predict_batch_device(t["off"], t["y"], t["cols"], o["rls"], 0.95, t["tc"] if opt else None, **kw),
        dict(core=lambda d: ((d["G"], d["p"] + 6), "float64"), pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_rls_fit_predict_window": (
        lambda c, t, o, opt, **kw: c.rls_fit_predict_window_device(t["off"], t["y"], t["cols"], o["rls"], (8, 1), 0.95, **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_rls_fit_predict_frames": (
        lambda c, t, o, opt, **kw: c.rls_fit_predict_frames_device(t["y"], t["cols"], t["lo"], t["hi"], o["rls"], 0.95, **kw),
        dict(pred=lambda d: ((d["N"], 3), "float64"))),
    "anofox_hip_bls_fit_batch": (
        lambda c, t, o, opt, **kw: c.bls_fit_batch_device(t["off"], t["y"], t["cols"], o["bls"], **kw),
        dict(records=lambda d: ((d["G"], 3 * d["p"] + 6), "float64"), iterations=lambda d: ((d["G"],), "int32"))),
    "anofox_hip_quantile_fit_batch": (
        lambda c, t, o, opt, **kw: c.quantile_fit_batch_device(t["off"], t["y"], t["cols"], o["q"], **kw),
        dict(records=lambda d: ((d["G"], d["p"] + 6), "float64"), iterations=lambda d: ((d["G"],), "int32"))),
    "anofox_hip_quantile_fit_path_batch": (
        lambda c, t, o, opt, **kw: c.quantile_fit_path_batch_device(t["off"], t["y"], t["cols"], o["q"], t["taus"], **kw),
        dict(records=lambda d: ((d["G"], 3, d["p"] + 6), "float64"), iterations=lambda d: ((d["G"], 3), "int32"))),
    "anofox_hip_quantile_fit_predict_window": (
        lambda c, t, o, opt, **kw: c.quantile_fit_predict_window_device(t["off"], t["y"], t["cols"], o["q"], (8, 1), opt, **kw), {}),
    "anofox_hip_quantile_fit_predict_frames": (
        lambda c, t, o, opt, **kw: c.quantile_fit_predict_frames_device(t["y"], t["cols"], t["lo"], t["hi"], o["q"], opt, **kw), {}),
    "anofox_hip_glm_fit_batch": (
        lambda c, t, o, opt, **kw: c.glm_fit_batch_device(t["off"], t["y_pois"], t["cols"], o["glm"]("poisson", opt),
                                                          t["offset"] if opt else None, opt, **kw), {}),
    "anofox_hip_glm_fit_batch/binomial": (
        lambda c, t, o, opt, **kw: c.glm_fit_batch_device(t["off"], t["y_bin"], t["cols"], o["glm"]("binomial"), **kw), {}),
    "anofox_hip_glm_fit_predict_batch": (
        lambda c, t, o, opt, **kw: c.glm_fit_predict_batch_device(t["off"], t["y_pois"], t["cols"], o["glm"]("poisson"),
                                                                  t["offset"] if opt else None, t["tc"] if opt else None, **kw), {}),
    "anofox_hip_glm_fit_predict_interval_batch": (
        lambda c, t, o, opt, **kw: c.glm_fit_predict_interval_batch_device(t["off"], t["y_pois"], t["cols"], o["glm"]("poisson"), 1.96,
                                                                           t["offset"] if opt else None, t["tc"] if opt else None, **kw), {}),
    "anofox_hip_glm_fit_accuracy_batch": (
        lambda c, t, o, opt, **kw: c.glm_fit_accuracy_batch_device(t["off"], t["y_bin"], t["cols"], o["glm"]("binomial", opt), 0.5,
                                                                   t["offset"] if opt else None, opt, **kw), {}),
}
HOST_ONLY = {"anofox_hip_fit_predict_frames", "anofox_hip_bls_fit_predict_batch", "anofox_hip_quantile_fit_predict_batch",
             "anofox_hip_quantile_fit_predict_path_batch"}
CASES = [(name, p, opt) for name in DEVICE for p in (1, 3) for opt in ((True, False) if ENTRIES[name][0] else (True,))]
WITH_OUTPUTS = [name for name, (_, outs) in DEVICE.items() if outs]
# the tensors of the batch a method takes that can be wrong: y (where there is one), the last column, and the keys of HOST
def _keys(name):
    if "information_criteria" in name:
        return ("core",)
    y = () if "vif" in name else ("y_bin",) if "accuracy" in name or "binomial" in name else ("y_pois",) if "glm" in name else ("y",)
    return y + ("cols",) + tuple(k for k in HOST[name][2] if k != "cols")


KEYS = {name: _keys(name) for name in DEVICE}
BAD = [(name, key, how) for name in DEVICE for key in KEYS[name] for how in ("cpu", "dtype", "strided", "short")
       if not (key == "core" and how == "short")]


def short(name):
    return name.replace("anofox_hip_", "")


class Guard:
    """In the library's place while a bad call is tried: the context's housekeeping goes through, every other entry is refused
    and noted, so that a call that reaches the library launches nothing and fails with AnofoxStatsError."""

    def __init__(self, lib):
        self.lib, self.reached = lib, []

    def __getattr__(self, name):
        if name.startswith("anofox_hip_context_") or name.startswith("anofox_hip_agg_state_slots"):
            return getattr(self.lib, name)

        def refuse(*args):
            self.reached.append(name)
            args[-1]._obj.code, args[-1]._obj.message = 99, b"the guard refused the call"
            return False
        return refuse


@pytest.fixture(scope="module")
def env():
    import torch
    pkg = import_pkg()
    ctx = pkg.Context(0)
    d = {p: batch(p) for p in (1, 3)}

    def tensors(b):
        t = {k: torch.from_numpy(v).to("cuda:0") for k, v in b.items() if isinstance(v, np.ndarray) and k != "taus"}
        t["cols"], t["taus"] = [torch.from_numpy(c).to("cuda:0") for c in b["cols"]], b["taus"]
        return t
    yield dict(pkg=pkg, ctx=ctx, torch=torch, o=options(pkg), d=d, t={p: tensors(b) for p, b in d.items()})
    ctx.close()


@pytest.fixture
def guard(env, monkeypatch):
    g = Guard(env["ctx"]._lib)
    monkeypatch.setattr(env["ctx"], "_lib", g)
    return g


def to_host(env, result):
    env["ctx"].synchronize()
    return [None if r is None else r.cpu().numpy() for r in flat(result)]


def test_inventory_is_complete():
    assert set(DEVICE) | HOST_ONLY == set(ENTRIES) and not set(DEVICE) & HOST_ONLY


@pytest.mark.parametrize("name,p,opt", CASES, ids=["%s-p%d-%s" % (short(n), p, "opt" if o else "null") for n, p, o in CASES])
def test_host_function_equals_device_method(env, name, p, opt):
    host = flat(HOST[name][0](env["pkg"], env["d"][p], env["o"], opt))
    device = to_host(env, DEVICE[name][0](env["ctx"], env["t"][p], env["o"], opt))
    assert len(host) == len(device) and len(host) > 0
    for k, (h, v) in enumerate(zip(host, device)):
        assert (h is None) == (v is None)
        if h is not None:
            assert h.shape == v.shape and h.dtype == v.dtype
            assert same_bits(h, v), "%s p=%d: output %d of the host function differs from the device method's" % (name, p, k)


def given_outputs(env, name, p, shrink=None, retype=None):
    torch = env["torch"]
    out = {}
    for kw, spec in DEVICE[name][1].items():
        shape, dtype = spec(env["d"][p])
        n = int(np.prod(shape)) - (1 if kw == shrink else 0)
        if kw == retype:
            dtype = "float32" if dtype == "float64" else "int64"
        out[kw] = torch.full((n,), -7, dtype=getattr(torch, dtype), device="cuda:0")
    return out


@pytest.mark.parametrize("name", WITH_OUTPUTS, ids=[short(n) for n in WITH_OUTPUTS])
def test_caller_supplied_outputs_are_written_and_returned(env, name):
    plain = to_host(env, DEVICE[name][0](env["ctx"], env["t"][3], env["o"], True))
    given = given_outputs(env, name, 3)
    result = flat(DEVICE[name][0](env["ctx"], env["t"][3], env["o"], True, **given))
    assert len(result) == len(given)
    for r, g in zip(result, given.values()):
        assert r is g
    for k, (a, b) in enumerate(zip(to_host(env, result), plain)):
        assert same_bits(a.ravel(), b.ravel()), "%s: output %d written into the caller's tensor differs" % (name, k)


@new_check
@pytest.mark.parametrize("name", WITH_OUTPUTS, ids=[short(n) for n in WITH_OUTPUTS])
def test_bad_caller_supplied_output_is_refused(env, guard, name):
    """New check: an output one element too small, or of the wrong dtype, raises ValueError before the library is reached."""
    for kw in DEVICE[name][1]:
        for bad in (dict(shrink=kw), dict(retype=kw)):
            with pytest.raises(ValueError):
                DEVICE[name][0](env["ctx"], env["t"][3], env["o"], True, **given_outputs(env, name, 3, **bad))
    assert guard.reached == []


def spoil(torch, x, how):
    if how == "cpu":
        return x.cpu()
    if how == "dtype":
        return x.to(torch.float32 if x.dtype == torch.float64 else torch.int32)
    if how == "strided":
        return torch.cat([x, x], dim=-1)[..., ::2]
    return x[:-1]


@new_check
@pytest.mark.parametrize("name,key,how", BAD, ids=["%s-%s-%s" % (short(n), k, h) for n, k, h in BAD])
def test_bad_input_tensor_is_refused(env, guard, name, key, how):
    """New checks: a CPU tensor, a tensor of the wrong dtype, a non-contiguous one (every second element of one twice as long)
    and one that is an element short each raise ValueError before the library is reached."""
    t = dict(env["t"][3])
    t[key] = t["cols"][:-1] + [spoil(env["torch"], t["cols"][-1], how)] if key == "cols" else spoil(env["torch"], t[key], how)
    with pytest.raises(ValueError):
        DEVICE[name][0](env["ctx"], t, env["o"], True)
    assert guard.reached == []


@new_check
def test_agg_state_device_calls_refuse_bad_tensors(env, monkeypatch):
    """New checks on AggState.update_device / finalize_device / finalize_elasticnet_device, which took any tensor as it came."""
    torch, pkg, d, t = env["torch"], env["pkg"], env["d"][3], env["t"][3]
    state = pkg.AggState(env["ctx"], 3, env["o"]["reg"]("ols"), retain_bytes=0)
    g = Guard(state._lib)
    monkeypatch.setattr(state, "_lib", g)
    n = d["N"]
    good = dict(slot=torch.zeros(n, dtype=torch.int32, device="cuda:0"), y=t["y"], x_rowmajor=torch.stack(t["cols"], dim=1).contiguous(),
                w=t["w"], valid=torch.ones(n, dtype=torch.uint8, device="cuda:0"))
    for key in good:
        for how in ("cpu", "dtype", "strided", "short"):
            if key in ("slot", "valid") and how == "dtype":
                continue   # (slot keeps taking any 32-bit integer tensor; valid has no second integer spelling to refuse here)
            bad = dict(good)
            bad[key] = spoil(torch, good[key].reshape(-1), how)
            with pytest.raises(ValueError):
                state.update_device(n_slots=1, **bad)
    core = torch.empty((1, 9), dtype=torch.float64, device="cuda:0")
    for bad in (core.cpu(), core.to(torch.float32), core.reshape(-1)[:-1], torch.empty((1, 18), dtype=torch.float64, device="cuda:0")[:, ::2]):
        with pytest.raises(ValueError):
            state.finalize_device(bad, n_slots=1)
        with pytest.raises(ValueError):
            state.finalize_elasticnet_device(env["o"]["en"], bad, n_slots=1)
    with pytest.raises(ValueError):
        state.finalize_elasticnet_device(env["o"]["en"], core, torch.empty(1, dtype=torch.int64, device="cuda:0"), n_slots=1)
    assert g.reached == []
    monkeypatch.undo()
    state.close()
