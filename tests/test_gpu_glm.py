"""GPU tier of the GLM family: the cases of tests/glm_cases.py through anofox_hip_glm_fit_batch_{host,device}, fit-predict and
the scalar symbols, against tests/glm_restate.py; repeatability of the bytes across calls and across the two entry points."""
import numpy as np
import pytest

import glm_cases as GC
from conftest import import_pkg

pytestmark = pytest.mark.gpu
CALLS = GC.calls()
IDS = ["%s-p%d-%s-lam%g-%s" % ("poisson" if c[0] == GC.POISSON else "binomial", c[1], "icpt" if c[2] else "noicpt", c[3],
                               "off" if c[4] else "nooff") for c in CALLS]


@pytest.fixture(scope="module")
def glm():
    return import_pkg("glm")


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


def options(call, tolerance, inference=True, max_iterations=100):
    abi = import_pkg("_abi")
    return abi.AnofoxHipGlmBatchOptions(call["family"], call["icpt"], max_iterations, tolerance, call["lam"], inference, 0.95)


def columns(call):
    return [np.ascontiguousarray(call["x"][:, j]) for j in range(call["p"])]


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_fit_host_and_device(glm, ctx, c):
    """tolerance = 1e-12 through the host entry (values to the bounds), the device entry gives the same bytes; then the
    default tolerance: converged and within 2e-8 (0.1 + objective) of the optimum."""
    import torch
    call = GC.make_call(*c)
    refs, p, errs = GC.reference(call), call["p"], {}
    rec, inf = glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), options(call, 1e-12), offset=call["off"], inference=True,
                                      ctx=ctx)
    compared = 0
    for g, ref in enumerate(refs):
        compared += GC.check_record(rec[g], inf[g], ref, p, True, errs, None, "group %d (%s)" % (g, call["kinds"][g]), call["kinds"][g],
                                    call["lam"])
    print(IDS[CALLS.index(c)], "compared", compared, {k: "%.2e" % v for k, v in errs.items()})
    assert compared >= 50
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    drec, dinf = ctx.glm_fit_batch_device(t(call["offsets"], torch.int64), t(call["y"]), [t(col) for col in columns(call)],
                                          options(call, 1e-12), offset=None if call["off"] is None else t(call["off"]), inference=True)
    torch.cuda.synchronize()
    assert drec.cpu().numpy().tobytes() == rec.tobytes() and dinf.cpu().numpy().tobytes() == inf.tobytes()
    rec8 = glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), options(call, 1e-8, False), offset=call["off"], ctx=ctx)
    errs8 = {}
    for g, ref in enumerate(refs):
        GC.check_record(rec8[g], None, ref, p, False, errs8, None, "group %d (%s)" % (g, call["kinds"][g]), call["kinds"][g], call["lam"])
    print(IDS[CALLS.index(c)], "default tolerance", {k: "%.2e" % v for k, v in errs8.items()})


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_fit_predict(glm, ctx, c):
    """Every call through fit-predict: the host entry against the restatement, the device entry with the same bytes, and
    train_counts through both."""
    import torch
    call = GC.make_call(*c)
    refs, p, o = GC.reference(call), call["p"], call["offsets"]
    core, pred = glm.glm_fit_predict_batch_host(o, call["y"], columns(call), options(call, 1e-12, False), offset=call["off"], ctx=ctx)
    assert np.all(np.isnan(pred[:, 1:]))
    compared = 0
    for g, ref in enumerate(refs):
        n = o[g + 1] - o[g]
        if n < 2:
            assert core[g, p + 10] == 100 and np.all(np.isnan(core[g, :p + 10])) and np.all(np.isnan(pred[o[g]:o[g + 1]]))
            continue
        compared += GC.check_record(core[g], None, ref, p, True, None, pred[o[g]:o[g + 1], 0], "group %d" % g, call["kinds"][g], call["lam"])
    assert compared >= 50
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    d_off, d_y, d_x = t(o, torch.int64), t(call["y"]), [t(col) for col in columns(call)]
    d_o = None if call["off"] is None else t(call["off"])
    dcore, dpred = ctx.glm_fit_predict_batch_device(d_off, d_y, d_x, options(call, 1e-12, False), offset=d_o)
    torch.cuda.synchronize()
    assert dcore.cpu().numpy().tobytes() == core.tobytes() and dpred.cpu().numpy().tobytes() == pred.tobytes()
    # train_counts: a group whose count says "fewer than 2 training rows" is NULL whatever its rows hold
    tc = np.diff(o).astype(np.int64)
    tc[20] = 1
    core2, pred2 = glm.glm_fit_predict_batch_host(o, call["y"], columns(call), options(call, 1e-12, False), offset=call["off"],
                                                  train_counts=tc, ctx=ctx)
    assert core2[20, p + 10] == 100 and np.all(np.isnan(pred2[o[20]:o[21]]))
    keep = np.arange(len(tc)) != 20
    assert core2[keep].tobytes() == core[keep].tobytes()
    dcore2, dpred2 = ctx.glm_fit_predict_batch_device(d_off, d_y, d_x, options(call, 1e-12, False), offset=d_o, train_counts=t(tc, torch.int64))
    torch.cuda.synchronize()
    assert dcore2.cpu().numpy().tobytes() == core2.tobytes() and dpred2.cpu().numpy().tobytes() == pred2.tobytes()


def test_same_bytes_with_another_family_between(glm, ctx):
    a, b = GC.make_call(*CALLS[10]), GC.make_call(*CALLS[14])
    run = lambda call: glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), options(call, 1e-8), offset=call["off"],
                                              inference=True, ctx=ctx)
    first = run(a)
    other = run(b)
    qopt = import_pkg("_abi").AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-6)
    import_pkg("runtime").quantile_fit_batch_host(b["offsets"], b["y"], columns(b), qopt, ctx=ctx)
    second = run(a)
    assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
    assert other[0].shape == (GC.N_GROUPS, b["p"] + 11)


def test_invalid_options_and_no_convergence(glm, ctx):
    call = GC.make_call(GC.POISSON, 2, True, 0.0, False, 77)
    for bad in (options(call, float("nan")), options(call, 1e-8, max_iterations=0)):
        rec, inf = glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), bad, inference=True, ctx=ctx)
        assert np.all(rec[:, -1] == 1) and np.all(np.isnan(rec[:, :-1])) and np.all(np.isnan(inf))
    call["family"] = 7
    rec = glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), options(call, 1e-8, False), ctx=ctx)
    assert np.all(rec[:, -1] == 1)
    call = GC.make_call(GC.BINOMIAL, 2, True, 0.0, False, 78)
    rec = glm.glm_fit_batch_host(call["offsets"], call["y"], columns(call), options(call, 1e-12, False, max_iterations=1), ctx=ctx)
    assert np.any(rec[:, -1] == 3) and np.all(np.isnan(rec[rec[:, -1] == 3, :-1]))


def test_scalar_symbols_and_aggregates(glm):
    """Three cases through the reference-compatible scalar symbols, and the aggregates over the same rows."""
    rng = np.random.default_rng(9)
    n = 80
    x = rng.uniform(-1, 1, (n, 3))
    expo = 1.0 + rng.integers(0, 3, n)
    y = rng.poisson(expo * np.exp(0.3 + x[:, :2] @ [0.5, -0.4])).astype(float)
    y[5] = np.nan
    # 1: Poisson with an offset column (x column 3 of the call = log exposure), inference on
    cols = [list(x[:, 0]), list(x[:, 1]), list(np.log(expo))]
    ylist = [None if np.isnan(v) else v for v in y]
    got = glm.poisson_fit(ylist, cols, {"offset": 3, "compute_inference": True, "tolerance": 1e-12})
    ref = GC.R.fit(GC.POISSON, y, x[:, :2], np.log(expo), True, 0.0)
    assert np.allclose(got["coefficients"], ref["coef"], rtol=0, atol=1e-9) and abs(got["intercept"] - ref["intercept"]) <= 1e-9
    assert GC.rel(got["deviance"], ref["deviance"]) <= 1e-9 and GC.rel(got["aic"], ref["aic"]) <= 1e-9
    assert got["n_observations"] == n - 1 and got["converged"] and got["n_features"] == 2
    assert np.allclose(got["std_errors"], ref["se"], rtol=1e-6, atol=0)
    # 2: logistic with a ridge penalty, accuracy at the threshold
    yb = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.2 + x @ [1.0, -1.0, 0.5])))).astype(float)
    got = glm.logistic_fit(list(yb), [list(x[:, j]) for j in range(3)], {"lambda": 0.5, "tolerance": 1e-12, "threshold": 0.4})
    ref = GC.R.fit(GC.BINOMIAL, yb, x, None, True, 0.5)
    assert np.allclose(got["coefficients"], ref["coef"], rtol=0, atol=1e-9)
    assert got["threshold"] == 0.4 and got["accuracy"] == np.mean((ref["mu_all"] >= 0.4) == (yb == 1))
    assert got["dispersion"] == 1.0
    # 3: a failing case: a negative count
    ybad = y.copy()
    ybad[0] = -2.0
    with pytest.raises(import_pkg("options").InvalidInputException, match="outside the support"):
        glm.poisson_fit([None if np.isnan(v) else v for v in ybad], cols, {"offset": 3})
    # the aggregates: two groups, the second without valid rows -> None
    keys = np.array([0] * n + [1] * 3)
    ya = np.concatenate([y, [np.nan] * 3])
    xa = np.vstack([np.column_stack([x[:, :2], np.log(expo)]), np.zeros((3, 3))])
    res = glm.poisson_fit_agg(keys, ya, xa, {"offset": 3, "tolerance": 1e-12})
    ref = GC.R.fit(GC.POISSON, y, x[:, :2], np.log(expo), True, 0.0)
    assert res.row(1) is None and np.allclose(res.row(0)["coefficients"], ref["coef"], rtol=0, atol=1e-9)
    fp = glm.poisson_fit_predict_agg(keys, ya, xa, {"offset": 3, "tolerance": 1e-12})
    assert np.allclose(fp.pred[:n, 0], ref["mu_all"], rtol=1e-9, atol=0) and np.all(np.isnan(fp.pred[n:]))
    lg = glm.logistic_fit_agg(np.zeros(n), yb, x, {"lambda": 0.5, "tolerance": 1e-12})
    bn = glm.binomial_fit_agg(np.zeros(n), yb, x, {"lambda": 0.5, "tolerance": 1e-12})
    assert lg.records.tobytes() == bn.records.tobytes()
