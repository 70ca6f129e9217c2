"""GPU tier of the GLM extras: the cases of tests/glm_extras_cases.py through anofox_hip_glm_fit_predict_interval_batch_{host,
device} and anofox_hip_glm_fit_accuracy_batch_{host,device}, against the host build of csrc/glm_irls.h
(tests/tools/glm_extras_host.cpp), against tests/glm_restate.py, and against the existing entry points' bytes.

Between the two builds of the header the sums run in the same order but exp / log are different libraries, so they agree as each
agrees with the restatement: coefficients and mu to 1e-9, the bounds to 1e-9 + 2 h (1e-9 + 0.5e-6) (glm_extras_cases), the
accuracy exactly (no compared row lies within 1e-6 of the threshold)."""
import os
import subprocess

import numpy as np
import pytest

import glm_cases as GC
import glm_extras_cases as XC
from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu
CALLS = XC.calls()
POISSON_CALLS = [c for c in CALLS if c[0] == XC.POISSON]
BINOMIAL_CALLS = [c for c in CALLS if c[0] == XC.BINOMIAL]


@pytest.fixture(scope="module")
def glm():
    return import_pkg("glm")


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_build(tmp_path_factory):
    """The host build of the header as a program of its own (no sanitizer here: that run is the CPU tier's)."""
    exe = str(tmp_path_factory.mktemp("glm_extras") / "glm_extras_host")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "tools", "glm_extras_host.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(call, predict, z, accuracy):
        out = subprocess.run([exe], input=XC.host_input(call, 1e-12, predict, z, XC.THRESHOLD, accuracy), capture_output=True)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        return [np.array([float(t) for t in ln.split()]) for ln in out.stdout.decode().strip().split("\n")]
    return run


def options(call, tolerance=1e-12):
    return import_pkg("_abi").AnofoxHipGlmBatchOptions(call["family"], call["icpt"], 100, tolerance, call["lam"], False, 0.95)


def columns(call):
    return [np.ascontiguousarray(call["x"][:, j]) for j in range(call["p"])]


def to_device(call):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    return t(call["offsets"], torch.int64), t(call["y"]), [t(col) for col in columns(call)], None if call["off"] is None else t(call["off"])


def close_records(rec, href, ref, p, label):
    """A group's record against the host build's, to the tolerances tests/test_gpu_glm.py holds between the two builds (its
    check_record at the tight tier): inside glm_cases.in_conditions status 0 on both sides, the NaN pattern of the coefficients
    equal, coefficients and intercept within 1e-9 max(1, max|b|), dispersion within 1e-6 relative, n_observations and n_params
    exact.  Outside the conditions a fit has no well-defined value (glm_cases' docstring): as there, a row rule's status is
    exact and a status of the fit is in {0, 3} on both sides, and nothing else is compared."""
    if GC.in_conditions(ref, p):
        assert rec[p + 10] == href[p + 10] == 0, label
    else:
        assert (rec[p + 10] in (0, 3) and href[p + 10] in (0, 3)) or rec[p + 10] == href[p + 10], label
        return False
    b, hb = rec[:p + 1], href[:p + 1]
    assert np.array_equal(np.isnan(b), np.isnan(hb)), label
    m = ~np.isnan(hb)
    assert np.max(np.abs(b[m] - hb[m])) <= 1e-9 * max(1.0, float(np.max(np.abs(hb[m])))), label
    assert GC.rel(rec[p + 5], href[p + 5]) <= 1e-6 and rec[p + 6] == href[p + 6] and rec[p + 7] == href[p + 7], label
    return True


@pytest.mark.parametrize("c", POISSON_CALLS, ids=[XC.ident(c) for c in POISSON_CALLS])
def test_interval(glm, ctx, host_build, c):
    call = XC.make_call(*c)
    refs, o, p, errs = GC.reference(call), call["offsets"], call["p"], {}
    args = (o, call["y"], columns(call), options(call))
    core0, pred0 = glm.glm_fit_predict_batch_host(*args, offset=call["off"], ctx=ctx)
    assert np.all(np.isnan(pred0[:, 1:]))
    corez, predz = glm.glm_fit_predict_interval_batch_host(*args, 0.0, offset=call["off"], ctx=ctx)
    assert corez.tobytes() == core0.tobytes() and predz.tobytes() == pred0.tobytes()       # interval_z = 0: the plain entry's bytes
    core, pred = glm.glm_fit_predict_interval_batch_host(*args, XC.Z, offset=call["off"], ctx=ctx)
    assert core.tobytes() == core0.tobytes() and pred[:, 0].tobytes() == pred0[:, 0].tobytes()
    core2, pred2 = glm.glm_fit_predict_interval_batch_host(*args, XC.Z, offset=call["off"], ctx=ctx)
    assert core2.tobytes() == core.tobytes() and pred2.tobytes() == pred.tobytes()           # two calls, the same bytes
    host = host_build(call, True, XC.Z, False)
    compared = fitted = 0
    for g, ref in enumerate(refs):
        s, n = slice(o[g], o[g + 1]), int(o[g + 1] - o[g])
        label = "group %d" % g
        if n < 2:
            assert core[g, p + 10] == 100 and np.all(np.isnan(core[g, :p + 10])) and np.all(np.isnan(pred[s])), label
            continue
        GC.check_record(core[g], None, ref, p, True, None, pred[s, 0], label)
        if core[g, p + 10] != 0:
            assert np.all(np.isnan(pred[s])), label
            continue
        fitted += 1
        compared += XC.check_interval(core[g], pred[s], ref, p, XC.Z, label, errs)
        hrec, hpred = host[g][:p + 11], host[g][p + 12:].reshape(n, 3)
        if close_records(core[g], hrec, ref, p, label):
            fin = np.isfinite(hpred[:, 0])
            assert np.array_equal(np.isfinite(pred[s, 0]), fin), label
            assert np.allclose(pred[s, 0][fin], hpred[fin, 0], rtol=1e-9, atol=0), label
            _, _, h = XC.formula(hpred[fin, 0], hrec[p + 5], XC.Z)
            m = h <= 10.0
            for col in (1, 2):
                d = np.abs(pred[s, col][fin][m] - hpred[fin, col][m]) / np.abs(hpred[fin, col][m])
                assert np.all(d <= 1e-9 + 2.0 * h[m] * (1e-9 + 0.5e-6)), (label, col)
        if call["kinds"][g] == "nanrow":
            assert np.all(np.isnan(pred[s][3])) and np.all(np.isfinite(pred[s][5])), label
    print(XC.ident(c), "fitted", fitted, "compared", compared, {k: "%.2e of the bound" % v for k, v in errs.items()})
    assert compared >= 3 and fitted >= 5


@pytest.mark.parametrize("c", BINOMIAL_CALLS, ids=[XC.ident(c) for c in BINOMIAL_CALLS])
def test_accuracy(glm, ctx, host_build, c):
    call = XC.make_call(*c)
    refs, o, p = GC.reference(call), call["offsets"], call["p"]
    assert XC.band_rows(call, refs) == 0
    args = (o, call["y"], columns(call), options(call))
    rec0 = glm.glm_fit_batch_host(*args, offset=call["off"], ctx=ctx)
    rec, acc = glm.glm_fit_accuracy_batch_host(*args, XC.THRESHOLD, offset=call["off"], ctx=ctx)
    assert rec.tobytes() == rec0.tobytes()                                                    # the fit is the plain entry's
    rec2, acc2 = glm.glm_fit_accuracy_batch_host(*args, XC.THRESHOLD, offset=call["off"], ctx=ctx)
    assert rec2.tobytes() == rec.tobytes() and acc2.tobytes() == acc.tobytes()
    _, pred = glm.glm_fit_predict_batch_host(*args, offset=call["off"], ctx=ctx)
    host = host_build(call, False, 0.0, True)
    compared = fitted = 0
    for g, ref in enumerate(refs):
        s, n = slice(o[g], o[g + 1]), int(o[g + 1] - o[g])
        label = "group %d" % g
        status = int(rec[g, p + 10])
        if n < 2:
            assert status in (0, 3) and np.isnan(acc[g]) == (status != 0), label
            continue
        GC.check_record(rec[g], None, ref, p, True, None, None, label)
        compared += XC.check_accuracy(acc[g], status, call["y"][s], pred[s, 0] if status == 0 else None, ref, p, XC.THRESHOLD, label)
        fitted += status == 0
        if close_records(rec[g], host[g][:p + 11], ref, p, label):
            assert acc[g] == host[g][p + 11], label
    print(XC.ident(c), "fitted", fitted, "compared", compared)
    assert compared >= 3 and fitted >= 5


def test_device_pointer_entries(glm, ctx):
    """One device-pointer call of each entry: the host entry's bytes."""
    import torch
    call = XC.make_call(*POISSON_CALLS[1])
    d_off, d_y, d_x, d_o = to_device(call)
    core, pred = glm.glm_fit_predict_interval_batch_host(call["offsets"], call["y"], columns(call), options(call), XC.Z, offset=call["off"], ctx=ctx)
    dcore, dpred = ctx.glm_fit_predict_interval_batch_device(d_off, d_y, d_x, options(call), XC.Z, offset=d_o)
    torch.cuda.synchronize()
    assert dcore.cpu().numpy().tobytes() == core.tobytes() and dpred.cpu().numpy().tobytes() == pred.tobytes()
    assert np.isfinite(pred[:, 1:]).any()
    call = XC.make_call(*BINOMIAL_CALLS[2])
    d_off, d_y, d_x, d_o = to_device(call)
    rec, acc = glm.glm_fit_accuracy_batch_host(call["offsets"], call["y"], columns(call), options(call), 0.4, offset=call["off"], ctx=ctx)
    drec, dacc = ctx.glm_fit_accuracy_batch_device(d_off, d_y, d_x, options(call), 0.4, offset=d_o)
    torch.cuda.synchronize()
    assert drec.cpu().numpy().tobytes() == rec.tobytes() and dacc.cpu().numpy().tobytes() == acc.tobytes()
    assert np.isfinite(acc).sum() >= 5


def test_invalid_combinations_fail_the_call(glm, ctx):
    err = import_pkg("_abi").AnofoxStatsError
    pc, bc = XC.make_call(*POISSON_CALLS[0]), XC.make_call(*BINOMIAL_CALLS[0])
    for call, z, text in ((pc, -1.0, "glm: interval_z"), (pc, float("nan"), "glm: interval_z"), (pc, float("inf"), "glm: interval_z"),
                          (bc, XC.Z, "glm: the prediction interval of the binomial")):
        with pytest.raises(err, match=text):
            glm.glm_fit_predict_interval_batch_host(call["offsets"], call["y"], columns(call), options(call), z, ctx=ctx)
    for call, thr, text in ((pc, 0.5, "glm: the accuracy is the binomial"), (bc, float("nan"), "glm: threshold"),
                            (bc, float("-inf"), "glm: threshold")):
        with pytest.raises(err, match=text):
            glm.glm_fit_accuracy_batch_host(call["offsets"], call["y"], columns(call), options(call), thr, ctx=ctx)
    # the binomial family at interval_z = 0 is the plain fit-predict
    core, pred = glm.glm_fit_predict_interval_batch_host(bc["offsets"], bc["y"], columns(bc), options(bc), 0.0, ctx=ctx)
    core0, pred0 = glm.glm_fit_predict_batch_host(bc["offsets"], bc["y"], columns(bc), options(bc), ctx=ctx)
    assert core.tobytes() == core0.tobytes() and pred.tobytes() == pred0.tobytes()


def test_aggregates_carry_the_extras(glm):
    rng = np.random.default_rng(12)
    n = 90
    x = rng.uniform(-1, 1, (n, 2))
    y = rng.poisson(np.exp(0.8 + x @ [0.5, -0.4])).astype(float)
    keys = np.repeat([0, 1], n // 2)
    plain = glm.poisson_fit_predict_agg(keys, y, x, {"tolerance": 1e-12})
    assert np.all(np.isnan(plain.pred[:, 1:]))
    for level, z in ((0.95, 1.96), (0.99, 2.576), (0.90, 1.645), (0.8, 1.96)):
        fp = glm.poisson_fit_predict_agg(keys, y, x, {"tolerance": 1e-12, "interval": True, "confidence_level": level})
        assert fp.pred[:, 0].tobytes() == plain.pred[:, 0].tobytes()
        for g in (0, 1):
            m = keys == g
            lo, hi, _ = XC.formula(fp.pred[m, 0], fp.records[g, 2 + 5], z)
            assert np.allclose(fp.pred[m, 1], lo, rtol=1e-9, atol=0) and np.allclose(fp.pred[m, 2], hi, rtol=1e-9, atol=0)
    yb = (rng.uniform(size=n) < 1 / (1 + np.exp(-(0.2 + x @ [1.0, -1.0])))).astype(float)
    lg = glm.logistic_fit_agg(keys, yb, x, {"tolerance": 1e-12, "threshold": 0.4})
    bn = glm.binomial_fit_agg(keys, yb, x, {"tolerance": 1e-12})
    assert lg.records.tobytes() == bn.records.tobytes() and lg.threshold == 0.4
    for g in (0, 1):
        m = keys == g
        ref = GC.R.fit(GC.BINOMIAL, yb[m], x[m], None, True, 0.0)
        assert not (np.abs(ref["mu_all"] - 0.4) <= XC.BAND).any()     # no row inside the band (cap 0), on the restatement alone
        assert lg.row(g)["accuracy"] == XC.count_accuracy(yb[m], ref["mu_all"], 0.4) and lg.row(g)["threshold"] == 0.4
