"""GPU tier of the AFT fit-predict: anofox_hip_aft_fit_predict_batch_{host,device} and aft_fit_predict_agg on the small calls of
tests/aft_predict_cases.py: p in {1, 8, 9, 32} with and without an intercept (the three entry classes of an_entry_class) for the
four distributions, groups of k + 1, 63, 64, 65 and 129 rows (the 64-row tile's edges), two failed groups.

What is asserted, and why the bounds are what they are: tests/aft_predict_cases.py (`check_pred`).  The restatement is evaluated
at the eta and scale the GPU returned, so the device's math library is the only difference; the largest errors seen on the MI355X
are recorded in docs/PARITY.md."""
import math

import numpy as np
import pytest

import aft_cases as AC
import aft_predict_cases as PC
from conftest import import_pkg

pytestmark = pytest.mark.gpu
CALLS = PC.calls()
IDS = [AC.call_id(c) for c in CALLS]
R = AC.R
QUANTILE = 0.3


@pytest.fixture(scope="module")
def aft():
    return import_pkg("aft")


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


def options(call, inference=True):
    return import_pkg("_abi").AnofoxHipAftBatchOptions(call["dist"], int(call["icpt"]), 100, 1e-9, int(inference), 0.95)


def predict_options(quantile, horizon):
    return import_pkg("_abi").AnofoxHipAftPredictOptions(quantile, float("nan") if horizon is None else horizon)


def fit_predict(aft, ctx, call, quantile, horizon, inference=True):
    return aft.aft_fit_predict_batch_host(call["offsets"], call["time"], AC.columns(call), call["event"], options(call, inference),
                                          predict_options(quantile, horizon), inference=inference, ctx=ctx)


def fit(aft, ctx, call, inference=True):
    return aft.aft_fit_batch_host(call["offsets"], call["time"], AC.columns(call), call["event"], options(call, inference),
                                  inference=inference, ctx=ctx)


def device_call(ctx, call, quantile, horizon, offsets=None, sentinel=None):
    import torch
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    out = None if sentinel is None else torch.full((len(call["time"]), 4), sentinel, dtype=torch.float64, device=dev)
    rec, inf, pred = ctx.aft_fit_predict_batch_device(t(call["offsets"] if offsets is None else offsets, torch.int64), t(call["time"]),
                                                      [t(c) for c in AC.columns(call)], t(call["event"]), options(call),
                                                      predict_options(quantile, horizon), inference=True, pred_out=out)
    torch.cuda.synchronize()
    return rec.cpu().numpy(), inf.cpu().numpy(), pred.cpu().numpy()


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_fit_predict(aft, ctx, c):
    """Cases 1 to 3 and 5 of the family's fit-predict: the record and the inference are the fit's own bytes; the rows to score
    leave the record what the training rows alone give; every rule and bound of check_pred; failed groups are all NaN; a second
    call and the device entry give the same bytes."""
    call = PC.make_call(*c, small=True)
    p, h, o = call["p"], PC.horizon_of(call), call["offsets"]
    rec, inf, pred = fit_predict(aft, ctx, call, QUANTILE, h)
    frec, finf = fit(aft, ctx, call)
    assert rec.tobytes() == frec.tobytes() and inf.tobytes() == finf.tobytes()
    alone, _ = fit(aft, ctx, call["base"])
    assert alone.tobytes() == rec.tobytes(), "rows to score changed a record"
    assert pred.shape == (len(call["time"]), 4)
    errs, n_tight = {}, 0
    for g in range(len(o) - 1):
        n_tight += PC.check_pred(pred[o[g]:o[g + 1]], rec[g], call, g, QUANTILE, h, errs)
    status = rec[:, p + 12].astype(int).tolist()
    # (the group of k + 1 rows is all but interpolated: it may stop at status 3, and then it is a failed group like the last two)
    assert status[0] in (0, 3) and status[1:5] == [0] * 4 and status[5:] == [1, 1], status
    print(AC.call_id(c), "rows under the tight bound %d of %d" % (n_tight, int(o[5])), {k: "%.2e" % v for k, v in errs.items()})
    assert n_tight >= 0.5 * int(o[5])
    again = fit_predict(aft, ctx, call, QUANTILE, h)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rec, inf, pred)))
    drec, dinf, dpred = device_call(ctx, call, QUANTILE, h)
    assert drec.tobytes() == rec.tobytes() and dinf.tobytes() == inf.tobytes() and dpred.tobytes() == pred.tobytes()
    rec_only, none, pred_only = fit_predict(aft, ctx, call, QUANTILE, h, inference=False)
    assert none is None and rec_only.tobytes() == rec.tobytes() and pred_only.tobytes() == pred.tobytes()


@pytest.mark.parametrize("dist", AC.DISTS, ids=[R.NAMES[d] for d in AC.DISTS])
def test_known_answers(aft, ctx, dist):
    """Case 4.  Horizon 0: risk exactly 0.  No horizon: risk all NaN and the other slots the same bytes.  time <= 0: cdf 0.  The
    exponential's risk does not depend on t (inside check_pred).  The median of a lognormal time is exp(eta) to 1 ulp."""
    call = PC.make_call(dist, 8, True, small=True)
    o, p = call["offsets"], call["p"]
    rec, _, pred = fit_predict(aft, ctx, call, 0.5, PC.horizon_of(call))
    _, _, pn = fit_predict(aft, ctx, call, 0.5, None)
    _, _, pz = fit_predict(aft, ctx, call, 0.5, 0.0)
    assert pn[:, :3].tobytes() == pred[:, :3].tobytes() and pz[:, :3].tobytes() == pred[:, :3].tobytes()
    assert np.all(np.isnan(pn[:, 3]))
    scored = np.isfinite(pred[:, 0])
    assert scored.sum() > 300
    timed = scored & np.isfinite(call["time"])
    assert np.all(pz[timed, 3] == 0.0) and not np.any(np.signbit(pz[timed, 3])) and np.all(np.isnan(pz[scored & ~timed, 3]))
    assert np.all(pred[timed & (call["time"] <= 0.0), 2] == 0.0) and np.sum(timed & (call["time"] <= 0.0)) >= 8
    for g in range(len(o) - 1):
        PC.check_pred(pred[o[g]:o[g + 1]], rec[g], call, g, 0.5, PC.horizon_of(call))
        PC.check_pred(pn[o[g]:o[g + 1]], rec[g], call, g, 0.5, None)
        PC.check_pred(pz[o[g]:o[g + 1]], rec[g], call, g, 0.5, 0.0)
    if dist == R.LOGNORMAL:
        want = np.array([math.exp(v) for v in pred[scored, 0]])
        ulps = np.abs(pred[scored, 1] - want) / np.spacing(want)
        print("lognormal median against exp(eta): max %.2f ulp" % float(np.max(ulps)))
        assert np.all(ulps <= 1.0)


def test_grid_stride_and_neighbours(aft, ctx):
    """Cases 5 and 6.  With two workgroups for seven groups the grid strides over the groups and the bytes stay.  A call on the
    middle groups alone writes exactly their rows' slots: the others keep the sentinel."""
    call = PC.make_call(R.WEIBULL, 9, True, small=True)
    o, h = call["offsets"], PC.horizon_of(call)
    rec, inf, pred = fit_predict(aft, ctx, call, QUANTILE, h)
    aft.aft_test_hooks(2)
    try:
        strided = fit_predict(aft, ctx, call, QUANTILE, h)
    finally:
        aft.aft_test_hooks(0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(strided, (rec, inf, pred)))
    sentinel = -4321.5
    drec, _, dpred = device_call(ctx, call, QUANTILE, h, offsets=o[2:6], sentinel=sentinel)
    assert drec.tobytes() == rec[2:5].tobytes()
    lo, hi = int(o[2]), int(o[5])
    assert np.all(dpred[:lo] == sentinel) and np.all(dpred[hi:] == sentinel)
    assert dpred[lo:hi].tobytes() == pred[lo:hi].tobytes() and not np.any(dpred[lo:hi] == sentinel)


def test_python_layer_and_option_errors(aft, ctx):
    """aft_fit_predict_agg: the input's row order, the named views, None for a row to score; the two option errors."""
    call = PC.make_call(R.LOGLOGISTIC, 8, True, small=True)
    o, h = call["offsets"], PC.horizon_of(call)
    rec, inf, pred = fit_predict(aft, ctx, call, 0.25, h)
    keys = np.repeat(np.arange(len(o) - 1), np.diff(o))
    # the groups' rows interleaved, each group's own order kept: the stable sort by key gives back the batch call's order
    shuffle = np.argsort(np.concatenate([np.arange(n) for n in np.diff(o)]), kind="stable")
    event = [None if np.isnan(v) else v for v in call["event"][shuffle]]
    res = aft.aft_fit_predict_agg(keys[shuffle], call["time"][shuffle], call["x"][shuffle], event,
                                  {"dist": "loglogistic", "quantile": 0.25, "horizon": h, "compute_inference": True}, context=ctx)
    assert res.status.tolist() == rec[:, -1].astype(int).tolist() and res.row(5) is None and res.row(1)["n_features"] == 8
    assert res.records.tobytes() == rec.tobytes() and res.inference.tobytes() == inf.tobytes()
    assert res.pred.tobytes() == pred[shuffle].tobytes()
    assert res.eta is not None and np.array_equal(res.cdf, res.pred[:, 2], equal_nan=True)
    assert np.array_equal(res.risk, res.pred[:, 3], equal_nan=True) and np.array_equal(res.time_quantile, res.pred[:, 1], equal_nan=True)
    assert np.all(np.isnan(aft.aft_fit_predict_agg(keys, call["time"], call["x"], call["event"], {"dist": "loglogistic"}, context=ctx).risk))
    err = import_pkg("_abi").AnofoxStatsError
    for q in (0.0, 1.0, float("nan"), -0.5):
        with pytest.raises(err, match=r"aft: quantile must be in \(0, 1\)"):
            fit_predict(aft, ctx, call, q, h)
    for bad in (-1.0, float("inf")):
        with pytest.raises(err, match="aft: horizon must be finite and >= 0"):
            fit_predict(aft, ctx, call, 0.5, bad)
