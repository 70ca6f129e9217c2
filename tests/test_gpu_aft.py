"""GPU tier of the AFT family: the cases of tests/aft_cases.py through anofox_hip_aft_fit_batch_{host,device}, the scalar symbol
and the Python layer, against tests/aft_restate.py; repeatability of the bytes across calls, across the two entry points and
across the kernel's stride over the groups."""
import numpy as np
import pytest

import aft_cases as AC
from conftest import import_pkg

pytestmark = pytest.mark.gpu
CALLS = AC.calls()
IDS = [AC.call_id(c) for c in CALLS]
R = AC.R


@pytest.fixture(scope="module")
def aft():
    return import_pkg("aft")


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


def options(call, tolerance=1e-9, inference=True, max_iterations=100, confidence_level=0.95):
    return import_pkg("_abi").AnofoxHipAftBatchOptions(call["dist"], int(call["icpt"]), max_iterations, tolerance, int(inference),
                                                       confidence_level)


def run_host(aft, ctx, call, opts, inference=True):
    return aft.aft_fit_batch_host(call["offsets"], call["time"], AC.columns(call), call["event"], opts, inference=inference, ctx=ctx)


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_fit_host_and_device(aft, ctx, c):
    """The default tolerance 1e-9 and the tight 1e-14 through the host entry, every bound of aft_cases.check_record; the device
    entry and a repeated call give the same bytes."""
    import torch
    call = AC.make_call(*c)
    refs = AC.reference(call)
    for tolerance, tight in ((1e-9, False), (1e-14, True)):
        rec, inf = run_host(aft, ctx, call, options(call, tolerance))
        errs, n_compared, iters = {}, 0, 0
        for g, ref in enumerate(refs):
            n_compared += AC.check_record(rec[g], inf[g], ref, call, g, tolerance, tight, errs)
        ok = rec[:, -1] == 0
        iters = int(np.max(rec[ok, call["p"] + 10])) if ok.any() else 0
        print(AC.call_id(c), "tolerance %g: compared %d of %d, max iterations %d" % (tolerance, n_compared, len(refs), iters),
              {k: "%.2e" % v for k, v in errs.items()})
        assert n_compared >= 6   # (half of the 12 groups of 63 rows or more; the share over all calls is asserted on its own)
    again = run_host(aft, ctx, call, options(call, 1e-14))
    assert again[0].tobytes() == rec.tobytes() and again[1].tobytes() == inf.tobytes()
    dev = torch.device("cuda:0")
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    drec, dinf = ctx.aft_fit_batch_device(t(call["offsets"], torch.int64), t(call["time"]), [t(col) for col in AC.columns(call)],
                                          t(call["event"]), options(call, 1e-14), inference=True)
    torch.cuda.synchronize()
    assert drec.cpu().numpy().tobytes() == rec.tobytes() and dinf.cpu().numpy().tobytes() == inf.tobytes()
    rec_only = run_host(aft, ctx, call, options(call, 1e-14, inference=False), inference=False)
    assert rec_only.tobytes() == rec.tobytes()


def test_compared_share():
    """At least 90 % of the generated groups that the restatement fits are inside the tests' condition."""
    refs = [r for c in CALLS for r in AC.reference(AC.make_call(*c))]
    fitted = [r for r in refs if r["status"] == 0]
    assert sum(AC.compared(r) for r in fitted) >= 0.9 * len(fitted)


def tiny_batch(n_groups=2000, seed=77):
    """2000 groups of 5 to 12 rows, Weibull, p = 2 with an intercept (k = 4), about 20 % censored."""
    rng = np.random.default_rng(seed)
    T, E, X = [], [], []
    for _ in range(n_groups):
        t, e, x = AC.draw_group(rng, R.WEIBULL, 2, True, int(rng.integers(5, 13)), 0.2)
        T.append(t), E.append(e), X.append(x)
    offsets = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int64)
    return dict(dist=R.WEIBULL, p=2, icpt=True, k=4, offsets=offsets, time=np.concatenate(T), event=np.concatenate(E), x=np.vstack(X),
                kinds=["tiny"] * n_groups)


def test_many_tiny_groups_and_the_stride(aft, ctx):
    """A batch of 2000 tiny groups: one workgroup per group, and 48 workgroups that stride over the groups and reuse their LDS,
    give the same bytes; a sample of the groups against the restatement."""
    call = tiny_batch()
    rec, inf = run_host(aft, ctx, call, options(call, 1e-14))
    try:
        aft.aft_test_hooks(48)
        rec2, inf2 = run_host(aft, ctx, call, options(call, 1e-14))
    finally:
        aft.aft_test_hooks(0)
    assert rec2.tobytes() == rec.tobytes() and inf2.tobytes() == inf.tobytes()
    o, n_compared = call["offsets"], 0
    for g in range(0, 2000, 25):
        ref = R.fit(R.WEIBULL, call["time"][o[g]:o[g + 1]], call["x"][o[g]:o[g + 1]], call["event"][o[g]:o[g + 1]], True)
        n_compared += AC.check_record(rec[g], inf[g], ref, call, g, 1e-14, True)
    assert n_compared >= 40
    assert np.all(np.isin(rec[:, -1], (0, 1, 3, 6)))


def test_invalid_options_and_no_convergence(aft, ctx):
    call = AC.make_call(R.WEIBULL, 2, True)
    for bad in (options(call, float("nan")), options(call, max_iterations=0), options(call, -1.0), options(call, confidence_level=1.5)):
        rec, inf = run_host(aft, ctx, call, bad)
        assert np.all(rec[:, -1] == 1) and np.all(np.isnan(rec[:, :-1])) and np.all(np.isnan(inf))
    unknown = options(call)
    unknown.dist = 7
    assert np.all(run_host(aft, ctx, call, unknown, inference=False)[:, -1] == 1)
    rec = run_host(aft, ctx, call, options(call, 1e-14, inference=False, max_iterations=1), inference=False)
    assert np.sum(rec[:, -1] == 3) >= 10 and np.all(np.isnan(rec[rec[:, -1] == 3, :-1]))
    # a confidence level is looked at only with inference
    rec = run_host(aft, ctx, call, options(call, inference=False, confidence_level=1.5), inference=False)
    assert np.any(rec[:, -1] == 0)


def test_uncensored_lognormal_is_ols_of_log_time(aft, ctx):
    """Without censoring the lognormal fit's coefficients are the project's own OLS batch fit of log t, within 1e-8."""
    pkg = import_pkg()
    for p in (2, 9):
        rng = np.random.default_rng(31 + p)
        T, X = [], []
        for n in (p + 3, 40, 64, 65, 130):
            t, e, x = AC.draw_group(rng, R.LOGNORMAL, p, True, n, 0.0)
            T.append(t), X.append(x)
        offsets = np.concatenate([[0], np.cumsum([len(t) for t in T])]).astype(np.int64)
        time, x = np.concatenate(T), np.vstack(X)
        cols = [np.ascontiguousarray(x[:, j]) for j in range(p)]
        call = dict(dist=R.LOGNORMAL, icpt=True)
        rec = aft.aft_fit_batch_host(offsets, time, cols, np.ones(len(time)), options(call), ctx=ctx)
        ols = pkg.fit_batch_host(offsets, np.log(time), cols, None, pkg.RegressionOptions().batch_options("ols"), ctx=ctx)
        ols = ols[0] if isinstance(ols, tuple) else ols
        assert np.all(rec[:, -1] == 0)
        assert np.max(np.abs(rec[:, :p + 1] - ols[:, :p + 1])) <= 1e-8


def test_python_layer(aft, ctx):
    """aft_fit_agg with shuffled keys equals the batch call on sorted groups; row() of a failed group is None; aft_fit equals
    anofox_aft_fit's record of the same rows; a failing scalar call raises with the status as its code."""
    call = AC.make_call(R.LOGLOGISTIC, 2, True)
    o, G = call["offsets"], len(call["offsets"]) - 1
    keys = np.repeat(np.arange(G), np.diff(o))
    perm = np.random.default_rng(5).permutation(len(keys))
    opt = {"dist": "log-logistic", "compute_inference": True, "tolerance": 1e-12}
    res = aft.aft_fit_agg(keys[perm], call["time"][perm], call["x"][perm], call["event"][perm], opt, context=ctx)
    # the batch call on the groups sorted as the aggregate sorts them (stable: the shuffled order inside a group is kept)
    order = perm[np.argsort(keys[perm], kind="stable")]
    call = dict(call, time=call["time"][order], event=call["event"][order], x=call["x"][order])
    rec, inf = run_host(aft, ctx, call, options(call, 1e-12))
    assert res.records.tobytes() == rec.tobytes() and res.inference.tobytes() == inf.tobytes()
    ok = rec[:, -1] == 0
    failed = int(np.nonzero(~ok)[0][0])
    assert res.row(failed) is None
    g = int(np.nonzero(ok)[0][2])
    row = res.row(g)
    assert row["n_features"] == 2 and len(row["std_errors"]) == 2 and row["converged"] and np.isfinite(row["log_scale_std_error"])
    sl = slice(o[g], o[g + 1])
    one = aft.aft_fit(list(call["time"][sl]), [list(call["x"][sl, j]) for j in range(2)], list(call["event"][sl]), opt)
    assert one["coefficients"] == rec[g, :2].tolist() and one["intercept"] == rec[g, 2] and one["scale"] == rec[g, 3]
    assert one["log_likelihood"] == rec[g, 4] and one["null_log_likelihood"] == rec[g, 5] and one["n_events"] == rec[g, 9]
    assert one["std_errors"] == inf[g, :2].tolist() and one["intercept_std_error"] == inf[g, 10]
    assert one["log_scale_std_error"] == inf[g, 11]
    bad = slice(o[failed], o[failed + 1])
    with pytest.raises(import_pkg("options").InvalidInputException) as ei:
        aft.aft_fit(list(call["time"][bad]), [list(call["x"][bad, j]) for j in range(2)], list(call["event"][bad]), opt)
    assert ei.value.code == int(rec[failed, -1])
    # None entries are rows that are left out
    tl = [None if i == 1 else v for i, v in enumerate(call["time"][sl])]
    assert aft.aft_fit(tl, [list(call["x"][sl, j]) for j in range(2)], list(call["event"][sl]), opt)["n_observations"] == one["n_observations"] - 1
