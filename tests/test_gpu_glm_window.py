"""GPU tier of the GLM window function (csrc/glm_window.hip): the cases of tests/glm_window_cases.py through
anofox_hip_glm_fit_predict_{window,frames}_{host,device}.  The yardstick of every value is tests/glm_restate.py per frame, never
another run of the code under test; with the warm start off a frame has to be, bit for bit, what
anofox_hip_glm_fit_predict_batch_host returns for a group that holds exactly the frame's rows."""
import numpy as np
import pytest

import glm_window_cases as WC
from conftest import import_pkg

pytestmark = pytest.mark.gpu
CALLS = WC.calls() + list(WC.EXPLICIT)


@pytest.fixture(scope="module")
def pkg():
    return import_pkg()


@pytest.fixture(autouse=True)
def _reset_hooks(pkg):
    yield
    pkg.glm_window_test_hooks(0, 0, True)


def _options(pkg, case, tolerance=1e-8, max_iterations=100):
    return import_pkg("_abi").AnofoxHipGlmBatchOptions(case["family"], bool(case["icpt"]), max_iterations, tolerance, case["lam"], False, 0.95)


def _cols(case):
    return [np.ascontiguousarray(case["x"][:, j]) for j in range(case["p"])]


def _host(pkg, case, opts, interval_z=None, ctx=None):
    """(pred, records) through the host entry the case calls for."""
    if case["frame"] == "explicit":
        return pkg.glm_fit_predict_frames_host(case["y"], _cols(case), case["lo"], case["hi"], opts, offset=case["off"],
                                               interval_z=interval_z, want_records=True, ctx=ctx)
    return pkg.glm_fit_predict_window_host(case["offsets"], case["y"], _cols(case), opts, case["frame"], offset=case["off"],
                                           interval_z=interval_z, want_records=True, ctx=ctx)


def _device(pkg, case, opts, interval_z=None):
    import torch
    ctx = pkg.Context(0)
    t = lambda a, dt=torch.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()  # noqa: E731
    cols = [t(c) for c in _cols(case)]
    if case["frame"] == "explicit":
        # (the kernel reads the caller's bounds: the planner has checked them)
        pred, rec = ctx.glm_fit_predict_frames_device(t(case["y"]), cols, t(case["lo"], torch.int64), t(case["hi"], torch.int64), opts,
                                                      offset=t(case["off"]), interval_z=interval_z, want_records=True)
    else:
        pred, rec = ctx.glm_fit_predict_window_device(t(case["offsets"], torch.int64), t(case["y"]), cols, opts, case["frame"],
                                                      offset=t(case["off"]), interval_z=interval_z, want_records=True)
    torch.cuda.synchronize()
    stats = pkg.glm_window_stats(ctx)
    return pred.cpu().numpy(), rec.cpu().numpy(), stats


def _gathered(case):
    """Every frame's rows as a group of their own: (row_offsets, y, cols, offset, train_counts, the last gathered row of every
    frame or -1)."""
    idx, offs, last = [], [0], []
    for e in range(len(case["lo"])):
        s = WC.frame_rows(case, e)
        idx.append(np.arange(s.start, s.stop))
        offs.append(offs[-1] + s.stop - s.start)
        last.append(offs[-1] - 1 if s.stop > s.start else -1)
    idx = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    offs = np.array(offs, dtype=np.int64)
    y = case["y"][idx]
    train = np.array([int(np.sum(~np.isnan(y[a:b]))) for a, b in zip(offs[:-1], offs[1:])], dtype=np.int64)
    return (offs, y, [np.ascontiguousarray(case["x"][idx, j]) for j in range(case["p"])], None if case["off"] is None else case["off"][idx],
            train, np.array(last))


@pytest.mark.parametrize("c", CALLS, ids=WC.case_id)
def test_cold_walk_is_the_batch_fit_of_every_frame_bit_for_bit(pkg, c):
    """warm = 0: records and {mu, lower, upper} are the bytes of anofox_hip_glm_fit_predict_[interval_]batch_host on the gathered
    frames; _host and _device give the same bytes."""
    case = WC.make(c)
    opts = _options(pkg, case)
    z = 1.96 if case["family"] == WC.POISSON else None
    pkg.glm_window_test_hooks(0, 0, False)
    pred, rec = _host(pkg, case, opts, z)
    st = pkg.glm_window_stats()
    assert st["frames"] == len(pred) == st["cold_starts"] and st["warm_starts"] == st["refits"] == 0
    dpred, drec, dst = _device(pkg, case, opts, z)
    assert pred.tobytes() == dpred.tobytes() and rec.tobytes() == drec.tobytes() and dst == st
    offs, gy, gcols, goff, train, last = _gathered(case)
    core, gpred = pkg.glm_fit_predict_batch_host(offs, gy, gcols, opts, offset=goff, train_counts=train, interval_z=z)
    assert core.tobytes() == rec.tobytes()
    want = np.where((last >= 0)[:, None], gpred[np.maximum(last, 0)], np.nan)
    assert want.tobytes() == pred.tobytes()


@pytest.mark.parametrize("c", CALLS, ids=WC.case_id)
def test_warm_walk_against_the_restatement(pkg, c, record_property):
    """warm = 1: tolerance 1e-12 under glm_cases.check_record's bounds, the default tolerance under the long-double objective
    gap; statuses and NaN patterns exact; warm + cold = the frames; _host and _device give the same bytes."""
    case = WC.make(c)
    refs = WC.reference(case)
    for tol, tight in ((1e-12, True), (1e-8, False)):
        opts = _options(pkg, case, tol)
        pred, rec = _host(pkg, case, opts)
        st = pkg.glm_window_stats()
        dpred, drec, dst = _device(pkg, case, opts)
        assert pred.tobytes() == dpred.tobytes() and rec.tobytes() == drec.tobytes() and dst == st
        assert st["frames"] == len(pred) == st["cold_starts"] + st["warm_starts"] and st["refits"] <= st["warm_starts"]
        assert np.all(np.isnan(pred[:, 1:]))
        errs, compared = {}, 0
        for e, ref in enumerate(refs):
            compared += WC.check_frame(rec[e], pred[e], ref, case, e, tight, errs)
        print(WC.case_id(c), tol, "compared", compared, st, {k: "%.2e" % v for k, v in errs.items()})
        for k, v in errs.items():
            record_property(k, v)
        assert c[2] == (None, None) or st["warm_starts"] > 0


@pytest.mark.parametrize("run_length, cap_waves", [(1, 0), (7, 0), (7, 3)])
def test_hooks_keep_statuses_and_bounds(pkg, run_length, cap_waves):
    """Runs of 1 and 7 rows, and a scratch cap that leaves 3 wavefronts for many walkers: the status and NaN patterns of the
    unhooked call, the values within the restatement's bounds."""
    c = WC.calls()[0]
    case = WC.make(c)
    refs = WC.reference(case)
    opts = _options(pkg, case, 1e-12)
    _, base = _host(pkg, case, opts)
    span = int(np.max(case["hi"] - case["lo"]))
    pkg.glm_window_test_hooks(run_length, 16 * span * cap_waves + 8 if cap_waves else 0, True)
    pred, rec = _host(pkg, case, opts)
    st = pkg.glm_window_stats()
    p = case["p"]
    assert st["walkers"] == len(WC.cut_runs(case, run_length)) - 1 and st["span_rows"] == span
    assert st["waves"] == (cap_waves or st["walkers"]) and st["waves"] <= st["walkers"]
    assert rec[:, p + 10].tobytes() == base[:, p + 10].tobytes() and np.array_equal(np.isnan(rec), np.isnan(base))
    for e, ref in enumerate(refs):
        WC.check_frame(rec[e], pred[e], ref, case, e, True, {})
    assert st["cold_starts"] + st["warm_starts"] == len(pred) and (run_length > 1 or st["warm_starts"] == 0)


def test_scratch_budget_failure_message(pkg):
    case = WC.make(WC.calls()[0])
    span = int(np.max(case["hi"] - case["lo"]))
    pkg.glm_window_test_hooks(0, 16 * span - 1, True)
    with pytest.raises(pkg.AnofoxStatsError, match=r"glm window: frame of %d rows exceeds the scratch budget" % span) as ei:
        _host(pkg, case, _options(pkg, case))
    assert ei.value.code == 1
    pkg.glm_window_test_hooks(0, 16 * span, True)
    assert pkg.glm_window_stats is not None and _host(pkg, case, _options(pkg, case))[0].shape == (len(case["y"]), 3)
    assert pkg.glm_window_stats()["waves"] == 1


def test_invalid_options_fail_every_row(pkg):
    case = WC.make(WC.calls()[0])
    pred, rec = _host(pkg, case, _options(pkg, case, tolerance=float("nan")))
    p = case["p"]
    assert np.all(rec[:, p + 10] == 1) and np.all(np.isnan(rec[:, :p + 10])) and np.all(np.isnan(pred))


def test_same_bytes_with_other_calls_in_between(pkg):
    """The slabs live in the context's workspace, which a batch GLM call and a quantile window call use too: a second window call
    after them gives the first one's bytes."""
    case = WC.make(WC.calls()[3])
    opts = _options(pkg, case)
    pred, rec = _host(pkg, case, opts)
    st = pkg.glm_window_stats()
    pkg.glm_fit_predict_batch_host(case["offsets"], case["y"], _cols(case), opts, offset=case["off"])
    q = pkg.QuantileOptions().batch_options()
    pkg.quantile_fit_predict_window_host(case["offsets"], case["y"], _cols(case), q, (30, 0))
    pred2, rec2 = _host(pkg, case, opts)
    assert pred.tobytes() == pred2.tobytes() and rec.tobytes() == rec2.tobytes() and pkg.glm_window_stats() == st


def test_python_functions_against_the_abi(pkg):
    """poisson_fit_predict / logistic_fit_predict on shuffled rows = the window entry on the sorted ones, in input row order."""
    for c, fn, options in ((WC.calls()[0], pkg.poisson_fit_predict, {"interval": True, "confidence_level": 0.99}),
                           (WC.calls()[17], pkg.logistic_fit_predict, None)):
        case = WC.make(c)
        N, p = len(case["y"]), case["p"]
        part = np.repeat(np.arange(len(case["offsets"]) - 1), np.diff(case["offsets"]))
        options = dict(options or {}, fit_intercept=bool(case["icpt"]), **{"lambda": case["lam"]})
        x = case["x"]
        if case["off"] is not None:
            x = np.hstack([x, case["off"][:, None]])
            options["offset"] = p + 1
        shuffle = np.random.default_rng(9).permutation(N)
        res = fn(part[shuffle], np.arange(N)[shuffle], case["y"][shuffle], x[shuffle], options, frame=c[2])
        z = 2.576 if "interval" in options else None
        want, _ = _host(pkg, case, _options(pkg, case), z)
        assert res.pred.shape == (N, 3) and res.pred.tobytes() == want[shuffle].tobytes()
        assert np.array_equal(res.yhat, res.pred[:, 0], equal_nan=True)
