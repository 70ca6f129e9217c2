"""The elastic net and BLS / NNLS Finalize of a streaming state (anofox_hip_agg_state_finalize_{elasticnet,bls}_*) on an MI355X
(run with -m gpu).  Inputs and tolerances: tests/state_models_cases.py — the restatement is held to what
test_gpu_fuzz_families applies to the batch entry points (conftest.COEF_RTOL / DIAG_RTOL), the batch entry point on the
grouped rows to what test_gpu_streaming applies between a regression state and its batch call (1e-10 / 1e-8).  Every test
uses a handful of states."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls_restate as br  # noqa: E402
import state_models_cases as smc  # noqa: E402
from conftest import assert_records_match, import_pkg  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = ["elasticnet", "bls"]


@pytest.fixture(scope="module")
def pkg():
    return import_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _opts(pkg, c, **over):
    kw = dict(c.kw, **over)
    if c.family == "elasticnet":
        return pkg.ElasticNetOptions(tolerance=1e-14, max_iterations=2_000_000, **kw).batch_options()
    return pkg.BlsOptions(**kw).batch_options()


def _state(pkg, ctx, c, retain=True, model="ols", **kw):
    ro = pkg.RegressionOptions(fit_intercept=c.icpt, **kw).batch_options(model)
    st = pkg.AggState(ctx, c.p, ro, retain_bytes=(1 << 28) if retain else 0)
    r0, k = 0, 0
    while r0 < len(c.slot):                                  # updates in chunks of 2048, 1, 7 and 64 rows
        n = smc.CHUNKS[k % len(smc.CHUNKS)]
        k += 1
        s = slice(r0, r0 + n)
        st.update(c.slot[s], c.y[s], c.X[s], np.ones(len(c.y[s])) if model == "wls" else None, c.valid[s], n_slots=c.S)
        r0 += n
    return st


def _finalize(st, c, o, slots=None):
    return (st.finalize_elasticnet if c.family == "elasticnet" else st.finalize_bls)(o, slots=slots)


def _batch(pkg, ctx, c, o):
    cols = [np.ascontiguousarray(c.gX[:, j]) for j in range(c.p)]
    fn = pkg.elasticnet_fit_batch_host if c.family == "elasticnet" else pkg.bls_fit_batch_host
    return fn(c.goffs, c.gy, cols, o, ctx=ctx)


def _xbar(c):
    xb = np.zeros((c.S, c.p))
    for g in range(c.S):
        s = slice(c.goffs[g], c.goffs[g + 1])
        ok = np.isfinite(c.gy[s]) & np.isfinite(c.gX[s]).all(axis=1)
        if ok.any():
            xb[g] = np.abs(c.gX[s][ok]).mean(axis=0)
    return xb


def _zero_df(c, rec):
    """Slots without residual degrees of freedom: diagnostics are ratios of rounding noise (assert_records_match)."""
    p = c.p
    k = np.sum(~np.isnan(rec[:, :p]), axis=1) + int(c.icpt)
    return [g for g in range(len(rec)) if rec[g, p + 5] == 0 and rec[g, p + (4 if c.family == "elasticnet" else 3)] - k[g] <= 0]


def _match(c, got, ref, what, idx=None, xbar=None, skip=(), **tol):
    """Statuses, NaN pattern, n_obs and the BLS flags exactly, numbers within `tol` (default: the restatement's tolerances)."""
    idx = np.arange(len(ref)) if idx is None else np.asarray(idx)
    if c.family == "elasticnet":
        skip_local = [k for k, g in enumerate(idx) if int(g) in set(skip)]
        assert_records_match(got[idx], ref[idx], c.p, what=what, skip_diag_groups=skip_local, xbar=None if xbar is None else xbar[idx], **tol)
        return
    for g in idx:
        if int(g) in set(skip) and ref[g, c.p + 5] == 0:      # coefficients, counts and flags only
            r, q = ref[g].copy(), got[g].copy()
            assert np.isnan(q[c.p + 1]) == np.isnan(r[c.p + 1])
            q[c.p + 1:c.p + 3] = r[c.p + 1:c.p + 3]
            br.assert_record_matches(q, r, c.p, xbar=None if xbar is None else xbar[g], what=f"{what} slot {g}", **tol)
        else:
            br.assert_record_matches(got[g], ref[g], c.p, xbar=None if xbar is None else xbar[g], what=f"{what} slot {g}", **tol)


def _iterations_match(c, its, bits):
    """Iteration counts of a state's Finalize against the batch call's.  Where the moments agree bit for bit the counts are
    equal: a log-only state runs the batch path on the same rows in the same groups (here), and so do the whole-number slots a
    moment state refits from its log (test_flagged_groups_with_and_without_a_row_log).  The other slots of a moment state see
    moments that were summed chunk by chunk, the batch call's up to rounding; with the tolerance these tests set (1e-14, next to
    the rounding of a coordinate move) the sweep at which the largest move drops below the threshold is not determined by the
    data alone, so there the counts are held to their sign — converged, shortcut or stopped alike — and the largest
    difference is printed."""
    d = np.abs(np.abs(its.astype(np.int64)) - np.abs(bits.astype(np.int64)))
    print(f"iterations {c.family} p={c.p} intercept={c.icpt}: largest difference {int(d.max())}, {int((d != 0).sum())} of {d.size} slots differ")
    assert np.array_equal(np.sign(its), np.sign(bits))
    if c.p > 8:
        assert np.array_equal(its, bits)


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("p", smc.MOMENT_P + smc.LOG_ONLY_P)
@pytest.mark.parametrize("family", FAMILIES)
def test_parity_with_restatement_and_batch(pkg, ctx, family, p, icpt):
    c, ref = smc.cached(family, p, icpt, restated=True)
    o = _opts(pkg, c)
    st = _state(pkg, ctx, c)
    try:
        rec, its, unrefined = _finalize(st, c, o)
        brec, bits = _batch(pkg, ctx, c, o)
    finally:
        st.close()
    what = f"state {family} p={p} intercept={icpt}"
    assert len(unrefined) == 0
    skip = ref[1] if family == "elasticnet" else _zero_df(c, ref[0])
    _match(c, rec, ref[0], what + " vs restatement", xbar=_xbar(c), skip=skip)
    _match(c, rec, brec, what + " vs batch", skip=_zero_df(c, brec), **smc.STATE_VS_BATCH)
    _iterations_match(c, its, bits)


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("p", smc.MOMENT_P)
@pytest.mark.parametrize("family", FAMILIES)
def test_flagged_groups_with_and_without_a_row_log(pkg, ctx, family, p, icpt):
    c = smc.cached(family, p, icpt, exact=True)
    o = _opts(pkg, c)
    with_log, without = _state(pkg, ctx, c, retain=True), _state(pkg, ctx, c, retain=False)
    try:
        rec, its, unrefined = _finalize(with_log, c, o)
        nrec, nits, nunref = _finalize(without, c, o)
        brec, bits = _batch(pkg, ctx, c, o)
    finally:
        with_log.close()
        without.close()
    what = f"flagged {family} p={p} intercept={icpt}"
    P = c.p
    r2_at = P + 1 if family == "elasticnet" else P + 2
    # with the log: numbers everywhere, the batch call's
    assert len(unrefined) == 0 and not np.any(rec[:, P + 5] == 101)
    _match(c, rec, brec, what + " with log vs batch", skip=_zero_df(c, brec), **smc.STATE_VS_BATCH)
    # without: exactly the cancelled slots are status 101 / NaN, listed and counted; nobody else is touched
    flagged = np.nonzero(nrec[:, P + 5] == 101)[0]
    assert np.array_equal(np.sort(nunref), flagged)
    assert np.all(np.isnan(np.delete(nrec[flagged], P + 5, axis=1)))
    designed = [g for g in c.exact_slots if brec[g, P + 5] == 0 and not np.isnan(brec[g, r2_at])]
    assert len(designed) >= 3 and set(designed) <= set(flagged.tolist())
    assert np.array_equal(its[designed], bits[designed])     # whole-number moments: the refit is the batch call bit for bit
    assert np.array_equal(rec[designed], brec[designed], equal_nan=True)
    assert np.all(brec[flagged, r2_at] > 1.0 - 1e-6), "a slot was flagged whose ssr had not cancelled"
    rest = np.setdiff1d(np.arange(c.S), flagged)
    assert np.array_equal(nrec[rest], rec[rest], equal_nan=True) and np.array_equal(nits[rest], its[rest])


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("p", [3, 9])
def test_reuse_of_one_state(pkg, ctx, p, icpt):
    c = smc.cached("elasticnet", p, icpt)
    a1, a2 = smc.alpha_grid(c)
    st, fresh = _state(pkg, ctx, c), _state(pkg, ctx, c)
    try:
        ols_core, _, _ = st.finalize()
        e1 = st.finalize_elasticnet(_opts(pkg, c, alpha=a1))
        e2 = st.finalize_elasticnet(_opts(pkg, c, alpha=a2))
        nn = st.finalize_bls(pkg.BlsOptions(fit_intercept=icpt).batch_options())
        e1b = st.finalize_elasticnet(_opts(pkg, c, alpha=a1))
        ols_again, _, _ = st.finalize()
        ols_fresh, _, _ = fresh.finalize()
    finally:
        st.close()
        fresh.close()
    assert np.array_equal(e1[0], e1b[0], equal_nan=True) and np.array_equal(e1[1], e1b[1])
    assert not np.array_equal(e1[0], e2[0], equal_nan=True)
    assert nn[0].shape == (c.S, 3 * p + 6) and (nn[0][:, p + 5] == 0).any()
    assert np.array_equal(ols_core, ols_fresh, equal_nan=True) and np.array_equal(ols_again, ols_fresh, equal_nan=True)


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("p", [3, 9])
def test_combine_then_finalize(pkg, ctx, family, p, icpt):
    c = smc.cached(family, p, icpt)
    o = _opts(pkg, c)
    # every slot's rows split over two slots: odd arrivals go to slot + S
    split = smc.Case()
    split.__dict__.update(c.__dict__)
    seen = np.zeros(c.S, dtype=np.int64)
    nth = np.empty(len(c.slot), dtype=np.int64)
    for i, s in enumerate(c.slot):
        nth[i] = seen[s]
        seen[s] += 1
    split.slot = np.where(nth % 2 == 1, c.slot + c.S, c.slot).astype(np.uint32)
    split.S = 2 * c.S
    whole, halves = _state(pkg, ctx, c), _state(pkg, ctx, split)
    try:
        rec, _, _ = _finalize(whole, c, o)
        halves.combine(np.arange(c.S, 2 * c.S, dtype=np.uint32), np.arange(c.S, dtype=np.uint32))
        crec, _, unref = _finalize(halves, c, o)
    finally:
        whole.close()
        halves.close()
    assert len(unref) == 0 and crec.shape[0] == 2 * c.S
    assert np.all(crec[c.S:, p + 5] == 100)                  # the emptied sources
    _match(c, crec[:c.S], rec, f"combine {family} p={p} intercept={icpt}", skip=_zero_df(c, rec), **smc.STATE_VS_BATCH)


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("p,exact", [(3, False), (9, False), (3, True), (8, True)])   # (flagged slots: moment states only)
def test_slots_host_equals_the_rows_of_the_full_finalize(pkg, ctx, family, p, exact, icpt):
    c = smc.cached(family, p, icpt, exact=exact)
    o = _opts(pkg, c)
    st = _state(pkg, ctx, c)
    try:
        rec, its, _ = _finalize(st, c, o)
        pick = np.random.default_rng(5).permutation(c.S)[:c.S // 3].astype(np.uint32)
        srec, sits, sunref = _finalize(st, c, o, slots=pick)
        assert len(sunref) == 0
        tight = np.ones(len(pick), dtype=bool)
        if exact:
            # Slots refitted from the log go through the batch path as a batch of the flagged slots alone, and that path sums a
            # group's moments in an order it picks by the batch's mean group size: the listed third is another batch than all
            # slots.  The exact-fit slots hold whole numbers (the same bits in any order); the other flagged slots (no residual
            # degrees of freedom) are held to the state-vs-batch tolerance on their coefficients instead.
            bare = _state(pkg, ctx, c, retain=False)
            try:
                flagged = _finalize(bare, c, o)[2]
            finally:
                bare.close()
            loose = np.setdiff1d(flagged, c.exact_slots)
            assert set(loose.tolist()) <= set(_zero_df(c, rec))
            tight = ~np.isin(pick, loose)
            assert np.isin(pick, c.exact_slots).any()
            sub = rec.copy()
            sub[pick] = srec
            if np.isin(pick, loose).any():
                _match(c, sub, rec, f"listed {family} p={p}", idx=np.intersect1d(pick, loose), skip=loose.tolist(), **smc.STATE_VS_BATCH)
        assert np.array_equal(srec[tight], rec[pick][tight], equal_nan=True) and np.array_equal(sits[tight], its[pick][tight])
        for bad in (np.array([1, 2, 1], dtype=np.uint32), np.array([0, c.S], dtype=np.uint32)):
            with pytest.raises(pkg.AnofoxStatsError) as ei:
                _finalize(st, c, o, slots=bad)
            assert ei.value.code == 1
    finally:
        st.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_option_errors(pkg, ctx, family):
    abi = import_pkg("_abi")
    lib = abi.load()
    c = smc.cached(family, 3, True)
    o = _opts(pkg, c)
    states = [(_state(pkg, ctx, c), dict(fit_intercept=False), "fit_intercept")]
    wls = smc.Case()
    wls.__dict__.update(c.__dict__)
    states.append((_state(pkg, ctx, wls, model="wls"), {}, "WLS"))
    states.append((_state(pkg, ctx, c, compute_inference=True, hc_type="hc1"), {}, "hc_type"))
    import ctypes as C
    try:
        for st, over, msg in states:
            # through the C entry point itself (the Python layer checks the same things before it gets there)
            oo = _opts(pkg, c, **over)
            rec = np.empty((c.S, 3 * c.p + 6))
            err = abi.AnofoxError()
            fn = getattr(lib, f"anofox_hip_agg_state_finalize_{family}_host")
            ok = fn(st._h, c.S, oo, rec.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, C.byref(err))
            assert not ok and err.code == abi.ERROR_INVALID_INPUT and msg in err.text(), err.text()
        st = states[0][0]
        if family == "elasticnet":
            with pytest.raises(pkg.AnofoxStatsError, match="tolerance") as ei:
                st.finalize_elasticnet(pkg.ElasticNetOptions(tolerance=-1.0, fit_intercept=True).batch_options())
            assert ei.value.code == abi.ERROR_INVALID_INPUT
        else:
            # bounds of a wrong length: status 1 everywhere except the status-100 slots
            good, _, _ = st.finalize_bls(o)
            rec, _, unref = st.finalize_bls(pkg.BlsOptions(fit_intercept=True, lower_bound=[0.0, 0.0]).batch_options())
            empty = good[:, c.p + 5] == 100
            assert empty.any() and np.all(rec[empty, c.p + 5] == 100) and np.all(rec[~empty, c.p + 5] == 1) and len(unref) == 0
    finally:
        for st, _, _ in states:
            st.close()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("p,exact,retain", [(3, True, True), (3, True, False), (9, False, True)])
@pytest.mark.parametrize("icpt", [True, False])
def test_device_forms_equal_the_host_forms(pkg, ctx, family, p, exact, retain, icpt):
    import torch
    c = smc.cached(family, p, icpt, exact=exact)
    o = _opts(pkg, c)
    st = _state(pkg, ctx, c, retain=retain)
    try:
        rec, its, _ = _finalize(st, c, o)
        d_rec = torch.empty(rec.shape, dtype=torch.float64, device="cuda")
        d_its = torch.empty(c.S, dtype=torch.int32, device="cuda")
        (st.finalize_elasticnet_device if family == "elasticnet" else st.finalize_bls_device)(o, d_rec, d_its)
        torch.cuda.synchronize()
    finally:
        st.close()
    assert np.array_equal(d_rec.cpu().numpy(), rec, equal_nan=True) and np.array_equal(d_its.cpu().numpy(), its)


@pytest.mark.parametrize("icpt", [True, False])
def test_streaming_states_methods_equal_the_state_calls(pkg, ctx, icpt):
    """StreamingStates.finalize_elasticnet / finalize_bls / finalize_nnls (MAP options in, result objects out) against
    AggState.finalize_* on the same state; two trailing slots never receive a row (reserved by the pool)."""
    c = smc.cached("elasticnet", 3, icpt)
    pool = pkg.StreamingStates(ctx)
    try:
        pool.ensure(c.p, pkg.RegressionOptions(fit_intercept=icpt).batch_options("ols"))
        assert len(pool.new_slots(c.S + 2)) == c.S + 2
        pool.state.update(c.slot, c.y, c.X, None, c.valid, n_slots=c.S)
        n = pool.n_slots
        en_map = {"alpha": c.kw["alpha"], "l1_ratio": 0.5, "fit_intercept": icpt, "tolerance": 1e-14, "max_iterations": 2_000_000}
        bls_map = {"fit_intercept": icpt, "lower_bound": -0.25, "upper_bound": 0.5}
        pick = np.random.default_rng(9).permutation(n)[:n // 3].astype(np.uint32)
        for slots in (None, pick):
            keys = np.arange(n, dtype=np.uint32) if slots is None else pick
            res, unref = pool.finalize_elasticnet(en_map, slots=slots)
            core, its, u = pool.state.finalize_elasticnet(pkg.parse_elasticnet_options(en_map).batch_options(), slots=slots, n_slots=n)
            assert isinstance(res, pkg.FitAggResult) and np.array_equal(res.keys, keys) and np.array_equal(unref, u)
            assert np.array_equal(res.coefficients, core[:, :3], equal_nan=True) and np.array_equal(res.intercept, core[:, 3], equal_nan=True)
            assert np.array_equal(res.r_squared, core[:, 4], equal_nan=True) and np.array_equal(res.residual_std_error, core[:, 6], equal_nan=True)
            assert np.array_equal(res.status, core[:, 8].astype(np.int64)) and np.array_equal(res.iterations, its)
            assert np.array_equal(res.is_null, core[:, 8] != 0) and res.row(int(np.nonzero(~res.is_null)[0][0])) is not None
            if slots is None:
                assert np.all(res.status[c.S:] == 100) and (res.status == 0).sum() >= 5
            for method, parse, m in ((pool.finalize_bls, pkg.parse_bls_options, bls_map), (pool.finalize_nnls, pkg.parse_nnls_options, bls_map)):
                bres, bunref = method(m, slots=slots)
                rec, bits, bu = pool.state.finalize_bls(parse(m).batch_options(), slots=slots, n_slots=n)
                assert isinstance(bres, pkg.BlsFitAggResult) and np.array_equal(bres.keys, keys) and np.array_equal(bunref, bu)
                assert np.array_equal(bres.coefficients, rec[:, :3], equal_nan=True) and np.array_equal(bres.ssr, rec[:, 4], equal_nan=True)
                assert np.array_equal(bres.status, rec[:, 8].astype(np.int64)) and np.array_equal(bres.iterations, bits)
                assert np.array_equal(bres.at_lower_bound, rec[:, 9:12] != 0) and np.array_equal(bres.at_upper_bound, rec[:, 12:15] != 0)
                fitted = bres.status == 0
                lo = -0.25 if method == pool.finalize_bls else 0.0
                assert fitted.sum() >= 5 and np.nanmin(bres.coefficients[fitted]) >= lo - 1e-12
                if method == pool.finalize_nnls:             # the bound keys are ignored: no upper bound binds
                    assert not bres.at_upper_bound[fitted].any()
    finally:
        if pool.state is not None:
            pool.state.close()
