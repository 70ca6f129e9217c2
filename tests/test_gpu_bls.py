"""Grouped bounded / non-negative least squares on the MI355X: the records of anofox_hip_bls_fit_batch_* against the row-based
restatement (tests/bls_restate.py) in every size class, with the conditions on generated inputs asserted for every case;
constant columns, non-finite rows, the shortcut, the statuses, exact fits, inactive bounds = OLS, a box that binds every
coefficient, several slabs, row-split groups, determinism, the fit-predict entry point and the reference-compatible C
symbols.

Tolerances (tests/conftest.py's rules, applied by bls_restate.assert_record_matches): coefficients within
1e-9 max(|ref_j|, 1e-3 max_k |ref_k|), the intercept with its sum |xbar_j| tol_j allowance, ssr and r2 within 1e-6 relative /
1e-12 absolute, flags, n_active_constraints, n_observations and statuses exactly."""
import ctypes as C

import numpy as np
import pytest

import bls_restate as br
from conftest import import_pkg

pytestmark = pytest.mark.gpu

# every size class of the batch path: <= 8 (lane per group), 9..26, 27..42, 43..64, 65..128 (the accumulate kernels differ)
WIDTHS = [1, 2, 3, 5, 8, 9, 16, 26, 27, 33, 42, 43, 64, 65, 100, 128]


def _variants(rng, p):
    return [
        ("nnls", None, None),
        ("lower", -0.5, None),
        ("upper", None, 0.25),
        ("box", -1.0, 1.5),
        ("per_column", rng.uniform(-2.0, -0.1, size=p), rng.uniform(0.1, 2.0, size=p)),
    ]


def _batch(groups):
    off = np.concatenate([[0], np.cumsum([len(y) for y, _ in groups])]).astype(np.int64)
    y = np.concatenate([g[0] for g in groups])
    X = np.concatenate([g[1] for g in groups], axis=0)
    return off, y, X


def _fit(pkg, off, y, X, **kw):
    o = pkg.BlsOptions(**kw)
    return pkg.bls_fit_batch_host(off, y, [np.ascontiguousarray(X[:, j]) for j in range(X.shape[1])], o.batch_options())


def _check(pkg, groups, what, **kw):
    """Fit the groups as one batch and compare every record with the restatement."""
    off, y, X = _batch(groups)
    p = X.shape[1]
    rec, its = _fit(pkg, off, y, X, **kw)
    icpt = kw.get("fit_intercept", False)
    for g, (yg, Xg) in enumerate(groups):
        res = br.fit_bls(yg, Xg, icpt, kw.get("lower_bound"), kw.get("upper_bound"), kw.get("max_iterations", 1000),
                         kw.get("tolerance", 1e-10))
        if res["status"] == 0:
            assert br.input_conditions(res, yg, Xg, icpt, kw.get("tolerance", 1e-10)) == [], f"{what} group {g}"
        xbar = None
        if res["status"] == 0:
            xbar = np.nanmean(np.where(res["valid"][:, None], Xg, np.nan), axis=0)
        br.assert_record_matches(rec[g], br.record(res), p, xbar=xbar, what=f"{what} group {g}")
        if res["status"] == 0:
            assert its[g] >= 0, f"{what} group {g}: the iteration limit stopped the solve"
    return rec, its


@pytest.mark.parametrize("p", WIDTHS)
def test_against_restatement(p):
    pkg = import_pkg()
    rng = np.random.default_rng(1000 + p)
    G = 4 if p <= 64 else 2
    groups = [br.make_case(rng, int(rng.integers(p + 2, 3 * p + 41)), p) for _ in range(G)]
    n_bound = 0
    for name, lo, hi in _variants(rng, p):
        for icpt in (False, True):
            rec, its = _check(pkg, groups, f"p={p} {name} intercept={icpt}", fit_intercept=icpt, lower_bound=lo, upper_bound=hi)
            n_bound += int(rec[:, p + 4].sum())
            assert np.abs(its).max() <= 8 * p + 64
    assert n_bound > 0


@pytest.mark.parametrize("p", [3, 8, 12, 40, 70])
def test_constant_columns_and_non_finite_rows(p):
    pkg = import_pkg()
    rng = np.random.default_rng(2000 + p)
    groups = []
    for g in range(4):
        y, X = br.make_case(rng, 3 * p + 30, p)
        X[:, g % p] = 2.5                               # a constant column
        if p > 4:
            X[:, (g + 2) % p] = 0.0
        y[1] = np.nan
        X[2, (g + 1) % p] = np.inf
        X[5, 0] = np.nan
        y[7] = -np.inf
        groups.append((y, X))
    for icpt in (False, True):
        _check(pkg, groups, f"p={p} constant/non-finite intercept={icpt}", fit_intercept=icpt)
        _check(pkg, groups, f"p={p} constant/non-finite box intercept={icpt}", fit_intercept=icpt, lower_bound=-1.0, upper_bound=1.5)


@pytest.mark.parametrize("p", [2, 8, 9, 33, 128])
def test_statuses_and_shortcut(p):
    pkg = import_pkg()
    rng = np.random.default_rng(3000 + p)
    good = br.make_case(rng, 2 * p + 20, p)
    one_row = (good[0][:1].copy(), good[1][:1].copy())                      # status 100
    no_valid = (np.full(p + 5, np.nan), good[1][:p + 5].copy())             # status 10
    all_const = (good[0][:p + 5].copy(), np.full((p + 5, p), 3.0))          # status 6 without, shortcut with an intercept
    exactly_p = (good[0][:p].copy(), good[1][:p].copy())                    # n = p: allowed without, status 6 with an intercept
    groups = [good, one_row, no_valid, all_const, good]
    rec, _ = _check(pkg, groups, f"p={p} statuses", fit_intercept=False)
    assert list(rec[:, p + 5]) == [0, 100, 10, 6, 0]
    rec, _ = _check(pkg, groups + [exactly_p], f"p={p} statuses (intercept)", fit_intercept=True)
    assert list(rec[:, p + 5]) == [0, 100, 10, 0, 0, 6]
    assert np.isnan(rec[3, p + 1]) and rec[3, p + 2] == 0.0 and rec[3, p + 4] == 0.0 and np.isnan(rec[3, :p]).all()
    assert np.array_equal(rec[3, p + 6:], np.zeros(2 * p))
    # unusable bounds: every group of the call has status 1 (status 100 keeps its precedence)
    for lo, hi in (([0.0] * (p + 1), None), (2.0, 1.0), (np.nan, None), (None, [1.0] * (p + 2))):
        rec, _ = _check(pkg, groups, f"p={p} invalid bounds", lower_bound=lo, upper_bound=hi)
        assert list(rec[:, p + 5]) == [1, 100, 1, 1, 1]
        assert np.isnan(np.delete(rec, p + 5, axis=1)).all()


@pytest.mark.parametrize("p", [1, 8, 9, 64, 65, 128])
def test_five_kinds_of_group_at_the_path_boundaries(p):
    """Both ends of the narrow path, the first wide width and both sides of the wide kernel's one / two columns per lane: a plain
    group of 2p + 3 rows, an exact fit inside the box (the moment ssr cancels: the rows give it), every column constant (the
    shortcut), p rows (status 6) and an empty group (status 100), against the restatement, twice with identical bytes."""
    pkg = import_pkg()
    rng = np.random.default_rng(4500 + p)
    plain = br.make_case(rng, 2 * p + 3, p)
    _, Xe = br.make_case(rng, 2 * p + 25, p)
    exact = (Xe @ rng.uniform(0.5, 2.0, size=p) + 4.0, Xe)
    groups = [plain, exact, (plain[0].copy(), np.full((2 * p + 3, p), 3.0)), (plain[0][:p].copy(), plain[1][:p].copy()),
              (np.zeros(0), np.zeros((0, p)))]
    kw = dict(fit_intercept=True, lower_bound=0.0, upper_bound=3.0)
    rec, its = _check(pkg, groups, f"p={p} five kinds", **kw)
    assert list(rec[:, p + 5]) == [0, 0, 0, 6 if p > 1 else 100, 100]    # (p = 1: the group of p rows has fewer than 2)
    assert rec[1, p + 4] == 0 and np.isnan(rec[2, :p]).all()    # (the exact fit lies inside the box: no active bound)
    rec2, its2 = _fit(pkg, *_batch(groups), **kw)
    assert rec.tobytes() == rec2.tobytes() and its.tobytes() == its2.tobytes()


@pytest.mark.parametrize("p", [3, 8, 20, 64])
def test_exact_fits_take_ssr_from_the_rows(p):
    """y = X beta exactly with beta inside the box: the moment ssr cancels, the rows give it (1e-12 absolute)."""
    pkg = import_pkg()
    rng = np.random.default_rng(4000 + p)
    groups = []
    for _ in range(3):
        _, X = br.make_case(rng, 2 * p + 25, p)
        beta = rng.uniform(0.5, 2.0, size=p)
        groups.append((X @ beta, X))
    rec, _ = _check(pkg, groups, f"p={p} exact NNLS")
    assert (rec[:, p + 1] < 1e-12).all() and (rec[:, p + 4] == 0).all()
    for g in range(3):
        groups[g] = (groups[g][0] + 4.0, groups[g][1])
    _check(pkg, groups, f"p={p} exact with intercept", fit_intercept=True, lower_bound=0.0, upper_bound=3.0)


def test_pivot_case_of_the_reference():
    """test/sql/regression/test_bls_nnls_pivot.test: [7, 2, 0.5] to three decimals through NNLS and default BLS."""
    pkg = import_pkg()
    y, X = br.pivot_table()
    rec, _ = _fit(pkg, np.array([0, 12], dtype=np.int64), y, X)
    assert np.array_equal(np.round(rec[0, :3], 3), [7.0, 2.0, 0.5])           # what the reference asserts
    assert rec[0, 3 + 5] == 0 and rec[0, 3 + 4] == 0 and rec[0, 3 + 1] < 1e-12 * float(y @ y)
    r = pkg.nnls_fit_agg(np.zeros(12, dtype=np.int64), y, X)
    assert np.array_equal(np.round(r.coefficients[0], 3), [7.0, 2.0, 0.5]) and r.row(0)["n_active_constraints"] == 0
    r = pkg.bls_fit_agg(np.zeros(12, dtype=np.int64), y, X, {"lower": 0.0})
    assert np.array_equal(np.round(r.coefficients[0], 3), [7.0, 2.0, 0.5])


@pytest.mark.parametrize("p", [4, 8, 12, 30, 50, 96])
def test_inactive_bounds_are_the_ols_record(p):
    pkg = import_pkg()
    rng = np.random.default_rng(5000 + p)
    groups = [br.make_case(rng, 3 * p + 30, p) for _ in range(3)]
    off, y, X = _batch(groups)
    cols = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    for icpt in (False, True):
        rec, _ = _check(pkg, groups, f"p={p} wide box", fit_intercept=icpt, lower_bound=-1e3, upper_bound=1e3)
        core, _ = pkg.fit_batch_host(off, y, cols, None, pkg.RegressionOptions(fit_intercept=icpt).batch_options("ols"))
        scale = np.max(np.abs(core[:, :p]), axis=1, keepdims=True)
        assert (np.abs(rec[:, :p] - core[:, :p]) <= 1e-9 * np.maximum(np.abs(core[:, :p]), 1e-3 * scale)).all()
        assert np.allclose(rec[:, p + 2], core[:, p + 1], rtol=1e-6, atol=1e-12)            # r2
        assert (rec[:, p + 4] == 0).all() and (rec[:, p + 6:] == 0).all()


@pytest.mark.parametrize("p", [5, 8, 17, 64, 128])
def test_tight_box_binds_every_coefficient(p):
    pkg = import_pkg()
    rng = np.random.default_rng(6000 + p)
    groups = [br.make_case(rng, 2 * p + 30, p) for _ in range(2)]
    for icpt in (False, True):
        rec, its = _check(pkg, groups, f"p={p} tight box", fit_intercept=icpt, lower_bound=100.0, upper_bound=100.001)
        assert (rec[:, p + 4] == p).all()
        assert np.isin(rec[:, :p], [100.0, 100.001]).all()                                    # exactly the bounds
        assert ((rec[:, p + 6:2 * p + 6] + rec[:, 2 * p + 6:]) == 1.0).all()


@pytest.mark.parametrize("p", [3, 12])
def test_row_split_group(p):
    """A group long enough to be cut into row segments by the accumulate kernels (more than 8192 rows)."""
    pkg = import_pkg()
    rng = np.random.default_rng(7000 + p)
    groups = [br.make_case(rng, 40, p), br.make_case(rng, 30000, p), br.make_case(rng, 50, p)]
    for icpt in (False, True):
        _check(pkg, groups, f"p={p} row split intercept={icpt}", fit_intercept=icpt)
        _check(pkg, groups, f"p={p} row split box intercept={icpt}", fit_intercept=icpt, lower_bound=-0.3, upper_bound=0.4)


def test_several_slabs_at_one_wide_width():
    """p = 128: 13 785 groups fill a slab of moment records; three slabs of a tiled batch.  Groups at both ends and across
    the slab boundaries against the restatement, every tile bit-identical to the first."""
    pkg = import_pkg()
    p, n, tile = 128, 132, 64
    T = (p + 15) // 16
    slab = max(256, (1 << 30) // ((T * (T + 1) // 2 * 256 + 4 * 16 * T + 8) * 8))
    reps = (2 * slab + 700) // tile + 1
    rng = np.random.default_rng(8128)
    base = [br.make_case(rng, n, p) for _ in range(tile)]
    off1, y1, X1 = _batch(base)
    G = tile * reps
    off = np.arange(G + 1, dtype=np.int64) * n
    y = np.tile(y1, reps)
    cols = [np.tile(np.ascontiguousarray(X1[:, j]), reps) for j in range(p)]
    rec, its = pkg.bls_fit_batch_host(off, y, cols, pkg.BlsOptions().batch_options())
    assert G > 2 * slab
    first = rec[:tile]
    for k in range(1, reps):
        assert np.array_equal(rec[k * tile:(k + 1) * tile], first, equal_nan=True), f"tile {k} differs from tile 0"
        assert np.array_equal(its[k * tile:(k + 1) * tile], its[:tile])
    for g in (0, 1, slab % tile, (slab - 1) % tile, (2 * slab) % tile, (G - 1) % tile):
        yg, Xg = base[g]
        res = br.fit_bls(yg, Xg)
        assert br.input_conditions(res, yg, Xg, False) == []
        br.assert_record_matches(rec[g], br.record(res), p, what=f"slab test, base group {g}")


@pytest.mark.parametrize("p", [6, 48])
def test_two_calls_are_bit_identical(p):
    pkg = import_pkg()
    rng = np.random.default_rng(9000 + p)
    groups = [br.make_case(rng, 3 * p + 20, p) for _ in range(40)]
    off, y, X = _batch(groups)
    a, ia = _fit(pkg, off, y, X, fit_intercept=True, lower_bound=-1.0, upper_bound=1.5)
    b, ib = _fit(pkg, off, y, X, fit_intercept=True, lower_bound=-1.0, upper_bound=1.5)
    assert a.tobytes() == b.tobytes() and ia.tobytes() == ib.tobytes()


def test_iteration_limit_returns_a_feasible_iterate():
    pkg = import_pkg()
    rng = np.random.default_rng(31)
    p = 10
    groups = [br.make_case(rng, 60, p) for _ in range(3)]
    off, y, X = _batch(groups)
    rec, its = _fit(pkg, off, y, X, max_iterations=1)
    assert (rec[:, p + 5] == 0).all() and (its == -1).all()
    assert (rec[:, :p] >= 0.0).all()
    full, its_full = _fit(pkg, off, y, X)
    assert (its_full > 1).all() and (full[:, p + 1] < rec[:, p + 1]).all()    # the full solve reaches a smaller ssr


def test_device_entry_point_matches_host():
    import torch
    pkg = import_pkg()
    rng = np.random.default_rng(77)
    for p in (4, 20):
        groups = [br.make_case(rng, 3 * p + 20, p) for _ in range(5)]
        off, y, X = _batch(groups)
        host, ih = _fit(pkg, off, y, X, lower_bound=-0.5, upper_bound=0.7, fit_intercept=True)
        ctx = pkg.Context(0)
        o = pkg.BlsOptions(lower_bound=-0.5, upper_bound=0.7, fit_intercept=True).batch_options()
        dev, idv = ctx.bls_fit_batch_device(torch.from_numpy(off).cuda(), torch.from_numpy(y).cuda(),
                                            [torch.from_numpy(np.ascontiguousarray(X[:, j])).cuda() for j in range(p)], o)
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), host, equal_nan=True) and np.array_equal(idv.cpu().numpy(), ih)
        ctx.close()


def _coef_close(got, ref):
    """The project's coefficient rule: |got - ref| <= 1e-9 max(|ref_j|, 1e-3 max_k |ref_k|)."""
    tol = 1e-9 * np.maximum(np.abs(ref), 1e-3 * np.nanmax(np.abs(ref)))
    assert (np.abs(got - ref) <= tol).all(), np.max(np.abs(got - ref) / tol)


def test_records_satisfy_kkt_from_the_rows():
    """Independent of the restatement's recipe: the GPU's coefficients are feasible and their multipliers x_j'r, computed here
    from the rows, have the sign the bound they sit on requires (free: ~0), at 1e-7 ||x_j|| ||y||."""
    pkg = import_pkg()
    rng = np.random.default_rng(99)
    for p in (4, 8, 20, 70):
        groups = [br.make_case(rng, 3 * p + 30, p) for _ in range(4)]
        off, y, X = _batch(groups)
        for icpt, lo, hi in ((False, None, None), (True, -1.0, 1.5), (False, None, 0.25)):
            rec, _ = _fit(pkg, off, y, X, fit_intercept=icpt, lower_bound=lo, upper_bound=hi)
            lo_v, hi_v = br.resolve_bounds(p, lo, hi)
            for g, (yg, Xg) in enumerate(groups):
                b = rec[g, :p]
                assert (b >= lo_v).all() and (b <= hi_v).all()
                r = yg - (rec[g, p] if icpt else 0.0) - Xg @ b
                gr = Xg.T @ r / (np.linalg.norm(Xg, axis=0) * np.linalg.norm(yg))
                at_lo, at_hi = b == lo_v, b == hi_v
                assert (np.abs(gr[~at_lo & ~at_hi]) <= 1e-7).all()
                assert (gr[at_lo] <= 1e-7).all() and (gr[at_hi] >= -1e-7).all()
                if icpt:
                    assert abs(r.sum()) <= 1e-7 * np.linalg.norm(yg) * np.sqrt(len(yg))


def _t_margin(sigma, n, p, has_icpt, conf):
    from scipy import stats as sps
    if np.isnan(sigma) or sigma <= 0.0 or n <= p + 1:
        return 0.0
    df = n - p - (1 if has_icpt else 0)
    if df <= 0:
        return 0.0
    return sps.t.ppf(0.5 * (1.0 + conf), df) * sigma * np.sqrt(1.0 + 1.0 / n)


@pytest.mark.parametrize("p", [3, 11])
def test_fit_predict_against_restatement_and_the_predict_formula(p):
    """Training rows fit, every row predicted: yhat at 1e-8, bounds at 1e-6 (the window tests' figures); sigma with the
    reference's unsigned df over all columns; a group with constant columns and few rows shows the wrap (sigma ~ 0)."""
    pkg = import_pkg()
    rng = np.random.default_rng(40 + p)
    groups = [br.make_case(rng, 3 * p + 25, p) for _ in range(3)]
    yq, Xq = br.make_case(rng, p, p)           # the quirk: p - 1 constant columns and n = p rows, so n - p - 1 wraps
    Xq[:, 1:] = 1.5
    groups.append((yq, Xq))
    off, y, X = _batch(groups)
    y_fit = y.copy()
    hold = np.zeros(len(y), dtype=bool)
    for g in range(3):
        hold[off[g + 1] - 5:off[g + 1]] = True          # the last five rows of a group are predicted only
    y_fit[hold] = np.nan
    counts = np.array([int((~hold[off[g]:off[g + 1]]).sum()) for g in range(4)], dtype=np.int64)
    cols = [np.ascontiguousarray(X[:, j]) for j in range(p)]
    for icpt, conf in ((False, 0.95), (True, 0.9)):
        o = pkg.BlsOptions(fit_intercept=icpt, lower_bound=-0.5, upper_bound=0.8)
        core, pred = pkg.bls_fit_predict_batch_host(off, y_fit, cols, o.batch_options(), conf, train_counts=counts)
        for g in range(4):
            sl = slice(off[g], off[g + 1])
            res = br.fit_bls(y_fit[sl], X[sl], icpt, -0.5, 0.8)
            assert core[g, p + 5] == res["status"] == 0
            if g < 3:       # (group 3 is the constructed unsigned-df case, not a generated one)
                assert br.input_conditions(res, y_fit[sl], X[sl], icpt) == []
            b = np.where(np.isnan(res["coefficients"]), 0.0, res["coefficients"])
            yhat = (res["intercept"] if icpt else 0.0) + X[sl] @ b
            n = res["n_observations"]
            df = (n - p - (1 if icpt else 0)) % (1 << 64)                         # unsigned 64-bit, all columns
            sigma = np.sqrt(res["ssr"] / df) if df > 0 and res["ssr"] >= 0 else np.nan
            margin = _t_margin(sigma, n, p, icpt, conf)
            scale = np.maximum(np.abs(yhat), 1.0)
            assert (np.abs(pred[sl, 0] - yhat) <= 1e-8 * scale).all()
            assert (np.abs(pred[sl, 1] - (yhat - margin)) <= 1e-6 * scale).all()
            assert (np.abs(pred[sl, 2] - (yhat + margin)) <= 1e-6 * scale).all()
            assert abs(core[g, p + 2] - res["ssr"]) <= 1e-6 * res["ssr"] + 1e-12
            if g == 3 and icpt:
                assert df > (1 << 62) and core[g, p + 3] < 1e-6      # wrapped df: sigma ~ 0, bounds = yhat
    # the aggregate: NULL lists for a group with fewer than two training rows, is_training flags, list lengths
    keys = np.repeat(np.arange(4), np.diff(off))
    keys = np.concatenate([keys, [9, 9]])
    ya = np.concatenate([np.where(hold, np.nan, y), [1.0, np.nan]])
    Xa = np.concatenate([X, X[:2]], axis=0)
    r = pkg.bls_fit_predict_agg(keys, [None if np.isnan(v) else float(v) for v in ya], Xa.tolist(), {"lower": -0.5, "upper": 0.8})
    assert list(r.is_null) == [False, False, False, False, True]
    rows = r.rows(0)
    assert len(rows) == off[1] - off[0] and sum(x["is_training"] for x in rows) == counts[0]
    assert all(x["yhat_lower"] <= x["yhat"] <= x["yhat_upper"] for x in rows) and r.rows(4) is None


def _data_array(abi, v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    return abi.AnofoxDataArray(v.ctypes.data_as(C.POINTER(C.c_double)), None, len(v)), v


def test_c_symbols():
    """anofox_bls_fit / anofox_nnls_fit / anofox_free_bls_result: results against the restatement, the NULL conventions of
    the reference's FFI (out_result NULL, x NULL or empty -> InvalidInput, nothing allocated), errors with its texts."""
    pkg = import_pkg()
    abi = import_pkg("_abi")
    lib = abi.load()
    rng = np.random.default_rng(5)
    p = 5
    y, X = br.make_case(rng, 50, p)
    ya, _keep_y = _data_array(abi, y)
    keep = [_data_array(abi, X[:, j]) for j in range(p)]
    xs = (abi.AnofoxDataArray * p)(*[k[0] for k in keep])
    err = abi.AnofoxError()
    out = abi.AnofoxBlsFitResultCore()
    assert lib.anofox_nnls_fit(ya, xs, p, C.byref(out), C.byref(err)), err.text()
    res = br.fit_bls(y, X)
    got = np.array([out.coefficients[j] for j in range(p)])
    assert (np.abs(got - res["coefficients"]) <= 1e-9 * np.maximum(np.abs(res["coefficients"]), 1e-3 * np.abs(res["coefficients"]).max())).all()
    assert np.isnan(out.intercept) and out.n_observations == 50 and out.n_features == p and out.coefficients_len == p
    assert out.n_active_constraints == res["n_active_constraints"]
    assert [bool(out.at_lower_bound[j]) for j in range(p)] == list(res["at_lower_bound"])
    assert not any(out.at_upper_bound[j] for j in range(p))
    assert br.input_conditions(res, y, X, False) == []
    assert abs(out.ssr - res["ssr"]) <= 1e-6 * res["ssr"] + 1e-12
    assert abs(out.r_squared - res["r_squared"]) <= 1e-6 * abs(res["r_squared"]) + 1e-12
    lib.anofox_free_bls_result(C.byref(out))
    assert not out.coefficients and not out.at_lower_bound and not out.at_upper_bound
    lib.anofox_free_bls_result(C.byref(out))                      # twice: nothing left to free
    lib.anofox_free_bls_result(None)

    o = pkg.BlsOptions(fit_intercept=True, lower_bound=-0.2, upper_bound=[0.1, 0.2, 0.3, 0.4, 0.5]).ffi_options()
    assert lib.anofox_bls_fit(ya, xs, p, o, C.byref(out), C.byref(err)), err.text()
    res = br.fit_bls(y, X, True, -0.2, [0.1, 0.2, 0.3, 0.4, 0.5])
    got = np.array([out.coefficients[j] for j in range(p)])
    assert (np.abs(got - res["coefficients"]) <= 1e-9 * np.maximum(np.abs(res["coefficients"]), 1e-3 * np.abs(res["coefficients"]).max())).all()
    assert [bool(out.at_upper_bound[j]) for j in range(p)] == list(res["at_upper_bound"])
    assert abs(out.intercept - res["intercept"]) <= 1e-8 * max(1.0, abs(res["intercept"]))
    lib.anofox_free_bls_result(C.byref(out))

    assert not lib.anofox_bls_fit(ya, xs, p, o, None, C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "out_result is NULL"
    fresh = abi.AnofoxBlsFitResultCore()
    assert not lib.anofox_bls_fit(ya, None, p, o, C.byref(fresh), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and err.text() == "x is NULL or empty" and not fresh.coefficients
    assert not lib.anofox_nnls_fit(ya, xs, 0, C.byref(fresh), C.byref(err)) and err.text() == "x is NULL or empty"
    assert lib.anofox_nnls_fit(ya, xs, p, C.byref(fresh), None)   # a NULL error pointer is accepted
    lib.anofox_free_bls_result(C.byref(fresh))
    bad = pkg.BlsOptions(lower_bound=[0.0, 1.0]).ffi_options()    # two bounds for five columns
    assert not lib.anofox_bls_fit(ya, xs, p, bad, C.byref(fresh), C.byref(err))
    assert err.code == abi.ERROR_INVALID_INPUT and not fresh.coefficients
    ynan, _k = _data_array(abi, np.full(50, np.nan))
    assert not lib.anofox_nnls_fit(ynan, xs, p, C.byref(fresh), C.byref(err))
    assert err.code == abi.ERROR_NO_VALID_DATA and err.text() == "All rows filtered due to NULL/NaN values"


def test_aggregates_group_by_with_combine():
    pkg = import_pkg()
    rng = np.random.default_rng(12)
    p = 4
    groups = [br.make_case(rng, 40 + 3 * g, p) for g in range(5)]
    off, y, X = _batch(groups)
    keys = np.repeat(np.arange(5), np.diff(off))
    perm = rng.permutation(len(y))
    opts = {"lower": -0.5, "upper": 0.6, "intercept": True}
    a = pkg.BlsFitAgg(opts).update(keys[perm[:70]], y[perm[:70]], X[perm[:70]])
    b = pkg.BlsFitAgg(opts).update(keys[perm[70:]], y[perm[70:]], X[perm[70:]])
    r = a.combine(b).finalize()
    for g in range(5):
        res = br.fit_bls(groups[g][0], groups[g][1], True, -0.5, 0.6)
        row = r.row(g)
        assert br.input_conditions(res, groups[g][0], groups[g][1], True) == []
        _coef_close(np.array(row["coefficients"], dtype=float), res["coefficients"])
        assert row["at_lower_bound"] == list(res["at_lower_bound"]) and row["at_upper_bound"] == list(res["at_upper_bound"])
        assert row["n_active_constraints"] == res["n_active_constraints"] and row["n_observations"] == len(groups[g][0])
    n = pkg.nnls_fit_agg(keys, y, X, {"lower": -5.0, "fit_intercept": False})       # the bound key is ignored
    for g in range(5):
        res = br.fit_bls(groups[g][0], groups[g][1])
        assert br.input_conditions(res, groups[g][0], groups[g][1], False) == []
        _coef_close(np.array(n.row(g)["coefficients"], dtype=float), res["coefficients"])
        assert n.row(g)["intercept"] is None
