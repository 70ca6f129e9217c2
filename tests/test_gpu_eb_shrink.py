"""GPU tier of eb_shrink: the cases of tests/eb_shrink_cases.py through anofox_hip_eb_shrink_batch_{host,device} on both paths
against tests/eb_shrink_restate.py; the bytes across repeated calls, across the two entry forms and against the host build of
csrc/eb_shrink.h; the scalar symbol and the Python layer."""
import numpy as np
import pytest

import eb_shrink_cases as EC
from conftest import import_pkg
from test_eb_shrink_cpu import build_host

pytestmark = pytest.mark.gpu
CALLS = EC.calls()
IDS = [EC.call_id(c) for c in CALLS]
R = EC.R


@pytest.fixture(scope="module")
def eb():
    m = import_pkg("eb_shrink")
    yield m
    m.eb_shrink_test_hooks()


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host_eb(tmp_path_factory):
    return build_host(tmp_path_factory)


def options(eb, call):
    return eb.EbShrinkOptions(call["method"], call["tau_squared"])


def run_host(eb, ctx, call):
    out, summary = eb.eb_shrink_batch_host(call["offsets"], call["est"], call["se"], call["n_cols"], call["est_stride"], call["se_stride"],
                                           options(eb, call), n_items=call["n_items"], ctx=ctx)
    return out, summary


def run_device(eb, ctx, call):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out, summary = eb.eb_shrink_batch_device(ctx, t(call["offsets"]), t(call["est"]), t(call["se"]), call["n_cols"], call["est_stride"],
                                             call["se_stride"], options(eb, call), n_items=call["n_items"])
    torch.cuda.synchronize()
    return out.cpu().numpy(), summary.cpu().numpy()


def same_bytes(a, b):
    return all(np.array_equal(x.ravel(), np.asarray(y).ravel(), equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("c", CALLS, ids=IDS)
def test_both_paths_both_forms(eb, ctx, host_eb, c):
    """Each path against the restatement; host form == device form == a second call, byte for byte; the wavefront-per-set path
    == the host build of the header, bit for bit."""
    call = EC.make_call(*c)
    ref = EC.reference(call, c)
    for path, chunk in ((1, 0), (2, 0), (2, 7)):
        eb.eb_shrink_test_hooks(path, chunk, 0)
        got = run_host(eb, ctx, call)
        errs = {}
        n, left = EC.check(call, *got, ref, errs)
        print(EC.call_id(c), "path %d chunk %d: compared %d, left out %d" % (path, chunk, n, left), {k: "%.2e" % v for k, v in errs.items()})
        assert n >= 8 * c[1]
        assert same_bytes(got, run_device(eb, ctx, call)), "host and device forms differ"
        assert same_bytes(got, run_host(eb, ctx, call)), "a repeated call differs"
        if path == 1:
            assert same_bytes(got, host_eb(call, 1)), "the GPU and the host build of eb_shrink.h differ"
    eb.eb_shrink_test_hooks()


@pytest.mark.parametrize("c", EC.wide_calls(), ids=[EC.call_id(c) for c in EC.wide_calls()])
def test_raw_wide_se_draw(eb, ctx, host_eb, c):
    """se log-uniform over 1e-3 .. 1e3 per pair (weights up to 12 decades apart within a set) on both paths: check_wide's
    condition-aware bounds, the bytes of the two forms, and the host build bit for bit on the wavefront-per-set path."""
    call = EC.make_call(*c)
    ref = EC.reference(call, c)
    for path, chunk in ((1, 0), (2, 0), (2, 7)):
        eb.eb_shrink_test_hooks(path, chunk, 0)
        got = run_host(eb, ctx, call)
        errs = {}
        assert EC.check_wide(call, *got, ref, errs) >= 8 * c[1]
        print(EC.call_id(c), "path %d chunk %d" % (path, chunk), {k: "%.2e" % v for k, v in errs.items()})
        assert same_bytes(got, run_device(eb, ctx, call))
        if path == 1:
            assert same_bytes(got, host_eb(call, 1))
    eb.eb_shrink_test_hooks()


@pytest.mark.parametrize("n_cols", [1, 9])
@pytest.mark.parametrize("chunk", [64, 100])
def test_chunk_seams(eb, ctx, n_cols, chunk):
    """One set of 1000 items in chunks of 64 and of 100: seams inside the set and at its end."""
    call = EC.chunk_call(n_cols, 7)
    eb.eb_shrink_test_hooks(2, chunk, 0)
    got = run_host(eb, ctx, call)
    assert EC.check(call, *got, EC.reference(call, ("chunk", n_cols)), {})[0] == n_cols
    assert same_bytes(got, run_device(eb, ctx, call)) and same_bytes(got, run_device(eb, ctx, call))
    eb.eb_shrink_test_hooks()


def test_stride_loop_and_the_library_s_own_choice(eb, ctx, host_eb):
    """7 sets on 2 workgroups (both paths), then no hook at all: the bytes do not depend on the grid."""
    call = EC.stride_loop_call(3)
    ref = EC.reference(call)
    for path, chunk in ((1, 0), (2, 16)):
        eb.eb_shrink_test_hooks(path, chunk, 0)
        free = run_host(eb, ctx, call)
        eb.eb_shrink_test_hooks(path, chunk, 2)
        strided = run_device(eb, ctx, call)
        EC.check(call, *strided, ref, {})
        assert same_bytes(free, strided)
    eb.eb_shrink_test_hooks()
    assert same_bytes(run_host(eb, ctx, call), host_eb(call, 1))      # small sets: one wavefront per set
    args = (call["offsets"], call["est"], call["se"], call["n_cols"], call["est_stride"], call["se_stride"])
    assert same_bytes(run_host(eb, ctx, call), ctx.eb_shrink_batch_host(*args, n_items=call["n_items"]))   # the Context's methods
    import torch
    dev = ctx.eb_shrink_batch_device(*[torch.from_numpy(a).cuda() for a in args[:3]], *args[3:], n_items=call["n_items"])
    torch.cuda.synchronize()
    assert same_bytes(run_host(eb, ctx, call), [t.cpu().numpy() for t in dev])
    big = EC.chunk_call(1, 9, m=5000)                                # one set of 5000 items: the chunk path by the library's rule
    got = run_host(eb, ctx, big)
    EC.check(big, *got, EC.reference(big), {})
    eb.eb_shrink_test_hooks(2, 0, 0)
    assert same_bytes(got, run_host(eb, ctx, big))
    eb.eb_shrink_test_hooks()


def test_wide_calls_go_by_column_blocks(eb, ctx):
    call = EC.make_call("heterogeneous", 70, "loose", 11, sizes=(3, 40, 0, 65), sparse=False)
    ref = EC.reference(call)
    for path, chunk in ((1, 0), (2, 16)):
        eb.eb_shrink_test_hooks(path, chunk, 0)
        EC.check(call, *run_device(eb, ctx, call), ref, {})
    eb.eb_shrink_test_hooks()


@pytest.mark.parametrize("kw", [dict(method=R.NONE), dict(tau_squared=0.04), dict(tau_squared=0.0), dict(tau_squared=-1.0),
                                dict(tau_squared=float("inf")), dict(method=5)])
def test_options_statuses_and_nan_placement(eb, ctx, kw):
    call = EC.make_call("heterogeneous", 2, "glm", 5, **kw)
    ref = EC.reference(call)
    for path, chunk in ((1, 0), (2, 50)):
        eb.eb_shrink_test_hooks(path, chunk, 0)
        out, summary = run_host(eb, ctx, call)
        EC.check(call, out, summary, ref, {})
        if R.options_invalid(call["method"], call["tau_squared"]):
            assert np.all(summary[..., 7] == 1) and np.all(np.isnan(out))
    eb.eb_shrink_test_hooks()


def test_items_outside_every_set_are_left_alone(eb, ctx):
    call = EC.make_call("heterogeneous", 2, "tight", 21, sizes=(5, 9), sparse=False)
    off = call["offsets"] + 3                      # items 0..2 and 17..19 belong to no set
    pad = lambda a, k: np.concatenate([np.full(3 * k, 1.0), a, np.full(3 * k, 1.0)])
    out, summary = eb.eb_shrink_batch_host(off, pad(call["est"], 2), pad(call["se"], 2), 2, n_items=20, ctx=ctx)
    rout, rsum, _ = EC.reference(call)
    assert np.all(np.isnan(out[:3])) and np.all(np.isnan(out[17:]))
    assert np.allclose(out[3:17], rout, rtol=1e-11, atol=0, equal_nan=True) and np.allclose(summary, rsum, rtol=1e-11, atol=0)


def test_scalar_entry_equals_the_batch_entry(eb, ctx):
    pkg = import_pkg()
    rng = np.random.default_rng(31)
    call = {"se": rng.uniform(0.1, 0.5, 40)}
    call["est"] = 0.5 + rng.normal(0, 0.3, 40) + call["se"] * rng.normal(0, 1, 40)
    est = [None if i == 7 else float(v) for i, v in enumerate(call["est"])]
    e = np.array([np.nan if v is None else v for v in est])
    out, summary = eb.eb_shrink_batch_host([0, 40], e, call["se"], ctx=ctx)
    d = pkg.eb_shrink(est, call["se"].tolist())
    assert [d[k] for k in ("mu", "mu_se", "tau_squared", "i_squared", "q", "n_groups")] == summary[0, 0, :6].tolist()
    got = np.array([[r["shrunken"], r["shrunken_se"], r["weight"]] for r in d["shrunken"]])
    assert np.array_equal(got, out[:, 0], equal_nan=True) and np.isnan(got[7]).all() and len(d["shrunken"]) == 40
    assert np.array_equal([r["se"] for r in d["shrunken"]], call["se"])
    with pytest.raises(pkg.InvalidInputException, match="Insufficient data") as failed:
        pkg.eb_shrink([0.5, None], [0.2, 0.2])
    assert failed.value.code == 6
    agg = pkg.eb_shrink_agg(["a"] * 40 + ["b", "b", "c"], est + [0.1, None, 0.3], call["se"].tolist() + [0.2, 0.2, 0.1], context=ctx)
    assert agg["b"] is None and agg["c"] is None and len(agg["a"]["shrunken"]) == 39
    keep = np.arange(40) != 7
    want = pkg.eb_shrink(e[keep].tolist(), call["se"][keep].tolist())
    assert agg["a"] == want


def test_shrink_coefficients_on_a_poisson_fit(eb, ctx):
    """40 groups, p = 3, inference on: the strided call on the result's own arrays == the batch entry on the columns copied out by
    numpy."""
    pkg = import_pkg()
    rng = np.random.default_rng(5)
    G, n, p = 40, 60, 3
    keys = np.repeat(np.arange(G), n)
    x = rng.normal(0, 0.5, (G * n, p))
    beta = 0.3 + rng.normal(0, 0.2, (G, p))
    y = rng.poisson(np.exp(0.5 + np.einsum("ij,ij->i", x, beta[keys]))).astype(float)
    fit = pkg.poisson_fit_agg(keys, y, x, {"compute_inference": True}, context=ctx)
    assert np.all(fit.status == 0)
    by = np.arange(G) % 3
    for groups in (None, by):
        res = pkg.shrink_coefficients(fit, by=groups, context=ctx)
        sets = [np.arange(G)] if groups is None else [np.flatnonzero(by == k) for k in range(3)]
        for s, g in enumerate(sets):
            # the coefficient and standard-error columns copied out as tight [len(g), p] matrices: the same lanes, the same bytes
            out, summary = eb.eb_shrink_batch_host([0, len(g)], fit.records[g, :p].copy(), fit.inference[g, :p].copy(), n_cols=p, ctx=ctx)
            assert np.array_equal(summary[0], res.summary[s])
            assert np.array_equal(out[..., 0], res.shrunken[g]) and np.array_equal(out[..., 1], res.shrunken_se[g])
            assert np.array_equal(out[..., 2], res.weight[g])
            for j in range(p):   # and one column at a time as a vector call: other lanes add the sums, so to rounding
                out, summary = eb.eb_shrink_batch_host([0, len(g)], fit.records[g, j].copy(), fit.inference[g, j].copy(), ctx=ctx)
                assert np.allclose(summary[0, 0], res.summary[s, j], rtol=1e-11, atol=0)
                assert np.allclose(out[:, 0], np.stack([res.shrunken[g, j], res.shrunken_se[g, j], res.weight[g, j]], 1), rtol=1e-11, atol=0)
        assert res.shrunken.shape == (G, p) and np.all(res.summary[..., 7] == 0) and res.set_summary(0, 0)["n_groups"] == len(sets[0])
    with pytest.raises(pkg.InvalidInputException, match="standard errors"):
        pkg.shrink_coefficients(pkg.poisson_fit_agg(keys, y, x, None, context=ctx))
