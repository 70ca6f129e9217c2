"""GPU tier of the randomised sweep of the five test families on the size-tiered launch driver (csrc/rank_launch.h), on the cases of
tests/stat_fuzz_cases.py against the five restatements, with their check_records bounds unchanged:

    a  the seeded sweep: 12 seeds a family (times ANOFOX_FUZZ_SCALE), each at the default cap and at one drawn cap, the exact
       columns byte-equal between the two, the device entry byte-equal to the host entry
    b  the cap ladder: every cap of stat_fuzz_cases.CAPS on groups of c - 1, c, c + 1 and 2 c + 1 rows and the tier boundaries
    c  a workgroup's second and third group on the small path: 2 x 65536 + 97 groups tiled from a pool of 97
    d  the same on the large path: the cap hooked to 16, 2 x 1024 + 61 groups tiled from a shuffled pool of 61
    e  the sort's second trip: groups of 2048, 2049, 4096 and 4097 rows
    f  signed zeros, infinities, subnormals and an all-NaN group between full ones, stated directly on both paths

The exact columns are those of the per-family GPU tiers.  The categorical family has label columns: its special contents in f are
the extreme alphabet, scattered NULL rows and an all-NULL group, and it has no signed zeros.  Every test puts the family's hook back
to 0.  Nothing here asserts a time."""
import numpy as np
import pytest

import stat_fuzz_cases as fc
from conftest import import_pkg
from test_gpu_normality_tests import _EXACT as _NORMALITY_EXACT
from test_gpu_rank_tests import _exact_columns as _rank_exact
from test_gpu_sample_tests import _exact_columns as _sample_exact
from test_stat_fuzz_cpu import GPU_SEEDS, drawn_cap

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]
COR, RT, ST, NT, CT = fc.COR, fc.RT, fc.ST, fc.NT, fc.CT
LADDER_TEST, EVERY_STAGED, EVERY_TEST = fc.LADDER_TEST, fc.EVERY_STAGED, fc.EVERY_TEST
HOOK = {"cor": "cor_test_hooks", "rank": "rank_test_hooks", "sample": "sample_test_hooks", "normality": "normality_test_hooks",
        "categorical": "categorical_test_hooks"}


def exact_columns(family, test):
    if family == "cor":
        return [0, 5, 6, 7]                      # tests/test_gpu_cor.py: the estimate, n, s and the status
    if family == "rank":
        return _rank_exact(test)
    if family == "sample":
        return _sample_exact(test)
    return _NORMALITY_EXACT if family == "normality" else list(range(12))      # categorical: the whole record


@pytest.fixture(scope="module")
def refs():
    """key -> reference records: computed once, read by every test that asks for the key."""
    cache = {}

    def get(key, call):
        if key not in cache:
            cache[key] = fc.reference(call)
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.fixture()
def pkg():
    p = import_pkg()
    try:
        yield p
    finally:
        for name in HOOK.values():
            getattr(p, name)(0)


def _options(pkg, call):
    f, o = call["family"], call["opts"]
    if f == "cor":
        return pkg.CorrelationOptions(alternative=o.get("alternative", 0), confidence_level=o.get("confidence_level", 0.95),
                                      tau_type=o.get("tau_type", 1))
    if f == "rank":
        return pkg.RankTestOptions(alternative=o.get("alternative", 0), continuity_correction=o.get("correction", True), mu=o.get("mu", 0.0))
    if f == "sample":
        return pkg.SampleTestOptions(alternative=o.get("alternative", 0), kind=o.get("kind", 0), mu=o.get("mu", 0.0), trim=o.get("trim", 0.2),
                                     confidence_level=o.get("confidence_level", 0.95))
    if f == "categorical":
        return pkg.CategoricalTestOptions(correction=o.get("correction", False), alternative=o.get("alternative", 0),
                                          exact=o.get("exact", False), confidence_level=o.get("confidence_level", 0.95))
    return None


def _columns(call):
    """The call's columns in the order of its entry point (None: a column the test does not take)."""
    f, t = call["family"], call["test"]
    if f == "cor":
        return [call["x"], call["y"]]
    if f == "normality":
        return [call["v"]]
    if f == "categorical":
        return [call["a"], call["b"]]
    paired = t == RT.WILCOXON if f == "rank" else (t == ST.T_TEST and call["opts"].get("kind", 0) == ST.PAIRED)
    return [call["v"], call["y"], None] if paired else [call["v"], None, call["sample"]]


def run(pkg, call, cap=0, ctx=None, device=False):
    """The call's records at the hooked cap (0: the default), by the host entry or by the device entry on the same arrays."""
    f, t = call["family"], call["test"]
    getattr(pkg, HOOK[f])(cap)
    cols, tail = _columns(call), ([t] if f == "normality" else [t, _options(pkg, call)])
    if not device:
        entry = {"cor": pkg.cor_batch_host, "rank": pkg.rank_test_batch_host, "sample": pkg.sample_test_batch_host,
                 "normality": pkg.normality_test_batch_host, "categorical": pkg.categorical_test_batch_host}[f]
        return entry(call["off"], *cols, *tail, ctx=ctx)
    import torch
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()   # noqa: E731
    entry = {"cor": ctx.cor_batch_device, "rank": ctx.rank_test_batch_device, "sample": ctx.sample_test_batch_device,
             "normality": ctx.normality_test_batch_device, "categorical": ctx.categorical_test_batch_device}[f]
    rec = entry(dev(call["off"]), *[dev(c) for c in cols], *tail)
    torch.cuda.synchronize()
    return rec.cpu().numpy()


def _same_bytes(a, b, cols=None):
    a, b = (a, b) if cols is None else (a[:, cols], b[:, cols])
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _report(record_property, tier, call, errs):
    for k, e in errs.items():
        record_property("worst_" + k, float(e))
    print("FUZZ", tier, call["family"], call["test"], " ".join("%s=%.2e" % (k, e) for k, e in sorted(errs.items())))


# ---- a ----
@pytest.mark.parametrize("seed", GPU_SEEDS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_seeded_sweep(pkg, refs, family, seed, record_property):
    call = fc.case(family, seed)
    ref = refs(("a", family, seed), call)
    cols = exact_columns(family, call["test"])
    errs = {}
    ctx = pkg.Context(0)
    try:
        plain, hooked = run(pkg, call, 0, ctx), run(pkg, call, drawn_cap(family, seed), ctx)
        fc.check(call, plain, ref, errs)
        fc.check(call, hooked, ref, errs)
        assert _same_bytes(plain, hooked, cols)
        assert _same_bytes(run(pkg, call, 0, ctx, device=True), plain)
    finally:
        ctx.close()
    _report(record_property, "a", call, errs)


# ---- b ----
@pytest.mark.parametrize("cap", fc.CAPS)
@pytest.mark.parametrize("family", fc.FAMILIES)
def test_cap_ladder(pkg, refs, family, cap, record_property):
    test = LADDER_TEST[family]
    call = fc.ladder_call(family, cap)
    ref = refs(("b", family, cap), call)
    errs = {}
    plain, hooked = run(pkg, call, 0), run(pkg, call, cap)
    fc.check(call, plain, ref, errs)
    fc.check(call, hooked, ref, errs)
    assert _same_bytes(plain, hooked, exact_columns(family, test))
    _report(record_property, "b", call, errs)


# ---- c, d ----
def _tiled(pkg, refs, tier, tiled, cap, record_property):
    call, index, pool = tiled
    family, test, n_pool = call["family"], call["test"], len(pool["sizes"])
    ref = refs((tier, family, test), pool)
    got = run(pkg, call, cap)
    errs = fc.check(pool, got[:n_pool], ref)                      # every record is its pool member's: these, and the replicas below
    assert _same_bytes(got, got[:n_pool][index])                  # every replica: the bytes of the first occurrence, the whole record
    _report(record_property, tier, call, errs)
    return call, got


@pytest.mark.parametrize("family, test", fc.SMALL_TILED)
def test_second_and_third_group_of_a_small_workgroup(pkg, refs, family, test, record_property):
    """2 x 65536 + 97 groups of 0 to 40 rows, every kind, empty and all-NaN groups beside full ones: a workgroup of either small
    instance takes a second group, and the first 97 a third."""
    _tiled(pkg, refs, "c", fc.small_pool_call(family, test), 0, record_property)


@pytest.mark.parametrize("family, test", EVERY_STAGED)
def test_second_and_third_group_of_a_large_workgroup(pkg, refs, family, test, record_property):
    """The cap hooked to 16 and 2 x 1024 + 61 groups of 0 to 80 rows in shuffled order: a workgroup of the large kernel passes over
    groups of at most 16 rows and takes the others, a second and a third time (Kendall: some 1700 listed groups)."""
    call, got = _tiled(pkg, refs, "d", fc.large_pool_call(family, test), fc.LARGE_POOL_CAP, record_property)
    assert sum(n > 16 for n in call["sizes"][:fc.LARGE_POOL]) >= 20 and sum(n <= 16 for n in call["sizes"][:fc.LARGE_POOL]) >= 8
    assert _same_bytes(got, run(pkg, call, 0), exact_columns(family, test))


# ---- e ----
@pytest.mark.parametrize("family, test", EVERY_STAGED)
def test_second_trip_of_the_large_sort(pkg, refs, family, test, record_property):
    """Groups of 2048, 2049, 4096 and 4097 rows at the default cap: a pad of 2048 (one trip of the 1024 threads), 4096 (two) and
    8192 (four).  The 2048-row groups also alone with the cap hooked to 1024: the exact columns do not change."""
    call = fc.stride_call(family, test)
    ref = refs(("e", family, test), call)
    got = run(pkg, call, 0)
    errs = fc.check(call, got, ref)
    one_trip = fc.select(call, [0, 4, 8])
    hooked = run(pkg, one_trip, 1024)
    fc.check(one_trip, hooked, ref[[0, 4, 8]], errs)
    assert _same_bytes(hooked, got[[0, 4, 8]], exact_columns(family, test))
    _report(record_property, "e", call, errs)


# ---- f ----
@pytest.mark.parametrize("family, test", EVERY_TEST)
def test_special_values_on_both_paths(pkg, refs, family, test, record_property):
    """Groups of 65 and 257 rows of signed zeros, infinities and subnormals (the label columns: the extreme alphabet and scattered
    NULL rows) and all-NaN (all-NULL) groups between full ones, at the default cap and with the cap hooked to 64.  The signed-zero
    groups give the bytes of the same rows with every -0.0 made +0.0; an all-NaN group has the insufficient-data status and a
    count of 0, and the other groups' records are those of the call without it."""
    labels = family == "categorical"
    call, gone = fc.special_call(family, test)
    kinds = call["kinds"]
    ref = refs(("f", family, test), call)
    kept = [g for g in range(len(kinds)) if g not in gone]
    without = fc.select(call, kept)
    positive = dict(call)
    for name in ("x", "y", "v"):
        if name in call and not labels:
            positive[name] = call[name] + 0.0            # -0.0 + 0.0 is +0.0; every other value, NaN and infinity stay
            assert not np.any(np.signbit(positive[name]) & (positive[name] == 0.0))
    errs = {}
    for cap in (0, 64):
        got = run(pkg, call, cap)
        fc.check(call, got, ref, errs)
        assert np.all(got[gone, fc.STATUS[family]] == fc.INSUFFICIENT) and np.all(got[gone, fc.COUNT[family]] == 0)
        assert _same_bytes(run(pkg, without, cap), got[kept])
        if not labels:
            zeros = [g for g, k in enumerate(kinds) if k == "signed_zeros"]
            assert len(zeros) == 2 and _same_bytes(run(pkg, positive, cap)[zeros], got[zeros])
    _report(record_property, "f", call, errs)
