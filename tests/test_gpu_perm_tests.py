"""GPU tier of the permutation tests: anofox_hip_perm_test_batch_{host,device} against tests/perm_test_restate.py.

Energy distance and the t-test use only + - x / and sqrt, in the restatement's order: statistic, aux and n_extreme are held to the
restatement exactly, on both size paths.  MMD calls exp, which the device's library and numpy round differently: its statistic is
held to MMD_STAT_BOUND, sigma to the bit, and n_extreme exactly under a condition that the test first asserts on the restatement:
no permuted statistic lies within 1e-9 (relative) of the observed one without being bit-equal to it, so a difference of the size of
the bound cannot move a permutation across the comparison.

Sizes: pooled N of 4, 5, 63, 64, 65 (the rounds of compaction), 256, 257 (the two small instances), 1462 and 1463 (the cap: the last
group of the small path and the first of the large one; MMD's status 7).  B of 0, 1, 63, 64, 65 and 1000 (none, one lane, a round
and its neighbours, 16 rounds: one per wavefront of the large path)."""
import numpy as np
import pytest

import perm_test_restate as R
from conftest import import_pkg

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0DE12345678
SIZES = (4, 5, 63, 64, 65, 256, 257, 1462, 1463)
MMD_SIZES = (4, 5, 63, 64, 65, 256, 257)
BS = (0, 1, 63, 64, 65, 1000)
# |statistic - restatement| / max(|restatement|, 1e-3), the largest over every MMD case of this file measured on an MI355X, times 10
# (docs/PARITY.md, "Permutation tests")
MMD_STAT_BOUND = 1e-14   # measured: 9.5e-16 (the 1462-row group; every other case 0)
NAN = float("nan")


def _edge_groups():
    """NaN rows, an infinity, an empty group, one-sided groups, equal arms, a constant group, heavy ties."""
    rng = np.random.default_rng(77)
    i32 = lambda a: np.asarray(a, np.int32)   # noqa: E731
    return [R.make_group(rng, 40, nan_share=0.3), R.make_group(rng, 20, n1=10), R.make_group(rng, 90, ties=0.8),
            (np.array([1.0, np.inf, 2.0, 3.0, 4.0]), i32([0, 0, 1, 1, 0])), (np.zeros(0), i32([])),
            (np.array([1.0, 2.0, 3.0]), i32([0, 0, 0])), (np.array([1.0, 2.0, 3.0]), i32([0, 0, 5])),
            (np.array([np.nan, np.nan, 1.0]), i32([0, 1, 1])), (np.full(6, 2.5), i32([0, 0, 0, 1, 1, 1])),
            (np.array([1.0, 1.0, 1.0, 1.0, 1.0, 2.0]), i32([0, 0, 0, 1, 1, 1]))]


@pytest.fixture(scope="module")
def sized_call():
    """Groups of every size of SIZES (n1 != n2 from 5 rows on, continuous draws) and the edge groups, in one call."""
    rng = np.random.default_rng(2024)
    groups = [R.make_group(rng, n, n1=2 if n == 4 else n // 3 + 1) for n in SIZES] + _edge_groups()
    return R.pack(groups)


@pytest.fixture(scope="module")
def mmd_call():
    rng = np.random.default_rng(2025)
    groups = [R.make_group(rng, n, n1=2 if n == 4 else n // 3 + 1) for n in MMD_SIZES] + _edge_groups()
    return R.pack(groups)


@pytest.fixture()
def pkg():
    p = import_pkg()
    yield p
    p.perm_test_hooks(0)


def _both_entries(pkg, off, v, s, test, opts):
    """The records of the host entry, which the device entry has to reproduce byte for byte."""
    import torch
    ctx = pkg.Context(0)
    try:
        host = pkg.perm_test_batch_host(off, v, s, test, opts, ctx=ctx)
        rec = ctx.perm_test_batch_device(*(torch.from_numpy(a).cuda() for a in (off, v, s)), test, opts)
        torch.cuda.synchronize()
        assert rec.cpu().numpy().tobytes() == host.tobytes()
    finally:
        ctx.close()
    return host


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def separated(stats):
    """The exact-count condition on the restatement's statistics (observed first)."""
    obs, perm = stats[0], stats[1:]
    near = np.abs(perm - obs) <= 1e-9 * abs(obs)
    return bool(np.all(~near | (perm == obs)))


@pytest.mark.parametrize("n_perm", BS)
@pytest.mark.parametrize("test, alternative", [(R.ENERGY, 0), (R.T_TEST, 0), (R.T_TEST, 1), (R.T_TEST, 2)])
def test_energy_and_t_equal_the_restatement_on_both_paths(pkg, sized_call, test, alternative, n_perm):
    off, v, s = sized_call
    opts = pkg.PermTestOptions(n_perm, SEED, None, alternative)
    ref = R.reference(off, v, s, test, alternative, n_perm, SEED)
    got = {}
    try:
        for cap in (0, 16):   # 16: the groups of 17 rows and more take the large path
            pkg.perm_test_hooks(cap)
            got[cap] = _both_entries(pkg, off, v, s, test, opts)
    finally:
        pkg.perm_test_hooks(0)
    for cap, rec in got.items():
        bad = np.argwhere(~((rec == ref) | (np.isnan(rec) & np.isnan(ref))))
        print("test", test, "alternative", alternative, "B", n_perm, "cap", cap or "default", "differing (group, field):", bad.tolist()[:8])
        assert _same(rec, ref)
    assert got[0].tobytes() == got[16].tobytes()


@pytest.mark.parametrize("n_perm", BS)
def test_mmd_against_the_restatement(pkg, mmd_call, n_perm):
    off, v, s = mmd_call
    ref = R.reference(off, v, s, R.MMD, 0, n_perm, SEED)
    for g in range(len(off) - 1):   # the condition under which n_extreme has to be equal: asserted, never skipped
        _, status, aux, stats = R.group_stats(v[off[g]:off[g + 1]], s[off[g]:off[g + 1]], R.MMD, n_perm, SEED)
        if status == 0 and stats[0] == stats[0]:
            assert separated(stats), "group %d: a permuted statistic is too close to the observed one" % g
    got = _both_entries(pkg, off, v, s, R.MMD, pkg.PermTestOptions(n_perm, SEED))
    err = np.nanmax(np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-3))
    print("MMD B", n_perm, "statistic error %.3e" % err)
    assert _same(got[:, 2:], ref[:, 2:])                       # sigma to the bit, n_extreme, the counts, the status
    assert _same(got[:, 1], ref[:, 1])                         # p follows from n_extreme
    assert np.array_equal(np.isnan(got[:, 0]), np.isnan(ref[:, 0])) and err <= MMD_STAT_BOUND


def test_mmd_at_the_cap_above_it_and_with_a_given_sigma(pkg):
    rng = np.random.default_rng(31)
    off, v, s = R.pack([R.make_group(rng, 1462, n1=500), R.make_group(rng, 1463, n1=500), R.make_group(rng, 30, n1=11)])
    for sigma in (NAN, 0.75):
        ref = R.reference(off, v, s, R.MMD, 0, 64, SEED, sigma)
        for g in (0, 2):
            assert separated(R.group_stats(v[off[g]:off[g + 1]], s[off[g]:off[g + 1]], R.MMD, 64, SEED, sigma)[3])
        got = _both_entries(pkg, off, v, s, R.MMD, pkg.PermTestOptions(64, SEED, None if sigma != sigma else sigma))
        err = np.nanmax(np.abs(got[:, 0] - ref[:, 0]) / np.maximum(np.abs(ref[:, 0]), 1e-3))
        print("MMD 1462 rows, sigma", sigma, "statistic error %.3e" % err)
        assert got[1, 7] == 7.0 and np.isnan(got[1, :4]).all() and got[1, 4] == 1463.0
        assert _same(got[:, 1:], ref[:, 1:]) and err <= MMD_STAT_BOUND
    try:   # a lowered cap lowers MMD's with it
        pkg.perm_test_hooks(16)
        got = pkg.perm_test_batch_host(off, v, s, R.MMD, pkg.PermTestOptions(64, SEED))
    finally:
        pkg.perm_test_hooks(0)
    assert got[:, 7].tolist() == [7.0, 7.0, 7.0]


def test_a_record_depends_on_its_rows_options_and_seed_alone(pkg):
    rng = np.random.default_rng(5)
    a, b = R.make_group(rng, 150, n1=61, shift=0.0), R.make_group(rng, 33, n1=9)
    for test in (R.ENERGY, R.T_TEST, R.MMD):
        o = pkg.PermTestOptions(200, SEED)
        twice = pkg.perm_test_batch_host(*R.pack([a, b, a]), test, o)
        alone = pkg.perm_test_batch_host(*R.pack([a]), test, o)
        assert twice[0].tobytes() == twice[2].tobytes() == alone[0].tobytes()
        other = pkg.perm_test_batch_host(*R.pack([a]), test, pkg.PermTestOptions(200, SEED + 1))
        assert other[0, 0].tobytes() == alone[0, 0].tobytes() and other[0, 2].tobytes() == alone[0, 2].tobytes()
        assert other[0, 3] != alone[0, 3]   # another stream: another count (the group was drawn without a shift: p is not at its floor)


def test_scalars_equal_the_one_group_aggregate(pkg):
    rng = np.random.default_rng(6)
    (v, s) = R.make_group(rng, 80, n1=30, nan_share=0.1)
    g1, g2 = v[s == 0], v[s != 0]
    for test, scalar, agg in ((R.ENERGY, pkg.energy_distance, pkg.energy_distance_agg), (R.MMD, pkg.mmd, pkg.mmd_agg),
                              (R.T_TEST, pkg.permutation_t_test, pkg.permutation_t_test_agg)):
        opts = {"n_permutations": 300, "seed": 99, "alternative": "greater"}
        one = scalar(g1, g2, opts)
        row = agg(np.zeros(len(v), np.int64), v, s, opts).row(0)
        ref = R.group_record(np.concatenate([g1, g2]), np.concatenate([np.zeros(len(g1)), np.ones(len(g2))]), test,
                             R.GREATER if test == R.T_TEST else 0, 300, 99)
        for key in ("p_value", "n_extreme", "n", "n1", "n2", "method", "seed"):
            assert one[key] == row[key], key
        # (the scalar lays sample 1 ahead of sample 2, the aggregate keeps the rows' order: equal values may swap places, the
        # statistic can differ in its last bits)
        assert one["statistic"] == pytest.approx(row["statistic"], rel=1e-12)
        assert one["n_extreme"] == ref[3] and one["statistic"] == pytest.approx(ref[0], rel=MMD_STAT_BOUND if test == R.MMD else 0)
        assert one["method"].endswith("300 permutations)")
    drawn = pkg.energy_distance(g1, g2)
    assert drawn["seed"] is not None and pkg.energy_distance(g1, g2, {"seed": drawn["seed"]})["p_value"] == drawn["p_value"]
    with pytest.raises(pkg.InvalidInputException, match="requires at least 2 observations in group 2"):
        pkg.mmd([1.0, 2.0, 3.0], [1.0, NAN])


def test_more_groups_than_the_grid_has_workgroups(pkg):
    """70 000 groups of 4 .. 8 rows at B = 64 in one call (the grid stops at 65 536 workgroups): 200 distinct groups, repeated; a
    record depends on its rows alone, so the restatement of the 200 serves them all."""
    rng = np.random.default_rng(8)
    distinct = [R.make_group(rng, int(n)) for n in rng.integers(4, 9, size=200)]
    off, v, s = R.pack(distinct * 350)
    for test in (R.ENERGY, R.T_TEST):
        ref = np.tile(R.reference(*R.pack(distinct), test, 0, 64, SEED), (350, 1))
        got = pkg.perm_test_batch_host(off, v, s, test, pkg.PermTestOptions(64, SEED))
        assert got.shape == (70000, 8) and _same(got, ref)
