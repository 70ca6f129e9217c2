"""The randomised GLM sweep without a GPU: every seed of tests/glm_fuzz_cases.py (k = 1 .. 33 in both families, the regimes
counts / fractional / noninteger / bigoffset / steep besides the plain draw) through the host build of csrc/glm_irls.h
(tests/tools/glm_host.cpp under ASan / UBSan, built by test_glm_cpu's fixture: a program of its own, never loaded into python),
against tests/glm_restate.py.  tolerance = 1e-12 with inference and fit-predict under glm_cases.check_record, the default
tolerance under glm_fuzz_cases.check_default_record, and the generator's input conditions on the restatement alone.
ANOFOX_FUZZ_SCALE multiplies the number of seeds.  Nothing here asserts an iteration count or a time."""
import numpy as np
import pytest

import glm_cases as GC
import glm_fuzz_cases as FC
from test_glm_cpu import host_glm, split  # noqa: F401  (host_glm: a fixture)


def test_generator_covers_every_width_and_regime():
    """One base pass: every k = 1 .. 33 in both families, 24 groups of at most 436 rows, every regime and pattern."""
    seen, kinds = set(), set()
    for seed in range(FC.BASE_SEEDS):
        call = FC.case(seed)
        rows = np.diff(call["offsets"])
        k = call["p"] + int(call["icpt"])
        assert 1 <= call["p"] <= 32 and len(rows) == FC.N_GROUPS and rows.max() <= 436 and rows.min() == k
        seen.add((call["family"], k))
        kinds |= {(call["family"], kind) for kind in call["kinds"]}
        assert set(FC.SPECIAL) <= set(call["kinds"])
    assert seen == {(f, k) for f in (FC.POISSON, FC.BINOMIAL) for k in range(1, 34)}
    assert {(FC.POISSON, "counts"), (FC.POISSON, "noninteger"), (FC.BINOMIAL, "fractional"), (FC.POISSON, "bigoffset"),
            (FC.BINOMIAL, "bigoffset"), (FC.POISSON, "steep"), (FC.BINOMIAL, "steep")} <= kinds
    a, b = FC.shape(5), FC.shape(5)
    assert a[:5] == b[:5]


@pytest.mark.parametrize("seed", FC.SEEDS, ids=FC.case_id)
def test_fuzz_glm_host(host_glm, seed, record_property):
    """tolerance = 1e-12 with inference and mu of every row: glm_cases.check_record's bounds (1e-9 coefficients, deviances,
    AIC and mu; 1e-6 se and dispersion).  Then tolerance = 1e-8: converged, and the long-double objective at the record's
    coefficients within [-1e-12, 2e-8] (0.1 + obj) of the restatement's.

    The Poisson seeds hold the defect this sweep found (tests/golden/glm/poisson_large_counts.json is its reduced form): with
    the step halved against the deviance at mustart on the first iteration, 11 `counts` groups of seeds 1 .. 30, all inside the
    input conditions, ended with status 3 at both tolerances."""
    call = FC.case(seed)
    refs = GC.reference(call)
    o, p, errs, compared = call["offsets"], call["p"], {}, 0
    assert FC.assert_seed_compares(call, refs) >= FC.MIN_COMPARED
    for g, (line, ref) in enumerate(zip(host_glm(GC.host_input(call, 1e-12, predict=True)), refs)):
        n = int(o[g + 1] - o[g])
        rec, inf, pred = split(line, p, n)
        if n < 2:  # the fit-predict rule (k = 1: the group of k rows); the plain fit of that group, as the GPU sweep makes it
            assert rec[p + 10] == 100 and np.all(np.isnan(rec[:p + 10])) and np.all(np.isnan(pred))
            rec, inf, _ = split(host_glm(GC.host_input(dict(call, offsets=o[g:g + 2] - o[g], y=call["y"][o[g]:], x=call["x"][o[g]:],
                                                            off=None if call["off"] is None else call["off"][o[g]:]), 1e-12))[0], p)
            pred = None
        compared += GC.check_record(rec, inf, ref, p, True, errs, pred, FC.label(call, g), call["kinds"][g], call["lam"])
    compared8 = 0
    for g, (line, ref) in enumerate(zip(host_glm(GC.host_input(call, 1e-8)), refs)):
        compared8 += FC.check_default_record(split(line, p)[0], call, g, ref, errs)
    print(FC.case_id(seed), "compared", compared, compared8, {k: "%.2e" % v for k, v in errs.items()})
    inside = [GC.in_conditions(r, p) for r in refs]  # every group inside the conditions was compared, none skipped
    assert compared8 == sum(inside) and compared == sum(inside)
    for name, v in errs.items():
        record_property(name, v)
    record_property("compared", compared)


def test_pooled_input_conditions():
    """Over all seeds of this module (the restatement alone; the references are cached): at most 5 % of the fitted groups of at
    least 12 k rows, `dup` and `degenerate` excluded, are outside the input conditions."""
    outside, pool = FC.pooled_share(FC.SEEDS)
    print("%d of %d groups outside the input conditions" % (outside, pool))
    assert pool >= 10 * len(FC.SEEDS) and outside <= FC.OUTSIDE_CAP * pool, (outside, pool)
