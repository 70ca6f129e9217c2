"""Randomised reference sweep of the grouped Poisson / logistic fits on the MI355X (run with -m gpu): every seed of
tests/glm_fuzz_cases.py (k = 1 .. 33 in both families: every slice width and entry class of the Gram mapping; large counts,
fractional and non-integer responses, large offsets, steep predictors) through anofox_hip_glm_fit_batch_{host,device} and,
on every third seed, fit-predict, against tests/glm_restate.py; and one launch of more groups than the grid has blocks.
tests/test_glm_fuzz_cpu.py runs the same generator through the host build and holds the pooled input-conditions test.
ANOFOX_FUZZ_SCALE multiplies the number of seeds.  Nothing here asserts an iteration count or a time."""
import numpy as np
import pytest

import glm_cases as GC
import glm_fuzz_cases as FC
from conftest import import_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def glm():
    return import_pkg("glm")


@pytest.fixture(scope="module")
def ctx():
    c = import_pkg("runtime").Context(0)
    yield c
    c.close()


def options(call, tolerance, inference):
    return import_pkg("_abi").AnofoxHipGlmBatchOptions(call["family"], call["icpt"], 100, tolerance, call["lam"], inference, 0.95)


def columns(call):
    return [np.ascontiguousarray(call["x"][:, j]) for j in range(call["p"])]


def on_device(a, dtype):
    import torch
    return torch.as_tensor(np.array(a), dtype=dtype, device=torch.device("cuda:0"))  # (np.array: the case's arrays are read-only)


@pytest.mark.parametrize("seed", FC.SEEDS, ids=FC.case_id)
def test_fuzz_glm(glm, ctx, seed, record_property):
    """tolerance = 1e-12 with inference through the host entry under glm_cases.check_record; the device entry gives the same
    bytes; tolerance = 1e-8 under glm_fuzz_cases.check_default_record; on every third seed fit-predict through the host entry
    (mu of every row, train_counts)."""
    import torch
    call = FC.case(seed)
    refs, p, o, errs = GC.reference(call), call["p"], call["offsets"], {}
    inside = [GC.in_conditions(r, p) for r in refs]
    assert FC.assert_seed_compares(call, refs) == sum(inside)
    cols = columns(call)
    rec, inf = glm.glm_fit_batch_host(o, call["y"], cols, options(call, 1e-12, True), offset=call["off"], inference=True, ctx=ctx)
    compared = 0
    for g, ref in enumerate(refs):
        compared += GC.check_record(rec[g], inf[g], ref, p, True, errs, None, FC.label(call, g), call["kinds"][g], call["lam"])
    assert compared == sum(inside)
    f64 = torch.float64
    drec, dinf = ctx.glm_fit_batch_device(on_device(o, torch.int64), on_device(call["y"], f64), [on_device(c, f64) for c in cols],
                                          options(call, 1e-12, True), offset=None if call["off"] is None else on_device(call["off"], f64),
                                          inference=True)
    torch.cuda.synchronize()
    assert drec.cpu().numpy().tobytes() == rec.tobytes() and dinf.cpu().numpy().tobytes() == inf.tobytes()
    rec8 = glm.glm_fit_batch_host(o, call["y"], cols, options(call, 1e-8, False), offset=call["off"], ctx=ctx)
    assert sum(FC.check_default_record(rec8[g], call, g, ref, errs) for g, ref in enumerate(refs)) == sum(inside)
    if seed % 3 == 0:
        tc = np.diff(o).astype(np.int64)
        tc[12] = 1  # (a long group of a regime) "fewer than 2 training rows": NULL whatever the rows hold
        core, pred = glm.glm_fit_predict_batch_host(o, call["y"], cols, options(call, 1e-12, False), offset=call["off"], train_counts=tc,
                                                    ctx=ctx)
        assert np.all(np.isnan(pred[:, 1:]))
        for g, ref in enumerate(refs):
            rows = pred[o[g]:o[g + 1], 0]
            if tc[g] < 2:
                assert core[g, p + 10] == 100 and np.all(np.isnan(core[g, :p + 10])) and np.all(np.isnan(rows)), FC.label(call, g)
                continue
            assert core[g].tobytes() == rec[g].tobytes(), FC.label(call, g)
            GC.check_record(core[g], None, ref, p, True, errs, rows, FC.label(call, g), call["kinds"][g], call["lam"])
    print(FC.case_id(seed), "compared", compared, {k: "%.2e" % v for k, v in errs.items()})
    for name, v in errs.items():
        record_property(name, v)
    record_property("compared", compared)


def test_more_groups_than_blocks(glm, ctx):
    """The grid is capped at 2^20 blocks and strides over the groups beyond: 64 distinct Poisson groups of 3 .. 6 rows (p = 1,
    an intercept) tiled to 2^20 + 64 groups, one launch through the device entry.  Every record has the bytes of group g mod 64,
    and the first and the last 64 meet glm_cases.check_record against the restatement."""
    import torch
    rng = np.random.default_rng(20261019)
    sizes = rng.integers(3, 7, size=64)
    rows = int(sizes.sum())
    x = rng.uniform(-1.0, 1.0, size=(rows, 1))
    y = rng.poisson(np.exp(1.0 + 0.8 * x[:, 0] + np.repeat(rng.uniform(-0.5, 0.5, size=64), sizes))).astype(float)
    tiles = (1 << 14) + 1
    G = 64 * tiles
    assert G == (1 << 20) + 64
    off = np.concatenate([[0], np.cumsum(np.tile(sizes, tiles))]).astype(np.int64)
    call = dict(family=GC.POISSON, p=1, icpt=True, lam=0.0, offsets=off[:65], y=y, x=x, off=None, kinds=["plain"] * 64, seed=("tiled", 0))
    refs = GC.reference(call)
    rec = ctx.glm_fit_batch_device(on_device(off, torch.int64), on_device(np.tile(y, tiles), torch.float64),
                                   [on_device(np.tile(x[:, 0], tiles), torch.float64)], options(call, 1e-12, False))
    torch.cuda.synchronize()
    assert rec.shape == (G, 12)
    bits = rec.view(torch.int64).view(tiles, 64 * 12)
    same = (bits == bits[0:1]).all(dim=1)
    assert bool(same.all()), "tile %d differs from tile 0" % int(torch.nonzero(~same)[0])
    first, last = rec[:64].cpu().numpy(), rec[G - 64:].cpu().numpy()
    compared = 0
    for g, ref in enumerate(refs):
        compared += GC.check_record(first[g], None, ref, 1, True, None, None, "group %d" % g, "plain", 0.0)
        GC.check_record(last[g], None, ref, 1, True, None, None, "group %d" % (G - 64 + g), "plain", 0.0)
    assert compared == 64  # (the restatement has every one of these groups inside the input conditions)
