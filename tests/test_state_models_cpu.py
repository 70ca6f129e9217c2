"""CPU-side checks of the elastic net / BLS Finalize of a streaming state (anofox_hip_agg_state_finalize_{elasticnet,bls}_*):
the header and the ctypes table carry the six symbols with matching arity, the Python methods reject a state that does not
hold the family's moments before any library call, and the inputs of tests/test_gpu_state_models.py meet the restatements'
input conditions (asserted, never skipped)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import state_models_cases as smc  # noqa: E402
from conftest import ROOT, import_pkg  # noqa: E402

HEADER = os.path.join(ROOT, "include", "anofox_stats_hip.h")
SYMBOLS = [f"anofox_hip_agg_state_finalize_{fam}_{form}" for fam in ("elasticnet", "bls") for form in ("host", "device", "slots_host")]


def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"ANOFOX_HIP_API[^;(]*?\b(anofox_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_header_declares_the_six_symbols_and_abi_binds_them_with_matching_arity():
    abi = import_pkg("_abi")
    decl = _declarations()
    for name in SYMBOLS:
        assert name in decl, f"{name} is not declared in the header"
        assert name in abi.SYMBOLS, f"{name} has no ctypes prototype"
        n_args = len([a for a in decl[name].split(",") if a.strip()])
        assert len(abi.SYMBOLS[name][1]) == n_args, f"{name}: {len(abi.SYMBOLS[name][1])} ctypes arguments, {n_args} declared"
    lib = abi.load()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None


class _NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the state was checked")


def _state(pkg, model="ols", fit_intercept=True, hc="none", inference=False):
    """An AggState object that has no device behind it: only what the checks read."""
    abi = import_pkg("_abi")
    st = object.__new__(pkg.AggState)
    opts = pkg.RegressionOptions(fit_intercept=fit_intercept, compute_inference=inference).batch_options(model)
    opts.hc_type = abi.HC_TYPE[hc]
    st.options, st.p, st._lib, st._h, st._ctx = opts, 3, _NoLibrary(), None, None
    return st


@pytest.mark.parametrize("family", ["elasticnet", "bls", "nnls"])
def test_python_methods_reject_a_mismatched_state_before_any_library_call(family):
    pkg = import_pkg()

    def call(st, fit_intercept):
        pool = object.__new__(pkg.StreamingStates)
        pool.context, pool.state, pool.n_slots, pool.unrefined, pool._solved = None, st, 4, 0, None
        getattr(pool, f"finalize_{family}")({"fit_intercept": fit_intercept})

    for st, icpt, msg in ((_state(pkg, fit_intercept=True), False, "fit_intercept"),
                          (_state(pkg, fit_intercept=False), True, "fit_intercept"),
                          (_state(pkg, model="wls"), True, "WLS"),
                          (_state(pkg, model="ridge"), True, "ridge"),
                          (_state(pkg, hc="hc1", inference=True), True, "hc_type")):
        with pytest.raises(pkg.AnofoxStatsError, match=msg) as ei:
            call(st, icpt)
        assert ei.value.code == import_pkg("_abi").ERROR_INVALID_INPUT
        # and the runtime layer on its own
        o = pkg.ElasticNetOptions(fit_intercept=icpt).batch_options() if family == "elasticnet" else pkg.BlsOptions(fit_intercept=icpt).batch_options()
        with pytest.raises(pkg.AnofoxStatsError, match=msg):
            (st.finalize_elasticnet if family == "elasticnet" else st.finalize_bls)(o)
    # a matching state passes the check and reaches the library
    with pytest.raises(AssertionError, match="library call"):
        call(_state(pkg, fit_intercept=True), True)


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("p", smc.MOMENT_P + smc.LOG_ONLY_P)
@pytest.mark.parametrize("family", ["elasticnet", "bls"])
def test_gpu_test_inputs_meet_the_restatements_input_conditions(family, p, icpt):
    """elasticnet_restate.input_conditions / bls_restate.moment_conditions on every slot of every parity case (asserted inside
    state_models_cases.restate through the sweep's own drivers)."""
    c, ref = smc.cached(family, p, icpt, restated=True)
    assert c.S % 64 != 0 and len(ref[0]) == c.S
    counts = np.diff(c.goffs)
    assert counts.max() > 8192 and (counts == 0).any() and (counts == 1).any() and (counts == 2).any()
    assert (c.valid == 0).any() and np.isnan(c.gy).any() and np.isnan(c.gX).any()
    status = ref[0][:, p + 5]
    assert (status == 100).any() and (status == 0).sum() >= 5


@pytest.mark.parametrize("icpt", [True, False])
@pytest.mark.parametrize("family", ["elasticnet", "bls"])
def test_exact_fit_inputs_are_built_as_described(family, icpt):
    """The flagged-group cases: the designated slots fit exactly, inside the bounds, in whole numbers whose moments are exact in
    any summation order (state_models_cases.make_case says why)."""
    for p in smc.MOMENT_P:
        c = smc.cached(family, p, icpt, exact=True)
        assert len(c.exact_slots) >= 5
        for g in c.exact_slots:
            s = slice(c.goffs[g], c.goffs[g + 1])
            ok = np.isfinite(c.gy[s]) & np.isfinite(c.gX[s]).all(axis=1)
            rows = np.column_stack([c.gX[s][ok], c.gy[s][ok]])
            assert np.array_equal(rows, np.rint(rows)) and np.sum(rows ** 2) < 2.0 ** 50
            D = np.column_stack([np.ones(ok.sum()), c.gX[s][ok]]) if icpt else c.gX[s][ok]
            b, *_ = np.linalg.lstsq(D, c.gy[s][ok], rcond=None)
            r = c.gy[s][ok] - D @ b
            assert np.linalg.norm(r) <= 1e-9 * np.linalg.norm(c.gy[s][ok])
