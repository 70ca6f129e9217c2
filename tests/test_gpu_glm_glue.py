"""The GLM family through its DuckDB glue (duckdb_shim/glm_family_hip.cpp, compiled against the stand-in of DuckDB's headers,
driven by tests/tools/glm_family_capi.cpp) on the GPU: poisson_fit_agg, binomial_fit_agg, logistic_fit_agg and
poisson_fit_predict_agg as a threaded GROUP BY.

Two oracles, neither the code under test, apply to every fitted group:
  * the C ABI called directly (glm.glm_fit_batch_host / glm_fit_accuracy_batch_host / glm_fit_predict_interval_batch_host) on the
    rows in the order the glue saw them: the glue adds no arithmetic and a group's fit reads only its own rows, so BIT FOR BIT,
    the interval columns and the accuracy included;
  * glm_cases.check_record against the numpy restatement (tests/glm_restate.py) at the default-tolerance tier.
    tests/test_glm_glue_cpu.py certifies without a GPU that with the fixed seeds of tests/glm_glue_cases.py every fitted group is
    inside the input conditions, and here no fitted group is left out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, import_pkg

sys.path.insert(0, os.path.dirname(__file__))
import glm_cases as GC  # noqa: E402
import glm_glue_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu

LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_glm_family_capi.so")
CONFIDENCE = {1.96: 0.95, 2.576: 0.99, 1.645: 0.9}
_P = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_P)


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.gg_open.restype = _P
    lib.gg_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.gg_close.argtypes = [_P]
    lib.gg_group_by.restype = C.c_int64
    lib.gg_group_by.argtypes = [_P, C.c_size_t, C.c_size_t, _P, C.c_size_t, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_size_t, C.c_int, C.c_size_t,
                                _P, _P, _P, _P, _P, C.c_char_p]
    return lib


def _bits_equal(got, want):
    return np.array_equal(np.asarray(got, dtype=np.float64).view(np.uint64), np.asarray(want, dtype=np.float64).view(np.uint64))


def _group_by(lib, c, run, family=None):
    """-> (return code / entries, offsets, vals (flat), flags, is_null, q, message)"""
    msg = C.create_string_buffer(512)
    q = lib.gg_open(run["fn"].encode(), None if run["spec"] is None else run["spec"].encode(), int(run["as_map"]), int(run["split"]), 1, msg)
    assert q, msg.value.decode()
    cap = max(c["n"] * 4, c["K"] * (6 * c["p"] + 11))
    offs = np.zeros(c["K"] + 1, dtype=np.int64)
    vals = np.full(cap, np.nan)
    flags = np.zeros(cap, dtype=np.uint8)
    isn = np.zeros(c["K"], dtype=np.uint8)
    out_q = C.c_size_t(0)
    y = np.ascontiguousarray(c["y"][run["family"] if family is None else family])
    rc = lib.gg_group_by(q, c["n"], c["p"], _ptr(c["key"]), c["K"], _ptr(y), _ptr(c["X"]), _ptr(c["y_null"]), _ptr(c["x_null"]), _ptr(c["xe_null"]),
                         None, _ptr(c["split"]) if run["split"] else None, G.N_THREADS, G.VECTOR_SIZE, 0, cap, _ptr(offs), _ptr(vals), _ptr(flags),
                         _ptr(isn), C.byref(out_q), msg)
    lib.gg_close(q)
    return rc, offs, vals, flags, isn, out_q.value, msg.value.decode()


def _options(run):
    return import_pkg("_abi").AnofoxHipGlmBatchOptions(run["family"], run["icpt"], 100, 1e-8, run["lam"], run["inference"], CONFIDENCE[run["z"]])


def _check_fit(lib, wide, run):
    glm = import_pkg("glm")
    c = G.case(wide)
    rc, _, vals, _, isn, q, text = _group_by(lib, c, run)
    assert rc == 0, text
    b = G.group_batch(c, run)
    refs = G.restated(wide, run)
    assert q == len(b["cols"]) == c["p"] - (1 if run["offset"] else 0)
    logistic = run["kind"] == "logistic"
    if logistic:
        out = glm.glm_fit_accuracy_batch_host(b["offsets"], b["y"], b["cols"], _options(run), run["threshold"], offset=b["off"], inference=run["inference"])
        rec, inf, acc = out if run["inference"] else (out[0], None, out[1])
    else:
        out = glm.glm_fit_batch_host(b["offsets"], b["y"], b["cols"], _options(run), offset=b["off"], inference=run["inference"])
        rec, inf = out if run["inference"] else (out, None)
    width = q + 11 + (5 * q if run["inference"] else 0)
    vals = vals[:c["K"] * width].reshape(c["K"], width)
    fitted, errs = 0, {}
    for g in range(c["K"]):
        if g not in b["groups"]:
            assert isn[g]                                      # fewer than 2 buffered rows
            continue
        i = b["groups"].index(g)
        assert (rec[i, q + 10] != 0) == (refs[i]["status"] != 0), g
        if refs[i]["status"] != 0:
            assert isn[g]                                      # a failed fit: a NULL group, the query goes on
            continue
        assert not isn[g]
        fitted += 1
        v = vals[g]
        # oracle 1: the ABI called directly, bit for bit
        assert _bits_equal(v[:q + 5], rec[i, :q + 5]), g       # coefficients, intercept, deviance, null_deviance, pseudo_r_squared, aic
        if logistic:
            assert _bits_equal(v[q + 5], acc[i]) and v[q + 6] == run["threshold"], g
        else:
            assert _bits_equal(v[q + 5], rec[i, q + 5]) and np.isnan(v[q + 6]), g
        assert v[q + 7] == rec[i, q + 6] and v[q + 8] == q and v[q + 9] == rec[i, q + 8] and v[q + 10] == rec[i, q + 9], g
        if run["inference"]:
            assert _bits_equal(v[q + 11:], inf[i]), g
        # oracle 2: the restatement
        assert GC.check_record(rec[i], None if inf is None else inf[i], refs[i], q, False, errs, label="%s g%d" % (G.run_id(run), g), lam=run["lam"]), g
        if logistic:                                           # accuracy as a count over the restatement's mu, outside the band
            a, e = int(b["offsets"][i]), int(b["offsets"][i + 1])
            mu, yy = refs[i]["mu_all"], b["y"][a:e]
            valid = np.isfinite(yy) & np.isfinite(mu)
            assert not (np.abs(mu[valid] - run["threshold"]) <= 1e-6).any(), g
            assert acc[i] == np.mean((mu[valid] >= run["threshold"]).astype(float) == yy[valid]), g
    print("restatement:", errs)
    return fitted, isn


@pytest.mark.parametrize("run", [r for r in G.RUNS if r["kind"] != "predict"], ids=G.run_id)
def test_fit_aggregates_group_by(lib, run):
    fitted, isn = _check_fit(lib, False, run)
    assert fitted == G.case()["K"] - 2 and isn[G.ONE_ROW_GROUP] and isn[G.NEGATIVE_Y_GROUP]


@pytest.mark.parametrize("run", [r for r in G.RUNS if r["kind"] == "predict"], ids=G.run_id)
def test_fit_predict_agg_group_by(lib, run):
    glm = import_pkg("glm")
    c = G.case()
    entries, offs, vals, flags, isn, _, text = _group_by(lib, c, run)
    assert entries >= 0, text
    vals = vals[:entries * 4].reshape(entries, 4)
    b = G.group_batch(c, run)
    refs = G.restated(False, run)
    p = c["p"]
    core, pred = glm.glm_fit_predict_interval_batch_host(b["offsets"], b["y"], b["cols"], _options(run), run["z"], train_counts=b["counts"])
    fitted, errs = 0, {}
    for g in range(c["K"]):
        if g not in b["groups"]:
            assert isn[g] and offs[g + 1] == offs[g]           # fewer than 2 training rows
            continue
        i = b["groups"].index(g)
        assert (core[i, p + 10] != 0) == (refs[i]["status"] != 0), g
        if refs[i]["status"] != 0:
            assert isn[g]
            continue
        assert not isn[g]
        fitted += 1
        idx = b["rows"][i]
        a, e, oa, ob = int(b["offsets"][i]), int(b["offsets"][i + 1]), int(offs[g]), int(offs[g + 1])
        assert ob - oa == len(idx)
        assert np.array_equal((flags[oa:ob] & 16) != 0, b["train"][idx])
        assert np.array_equal((flags[oa:ob] & 1) != 0, c["y_null"][idx] == 1)
        keep = c["y_null"][idx] == 0
        assert _bits_equal(vals[oa:ob, 0][keep], c["y"][run["family"]][idx][keep])      # y as given, a non-NULL NaN included
        no_x = c["xe_null"][idx].any(axis=1)
        assert np.array_equal((flags[oa:ob] & 14) == 14, no_x) and np.array_equal((flags[oa:ob] & 14) != 0, no_x)   # NULL yhat* on a NULL x element only
        assert _bits_equal(vals[oa:ob, 1:4][~no_x], pred[a:e][~no_x]), g                # oracle 1, the interval columns included
        assert np.isnan(pred[a:e][no_x]).all()
        assert GC.check_record(core[i], None, refs[i], p, False, errs, pred=None, label="%s g%d" % (G.run_id(run), g), lam=run["lam"]), g
        # the default tier bounds the objective, not mu: the values stand on the bit-exact oracle above, the restatement gives the
        # NaN pattern and the order lower <= yhat <= upper
        ok = ~no_x
        assert np.array_equal(np.isnan(refs[i]["mu_all"]), no_x)
        assert np.all(vals[oa:ob, 2][ok] <= vals[oa:ob, 1][ok]) and np.all(vals[oa:ob, 1][ok] <= vals[oa:ob, 3][ok])
    print("restatement:", errs)
    assert fitted == c["K"] - 2 and isn[G.ONE_ROW_GROUP] and isn[G.NEGATIVE_Y_GROUP]
    order = list(b["rows"][b["groups"].index(G.NAN_Y_GROUP)])
    at = int(offs[G.NAN_Y_GROUP]) + order.index(c["nan_row"])
    assert not flags[at] & 1 and np.isnan(vals[at, 0])         # the non-NULL NaN y comes back NaN and not NULL; it does not train
    order = list(b["rows"][b["groups"].index(G.NULL_ELEMENT_GROUP)])
    at = int(offs[G.NULL_ELEMENT_GROUP]) + order.index(c["null_row"])
    assert flags[at] & 14 == 14 and not flags[at] & 1          # NULL yhat, yhat_lower, yhat_upper on the row with the NULL x element


def test_wide_group_by_k_33(lib):
    fitted, isn = _check_fit(lib, True, G.WIDE_RUN)
    assert fitted == 3 and not isn.any()


def test_more_than_32_features_raises_the_library_message(lib):
    rng = np.random.default_rng(5)
    n, p = 80, 33
    c = dict(K=2, p=p, n=n, key=(np.arange(n) % 2).astype(np.uint32), X=np.ascontiguousarray(rng.uniform(-1, 1, size=(n, p))),
             y={G.POISSON: rng.poisson(2.0, size=n).astype(float)}, y_null=np.zeros(n, np.uint8), x_null=np.zeros(n, np.uint8),
             xe_null=np.zeros((n, p), np.uint8), split=np.ones(n, np.uint8))
    for run in (G.RUNS[0], G.RUNS[8]):
        rc, _, _, _, _, _, text = _group_by(lib, c, run)
        assert rc == -1 and "glm: n_features > 32 is not built" in text, text
    run = dict(G.RUNS[0], spec="offset=34", fn="poisson_fit_agg")
    rc, _, _, _, _, _, text = _group_by(lib, c, run)
    assert rc == -1 and "offset must be a 1-based index into x (1..=33), got 34" in text, text
