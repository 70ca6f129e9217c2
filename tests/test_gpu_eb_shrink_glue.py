"""GPU tier of eb_shrink_agg's DuckDB glue: duckdb_shim/eb_shrink_hip.cpp driven through tests/tools/eb_shrink_capi.cpp
(libanofox_eb_shrink_capi.so) on the REAL library.  One GROUP BY over the sets of a call of tests/eb_shrink_cases.py, Update from
two threads (so every set is a Combine of two states), NULL estimates and standard errors, a key with one pair, a key no row has
and a set left with one usable pair: every field equals the C ABI's result on the same pairs in the same order."""
import ctypes as C
import os

import numpy as np
import pytest

import eb_shrink_cases as EC
from conftest import ROOT, import_pkg

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim", "libanofox_eb_shrink_capi.so")
THREADS, VSIZE = 2, 64
_P, _U8, _DP = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.eg_open.restype = _P
    lib.eg_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p]
    lib.eg_close.argtypes = [_P]
    lib.eg_group_by.restype = C.c_int64
    lib.eg_group_by.argtypes = [_P, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, _DP, _DP, _U8, _U8, C.c_int, C.c_size_t, C.c_int,
                                C.c_size_t, _U8, _DP, C.POINTER(C.c_int64), _DP, C.c_char_p]
    return lib


@pytest.fixture(scope="module")
def table():
    """The pairs of a one-column call (13 sets: keys 0 .. 12, rows shuffled), every 19th estimate and every 23rd se a SQL NULL;
    key 13 has no row.  NaN / inf / non-positive values of the call stay values: the library's own rule leaves them out."""
    call = EC.make_call("heterogeneous", 1, "tight", 41)
    off = call["offsets"]
    key = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = np.random.default_rng(3).permutation(len(key))
    key, est, se = key[order], call["est"][:len(key)][order], call["se"][:len(key)][order]
    idx = np.arange(len(key))
    return dict(key=key.astype(np.uint32), est=est, se=se, est_null=idx % 19 == 0, se_null=idx % 23 == 0, n_keys=len(off))


def arrival(t, k):
    """The pairs of key k in the order the driver makes them arrive: thread by thread, within a thread vector by vector."""
    rows = np.flatnonzero((t["key"] == k) & ~t["est_null"] & ~t["se_null"])
    return np.concatenate([rows[(rows // VSIZE) % THREADS == th] for th in range(THREADS)]) if len(rows) else rows


@pytest.mark.parametrize("spec, options", [(None, None), ("tau_method=none", {"tau_method": "none"}), ("tau2=0.04", {"tau2": 0.04}),
                                           ("tau2=-1", {"tau2": -1.0})])
def test_group_by_equals_the_c_abi(lib, table, spec, options):
    pkg = import_pkg()
    t = table
    n, K = len(t["key"]), t["n_keys"]
    msg = C.create_string_buffer(512)
    q = lib.eg_open(b"eb_shrink_agg", None if spec is None else spec.encode(), 0, 1, msg)
    assert q, msg.value.decode()
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    is_null, summary, offs, rows = np.zeros(K, np.uint8), np.zeros(K * 6), np.zeros(K + 1, np.int64), np.zeros(n * 5)
    est_null, se_null = u8(t["est_null"]), u8(t["se_null"])
    rc = lib.eg_group_by(q, n, t["key"].ctypes.data_as(C.POINTER(C.c_uint32)), K, t["est"].ctypes.data_as(_DP), t["se"].ctypes.data_as(_DP),
                         est_null.ctypes.data_as(_U8), se_null.ctypes.data_as(_U8), THREADS, VSIZE, 0, n, is_null.ctypes.data_as(_U8),
                         summary.ctypes.data_as(_DP), offs.ctypes.data_as(C.POINTER(C.c_int64)), rows.ctypes.data_as(_DP), msg)
    lib.eg_close(q)
    assert rc >= 0, msg.value.decode()
    summary, rows = summary.reshape(K, 6), rows.reshape(n, 5)
    # the same pairs in the same order through the C ABI: every state with 2 pairs or more is a set of one call
    order = [arrival(t, k) for k in range(K)]
    sent = [k for k in range(K) if len(order[k]) >= 2]
    cat = np.concatenate([order[k] for k in sent])
    off = np.concatenate([[0], np.cumsum([len(order[k]) for k in sent])]).astype(np.int64)
    out, ref = pkg.eb_shrink_batch_host(off, t["est"][cat], t["se"][cat], options=options)
    n_live = 0
    for k in range(K):
        if k not in sent:
            assert is_null[k] and offs[k + 1] == offs[k]
            continue
        s = sent.index(k)
        assert bool(is_null[k]) == (ref[s, 0, 7] != 0)
        if is_null[k]:
            continue
        n_live += 1
        assert np.array_equal(summary[k], ref[s, 0, :6])
        got = rows[offs[k]:offs[k + 1]]
        assert len(got) == len(order[k])
        assert np.array_equal(got[:, 0], t["est"][order[k]], equal_nan=True) and np.array_equal(got[:, 1], t["se"][order[k]], equal_nan=True)
        assert np.array_equal(got[:, 2:], out[off[s]:off[s + 1], 0], equal_nan=True)
    assert rc == sum(offs[k + 1] - offs[k] for k in range(K))
    assert n_live == 0 if spec == "tau2=-1" else n_live >= 6   # (the invalid tau_squared: every set NULL)
