"""ctypes binding of tests/tools/glmm_family_capi.cpp (libanofox_glmm_family_capi.so) for the glmm glue tests."""
import ctypes as C
import os

import numpy as np

from conftest import ROOT, import_pkg

SHIM = os.path.join(ROOT, "anofox-statistics_amd", "duckdb_shim")
TOOLS = os.path.join(ROOT, "tests", "tools")
LIB = os.path.join(SHIM, "libanofox_glmm_family_capi.so")
VARCHAR, BIGINT, INTEGER = 0, 1, 2
_P = C.c_void_p
_U8, _F64, _I64, _U32 = C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)


def load():
    import_pkg()
    lib = C.CDLL(LIB)
    lib.ag_open.restype = _P
    lib.ag_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p]
    lib.ag_close.argtypes = [_P]
    lib.ag_registered.argtypes = [_P, C.c_char_p]
    lib.ag_registered_count.argtypes = [_P]
    lib.ag_overloads.argtypes = [_P, C.c_char_p, C.POINTER(C.c_int)]
    lib.ag_result_fields.argtypes = [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p]
    lib.ag_group_by.restype = C.c_int64
    lib.ag_group_by.argtypes = [_P, C.c_size_t, C.c_size_t, _U32, C.c_size_t, _F64, _F64, _I64, _U8, _U8, _U8, _U8, _U8, _U8, _U32, C.c_int,
                                C.c_size_t, C.c_int, C.c_size_t, _I64, _F64, _U8, _U8, C.POINTER(C.c_size_t), C.c_size_t, _F64, C.c_char_p]
    return lib


def open_query(lib, fn, spec=None, as_map=False, foldable=True, group_kind=VARCHAR, split=False):
    msg = C.create_string_buffer(512)
    q = lib.ag_open(fn.encode(), None if spec is None else spec.encode(), int(as_map), int(foldable), group_kind, int(split), msg)
    return q, msg.value.decode()


def fields(lib, q):
    kinds, is_list, names = (C.c_int * 24)(), C.c_int(-1), C.create_string_buffer(512)
    k = lib.ag_result_fields(q, kinds, C.byref(is_list), names)
    return is_list.value, list(kinds[:k]), names.value.decode()


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def group_by(lib, q, key, n_keys, y, X, group, y_null=None, x_null=None, group_null=None, split_train=None, x_len=None, threads=2, vector_size=64,
             dictionary=True):
    """-> dict(is_null, and for the fit vals[n_keys, width], q, r_offsets, ranef[.., 4]; for fit-predict offsets, vals[.., 5], flags)"""
    n, p = X.shape
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8)   # noqa: E731
    key, y, X, group = np.ascontiguousarray(key, np.uint32), np.ascontiguousarray(y, float), np.ascontiguousarray(X, float), np.ascontiguousarray(group, np.int64)
    y_null, x_null, group_null, split_train = u8(y_null), u8(x_null), u8(group_null), u8(split_train)
    x_len = None if x_len is None else np.ascontiguousarray(x_len, np.uint32)
    cap = max(n, n_keys * (6 * p + 18)) + 16
    offsets, vals, flags, is_null = np.zeros(n_keys + 1, np.int64), np.full(cap * 5, np.nan), np.zeros(cap, np.uint8), np.zeros(n_keys, np.uint8)
    ranef, out_q, msg = np.full((n + 1) * 4, np.nan), C.c_size_t(0), C.create_string_buffer(512)
    r = lib.ag_group_by(q, n, p, _ptr(key, _U32), n_keys, _ptr(y, _F64), _ptr(X, _F64), _ptr(group, _I64), _ptr(y_null, _U8), _ptr(x_null, _U8), None,
                        _ptr(group_null, _U8), _ptr(split_train, _U8), None, _ptr(x_len, _U32), threads, vector_size, int(dictionary), cap, _ptr(offsets, _I64),
                        _ptr(vals, _F64), _ptr(flags, _U8), _ptr(is_null, _U8), C.byref(out_q), n + 1, _ptr(ranef, _F64), msg)
    if r < 0:
        raise RuntimeError(msg.value.decode())
    is_list, kinds, _ = fields(lib, q)
    if not is_list:   # the fit
        w = len(kinds)
        width = out_q.value + 17 + (5 * out_q.value + 1 if w == 24 else 0)
        return dict(is_null=is_null.astype(bool), q=out_q.value, vals=vals[:n_keys * width].reshape(n_keys, width), r_offsets=offsets,
                    ranef=ranef[:4 * offsets[-1]].reshape(-1, 4))
    return dict(is_null=is_null.astype(bool), offsets=offsets, vals=vals[:5 * r].reshape(-1, 5), flags=flags[:r])
