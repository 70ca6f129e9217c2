"""The marshalling layer of the Python binding: everything between a numpy array or a torch tensor and an argument of the C ABI
(include/anofox_stats_hip.h).  It owns, once each:

- host inputs: contiguous arrays of the slot's dtype (an array that already is one is passed in place), every length checked;
- device inputs: the same rules on tensors, which have to be CUDA, contiguous, of the slot's dtype and on one device;
- the table of column pointers, always max(p, 1) long;
- outputs: allocated, or a caller's tensor checked like an input (at least the required element count);
- the stream of a device call, the handle of an optional context, and the one-shot accumulate gate of the entries that consume it;
- the call: arrays and tensors go in as they are, `_abi.SYMBOLS` says what each becomes, a false return raises AnofoxStatsError;
- the scalar entries of the reference's layout (data arrays in, a result struct out, its text freed);
- the rows of a GROUP BY as the batch entries take them: sorted by key, with their offsets.

Every check raises ValueError before the library is reached.  runtime.py and glm.py state the contract of each entry on top of
this: which inputs, which output shapes, which symbol, what it returns."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from .options import InvalidInputException

_DP = C.POINTER(C.c_double)
F64, I64, I32, U32, U8 = "float64", "int64", "int32", "uint32", "uint8"

# the device entries whose C side consumes the context's accumulate gate (anofox_hip_context_set_accumulate_gate): the torch
# events behind it are released after these calls and after no other
_GATE_CONSUMERS = frozenset(("anofox_hip_fit_batch_device", "anofox_hip_elasticnet_fit_batch_device",
                             "anofox_hip_bls_fit_batch_device", "anofox_hip_elasticnet_fit_predict_batch_device"))


def handle(ctx):
    """The AnofoxHipContext of an optional Context (None: the calling thread's default context)."""
    return None if ctx is None else ctx._h


def _argument(a, argtype):
    # (a POINTER(c_double) argtype does not take a bare address, so an array is cast to its slot's type; a c_void_p slot takes
    # the integer a tensor gives; None is NULL everywhere)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(argtype)
    return a.data_ptr() if hasattr(a, "data_ptr") else a


def _invoke(lib, name, args):
    """-> (ok, err) of lib.<name>(*args, &err).  `args` keeps every array and tensor referenced until the call has returned."""
    argtypes = _abi.SYMBOLS[name][1]
    if len(args) != len(argtypes) - 1:
        raise TypeError(f"{name} takes {len(argtypes) - 1} arguments before the error, got {len(args)}")
    err = _abi.AnofoxError()
    return getattr(lib, name)(*[_argument(a, t) for a, t in zip(args, argtypes)], C.byref(err)), err


def call(lib, name, *args):
    """lib.<name>(*args, &err); a false return raises AnofoxStatsError with the library's code and text."""
    ok, err = _invoke(lib, name, args)
    if not ok:
        raise AnofoxStatsError(err.code, err.text())


def create(lib, name, *args):
    """call() of an entry whose last argument before the error receives a new handle; returns the handle."""
    h = C.c_void_p()
    call(lib, name, *args, C.byref(h))
    return h


def host_array(a, dtype, n=None, what="array"):
    """`a` as a contiguous numpy array of `dtype` (itself when it already is one) of exactly n elements (None: any)."""
    v = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and v.size != n:
        raise ValueError(f"{what} has {v.size} elements, the call needs {n}")
    return v


def device_tensor(t, dtype, n=None, what="tensor", device=None, at_least=False):
    """`t` checked as a contiguous CUDA tensor of `dtype` (None: any) on `device` (None: any) with exactly, or at least, n
    elements (None: any)."""
    import torch

    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous CUDA tensor")
    if dtype is not None and t.dtype != getattr(torch, dtype):
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    if device is not None and t.device != device:
        raise ValueError(f"{what} is on {t.device}, the call's other tensors are on {device}")
    if n is not None and (t.numel() < n if at_least else t.numel() != n):
        raise ValueError(f"{what} has {t.numel()} elements, the call needs {'at least ' if at_least else ''}{n}")
    return t


def scalar_call(symbol, arrays, options, result, free, fields) -> dict:
    """lib.<symbol>(*arrays as AnofoxDataArray (a None entry is a NULL)[, options], &result) -> {name: result.<field>} for the
    (name, field) pairs of `fields`, a text decoded; the result is released through lib.<free> (None: it holds no memory).
    `options`: None, one struct, or a tuple of the arguments that stand in its place.  A failure raises InvalidInputException with the library's text and its code in `.code`."""
    from .scalar import _data_array
    lib = _abi.load()
    data = [_data_array(a) for a in arrays]   # (array, what keeps its memory alive)
    res = result()
    try:
        call(lib, symbol, *[d[0] for d in data], *(() if options is None else options if isinstance(options, tuple) else (options,)),
             C.byref(res))
    except AnofoxStatsError as failed:
        e = InvalidInputException(f"{symbol.replace('anofox_', '')} failed: {failed}")
        e.code = failed.code
        raise e from None
    try:
        values = [(name, getattr(res, field)) for name, field in fields]
        return {name: v.decode() if isinstance(v, bytes) else v for name, v in values}
    finally:
        if free is not None:
            getattr(lib, free)(C.byref(res))


def column(values) -> np.ndarray:
    """A column of an aggregate as float64; a None (SQL NULL) becomes NaN."""
    a = np.asarray(values)
    return np.array([np.nan if v is None else v for v in values], dtype=np.float64) if a.dtype == object else np.asarray(a, np.float64)


def group_rows(keys):
    """The rows of a GROUP BY -> (the sorted unique keys, the permutation that sorts the rows by key and keeps the order of a
    key's rows, row_offsets[n_keys + 1] into the permuted rows)."""
    uniq, inv = np.unique(np.asarray(keys), return_inverse=True)
    perm = np.argsort(inv, kind="stable")
    return uniq, perm, np.concatenate([[0], np.cumsum(np.bincount(inv, minlength=len(uniq)))]).astype(np.int64)


class _Batch:
    """The checked inputs of one call: G groups, p columns, N rows, `off` (row_offsets), `y` and `cols` (the pointer table).
    row_offsets / y None: the entry has none (N is then the length of column 0).  `lead`: what an error calls `y`."""
    suffix = ""

    def __init__(self, row_offsets, y, x_cols, lead="y"):
        self.off = None if row_offsets is None else self.array(row_offsets, I64, None, "row_offsets")
        self.G = None if self.off is None else self._size(self.off) - 1
        if self.G is not None and self.G < 0:
            raise ValueError("row_offsets needs one entry more than there are groups")
        self.y = None if y is None else self.array(y, F64, None, lead)
        lead = self.y if y is not None else self.array(x_cols[0], F64, None, "column 0") if len(x_cols) else None
        self.N = 0 if lead is None else self._size(lead)
        self._cols = [self.array(c, F64, self.N, f"column {j}") for j, c in enumerate(x_cols)]
        self.p = len(self._cols)
        self.cols = self._table(self._cols)

    @property
    def head(self):
        """What a grouped entry begins with."""
        return self.G, self.p, self.N, self.off, self.y, self.cols

    @property
    def rows_head(self):
        """What an explicit-frames entry begins with."""
        return self.N, self.p, self.y, self.cols

    def rows(self, a, what, dtype=F64):
        """An optional array with one element per row."""
        return None if a is None else self.array(a, dtype, self.N, what)

    def groups(self, a, what, dtype=I64):
        """An optional array with one element per group."""
        return None if a is None else self.array(a, dtype, self.G, what)

    def frames(self, frame_lo, frame_hi):
        return self.array(frame_lo, I64, self.N, "frame_lo"), self.array(frame_hi, I64, self.N, "frame_hi")


class HostBatch(_Batch):
    """numpy in, numpy out, on an optional Context."""
    suffix = "_host"

    def __init__(self, ctx, row_offsets, y, x_cols, lead="y"):
        self.lib, self.h = _abi.load(), handle(ctx)
        super().__init__(row_offsets, y, x_cols, lead)

    array = staticmethod(host_array)

    @staticmethod
    def _size(v):
        return v.size

    @staticmethod
    def _table(cols):
        return (_DP * max(len(cols), 1))(*[c.ctypes.data_as(_DP) for c in cols])

    def out(self, shape, dtype=F64, given=None):
        return np.empty(shape, dtype=dtype)

    def call(self, name, *args):
        call(self.lib, name + self.suffix, self.h, *args)


class DeviceBatch(_Batch):
    """CUDA tensors in and out, asynchronous, on a Context (`owner`: the object whose handle the entry takes, the context
    itself unless it is an AggState).  use_current_torch_stream: the call is enqueued on torch's current stream."""
    suffix = "_device"

    def __init__(self, ctx, row_offsets, y, x_cols, use_current_torch_stream, owner=None, lead="y"):
        self.ctx, self.owner, self.stream, self.device = ctx, ctx if owner is None else owner, use_current_torch_stream, None
        super().__init__(row_offsets, y, x_cols, lead)

    def array(self, t, dtype, n=None, what="tensor", at_least=False):
        device_tensor(t, dtype, n, what, self.device, at_least)
        self.device = t.device     # (the first tensor's; every later one has to be on it)
        return t

    @staticmethod
    def _size(t):
        return int(t.numel())

    @staticmethod
    def _table(cols):
        return (C.c_void_p * max(len(cols), 1))(*[c.data_ptr() for c in cols])

    def out(self, shape, dtype=F64, given=None):
        """An output of `shape`: a new tensor, or the caller's, which has to hold at least that many elements."""
        import torch

        if given is not None:
            return self.array(given, dtype, math.prod(shape), "a caller-supplied output", at_least=True)
        if self.device is None:
            raise ValueError("a device call needs at least one tensor to know its device from")
        return torch.empty(shape, dtype=getattr(torch, dtype), device=self.device)

    def call(self, name, *args):
        import torch

        name += self.suffix
        if self.stream:
            self.ctx.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        ok, err = _invoke(self.owner._lib, name, (self.owner._h,) + args)
        if name in _GATE_CONSUMERS:
            self.ctx._gate_events = None   # consumed (or dropped) by the call above
        if not ok:
            raise AnofoxStatsError(err.code, err.text())
