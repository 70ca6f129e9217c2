"""CPU-side checks of the interval and accuracy entry points of the GLM family: the four symbols, their _abi.py signatures
against the declarations in include/anofox_stats_hip.h, and the argument errors that are answered before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, import_pkg

NEW = ("anofox_hip_glm_fit_predict_interval_batch_device", "anofox_hip_glm_fit_predict_interval_batch_host",
       "anofox_hip_glm_fit_accuracy_batch_device", "anofox_hip_glm_fit_accuracy_batch_host")
_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)


def _declared(name):
    """The parameter types of a declaration in the header, spaces normalised, names stripped."""
    text = open(os.path.join(ROOT, "include", "anofox_stats_hip.h")).read()
    m = re.search(r"ANOFOX_HIP_API bool %s\((.*?)\);" % name, text, re.S)
    assert m, name
    out = []
    for part in m.group(1).split(","):
        t = re.sub(r"\s+", " ", part.strip())
        t = re.sub(r"\s*\w+$", "", t)   # drop the parameter's name
        out.append(t.replace(" *", "*"))
    return out


def test_symbols_and_signatures_mirror_the_header():
    abi = import_pkg("_abi")
    lib = abi.load()
    for name in NEW:
        assert name in abi.SYMBOLS and getattr(lib, name) is not None
        res, args = abi.SYMBOLS[name]
        assert res is C.c_bool
        device = name.endswith("_device")
        kinds = {"AnofoxHipContext*": (abi._CTX,), "int64_t": (C.c_int64,), "size_t": (C.c_size_t,), "double": (C.c_double,),
                 "AnofoxHipGlmBatchOptions": (abi.AnofoxHipGlmBatchOptions,), "AnofoxError*": (abi._ERRP,),
                 "const int64_t*": (C.c_void_p,) if device else (_I64P,), "const double*": (C.c_void_p,) if device else (_DP,),
                 "double*": (C.c_void_p,) if device else (_DP,),
                 "const double*const*": (C.POINTER(C.c_void_p),) if device else (C.POINTER(_DP),)}
        want = _declared(name)
        assert len(want) == len(args), (name, want)
        for t, a in zip(want, args):
            assert a in kinds[t], (name, t, a)
    # each takes its sibling's arguments plus the ones the header names
    for new, old, extra in ((NEW[0], "anofox_hip_glm_fit_predict_batch_device", 1), (NEW[1], "anofox_hip_glm_fit_predict_batch_host", 1),
                            (NEW[2], "anofox_hip_glm_fit_batch_device", 2), (NEW[3], "anofox_hip_glm_fit_batch_host", 2)):
        a, b = abi.SYMBOLS[new][1], abi.SYMBOLS[old][1]
        opt = a.index(abi.AnofoxHipGlmBatchOptions)
        assert len(a) == len(b) + extra and a[:opt + 1] == b[:opt + 1] and a[opt + 1] is C.c_double
        assert a[opt + 2:opt + 4] == b[opt + 1:opt + 3] and a[-1] == b[-1]
    assert abi.AnofoxHipGlmBatchOptions.confidence_level.offset == 40 and C.sizeof(abi.AnofoxHipGlmBatchOptions) == 48


def _fixture():
    abi = import_pkg("_abi")
    n = 8
    y = np.ones(n)
    off = np.array([0, n], dtype=np.int64)
    c = y.ctypes.data_as(_DP)
    return abi, abi.load(), n, y, off, c


@pytest.mark.parametrize("family, z, text", [(0, -1.0, "glm: interval_z"), (0, float("nan"), "glm: interval_z"),
                                             (0, float("inf"), "glm: interval_z"), (1, 1.96, "glm: the prediction interval of the binomial")])
def test_interval_argument_errors(family, z, text):
    abi, lib, n, y, off, c = _fixture()
    err = abi.AnofoxError()
    opts = abi.AnofoxHipGlmBatchOptions(family, True, 100, 1e-8, 0.0, False, 0.95)
    core, pred = np.full(13, 7.0), np.full((n, 3), 7.0)
    ok = lib.anofox_hip_glm_fit_predict_interval_batch_host(None, 1, 2, n, off.ctypes.data_as(_I64P), c, (_DP * 2)(c, c), None, None, opts, z,
                                                            core.ctypes.data_as(_DP), pred.ctypes.data_as(_DP), C.byref(err))
    assert not ok and err.code == 1 and text in err.text(), err.text()
    assert np.all(core == 7.0) and np.all(pred == 7.0)
    fake = C.c_void_p(y.ctypes.data)
    ok = lib.anofox_hip_glm_fit_predict_interval_batch_device(None, 1, 2, n, fake, fake, (C.c_void_p * 2)(fake, fake), None, None, opts, z,
                                                              fake, fake, C.byref(err))
    assert not ok and err.code == 1 and text in err.text(), err.text()


@pytest.mark.parametrize("family, thr, text", [(0, 0.5, "glm: the accuracy is the binomial"), (1, float("nan"), "glm: threshold"),
                                               (1, float("inf"), "glm: threshold")])
def test_accuracy_argument_errors(family, thr, text):
    abi, lib, n, y, off, c = _fixture()
    err = abi.AnofoxError()
    opts = abi.AnofoxHipGlmBatchOptions(family, True, 100, 1e-8, 0.0, False, 0.95)
    rec, acc = np.full(13, 7.0), np.full(1, 7.0)
    ok = lib.anofox_hip_glm_fit_accuracy_batch_host(None, 1, 2, n, off.ctypes.data_as(_I64P), c, (_DP * 2)(c, c), None, opts, thr,
                                                    rec.ctypes.data_as(_DP), None, acc.ctypes.data_as(_DP), C.byref(err))
    assert not ok and err.code == 1 and text in err.text(), err.text()
    assert np.all(rec == 7.0) and acc[0] == 7.0
    fake = C.c_void_p(y.ctypes.data)
    ok = lib.anofox_hip_glm_fit_accuracy_batch_device(None, 1, 2, n, fake, fake, (C.c_void_p * 2)(fake, fake), None, opts, thr, fake, None,
                                                      fake, C.byref(err))
    assert not ok and err.code == 1 and text in err.text(), err.text()


def test_pointer_checks_of_the_new_entries():
    abi, lib, n, y, off, c = _fixture()
    err = abi.AnofoxError()
    po = abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    bo = abi.AnofoxHipGlmBatchOptions(1, True, 100, 1e-8, 0.0, False, 0.95)
    offp, cols = off.ctypes.data_as(_I64P), (_DP * 2)(c, c)
    rec = np.empty(13)
    assert not lib.anofox_hip_glm_fit_predict_interval_batch_host(None, 1, 2, n, offp, c, cols, None, None, po, 1.96, rec.ctypes.data_as(_DP),
                                                                  None, C.byref(err))
    assert err.code == 1 and "pred is NULL" in err.text()
    assert not lib.anofox_hip_glm_fit_accuracy_batch_host(None, 1, 2, n, offp, c, cols, None, bo, 0.5, rec.ctypes.data_as(_DP), None, None,
                                                          C.byref(err))
    assert err.code == 1 and "accuracy is NULL" in err.text()
    c33 = (_DP * 33)(*[c] * 33)
    assert not lib.anofox_hip_glm_fit_accuracy_batch_host(None, 1, 33, n, offp, c, c33, None, bo, 0.5, rec.ctypes.data_as(_DP), None,
                                                          rec.ctypes.data_as(_DP), C.byref(err))
    assert err.code == 1 and "glm: n_features > 32 is not built" in err.text()
    fake = C.c_void_p(y.ctypes.data)
    vcols = (C.c_void_p * 2)(fake, fake)
    assert not lib.anofox_hip_glm_fit_predict_interval_batch_device(None, 1, 2, n, fake, fake, vcols, None, None, po, 1.96, fake, fake,
                                                                    C.byref(err))
    assert err.code == 1 and "context is NULL" in err.text()
    assert not lib.anofox_hip_glm_fit_accuracy_batch_device(None, 1, 2, n, fake, fake, vcols, None, bo, 0.5, fake, None, fake, C.byref(err))
    assert err.code == 1 and "context is NULL" in err.text()
    # no groups: nothing to do, nothing touched
    assert lib.anofox_hip_glm_fit_accuracy_batch_host(None, 0, 2, 0, None, None, cols, None, bo, 0.5, None, None, None, C.byref(err))


def test_interval_z_table():
    glm = import_pkg("glm")
    assert [glm.interval_z(v) for v in (0.95, 0.9505, 0.99, 0.9895, 0.90, 0.9, 0.8, 0.952, 0.5)] == \
        [1.96, 1.96, 2.576, 2.576, 1.645, 1.645, 1.96, 1.96, 1.96]
