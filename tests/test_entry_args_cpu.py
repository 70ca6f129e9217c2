"""Every argument check that an entry point answers before it needs a device, as one table: entry point x bad argument ->
(code, exact text).  The texts are written out here; a call with two bad arguments per entry pins which check comes first."""
import ctypes as C

import numpy as np
import pytest

from conftest import import_pkg

_DP = C.POINTER(C.c_double)
_I64P = C.POINTER(C.c_int64)
N = 8
INPUT, ALPHA, L1, MISMATCH = 1, 4, 5, 9

NEG = "negative n_groups or n_rows"
X_EMPTY = "x is NULL or empty"
COL_NULL = "x column pointer is NULL"
OUT_NULL = "row_offsets, y or an output is NULL"
WIDE = "n_features = 129 exceeds the supported maximum of 128"
Q_WIDE = "quantile regression: n_features > 32 is not built"
G_WIDE = "glm: n_features > 32 is not built"
CTX = "context is NULL"
Y_EMPTY = "Empty input: y cannot be empty"


def mismatch(ny, nx):
    return "Dimension mismatch: y has %d elements, X has %d rows" % (ny, nx)


class Env:
    """The arguments of a good call, host and device flavoured (the device pointers are never dereferenced: every call here fails
    before a device is needed)."""

    def __init__(self):
        self.abi = import_pkg("_abi")
        self.lib = self.abi.load()
        self.y = np.ones(N)
        self.off = np.array([0, N], dtype=np.int64)
        self.out = np.zeros(4096)
        self.it = np.zeros(64, dtype=np.int32)
        self.taus = np.array([0.25, 0.5])
        self.err = self.abi.AnofoxError()

    def host(self, p=2, offsets=True, y=True, out=True, null_col=None, cols=True):
        c = self.y.ctypes.data_as(_DP)
        col = (_DP * max(p, 1))(*[c] * max(p, 1))
        if null_col is not None:
            col[null_col] = None
        return (self.off.ctypes.data_as(_I64P) if offsets else None, c if y else None, col if cols else None,
                self.out.ctypes.data_as(_DP) if out else None)

    def device(self, p=2, offsets=True, y=True, out=True, null_col=None, cols=True):
        f = C.c_void_p(self.y.ctypes.data)
        col = (C.c_void_p * max(p, 1))(*[f] * max(p, 1))
        if null_col is not None:
            col[null_col] = None
        return (f if offsets else None, f if y else None, col if cols else None, f if out else None)

    def data(self, n=N, p=2, lens=None):
        a = self.abi.AnofoxDataArray
        c = self.y.ctypes.data_as(_DP)
        lens = lens if lens is not None else [n] * p
        xs = (a * max(p, 1))(*[a(c, None, ln) for ln in (lens or [n])])
        return a(c, None, n), xs


# ---- the batch entries: (name, flavour, call(env, G, p, n_rows, off, y, cols, out) -> bool) ----
def _rls(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipRlsBatchOptions(True, 0.99, 100.0)
    return getattr(e.lib, "anofox_hip_rls_fit_batch_" + form)(None, G, p, n, off, y, cols, o, out, C.byref(e.err))


def _quantile(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-9)
    return getattr(e.lib, "anofox_hip_quantile_fit_batch_" + form)(None, G, p, n, off, y, cols, o, out, None, C.byref(e.err))


def _quantile_path(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-9)
    return getattr(e.lib, "anofox_hip_quantile_fit_path_batch_" + form)(None, G, p, n, off, y, cols, o, e.taus.ctypes.data_as(_DP), 2, out,
                                                                         None, C.byref(e.err))


def _quantile_window(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-9)
    fr = e.abi.AnofoxHipWindowFrame(5, 0)
    return getattr(e.lib, "anofox_hip_quantile_fit_predict_window_" + form)(None, G, p, n, off, y, cols, fr, o, out, None, None, C.byref(e.err))


def _quantile_frames(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipQuantileBatchOptions(0.5, True, 1000, 1e-9)
    lo = off  # (any non-NULL pointer: never read)
    return getattr(e.lib, "anofox_hip_quantile_fit_predict_frames_" + form)(None, n, p, y, cols, lo, lo, o, out, None, None, C.byref(e.err))


def _glm(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    return getattr(e.lib, "anofox_hip_glm_fit_batch_" + form)(None, G, p, n, off, y, cols, None, o, out, None, C.byref(e.err))


def _glm_window(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    fr = e.abi.AnofoxHipWindowFrame(5, 0)
    return getattr(e.lib, "anofox_hip_glm_fit_predict_window_" + form)(None, G, p, n, off, y, cols, None, fr, o, 0.0, out, None, C.byref(e.err))


def _glm_frames(e, form, G, p, n, off, y, cols, out):
    o = e.abi.AnofoxHipGlmBatchOptions(0, True, 100, 1e-8, 0.0, False, 0.95)
    lo = off  # (any non-NULL pointer: never read)
    return getattr(e.lib, "anofox_hip_glm_fit_predict_frames_" + form)(None, n, p, y, cols, None, lo, lo, o, 0.0, out, None, C.byref(e.err))


# bad argument -> (keyword changes of a good call, expected text); the last rows have TWO bad arguments: the first check wins
def batch_rows(wide_p, wide_text, out_null, by_rows):
    rows = [("negative-rows", dict(n=-1), NEG), ("no-features", dict(p=0), X_EMPTY), ("null-x", dict(cols=False), X_EMPTY),
            ("too-wide", dict(p=wide_p), wide_text), ("null-y", dict(y=False), out_null), ("null-out", dict(out=False), out_null),
            ("null-column", dict(null_col=1), COL_NULL),
            ("negative-rows+no-features", dict(n=-1, p=0), NEG), ("no-features+null-y", dict(p=0, y=False), X_EMPTY),
            ("too-wide+null-out", dict(p=wide_p, out=False), wide_text), ("null-out+null-column", dict(out=False, null_col=0), out_null)]
    if not by_rows:
        rows += [("negative-groups", dict(G=-1), NEG), ("null-offsets", dict(offsets=False), out_null),
                 ("negative-groups+null-x", dict(G=-1, cols=False), NEG)]
    return rows


BATCH = []
for _name, _fn, _wide_p, _wide_text, _out_null, _by_rows in (
        ("rls", _rls, 129, WIDE, OUT_NULL, False), ("quantile", _quantile, 33, Q_WIDE, OUT_NULL, False),
        ("quantile_path", _quantile_path, 33, Q_WIDE, OUT_NULL, False), ("glm", _glm, 33, G_WIDE, OUT_NULL, False),
        ("glm_window", _glm_window, 33, G_WIDE, "y or pred is NULL", True), ("glm_frames", _glm_frames, 33, G_WIDE, "y or pred is NULL", True),
        ("quantile_window", _quantile_window, 33, Q_WIDE, "y or pred is NULL", True),
        ("quantile_frames", _quantile_frames, 33, Q_WIDE, "y or pred is NULL", True)):
    for _form in ("host", "device"):
        for _case, _kw, _text in batch_rows(_wide_p, _wide_text, _out_null, _by_rows):
            BATCH.append(pytest.param(_fn, _form, _kw, _text, id="%s_%s-%s" % (_name, _form, _case)))
    # the context is asked for after the arguments: a good device call with ctx == NULL
    BATCH.append(pytest.param(_fn, "device", dict(), CTX, id="%s_device-null-context" % _name))


@pytest.fixture(scope="module")
def env():
    return Env()


@pytest.mark.parametrize("fn,form,kw,text", BATCH)
def test_batch_entry(env, fn, form, kw, text):
    kw = dict(kw)
    G, n, p = kw.pop("G", 1), kw.pop("n", N), kw.get("p", 2)
    off, y, cols, out = (env.host if form == "host" else env.device)(**kw)
    assert not fn(env, form, G, p, n, off, y, cols, out)
    assert (env.err.code, env.err.text()) == (INPUT, text)


# ---- ctx == NULL on the entries that ask for the context first (elastic net, BLS, OLS device forms): it wins over everything ----
def test_context_first_entries(env):
    e, lib = env, env.lib
    f = C.c_void_p(e.y.ctypes.data)
    cols = (C.c_void_p * 2)(f, f)
    en = e.abi.AnofoxHipElasticNetBatchOptions(True, 0.1, 0.5, 100, -1.0, 0)   # (a bad tolerance as well)
    bls = e.abi.AnofoxHipBlsBatchOptions(True, None, 0, None, 0, 100, -1.0)
    ols = e.abi.AnofoxHipBatchOptions()
    for p, G in ((2, 1), (0, -1)):  # a good call, and one with two more bad arguments
        assert not lib.anofox_hip_elasticnet_fit_batch_device(None, G, p, N, f, f, cols, en, f, None, C.byref(e.err))
        assert (e.err.code, e.err.text()) == (INPUT, CTX)
        assert not lib.anofox_hip_bls_fit_batch_device(None, G, p, N, f, f, cols, bls, f, None, C.byref(e.err))
        assert (e.err.code, e.err.text()) == (INPUT, CTX)
        assert not lib.anofox_hip_fit_batch_device(None, G, p, N, f, f, cols, None, ols, f, None, C.byref(e.err))
        assert (e.err.code, e.err.text()) == (INPUT, CTX)


# ---- the one-group entries: call(env, y, xs, x_count, out=True, **options) ----
# `tail`: the optional outputs after the result (inference, the logistic extras), passed as NULL; `weights`: the entry takes a
# weights array before its options, of y's length unless the row says otherwise (wlen); opt_cls None: the entry has no options
def _scalar(sym, opt_cls, res_cls, defaults, extra=(), tail=0, weights=False):
    def call(e, y, xs, count, out=True, wlen=None, **o):
        args = [y, xs, count]
        if weights:
            args.append(e.abi.AnofoxDataArray(e.y.ctypes.data_as(_DP), None, y.len if wlen is None else wlen))
        if opt_cls:
            opts = getattr(e.abi, opt_cls)()
            for k, v in {**defaults, **o}.items():
                setattr(opts, k, v)
            args.append(opts)
        res = getattr(e.abi, res_cls)()
        return getattr(e.lib, sym)(*args, *[x(e) for x in extra], C.byref(res) if out else None, *[None] * tail, C.byref(e.err))
    return call


_GLM = dict(fit_intercept=True, max_iterations=25, tolerance=1e-8, confidence_level=0.95)
_taus = lambda e: e.taus.ctypes.data_as(_DP)  # noqa: E731
SCALAR = {
    "elasticnet": (_scalar("anofox_elasticnet_fit", "AnofoxElasticNetOptions", "AnofoxFitResultCore",
                           dict(alpha=0.1, l1_ratio=0.5, fit_intercept=True, max_iterations=100, tolerance=1e-6)),
                   "out_core is NULL", 129, "Elastic Net fit: more than 128 features are not supported by the GPU path"),
    "bls": (_scalar("anofox_bls_fit", "AnofoxBlsOptions", "AnofoxBlsFitResultCore", dict(fit_intercept=True, max_iterations=100, tolerance=1e-10)),
            "out_result is NULL", 129, "BLS fit: more than 128 features are not supported by the GPU path"),
    "rls": (_scalar("anofox_rls_fit", "AnofoxRlsOptions", "AnofoxFitResultCore", dict(forgetting_factor=0.99, fit_intercept=True, initial_p_diagonal=100.0)),
            "out_core is NULL", 129, "RLS fit: more than 128 features are not supported by the GPU path"),
    "quantile": (_scalar("anofox_quantile_fit", "AnofoxQuantileOptions", "AnofoxQuantileFitResultCore",
                         dict(tau=0.5, fit_intercept=True, max_iterations=1000, tolerance=1e-9)), "out_core is NULL", 33, Q_WIDE),
    "quantile_path": (_scalar("anofox_quantile_fit_path", "AnofoxQuantileOptions", "AnofoxQuantileFitResultCore",
                              dict(tau=0.5, fit_intercept=True, max_iterations=1000, tolerance=1e-9), extra=(_taus, lambda e: 2)),
                      "out_results is NULL", 33, Q_WIDE),
    "ols": (_scalar("anofox_ols_fit", "AnofoxOlsOptions", "AnofoxFitResultCore", dict(fit_intercept=True, confidence_level=0.95), tail=1),
            "out_core is NULL", 129, "OLS fit: more than 128 features are not supported by the GPU path"),
    "ridge": (_scalar("anofox_ridge_fit", "AnofoxRidgeOptions", "AnofoxFitResultCore", dict(alpha=1.0, fit_intercept=True, confidence_level=0.95),
                      tail=1),
              "out_core is NULL", 129, "Ridge fit: more than 128 features are not supported by the GPU path"),
    "wls": (_scalar("anofox_wls_fit", "AnofoxWlsOptions", "AnofoxFitResultCore", dict(fit_intercept=True, confidence_level=0.95), tail=1,
                    weights=True),
            "out_core is NULL", 129, "WLS fit: more than 128 features are not supported by the GPU path"),
    "nnls": (_scalar("anofox_nnls_fit", None, "AnofoxBlsFitResultCore", {}),
             "out_result is NULL", 129, "BLS fit: more than 128 features are not supported by the GPU path"),
    "poisson": (_scalar("anofox_poisson_fit", "AnofoxPoissonOptions", "AnofoxGlmFitResultCore", _GLM, tail=1), "out_core is NULL", 33, G_WIDE),
    "binomial": (_scalar("anofox_binomial_fit", "AnofoxBinomialOptions", "AnofoxGlmFitResultCore", _GLM, tail=1), "out_core is NULL", 33, G_WIDE),
    "logistic": (_scalar("anofox_logistic_fit", "AnofoxLogisticOptions", "AnofoxGlmFitResultCore", dict(_GLM, threshold=0.5), tail=2),
                 "out_core is NULL", 33, G_WIDE),
}
BAD_ALPHA = (ALPHA, "Invalid alpha parameter: -1 (must be >= 0)")
BAD_L1 = (L1, "Invalid L1 ratio: 1.5 (must be in [0, 1])")
BAD_TAU = (INPUT, "Invalid value for tau: tau must be in (0, 1)")


def scalar_rows():
    rows = []
    for name, (call, out_text, wide_p, wide_text) in SCALAR.items():
        empty = (INPUT, "Empty input: x[0] cannot be empty") if name == "rls" else (INPUT, Y_EMPTY)
        # (y of N rows against a first column of N - 1: the RLS entry compares y with x[0] first, every other entry each column with y)
        rows += [(name, "null-out", dict(out=False), (INPUT, out_text)), (name, "null-x", dict(x=None), (INPUT, X_EMPTY)),
                 (name, "no-x", dict(count=0), (INPUT, X_EMPTY)), (name, "empty", dict(n=0), empty),
                 (name, "mismatch-first", dict(lens=[N - 1, N]), (MISMATCH, mismatch(N, N - 1))),
                 (name, "mismatch-second", dict(lens=[N, N + 2]), (MISMATCH, mismatch(N, N + 2))),
                 (name, "too-wide", dict(p=wide_p), (INPUT, wide_text)),
                 # two bad arguments: the first check wins
                 (name, "null-out+no-x", dict(out=False, count=0), (INPUT, out_text)),
                 (name, "no-x+empty", dict(count=0, n=0), (INPUT, X_EMPTY)),
                 (name, "empty+mismatch", dict(n=0, lens=[0, 3]), empty),
                 (name, "mismatch+too-wide", dict(p=wide_p, lens=[N] * (wide_p - 1) + [N + 1]), (MISMATCH, mismatch(N, N + 1)))]
    rows += [("elasticnet", "alpha", dict(o=dict(alpha=-1.0)), BAD_ALPHA), ("elasticnet", "l1-ratio", dict(o=dict(l1_ratio=1.5)), BAD_L1),
             ("elasticnet", "alpha+l1-ratio", dict(o=dict(alpha=-1.0, l1_ratio=1.5)), BAD_ALPHA),
             ("elasticnet", "l1-ratio+empty", dict(o=dict(l1_ratio=1.5), n=0), BAD_L1),
             ("elasticnet", "no-x+alpha", dict(count=0, o=dict(alpha=-1.0)), (INPUT, X_EMPTY)),
             ("ridge", "alpha", dict(o=dict(alpha=-1.0)), BAD_ALPHA), ("ridge", "alpha+empty", dict(o=dict(alpha=-1.0), n=0), BAD_ALPHA),
             # WLS: the weights after y and before the columns
             ("wls", "empty-weights", dict(wlen=0), (INPUT, "Empty input: weights cannot be empty")),
             ("wls", "weights-mismatch", dict(wlen=N + 1), (MISMATCH, mismatch(N, N + 1))),
             ("wls", "empty+empty-weights", dict(n=0, wlen=0), (INPUT, Y_EMPTY)),
             ("wls", "empty-weights+mismatch", dict(wlen=0, lens=[N - 1, N]), (INPUT, "Empty input: weights cannot be empty")),
             ("wls", "weights-mismatch+mismatch", dict(wlen=N + 3, lens=[N - 1, N]), (MISMATCH, mismatch(N, N + 3))),
             ("wls", "weights-mismatch+too-wide", dict(wlen=N + 3, p=129), (MISMATCH, mismatch(N, N + 3))),
             ("quantile", "tau", dict(o=dict(tau=1.0)), BAD_TAU), ("quantile", "tau-nan", dict(o=dict(tau=float("nan"))), BAD_TAU),
             ("quantile", "empty+tau", dict(n=0, o=dict(tau=0.0)), (INPUT, Y_EMPTY)),
             ("quantile", "tau+mismatch", dict(o=dict(tau=0.0), lens=[N, N + 1]), BAD_TAU)]
    return [pytest.param(*r, id="%s-%s" % r[:2]) for r in rows]


@pytest.mark.parametrize("name,case,kw,expect", scalar_rows())
def test_scalar_entry(env, name, case, kw, expect):
    call = SCALAR[name][0]
    kw = dict(kw)
    p = kw.pop("p", 2)
    y, xs = env.data(n=kw.pop("n", N), p=p, lens=kw.pop("lens", None))
    if "x" in kw:
        xs = kw.pop("x")
    assert not call(env, y, xs, kw.pop("count", p), out=kw.pop("out", True), wlen=kw.pop("wlen", None), **kw.pop("o", {}))
    assert (env.err.code, env.err.text()) == expect


def test_quantile_path_taus(env):
    bad = np.array([0.5, 1.0])
    for taus, count, lens, text in ((None, 2, None, "taus is NULL or empty"), (env.taus, 0, None, "taus is NULL or empty"),
                                    (env.taus, 65, None, "quantile path: n_taus > 64 is not built"),
                                    (bad, 2, None, "Invalid value for tau: tau must be in (0, 1)"),
                                    (bad, 2, [N, N + 1], "Invalid value for tau: tau must be in (0, 1)"),   # tau before the lengths
                                    (None, 2, [N, N + 1], "taus is NULL or empty")):
        yy, xx = env.data(lens=lens)
        res = (env.abi.AnofoxQuantileFitResultCore * 2)()
        o = env.abi.AnofoxQuantileOptions(0.5, True, 1000, 1e-9)
        tp = taus.ctypes.data_as(_DP) if taus is not None else None
        assert not env.lib.anofox_quantile_fit_path(yy, xx, 2, o, tp, count, res, C.byref(env.err))
        assert (env.err.code, env.err.text()) == (INPUT, text)
