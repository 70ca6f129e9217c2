"""Bind-time options of the three aggregates — mirror of the reference's
RegressionMapOptions::ParseFromValue (src/include/map_options_parser.cpp:637-750),
ExtractBool (:21-45), ExtractSolverType / ExtractHcType / ExtractLambdaScaling (:222-266)
and GetRegularizationStrength (src/include/map_options_parser.hpp:265-270), with the
bind-data defaults of ols_aggregate.cpp:48-52, ridge_aggregate.cpp:49-54, wls_aggregate.cpp:49-54.

Keys are case-insensitive; unknown keys are silently ignored (map_options_parser.cpp:798);
`alpha` wins over `lambda`; there is no range check on confidence_level.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Mapping, Optional

from . import _abi


class InvalidInputException(ValueError):
    """Counterpart of duckdb::InvalidInputException for option / input errors."""


def _extract_bool(val: Any) -> Optional[bool]:
    if val is None:
        return None
    if isinstance(val, bool):
        return val
    if isinstance(val, int):
        return val != 0
    if isinstance(val, float):
        return val != 0.0
    try:  # DECIMAL-like
        import decimal
        if isinstance(val, decimal.Decimal):
            return val != 0
    except Exception:  # pragma: no cover
        pass
    raise InvalidInputException(f"Cannot convert value of type {type(val).__name__.upper()} to boolean")


def _extract_double(val: Any) -> Optional[float]:
    return None if val is None else float(val)


def _extract_enum(val: Any, table: Mapping[str, int], what: str, valid: str) -> Optional[str]:
    if val is None:
        return None
    s = str(val).lower()
    if s not in table:
        raise InvalidInputException(f"Invalid {what}: '{s}'. Valid values are {valid}")
    return s


ALTERNATIVE = {"two_sided": 0, "two-sided": 0, "two.sided": 0, "twosided": 0, "less": 1, "greater": 2}


def _extract_alternative(val: Any) -> int:
    """The `alternative` key of the correlation and rank test options (case-insensitive) as the reference's AnofoxAlternative."""
    name = str(val).lower()
    if name not in ALTERNATIVE:
        raise InvalidInputException("Unknown alternative '%s'. Expected 'two_sided', 'less' or 'greater'." % (val,))
    return ALTERNATIVE[name]


@dataclass
class RegressionOptions:
    """Resolved options (defaults = the C++ bind data of the aggregates)."""
    fit_intercept: bool = True
    compute_inference: bool = False
    confidence_level: float = 0.95
    alpha: float = 1.0                 # ridge_aggregate.cpp:49
    solver: str = "svd"                # ols_aggregate.cpp:51 (accepted, ignored by the GPU path)
    hc_type: str = "none"
    lambda_scaling: str = "raw"
    null_policy: str = "drop"          # predict aggregates only (ols_predict_aggregate.cpp:68)

    def batch_options(self, model: str) -> _abi.AnofoxHipBatchOptions:
        return _abi.AnofoxHipBatchOptions(
            _abi.MODEL[model], self.fit_intercept, self.compute_inference, self.confidence_level, self.alpha,
            _abi.SOLVER[self.solver], _abi.LAMBDA_SCALING[self.lambda_scaling], _abi.HC_TYPE[self.hc_type])


def parse_options(opts: Optional[Mapping[str, Any]]) -> RegressionOptions:
    """Parse a constant MAP / STRUCT literal, given as a Python mapping."""
    out = RegressionOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    alpha = lam = None
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("compute_inference", "inference"):
            v = _extract_bool(val)
            if v is not None:
                out.compute_inference = v
        elif key in ("confidence_level", "confidence"):
            v = _extract_double(val)
            if v is not None:
                out.confidence_level = v
        elif key == "alpha":
            alpha = _extract_double(val)
        elif key == "lambda":
            lam = _extract_double(val)
        elif key == "solver":
            v = _extract_enum(val, _abi.SOLVER, "solver", "'qr', 'svd', 'cholesky'")
            if v is not None:
                out.solver = v
        elif key == "hc_type":
            v = _extract_enum(val, _abi.HC_TYPE, "hc_type", "'none', 'hc0', 'hc1', 'hc2', 'hc3'")
            if v is not None:
                out.hc_type = v
        elif key == "lambda_scaling":
            v = _extract_enum(val, _abi.LAMBDA_SCALING, "lambda_scaling", "'raw', 'glmnet'")
            if v is not None:
                out.lambda_scaling = v
        elif key == "null_policy":
            if val is not None:
                v = str(val).lower()
                if v not in ("drop", "drop_y_zero_x"):
                    raise InvalidInputException(
                        f"Invalid null_policy: '{v}'. Valid values are 'drop', 'drop_y_zero_x'")
                out.null_policy = v
        # every other key: ignored, as in the reference
    if alpha is not None:      # GetRegularizationStrength: alpha first, then lambda
        out.alpha = alpha
    elif lam is not None:
        out.alpha = lam
    return out


@dataclass
class ElasticNetOptions:
    """Resolved options of the elastic net (defaults = the reference's ElasticNetOptions bind data)."""
    alpha: float = 1.0
    l1_ratio: float = 0.5
    fit_intercept: bool = True
    max_iterations: int = 1000
    tolerance: float = 1e-6
    lambda_scaling: str = "raw"

    def batch_options(self) -> _abi.AnofoxHipElasticNetBatchOptions:
        return _abi.AnofoxHipElasticNetBatchOptions(self.fit_intercept, self.alpha, self.l1_ratio, self.max_iterations,
                                                    self.tolerance, _abi.LAMBDA_SCALING[self.lambda_scaling])

    def ffi_options(self) -> _abi.AnofoxElasticNetOptions:
        return _abi.AnofoxElasticNetOptions(self.alpha, self.l1_ratio, self.fit_intercept, self.max_iterations,
                                            self.tolerance, _abi.LAMBDA_SCALING[self.lambda_scaling])


@dataclass
class ElasticNetPredictOptions(ElasticNetOptions):
    """Options of the elastic net fit-predict family (anofox_stats_elasticnet_fit_predict_agg and
    anofox_stats_elasticnet_fit_predict): the elastic net options plus the interval's confidence level and the null policy
    (defaults of elasticnet_predict_aggregate.cpp:40-44)."""
    confidence_level: float = 0.95
    null_policy: str = "drop"


def _extract_uint32(val: Any) -> Optional[int]:
    if val is None:
        return None
    v = int(val)
    if v < 0 or v > 0xFFFFFFFF:
        raise InvalidInputException(f"Value {v} is out of range for UINTEGER")
    return v


def parse_elasticnet_options(opts: Optional[Mapping[str, Any]]) -> ElasticNetOptions:
    """The elastic net's MAP options (map_options_parser.cpp:637-750 with the keys of :651-656): alpha / lambda
    (alpha wins), l1_ratio, fit_intercept / intercept, max_iterations / max_iter, tolerance / tol, lambda_scaling.
    Keys are case-insensitive; unknown keys are ignored."""
    out = ElasticNetOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    alpha = lam = None
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key == "alpha":
            alpha = _extract_double(val)
        elif key == "lambda":
            lam = _extract_double(val)
        elif key == "l1_ratio":
            v = _extract_double(val)
            if v is not None:
                out.l1_ratio = v
        elif key in ("max_iterations", "max_iter"):
            v = _extract_uint32(val)
            if v is not None:
                out.max_iterations = v
        elif key in ("tolerance", "tol"):
            v = _extract_double(val)
            if v is not None:
                out.tolerance = v
        elif key == "lambda_scaling":
            v = _extract_enum(val, _abi.LAMBDA_SCALING, "lambda_scaling", "'raw', 'glmnet'")
            if v is not None:
                out.lambda_scaling = v
    if alpha is not None:      # GetRegularizationStrength: alpha first, then lambda
        out.alpha = alpha
    elif lam is not None:
        out.alpha = lam
    return out


def parse_elasticnet_predict_options(opts: Optional[Mapping[str, Any]], use_lambda: bool = True) -> ElasticNetPredictOptions:
    """Options of the elastic net fit-predict family: parse_elasticnet_options plus confidence_level / confidence and
    null_policy ('drop', 'drop_y_zero_x').  use_lambda=False is the fit-predict aggregate's bind, which reads opts.alpha
    only (elasticnet_predict_aggregate.cpp:405-431): a `lambda` key is ignored there, while the window function's bind
    uses GetRegularizationStrength (alpha wins over lambda)."""
    base = parse_elasticnet_options(opts)
    out = ElasticNetPredictOptions(**vars(base))
    if opts is None:
        return out
    has_alpha = False
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "alpha" and val is not None:
            has_alpha = True
        elif key in ("confidence_level", "confidence"):
            v = _extract_double(val)
            if v is not None:
                out.confidence_level = v
        elif key == "null_policy":
            if val is not None:
                v = str(val).lower()
                if v not in ("drop", "drop_y_zero_x"):
                    raise InvalidInputException(
                        f"Invalid null_policy: '{v}'. Valid values are 'drop', 'drop_y_zero_x'")
                out.null_policy = v
    if not use_lambda and not has_alpha:
        out.alpha = ElasticNetPredictOptions.alpha
    return out


@dataclass
class BlsOptions:
    """Resolved options of bounded least squares (defaults = the bind data of bls_aggregate.cpp:49-55 and
    bls_fit_predict_aggregate.cpp:67-76).  lower_bound / upper_bound: None = that side absent, a number = every column, a
    sequence = per column (the SQL MAP only carries a number); both absent = NNLS."""
    fit_intercept: bool = False
    lower_bound: Any = None
    upper_bound: Any = None
    max_iterations: int = 1000
    tolerance: float = 1e-10
    confidence_level: float = 0.95
    null_policy: str = "drop"

    def _bounds(self):
        import numpy as np
        out = []
        for b in (self.lower_bound, self.upper_bound):
            out.append(None if b is None else np.ascontiguousarray(np.atleast_1d(np.asarray(b, dtype=np.float64))))
        return out

    def batch_options(self) -> _abi.AnofoxHipBlsBatchOptions:
        return self._fill(_abi.AnofoxHipBlsBatchOptions())

    def ffi_options(self) -> _abi.AnofoxBlsOptions:
        return self._fill(_abi.AnofoxBlsOptions())

    def _fill(self, o):
        import ctypes as C
        lo, hi = self._bounds()
        o.fit_intercept = self.fit_intercept
        o.lower_bounds = None if lo is None else lo.ctypes.data_as(C.POINTER(C.c_double))
        o.lower_bounds_len = 0 if lo is None else len(lo)
        o.upper_bounds = None if hi is None else hi.ctypes.data_as(C.POINTER(C.c_double))
        o.upper_bounds_len = 0 if hi is None else len(hi)
        o.max_iterations = self.max_iterations
        o.tolerance = self.tolerance
        o._keepalive = (lo, hi)          # the struct points into these arrays
        return o


def _parse_bls(opts: Optional[Mapping[str, Any]], bounds: bool, predict: bool) -> BlsOptions:
    out = BlsOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("max_iterations", "max_iter"):
            v = _extract_uint32(val)
            if v is not None:
                out.max_iterations = v
        elif key in ("tolerance", "tol"):
            v = _extract_double(val)
            if v is not None:
                out.tolerance = v
        elif key in ("lower_bound", "lower", "upper_bound", "upper"):
            if val is None:
                continue
            v = [_extract_double(e) for e in val] if isinstance(val, (list, tuple)) or hasattr(val, "__array__") else _extract_double(val)
            if bounds:                                   # (nnls: parsed by the shared parser, never read)
                if key.startswith("lower"):
                    out.lower_bound = v
                else:
                    out.upper_bound = v
        elif key in ("confidence_level", "confidence"):
            v = _extract_double(val)
            if v is not None and predict:
                out.confidence_level = v
        elif key == "null_policy":
            if val is not None:
                v = str(val).lower()
                if v not in ("drop", "drop_y_zero_x"):
                    raise InvalidInputException(
                        f"Invalid null_policy: '{v}'. Valid values are 'drop', 'drop_y_zero_x'")
                if predict:
                    out.null_policy = v
    return out


def parse_bls_options(opts: Optional[Mapping[str, Any]]) -> BlsOptions:
    """anofox_stats_bls_fit_agg's MAP options (bls_aggregate.cpp:340-366): fit_intercept / intercept, lower_bound / lower,
    upper_bound / upper, max_iterations / max_iter, tolerance / tol.  Keys are case-insensitive; other keys are ignored."""
    return _parse_bls(opts, bounds=True, predict=False)


def parse_nnls_options(opts: Optional[Mapping[str, Any]]) -> BlsOptions:
    """anofox_stats_nnls_fit_agg's MAP options (bls_aggregate.cpp:370-396): fit_intercept, max_iterations and tolerance
    only — bound keys are silently ignored, the fit is always the non-negative one."""
    return _parse_bls(opts, bounds=False, predict=False)


def parse_bls_predict_options(opts: Optional[Mapping[str, Any]]) -> BlsOptions:
    """anofox_stats_bls_fit_predict_agg's MAP options: parse_bls_options plus confidence_level / confidence (default 0.95)
    and null_policy ('drop', 'drop_y_zero_x')."""
    return _parse_bls(opts, bounds=True, predict=True)


@dataclass
class QuantileOptions:
    """Resolved options of quantile regression (defaults = the bind data of quantile_fit_predict_aggregate.cpp:54-57 and the
    reference's QuantileOptions: tau 0.5, an intercept, 1000 iterations, tolerance 1e-6 — accepted and unused, the fit is the
    exact vertex)."""
    tau: float = 0.5
    fit_intercept: bool = True
    max_iterations: int = 1000
    tolerance: float = 1e-6
    null_policy: str = "drop"

    def batch_options(self) -> _abi.AnofoxHipQuantileBatchOptions:
        return _abi.AnofoxHipQuantileBatchOptions(self.tau, self.fit_intercept, self.max_iterations, self.tolerance)

    def ffi_options(self) -> _abi.AnofoxQuantileOptions:
        return _abi.AnofoxQuantileOptions(self.tau, self.fit_intercept, self.max_iterations, self.tolerance)


def parse_quantile_options(opts: Optional[Mapping[str, Any]]) -> QuantileOptions:
    """anofox_stats_quantile_fit_predict_agg's MAP options (quantile_fit_predict_aggregate.cpp): tau, fit_intercept /
    intercept; max_iterations / max_iter and tolerance / tol as the scalar function's.  Keys are case-insensitive; other keys
    are ignored.  tau is not range-checked here: the fit reports it (status 1 / InvalidInput)."""
    out = QuantileOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key == "tau":
            v = _extract_double(val)
            if v is not None:
                out.tau = v
        elif key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("max_iterations", "max_iter"):
            v = _extract_uint32(val)
            if v is not None:
                out.max_iterations = v
        elif key in ("tolerance", "tol"):
            v = _extract_double(val)
            if v is not None:
                out.tolerance = v
    return out


@dataclass
class QuantilePathOptions(QuantileOptions):
    """QuantileOptions with a grid: taus, in the caller's order; the inherited tau is unused."""
    taus: tuple = ()


def parse_quantile_path_options(opts: Optional[Mapping[str, Any]]) -> QuantilePathOptions:
    """The MAP options of the tau-path functions: taus (a non-empty list of numbers) and parse_quantile_options' other keys.
    The key tau is rejected: a path takes its quantiles from taus.  The values are not range-checked here: the fit reports
    them (status 1 / InvalidInput)."""
    if opts is None or not isinstance(opts, Mapping):
        if opts is not None:
            raise InvalidInputException("Options parameter must be a constant expression")
        raise InvalidInputException("the quantile path needs the option 'taus': a non-empty list of quantiles")
    keys = {str(k).lower(): k for k in opts}
    if "tau" in keys:
        raise InvalidInputException("the quantile path takes a list of quantiles in 'taus', not 'tau'")
    raw = opts[keys["taus"]] if "taus" in keys else None
    if raw is None or isinstance(raw, (str, bytes)) or not (isinstance(raw, (list, tuple)) or hasattr(raw, "__array__")):
        raise InvalidInputException("the quantile path needs the option 'taus': a non-empty list of quantiles")
    taus = []
    for e in list(raw):
        v = _extract_double(e)
        taus.append(float("nan") if v is None else v)        # a NULL element is an invalid quantile, reported by the fit
    if not taus:
        raise InvalidInputException("the quantile path needs the option 'taus': a non-empty list of quantiles")
    base = parse_quantile_options({k: v for k, v in opts.items() if str(k).lower() != "taus"})
    return QuantilePathOptions(tau=base.tau, fit_intercept=base.fit_intercept, max_iterations=base.max_iterations,
                               tolerance=base.tolerance, null_policy=base.null_policy, taus=tuple(taus))


@dataclass
class RlsOptions:
    """Resolved options of recursive least squares (defaults = the reference's RlsOptions and the bind data of
    rls_aggregate.cpp / rls_predict_aggregate.cpp / rls_fit_predict.cpp)."""
    forgetting_factor: float = 1.0
    initial_p_diagonal: float = 100.0
    fit_intercept: bool = True
    confidence_level: float = 0.95
    null_policy: str = "drop"

    def batch_options(self) -> _abi.AnofoxHipRlsBatchOptions:
        return _abi.AnofoxHipRlsBatchOptions(self.fit_intercept, self.forgetting_factor, self.initial_p_diagonal)

    def ffi_options(self) -> _abi.AnofoxRlsOptions:
        return _abi.AnofoxRlsOptions(self.forgetting_factor, self.fit_intercept, self.initial_p_diagonal)


def parse_rls_options(opts: Optional[Mapping[str, Any]]) -> RlsOptions:
    """The RLS functions' MAP options through the shared parser (map_options_parser.cpp:637-681): forgetting_factor,
    initial_p_diagonal / p_diagonal, fit_intercept / intercept, confidence_level / confidence and null_policy are read.
    Every other key is ignored — `lambda` included: the reference's own tests pass {'lambda': 0.99}, which the parser
    stores as a regularisation strength that RLS never reads, so the forgetting factor stays 1.0.  A value the shared
    parser cannot convert is still an error, whichever key it sits under."""
    out = RlsOptions()
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("compute_inference", "inference"):
            _extract_bool(val)
        elif key in ("confidence_level", "confidence"):
            v = _extract_double(val)
            if v is not None:
                out.confidence_level = v
        elif key == "forgetting_factor":
            v = _extract_double(val)
            if v is not None:
                out.forgetting_factor = v
        elif key in ("initial_p_diagonal", "p_diagonal"):
            v = _extract_double(val)
            if v is not None:
                out.initial_p_diagonal = v
        elif key == "null_policy":
            if val is not None:
                v = str(val).lower()
                if v not in ("drop", "drop_y_zero_x"):
                    raise InvalidInputException(
                        f"Invalid null_policy: '{v}'. Valid values are 'drop', 'drop_y_zero_x'")
                out.null_policy = v
        elif key in ("alpha", "lambda", "l1_ratio", "tolerance", "tol", "epsilon"):
            _extract_double(val)                     # parsed by the shared parser, not read by RLS
        elif key in ("max_iterations", "max_iter"):
            _extract_uint32(val)
        elif key == "lambda_scaling":
            _extract_enum(val, _abi.LAMBDA_SCALING, "lambda_scaling", "'raw', 'glmnet'")
    return out


@dataclass
class GlmOptions:
    """Resolved options of the GLM family (the reference's PoissonOptions / BinomialOptions defaults: an intercept, 100 IRLS
    iterations, tolerance 1e-8, lambda 0, no inference, confidence 0.95).  offset: the 1-based index into x of the offset column
    (0 = none), as the reference's offset_column."""
    family: str = "poisson"
    fit_intercept: bool = True
    max_iterations: int = 100
    tolerance: float = 1e-8
    lambda_: float = 0.0
    link: str = ""
    compute_inference: bool = False
    confidence_level: float = 0.95
    offset: int = 0

    def batch_options(self) -> "_abi.AnofoxHipGlmBatchOptions":
        return _abi.AnofoxHipGlmBatchOptions(_abi.GLM_FAMILY[self.family], self.fit_intercept, self.max_iterations, self.tolerance,
                                             self.lambda_, self.compute_inference, self.confidence_level)


_GLM_LINKS = {"poisson": ("log", ("identity", "sqrt")), "binomial": ("logit", ("probit", "cloglog"))}


def _parse_glm(opts: Optional[Mapping[str, Any]], family: str) -> GlmOptions:
    out = GlmOptions(family=family, link=_GLM_LINKS[family][0])
    if opts is None:
        return out
    if not isinstance(opts, Mapping):
        raise InvalidInputException("Options parameter must be a constant expression")
    for raw_key, val in opts.items():
        key = str(raw_key).lower()
        if key in ("intercept", "fit_intercept"):
            v = _extract_bool(val)
            if v is not None:
                out.fit_intercept = v
        elif key in ("max_iterations", "max_iter"):
            v = _extract_uint32(val)
            if v is not None:
                out.max_iterations = v
        elif key in ("tolerance", "tol"):
            v = _extract_double(val)
            if v is not None:
                out.tolerance = v
        elif key == "lambda":
            v = _extract_double(val)
            if v is not None:
                out.lambda_ = v
        elif key == "compute_inference":
            v = _extract_bool(val)
            if v is not None:
                out.compute_inference = v
        elif key == "confidence_level":
            v = _extract_double(val)
            if v is not None:
                out.confidence_level = v
        elif key == "offset":
            v = _extract_uint32(val)
            if v is not None:
                out.offset = v
        elif key == "link" and val is not None:
            out.link = str(val).lower()
        elif key == "vcov" and val is not None and str(val).lower() != "laplace":
            raise InvalidInputException("glm: vcov %s is not built" % str(val).lower())
        elif key in ("priors", "prior") and val is not None:
            raise InvalidInputException("glm: priors are not built")
    if out.link != _GLM_LINKS[family][0]:
        raise InvalidInputException("glm: link %s is not built" % out.link)
    return out


def parse_poisson_options(opts: Optional[Mapping[str, Any]]) -> GlmOptions:
    """poisson_fit_agg's MAP options: fit_intercept / intercept, max_iterations / max_iter, tolerance / tol, lambda, link (only
    'log' is built), compute_inference, confidence_level, offset.  Keys are case-insensitive; other keys are ignored, except that
    vcov other than 'laplace' and priors fail with "not built" (the contract: they fail the call, they are not dropped).  The
    values are not range-checked here: the fit reports them (status 1 / InvalidInput)."""
    return _parse_glm(opts, "poisson")


def parse_binomial_options(opts: Optional[Mapping[str, Any]]) -> GlmOptions:
    """binomial_fit_agg's / logistic_fit_agg's MAP options: parse_poisson_options' keys; only the 'logit' link is built."""
    return _parse_glm(opts, "binomial")
