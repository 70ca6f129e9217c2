"""Contexts, the streaming aggregate state and the batch entry points (host pointers / device pointers).

Every entry is stated once, as its contract on a checked batch `b` (_marshal.HostBatch or _marshal.DeviceBatch): which inputs,
which output shapes, which symbol, what it returns.  The `*_host` functions and the `Context.*_device` methods below put their
arguments into the batch of their kind and run that contract."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError
from ._marshal import F64, I32, I64, U8, U32, DeviceBatch, HostBatch, call, create, handle, host_array

FRAME_UNBOUNDED = 2 ** 63 - 1        # ANOFOX_HIP_FRAME_UNBOUNDED


def _frame(frame) -> _abi.AnofoxHipWindowFrame:
    """(start, end) in rows PRECEDING the current row (negative = FOLLOWING); start None = UNBOUNDED PRECEDING,
    end None = UNBOUNDED FOLLOWING."""
    start, end = frame
    return _abi.AnofoxHipWindowFrame(FRAME_UNBOUNDED if start is None else int(start),
                                     -FRAME_UNBOUNDED if end is None else int(end))


# ---- the contracts, each for both kinds of batch -----------------------------------------------------------------------------

def _fit(b, w, options, core=None, inference=None):
    core = b.out((b.G, b.p + 6), given=core)
    want = bool(options.compute_inference)
    inf = b.out((b.G, 5 * b.p + 2), given=inference) if want or inference is not None else None
    b.call("anofox_hip_fit_batch", *b.head, b.rows(w, "w"), options, core, inf)
    return core, (inf if want else None)


def _fit_predict(b, w, options, train_counts, core=None, pred=None):
    core, pred = b.out((b.G, b.p + 6), given=core), b.out((b.N, 3), given=pred)
    b.call("anofox_hip_fit_predict_batch", *b.head, b.rows(w, "w"), b.groups(train_counts, "train_counts"), options, core, pred)
    return core, pred


def _fit_predict_window(b, w, options, frame, pred=None):
    pred = b.out((b.N, 3), given=pred)
    b.call("anofox_hip_fit_predict_window", *b.head, b.rows(w, "w"), _frame(frame), options, pred)
    return pred


def _information_criteria(b, core, options, out=None):
    core = b.array(core, F64, None, "core")
    G, p = int(core.shape[0]), int(core.shape[1]) - 6
    out = b.out((G, 3), given=out)
    b.call("anofox_hip_information_criteria_batch", G, p, core, options, out)
    return out


def _vif(b, out=None):
    out = b.out((b.G, b.p + 1), given=out)
    b.call("anofox_hip_vif_batch", b.G, b.p, b.N, b.off, b.cols, out)
    return out


def _residuals(b, y_hat, rse, include_studentized, drop_nan_rows, out=None, group=None):
    out, group = b.out((b.N, 4), given=out), b.out((b.G, 2), given=group)
    b.call("anofox_hip_residuals_batch", b.G, b.p, b.N, b.off, b.y, b.array(y_hat, F64, b.N, "y_hat"), b.cols if b.p else None,
           b.groups(rse, "rse", F64), bool(include_studentized), bool(drop_nan_rows), out, group)
    return out, group


def _iterative_fit(b, family, record_len, options, records=None, iterations=None):
    """elasticnet / bls / quantile fit: (records[G, record_len], iterations int32[G])."""
    records, iterations = b.out((b.G, record_len), given=records), b.out((b.G,), I32, given=iterations)
    b.call(f"anofox_hip_{family}_fit_batch", *b.head, options, records, iterations)
    return records, iterations


def _quantile_fit_path(b, options, taus, records=None, iterations=None):
    tv = host_array(taus, F64).ravel()
    records = b.out((b.G, tv.size, b.p + 6), given=records)
    iterations = b.out((b.G, tv.size), I32, given=iterations)
    b.call("anofox_hip_quantile_fit_path_batch", *b.head, options, tv, tv.size, records, iterations)
    return records, iterations


def _family_fit_predict(b, family, options, confidence_level, train_counts, core=None, pred=None):
    """elasticnet / rls / bls fit + predict: (core[G, p+6], pred[N, 3])."""
    core, pred = b.out((b.G, b.p + 6), given=core), b.out((b.N, 3), given=pred)
    b.call(f"anofox_hip_{family}_fit_predict_batch", *b.head, b.groups(train_counts, "train_counts"), options,
           float(confidence_level), core, pred)
    return core, pred


def _family_window(b, family, options, confidence_level, pred=None, frame=None, bounds=None):
    """elasticnet / rls window fit + predict over a ROWS frame, or over explicit frames `bounds` = (frame_lo, frame_hi)."""
    pred = b.out((b.N, 3), given=pred)
    if bounds is None:
        b.call(f"anofox_hip_{family}_fit_predict_window", *b.head, _frame(frame), options, float(confidence_level), pred)
    else:
        b.call(f"anofox_hip_{family}_fit_predict_frames", *b.rows_head, *b.frames(*bounds), options, float(confidence_level), pred)
    return pred


def _quantile_window(b, options, want_records, frame=None, bounds=None):
    pred = b.out((b.N, 3))
    rec = b.out((b.N, b.p + 6)) if want_records else None
    its = b.out((b.N,), I32) if want_records else None
    if bounds is None:
        b.call("anofox_hip_quantile_fit_predict_window", *b.head, _frame(frame), options, pred, rec, its)
    else:
        b.call("anofox_hip_quantile_fit_predict_frames", *b.rows_head, *b.frames(*bounds), options, pred, rec, its)
    return (pred, rec, its) if want_records else pred


def _rls_fit(b, options, core=None):
    core = b.out((b.G, b.p + 6), given=core)
    b.call("anofox_hip_rls_fit_batch", *b.head, options, core)
    return core


class Context:
    """Owns one AnofoxHipContext (device + stream + reusable workspace)."""

    def __init__(self, device: int = -1):
        self._lib = _abi.load()
        self._h = create(self._lib, "anofox_hip_context_create", int(device))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.anofox_hip_context_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: Optional[int]):
        """Launch on the given hipStream_t handle.  0 is HIP's default stream (= torch's default stream) and is used
        as given; None goes back to the context's own non-blocking stream."""
        if hip_stream is None:
            call(self._lib, "anofox_hip_context_use_own_stream", self._h)
        else:
            call(self._lib, "anofox_hip_context_set_stream", self._h, int(hip_stream))

    def set_accumulate_gate(self, wait_event=None, record_event=None):
        """torch.cuda.Event objects (or None): wait for `wait_event` before the accumulate kernel of the next fit
        calls, record `record_event` right after it (see anofox_hip_context_set_accumulate_gate)."""
        h = lambda ev: None if ev is None else int(ev.cuda_event)
        # the library holds the raw hipEvent_t handles until the next fit call consumes the (one-shot) gate: keep the
        # torch objects alive at least that long, whatever the caller does with its own references
        self._gate_events = (wait_event, record_event)
        call(self._lib, "anofox_hip_context_set_accumulate_gate", self._h, h(wait_event), h(record_event))

    def synchronize(self):
        call(self._lib, "anofox_hip_context_synchronize", self._h)

    def enable_timing(self, enable: bool = True):
        call(self._lib, "anofox_hip_context_enable_timing", self._h, bool(enable))

    def collect_timing(self) -> dict:
        t = _abi.AnofoxHipKernelTimes()
        call(self._lib, "anofox_hip_context_collect_timing", self._h, C.byref(t))
        return {"accumulate_ms": t.accumulate_ms, "accumulate_count": t.accumulate_count,
                "solve_ms": t.solve_ms, "solve_count": t.solve_count,
                "predict_ms": t.predict_ms, "predict_count": t.predict_count,
                "accumulate_ms_min": t.accumulate_ms_min, "accumulate_ms_max": t.accumulate_ms_max}

    def _count(self, name) -> int:
        n = C.c_int64()
        call(self._lib, name, self._h, C.byref(n))
        return int(n.value)

    def last_window_refit_count(self) -> int:
        """Output rows of the most recent window call that were refitted with refinement (diagnostic)."""
        return self._count("anofox_hip_context_last_window_refit_count")

    def last_refine_count(self) -> int:
        """Groups of the most recent fit launch that took the on-device refinement passes (diagnostic)."""
        return self._count("anofox_hip_context_last_refine_count")

    # ---- device-resident batch (torch tensors on this context's GPU): row_offsets int64[G+1]; y, x_cols[j], w float64[N];
    # ---- train_counts int64[G]; frame_lo / frame_hi int64[N].  Asynchronous.  An output the caller passes is written and returned.
    def fit_batch_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                         core=None, inference=None, use_current_torch_stream: bool = True):
        """Returns (core[G, p+6], inference[G, 5p+2] or None) CUDA tensors."""
        return _fit(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), w, options, core, inference)

    def fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                 train_counts=None, core=None, pred=None, use_current_torch_stream: bool = True):
        """fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        return _fit_predict(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), w, options, train_counts, core, pred)

    def fit_predict_expanding_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                     pred=None, use_current_torch_stream: bool = True):
        """Expanding-window fit + predict, device resident.  Returns pred[N, 3] (CUDA tensor)."""
        return self.fit_predict_window_device(row_offsets, y, x_cols, w, options, (None, 0), pred, use_current_torch_stream)

    def fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                  frame=(None, 0), pred=None, use_current_torch_stream: bool = True):
        """Window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING (frame[0] None =
        UNBOUNDED), device resident.  Returns pred[N, 3] (CUDA tensor)."""
        return _fit_predict_window(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), w, options, frame, pred)

    def information_criteria_device(self, core, options: _abi.AnofoxHipBatchOptions, out=None, use_current_torch_stream: bool = True):
        """CUDA fit records [G, p+6] -> out[G, 3] = {rss, aic, bic}; asynchronous."""
        return _information_criteria(DeviceBatch(self, None, None, (), use_current_torch_stream), core, options, out)

    def vif_batch_device(self, row_offsets, x_cols: Sequence, out=None, use_current_torch_stream: bool = True):
        """Grouped variance inflation factors, device resident.  Returns out[G, p+1] = {vif[p], status}."""
        return _vif(DeviceBatch(self, row_offsets, None, x_cols, use_current_torch_stream), out)

    def residuals_batch_device(self, row_offsets, y, y_hat, x_cols: Sequence = (), rse=None, include_studentized: bool = True,
                               drop_nan_rows: bool = True, out=None, group=None, use_current_torch_stream: bool = True):
        """Grouped residual diagnostics, device resident (y_hat float64[N], rse float64[G] or None).  Returns (out[N, 4] = raw /
        standardized / studentized / leverage per row, group[G, 2] = rows used / ANOFOX_HIP_RESIDUALS_HAS_* flags)."""
        return _residuals(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), y_hat, rse, include_studentized,
                          drop_nan_rows, out, group)

    def elasticnet_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                    core=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped elastic net.  Returns (core[G, p+6], iterations int32[G]) CUDA tensors."""
        b = DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream)
        return _iterative_fit(b, "elasticnet", b.p + 6, options, core, iterations)

    def bls_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions,
                             records=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped bounded least squares.  Returns (bls[G, 3p+6], iterations int32[G]) CUDA tensors."""
        b = DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream)
        return _iterative_fit(b, "bls", 3 * b.p + 6, options, records, iterations)

    def quantile_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                  records=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped quantile regression.  Returns (quantile[G, p+6], iterations int32[G]) CUDA tensors."""
        b = DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream)
        return _iterative_fit(b, "quantile", b.p + 6, options, records, iterations)

    def quantile_fit_path_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                       records=None, iterations=None, use_current_torch_stream: bool = True):
        """The tau path (inputs as quantile_fit_batch_device; taus: a host sequence of 1 .. 64 floats).  Returns
        (quantile[G, T, p+6], iterations int32[G, T]) CUDA tensors, indexed by the position in taus."""
        return _quantile_fit_path(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), options, taus, records, iterations)

    def quantile_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                           frame=(None, 0), want_records: bool = False, use_current_torch_stream: bool = True):
        """The quantile window function over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING (as
        fit_predict_window_device).  The planner reads row_offsets back to the host (one synchronising copy); the kernel is
        enqueued.  Returns pred[N, 3], or (pred, quantile[N, p+6], iterations int32[N]) with want_records."""
        return _quantile_window(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), options, want_records, frame=frame)

    def quantile_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipQuantileBatchOptions,
                                           want_records: bool = False, use_current_torch_stream: bool = True):
        """The same over explicit frames [frame_lo[e], frame_hi[e])."""
        return _quantile_window(DeviceBatch(self, None, y, x_cols, use_current_torch_stream), options, want_records,
                                bounds=(frame_lo, frame_hi))

    def elasticnet_fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                            confidence_level: float = 0.95, train_counts=None, core=None, pred=None,
                                            use_current_torch_stream: bool = True):
        """Elastic net fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        return _family_fit_predict(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), "elasticnet", options,
                                   confidence_level, train_counts, core, pred)

    def elasticnet_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                             frame=(None, 0), confidence_level: float = 0.95, pred=None,
                                             use_current_torch_stream: bool = True):
        """Elastic net window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING, device resident.
        Returns pred[N, 3] (CUDA tensor)."""
        return _family_window(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), "elasticnet", options,
                              confidence_level, pred, frame=frame)

    def elasticnet_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi,
                                             options: _abi.AnofoxHipElasticNetBatchOptions, confidence_level: float = 0.95,
                                             pred=None, use_current_torch_stream: bool = True):
        """Elastic net fit + predict over explicit frames [frame_lo[e], frame_hi[e]), device resident.  Returns pred[N, 3]."""
        return _family_window(DeviceBatch(self, None, y, x_cols, use_current_torch_stream), "elasticnet", options,
                              confidence_level, pred, bounds=(frame_lo, frame_hi))

    # ---- recursive least squares (device resident) ---------------------------------------------
    def rls_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, core=None,
                             use_current_torch_stream: bool = True):
        """Grouped RLS.  Returns core[G, p+6]."""
        return _rls_fit(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), options, core)

    def rls_fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                     confidence_level: float = 0.95, train_counts=None, core=None, pred=None,
                                     use_current_torch_stream: bool = True):
        """RLS fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        return _family_fit_predict(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), "rls", options,
                                   confidence_level, train_counts, core, pred)

    def rls_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                      frame=(None, 0), confidence_level: float = 0.95, pred=None,
                                      use_current_torch_stream: bool = True):
        """RLS window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING.  Returns pred[N, 3]."""
        return _family_window(DeviceBatch(self, row_offsets, y, x_cols, use_current_torch_stream), "rls", options,
                              confidence_level, pred, frame=frame)

    def rls_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipRlsBatchOptions,
                                      confidence_level: float = 0.95, pred=None, use_current_torch_stream: bool = True):
        """RLS fit + predict over explicit frames [frame_lo[e], frame_hi[e]), device resident.  Returns pred[N, 3]."""
        return _family_window(DeviceBatch(self, None, y, x_cols, use_current_torch_stream), "rls", options, confidence_level,
                              pred, bounds=(frame_lo, frame_hi))

    # ---- generalised linear models (glm.py) ------------------------------------------------------
    def glm_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                             inference: bool = False, use_current_torch_stream: bool = True):
        """Grouped Poisson / binomial fits on CUDA tensors through the fused IRLS kernel (glm.glm_fit_batch_device)."""
        from .glm import glm_fit_batch_device
        return glm_fit_batch_device(self, row_offsets, y, x_cols, options, offset, inference, use_current_torch_stream)

    def glm_fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                                     train_counts=None, use_current_torch_stream: bool = True):
        """GLM fit + predict on CUDA tensors: (core[G, p + 11], pred[N, 3]) (glm.glm_fit_predict_batch_device)."""
        from .glm import glm_fit_predict_batch_device
        return glm_fit_predict_batch_device(self, row_offsets, y, x_cols, options, offset, train_counts, use_current_torch_stream)

    def glm_fit_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, offset=None,
                           inference: bool = False):
        from .glm import glm_fit_batch_host
        return glm_fit_batch_host(row_offsets, y, x_cols, options, offset, inference, ctx=self)

    def glm_fit_predict_interval_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions,
                                              interval_z: float, offset=None, train_counts=None, use_current_torch_stream: bool = True):
        """GLM fit + predict with the Poisson interval on CUDA tensors: (core[G, p + 11], pred[N, 3] = mu, lower, upper)."""
        from .glm import glm_fit_predict_batch_device
        return glm_fit_predict_batch_device(self, row_offsets, y, x_cols, options, offset, train_counts, use_current_torch_stream,
                                            interval_z=interval_z)

    def glm_fit_predict_interval_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions,
                                            interval_z: float, offset=None, train_counts=None):
        from .glm import glm_fit_predict_batch_host
        return glm_fit_predict_batch_host(row_offsets, y, x_cols, options, offset, train_counts, ctx=self, interval_z=interval_z)

    def glm_fit_accuracy_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions,
                                      threshold: float = 0.5, offset=None, inference: bool = False,
                                      use_current_torch_stream: bool = True):
        """Binomial fits with the training accuracy on CUDA tensors: (records, [inference,] accuracy[G])."""
        from .glm import glm_fit_batch_device
        return glm_fit_batch_device(self, row_offsets, y, x_cols, options, offset, inference, use_current_torch_stream, threshold=threshold)

    def glm_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions, frame=(None, 0),
                                      offset=None, interval_z=None, want_records: bool = False, use_current_torch_stream: bool = True):
        """The GLM window function over ROWS frames on CUDA tensors: pred[N, 3], or (pred, records[N, p + 11])."""
        from .glm import glm_fit_predict_window_device
        return glm_fit_predict_window_device(self, row_offsets, y, x_cols, options, frame, offset, interval_z, want_records,
                                             use_current_torch_stream)

    def glm_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipGlmBatchOptions,
                                      offset=None, interval_z=None, want_records: bool = False, use_current_torch_stream: bool = True):
        """The GLM window function over explicit frames [frame_lo[e], frame_hi[e]) on CUDA tensors."""
        from .glm import glm_fit_predict_frames_device
        return glm_fit_predict_frames_device(self, y, x_cols, frame_lo, frame_hi, options, offset, interval_z, want_records,
                                             use_current_torch_stream)

    def glm_fit_accuracy_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions,
                                    threshold: float = 0.5, offset=None, inference: bool = False):
        from .glm import glm_fit_batch_host
        return glm_fit_batch_host(row_offsets, y, x_cols, options, offset, inference, ctx=self, threshold=threshold)

    # ---- accelerated failure time models (aft.py) --------------------------------------------------
    def eb_shrink_batch_device(self, set_offsets, est, se, n_cols: int = 1, est_stride=None, se_stride=None, options=None, n_items=None,
                               use_current_torch_stream: bool = True):
        """Empirical-Bayes shrinkage of (estimate, se) pairs on CUDA tensors, the strided matrix form (eb_shrink.eb_shrink_batch_device):
        (out[n_items, n_cols, 3], summary[n_sets, n_cols, 8])."""
        from .eb_shrink import eb_shrink_batch_device
        return eb_shrink_batch_device(self, set_offsets, est, se, n_cols, est_stride, se_stride, options, n_items, use_current_torch_stream)

    def eb_shrink_batch_host(self, set_offsets, est, se, n_cols: int = 1, est_stride=None, se_stride=None, options=None, n_items=None):
        from .eb_shrink import eb_shrink_batch_host
        return eb_shrink_batch_host(set_offsets, est, se, n_cols, est_stride, se_stride, options, n_items, ctx=self)

    def cor_batch_device(self, row_offsets, x, y, method: int, options=None, use_current_torch_stream: bool = True):
        """Grouped Pearson (0), Spearman (1) or Kendall (2) correlation on CUDA tensors (correlation.cor_batch_device): records[n_groups, 8]."""
        from .correlation import cor_batch_device
        return cor_batch_device(self, row_offsets, x, y, method, options, use_current_torch_stream)

    def cor_batch_host(self, row_offsets, x, y, method: int, options=None):
        from .correlation import cor_batch_host
        return cor_batch_host(row_offsets, x, y, method, options, ctx=self)

    def rank_test_batch_device(self, row_offsets, v, y, sample, test: int, options=None, use_current_torch_stream: bool = True):
        """Grouped Mann-Whitney (0), Wilcoxon signed-rank (1) or Kruskal-Wallis (2) tests on CUDA tensors
        (rank_tests.rank_test_batch_device): records[n_groups, 8]."""
        from .rank_tests import rank_test_batch_device
        return rank_test_batch_device(self, row_offsets, v, y, sample, test, options, use_current_torch_stream)

    def rank_test_batch_host(self, row_offsets, v, y, sample, test: int, options=None):
        from .rank_tests import rank_test_batch_host
        return rank_test_batch_host(row_offsets, v, y, sample, test, options, ctx=self)

    def sample_test_batch_device(self, row_offsets, v, y, sample, test: int, options=None, use_current_torch_stream: bool = True):
        """Grouped t (0), Yuen (1), one-way ANOVA (2), Brown-Forsythe (3) or Brunner-Munzel (4) tests on CUDA tensors
        (sample_tests.sample_test_batch_device): records[n_groups, 12]."""
        from .sample_tests import sample_test_batch_device
        return sample_test_batch_device(self, row_offsets, v, y, sample, test, options, use_current_torch_stream)

    def sample_test_batch_host(self, row_offsets, v, y, sample, test: int, options=None):
        from .sample_tests import sample_test_batch_host
        return sample_test_batch_host(row_offsets, v, y, sample, test, options, ctx=self)

    def normality_test_batch_device(self, row_offsets, v, test: int, use_current_torch_stream: bool = True):
        """Grouped Shapiro-Wilk (0), D'Agostino K2 (1) or Jarque-Bera (2) tests on CUDA tensors
        (normality_tests.normality_test_batch_device): records[n_groups, 8]."""
        from .normality_tests import normality_test_batch_device
        return normality_test_batch_device(self, row_offsets, v, test, use_current_torch_stream)

    def normality_test_batch_host(self, row_offsets, v, test: int):
        from .normality_tests import normality_test_batch_host
        return normality_test_batch_host(row_offsets, v, test, ctx=self)

    def categorical_test_batch_device(self, row_offsets, a, b, test: int, options=None, use_current_torch_stream: bool = True):
        """Grouped chi-square (0), G (1), Fisher exact (2) or McNemar (3) tests of two int32 label columns on CUDA tensors
        (categorical_tests.categorical_test_batch_device): records[n_groups, 12]."""
        from .categorical_tests import categorical_test_batch_device
        return categorical_test_batch_device(self, row_offsets, a, b, test, options, use_current_torch_stream)

    def categorical_test_batch_host(self, row_offsets, a, b, test: int, options=None):
        from .categorical_tests import categorical_test_batch_host
        return categorical_test_batch_host(row_offsets, a, b, test, options, ctx=self)

    def perm_test_batch_device(self, row_offsets, v, sample, test: int, options=None, use_current_torch_stream: bool = True):
        """Grouped energy distance (0), permutation t- (1) or MMD (2) tests on CUDA tensors (perm_tests.perm_test_batch_device):
        records[n_groups, 8].  The options need a seed."""
        from .perm_tests import perm_test_batch_device
        return perm_test_batch_device(self, row_offsets, v, sample, test, options, use_current_torch_stream)

    def perm_test_batch_host(self, row_offsets, v, sample, test: int, options=None):
        from .perm_tests import perm_test_batch_host
        return perm_test_batch_host(row_offsets, v, sample, test, options, ctx=self)

    def glmm_fit_batch_device(self, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False,
                              use_current_torch_stream: bool = True):
        """Grouped Gaussian random-intercept mixed models on CUDA tensors (glmm.glmm_fit_batch_device): (records, inference or None,
        ranef, level_n)."""
        from .glmm import glmm_fit_batch_device
        return glmm_fit_batch_device(self, panel_level_offsets, level_row_offsets, y, x_cols, options, inference, use_current_torch_stream)

    def glmm_fit_batch_host(self, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False):
        from .glmm import glmm_fit_batch_host
        return glmm_fit_batch_host(panel_level_offsets, level_row_offsets, y, x_cols, options, inference, ctx=self)

    def glmm_fit_predict_batch_device(self, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False,
                                      use_current_torch_stream: bool = True):
        """glmm_fit_batch_device and a score of every row (glmm.glmm_fit_predict_batch_device): (records, inference or None, ranef,
        level_n, pred[n_rows, 5])."""
        from .glmm import glmm_fit_predict_batch_device
        return glmm_fit_predict_batch_device(self, panel_level_offsets, level_row_offsets, y, x_cols, options, inference,
                                             use_current_torch_stream)

    def glmm_fit_predict_batch_host(self, panel_level_offsets, level_row_offsets, y, x_cols: Sequence, options=None, inference: bool = False):
        from .glmm import glmm_fit_predict_batch_host
        return glmm_fit_predict_batch_host(panel_level_offsets, level_row_offsets, y, x_cols, options, inference, ctx=self)

    def aft_fit_batch_device(self, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                             inference: bool = False, use_current_torch_stream: bool = True):
        """Grouped AFT fits on CUDA tensors through the fused Newton kernel (aft.aft_fit_batch_device)."""
        from .aft import aft_fit_batch_device
        return aft_fit_batch_device(self, row_offsets, time, x_cols, event, options, inference, use_current_torch_stream)

    def aft_fit_batch_host(self, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                           inference: bool = False):
        from .aft import aft_fit_batch_host
        return aft_fit_batch_host(row_offsets, time, x_cols, event, options, inference, ctx=self)

    def aft_fit_predict_batch_device(self, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                                     predict: _abi.AnofoxHipAftPredictOptions, inference: bool = False,
                                     use_current_torch_stream: bool = True, pred_out=None):
        """Grouped AFT fits and a score per row on CUDA tensors (aft.aft_fit_predict_batch_device)."""
        from .aft import aft_fit_predict_batch_device
        return aft_fit_predict_batch_device(self, row_offsets, time, x_cols, event, options, predict, inference, use_current_torch_stream,
                                            pred_out)

    def aft_fit_predict_batch_host(self, row_offsets, time, x_cols: Sequence, event, options: _abi.AnofoxHipAftBatchOptions,
                                   predict: _abi.AnofoxHipAftPredictOptions, inference: bool = False):
        from .aft import aft_fit_predict_batch_host
        return aft_fit_predict_batch_host(row_offsets, time, x_cols, event, options, predict, inference, ctx=self)


class AggState:
    """The streaming aggregate state of {ols,ridge,wls}_fit_agg on the GPU (anofox_hip_agg_state_*): one O(p^2)
    moment record per slot; `update` folds row chunks in, `combine` merges slots, `finalize` solves them."""

    def __init__(self, ctx: Context, n_features: int, options: _abi.AnofoxHipBatchOptions, initial_slots: int = 0,
                 retain_bytes: Optional[int] = None, retain_host_bytes: Optional[int] = None):
        """retain_bytes: HBM for a row log next to the moments (anofox_hip_agg_state_retain_rows), so that finalize can
        refit the groups the moments alone cannot resolve; retain_host_bytes: page-locked host memory the log continues
        in once that is spent (anofox_hip_agg_state_retain_rows_host).  None = the shim's defaults (64 GiB / 32 GiB,
        ANOFOX_HIP_RETAIN_BYTES / ANOFOX_HIP_RETAIN_HOST_BYTES; slabs are allocated as rows arrive), 0 = moments only.
        Groups that finalize can neither resolve nor refit come back as NaN records with status 101."""
        log_only = int(n_features) > 8 or (bool(options.compute_inference) and int(options.hc_type) != 0 and int(options.model) != 1)
        if retain_bytes is None:      # (a log-only state IS its log: uncapped unless the caller caps it)
            retain_bytes = 0 if log_only else int(os.environ.get("ANOFOX_HIP_RETAIN_BYTES", 64 << 30))
        if retain_host_bytes is None:
            # (an explicit retain_bytes = 0 on a moment state means "moments only", as documented: round 3 left the host
            # continuation on in that case, and every chunk was copied back into page-locked slabs — 9 GB/s instead of 55)
            moments_only = (not log_only) and retain_bytes == 0
            retain_host_bytes = 0 if moments_only else int(os.environ.get("ANOFOX_HIP_RETAIN_HOST_BYTES", 32 << 30))
        self._lib = _abi.load()
        self._ctx = ctx          # keeps the context alive
        self.p = int(n_features)
        self.options = options
        self._h = create(self._lib, "anofox_hip_agg_state_create", ctx._h, self.p, options, int(initial_slots))
        self.unrefined_slots = np.empty(0, dtype=np.int32)
        if retain_bytes:
            call(self._lib, "anofox_hip_agg_state_retain_rows", self._h, int(retain_bytes))
        if retain_host_bytes:
            call(self._lib, "anofox_hip_agg_state_retain_rows_host", self._h, int(retain_host_bytes))

    @property
    def retaining(self) -> bool:
        return bool(self._lib.anofox_hip_agg_state_retaining(self._h))

    @property
    def retained_bytes(self) -> int:
        return int(self._lib.anofox_hip_agg_state_retained_bytes(self._h))

    @property
    def retained_host_bytes(self) -> int:
        return int(self._lib.anofox_hip_agg_state_retained_host_bytes(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.anofox_hip_agg_state_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_slots(self) -> int:
        return int(self._lib.anofox_hip_agg_state_slots(self._h))

    @property
    def n_rows(self) -> int:
        return int(self._lib.anofox_hip_agg_state_rows(self._h))

    def reserve(self, n_slots: int):
        call(self._lib, "anofox_hip_agg_state_reserve", self._h, int(n_slots))

    def _device(self, use_current_torch_stream):
        """A device call on this state: no batch, the state's handle, the context's stream."""
        return DeviceBatch(self._ctx, None, None, (), use_current_torch_stream, owner=self)

    def update(self, slot, y, x_rowmajor, w=None, valid=None, n_slots: Optional[int] = None):
        """Host chunk (numpy): slot uint32[n], y float64[n], x_rowmajor float64[n, p], w float64[n], valid uint8[n]."""
        yv = host_array(y, F64, None, "y")
        n = yv.size
        sl, xv = host_array(slot, U32, n, "slot"), host_array(x_rowmajor, F64, n * self.p, "x_rowmajor")
        wv = None if w is None else host_array(w, F64, n, "w")
        vv = None if valid is None else host_array(valid, U8, n, "valid")
        if n_slots is None:
            n_slots = max(self.n_slots, int(sl.max()) + 1 if n else 0)
        call(self._lib, "anofox_hip_agg_state_update_host", self._h, n, int(n_slots), sl, yv, xv, wv, vv)

    def update_device(self, slot, y, x_rowmajor, w=None, valid=None, n_slots: Optional[int] = None,
                      use_current_torch_stream: bool = True):
        """Device chunk (CUDA tensors): slot int32/uint32-as-int32[n], y[n], x_rowmajor[n, p], w[n], valid uint8[n]."""
        b = self._device(use_current_torch_stream)
        n = int(b.array(y, F64, None, "y").numel())
        b.array(slot, None, n, "slot")
        b.array(x_rowmajor, F64, n * self.p, "x_rowmajor")
        if w is not None:
            b.array(w, F64, n, "w")
        if valid is not None:
            b.array(valid, U8, n, "valid")
        if n_slots is None:
            n_slots = max(self.n_slots, int(slot.max().item()) + 1 if n else 0)
        b.call("anofox_hip_agg_state_update", n, int(n_slots), slot, y, x_rowmajor, w, valid)

    def combine(self, source_slots, target_slots):
        src = host_array(source_slots, U32, None, "source_slots")
        dst = host_array(target_slots, U32, src.size, "target_slots")
        call(self._lib, "anofox_hip_agg_state_combine", self._h, src.size, src, dst)

    def finalize(self, n_slots: Optional[int] = None):
        """-> (core[G, p+6], inference[G, 5p+2] or None, number of groups flagged as unrefined: status 101, NaN record —
        they asked for the refinement passes and their rows were not kept)."""
        G = self.n_slots if n_slots is None else int(n_slots)
        p = self.p
        core = np.empty((G, p + 6), dtype=np.float64)
        inf = np.empty((G, 5 * p + 2), dtype=np.float64) if self.options.compute_inference else None
        unref = C.c_int64()
        slots = np.empty(max(G, 1), dtype=np.int32)
        call(self._lib, "anofox_hip_agg_state_finalize_host", self._h, G, core, inf, C.byref(unref), slots)
        self.unrefined_slots = np.sort(slots[:int(unref.value)])   # groups that would have taken the refinement passes
        return core, inf, int(unref.value)

    def finalize_device(self, core, inference=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        """core: float64 CUDA tensor [G, p+6]; inference: float64 CUDA tensor [G, 5p+2] or None."""
        G = self.n_slots if n_slots is None else int(n_slots)
        b = self._device(use_current_torch_stream)
        b.out((G, self.p + 6), given=core)
        if inference is not None:
            b.out((G, 5 * self.p + 2), given=inference)
        b.call("anofox_hip_agg_state_finalize", G, core, inference)
        return core, inference

    # ---- the elastic net and bounded least squares from the same state (anofox_hip_agg_state_finalize_{elasticnet,bls}_*) ----
    def check_family(self, family: str, fit_intercept: bool):
        """The state has to hold the moments of the unweighted fit the family's batch call accumulates: model OLS (no
        weights), hc_type none, the family's fit_intercept.  Raises before any library call."""
        o = self.options
        if int(o.model) != _abi.MODEL["ols"]:
            what = "WLS (weights)" if int(o.model) == _abi.MODEL["wls"] else "ridge"
            raise AnofoxStatsError(_abi.ERROR_INVALID_INPUT,
                                   f"{family} finalize: the state was created with model {what}, it needs the unweighted OLS moments")
        if int(o.hc_type) != 0:
            raise AnofoxStatsError(_abi.ERROR_INVALID_INPUT,
                                   f"{family} finalize: the state was created with an hc_type other than none")
        if bool(o.fit_intercept) != bool(fit_intercept):
            raise AnofoxStatsError(_abi.ERROR_INVALID_INPUT,
                                   f"{family} finalize: fit_intercept of the options differs from the fit_intercept the state was created with")

    def _finalize_family(self, family, symbol, rec_len, options, slots, n_slots):
        self.check_family(family, options.fit_intercept)
        unref = C.c_int64()
        if slots is None:
            G = self.n_slots if n_slots is None else int(n_slots)
            rec = np.empty((G, rec_len), dtype=np.float64)
            its = np.empty(G, dtype=np.int32)
            listed = np.empty(max(G, 1), dtype=np.int32)
            call(self._lib, f"anofox_hip_agg_state_finalize_{symbol}_host", self._h, G, options, rec, its, C.byref(unref), listed)
            return rec, its, listed[:int(unref.value)].copy()
        sl = host_array(slots, U32, None, "slots")
        rec = np.empty((len(sl), rec_len), dtype=np.float64)
        its = np.empty(len(sl), dtype=np.int32)
        call(self._lib, f"anofox_hip_agg_state_finalize_{symbol}_slots_host", self._h, len(sl), sl, options, rec, its, C.byref(unref))
        unrefined = sl[rec[:, self.p + 5] == _abi.STATUS_UNREFINED].astype(np.int32)
        if len(unrefined) != int(unref.value):
            raise AnofoxStatsError(_abi.ERROR_INTERNAL, f"{family} finalize: {int(unref.value)} slots counted as unrefined, {len(unrefined)} marked")
        return rec, its, unrefined

    def finalize_elasticnet(self, options: _abi.AnofoxHipElasticNetBatchOptions, slots=None, n_slots: Optional[int] = None):
        """The elastic net of every slot (or of the listed ones) from this state, which stays as it is:
        -> (core[G, p+6], iterations int32[G], the slot numbers that came back unrefined: status 101, NaN record)."""
        return self._finalize_family("elastic net", "elasticnet", self.p + 6, options, slots, n_slots)

    def finalize_bls(self, options: _abi.AnofoxHipBlsBatchOptions, slots=None, n_slots: Optional[int] = None):
        """Bounded / non-negative least squares of every slot (or of the listed ones) from this state:
        -> (bls[G, 3p+6], iterations int32[G], the unrefined slot numbers)."""
        return self._finalize_family("bounded least squares", "bls", 3 * self.p + 6, options, slots, n_slots)

    def _finalize_family_device(self, family, symbol, rec_len, options, records, iterations, n_slots, use_current_torch_stream):
        self.check_family(family, options.fit_intercept)
        G = self.n_slots if n_slots is None else int(n_slots)
        b = self._device(use_current_torch_stream)
        b.out((G, rec_len), given=records)
        if iterations is not None:
            b.out((G,), I32, given=iterations)
        b.call(f"anofox_hip_agg_state_finalize_{symbol}", G, options, records, iterations)
        return records, iterations

    def finalize_elasticnet_device(self, options, core, iterations=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        """core: float64 CUDA tensor [G, p+6]; iterations: int32 CUDA tensor [G] or None."""
        return self._finalize_family_device("elastic net", "elasticnet", self.p + 6, options, core, iterations, n_slots,
                                            use_current_torch_stream)

    def finalize_bls_device(self, options, bls, iterations=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        """bls: float64 CUDA tensor [G, 3p+6]; iterations: int32 CUDA tensor [G] or None."""
        return self._finalize_family_device("bounded least squares", "bls", 3 * self.p + 6, options, bls, iterations, n_slots,
                                            use_current_torch_stream)


# ---- host-resident batch (numpy in, numpy out): inputs as the device methods'; ctx None = the thread's default context -------

def fit_batch_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                   ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], inference[G, 5p+2] or None)."""
    return _fit(HostBatch(ctx, row_offsets, y, x_cols), w, options)


def fit_predict_batch_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions, train_counts=None,
                           ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = SQL NULL)."""
    return _fit_predict(HostBatch(ctx, row_offsets, y, x_cols), w, options, train_counts)


def fit_predict_expanding_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                               ctx: Optional[Context] = None):
    """numpy in, numpy out: pred[N, 3] — prediction of x_e from the fit on rows 0..e of its partition."""
    return fit_predict_window_host(row_offsets, y, x_cols, w, options, (None, 0), ctx=ctx)


def fit_predict_window_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                            frame=(None, 0), ctx: Optional[Context] = None):
    """numpy in, numpy out: pred[N, 3] of the window functions over ROWS BETWEEN frame[0] PRECEDING AND frame[1]
    PRECEDING (negative = FOLLOWING; frame[0] None = UNBOUNDED PRECEDING, frame[1] 0 = CURRENT ROW, None = UNBOUNDED
    FOLLOWING)."""
    return _fit_predict_window(HostBatch(ctx, row_offsets, y, x_cols), w, options, frame)


def fit_predict_frames_host(y, x_cols: Sequence, w, frame_lo, frame_hi, options: _abi.AnofoxHipBatchOptions,
                            ctx: Optional[Context] = None):
    """Window fit + predict over explicit frames: frame of row e = rows [frame_lo[e], frame_hi[e]).  numpy in / out:
    pred[N, 3]."""
    b = HostBatch(ctx, None, y, x_cols)
    pred = b.out((b.N, 3))
    b.call("anofox_hip_fit_predict_frames", *b.rows_head, b.rows(w, "w"), *b.frames(frame_lo, frame_hi), options, pred)
    return pred


def information_criteria_host(core, options: _abi.AnofoxHipBatchOptions, ctx: Optional[Context] = None):
    """numpy fit records [G, p+6] -> out[G, 3] = {rss, aic, bic} (anofox_hip_information_criteria_batch_host)."""
    return _information_criteria(HostBatch(ctx, None, None, ()), core, options)


def vif_batch_host(row_offsets, x_cols: Sequence, ctx: Optional[Context] = None):
    """numpy in, numpy out: out[G, p+1] = {vif[p], status} (status 100 = fewer than 3 rows -> SQL NULL)."""
    return _vif(HostBatch(ctx, row_offsets, None, x_cols))


def residuals_batch_host(row_offsets, y, y_hat, x_cols: Sequence = (), rse=None, include_studentized: bool = True,
                         drop_nan_rows: bool = True, ctx: Optional[Context] = None):
    """numpy in, numpy out: (out[N, 4] = raw / standardized / studentized / leverage, group[G, 2] = rows used / flags)."""
    return _residuals(HostBatch(ctx, row_offsets, y, x_cols), y_hat, rse, include_studentized, drop_nan_rows)


def elasticnet_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                              ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], iterations int32[G])."""
    b = HostBatch(ctx, row_offsets, y, x_cols)
    return _iterative_fit(b, "elasticnet", b.p + 6, options)


def elasticnet_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                      confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """Elastic net fit + predict, numpy in / out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    return _family_fit_predict(HostBatch(ctx, row_offsets, y, x_cols), "elasticnet", options, confidence_level, train_counts)


def elasticnet_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                       frame=(None, 0), confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """Elastic net window fit + predict over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3]."""
    return _family_window(HostBatch(ctx, row_offsets, y, x_cols), "elasticnet", options, confidence_level, frame=frame)


def elasticnet_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipElasticNetBatchOptions,
                                       confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """Elastic net fit + predict over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out: pred[N, 3]."""
    return _family_window(HostBatch(ctx, None, y, x_cols), "elasticnet", options, confidence_level, bounds=(frame_lo, frame_hi))


def bls_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions, ctx: Optional[Context] = None):
    """Grouped bounded least squares, numpy in / out: (bls[G, 3p+6], iterations int32[G]); the record layout is
    anofox_hip_bls_fit_batch_host's (include/anofox_stats_hip.h)."""
    b = HostBatch(ctx, row_offsets, y, x_cols)
    return _iterative_fit(b, "bls", 3 * b.p + 6, options)


def bls_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions,
                               confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """Bounded least squares fit + predict, numpy in / out: (core[G, p+6] = coefficients, intercept, r2, ssr, sigma, n,
    status; pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    return _family_fit_predict(HostBatch(ctx, row_offsets, y, x_cols), "bls", options, confidence_level, train_counts)


def quantile_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, ctx: Optional[Context] = None):
    """Grouped quantile regression, numpy in / out: (quantile[G, p+6], iterations int32[G]); the record layout is
    anofox_hip_quantile_fit_batch_host's (include/anofox_stats_hip.h)."""
    b = HostBatch(ctx, row_offsets, y, x_cols)
    return _iterative_fit(b, "quantile", b.p + 6, options)


def quantile_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                    train_counts=None, ctx: Optional[Context] = None):
    """Quantile regression fit + predict, numpy in / out: (core[G, p+6] = coefficients, intercept, NaN, NaN, NaN, n, status;
    pred[N, 3] = yhat, NaN, NaN; a NaN yhat = NULL)."""
    b = HostBatch(ctx, row_offsets, y, x_cols)
    core, pred = b.out((b.G, b.p + 6)), b.out((b.N, 3))
    b.call("anofox_hip_quantile_fit_predict_batch", *b.head, b.groups(train_counts, "train_counts"), options, core, pred)
    return core, pred


def quantile_fit_path_batch_device(ctx: Context, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                   **kwargs):
    """Context.quantile_fit_path_batch_device as a function (the device path needs an explicit context)."""
    return ctx.quantile_fit_path_batch_device(row_offsets, y, x_cols, options, taus, **kwargs)


def quantile_fit_path_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                 ctx: Optional[Context] = None):
    """The tau path, numpy in / out: (quantile[G, T, p+6], iterations int32[G, T]), indexed by the position in taus; the
    contract is anofox_hip_quantile_fit_path_batch_host's (include/anofox_stats_hip.h).  options.tau is ignored."""
    return _quantile_fit_path(HostBatch(ctx, row_offsets, y, x_cols), options, taus)


def quantile_fit_predict_path_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                         train_counts=None, ctx: Optional[Context] = None):
    """The tau path with its fused prediction, numpy in / out: (quantile[G, T, p+6], iterations int32[G, T], pred[N, T]);
    pred[i, t] is the prediction of row i at taus[t], NaN = NULL."""
    b = HostBatch(ctx, row_offsets, y, x_cols)
    tv = host_array(taus, F64).ravel()
    rec, its, pred = b.out((b.G, tv.size, b.p + 6)), b.out((b.G, tv.size), I32), b.out((b.N, tv.size))
    b.call("anofox_hip_quantile_fit_predict_path_batch", *b.head, b.groups(train_counts, "train_counts"), options, tv, tv.size,
           rec, its, pred)
    return rec, its, pred


def quantile_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, frame=(None, 0),
                                     want_records: bool = False, ctx: Optional[Context] = None):
    """The quantile regression window function over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3] =
    {yhat, NaN, NaN}; with want_records (pred, quantile[N, p+6], iterations int32[N]) — the record of every frame in
    anofox_hip_quantile_fit_batch_host's layout and its pivots."""
    return _quantile_window(HostBatch(ctx, row_offsets, y, x_cols), options, want_records, frame=frame)


def quantile_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipQuantileBatchOptions,
                                     want_records: bool = False, ctx: Optional[Context] = None):
    """The quantile regression window function over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out (as
    quantile_fit_predict_window_host)."""
    return _quantile_window(HostBatch(ctx, None, y, x_cols), options, want_records, bounds=(frame_lo, frame_hi))


def quantile_window_plan(row_offsets, frame_lo, frame_hi, run_length: int = 0, scratch_cap_bytes: int = 0):
    """The planner of the quantile window function alone (host arrays, no device): -> (run_begin int64[walkers + 1], scratch
    rows per wavefront, launched wavefronts).  run_length / scratch_cap_bytes 0: the library's rule."""
    off = host_array(row_offsets, I64, None, "row_offsets")
    lo = host_array(frame_lo, I64, None, "frame_lo")
    hi = host_array(frame_hi, I64, lo.size, "frame_hi")
    runs = np.empty(lo.size + 2, dtype=np.int64)
    n_runs, span, waves = C.c_int64(), C.c_int64(), C.c_int64()
    call(_abi.load(), "anofox_hip_quantile_window_plan", off.size - 1, off, lo.size, lo, hi, int(run_length), int(scratch_cap_bytes),
         runs, runs.size, C.byref(n_runs), C.byref(span), C.byref(waves))
    return runs[:n_runs.value + 1].copy(), int(span.value), int(waves.value)


def quantile_window_test_hooks(run_length: int = 0, scratch_cap_bytes: int = 0):
    """For tests and measurements: the run length and the scratch cap of every later window call (0: the library's rule)."""
    _abi.load().anofox_hip_quantile_window_test_hooks(int(run_length), int(scratch_cap_bytes))


def quantile_window_stats(ctx: Optional[Context] = None):
    """The most recent quantile window call on the context: dict(frames, cold_starts, walkers, waves, span_rows, restarts);
    cold_starts counts every frame that began afresh, restarts those of them that followed a fitted frame."""
    out = (C.c_int64 * 6)()
    call(_abi.load(), "anofox_hip_quantile_window_stats", handle(ctx), out)
    return dict(frames=int(out[0]), cold_starts=int(out[1]), walkers=int(out[2]), waves=int(out[3]), span_rows=int(out[4]),
                restarts=int(out[5]))


def rls_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, ctx: Optional[Context] = None):
    """Grouped RLS, numpy in / out: core[G, p+6] (DESIGN.md §1 "Recursive least squares")."""
    return _rls_fit(HostBatch(ctx, row_offsets, y, x_cols), options)


def rls_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                               confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """RLS fit + predict, numpy in / out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    return _family_fit_predict(HostBatch(ctx, row_offsets, y, x_cols), "rls", options, confidence_level, train_counts)


def rls_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, frame=(None, 0),
                                confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """RLS window fit + predict over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3]."""
    return _family_window(HostBatch(ctx, row_offsets, y, x_cols), "rls", options, confidence_level, frame=frame)


def rls_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipRlsBatchOptions,
                                confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """RLS fit + predict over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out: pred[N, 3]."""
    return _family_window(HostBatch(ctx, None, y, x_cols), "rls", options, confidence_level, bounds=(frame_lo, frame_hi))


def _on_context(fn):
    """Context.<fn> = the host function `fn` on that context: the same positional and keyword arguments, without ctx."""
    def method(self, *args, **kwargs):
        return fn(*args, ctx=self, **kwargs)
    method.__name__, method.__qualname__, method.__doc__ = fn.__name__, f"Context.{fn.__name__}", fn.__doc__
    return method


for _fn in (fit_batch_host, elasticnet_fit_batch_host, elasticnet_fit_predict_batch_host, elasticnet_fit_predict_window_host,
            elasticnet_fit_predict_frames_host, bls_fit_batch_host, bls_fit_predict_batch_host, quantile_fit_batch_host,
            quantile_fit_predict_batch_host, quantile_fit_path_batch_host, quantile_fit_predict_path_batch_host,
            quantile_fit_predict_window_host, quantile_fit_predict_frames_host, quantile_window_stats, rls_fit_batch_host,
            rls_fit_predict_batch_host, rls_fit_predict_window_host, rls_fit_predict_frames_host):
    setattr(Context, _fn.__name__, _on_context(_fn))
del _fn
