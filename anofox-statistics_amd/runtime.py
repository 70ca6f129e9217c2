"""Contexts and the two batch entry points (host pointers / device pointers)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._abi import AnofoxStatsError


class Context:
    """Owns one AnofoxHipContext (device + stream + reusable workspace)."""

    def __init__(self, device: int = -1):
        lib = _abi.load()
        err = _abi.AnofoxError()
        handle = C.c_void_p()
        if not lib.anofox_hip_context_create(int(device), C.byref(handle), C.byref(err)):
            raise AnofoxStatsError(err.code, err.text())
        self._h = handle
        self._lib = lib

    def close(self):
        if getattr(self, "_h", None):
            self._lib.anofox_hip_context_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _check(self, ok, err):
        if not ok:
            raise AnofoxStatsError(err.code, err.text())

    def set_stream(self, hip_stream: Optional[int]):
        """Launch on the given hipStream_t handle.  0 is HIP's default stream (= torch's default stream) and is used
        as given; None goes back to the context's own non-blocking stream."""
        err = _abi.AnofoxError()
        if hip_stream is None:
            self._check(self._lib.anofox_hip_context_use_own_stream(self._h, C.byref(err)), err)
        else:
            self._check(self._lib.anofox_hip_context_set_stream(self._h, C.c_void_p(int(hip_stream)), C.byref(err)), err)

    def set_accumulate_gate(self, wait_event=None, record_event=None):
        """torch.cuda.Event objects (or None): wait for `wait_event` before the accumulate kernel of the next fit
        calls, record `record_event` right after it (see anofox_hip_context_set_accumulate_gate)."""
        err = _abi.AnofoxError()
        h = lambda ev: C.c_void_p(0 if ev is None else int(ev.cuda_event))
        # the library holds the raw hipEvent_t handles until the next fit call consumes the (one-shot) gate: keep the
        # torch objects alive at least that long, whatever the caller does with its own references
        self._gate_events = (wait_event, record_event)
        self._check(self._lib.anofox_hip_context_set_accumulate_gate(self._h, h(wait_event), h(record_event), C.byref(err)), err)

    def synchronize(self):
        err = _abi.AnofoxError()
        self._check(self._lib.anofox_hip_context_synchronize(self._h, C.byref(err)), err)

    def enable_timing(self, enable: bool = True):
        err = _abi.AnofoxError()
        self._check(self._lib.anofox_hip_context_enable_timing(self._h, bool(enable), C.byref(err)), err)

    def collect_timing(self) -> dict:
        err = _abi.AnofoxError()
        t = _abi.AnofoxHipKernelTimes()
        self._check(self._lib.anofox_hip_context_collect_timing(self._h, C.byref(t), C.byref(err)), err)
        return {"accumulate_ms": t.accumulate_ms, "accumulate_count": t.accumulate_count,
                "solve_ms": t.solve_ms, "solve_count": t.solve_count,
                "predict_ms": t.predict_ms, "predict_count": t.predict_count,
                "accumulate_ms_min": t.accumulate_ms_min, "accumulate_ms_max": t.accumulate_ms_max}

    # ---- device-resident batch (torch tensors on this context's GPU) -------------------------
    def fit_batch_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                         core=None, inference=None, use_current_torch_stream: bool = True):
        """row_offsets: int64[G+1]; y, x_cols[j], w: float64[N] CUDA tensors.  Asynchronous.
        Returns (core[G, p+6], inference[G, 5p+2] or None) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        for t in (row_offsets, y, *x_cols) + ((w,) if w is not None else ()):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols) or (w is not None and int(w.numel()) != N):
            raise ValueError("every column must have y's length")
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if options.compute_inference and inference is None:
            inference = torch.empty((G, 5 * p + 2), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_fit_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(w.data_ptr() if w is not None else 0), options, C.c_void_p(core.data_ptr()),
            C.c_void_p(inference.data_ptr() if inference is not None else 0), C.byref(err))
        self._gate_events = None   # consumed (or dropped) by the call above
        self._check(ok, err)
        return core, (inference if options.compute_inference else None)

    def fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                 train_counts=None, core=None, pred=None, use_current_torch_stream: bool = True):
        """fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_fit_predict_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(w.data_ptr() if w is not None else 0),
            C.c_void_p(train_counts.data_ptr() if train_counts is not None else 0), options,
            C.c_void_p(core.data_ptr()), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return core, pred

    def fit_predict_expanding_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                     pred=None, use_current_torch_stream: bool = True):
        """Expanding-window fit + predict, device resident.  Returns pred[N, 3] (CUDA tensor)."""
        return self.fit_predict_window_device(row_offsets, y, x_cols, w, options, (None, 0), pred, use_current_torch_stream)

    def fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                                  frame=(None, 0), pred=None, use_current_torch_stream: bool = True):
        """Window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING (frame[0] None =
        UNBOUNDED), device resident.  Returns pred[N, 3] (CUDA tensor)."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_fit_predict_window_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(w.data_ptr() if w is not None else 0), _frame(frame), options, C.c_void_p(pred.data_ptr()),
            C.byref(err))
        self._check(ok, err)
        return pred

    def information_criteria_device(self, core, options: _abi.AnofoxHipBatchOptions, out=None, use_current_torch_stream: bool = True):
        """CUDA fit records [G, p+6] -> out[G, 3] = {rss, aic, bic}; asynchronous."""
        import torch
        G, p = int(core.shape[0]), int(core.shape[1]) - 6
        if out is None:
            out = torch.empty((G, 3), dtype=torch.float64, device=core.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(core.device).cuda_stream)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_information_criteria_batch_device(self._h, G, p, C.c_void_p(core.data_ptr()), options,
                                                                    C.c_void_p(out.data_ptr()), C.byref(err))
        self._check(ok, err)
        return out

    def last_window_refit_count(self) -> int:
        """Output rows of the most recent window call that were refitted with refinement (diagnostic)."""
        n = C.c_int64()
        err = _abi.AnofoxError()
        self._check(self._lib.anofox_hip_context_last_window_refit_count(self._h, C.byref(n), C.byref(err)), err)
        return int(n.value)

    def last_refine_count(self) -> int:
        """Groups of the most recent fit launch that took the on-device refinement passes (diagnostic)."""
        n = C.c_int64()
        err = _abi.AnofoxError()
        self._check(self._lib.anofox_hip_context_last_refine_count(self._h, C.byref(n), C.byref(err)), err)
        return int(n.value)

    def vif_batch_device(self, row_offsets, x_cols: Sequence, out=None, use_current_torch_stream: bool = True):
        """Grouped variance inflation factors, device resident.  Returns out[G, p+1] = {vif[p], status}."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(x_cols[0].numel())
        if out is None:
            out = torch.empty((G, p + 1), dtype=torch.float64, device=x_cols[0].device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(x_cols[0].device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_vif_batch_device(self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), cols,
                                                   C.c_void_p(out.data_ptr()), C.byref(err))
        self._check(ok, err)
        return out

    def residuals_batch_device(self, row_offsets, y, y_hat, x_cols: Sequence = (), rse=None, include_studentized: bool = True,
                               drop_nan_rows: bool = True, out=None, group=None, use_current_torch_stream: bool = True):
        """Grouped residual diagnostics, device resident.  Returns (out[N, 4] = raw / standardized / studentized /
        leverage per row, group[G, 2] = rows used / ANOFOX_HIP_RESIDUALS_HAS_* flags)."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        if out is None:
            out = torch.empty((N, 4), dtype=torch.float64, device=y.device)
        if group is None:
            group = torch.empty((G, 2), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_residuals_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(y_hat.data_ptr()),
            cols if p else None, C.c_void_p(rse.data_ptr()) if rse is not None else None, bool(include_studentized),
            bool(drop_nan_rows), C.c_void_p(out.data_ptr()), C.c_void_p(group.data_ptr()), C.byref(err))
        self._check(ok, err)
        return out, group

    def elasticnet_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                    core=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped elastic net on CUDA tensors (row_offsets int64[G+1], y / x_cols[j] float64[N]).  Asynchronous.
        Returns (core[G, p+6], iterations int32[G]) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        for t in (row_offsets, y, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols):
            raise ValueError("every column must have y's length")
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if iterations is None:
            iterations = torch.empty((G,), dtype=torch.int32, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_elasticnet_fit_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, options,
            C.c_void_p(core.data_ptr()), C.c_void_p(iterations.data_ptr()), C.byref(err))
        self._gate_events = None
        self._check(ok, err)
        return core, iterations

    def bls_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions,
                             records=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped bounded least squares on CUDA tensors (row_offsets int64[G+1], y / x_cols[j] float64[N]).  Asynchronous.
        Returns (bls[G, 3p+6], iterations int32[G]) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        for t in (row_offsets, y, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols):
            raise ValueError("every column must have y's length")
        if records is None:
            records = torch.empty((G, 3 * p + 6), dtype=torch.float64, device=y.device)
        if iterations is None:
            iterations = torch.empty((G,), dtype=torch.int32, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_bls_fit_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, options,
            C.c_void_p(records.data_ptr()), C.c_void_p(iterations.data_ptr()), C.byref(err))
        self._gate_events = None
        self._check(ok, err)
        return records, iterations

    def bls_fit_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions):
        return bls_fit_batch_host(row_offsets, y, x_cols, options, ctx=self)

    def quantile_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                  records=None, iterations=None, use_current_torch_stream: bool = True):
        """Grouped quantile regression on CUDA tensors (row_offsets int64[G+1], y / x_cols[j] float64[N]).  Asynchronous.
        Returns (quantile[G, p+6], iterations int32[G]) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        for t in (row_offsets, y, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols):
            raise ValueError("every column must have y's length")
        if records is None:
            records = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if iterations is None:
            iterations = torch.empty((G,), dtype=torch.int32, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_quantile_fit_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, options,
            C.c_void_p(records.data_ptr()), C.c_void_p(iterations.data_ptr()), C.byref(err))
        self._check(ok, err)
        return records, iterations

    def quantile_fit_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions):
        return quantile_fit_batch_host(row_offsets, y, x_cols, options, ctx=self)

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

    def glm_fit_accuracy_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipGlmBatchOptions,
                                    threshold: float = 0.5, offset=None, inference: bool = False):
        from .glm import glm_fit_batch_host
        return glm_fit_batch_host(row_offsets, y, x_cols, options, offset, inference, ctx=self, threshold=threshold)

    def quantile_fit_path_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                       records=None, iterations=None, use_current_torch_stream: bool = True):
        """The tau path on CUDA tensors (inputs as quantile_fit_batch_device; taus: a host sequence of 1 .. 64 floats).
        Asynchronous.  Returns (quantile[G, T, p+6], iterations int32[G, T]) CUDA tensors, indexed by the position in taus."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        tv = np.ascontiguousarray(taus, dtype=np.float64).ravel()
        T = len(tv)
        for t in (row_offsets, y, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols):
            raise ValueError("every column must have y's length")
        if records is None:
            records = torch.empty((G, T, p + 6), dtype=torch.float64, device=y.device)
        if iterations is None:
            iterations = torch.empty((G, T), dtype=torch.int32, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_quantile_fit_path_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, options,
            tv.ctypes.data_as(_DP), T, C.c_void_p(records.data_ptr()), C.c_void_p(iterations.data_ptr()), C.byref(err))
        self._check(ok, err)
        return records, iterations

    def quantile_fit_path_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus):
        return quantile_fit_path_batch_host(row_offsets, y, x_cols, options, taus, ctx=self)

    def quantile_fit_predict_path_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                             taus, train_counts=None):
        return quantile_fit_predict_path_batch_host(row_offsets, y, x_cols, options, taus, train_counts, ctx=self)

    def quantile_fit_predict_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                        train_counts=None):
        return quantile_fit_predict_batch_host(row_offsets, y, x_cols, options, train_counts, ctx=self)

    def quantile_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                           frame=(None, 0), want_records: bool = False, use_current_torch_stream: bool = True):
        """The quantile window function on CUDA tensors over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING (as
        fit_predict_window_device).  The planner reads row_offsets back to the host (one synchronising copy); the kernel is
        enqueued.  Returns pred[N, 3], or (pred, quantile[N, p+6], iterations int32[N]) with want_records."""
        import torch

        p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
        for t in (row_offsets, y, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if row_offsets.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("row_offsets must be int64 and data float64")
        if any(int(c.numel()) != N for c in x_cols):
            raise ValueError("every column must have y's length")
        pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        rec = torch.empty((N, p + 6), dtype=torch.float64, device=y.device) if want_records else None
        its = torch.empty((N,), dtype=torch.int32, device=y.device) if want_records else None
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_quantile_fit_predict_window_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, _frame(frame), options,
            C.c_void_p(pred.data_ptr()), C.c_void_p(rec.data_ptr()) if want_records else None,
            C.c_void_p(its.data_ptr()) if want_records else None, C.byref(err))
        self._check(ok, err)
        return (pred, rec, its) if want_records else pred

    def quantile_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipQuantileBatchOptions,
                                           want_records: bool = False, use_current_torch_stream: bool = True):
        """The same over explicit frames [frame_lo[e], frame_hi[e]) (int64 CUDA tensors of y's length)."""
        import torch

        p, N = len(x_cols), int(y.numel())
        for t in (y, frame_lo, frame_hi, *x_cols):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device batch needs contiguous CUDA tensors")
        if frame_lo.dtype != torch.int64 or frame_hi.dtype != torch.int64 or y.dtype != torch.float64 or any(c.dtype != torch.float64 for c in x_cols):
            raise ValueError("frame bounds must be int64 and data float64")
        if any(int(c.numel()) != N for c in (frame_lo, frame_hi, *x_cols)):
            raise ValueError("every column and both frame bounds must have y's length")
        pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        rec = torch.empty((N, p + 6), dtype=torch.float64, device=y.device) if want_records else None
        its = torch.empty((N,), dtype=torch.int32, device=y.device) if want_records else None
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * max(p, 1))(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_quantile_fit_predict_frames_device(
            self._h, N, p, C.c_void_p(y.data_ptr()), cols, C.c_void_p(frame_lo.data_ptr()), C.c_void_p(frame_hi.data_ptr()), options,
            C.c_void_p(pred.data_ptr()), C.c_void_p(rec.data_ptr()) if want_records else None,
            C.c_void_p(its.data_ptr()) if want_records else None, C.byref(err))
        self._check(ok, err)
        return (pred, rec, its) if want_records else pred

    def quantile_fit_predict_window_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                         frame=(None, 0), want_records: bool = False):
        return quantile_fit_predict_window_host(row_offsets, y, x_cols, options, frame, want_records, ctx=self)

    def quantile_fit_predict_frames_host(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipQuantileBatchOptions,
                                         want_records: bool = False):
        return quantile_fit_predict_frames_host(y, x_cols, frame_lo, frame_hi, options, want_records, ctx=self)

    def quantile_window_stats(self):
        return quantile_window_stats(ctx=self)

    def bls_fit_predict_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions,
                                   confidence_level: float = 0.95, train_counts=None):
        return bls_fit_predict_batch_host(row_offsets, y, x_cols, options, confidence_level, train_counts, ctx=self)

    def elasticnet_fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                            confidence_level: float = 0.95, train_counts=None, core=None, pred=None,
                                            use_current_torch_stream: bool = True):
        """Elastic net fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_elasticnet_fit_predict_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(train_counts.data_ptr() if train_counts is not None else 0), options, float(confidence_level),
            C.c_void_p(core.data_ptr()), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._gate_events = None
        self._check(ok, err)
        return core, pred

    def elasticnet_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                             frame=(None, 0), confidence_level: float = 0.95, pred=None,
                                             use_current_torch_stream: bool = True):
        """Elastic net window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING, device resident.
        Returns pred[N, 3] (CUDA tensor)."""
        import torch

        p = len(x_cols)
        G = int(row_offsets.numel()) - 1
        N = int(y.numel())
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_elasticnet_fit_predict_window_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, _frame(frame), options,
            float(confidence_level), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return pred

    def elasticnet_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi,
                                             options: _abi.AnofoxHipElasticNetBatchOptions, confidence_level: float = 0.95,
                                             pred=None, use_current_torch_stream: bool = True):
        """Elastic net fit + predict over explicit frames [frame_lo[e], frame_hi[e]), device resident.  Returns pred[N, 3]."""
        import torch

        p = len(x_cols)
        N = int(y.numel())
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        cols = (C.c_void_p * p)(*[c.data_ptr() for c in x_cols])
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_elasticnet_fit_predict_frames_device(
            self._h, N, p, C.c_void_p(y.data_ptr()), cols, C.c_void_p(frame_lo.data_ptr()), C.c_void_p(frame_hi.data_ptr()),
            options, float(confidence_level), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return pred

    # ---- recursive least squares (device resident) ---------------------------------------------
    def _rls_cols(self, y, x_cols, use_current_torch_stream):
        import torch

        for t in (y, *x_cols):
            if not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float64:
                raise ValueError("device calls need contiguous float64 CUDA tensors")
        if any(int(c.numel()) != int(y.numel()) for c in x_cols):
            raise ValueError("every column must have y's length")
        if use_current_torch_stream:
            self.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        return (C.c_void_p * len(x_cols))(*[c.data_ptr() for c in x_cols])

    def rls_fit_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, core=None,
                             use_current_torch_stream: bool = True):
        """Grouped RLS on CUDA tensors (row_offsets int64[G+1], y / x_cols[j] float64[N]).  Asynchronous.  Returns core[G, p+6]."""
        import torch

        p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
        cols = self._rls_cols(y, x_cols, use_current_torch_stream)
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_rls_fit_batch_device(self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()),
                                                       cols, options, C.c_void_p(core.data_ptr()), C.byref(err))
        self._check(ok, err)
        return core

    def rls_fit_predict_batch_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                     confidence_level: float = 0.95, train_counts=None, core=None, pred=None,
                                     use_current_torch_stream: bool = True):
        """RLS fit + per-row predictions, device resident.  Returns (core[G, p+6], pred[N, 3]) CUDA tensors."""
        import torch

        p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
        cols = self._rls_cols(y, x_cols, use_current_torch_stream)
        if core is None:
            core = torch.empty((G, p + 6), dtype=torch.float64, device=y.device)
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_rls_fit_predict_batch_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols,
            C.c_void_p(train_counts.data_ptr() if train_counts is not None else 0), options, float(confidence_level),
            C.c_void_p(core.data_ptr()), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return core, pred

    def rls_fit_predict_window_device(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                      frame=(None, 0), confidence_level: float = 0.95, pred=None,
                                      use_current_torch_stream: bool = True):
        """RLS window fit + predict over ROWS BETWEEN frame[0] PRECEDING AND frame[1] PRECEDING.  Returns pred[N, 3]."""
        import torch

        p, G, N = len(x_cols), int(row_offsets.numel()) - 1, int(y.numel())
        cols = self._rls_cols(y, x_cols, use_current_torch_stream)
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_rls_fit_predict_window_device(
            self._h, G, p, N, C.c_void_p(row_offsets.data_ptr()), C.c_void_p(y.data_ptr()), cols, _frame(frame), options,
            float(confidence_level), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return pred

    def rls_fit_predict_frames_device(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipRlsBatchOptions,
                                      confidence_level: float = 0.95, pred=None, use_current_torch_stream: bool = True):
        """RLS fit + predict over explicit frames [frame_lo[e], frame_hi[e]), device resident.  Returns pred[N, 3]."""
        import torch

        p, N = len(x_cols), int(y.numel())
        cols = self._rls_cols(y, x_cols, use_current_torch_stream)
        if pred is None:
            pred = torch.empty((N, 3), dtype=torch.float64, device=y.device)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_rls_fit_predict_frames_device(
            self._h, N, p, C.c_void_p(y.data_ptr()), cols, C.c_void_p(frame_lo.data_ptr()), C.c_void_p(frame_hi.data_ptr()),
            options, float(confidence_level), C.c_void_p(pred.data_ptr()), C.byref(err))
        self._check(ok, err)
        return pred

    def rls_fit_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions):
        return rls_fit_batch_host(row_offsets, y, x_cols, options, ctx=self)

    def rls_fit_predict_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                   confidence_level: float = 0.95, train_counts=None):
        return rls_fit_predict_batch_host(row_offsets, y, x_cols, options, confidence_level, train_counts, ctx=self)

    def rls_fit_predict_window_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                                    frame=(None, 0), confidence_level: float = 0.95):
        return rls_fit_predict_window_host(row_offsets, y, x_cols, options, frame, confidence_level, ctx=self)

    def rls_fit_predict_frames_host(self, y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipRlsBatchOptions,
                                    confidence_level: float = 0.95):
        return rls_fit_predict_frames_host(y, x_cols, frame_lo, frame_hi, options, confidence_level, ctx=self)

    # ---- host-resident batch (numpy) ----------------------------------------------------------
    def fit_batch_host(self, row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions):
        return fit_batch_host(row_offsets, y, x_cols, w, options, ctx=self)

    def elasticnet_fit_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions):
        return elasticnet_fit_batch_host(row_offsets, y, x_cols, options, ctx=self)

    def elasticnet_fit_predict_batch_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                          confidence_level: float = 0.95, train_counts=None):
        return elasticnet_fit_predict_batch_host(row_offsets, y, x_cols, options, confidence_level, train_counts, ctx=self)

    def elasticnet_fit_predict_window_host(self, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                           frame=(None, 0), confidence_level: float = 0.95):
        return elasticnet_fit_predict_window_host(row_offsets, y, x_cols, options, frame, confidence_level, ctx=self)

    def elasticnet_fit_predict_frames_host(self, y, x_cols: Sequence, frame_lo, frame_hi,
                                           options: _abi.AnofoxHipElasticNetBatchOptions, confidence_level: float = 0.95):
        return elasticnet_fit_predict_frames_host(y, x_cols, frame_lo, frame_hi, options, confidence_level, ctx=self)


_DP = C.POINTER(C.c_double)


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
        err = _abi.AnofoxError()
        h = C.c_void_p()
        if not self._lib.anofox_hip_agg_state_create(ctx._h, self.p, options, int(initial_slots), C.byref(h), C.byref(err)):
            raise AnofoxStatsError(err.code, err.text())
        self._h = h
        self.unrefined_slots = np.empty(0, dtype=np.int32)
        if retain_bytes:
            if not self._lib.anofox_hip_agg_state_retain_rows(self._h, int(retain_bytes), C.byref(err)):
                raise AnofoxStatsError(err.code, err.text())
        if retain_host_bytes:
            if not self._lib.anofox_hip_agg_state_retain_rows_host(self._h, int(retain_host_bytes), C.byref(err)):
                raise AnofoxStatsError(err.code, err.text())

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
        err = _abi.AnofoxError()
        if not self._lib.anofox_hip_agg_state_reserve(self._h, int(n_slots), C.byref(err)):
            raise AnofoxStatsError(err.code, err.text())

    def update(self, slot, y, x_rowmajor, w=None, valid=None, n_slots: Optional[int] = None):
        """Host chunk (numpy): slot uint32[n], y float64[n], x_rowmajor float64[n, p], w float64[n], valid uint8[n]."""
        sl = np.ascontiguousarray(slot, dtype=np.uint32)
        yv = np.ascontiguousarray(y, dtype=np.float64)
        xv = np.ascontiguousarray(x_rowmajor, dtype=np.float64)
        n = len(yv)
        if len(sl) != n or xv.size != n * self.p:
            raise ValueError("slot, y and x disagree in length")
        wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        vv = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
        if n_slots is None:
            n_slots = max(self.n_slots, int(sl.max()) + 1 if n else 0)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_agg_state_update_host(
            self._h, n, int(n_slots), sl.ctypes.data, yv.ctypes.data, xv.ctypes.data,
            None if wv is None else wv.ctypes.data, None if vv is None else vv.ctypes.data, C.byref(err))
        if not ok:
            raise AnofoxStatsError(err.code, err.text())

    def update_device(self, slot, y, x_rowmajor, w=None, valid=None, n_slots: Optional[int] = None,
                      use_current_torch_stream: bool = True):
        """Device chunk (CUDA tensors): slot int32/uint32-as-int32[n], y[n], x_rowmajor[n, p], w[n], valid uint8[n]."""
        import torch
        n = int(y.numel())
        if n_slots is None:
            n_slots = max(self.n_slots, int(slot.max().item()) + 1 if n else 0)
        if use_current_torch_stream:
            self._ctx.set_stream(torch.cuda.current_stream(y.device).cuda_stream)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_agg_state_update_device(
            self._h, n, int(n_slots), C.c_void_p(slot.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(x_rowmajor.data_ptr()),
            C.c_void_p(w.data_ptr() if w is not None else 0), C.c_void_p(valid.data_ptr() if valid is not None else 0),
            C.byref(err))
        if not ok:
            raise AnofoxStatsError(err.code, err.text())

    def combine(self, source_slots, target_slots):
        src = np.ascontiguousarray(source_slots, dtype=np.uint32)
        dst = np.ascontiguousarray(target_slots, dtype=np.uint32)
        if len(src) != len(dst):
            raise ValueError("source and target differ in length")
        err = _abi.AnofoxError()
        if not self._lib.anofox_hip_agg_state_combine(self._h, len(src), src.ctypes.data, dst.ctypes.data, C.byref(err)):
            raise AnofoxStatsError(err.code, err.text())

    def finalize(self, n_slots: Optional[int] = None):
        """-> (core[G, p+6], inference[G, 5p+2] or None, number of groups flagged as unrefined: status 101, NaN record —
        they asked for the refinement passes and their rows were not kept)."""
        G = self.n_slots if n_slots is None else int(n_slots)
        p = self.p
        core = np.empty((G, p + 6), dtype=np.float64)
        inf = np.empty((G, 5 * p + 2), dtype=np.float64) if self.options.compute_inference else None
        unref = C.c_int64()
        slots = np.empty(max(G, 1), dtype=np.int32)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_agg_state_finalize_host(
            self._h, G, core.ctypes.data_as(_DP), None if inf is None else inf.ctypes.data_as(_DP), C.byref(unref),
            slots.ctypes.data, C.byref(err))
        if not ok:
            raise AnofoxStatsError(err.code, err.text())
        self.unrefined_slots = np.sort(slots[:int(unref.value)])   # groups that would have taken the refinement passes
        return core, inf, int(unref.value)

    def finalize_device(self, core, inference=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        import torch
        G = self.n_slots if n_slots is None else int(n_slots)
        if use_current_torch_stream:
            self._ctx.set_stream(torch.cuda.current_stream(core.device).cuda_stream)
        err = _abi.AnofoxError()
        ok = self._lib.anofox_hip_agg_state_finalize_device(
            self._h, G, C.c_void_p(core.data_ptr()), C.c_void_p(inference.data_ptr() if inference is not None else 0),
            C.byref(err))
        if not ok:
            raise AnofoxStatsError(err.code, err.text())
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

    def _finalize_family(self, family, fn_host, fn_slots, rec_len, options, slots, n_slots):
        self.check_family(family, options.fit_intercept)
        fn_host, fn_slots = getattr(self._lib, fn_host), getattr(self._lib, fn_slots)
        err = _abi.AnofoxError()
        unref = C.c_int64()
        if slots is None:
            G = self.n_slots if n_slots is None else int(n_slots)
            rec = np.empty((G, rec_len), dtype=np.float64)
            its = np.empty(G, dtype=np.int32)
            listed = np.empty(max(G, 1), dtype=np.int32)
            ok = fn_host(self._h, G, options, rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(unref),
                         listed.ctypes.data, C.byref(err))
            if not ok:
                raise AnofoxStatsError(err.code, err.text())
            return rec, its, listed[:int(unref.value)].copy()
        sl = np.ascontiguousarray(slots, dtype=np.uint32)
        rec = np.empty((len(sl), rec_len), dtype=np.float64)
        its = np.empty(len(sl), dtype=np.int32)
        ok = fn_slots(self._h, len(sl), sl.ctypes.data, options, rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)),
                      C.byref(unref), C.byref(err))
        if not ok:
            raise AnofoxStatsError(err.code, err.text())
        unrefined = sl[rec[:, self.p + 5] == _abi.STATUS_UNREFINED].astype(np.int32)
        if len(unrefined) != int(unref.value):
            raise AnofoxStatsError(_abi.ERROR_INTERNAL, f"{family} finalize: {int(unref.value)} slots counted as unrefined, {len(unrefined)} marked")
        return rec, its, unrefined

    def finalize_elasticnet(self, options: _abi.AnofoxHipElasticNetBatchOptions, slots=None, n_slots: Optional[int] = None):
        """The elastic net of every slot (or of the listed ones) from this state, which stays as it is:
        -> (core[G, p+6], iterations int32[G], the slot numbers that came back unrefined: status 101, NaN record)."""
        return self._finalize_family("elastic net", "anofox_hip_agg_state_finalize_elasticnet_host",
                                     "anofox_hip_agg_state_finalize_elasticnet_slots_host", self.p + 6, options, slots, n_slots)

    def finalize_bls(self, options: _abi.AnofoxHipBlsBatchOptions, slots=None, n_slots: Optional[int] = None):
        """Bounded / non-negative least squares of every slot (or of the listed ones) from this state:
        -> (bls[G, 3p+6], iterations int32[G], the unrefined slot numbers)."""
        return self._finalize_family("bounded least squares", "anofox_hip_agg_state_finalize_bls_host",
                                     "anofox_hip_agg_state_finalize_bls_slots_host", 3 * self.p + 6, options, slots, n_slots)

    def _finalize_family_device(self, family, fn, options, records, iterations, n_slots, use_current_torch_stream):
        import torch
        self.check_family(family, options.fit_intercept)
        fn = getattr(self._lib, fn)
        G = self.n_slots if n_slots is None else int(n_slots)
        if use_current_torch_stream:
            self._ctx.set_stream(torch.cuda.current_stream(records.device).cuda_stream)
        err = _abi.AnofoxError()
        if not fn(self._h, G, options, C.c_void_p(records.data_ptr()), C.c_void_p(iterations.data_ptr() if iterations is not None else 0),
                  C.byref(err)):
            raise AnofoxStatsError(err.code, err.text())
        return records, iterations

    def finalize_elasticnet_device(self, options, core, iterations=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        """core: float64 CUDA tensor [G, p+6]; iterations: int32 CUDA tensor [G] or None."""
        return self._finalize_family_device("elastic net", "anofox_hip_agg_state_finalize_elasticnet_device", options, core,
                                            iterations, n_slots, use_current_torch_stream)

    def finalize_bls_device(self, options, bls, iterations=None, n_slots: Optional[int] = None, use_current_torch_stream: bool = True):
        """bls: float64 CUDA tensor [G, 3p+6]; iterations: int32 CUDA tensor [G] or None."""
        return self._finalize_family_device("bounded least squares", "anofox_hip_agg_state_finalize_bls_device", options, bls,
                                            iterations, n_slots, use_current_torch_stream)


def fit_batch_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                   ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], inference[G, 5p+2] or None)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    p = len(cols)
    G = len(off) - 1
    N = len(yv)
    if any(len(c) != N for c in cols) or (wv is not None and len(wv) != N):
        raise ValueError("every column must have y's length")
    core = np.empty((G, p + 6), dtype=np.float64)
    inf = np.empty((G, 5 * p + 2), dtype=np.float64) if options.compute_inference else None
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_fit_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)),
        yv.ctypes.data_as(_DP), colp, None if wv is None else wv.ctypes.data_as(_DP), options,
        core.ctypes.data_as(_DP), None if inf is None else inf.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, inf


def elasticnet_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                              ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], iterations int32[G])."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p = len(cols)
    G = len(off) - 1
    N = len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    core = np.empty((G, p + 6), dtype=np.float64)
    its = np.empty((max(G, 0),), dtype=np.int32)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_elasticnet_fit_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, options, core.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, its


def bls_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions, ctx: Optional[Context] = None):
    """Grouped bounded least squares, numpy in / out: (bls[G, 3p+6], iterations int32[G]); the record layout is
    anofox_hip_bls_fit_batch_host's (include/anofox_stats_hip.h)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    rec = np.empty((G, 3 * p + 6), dtype=np.float64)
    its = np.empty((max(G, 0),), dtype=np.int32)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_bls_fit_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, options, rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return rec, its


def bls_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipBlsBatchOptions,
                               confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """Bounded least squares fit + predict, numpy in / out: (core[G, p+6] = coefficients, intercept, r2, ssr, sigma, n,
    status; pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    core = np.empty((G, p + 6), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_bls_fit_predict_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, float(confidence_level),
        core.ctypes.data_as(_DP), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def quantile_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, ctx: Optional[Context] = None):
    """Grouped quantile regression, numpy in / out: (quantile[G, p+6], iterations int32[G]); the record layout is
    anofox_hip_quantile_fit_batch_host's (include/anofox_stats_hip.h)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    rec = np.empty((G, p + 6), dtype=np.float64)
    its = np.empty((max(G, 0),), dtype=np.int32)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, options, rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return rec, its


def quantile_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions,
                                    train_counts=None, ctx: Optional[Context] = None):
    """Quantile regression fit + predict, numpy in / out: (core[G, p+6] = coefficients, intercept, NaN, NaN, NaN, n, status;
    pred[N, 3] = yhat, NaN, NaN; a NaN yhat = NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    core = np.empty((G, p + 6), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_predict_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, core.ctypes.data_as(_DP),
        pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def quantile_fit_path_batch_device(ctx: Context, row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                   **kwargs):
    """Context.quantile_fit_path_batch_device as a function (the device path needs an explicit context)."""
    return ctx.quantile_fit_path_batch_device(row_offsets, y, x_cols, options, taus, **kwargs)


def quantile_fit_path_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                 ctx: Optional[Context] = None):
    """The tau path, numpy in / out: (quantile[G, T, p+6], iterations int32[G, T]), indexed by the position in taus; the
    contract is anofox_hip_quantile_fit_path_batch_host's (include/anofox_stats_hip.h).  options.tau is ignored."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    tv = np.ascontiguousarray(taus, dtype=np.float64).ravel()
    p, G, N, T = len(cols), len(off) - 1, len(yv), len(tv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    rec = np.empty((G, T, p + 6), dtype=np.float64)
    its = np.empty((max(G, 0), T), dtype=np.int32)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_path_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, options, tv.ctypes.data_as(_DP), T, rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return rec, its


def quantile_fit_predict_path_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, taus,
                                         train_counts=None, ctx: Optional[Context] = None):
    """The tau path with its fused prediction, numpy in / out: (quantile[G, T, p+6], iterations int32[G, T], pred[N, T]);
    pred[i, t] is the prediction of row i at taus[t], NaN = NULL."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    tv = np.ascontiguousarray(taus, dtype=np.float64).ravel()
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N, T = len(cols), len(off) - 1, len(yv), len(tv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    rec = np.empty((G, T, p + 6), dtype=np.float64)
    its = np.empty((max(G, 0), T), dtype=np.int32)
    pred = np.empty((N, T), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_predict_path_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, tv.ctypes.data_as(_DP), T,
        rec.ctypes.data_as(_DP), its.ctypes.data_as(C.POINTER(C.c_int32)), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return rec, its, pred


def fit_predict_batch_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions, train_counts=None,
                           ctx: Optional[Context] = None):
    """numpy in, numpy out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = SQL NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    core = np.empty((G, p + 6), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_fit_predict_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, None if wv is None else wv.ctypes.data_as(_DP),
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, core.ctypes.data_as(_DP),
        pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def information_criteria_host(core, options: _abi.AnofoxHipBatchOptions, ctx: Optional[Context] = None):
    """numpy fit records [G, p+6] -> out[G, 3] = {rss, aic, bic} (anofox_hip_information_criteria_batch_host)."""
    lib = _abi.load()
    c = np.ascontiguousarray(core, dtype=np.float64)
    G, p = c.shape[0], c.shape[1] - 6
    out = np.empty((G, 3), dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_information_criteria_batch_host(ctx._h if ctx is not None else None, G, p, c.ctypes.data_as(_DP), options,
                                                        out.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return out


FRAME_UNBOUNDED = 2 ** 63 - 1        # ANOFOX_HIP_FRAME_UNBOUNDED


def _frame(frame) -> _abi.AnofoxHipWindowFrame:
    """(start, end) in rows PRECEDING the current row (negative = FOLLOWING); start None = UNBOUNDED PRECEDING,
    end None = UNBOUNDED FOLLOWING."""
    start, end = frame
    return _abi.AnofoxHipWindowFrame(FRAME_UNBOUNDED if start is None else int(start),
                                     -FRAME_UNBOUNDED if end is None else int(end))


def fit_predict_expanding_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                               ctx: Optional[Context] = None):
    """numpy in, numpy out: pred[N, 3] — prediction of x_e from the fit on rows 0..e of its partition."""
    return fit_predict_window_host(row_offsets, y, x_cols, w, options, (None, 0), ctx=ctx)


def fit_predict_window_host(row_offsets, y, x_cols: Sequence, w, options: _abi.AnofoxHipBatchOptions,
                            frame=(None, 0), ctx: Optional[Context] = None):
    """numpy in, numpy out: pred[N, 3] of the window functions over ROWS BETWEEN frame[0] PRECEDING AND frame[1]
    PRECEDING (negative = FOLLOWING; frame[0] None = UNBOUNDED PRECEDING, frame[1] 0 = CURRENT ROW, None = UNBOUNDED
    FOLLOWING)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_fit_predict_window_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        colp, None if wv is None else wv.ctypes.data_as(_DP), _frame(frame), options, pred.ctypes.data_as(_DP),
        C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred


def fit_predict_frames_host(y, x_cols: Sequence, w, frame_lo, frame_hi, options: _abi.AnofoxHipBatchOptions,
                            ctx: Optional[Context] = None):
    """Window fit + predict over explicit frames: frame of row e = rows [frame_lo[e], frame_hi[e]).  numpy in / out:
    pred[N, 3]."""
    lib = _abi.load()
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    lo = np.ascontiguousarray(frame_lo, dtype=np.int64)
    hi = np.ascontiguousarray(frame_hi, dtype=np.int64)
    p, N = len(cols), len(yv)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_fit_predict_frames_host(
        ctx._h if ctx is not None else None, N, p, yv.ctypes.data_as(_DP), colp, None if wv is None else wv.ctypes.data_as(_DP),
        lo.ctypes.data_as(C.POINTER(C.c_int64)), hi.ctypes.data_as(C.POINTER(C.c_int64)), options, pred.ctypes.data_as(_DP),
        C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred


def elasticnet_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                      confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """Elastic net fit + predict, numpy in / out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    core = np.empty((G, p + 6), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_elasticnet_fit_predict_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, float(confidence_level),
        core.ctypes.data_as(_DP), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def elasticnet_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipElasticNetBatchOptions,
                                       frame=(None, 0), confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """Elastic net window fit + predict over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3]."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_elasticnet_fit_predict_window_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        _frame(frame), options, float(confidence_level), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred


def elasticnet_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipElasticNetBatchOptions,
                                       confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """Elastic net fit + predict over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out: pred[N, 3]."""
    lib = _abi.load()
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    lo = np.ascontiguousarray(frame_lo, dtype=np.int64)
    hi = np.ascontiguousarray(frame_hi, dtype=np.int64)
    p, N = len(cols), len(yv)
    if any(len(c) != N for c in cols) or len(lo) != N or len(hi) != N:
        raise ValueError("every column and both frame bounds must have y's length")
    pred = np.empty((N, 3), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_elasticnet_fit_predict_frames_host(
        ctx._h if ctx is not None else None, N, p, yv.ctypes.data_as(_DP), colp, lo.ctypes.data_as(C.POINTER(C.c_int64)),
        hi.ctypes.data_as(C.POINTER(C.c_int64)), options, float(confidence_level), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred


def quantile_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipQuantileBatchOptions, frame=(None, 0),
                                     want_records: bool = False, ctx: Optional[Context] = None):
    """The quantile regression window function over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3] =
    {yhat, NaN, NaN}; with want_records (pred, quantile[N, p+6], iterations int32[N]) — the record of every frame in
    anofox_hip_quantile_fit_batch_host's layout and its pivots."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G, N = len(cols), len(off) - 1, len(yv)
    if any(len(c) != N for c in cols):
        raise ValueError("every column must have y's length")
    pred = np.empty((N, 3), dtype=np.float64)
    rec = np.empty((N, p + 6), dtype=np.float64) if want_records else None
    its = np.empty(N, dtype=np.int32) if want_records else None
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_predict_window_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        _frame(frame), options, pred.ctypes.data_as(_DP), rec.ctypes.data_as(_DP) if want_records else None,
        its.ctypes.data_as(C.POINTER(C.c_int32)) if want_records else None, C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return (pred, rec, its) if want_records else pred


def quantile_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipQuantileBatchOptions,
                                     want_records: bool = False, ctx: Optional[Context] = None):
    """The quantile regression window function over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out (as
    quantile_fit_predict_window_host)."""
    lib = _abi.load()
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    lo = np.ascontiguousarray(frame_lo, dtype=np.int64)
    hi = np.ascontiguousarray(frame_hi, dtype=np.int64)
    p, N = len(cols), len(yv)
    if any(len(c) != N for c in cols) or len(lo) != N or len(hi) != N:
        raise ValueError("every column and both frame bounds must have y's length")
    pred = np.empty((N, 3), dtype=np.float64)
    rec = np.empty((N, p + 6), dtype=np.float64) if want_records else None
    its = np.empty(N, dtype=np.int32) if want_records else None
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_quantile_fit_predict_frames_host(
        ctx._h if ctx is not None else None, N, p, yv.ctypes.data_as(_DP), colp, lo.ctypes.data_as(C.POINTER(C.c_int64)),
        hi.ctypes.data_as(C.POINTER(C.c_int64)), options, pred.ctypes.data_as(_DP), rec.ctypes.data_as(_DP) if want_records else None,
        its.ctypes.data_as(C.POINTER(C.c_int32)) if want_records else None, C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return (pred, rec, its) if want_records else pred


def quantile_window_plan(row_offsets, frame_lo, frame_hi, run_length: int = 0, scratch_cap_bytes: int = 0):
    """The planner of the quantile window function alone (host arrays, no device): -> (run_begin int64[walkers + 1], scratch
    rows per wavefront, launched wavefronts).  run_length / scratch_cap_bytes 0: the library's rule."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    lo = np.ascontiguousarray(frame_lo, dtype=np.int64)
    hi = np.ascontiguousarray(frame_hi, dtype=np.int64)
    if len(lo) != len(hi):
        raise ValueError("both frame bounds must have the same length")
    N = len(lo)
    runs = np.empty(N + 2, dtype=np.int64)
    n_runs, span, waves = C.c_int64(), C.c_int64(), C.c_int64()
    err = _abi.AnofoxError()
    I64 = C.POINTER(C.c_int64)
    ok = lib.anofox_hip_quantile_window_plan(len(off) - 1, off.ctypes.data_as(I64), N, lo.ctypes.data_as(I64), hi.ctypes.data_as(I64),
                                             int(run_length), int(scratch_cap_bytes), runs.ctypes.data_as(I64), len(runs),
                                             C.byref(n_runs), C.byref(span), C.byref(waves), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return runs[:n_runs.value + 1].copy(), int(span.value), int(waves.value)


def quantile_window_test_hooks(run_length: int = 0, scratch_cap_bytes: int = 0):
    """For tests and measurements: the run length and the scratch cap of every later window call (0: the library's rule)."""
    _abi.load().anofox_hip_quantile_window_test_hooks(int(run_length), int(scratch_cap_bytes))


def quantile_window_stats(ctx: Optional[Context] = None):
    """The most recent quantile window call on the context: dict(frames, cold_starts, walkers, waves, span_rows, restarts);
    cold_starts counts every frame that began afresh, restarts those of them that followed a fitted frame."""
    out = (C.c_int64 * 6)()
    err = _abi.AnofoxError()
    if not _abi.load().anofox_hip_quantile_window_stats(ctx._h if ctx is not None else None, out, C.byref(err)):
        raise AnofoxStatsError(err.code, err.text())
    return dict(frames=int(out[0]), cold_starts=int(out[1]), walkers=int(out[2]), waves=int(out[3]), span_rows=int(out[4]),
                restarts=int(out[5]))


def vif_batch_host(row_offsets, x_cols: Sequence, ctx: Optional[Context] = None):
    """numpy in, numpy out: out[G, p+1] = {vif[p], status} (status 100 = fewer than 3 rows -> SQL NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G = len(cols), len(off) - 1
    N = len(cols[0]) if cols else 0
    out = np.empty((G, p + 1), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_vif_batch_host(ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                       colp, out.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return out


def residuals_batch_host(row_offsets, y, y_hat, x_cols: Sequence = (), rse=None, include_studentized: bool = True,
                         drop_nan_rows: bool = True, ctx: Optional[Context] = None):
    """numpy in, numpy out: (out[N, 4] = raw / standardized / studentized / leverage, group[G, 2] = rows used / flags)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv = np.ascontiguousarray(y, dtype=np.float64)
    yh = np.ascontiguousarray(y_hat, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    p, G, N = len(cols), len(off) - 1, len(yv)
    out = np.empty((N, 4), dtype=np.float64)
    group = np.empty((G, 2), dtype=np.float64)
    colp = (_DP * max(p, 1))(*[c.ctypes.data_as(_DP) for c in cols])
    rse_arr = None if rse is None else np.ascontiguousarray(rse, dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_residuals_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP),
        yh.ctypes.data_as(_DP), colp if p else None, None if rse_arr is None else rse_arr.ctypes.data_as(_DP),
        bool(include_studentized), bool(drop_nan_rows), out.ctypes.data_as(_DP), group.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return out, group


def _host_cols(y, x_cols):
    yv = np.ascontiguousarray(y, dtype=np.float64)
    cols = [np.ascontiguousarray(c, dtype=np.float64) for c in x_cols]
    if any(len(c) != len(yv) for c in cols):
        raise ValueError("every column must have y's length")
    return yv, cols, (_DP * max(len(cols), 1))(*[c.ctypes.data_as(_DP) for c in cols])


def rls_fit_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, ctx: Optional[Context] = None):
    """Grouped RLS, numpy in / out: core[G, p+6] (DESIGN.md §1 "Recursive least squares")."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv, cols, colp = _host_cols(y, x_cols)
    p, G, N = len(cols), len(off) - 1, len(yv)
    core = np.empty((max(G, 0), p + 6), dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_rls_fit_batch_host(ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                           yv.ctypes.data_as(_DP), colp, options, core.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core


def rls_fit_predict_batch_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions,
                               confidence_level: float = 0.95, train_counts=None, ctx: Optional[Context] = None):
    """RLS fit + predict, numpy in / out: (core[G, p+6], pred[N, 3] = yhat / yhat_lower / yhat_upper, NaN = NULL)."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv, cols, colp = _host_cols(y, x_cols)
    tc = None if train_counts is None else np.ascontiguousarray(train_counts, dtype=np.int64)
    p, G, N = len(cols), len(off) - 1, len(yv)
    core = np.empty((max(G, 0), p + 6), dtype=np.float64)
    pred = np.empty((N, 3), dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_rls_fit_predict_batch_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        None if tc is None else tc.ctypes.data_as(C.POINTER(C.c_int64)), options, float(confidence_level),
        core.ctypes.data_as(_DP), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return core, pred


def rls_fit_predict_window_host(row_offsets, y, x_cols: Sequence, options: _abi.AnofoxHipRlsBatchOptions, frame=(None, 0),
                                confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """RLS window fit + predict over ROWS frames (as fit_predict_window_host), numpy in / out: pred[N, 3]."""
    lib = _abi.load()
    off = np.ascontiguousarray(row_offsets, dtype=np.int64)
    yv, cols, colp = _host_cols(y, x_cols)
    p, G, N = len(cols), len(off) - 1, len(yv)
    pred = np.empty((N, 3), dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_rls_fit_predict_window_host(
        ctx._h if ctx is not None else None, G, p, N, off.ctypes.data_as(C.POINTER(C.c_int64)), yv.ctypes.data_as(_DP), colp,
        _frame(frame), options, float(confidence_level), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred


def rls_fit_predict_frames_host(y, x_cols: Sequence, frame_lo, frame_hi, options: _abi.AnofoxHipRlsBatchOptions,
                                confidence_level: float = 0.95, ctx: Optional[Context] = None):
    """RLS fit + predict over explicit frames [frame_lo[e], frame_hi[e]), numpy in / out: pred[N, 3]."""
    lib = _abi.load()
    yv, cols, colp = _host_cols(y, x_cols)
    lo = np.ascontiguousarray(frame_lo, dtype=np.int64)
    hi = np.ascontiguousarray(frame_hi, dtype=np.int64)
    p, N = len(cols), len(yv)
    if len(lo) != N or len(hi) != N:
        raise ValueError("both frame bounds must have y's length")
    pred = np.empty((N, 3), dtype=np.float64)
    err = _abi.AnofoxError()
    ok = lib.anofox_hip_rls_fit_predict_frames_host(
        ctx._h if ctx is not None else None, N, p, yv.ctypes.data_as(_DP), colp, lo.ctypes.data_as(C.POINTER(C.c_int64)),
        hi.ctypes.data_as(C.POINTER(C.c_int64)), options, float(confidence_level), pred.ctypes.data_as(_DP), C.byref(err))
    if not ok:
        raise AnofoxStatsError(err.code, err.text())
    return pred
