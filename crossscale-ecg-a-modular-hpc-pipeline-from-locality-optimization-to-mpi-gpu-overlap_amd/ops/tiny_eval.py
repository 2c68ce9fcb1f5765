"""Evaluation of a classifier on a set of windows: loss, accuracy and the confusion matrix.

``tiny_evaluate`` is the Python side of csrc/kernels/tiny_ecg_eval.hip: a persistent forward-only TinyECG kernel
(bf16 MFMA operands, fp32 accumulation, one wave per window, no workgroup barrier) that reduces the metrics inside
the launch - the production path writes neither predictions nor logits.  ``precision="fp32"`` runs the fp32
forward kernel of the training step in chunks and computes the metrics with torch ops (correct, not hot).
``evaluate_torch`` is the eager path for every other model / backend and for the CPU.  All three return the same
``EvalResult`` record of device tensors, which synchronises only when one of its properties is read.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from . import _lib
from ..models.tiny_ecg import num_params

MAX_CLASSES = 16


class EvalResult:
    """Metrics of one evaluation as device tensors: ``loss_sum`` float64 [1], ``counts`` int64 [2 + C*C] =
    {count, correct, conf[true][pred] row-major}; ``pred`` int32 [N] / ``logits`` fp32 [N, C] when requested.
    Reading ``loss`` / ``accuracy`` / ``confusion`` / ``count`` copies to the host (synchronises)."""

    def __init__(self, loss_sum: torch.Tensor, counts: torch.Tensor, num_classes: int,
                 pred: Optional[torch.Tensor] = None, logits: Optional[torch.Tensor] = None):
        self.loss_sum_t, self.counts_t, self.num_classes = loss_sum, counts, int(num_classes)
        self._pred, self._logits = pred, logits

    @property
    def count(self) -> int:
        return int(self.counts_t[0].item())

    @property
    def correct(self) -> int:
        return int(self.counts_t[1].item())

    @property
    def loss_sum(self) -> float:
        return float(self.loss_sum_t.item())

    @property
    def loss(self) -> float:
        """Mean cross-entropy per window."""
        n = self.count
        return self.loss_sum / n if n else float("nan")

    @property
    def accuracy(self) -> float:
        n = self.count
        return self.correct / n if n else float("nan")

    @property
    def confusion(self) -> torch.Tensor:
        """int64 [C, C] on the host: ``confusion[true][pred]``."""
        return self.counts_t[2:].reshape(self.num_classes, self.num_classes).cpu()

    @property
    def pred(self) -> Optional[torch.Tensor]:
        return self._pred

    @property
    def logits(self) -> Optional[torch.Tensor]:
        return self._logits

    # one float64 vector (for a single all_reduce(SUM) across clients; counts are exact below 2^53)
    def to_vector(self) -> torch.Tensor:
        return torch.cat([self.loss_sum_t.reshape(1).double(), self.counts_t.double()])

    @staticmethod
    def from_vector(v: torch.Tensor, num_classes: int) -> "EvalResult":
        return EvalResult(v[:1].clone(), v[1:].round().to(torch.int64), num_classes)


def confusion_str(conf: torch.Tensor) -> str:
    """Row-major integers in one CSV field: rows joined by ';', entries by ' ' (e.g. ``"3 1;0 4"``)."""
    return ";".join(" ".join(str(int(v)) for v in row) for row in conf.tolist())


def metrics_from_logits(logits: torch.Tensor, y: torch.Tensor, num_classes: int):
    """(loss_sum float64 [1], counts int64 [2 + C*C], pred) of ``logits`` [n, C] against labels ``y`` with torch ops."""
    y = y.long()
    pred = logits.argmax(1)
    loss_sum = F.cross_entropy(logits.double(), y, reduction="sum").reshape(1)
    conf = torch.bincount(y * num_classes + pred, minlength=num_classes * num_classes)
    counts = torch.cat([torch.tensor([y.numel()], dtype=torch.int64, device=y.device),
                        (pred == y).sum().reshape(1), conf])
    return loss_sum, counts, pred


def evaluate_torch(model: torch.nn.Module, x: torch.Tensor, y: torch.Tensor, chunk: int = 4096) -> EvalResult:
    """Evaluate ``model`` (eval mode, no grad, fp32) on windows ``x`` [N, L] in chunks of ``chunk`` windows; the
    model's previous train / eval mode is restored."""
    nc = int(getattr(model, "num_classes", 0)) or None
    was_training = model.training
    model.eval()
    loss_sum = counts = None
    try:
        with torch.no_grad():
            for s in range(0, x.shape[0], int(chunk)):
                xb = x[s:s + chunk]
                logits = model(xb.unsqueeze(1) if xb.dim() == 2 else xb).float()
                nc = nc or logits.shape[1]
                ls, ct, _ = metrics_from_logits(logits, y[s:s + chunk], nc)
                loss_sum = ls if loss_sum is None else loss_sum + ls
                counts = ct if counts is None else counts + ct
    finally:
        model.train(was_training)
    if counts is None:
        raise ValueError("evaluate_torch: no windows")
    return EvalResult(loss_sum, counts, nc)


def _check_inputs(flat_params, x, y32, idx, num_classes):
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
    if x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.stride(1) != 1 or x.shape[0] < 1:
        raise ValueError(f"windows must be a CUDA float32 [N, L] tensor with unit stride along L, got {x.dtype} "
                         f"{tuple(x.shape)} stride {x.stride()} on {x.device}")
    if (flat_params.dtype != torch.float32 or flat_params.device != x.device or not flat_params.is_contiguous()
            or flat_params.numel() < num_params(num_classes)):
        raise ValueError("flat_params must be a contiguous float32 tensor on the windows' device holding the "
                         f"{num_params(num_classes)} TinyECG parameters")
    if y32 is not None and (y32.dtype != torch.int32 or y32.dim() != 1 or y32.shape[0] != x.shape[0]
                            or y32.device != x.device or not y32.is_contiguous()):
        raise ValueError("labels must be a contiguous int32 [N] tensor (one per row of x) on the windows' device")
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 1 or idx.numel() < 1 or idx.device != x.device
                            or not idx.is_contiguous()):
        raise ValueError("idx must be a contiguous int32 [n] tensor on the windows' device")


class TinyEvaluator:
    """The buffers of the evaluation kernel for one device and class count, allocated once: its own
    prepared-fragment image (rebuilt from the weights on every call), the loss-partial scratch and the output
    record.  A result's metric tensors are these buffers: read them before the next ``run``."""

    def __init__(self, device, num_classes: int):
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [1, {MAX_CLASSES}], got {num_classes}")
        lib = _lib.kernels()
        self.device, self.nc = torch.device(device), int(num_classes)
        self.wprep = torch.zeros(lib.ecg_tiny_wprep_bytes(), dtype=torch.uint8, device=device)
        self.scratch = torch.zeros(lib.ecg_tiny_eval_scratch_bytes(self.nc) // 8, dtype=torch.float64, device=device)
        self.out = torch.zeros(lib.ecg_tiny_eval_out_bytes(self.nc) // 8, dtype=torch.int64, device=device)

    def run(self, flat_params: torch.Tensor, x: torch.Tensor, y32: Optional[torch.Tensor],
            idx: Optional[torch.Tensor] = None, return_pred: bool = False, return_logits: bool = False,
            max_workgroups: int = 0) -> EvalResult:
        _check_inputs(flat_params, x, y32, idx, self.nc)
        n = x.shape[0] if idx is None else idx.numel()
        if y32 is None and not (return_pred or return_logits):
            return_pred = return_logits = True  # pure inference: predictions and logits are the result
        pred = torch.empty(n, dtype=torch.int32, device=x.device) if return_pred else None
        logits = torch.empty((n, self.nc), dtype=torch.float32, device=x.device) if return_logits else None
        st = _lib.kernels().ecg_tiny_eval(
            x.data_ptr(), x.shape[1], x.stride(0), _lib.ptr(idx), _lib.ptr(y32), n, flat_params.data_ptr(), self.nc,
            self.wprep.data_ptr(), self.scratch.data_ptr(), self.out.data_ptr(), _lib.ptr(pred), _lib.ptr(logits),
            int(max_workgroups), _lib.stream_ptr(x.device))
        _lib.check(st, "ecg_tiny_eval")
        return EvalResult(self.out[:1].view(torch.float64), self.out[1:], self.nc, pred, logits)


def _evaluate_fp32(flat_params, x, y32, idx, num_classes, return_pred, return_logits, chunk=16384) -> EvalResult:
    """fp32: the training step's fp32 forward kernel over the range in chunks, metrics with torch ops."""
    from .fused_tiny import tiny_forward
    n = x.shape[0] if idx is None else idx.numel()
    outs = []
    for s in range(0, n, chunk):
        b = min(chunk, n - s)
        if idx is None:
            outs.append(tiny_forward(flat_params, x[s:s + b], None, b, num_classes, "fp32", prefrag=False))
        else:
            outs.append(tiny_forward(flat_params, x, idx[s:s + b], b, num_classes, "fp32", prefrag=False))
    logits = torch.cat(outs)
    if y32 is None:
        z = torch.zeros(2 + num_classes * num_classes, dtype=torch.int64, device=x.device)
        return EvalResult(torch.zeros(1, dtype=torch.float64, device=x.device), z, num_classes,
                          logits.argmax(1).int(), logits)
    y = y32 if idx is None else y32[idx.long()]
    loss_sum, counts, pred = metrics_from_logits(logits, y, num_classes)
    return EvalResult(loss_sum, counts, num_classes, pred.int() if return_pred else None,
                      logits if return_logits else None)


def tiny_evaluate(flat_params: torch.Tensor, x: torch.Tensor, y32: Optional[torch.Tensor],
                  idx: Optional[torch.Tensor] = None, num_classes: int = 2, precision: str = "bf16",
                  return_pred: bool = False, return_logits: bool = False, max_workgroups: int = 0,
                  evaluator: Optional[TinyEvaluator] = None) -> EvalResult:
    """Evaluate TinyECG with weights ``flat_params`` on windows ``x[idx[i]]`` (every row of ``x`` when ``idx`` is
    None) against int32 labels ``y32`` (one per ROW of ``x``, in [0, num_classes); None: inference only, the result
    holds ``pred`` and ``logits`` and zero metrics).  ``x`` may be any row-slice view of a resident shard (storage
    offset, odd alignment, row stride > L).  Enqueued on the current stream; nothing synchronises.
    ``max_workgroups`` (> 0) caps the persistent grid - a test knob; ``evaluator`` reuses a ``TinyEvaluator``'s
    buffers instead of allocating them."""
    if precision not in ("bf16", "fp32"):
        raise ValueError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
    if precision == "fp32":
        _check_inputs(flat_params, x, y32, idx, num_classes)
        return _evaluate_fp32(flat_params, x, y32, idx, num_classes, return_pred, return_logits)
    ev = evaluator if evaluator is not None else TinyEvaluator(x.device, num_classes)
    if ev.nc != int(num_classes):
        raise ValueError(f"evaluator was built for {ev.nc} classes, not {num_classes}")
    return ev.run(flat_params, x, y32, idx, return_pred, return_logits, max_workgroups)
