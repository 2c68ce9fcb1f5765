"""Operand-exact reference of the fused TinyECG kernels (numerics oracle for csrc/kernels/tiny_ecg_step.hip and
tiny_ecg_eval.hip): plain PyTorch on the CPU, float64 by default, no autograd - forward and backward are written out
with the kernel's algebra, and values are rounded to bf16 exactly where the bf16 kernels round them.

Rounding points with ``rounding="bf16"`` (read from the kernel: ``wprep_put`` / ``put_param`` / ``load_aw``,
``conv1_operand``, ``conv1_pair``, ``conv2``, ``head_and_M``, ``dgrad``, and the comment above ``TinySample``):

* MFMA operands: the window x, w1, b1, w2 and b2 are bf16 (both biases ride in the K padding of their GEMM);
* ``h1 = bf16(relu(acc1))``; relu'(h1) is ``h1 > 0`` of the stored bf16 value (the sign of the fp32 accumulator for
  every accumulator that is not below the smallest bf16 subnormal);
* conv2's accumulator, ``m = relu'(h2)`` (exact 0 / 1), the mean pool, the head (unrounded head weights), the
  softmax cross-entropy, ``dWh``, ``dbh`` and ``g`` are fp32;
* ``g = (dlogits @ Wh) / L`` with ``dlogits = (softmax - onehot) * loss_scale``: both the loss scale (1 / B) and the
  1 / L of the pool are inside ``g`` before anything is rounded;
* ``M = sum_t m h1`` (fp32 accumulation of bf16 h1), ``dW2 = g M`` and ``db2 = g sum_t m`` in fp32;
* the conv2 dgrad operand is ``bf16(bf16(w2) * g)``, its other operand the exact mask;
* ``dh1 = bf16(acc) * relu'(h1)``, stored over h1;
* ``dW1`` and ``db1`` are sums over t of ``dh1`` (bf16) times the bf16 window (fp32 accumulation).

``rounding=None`` rounds nowhere: the computation of the fp32 kernels (``precision="fp32"``) and, in float64, plain
autograd of ``TinyECG`` (tests/test_tiny_ref_cpu.py checks that to 1e-10).  ``dtype=torch.float32`` evaluates the same
model in fp32: the difference from float64 is the reference's own noise floor - summation order, and the rare value
that lands on the other side of a bf16 rounding boundary or of a ReLU because of it.

What is left between a kernel and this reference is of that kind only: the order of the kernel's fp32 sums (MFMA
blocks of 32 steps, per-wave partials), its fp32 ``exp`` / ``log``, and the double rounding fp32 -> bf16 of
``bf16(w2) * g``.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import torch
import torch.nn.functional as F

from .tiny_ecg import C_HID, K1, K2, P1, P2, num_params, param_layout

INTERMEDIATES = ("h1", "m", "g", "dh1")


class TinyRef(NamedTuple):
    logits: torch.Tensor  # [B, nc]
    loss: torch.Tensor    # [B] per-sample cross-entropy (not scaled)
    rows: torch.Tensor    # [B, P + 1]: per-sample gradient (times loss_scale) in param_layout order, loss in column P
    inter: Dict[str, torch.Tensor]  # h1 [B, 16, L], m [B, 16, L], g [B, 16], dh1 [B, 16, L]


def _bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _identity(t: torch.Tensor) -> torch.Tensor:
    return t


def split_params(flat: torch.Tensor, num_classes: int, dtype=torch.float64):
    """The six parameter tensors (param_layout order) of a flat vector, as ``dtype`` on the CPU."""
    out = []
    flat = flat.detach().cpu()
    for off, shp in param_layout(num_classes).values():
        n = 1
        for s in shp:
            n *= s
        out.append(flat[off:off + n].to(dtype).reshape(shp))
    return out


def tiny_ecg_reference(flat_params: torch.Tensor, x: torch.Tensor, y: torch.Tensor, loss_scale: float,
                       num_classes: int = 2, dtype: torch.dtype = torch.float64, rounding: Optional[str] = "bf16",
                       replace: Optional[Dict[str, torch.Tensor]] = None) -> TinyRef:
    """Forward and per-sample backward of TinyECG for windows ``x`` [B, L], labels ``y`` [B] and the weights
    ``flat_params`` (>= P floats, param_layout order).  ``loss_scale`` multiplies every gradient (1 / B for the mean
    loss of a batch of B); the loss column is not scaled.  ``replace``: tensors that stand in for the named
    intermediates (``INTERMEDIATES``) - teacher forcing: everything downstream is computed from the replacement."""
    if rounding not in ("bf16", None):
        raise ValueError(f"rounding must be 'bf16' or None, got {rounding!r}")
    replace = dict(replace or {})
    unknown = set(replace) - set(INTERMEDIATES)
    if unknown:
        raise ValueError(f"unknown intermediates {sorted(unknown)}; known: {INTERMEDIATES}")
    R = _bf16 if rounding == "bf16" else _identity
    w1, b1, w2, b2, wh, bh = split_params(flat_params, num_classes, dtype)
    x = x.detach().cpu().to(dtype)
    y = y.detach().cpu().long()
    B, L = x.shape
    rows_i = torch.arange(B)

    def forced(name, value):
        return replace[name].to(dtype) if name in replace else value

    # forward
    xb, w1b, b1b, w2b, b2b = R(x), R(w1), R(b1), R(w2), R(b2)
    h1 = forced("h1", R(F.relu(F.conv1d(xb[:, None], w1b, b1b, padding=P1))))
    m1 = (h1 > 0).to(dtype)
    a2 = F.conv1d(h1, w2b, b2b, padding=P2)
    m = forced("m", (a2 > 0).to(dtype))
    pooled = (a2 * m).sum(2) / L
    logits = pooled @ wh.T + bh
    logp = torch.log_softmax(logits, 1)
    loss = -logp[rows_i, y]

    # backward
    dlogits = torch.exp(logp)
    dlogits[rows_i, y] -= 1.0
    dlogits = dlogits * loss_scale
    dwh = dlogits[:, :, None] * pooled[:, None, :]
    g = forced("g", (dlogits @ wh) / L)
    h1p = F.pad(h1, (P2, P2))
    # M[b, co, ci, k] = sum_t m[b, co, t] h1[b, ci, t + k - 2]
    M = torch.stack([torch.einsum("bot,bit->boi", m, h1p[:, :, k:k + L]) for k in range(K2)], 3)
    dw2 = g[:, :, None, None] * M
    db2 = g * m.sum(2)
    w2g = R(w2b[None] * g[:, :, None, None])  # [B, co, ci, k]
    mp = F.pad(m, (P2, P2))
    # dh1[b, ci, t] = sum_{co, k} m[b, co, t - k + 2] w2g[b, co, ci, k]
    acc = sum(torch.einsum("bot,boi->bit", mp[:, :, 2 * P2 - k:2 * P2 - k + L], w2g[:, :, :, k]) for k in range(K2))
    dh1 = forced("dh1", R(acc) * m1)
    xp = F.pad(xb, (P1, P1))
    dw1 = torch.stack([torch.einsum("bit,bt->bi", dh1, xp[:, k:k + L]) for k in range(K1)], 2)
    db1 = dh1.sum(2)

    rows = torch.cat([dw1.reshape(B, -1), db1, dw2.reshape(B, -1), db2, dwh.reshape(B, -1), dlogits,
                      loss[:, None]], 1)
    assert rows.shape[1] == num_params(num_classes) + 1 and dw1.shape[1] == C_HID
    return TinyRef(logits, loss, rows, {"h1": h1, "m": m, "g": g, "dh1": dh1})


def row_tensors(num_classes: int):
    """(name, column slice) of every parameter tensor in a gradient row, then ("loss", the loss column)."""
    out = []
    for name, (off, shp) in param_layout(num_classes).items():
        n = 1
        for s in shp:
            n *= s
        out.append((name, slice(off, off + n)))
    P = num_params(num_classes)
    out.append(("loss", slice(P, P + 1)))
    return out


def row_errors(got: torch.Tensor, ref: torch.Tensor, num_classes: int):
    """Per tensor of the row layout: the worst over the sample rows of ``|got - ref|_2 / |ref|_2`` (float64).  A
    reference tensor that is exactly zero (a sample none of whose conv1 outputs is active) must be matched exactly:
    its error is 0 then and infinite otherwise."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    out = {}
    for name, sl in row_tensors(num_classes):
        d, r = (got[:, sl] - ref[:, sl]).norm(dim=1), ref[:, sl].norm(dim=1)
        e = torch.where(r > 0, d / r.clamp_min(1e-300), torch.where(d > 0, torch.full_like(d, float("inf")), d))
        out[name] = e.max().item()
    return out


def logit_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref|."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return ((got - ref).abs().max() / ref.abs().max()).item()
