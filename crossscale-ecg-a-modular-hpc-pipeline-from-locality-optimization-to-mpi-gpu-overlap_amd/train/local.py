"""Local (per-client) trainers.

``TorchLocalTrainer`` is the eager-PyTorch client (reference code path: per step ``next(batch_iter)``
device gather + fwd/CE/bwd/SGD, Module_3/TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py:197-204), used for
``--kernel-backend torch``, for models without a fused kernel (ResNet1D) and as the CPU/gloo path.
It shares the ``run_steps`` / ``avg_loss`` interface of ``ops.fused_tiny.FusedTinyTrainer``.

DP-SGD (``dp_clip`` > 0, the definition of ``FusedTinyTrainer``): per-sample gradients from ``torch.func``
(``functional_call`` + ``vmap(grad)``), clipped in fp32 to l2 norm ``dp_clip``, summed, plus ``dp_noise * dp_clip * z``
with ``z`` from ``utils/philox.py`` at (``dp_seed``, step counter), divided by B, then the optimizer's usual update.
The same seed and counter give the noise the HIP kernels draw.  The reported loss is not private.

FedProx (``prox_mu`` mu > 0): ``run_steps`` / ``run_round`` snapshot the weights ``a`` they start from, and every step
adds ``mu * (p - a)`` to ``p.grad`` in fp32 after ``backward()`` and before ``opt.step()`` - the gradient of
``mu / 2 * |w - a|^2`` passed through the optimizer like any other gradient, which is the definition
``slab_reduce_prox_sgd_kernel`` implements.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from ..data.dataset import DeviceIndexSampler
from ..utils import philox


def check_prox(prox_mu: float, amp_dtype, model) -> None:
    if not prox_mu >= 0.0:
        raise ValueError(f"prox_mu must be >= 0, got {prox_mu}")
    if prox_mu > 0.0:
        if amp_dtype == torch.float16:
            raise ValueError("FedProx does not support fp16 AMP (a GradScaler would rescale the proximal gradient)")
        if isinstance(model, torch.nn.parallel.DistributedDataParallel):
            raise ValueError("FedProx does not support a DistributedDataParallel model (--sync ddp)")


def add_prox_grad(params, anchors, mu: float) -> None:
    """``p.grad += mu * (p - a)`` for every parameter, computed in fp32."""
    with torch.no_grad():
        for p, a in zip(params, anchors):
            p.grad.add_(((p.detach().float() - a.detach().float()) * mu).to(p.grad.dtype))


class TorchLocalTrainer:
    def __init__(self, model: torch.nn.Module, x: torch.Tensor, y: torch.Tensor, batch_size: int,
                 lr: float = 1e-2, momentum: float = 0.9, weight_decay: float = 0.0,
                 amp_dtype: Optional[torch.dtype] = torch.bfloat16, seed: Optional[int] = None,
                 sync_each_step: bool = False, dp_clip: float = 0.0, dp_noise: float = 0.0,
                 dp_seed: Optional[int] = None, prox_mu: float = 0.0):
        check_prox(prox_mu, amp_dtype, model)
        if prox_mu > 0.0 and dp_clip > 0.0:
            raise ValueError("FedProx (prox_mu > 0) is not combined with DP-SGD (dp_clip > 0)")
        self.prox_mu = float(prox_mu)
        self._anchor = None  # FedProx: the weights the current round started from (set by run_steps)
        self.model, self.x, self.y, self.B = model, x, y, batch_size
        self.device = x.device
        self.opt = torch.optim.SGD(model.parameters(), lr=lr, momentum=momentum, weight_decay=weight_decay)
        self.amp_dtype = amp_dtype
        self.scaler = torch.amp.GradScaler("cuda") if (amp_dtype == torch.float16 and x.is_cuda) else None
        self.sampler = DeviceIndexSampler(x.shape[0], batch_size, self.device, seed=seed)
        self._idx = torch.empty((1, batch_size), dtype=torch.int32, device=self.device)
        self.loss_acc = torch.zeros((), dtype=torch.float32, device=self.device)
        self._loss_steps = 0
        self.sync_each_step = sync_each_step
        self.steps_done = 0
        if not dp_clip >= 0.0 or not dp_noise >= 0.0:
            raise ValueError(f"dp_clip and dp_noise must be >= 0, got {dp_clip} and {dp_noise}")
        if dp_noise > 0.0 and dp_clip == 0.0:
            raise ValueError("dp_noise > 0 needs a clip norm (dp_clip > 0): the noise is scaled by it")
        self.dp_clip, self.dp_noise = float(dp_clip), float(dp_noise)
        self.dp = self.dp_clip > 0.0
        self.dp_seed = (philox.mix64(0 if seed is None else seed) if dp_seed is None else int(dp_seed)) & philox.MASK64
        self.dp_steps = 0  # DP step counter: the t of the next step's noise
        if self.dp:
            if amp_dtype == torch.float16:
                raise ValueError("DP-SGD does not support fp16 AMP (a GradScaler would rescale the clipped gradients)")
            if isinstance(model, torch.nn.parallel.DistributedDataParallel):
                raise ValueError("DP-SGD does not support a DistributedDataParallel model (--sync ddp)")

    def _dp_step(self, xb: torch.Tensor, yb: torch.Tensor, use_amp: bool) -> torch.Tensor:
        """Per-sample gradients -> clip -> sum + noise -> /B into ``p.grad``, then ``opt.step()``."""
        from torch.func import functional_call, grad, vmap
        names = [n for n, _ in self.model.named_parameters()]
        params = {n: p.detach() for n, p in self.model.named_parameters()}

        def sample_loss(p, x1, y1):
            with torch.autocast(device_type=self.device.type, dtype=self.amp_dtype or torch.float32, enabled=use_amp):
                loss = F.cross_entropy(functional_call(self.model, p, (x1.unsqueeze(0),)), y1.unsqueeze(0))
            return loss, loss.detach()

        grads, losses = vmap(grad(sample_loss, has_aux=True), in_dims=(None, 0, 0))(params, xb, yb)
        B = xb.shape[0]
        g = torch.cat([grads[n].reshape(B, -1).float() for n in names], dim=1)  # [B, P]
        norms = g.norm(dim=1)
        c = torch.where(norms > 0, (self.dp_clip / norms).clamp(max=1.0), torch.ones_like(norms))
        total = (g * c[:, None]).sum(0)
        if self.dp_noise > 0.0:
            z = philox.normal(self.dp_seed, self.dp_steps, g.shape[1])
            total = total + (self.dp_noise * self.dp_clip) * torch.from_numpy(z).to(total)
        total = total / B
        off = 0
        for p in self.model.parameters():
            p.grad = total[off:off + p.numel()].view_as(p).to(p.dtype)
            off += p.numel()
        self.opt.step()
        self.dp_steps += 1
        return losses.float().mean()

    def set_dp_steps(self, n: int) -> None:
        """Continue the noise stream at step ``n`` (checkpoint resume)."""
        self.dp_steps = int(n)

    def step(self) -> torch.Tensor:
        self.sampler.fill(self._idx)
        sel = self._idx[0].long()
        xb, yb = self.x[sel].unsqueeze(1), self.y[sel]
        self.model.train()
        self.opt.zero_grad(set_to_none=True)
        use_amp = self.amp_dtype is not None and (self.device.type == "cuda" or self.amp_dtype == torch.bfloat16)
        if self.dp:
            loss = self._dp_step(xb, yb, use_amp)
            if self.sync_each_step and self.device.type == "cuda":
                torch.cuda.synchronize(self.device)
            self.steps_done += 1
            return loss
        with torch.autocast(device_type=self.device.type, dtype=self.amp_dtype or torch.float32, enabled=use_amp):
            loss = F.cross_entropy(self.model(xb), yb)
        if self.scaler is not None:
            self.scaler.scale(loss).backward()
            self.scaler.step(self.opt)
            self.scaler.update()
        else:
            loss.backward()
            if self.prox_mu > 0.0:
                if self._anchor is None:  # a step outside run_steps anchors on the weights it finds
                    self._anchor = [p.detach().clone() for p in self.model.parameters()]
                add_prox_grad(self.model.parameters(), self._anchor, self.prox_mu)
            self.opt.step()
        if self.sync_each_step and self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.steps_done += 1
        return loss.detach()

    def run_steps(self, n: int, reset_loss: bool = True) -> None:
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0
        if self.prox_mu > 0.0:
            self._anchor = [p.detach().clone() for p in self.model.parameters()]
        for _ in range(n):
            self.loss_acc += self.step().float()
        self._loss_steps += n

    run_round = run_steps

    def prepare_round(self, n: int, reset_loss: bool = True) -> None:
        """Eager steps draw their batch inside ``step``; only the loss window is reset here."""
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0

    def launch_round(self, n: int, next_n=None) -> None:
        self.run_steps(n, reset_loss=False)

    def avg_loss(self) -> float:
        return float(self.loss_acc.item()) / max(1, self._loss_steps)

    def reset_momentum(self):
        for st in self.opt.state.values():
            if "momentum_buffer" in st and st["momentum_buffer"] is not None:
                st["momentum_buffer"].zero_()
