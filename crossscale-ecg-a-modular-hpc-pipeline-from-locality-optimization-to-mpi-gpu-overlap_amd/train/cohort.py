"""``TorchCohortTrainer``: cohorts of virtual clients on eager PyTorch - the independent reference of
``ops.fused_cohort.FusedCohortTrainer`` and the CPU / ``--kernel-backend torch`` path.  Correct, not fast.

Per round: the cohort and its batches from the same ``CohortSampler`` (same ``(seed, round)`` -> same table on the same
device); for every cohort client a copy of the global weights, ``S`` plain SGD steps with zero initial momentum on its
columns of the table, then ``global = (((p_0 + p_1) + ...) + p_{M-1}) * fp32(1 / M)`` in ascending cohort order,
written into the model's parameters (its flat buffer when it has one).
"""
from __future__ import annotations

import copy
from typing import List, Optional

import torch
import torch.nn.functional as F

from ..data.dataset import CohortSampler


class TorchCohortTrainer:
    def __init__(self, model: torch.nn.Module, x: torch.Tensor, y: torch.Tensor, batch_size: int,
                 steps_per_round: int, clients: int, cohort: Optional[int] = None, lr: float = 1e-2,
                 momentum: float = 0.9, weight_decay: float = 0.0, nesterov: bool = False,
                 amp_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None, dp_clip: float = 0.0):
        if dp_clip > 0.0:
            raise ValueError("DP-SGD (dp_clip > 0) is not implemented for cohorts of virtual clients")
        self.model, self.x, self.y = model, x, y
        self.device = x.device
        self.B, self.S, self.K = int(batch_size), int(steps_per_round), int(clients)
        self.M = self.K if not cohort else int(cohort)
        self.opt_args = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        self.amp_dtype = amp_dtype
        self.sampler = CohortSampler(x.shape[0], self.B, self.S, self.K, self.M, self.device, seed=seed)
        self.table = torch.zeros((self.S, self.M * self.B), dtype=torch.int32, device=self.device)
        self.work = copy.deepcopy(model)  # one client's model: reloaded from the global weights per client
        if getattr(self.work, "_flat", None) is not None:
            self.work._flat = None  # plain parameters: nothing reads the copy's flat buffer
        self.loss_acc = torch.zeros((), dtype=torch.float32, device=self.device)
        self._loss_steps = 0
        self.cohort_round = 0
        self.round_clients: List[int] = []
        self.steps_done = 0
        self.precision = "fp32" if amp_dtype is None else str(amp_dtype).replace("torch.", "").replace("bfloat16", "bf16")

    def set_cohort_round(self, r: int) -> None:
        self.cohort_round = int(r)

    def _client_round(self, j: int, n: int, table: torch.Tensor) -> List[torch.Tensor]:
        """Client j of the cohort: ``n`` SGD steps from the global weights; returns its parameters (detached copies)."""
        with torch.no_grad():
            for pw, pg in zip(self.work.parameters(), self.model.parameters()):
                pw.copy_(pg)
        opt = torch.optim.SGD(self.work.parameters(), **self.opt_args)  # fresh: zero momentum
        use_amp = self.amp_dtype is not None and (self.device.type == "cuda" or self.amp_dtype == torch.bfloat16)
        self.work.train()
        for s in range(n):
            sel = table[s, j * self.B:(j + 1) * self.B].long()
            xb, yb = self.x[sel].unsqueeze(1), self.y[sel]
            opt.zero_grad(set_to_none=True)
            with torch.autocast(device_type=self.device.type, dtype=self.amp_dtype or torch.float32, enabled=use_amp):
                loss = F.cross_entropy(self.work(xb), yb)
            loss.backward()
            opt.step()
            self.loss_acc += loss.detach().float()
        return [p.detach().clone() for p in self.work.parameters()]

    def run_table(self, n: int, table: torch.Tensor) -> None:
        """One cohort round on ``table`` (int32 ``[>= n, M * B]``): the clients one after another, then the mean."""
        total = None
        for j in range(self.M):
            ps = self._client_round(j, n, table)
            total = ps if total is None else [t + p for t, p in zip(total, ps)]
        inv = torch.tensor(1.0 / self.M, dtype=torch.float32, device=self.device)  # fp32(1 / M), rounded once
        with torch.no_grad():
            for pg, t in zip(self.model.parameters(), total):
                pg.copy_(t * inv)
        self.steps_done += n
        self._loss_steps += n

    def run_steps(self, n: int, reset_loss: bool = True) -> None:
        self.prepare_round(n, reset_loss)
        self.launch_round(n)

    run_round = run_steps

    def prepare_round(self, n: int, reset_loss: bool = True) -> None:
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0

    def launch_round(self, n: int, next_n=None) -> None:
        self.round_clients = self.sampler.fill(self.cohort_round, self.table)
        self.cohort_round += 1
        self.run_table(n, self.table)

    def avg_loss(self) -> float:
        return float(self.loss_acc.item()) / (self.M * max(1, self._loss_steps))
