"""``TorchCohortTrainer``: cohorts of virtual clients on eager PyTorch - the independent reference of
``ops.fused_cohort.FusedCohortTrainer`` and the CPU / ``--kernel-backend torch`` path.  Correct, not fast.

Per round: the cohort and its batches from the same ``CohortSampler`` (same ``(seed, round)`` -> same table on the same
device); for every cohort client a copy of the global weights, ``S`` plain SGD steps with zero initial momentum on its
columns of the table, then ``global = (((p_0 + p_1) + ...) + p_{M-1}) * fp32(1 / M)`` in ascending cohort order,
written into the model's parameters (its flat buffer when it has one).

Client-level DP (``client_dp_clip`` C > 0; DP-FedAvg) and a server step size ``server_lr`` eta != 1 replace that mean:
with g the global weights the round started from, ``d_c = p_c - g`` over all P parameters, ``n_c = |d_c|_2`` and
``s_c = min(1, C / n_c)`` (``n_c == 0 -> 1``; C == 0: no clipping),

    g_new = g + eta * ((((s_0 d_0 + s_1 d_1) + ...) + s_{M-1} d_{M-1}) * fp32(1 / M) + nu * z)

in fp32, ``nu = fp32(sigma * C / (M * sqrt(W)))`` with sigma = ``client_dp_noise`` and W = ``world_size`` (the driver
averages W ranks' weights, which leaves noise of standard deviation sigma * C / (M * W) on a mean of sensitivity
C / (M * W)), and ``z = philox.normal(client_dp_seed, round, P, stream=1)``: the definition that
``cohort_dp_mean_kernel`` of csrc/kernels/tiny_ecg_close.hip implements.

A server optimizer (``server_opt`` sgdm / adagrad / adam / yogi; ``train/server_opt.py`` states the rules) takes the
bracket above - Delta, the averaged, clipped, noised delta - as its pseudo-gradient in place of the plain step
``g + eta * Delta``; its state ``server_m`` / ``server_v`` lives across rounds (``server_state`` / ``load_server_state``).

``server_scope="global"`` takes the same two phases apart: ``launch_round`` ends with Delta in ``server_delta`` (a
tensor written in place) and the model untouched, and ``apply_server_step`` takes the plain step or the optimizer's on
whatever ``server_delta`` then holds - the mean of the ranks' Deltas once a driver all-reduced it.

FedProx (``prox_mu`` mu > 0): every client's local objective gains ``mu / 2 * |w - g|^2``, g the global weights the
round started from: after ``backward()`` every ``p.grad`` gains ``mu * (p - g)`` in fp32, before ``opt.step()`` - the
definition ``slab_reduce_cohort_prox_sgd_kernel`` implements.  ``partition="shards"``: label-skewed clients
(``data.dataset.shard_partition``).

Unequal clients (``partition="dirichlet"`` with ``dirichlet_alpha``: ``data.dataset.dirichlet_partition``, client k owns
``n_k`` rows), unequal local work (``local_epochs`` E > 0: client c of the cohort runs the first
``S_c = min(S, max(1, E * (n_c // B)))`` rows of its table columns; 0: all S) and the aggregate (``weights_of``):
``Delta = ((w_0 d_0 + w_1 d_1) + ...) + w_{M-1} d_{M-1}`` in ascending cohort order in fp32, with ``p_c = n_c / sum n_c``
over the cohort and w_c = ``p_c`` ("weighted", FedAvg's own weights) or ``p_c * tau_eff / a_c`` ("nova", FedNova: Wang et
al., "Tackling the Objective Inconsistency Problem in Heterogeneous Federated Optimization"); "mean" keeps the closes
above, ``1 / M`` each.  Delta then takes the server step or the split close exactly as the unweighted one does; there is
no clip and no noise on a weighted Delta (its sensitivity is not C / M).  ``cohort_delta_wscale_kernel`` and the STEPS
form of the cohort reduce implement these definitions.  Every rank normalises over its own cohort.

Robust aggregates (``robust`` "trimmed" with ``trim_frac``, or "median"; Yin et al., "Byzantine-Robust Distributed
Learning"; an argument of its own beside ``aggregate``, which names the clients' weights and stays "mean" - a robust
estimate takes none; the driver's ``--aggregate trimmed | median`` sets it): Delta_i is the coordinate-wise trimmed mean of the clients' ``d_c[i]`` - ``robust_delta`` below states it,
``trim_count`` gives the k clients dropped at each end - and then takes the server step or the split close like every
other Delta.  No clip, no noise, no weight; a cohort of at most 64 clients (``cohort_robust_delta_kernel`` holds a
parameter's clients in the lanes of one wave); "median" with M <= 2 has k == 0 and is the mean.  Every rank trims within
its own cohort: W ranks end on the mean of W robust estimates, not on one estimate over all W * M clients.
``flip_clients`` F > 0 (``data.dataset.flip_client_labels``): the training labels of clients 0..F-1 are mirrored - the
poisoned clients a robust aggregate is there for.

Record-level DP-SGD inside the cohort (``dp_clip`` C > 0, ``dp_noise`` sigma; not with FedProx, fp16 AMP or DDP): local
step s of cohort slot j is ``TorchLocalTrainer``'s DP step - per-sample gradients from ``torch.func``, each clipped in
fp32 to l2 norm C, summed, plus ``sigma * C * z``, divided by B, then the optimizer's update - with ``z =
philox.normal(dp_seed, t0 + s, P, stream=2 + j)``: stream 2 + j keeps the M clients of one step independent (0 is the
single client's DP-SGD, 1 the client-level close), and ``t0`` is ``dp_steps`` at the round's start, which every round
advances by its ``n`` whichever clients run fewer steps (``set_dp_steps`` on resume).  The close is whichever the other
arguments name; ``dp_seed`` has no default (``dp_clip`` > 0 without it is an error); ``dp_row_scale_cohort_kernel`` and ``slab_reduce_cohort_dp_sgd_kernel`` implement the step.
"""
from __future__ import annotations

import copy
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from ..data.dataset import CohortSampler, client_partition, flipped_labels
from ..utils import philox
from .local import add_prox_grad, check_prox
from .server_opt import (BETA1, BETA2, TAU, check_server_opt, check_server_scope, server_opt_init,
                         server_opt_step)


class TorchCohortTrainer:
    def __init__(self, model: torch.nn.Module, x: torch.Tensor, y: torch.Tensor, batch_size: int,
                 steps_per_round: int, clients: int, cohort: Optional[int] = None, lr: float = 1e-2,
                 momentum: float = 0.9, weight_decay: float = 0.0, nesterov: bool = False,
                 amp_dtype: Optional[torch.dtype] = None, seed: Optional[int] = None, dp_clip: float = 0.0,
                 dp_noise: float = 0.0, dp_seed: Optional[int] = None, client_dp_clip: float = 0.0, client_dp_noise: float = 0.0, client_dp_seed: Optional[int] = None,
                 server_lr: float = 1.0, world_size: int = 1, server_opt: str = "none", server_beta1: float = BETA1,
                 server_beta2: float = BETA2, server_tau: float = TAU, server_scope: str = "rank",
                 prox_mu: float = 0.0, partition: str = "contiguous", shards_per_client: int = 2,
                 dirichlet_alpha: float = 0.0, local_epochs: int = 0, aggregate: str = "mean",
                 robust: str = "none", trim_frac: Optional[float] = None, flip_clients: int = 0):
        check_prox(prox_mu, amp_dtype, model)
        check_aggregate(aggregate, local_epochs, nesterov, prox_mu, client_dp_clip)
        check_robust(robust, aggregate, client_dp_clip)
        self.robust = robust
        self.trim = trim_count(robust, clients if not cohort else int(cohort), trim_frac)
        self.prox_mu = float(prox_mu)
        check_cohort_dp(dp_clip, dp_noise, dp_seed, prox_mu, amp_dtype, model)
        self.dp_clip, self.dp_noise = float(dp_clip), float(dp_noise)
        self.dp = self.dp_clip > 0.0
        self.dp_seed = (0 if dp_seed is None else int(dp_seed)) & philox.MASK64  # (None: DP-SGD is off)
        self.dp_steps = 0  # the t of the next cohort step's noise
        check_client_dp(client_dp_clip, client_dp_noise, server_lr, world_size)
        check_server_opt(server_opt, server_beta1, server_beta2, server_tau)
        self.server_scope = check_server_scope(server_scope)
        self.model, self.x, self.y = model, x, y
        self.device = x.device
        self.B, self.S, self.K = int(batch_size), int(steps_per_round), int(clients)
        self.M = self.K if not cohort else int(cohort)
        self.opt_args = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov)
        self.amp_dtype = amp_dtype
        self.partition, self.shards_per_client = partition, int(shards_per_client)
        self.dirichlet_alpha, self.local_epochs, self.aggregate = float(dirichlet_alpha), int(local_epochs), aggregate
        self.momentum = float(momentum)
        self.hetero = partition == "dirichlet" or self.local_epochs > 0 or aggregate != "mean"
        order = client_partition(partition, y, self.K, self.shards_per_client, seed, self.device,
                                 alpha=self.dirichlet_alpha, min_rows=self.B)
        order, sizes = order if isinstance(order, tuple) else (order, None)
        self.flip_clients = int(flip_clients)
        nc = getattr(model, "num_classes", None) or int(y.max()) + 1
        self.y = y = flipped_labels(y, order, sizes, self.K, self.flip_clients, nc)
        self.sampler = CohortSampler(x.shape[0], self.B, self.S, self.K, self.M, self.device, seed=seed, order=order,
                                     sizes=sizes)
        self._shape: Tuple[List[int], List[int], List[float]] = ([], [], [])
        self._loss_client_steps = 0
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
        self.cdp_clip, self.cdp_noise, self.server_lr = float(client_dp_clip), float(client_dp_noise), float(server_lr)
        self.cdp_seed = client_dp_seed_of(seed, client_dp_seed)
        self.cdp_nu = client_dp_nu(self.cdp_noise, self.cdp_clip, self.M, world_size)
        self.server_opt = server_opt
        self.server_beta1, self.server_beta2, self.server_tau = float(server_beta1), float(server_beta2), float(server_tau)
        self.server_m, self.server_v = server_opt_init(server_opt, sum(p.numel() for p in model.parameters()),
                                                       self.server_tau, self.device)
        numel = sum(p.numel() for p in model.parameters())
        self.server_delta = (torch.zeros(numel, dtype=torch.float32, device=self.device)
                             if self.server_scope == "global" else None)
        self.client_dp = (self.cdp_clip > 0.0 or self.server_lr != 1.0 or server_opt != "none"
                          or self.server_delta is not None or self.trim > 0)
        self._norms: List[float] = []
        self._scales: List[float] = []

    def set_cohort_round(self, r: int) -> None:
        self.cohort_round = int(r)

    def set_dp_steps(self, n: int) -> None:
        """Continue the record-level noise at cohort step ``n`` (checkpoint resume)."""
        self.dp_steps = int(n)

    def _dp_step(self, opt, j: int, t: int, xb: torch.Tensor, yb: torch.Tensor, use_amp: bool) -> torch.Tensor:
        """One DP-SGD step of cohort slot j on the work model (the module docstring's definition); the batch's mean
        loss."""
        from torch.func import functional_call, grad, vmap
        names = [n for n, _ in self.work.named_parameters()]
        params = {n: p.detach() for n, p in self.work.named_parameters()}

        def sample_loss(p, x1, y1):
            with torch.autocast(device_type=self.device.type, dtype=self.amp_dtype or torch.float32, enabled=use_amp):
                loss = F.cross_entropy(functional_call(self.work, p, (x1.unsqueeze(0),)), y1.unsqueeze(0))
            return loss, loss.detach()

        grads, losses = vmap(grad(sample_loss, has_aux=True), in_dims=(None, 0, 0))(params, xb, yb)
        B = xb.shape[0]
        g = torch.cat([grads[n].reshape(B, -1).float() for n in names], dim=1)  # [B, P]
        norms = g.norm(dim=1)
        c = torch.where(norms > 0, (self.dp_clip / norms).clamp(max=1.0), torch.ones_like(norms))
        total = (g * c[:, None]).sum(0)
        if self.dp_noise > 0.0:
            z = philox.normal(self.dp_seed, t, g.shape[1], stream=2 + j)
            total = total + (self.dp_noise * self.dp_clip) * torch.from_numpy(z).to(total)
        total = total / B
        off = 0
        for p in self.work.parameters():
            p.grad = total[off:off + p.numel()].view_as(p).to(p.dtype)
            off += p.numel()
        opt.step()
        return losses.float().mean()

    def server_state(self) -> Dict[str, torch.Tensor]:
        """The server optimizer's state (copies on the CPU): ``server_m`` and, for the adaptive rules, ``server_v``."""
        return {k: t.detach().cpu().clone() for k, t in (("server_m", self.server_m), ("server_v", self.server_v))
                if t is not None}

    def load_server_state(self, st: Dict[str, torch.Tensor]) -> None:
        load_server_state(self, st)

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
            if self.dp:
                self.loss_acc += self._dp_step(opt, j, self.dp_steps + s, xb, yb, use_amp)
                continue
            with torch.autocast(device_type=self.device.type, dtype=self.amp_dtype or torch.float32, enabled=use_amp):
                loss = F.cross_entropy(self.work(xb), yb)
            loss.backward()
            if self.prox_mu > 0.0:
                add_prox_grad(self.work.parameters(), self.model.parameters(), self.prox_mu)
            opt.step()
            self.loss_acc += loss.detach().float()
        return [p.detach().clone() for p in self.work.parameters()]

    def round_shape(self, ids: List[int], n: int) -> Tuple[List[int], List[int], List[float]]:
        """(sizes, steps, weights) of the cohort ``ids`` in a round of ``n`` steps: ``n_c``, ``min(n, S_c)`` and
        ``weights_of`` of the two."""
        return cohort_round_shape(self.sampler, ids, n, self.local_epochs, self.aggregate, self.momentum)

    def last_round_shape(self) -> Tuple[List[int], List[int], List[float]]:
        """The last round's cohort: its clients' sizes, local steps and aggregation weights, in cohort order."""
        return self._shape

    def run_table(self, n: int, table: torch.Tensor, r: Optional[int] = None,
                  steps: Optional[List[int]] = None, weights: Optional[List[float]] = None) -> None:
        """One cohort round on ``table`` (int32 ``[>= n, M * B]``): the clients one after another, then the mean (or
        the DP close, which draws the noise of round ``r``; default: the round counter).  ``steps`` [M]: client j runs
        its first ``steps[j]`` table rows (default: n each); ``weights`` [M] (fp32 values): the weighted close."""
        steps = [n] * self.M if steps is None else [min(n, int(v)) for v in steps]
        self._steps = steps
        if self.client_dp or weights is not None:
            self._run_table_client_dp(n, table, self.cohort_round if r is None else r, weights)
        else:
            total = None
            for j in range(self.M):
                ps = self._client_round(j, steps[j], table)
                total = ps if total is None else [t + p for t, p in zip(total, ps)]
            inv = torch.tensor(1.0 / self.M, dtype=torch.float32, device=self.device)  # fp32(1 / M), rounded once
            with torch.no_grad():
                for pg, t in zip(self.model.parameters(), total):
                    pg.copy_(t * inv)
        self.steps_done += n
        if self.dp:
            self.dp_steps += n
        self._loss_steps += n
        self._loss_client_steps += sum(steps)

    def _run_table_client_dp(self, n: int, table: torch.Tensor, r: int, weights: Optional[List[float]] = None) -> None:
        """The DP close of round ``r`` (the module docstring's definition), everything in fp32.  ``weights``: the
        weighted close - ``s_c w_c`` in place of ``s_c`` and no ``1 / M``."""
        f32 = dict(dtype=torch.float32, device=self.device)
        g = torch.cat([p.detach().reshape(-1) for p in self.model.parameters()]).float()
        acc, self._norms, self._scales = None, [], []
        for j in range(self.M):
            pc = torch.cat([p.reshape(-1) for p in self._client_round(j, self._steps[j], table)]).float()
            d = pc - g
            nrm = torch.linalg.vector_norm(d)
            sc = torch.ones((), **f32)
            if self.cdp_clip > 0.0 and float(nrm) > 0.0:
                sc = torch.minimum(sc, torch.tensor(self.cdp_clip, **f32) / nrm)
            self._norms.append(float(nrm))
            self._scales.append(float(sc))
            if weights is not None:
                sc = sc * torch.tensor(weights[j], **f32)
            if self.trim > 0:  # the robust close takes the clients' weights themselves, every one of them
                acc = [] if acc is None else acc
                acc.append(pc)
            else:
                acc = sc * d if acc is None else acc + sc * d
        if self.trim > 0:
            upd = robust_delta(torch.stack(acc), g, self.trim)
        else:
            upd = acc * torch.tensor(1.0 if weights is not None else 1.0 / self.M, **f32)
        if self.cdp_nu != 0.0:
            z = philox.normal(self.cdp_seed, r, g.numel(), stream=1).astype(np.float32)
            upd = upd + torch.tensor(self.cdp_nu, **f32) * torch.from_numpy(z).to(self.device)
        if self.server_delta is not None:  # scope "global": the round ends here; apply_server_step takes the step
            self.server_delta.copy_(upd)
            return
        self._server_step(g, upd)

    def _server_step(self, g: torch.Tensor, upd: torch.Tensor) -> None:
        """The plain server step or the server optimizer's on the delta ``upd``, written into the model."""
        if self.server_opt == "none":
            new = g + torch.tensor(self.server_lr, dtype=torch.float32, device=self.device) * upd
        else:
            new, self.server_m, self.server_v = server_opt_step(
                self.server_opt, g, upd, self.server_m, self.server_v, self.server_lr, self.server_beta1,
                self.server_beta2, self.server_tau)
        off = 0
        with torch.no_grad():
            for pg in self.model.parameters():
                pg.copy_(new[off:off + pg.numel()].view_as(pg))
                off += pg.numel()

    def apply_server_step(self) -> None:
        """Scope "global": one server step on the model from ``server_delta`` - this rank's delta as ``launch_round``
        left it, or the ranks' average once the driver all-reduced it."""
        if self.server_delta is None:
            raise RuntimeError('apply_server_step needs server_scope="global": scope "rank" steps inside the round')
        g = torch.cat([p.detach().reshape(-1) for p in self.model.parameters()]).float()
        self._server_step(g, self.server_delta.clone())

    def last_clip_stats(self) -> Tuple[List[float], float]:
        """(the last round's delta norms in cohort order, the share of its clients that were clipped)."""
        return list(self._norms), sum(s < 1.0 for s in self._scales) / max(1, len(self._scales))

    def run_steps(self, n: int, reset_loss: bool = True) -> None:
        self.prepare_round(n, reset_loss)
        self.launch_round(n)
        if self.server_delta is not None:
            self.apply_server_step()

    run_round = run_steps

    def prepare_round(self, n: int, reset_loss: bool = True) -> None:
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0
            self._loss_client_steps = 0

    def launch_round(self, n: int, next_n=None) -> None:
        self.round_clients = self.sampler.fill(self.cohort_round, self.table)
        self.cohort_round += 1
        self._shape = self.round_shape(self.round_clients, n)
        if self.hetero:
            self.run_table(n, self.table, self.cohort_round - 1, self._shape[1],
                           self._shape[2] if self.aggregate != "mean" else None)
        else:
            self.run_table(n, self.table, self.cohort_round - 1)

    def avg_loss(self) -> float:
        """Mean per-sample loss over the clients' steps since the last reset (``sum_c S_c`` per round)."""
        return float(self.loss_acc.item()) / max(1, self._loss_client_steps)


def load_server_state(trainer, st: Dict[str, torch.Tensor]) -> None:
    """Copy ``server_m`` / ``server_v`` of ``st`` into a cohort trainer's state tensors (those it has)."""
    for key in ("server_m", "server_v"):
        t = getattr(trainer, key, None)
        if t is None or st.get(key) is None:
            continue
        if st[key].shape != t.shape:
            raise ValueError(f"{key} shape {tuple(st[key].shape)} != {tuple(t.shape)}")
        t.copy_(st[key].to(t.device))


AGGREGATES = ("mean", "weighted", "nova")  # the clients' weights in Delta = sum_c w_c d_c (weights_of)
ROBUST_AGGREGATES = ("trimmed", "median")  # the robust estimates: Delta = robust_delta with trim_count's k, no weights
ROBUST_MAX_COHORT = 64  # check_cohort_close's bound: cohort_robust_delta_kernel holds a parameter's clients in one wave


def check_aggregate(aggregate: str, local_epochs: int, nesterov: bool, prox_mu: float, client_dp_clip: float) -> None:
    if aggregate not in AGGREGATES:
        raise ValueError(f"aggregate must be one of {list(AGGREGATES)}, got {aggregate!r}")
    if int(local_epochs) < 0:
        raise ValueError("local_epochs must be >= 0")
    if aggregate != "mean" and client_dp_clip > 0.0:
        raise ValueError(f"aggregate {aggregate!r} is not combined with client-level DP (client_dp_clip > 0): the "
                         "sensitivity of a weighted, clipped mean is not C / M, and no accountant here covers it")
    if aggregate == "nova" and (nesterov or prox_mu > 0.0):
        raise ValueError('aggregate "nova" is not combined with nesterov momentum or FedProx (prox_mu > 0): its '
                         "normaliser a_c is derived for heavy-ball momentum SGD only")


def check_robust(robust: str, aggregate: str, client_dp_clip: float) -> None:
    if robust not in ("none",) + ROBUST_AGGREGATES:
        raise ValueError(f"robust must be one of {['none'] + list(ROBUST_AGGREGATES)}, got {robust!r}")
    if robust == "none":
        return
    if aggregate != "mean":
        raise ValueError(f"robust {robust!r} is not combined with aggregate {aggregate!r}: a trimmed mean takes no "
                         "client weights")
    if client_dp_clip > 0.0:
        raise ValueError(f"robust {robust!r} is not combined with client-level DP (client_dp_clip > 0): the "
                         "sensitivity of a trimmed mean is not C / M, and no accountant here covers it")


def trim_count(aggregate: str, cohort: int, trim_frac: Optional[float] = None) -> int:
    """k, the clients a robust aggregate drops at each end of every parameter's order, for a cohort of M: "trimmed"
    ``floor(trim_frac * M)`` with ``0 < trim_frac < 0.5`` (so 2 k < M), rejected when that is 0; "median"
    ``(M - 1) // 2`` - the middle value for odd M, the mean of the two middle ones for even M, and 0, the plain mean,
    for M <= 2; 0 for "none" and the names of ``AGGREGATES``.  ``trim_frac`` belongs to "trimmed" alone and has no
    default."""
    M = int(cohort)
    if aggregate not in ("none",) + AGGREGATES + ROBUST_AGGREGATES:
        raise ValueError(f"aggregate must be one of {list(AGGREGATES + ROBUST_AGGREGATES)}, got {aggregate!r}")
    if M < 1:
        raise ValueError(f"a cohort has at least one client, got {M}")
    if aggregate != "trimmed" and trim_frac is not None:
        raise ValueError(f'trim_frac is the share aggregate "trimmed" drops at each end: aggregate {aggregate!r} takes '
                         "none")
    if aggregate not in ROBUST_AGGREGATES:
        return 0
    if M > ROBUST_MAX_COHORT:
        raise ValueError(f"aggregate {aggregate!r} needs a cohort of at most {ROBUST_MAX_COHORT} clients, got {M}: the "
                         "selection kernel holds one parameter's clients in the lanes of one wave")
    if aggregate == "median":
        return (M - 1) // 2
    if trim_frac is None:
        raise ValueError('aggregate "trimmed" needs trim_frac, the share of the cohort dropped at each end: there is '
                         "no default")
    f = float(trim_frac)
    if not 0.0 < f < 0.5:
        raise ValueError(f"trim_frac must be in (0, 0.5), got {f:g}")
    k = int(math.floor(f * M))
    if k == 0:
        raise ValueError(f"trim_frac {f:g} of a cohort of {M} drops floor({f:g} * {M}) = 0 clients: that is the plain "
                         'mean - use aggregate "mean", a larger trim_frac or a larger cohort')
    return k


def _order_keys(x: torch.Tensor) -> torch.Tensor:
    """The 32-bit keys (as int64) that order fp32 values as -inf < ... < -0 < +0 < ... < +inf < NaN: a NaN of either
    sign 0xFFFFFFFF, else the bit pattern with the sign bit flipped (non-negative sign) or all bits flipped."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    key = torch.where((b >> 31) != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)
    return torch.where(torch.isnan(x), torch.full_like(key, 0xFFFFFFFF), key)


def robust_delta(stack: torch.Tensor, g: torch.Tensor, k: int) -> torch.Tensor:
    """The coordinate-wise trimmed mean of M clients' round deltas, the definition ``cohort_robust_delta_kernel``
    implements: ``stack`` [M, P] the clients' weights p_c, ``g`` [P] the round's starting weights, ``1 <= k``, ``2 k < M``.

    ``x_c = p_c - g`` in fp32.  The M values of a parameter are ordered by ``_order_keys``, ties by client index:
    ``rank_c = #{j : key_j < key_c, or key_j == key_c and j < c}``, a permutation of 0..M-1.  Client c is kept when
    ``k <= rank_c < M - k``, and ``Delta = (((x_c1 + x_c2) + ...) + x_cn) * fp32(1 / n)`` over the ``n = M - 2 k`` kept
    clients in ascending client order, every sum and the product rounded on its own in fp32.  (The running sum starts
    from -0, for which ``-0 + x`` is x bit for bit.)  Integer keys, ranks, selects and sequential adds: on the CPU this
    yields the kernel's bits.  At most k bad clients (NaN, +-inf) at a parameter are trimmed away; more propagate."""
    M, k = int(stack.shape[0]), int(k)
    if stack.dim() != 2 or g.shape != stack.shape[1:] or not (k >= 1 and 2 * k < M):
        raise ValueError(f"need stack [M, P], g [P] and 1 <= k, 2 k < M; got {tuple(stack.shape)}, {tuple(g.shape)}, k {k}")
    x = stack.float() - g.float()
    key = _order_keys(x)
    c = torch.arange(M, device=x.device)[:, None]
    rank = torch.zeros_like(key)
    for j in range(M):
        rank += ((key[j] < key) | ((key[j] == key) & (j < c))).to(torch.int64)
    kept = (rank >= k) & (rank < M - k)
    s = torch.full_like(x[0], -0.0)
    for j in range(M):
        s = torch.where(kept[j], s + x[j], s)
    one = torch.ones((), dtype=torch.float32, device=x.device)
    return s * (one / (M - 2 * k))


def robust_delta_f64(stack: torch.Tensor, g: torch.Tensor, k: int) -> torch.Tensor:
    """``robust_delta`` in plain float64: the deltas sorted per parameter (NaN largest), k dropped at each end, the mean
    of the rest.  [P] float64."""
    M, k = int(stack.shape[0]), int(k)
    x = torch.sort(stack.double() - g.double(), dim=0).values  # (torch orders NaN above +inf)
    return x[k:M - k].mean(dim=0)


def nova_norm(tau: int, rho: float) -> float:
    """a(tau, rho): the displacement of ``tau`` SGD steps under a constant unit gradient and unit learning rate with
    heavy-ball momentum rho (m_t = rho m_{t-1} + 1, x -= m_t): ``sum_{t=1..tau} (1 - rho^t) / (1 - rho)
    = [tau - rho (1 - rho^tau) / (1 - rho)] / (1 - rho)``; tau at rho == 0.  In double."""
    tau, rho = int(tau), float(rho)
    if rho == 0.0:
        return float(tau)
    return (tau - rho * (1.0 - rho ** tau) / (1.0 - rho)) / (1.0 - rho)


def weights_of(sizes: List[int], steps: List[int], mode: str, momentum: float = 0.0) -> List[float]:
    """The aggregation weights w_c of a cohort whose clients own ``sizes`` n_c rows and run ``steps`` S_c local steps
    (both in cohort order), computed in double and rounded once to fp32 (returned as Python floats that are fp32
    values).  With ``p_c = n_c / sum n_c``: "mean" ``1 / M``; "weighted" ``p_c``; "nova" ``p_c * tau_eff / a_c`` with
    ``a_c = nova_norm(S_c, momentum)`` and ``tau_eff = sum_c p_c a_c`` (FedNova: every client's delta normalised by its
    own amount of local work, the sum rescaled to the cohort's mean amount; equal steps: "weighted")."""
    if mode not in AGGREGATES:
        raise ValueError(f"aggregate must be one of {list(AGGREGATES)}, got {mode!r}")
    M = len(sizes)
    if M < 1 or len(steps) != M or min(sizes) < 1 or min(steps) < 1:
        raise ValueError("need one size >= 1 and one step count >= 1 per client")
    if mode == "mean":
        w = [1.0 / M] * M
    else:
        total = float(sum(sizes))
        w = [n / total for n in sizes]
        if mode == "nova":
            a = [nova_norm(t, momentum) for t in steps]
            tau_eff = sum(p * ac for p, ac in zip(w, a))
            w = [p * tau_eff / ac for p, ac in zip(w, a)]
    return [float(np.float32(v)) for v in w]


def cohort_round_shape(sampler, ids: List[int], n: int, local_epochs: int, aggregate: str,
                       momentum: float) -> Tuple[List[int], List[int], List[float]]:
    """(sizes, steps, weights) of the cohort ``ids`` in a round of ``n`` <= S steps: ``sampler.sizes_of``,
    ``min(n, sampler.steps_of)`` and ``weights_of`` of the two - what both cohort trainers run a round with."""
    sizes = sampler.sizes_of(ids)
    steps = [min(int(n), s) for s in sampler.steps_of(ids, local_epochs)]
    return sizes, steps, weights_of(sizes, steps, aggregate, momentum)


def check_client_dp(clip: float, noise: float, server_lr: float, world_size: int) -> None:
    if clip < 0 or noise < 0:
        raise ValueError("client_dp_clip and client_dp_noise must be >= 0")
    if noise > 0 and clip == 0:
        raise ValueError("client_dp_noise needs client_dp_clip > 0: the noise is scaled by the clip norm")
    if not server_lr > 0:
        raise ValueError("server_lr must be > 0")
    if world_size < 1:
        raise ValueError("world_size must be >= 1")


def check_cohort_dp(dp_clip: float, dp_noise: float, dp_seed: Optional[int], prox_mu: float = 0.0, amp_dtype=None,
                    model=None) -> None:
    """Record-level DP-SGD inside a cohort: the single client's rules (``TorchLocalTrainer``), and the noise key has
    no default - ``dp_clip`` > 0 without ``dp_seed`` stays the error it was before the cohort trainers took DP-SGD."""
    if not dp_clip >= 0.0 or not dp_noise >= 0.0:
        raise ValueError(f"dp_clip and dp_noise must be >= 0, got {dp_clip} and {dp_noise}")
    if dp_noise > 0.0 and dp_clip == 0.0:
        raise ValueError("dp_noise > 0 needs a clip norm (dp_clip > 0): the noise is scaled by it")
    if dp_clip == 0.0:
        return
    if prox_mu > 0.0:
        raise ValueError("FedProx (prox_mu > 0) is not combined with DP-SGD (dp_clip > 0): the DP reduce has no "
                         "proximal form")
    if amp_dtype == torch.float16:
        raise ValueError("DP-SGD does not support fp16 AMP (a GradScaler would rescale the clipped gradients)")
    if isinstance(model, torch.nn.parallel.DistributedDataParallel):
        raise ValueError("DP-SGD does not support a DistributedDataParallel model (--sync ddp)")
    if dp_seed is None:
        raise ValueError("DP-SGD (dp_clip > 0) in a cohort of virtual clients needs dp_seed, the 64-bit key of its "
                         "noise: it is not derived from the trainer's seed, which orders the batches, may be None and "
                         "already keys the client-level close")


def client_dp_seed_of(seed: Optional[int], client_dp_seed: Optional[int]) -> int:
    """The 64-bit Philox key of the client-level noise: ``client_dp_seed``, by default a mix of the trainer's seed."""
    return (philox.mix64(0 if seed is None else seed) if client_dp_seed is None else int(client_dp_seed)) & philox.MASK64


def client_dp_sigma_share(noise: float, world_size: int) -> float:
    """sigma / sqrt(W): the noise multiplier of one rank's share (what the native round takes as ``cdp_sigma``)."""
    return float(noise) / math.sqrt(world_size)


def client_dp_nu(noise: float, clip: float, cohort: int, world_size: int) -> float:
    """nu = sigma * C / (M * sqrt(W)): the standard deviation of the noise a rank adds per parameter."""
    return float(np.float32(client_dp_sigma_share(noise, world_size) * float(clip) / cohort))
