"""Cohorts of virtual FedAvg clients on one GPU (Python side of the cohort entries of csrc/kernels/tiny_ecg_step.hip
and, for the close of a round, csrc/kernels/tiny_ecg_close.hip).

The fused step kernel runs one workgroup per window, so a client with a small batch leaves most of the GPU idle.
``FusedCohortTrainer`` holds ``clients`` virtual clients (contiguous partitions of its windows) and trains a
``cohort`` of them per round side by side: a fan-out of the global weights, then per step ONE step launch over the
cohort's ``cohort * B`` windows and ONE reduce + SGD launch over its clients, then the clients' mean in ascending
cohort order into the global weights - captured into one hipGraph like a single client's round.  Virtual clients keep
no state between rounds (weights from the global model, zero momentum), and which clients and rows a round uses is a
pure function of ``(seed, round)`` (``data.dataset.CohortSampler``).

Record-level DP-SGD (``dp_clip`` C > 0, ``dp_noise`` sigma; not with FedProx): every client's every local step clips
its B per-sample gradients to l2 norm C and adds noise of standard deviation ``sigma * C / B`` per parameter - per step
``dp_row_scale_cohort_kernel`` over the cohort's ``M * B`` slab rows and ``slab_reduce_cohort_dp_sgd_kernel`` (its
STEPS form with unequal local work) in place of the plain cohort reduce, whichever close the round has.  Cohort slot c
draws ``philox.normal(dp_seed, t, P, stream=2 + c)`` (``dp_seed`` has no default: ``dp_clip`` > 0 without it is an error), t the 64-bit step word this trainer owns on the device
(``dp_step``; host mirror ``dp_steps``, ``set_dp_steps`` on resume), advanced once per cohort step whichever clients
are frozen (``train/cohort.py`` states the definition).

Client-level DP (``client_dp_clip`` > 0; DP-FedAvg) and a server step size ``server_lr`` != 1 close the round with
``cohort_delta_scale_kernel`` + ``cohort_dp_mean_kernel`` in place of the mean: every client's round delta clipped to
l2 norm C, averaged, Gaussian noise of standard deviation ``sigma * C / (M * sqrt(world_size))`` per parameter added,
the result applied with step size ``server_lr`` (``train/cohort.py`` states the definition).  The noise is a function
of ``(client_dp_seed, round, parameter index)``; the round counter the kernels read is a device word this trainer owns.

A server optimizer (``server_opt`` sgdm / adagrad / adam / yogi; ``train/server_opt.py`` states the rules) puts
``cohort_server_opt_kernel`` in place of ``cohort_dp_mean_kernel``: the same averaged, clipped, noised delta, then the
optimizer's update of its state ``server_m`` / ``server_v`` ([P] fp32 device tensors this trainer owns, kept across
rounds, rolled back by ``prepare``, saved and restored with ``server_state`` / ``load_server_state``) and its step.

``server_scope="global"`` splits that close where the delta exists, for drivers of several ranks that want ONE server
optimizer over all their clients: the round graph ends with ``cohort_delta_scale_kernel`` + ``cohort_delta_kernel``,
which leave this rank's averaged, clipped, noised delta in ``server_delta`` ([P] fp32) and the global weights, m and v
untouched; the driver all-reduces ``server_delta`` and ``apply_server_step`` (``server_step_kernel``) then takes the
step - the plain one for ``server_opt="none"`` - on every rank alike.  On one rank the two halves leave the bits of the
default ``server_scope="rank"``.

FedProx (``prox_mu`` > 0): every client's local steps add ``prox_mu * (w - g)`` to the gradient, g the global weights the
round started from (``slab_reduce_cohort_prox_sgd_kernel``).  The anchor is the global weight buffer itself: the fan-out
leaves g there and no launch writes it before the close, so the round needs no copy and no further buffer.

``partition="shards"`` deals the clients label-skewed partitions (``data.dataset.shard_partition``: ``shards_per_client``
runs of the label-sorted windows each) instead of contiguous slices of the windows.

Unequal clients: ``partition="dirichlet"`` (``data.dataset.dirichlet_partition`` with ``dirichlet_alpha``: clients of
unequal sizes n_k and label mixes), ``local_epochs`` E > 0 (client c runs ``S_c = min(S, max(1, E * (n_c // B)))`` of the
round's S steps and is frozen for the rest: the STEPS form of the cohort reduce, ``slab_reduce_cohort_steps_*``) and
``aggregate`` "weighted" (n_c / n, FedAvg's own weights) or "nova" (FedNova) in place of "mean": the close is then
``cohort_delta_wscale_kernel`` + the second kernel of whichever close the round has, on the weights of
``train.cohort.weights_of``.  Step counts and weights change with every round's cohort, so they live in device arrays
the kernels read - one pair per index table, filled by ``stage()`` beside it - and one captured graph serves every
round.  A weighted close takes no clip and no noise.

Robust aggregates: ``robust`` "trimmed" (with ``trim_frac``) or "median" (beside ``aggregate``, which stays "mean") close the round with the coordinate-wise
trimmed mean of the clients' deltas (``train.cohort.robust_delta`` states it, ``train.cohort.trim_count`` the k dropped at
each end): ``cohort_delta_scale_kernel`` without a clip, ``cohort_robust_delta_kernel`` into ``server_delta`` (scope
"global") or into a [P] scratch tensor this trainer owns, and from there ``server_step_kernel`` - the plain step or the
server optimizer's.  k is a scalar in the round's description, baked into its graphs.  No clip, noise or weights; a cohort
of at most 64; a robust aggregate alone leaves the reduce in its plain form (``client_steps`` stays null).
``flip_clients`` F > 0 mirrors the training labels of clients 0..F-1 (``data.dataset.flip_client_labels``).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ..data.dataset import CohortSampler, client_partition, flipped_labels
from ..models.tiny_ecg import TinyECG, num_params
from .fused_tiny import _check_dataset, labels_int32, prec_id, slab_stride
from .tiny_eval import EvalResult, TinyEvaluator, tiny_evaluate
from ..train.cohort import (check_aggregate, check_client_dp, check_cohort_dp, check_robust, client_dp_seed_of,
                            client_dp_sigma_share, cohort_round_shape, load_server_state, trim_count)
from ..train.server_opt import BETA1, BETA2, TAU, check_server_opt, check_server_scope, server_opt_init


class FusedCohortTrainer:
    """``cohort`` of ``clients`` virtual clients per round on the fused HIP step; the trainer interface of
    ``FusedTinyTrainer``.  ``params`` is the model's flat buffer: the global weights that FedAvg all-reduces."""

    def __init__(self, model: TinyECG, x_gpu: torch.Tensor, y_gpu: torch.Tensor, batch_size: int,
                 steps_per_round: int, clients: int, cohort: Optional[int] = None, lr: float = 1e-2,
                 momentum: float = 0.9, weight_decay: float = 0.0, nesterov: bool = False, seed: Optional[int] = None,
                 use_graph: Optional[bool] = None, precision: str = "bf16", dp_clip: float = 0.0,
                 dp_noise: float = 0.0, dp_seed: Optional[int] = None, client_dp_clip: float = 0.0, client_dp_noise: float = 0.0, client_dp_seed: Optional[int] = None,
                 server_lr: float = 1.0, world_size: int = 1, server_opt: str = "none", server_beta1: float = BETA1,
                 server_beta2: float = BETA2, server_tau: float = TAU, server_scope: str = "rank",
                 prox_mu: float = 0.0, partition: str = "contiguous", shards_per_client: int = 2,
                 dirichlet_alpha: float = 0.0, local_epochs: int = 0, aggregate: str = "mean",
                 robust: str = "none", trim_frac: Optional[float] = None, flip_clients: int = 0):
        if not prox_mu >= 0.0:
            raise ValueError(f"prox_mu must be >= 0, got {prox_mu}")
        check_aggregate(aggregate, local_epochs, nesterov, prox_mu, client_dp_clip)
        check_robust(robust, aggregate, client_dp_clip)
        self.robust = robust
        self.trim = trim_count(robust, clients if not cohort else int(cohort), trim_frac)  # 0: not a robust close
        check_cohort_dp(dp_clip, dp_noise, dp_seed, prox_mu)  # (fp16 is no precision of the fused kernels: prec_id)
        check_client_dp(client_dp_clip, client_dp_noise, server_lr, world_size)
        self.server_opt_id = check_server_opt(server_opt, server_beta1, server_beta2, server_tau)
        self.server_scope = check_server_scope(server_scope)
        self.device = x_gpu.device
        self.precision = precision
        self.prec = prec_id(precision)
        self.model = model
        self.nc = model.num_classes
        self.params = model.flat if model.flat is not None else model.flatten_parameters()
        if self.params.device != self.device:
            raise ValueError("model and dataset must be on the same device")
        self.P = num_params(self.nc)
        self.x = x_gpu.contiguous()
        self.B, self.S = int(batch_size), int(steps_per_round)
        self.K = int(clients)
        self.M = self.K if not cohort else int(cohort)
        self.lr, self.momentum, self.wd, self.nesterov = float(lr), float(momentum), float(weight_decay), bool(nesterov)
        self.partition, self.shards_per_client = partition, int(shards_per_client)
        self.dirichlet_alpha, self.local_epochs, self.aggregate = float(dirichlet_alpha), int(local_epochs), aggregate
        self.hetero = partition == "dirichlet" or self.local_epochs > 0 or aggregate != "mean"
        order = client_partition(partition, y_gpu, self.K, self.shards_per_client, seed, self.device,
                                 alpha=self.dirichlet_alpha, min_rows=self.B)
        order, sizes = order if isinstance(order, tuple) else (order, None)
        self.flip_clients = int(flip_clients)
        self.y32 = labels_int32(flipped_labels(y_gpu, order, sizes, self.K, self.flip_clients, self.nc), self.nc)
        _check_dataset(self.x, self.y32, self.nc)
        self.sampler = CohortSampler(self.x.shape[0], self.B, self.S, self.K, self.M, self.device, seed=seed,
                                     order=order, sizes=sizes)
        self.prox_mu = float(prox_mu)
        lib = _lib.kernels()
        L = self.x.shape[1]
        if lib.ecg_tiny_smem_bytes(L, self.prec) > 160 * 1024:
            raise ValueError(f"window length {L} too long for the fused kernel")
        rows = self.M * self.B
        self.stride = slab_stride(self.nc)
        self.pstride = lib.ecg_tiny_cohort_param_stride(self.nc)
        self.wstride = lib.ecg_tiny_cohort_wprep_stride()
        f32 = dict(dtype=torch.float32, device=self.device)
        # per-client scratch of a round: weights, momenta, images (zero-initialised: the K-padding slots of an image
        # are never written by the SGD epilogue), gradient rows, loss words
        self.cparams = torch.zeros(self.M * self.pstride, **f32)
        self.cmom = torch.zeros(self.M * self.pstride, **f32)
        self.slab = torch.empty((rows, self.stride), **f32)
        self.loss_acc = torch.zeros(self.M, **f32)
        self.wprep = self.xg = self.yg = self.xbg = None
        if precision == "bf16":
            self.wprep = torch.zeros(self.M * self.wstride, dtype=torch.uint8, device=self.device)
            self.xg = torch.zeros(lib.ecg_tiny_gather_floats(L, rows), **f32)
            self.yg = torch.zeros(2 * rows, dtype=torch.int32, device=self.device)
            self.xbg = torch.zeros(lib.ecg_tiny_gather_halfs(L, rows), dtype=torch.bfloat16, device=self.device)
        self.idx_table = torch.zeros((self.S, rows), dtype=torch.int32, device=self.device)
        self.idx_stage = torch.zeros((self.S, rows), dtype=torch.int32, device=self.device)
        self._staged: Optional[int] = None
        self._staged_clients: List[int] = []
        self.round_clients: List[int] = []  # the cohort of the last round taken
        self.cohort_round = 0  # rounds taken so far = the round the next staging draws
        self._loss_steps = 0
        self._loss_samples = 0  # B * sum_c S_c of the rounds since the loss words were reset
        self.steps_done = 0
        # unequal clients: one (step counts, weights) pair per index table - stage() fills the pair of idx_stage while
        # the round before may still read the other - holding values every graph can run on until then
        self._pairs: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._shape: Tuple[List[int], List[int], List[float]] = ([], [], [])
        self._staged_shape = self._shape
        if self.hetero:
            for t in (self.idx_table, self.idx_stage):
                self._pairs[t.data_ptr()] = (torch.full((self.M,), self.S, dtype=torch.int32, device=self.device),
                                             torch.full((self.M,), 1.0 / self.M, **f32))
        self.use_graph = (os.environ.get("ECG_TINY_GRAPH", "1") != "0") if use_graph is None else bool(use_graph)
        self._graphs = {}
        self._evaluator: Optional[TinyEvaluator] = None
        # client-level DP / server step size: the clip factors and delta norms of the last round and the round counter
        # the close draws its noise from (a device word: kernel arguments are baked into a captured graph)
        self.cdp_clip, self.cdp_noise, self.server_lr = float(client_dp_clip), float(client_dp_noise), float(server_lr)
        self.cdp_seed = client_dp_seed_of(seed, client_dp_seed)
        self.server_opt = server_opt
        self.server_beta1, self.server_beta2, self.server_tau = float(server_beta1), float(server_beta2), float(server_tau)
        self.server_m, self.server_v = server_opt_init(server_opt, self.P, self.server_tau, self.device)
        # scope "global": the round ends with this rank's delta in server_delta (written in place: graphs hold its
        # address) and always takes the two-launch close, so the factor, norm and round-word buffers always exist
        split = self.server_scope == "global"
        self.server_delta = torch.zeros(self.P, **f32) if split else None
        self.client_dp = (self.cdp_clip > 0.0 or self.server_lr != 1.0 or server_opt != "none" or split
                          or aggregate != "mean" or self.trim > 0)
        # a robust close that is not split: Delta passes through this buffer on its way to server_step_kernel
        self.robust_scratch = torch.zeros(self.P, **f32) if (self.trim > 0 and not split) else None
        self.cdp_scale = self.cdp_norm = self.cdp_round = None
        if self.client_dp:
            self.cdp_scale = torch.ones(self.M, **f32)
            self.cdp_norm = torch.zeros(self.M, **f32)
            self.cdp_round = torch.zeros(1, dtype=torch.int64, device=self.device)
        # record-level DP-SGD: the cohort's clip factors (scratch) and the step word every step's noise is drawn from
        self.dp_clip, self.dp_noise = float(dp_clip), float(dp_noise)
        self.dp = self.dp_clip > 0.0
        self.dp_seed = (0 if dp_seed is None else int(dp_seed)) & (2 ** 64 - 1)  # (None: DP-SGD is off)
        self.dp_steps = 0  # host mirror of dp_step: the t of the next cohort step's noise
        self.dp_scale = self.dp_step = None
        if self.dp:
            self.dp_scale = torch.zeros(rows, **f32)
            self.dp_step = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._round = _lib.TinyCohortRound(
            X=self.x.data_ptr(), ldx=self.x.stride(0), Y=self.y32.data_ptr(), params=self.cparams.data_ptr(),
            mom=self.cmom.data_ptr(), slab=self.slab.data_ptr(), loss_acc=self.loss_acc.data_ptr(),
            wprep=_lib.ptr(self.wprep), xg=_lib.ptr(self.xg), yg=_lib.ptr(self.yg), xbg=_lib.ptr(self.xbg),
            global_params=self.params.data_ptr(), L=L, nc=self.nc, slab_stride=self.stride, B=self.B, M=self.M,
            fanout=1, lr=self.lr, momentum=self.momentum, wd=self.wd, nesterov=int(self.nesterov), prec=self.prec,
            prox_mu=self.prox_mu)
        if self.dp:  # (all-zero fields otherwise, here and below: the launches the round always issued)
            r = self._round
            r.dp_clip, r.dp_sigma, r.dp_seed = self.dp_clip, self.dp_noise, self.dp_seed
            r.dp_scale, r.dp_step = self.dp_scale.data_ptr(), self.dp_step.data_ptr()
        if self.client_dp:
            r = self._round
            r.cdp_clip, r.cdp_sigma = self.cdp_clip, client_dp_sigma_share(self.cdp_noise, world_size)
            r.server_lr, r.cdp_seed = self.server_lr, self.cdp_seed
            r.cdp_scale, r.cdp_norm, r.cdp_round = (t.data_ptr() for t in (self.cdp_scale, self.cdp_norm, self.cdp_round))
        if self.trim > 0:
            self._round.robust_trim, self._round.robust_scratch = self.trim, _lib.ptr(self.robust_scratch)
        if split:  # (the struct's server_opt stays 0: apply_server_step takes the step, outside the round)
            self._round.server_delta = self.server_delta.data_ptr()
        elif self.server_opt_id:
            r = self._round
            r.server_opt, r.server_beta1, r.server_beta2 = self.server_opt_id, self.server_beta1, self.server_beta2
            r.server_tau, r.server_m, r.server_v = self.server_tau, _lib.ptr(self.server_m), _lib.ptr(self.server_v)

    # ------------------------------------------------------------------ graph management
    def _round_of(self, n: int, table: torch.Tensor):
        r = self._round
        r.idx, r.steps = table.data_ptr(), n
        if self.hetero:  # the table's own pair; the weights only where the close is a weighted one
            st, w = self._pairs[table.data_ptr()]
            r.client_steps = st.data_ptr()
            r.client_weight = w.data_ptr() if self.aggregate != "mean" else None
        return C.byref(r)

    def _graph_for(self, n: int, table: torch.Tensor) -> C.c_void_p:
        key = (n, table.data_ptr())
        g = self._graphs.get(key)
        if g is None:
            g = C.c_void_p()
            torch.cuda.synchronize(self.device)
            _lib.check(_lib.kernels().ecg_tiny_cohort_round_capture(C.byref(g), self._round_of(n, table)),
                       "ecg_tiny_cohort_round_capture")
            self._graphs[key] = g
        return g

    def close(self):
        graphs, self._graphs = getattr(self, "_graphs", {}), {}
        for g in graphs.values():
            if g.value:
                _lib.kernels().ecg_round_graph_destroy(g)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ execution
    def prepare(self, sizes) -> None:
        """Capture, upload and warm every round graph whose step count is in ``sizes`` (on both index tables).  The
        warm-up replays are rolled back: global weights, loss words, tables and the round counter - the device word of
        the DP close, the DP-SGD step word and the server optimizer's m / v with it - stay as found (the per-client buffers are scratch that
        every round's fan-out rewrites; so is ``server_delta`` of scope "global", whose graphs write neither the
        weights nor m / v: no step has to be replayed or undone)."""
        if not self.use_graph:
            return
        lib = _lib.kernels()
        sizes = [self._check_n(n) for n in sizes]
        state = (self.params, self.loss_acc, self.idx_stage, self.idx_table)
        state += tuple(t for pair in self._pairs.values() for t in pair)
        if self.client_dp:
            state += (self.cdp_round, self.cdp_scale, self.cdp_norm)
        state += tuple(t for t in (self.server_m, self.server_v, self.dp_step) if t is not None)
        snap = [t.clone() for t in state]
        stream = _lib.stream_ptr(self.device)
        for n in sizes:
            for table in (self.idx_stage, self.idx_table):
                g = self._graph_for(n, table)
                _lib.check(lib.ecg_round_graph_upload(g, stream), "ecg_round_graph_upload")
                _lib.check(lib.ecg_round_graph_launch(g, stream), "ecg_round_graph_launch")
        for t, v in zip(state, snap):
            t.copy_(v)
        torch.cuda.synchronize(self.device)

    def _check_n(self, n_steps: Optional[int]) -> int:
        n = self.S if n_steps is None else int(n_steps)
        if not 0 < n <= self.S:
            raise ValueError(f"n_steps must be in [1, {self.S}]")
        return n

    def set_cohort_round(self, r: int) -> None:
        """Continue at round ``r`` (checkpoint resume): the next staging draws that round's cohort, and the DP close
        that round's noise."""
        if self._staged is not None:
            raise RuntimeError("a round is staged: set the round counter before staging")
        self.cohort_round = int(r)
        if self.cdp_round is not None:
            self.cdp_round.fill_(int(r))

    def set_dp_steps(self, n: int) -> None:
        """Continue the record-level noise at cohort step ``n`` (checkpoint resume)."""
        self.dp_steps = int(n)
        if self.dp_step is not None:
            self.dp_step.fill_(int(n))

    def server_state(self) -> Dict[str, torch.Tensor]:
        """The server optimizer's state (copies on the CPU): ``server_m`` and, for the adaptive rules, ``server_v``;
        synchronises."""
        return {k: t.detach().cpu().clone() for k, t in (("server_m", self.server_m), ("server_v", self.server_v))
                if t is not None}

    def load_server_state(self, st: Dict[str, torch.Tensor]) -> None:
        """Continue the server optimizer from ``st`` (``server_state``'s keys; checkpoint resume).  The state tensors
        are written in place: captured graphs hold their addresses."""
        load_server_state(self, st)

    def last_clip_stats(self) -> Tuple[List[float], float]:
        """(the last round's delta norms in cohort order, the share of its clients that were clipped); synchronises."""
        if not self.client_dp:
            return [], 0.0
        return self.cdp_norm.tolist(), float((self.cdp_scale < 1.0).float().mean().item())

    def stage(self, n_steps: Optional[int] = None) -> None:
        """Draw the next round's cohort and batches into the staging table (a round of ``n_steps`` < S steps reads
        the first ``n_steps`` rows of the table the sampler draws for a full round)."""
        n = self._check_n(n_steps)
        self._staged_clients = self.sampler.fill(self.cohort_round, self.idx_stage)
        self._staged_shape = cohort_round_shape(self.sampler, self._staged_clients, n, self.local_epochs,
                                                self.aggregate, self.momentum)
        if self.hetero:  # 1 <= steps <= n: the native round cannot check device values
            st, w = self._pairs[self.idx_stage.data_ptr()]
            st.copy_(torch.tensor(self._staged_shape[1], dtype=torch.int32), non_blocking=True)
            w.copy_(torch.tensor(self._staged_shape[2], dtype=torch.float32), non_blocking=True)
        self._staged = n

    def prepare_round(self, n_steps: Optional[int] = None, reset_loss: bool = True) -> None:
        n = self._check_n(n_steps)
        if reset_loss:
            self.loss_acc.zero_()
            self._loss_steps = 0
            self._loss_samples = 0
        if self._staged != n:
            if self._staged is not None:
                raise RuntimeError(f"{self._staged} rows are staged for the next round, not {n}")
            self.stage(n)

    def take_staged(self, n_steps: Optional[int] = None) -> torch.Tensor:
        n = self._check_n(n_steps)
        if self._staged != n:
            raise RuntimeError("launch_round without prepare_round: no batches staged for this round")
        self._staged = None
        self.idx_table, self.idx_stage = self.idx_stage, self.idx_table
        self.round_clients = self._staged_clients
        self._shape = self._staged_shape
        self.cohort_round += 1
        self.steps_done += n
        if self.dp:
            self.dp_steps += n
        self._loss_steps += n
        self._loss_samples += self.B * (sum(self._shape[1]) if self.hetero else self.M * n)
        return self.idx_table

    def run_round(self, n_steps: Optional[int] = None, reset_loss: bool = True, next_n: Optional[int] = None) -> None:
        self.prepare_round(n_steps, reset_loss)
        self.launch_round(n_steps, next_n)
        if self.server_delta is not None:
            self.apply_server_step()

    def apply_server_step(self) -> None:
        """Scope "global": one server step on the global weights from ``server_delta`` - this rank's delta as
        ``launch_round`` left it, or the ranks' average once the driver all-reduced it - with the trainer's optimizer
        and constants (``server_opt="none"``: the plain step with ``server_lr``), enqueued on the current stream."""
        if self.server_delta is None:
            raise RuntimeError('apply_server_step needs server_scope="global": scope "rank" steps inside the round')
        _lib.check(_lib.kernels().ecg_server_opt_step(
            self.params.data_ptr(), self.server_delta.data_ptr(), self.P, self.server_opt_id, self.server_lr,
            self.server_beta1, self.server_beta2, self.server_tau, _lib.ptr(self.server_m), _lib.ptr(self.server_v),
            _lib.stream_ptr(self.device)), "ecg_server_opt_step")

    def launch_round(self, n_steps: Optional[int] = None, next_n: Optional[int] = None) -> None:
        """Enqueue the staged round.  Scope "global": it ends with this rank's delta in ``server_delta`` and the global
        weights as they were; ``apply_server_step`` completes it."""
        n = self._check_n(n_steps)
        table = self.take_staged(n)
        stream = _lib.stream_ptr(self.device)
        if self.use_graph:
            _lib.check(_lib.kernels().ecg_round_graph_launch(self._graph_for(n, table), stream),
                       "ecg_round_graph_launch")
        else:
            _lib.check(_lib.kernels().ecg_tiny_cohort_round_enqueue(self._round_of(n, table), stream),
                       "ecg_tiny_cohort_round_enqueue")
        if next_n is not None:
            self.stage(next_n)

    def evaluate(self, x: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None) -> EvalResult:
        """Loss / accuracy / confusion matrix of the GLOBAL weights (``FusedTinyTrainer.evaluate``'s contract: reads
        the weights only, leaves the training state as it was)."""
        if (x is None) != (y is None):
            raise ValueError("evaluate takes both windows and labels, or neither")
        if x is None:
            x, y32 = self.x, self.y32
        else:
            y32 = y if y.dtype == torch.int32 else labels_int32(y, self.nc)
        if self.precision != "bf16":
            return tiny_evaluate(self.params, x, y32, None, self.nc, self.precision)
        if self._evaluator is None:
            self._evaluator = TinyEvaluator(self.device, self.nc)
        return self._evaluator.run(self.params, x, y32)

    def avg_loss(self) -> float:
        """Mean per-sample loss over the cohort's clients and the steps they ran since the last reset - ``B * sum_c
        S_c`` samples per round (synchronises)."""
        return float(self.loss_acc.sum().item()) / max(1, self._loss_samples)

    def last_round_shape(self) -> Tuple[List[int], List[int], List[float]]:
        """The last round's cohort: its clients' sizes, local steps and aggregation weights, in cohort order."""
        return self._shape
