"""Federated averaging driver: one FL client per GPU (or per CPU process under gloo).

Reference: TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py:137-239 (``main``).  Per configuration (G0 fp32,
G1 AMP) a fresh TinyECG + SGD(lr 1e-2, momentum 0.9); per round: broadcast the global model, run
``local_steps`` local SGD steps on this client's GPU-resident shard, average the weights over clients.
Every round emits a ``RoundStats`` row with the reference's columns (``samples_per_s = n / local_ms``,
excluding comm) and MI355X columns (``comm_exposed_ms``, ``round_wall_ms``); rank 0 appends all rows to
the results CSV and prints node-aggregate samples/s (sum over clients, wall time including comm).

MI355X execution (vs the reference's host-staged per-tensor MPI calls and per-step sync):
  * G1 local round = ONE native hipGraph replay of ``local_steps`` fused HIP steps (``ops.fused_tiny``);
  * FedAvg = ONE RCCL ``all_reduce(AVG)`` of the flat fp32 weight buffer; broadcast = ONE RCCL broadcast;
  * collectives run from a dedicated comm stream with hipEvents on both streams (``parallel.overlap``), so each
    row's ``comm_ms`` is the collectives' own span and ``comm_exposed_ms`` the MEASURED compute-stream stall;
  * ``--overlap tail`` (exact FedAvg): TinyECG / eager clients issue the all-reduce asynchronously and prepare
    the next round's batches before the compute stream waits; the ResNet engine applies the last step's SGD per
    backward segment and all-reduces each segment while earlier segments still run backward;
  * ``--overlap delayed``: the all-reduce runs under the next round's local steps (stale-by-one FedAvg);
  * ResNet1D G1 runs on the native step engine (``train.resnet_trainer``; one hipGraph replay per step);
  * ``--sync none``: pseudo-federated independent clients; ``--sync ddp``: synchronous gradient DP;
  * ``--drop-prob``: client dropout with sample-weighted averaging; ``--ckpt-every``/``--resume``;
  * ``--eval-every R`` / ``--eval-windows H``: after every R-th round each client evaluates the weights a checkpoint
    of that round would hold (the averaged model; ``--sync none``: its own) on its last H windows, which are held
    out of training (H = 0: on its training windows) - the fused backend on the HIP evaluation kernel
    (``trainer.evaluate``), every other backend with ``ops.tiny_eval.evaluate_torch``.  The clients' records are
    summed with one all-reduce and rank 0 appends a row to ``--eval-csv``.  An evaluated round drains its FedAvg
    all-reduce first, i.e. gives up that round's ``--overlap tail`` overlap (``delayed``: evaluates avg_r in place
    and keeps the stale correction pending, as a checkpoint does).  Evaluation is timed on its own (``eval_ms``),
    outside ``local_train_ms`` / ``comm_ms`` / ``round_wall_ms``; the round rows do not change.
  * ``--dp-clip C`` / ``--dp-noise sigma`` / ``--dp-delta delta``: DP-SGD local steps (per-sample clip to l2 norm C,
    Gaussian noise sigma * C on the clipped sum) for TinyECG on the fused and torch backends; every client's DP seed
    is a 64-bit mix of ``seed + 7919 * rank``.  Each round every client logs its cumulative epsilon
    (``utils.privacy``: the Poisson-subsampling bound at ``sample_rate = batch / training windows``, an approximation
    for the epoch-permutation sampler used here) and rank 0 appends the rows to ``--privacy-csv``.  The training loss in
    the round rows is computed from unclipped, un-noised per-sample losses: it is not private.
  * ``--clients-per-gpu K`` / ``--cohort M``: client sampling.  Every GPU holds K virtual clients (contiguous
    partitions of its training windows, after the evaluation hold-out); each round M of them (default K) are drawn as a
    function of (seed + 7919 * rank, round), train from the global weights with zero momentum on batches of
    ``--batch-size`` windows, and their mean is what the GPU contributes to FedAvg.  The fused backend trains the
    whole cohort in one step launch and one reduce launch per step (``ops.fused_cohort``); ``train.cohort`` is the
    eager reference.  ``samples_per_s`` counts all M * B * S windows of a round; ``batch_size`` in the round rows stays
    the per-client B; rank 0 appends the cohort's shape per round to ``--cohort-csv``.  TinyECG only; not combined
    with ``--sync ddp``, ``--drop-prob`` (client sampling replaces it) or ``--overlap delayed``.
    With ``--dp-clip`` every virtual client's local steps are DP-SGD steps (record-level DP inside the cohort, whichever
    close the round has; it needs ``--dp-noise`` > 0, and is not combined with ``--prox-mu``, fp16 AMP or ``--sync ddp``): cohort slot c draws its noise from Philox
    stream 2 + c of the rank's key (the 64-bit mix of ``seed + 7919 * rank``) and the cohort step counter.  A record of
    virtual client k is touched only in the rounds that draw k, at sample rate ``B / n_k``: the driver counts the local
    steps each of the K clients has run (recounted from the sampler on ``--resume``) and reports per round the largest
    ``epsilon(sigma, B / n_k, steps_k, delta)`` over the rank's clients in the columns of ``--privacy-csv`` (steps and
    sample rate of that client).  This ignores the amplification by client sampling, which is conservative, and is the
    same Poisson approximation as for DP-SGD above.
  * ``--client-dp-clip C`` / ``--client-dp-noise sigma`` / ``--client-dp-delta delta`` / ``--server-lr eta``: client-level
    DP on a cohort round (DP-FedAvg; needs ``--clients-per-gpu``).  Every rank clips each of its M clients' round
    deltas to l2 norm C, averages them, adds N(0, (sigma C / (M sqrt(W)))^2) per parameter and applies the result to the
    global weights with step size eta; the unchanged all-reduce(AVG) of the W ranks' weights then holds the clipped mean
    over all W * M clients plus noise of standard deviation sigma C / (M W): noise multiplier sigma at sensitivity
    C / (M W).  Without that all-reduce (``--sync none``, one process) W is 1: every rank adds the whole sigma C / M.  Every rank's noise key is the 64-bit mix of ``seed + 7919 * rank``.  Rank 0 appends the cumulative
    epsilon per round (``utils.privacy`` at ``sample_rate = M / K``, one composition per round: the Poisson-subsampling
    bound applied to fixed-size sampling without replacement - an approximation, as for DP-SGD) with rank 0's median
    client norm and clipped share to ``--client-privacy-csv``.  ``avg_loss`` and the evaluation metrics are not private.
  * ``--server-opt {none,sgdm,adagrad,adam,yogi}`` / ``--server-beta1`` / ``--server-beta2`` / ``--server-tau``: a server
    optimizer (FedOpt) on a cohort round's averaged, clipped, noised client delta, with step size ``--server-lr`` (needs
    ``--clients-per-gpu``; ``train/server_opt.py`` states the rules).  Its state m / v is per rank, lives across rounds
    and is part of the per-rank checkpoint, so ``--resume`` continues it.  sgdm is linear in the delta: under ``--sync
    fedavg`` every rank keeps its own m and the unchanged all-reduce(AVG) of ``g + eta * m_rank`` is the global FedAvgM
    step with ``m = AVG(m_rank)``.  adagrad, adam and yogi are nonlinear in the delta and are rejected under ``--sync
    fedavg`` on more than one rank unless ``--server-scope global`` is given (they have to follow an all-reduce of the
    deltas); they run on one rank and under ``--sync none``.
  * ``--server-scope {rank,global}`` (default rank; global needs ``--clients-per-gpu``): with ``global`` a cohort round
    ends with the rank's averaged, clipped, noised delta in ``trainer.server_delta`` and the weights untouched; under
    ``--sync fedavg`` on several ranks that 5.8 KB buffer is all-reduced(AVG) in place of the weights and
    ``trainer.apply_server_step`` - the plain step or the server optimizer's - runs on every rank right after the wait
    that completes the collective (``FedAvgRound(on_averaged=...)``; ``--overlap tail``: after the next round's batch
    preparation, before its launch).  Every rank steps from the same g, m, v and averaged delta, so weights and
    optimizer state stay replicated, all five rules are exact, and m / v are global.  The mean of W deltas that each
    carry a sigma / sqrt(W) noise share has the noise the accountant assumes.  Without a collective (one rank,
    ``--sync none``) the step follows the round at once and ends on the bits of ``rank``.
  * ``--prox-mu mu``: FedProx local steps.  The local objective gains ``mu / 2 * |w - w_start|^2``, ``w_start`` the weights
    the local round started from - the averaged model; for a virtual client the round's global weights - so every step's
    gradient gains ``mu * (w - w_start)`` and passes through momentum like any other gradient.  TinyECG on the fused
    backend (in the reduce kernel's SGD epilogue, with or without ``--clients-per-gpu``) and any model on the torch
    backend; it composes with the server optimizers, client-level DP and ``--server-scope global``.  Not combined with
    ``--dp-clip``, ``--sync ddp``, fp16 AMP, the ResNet1D engine or ``--overlap delayed``.
  * ``--client-partition {contiguous,shards}`` / ``--client-shards s`` (need ``--clients-per-gpu``): with ``shards``
    every GPU's training windows are sorted by label, cut into K * s shards and dealt s to a virtual client
    (``data.dataset.shard_partition``, a function of the labels, K, s and ``seed + 7919 * rank``): label-skewed clients.
    A ``prox`` event in ``--jsonl`` records mu, the partition and s; no CSV and no checkpoint changes.
  * ``--client-partition dirichlet --client-alpha a`` / ``--local-epochs E`` / ``--aggregate {mean,weighted,nova}`` (need
    ``--clients-per-gpu``): unequal virtual clients.  ``dirichlet`` deals every GPU's training windows by the
    label-Dirichlet split (``data.dataset.dirichlet_partition``: sizes n_k and label mixes vary, every client holds at
    least a batch); ``--local-epochs E`` > 0 gives client k ``min(local_steps, max(1, E * (n_k // B)))`` local steps - the
    fused round freezes a finished client in the reduce kernel, the launches stay those of a full round;
    ``--aggregate weighted`` averages the clients' deltas with ``n_k / n`` over the cohort, ``nova`` with FedNova's
    ``p_k tau_eff / a_k`` (``train.cohort.weights_of``).  They compose with ``--prox-mu`` (not ``nova``), the server
    optimizers and ``--server-scope global`` and are rejected with ``--client-dp-clip``.  ``samples_per_s`` counts the
    ``B * sum_k S_k`` windows the cohort trained on; a ``cohort_shape`` event per round in ``--jsonl`` records rank 0's
    sizes, steps and weights; no CSV and no checkpoint changes (all three are functions of (seed, round)).  Every rank
    normalises over its own cohort, so under ``--sync fedavg`` the all-reduce(AVG) gives every rank's cohort the same
    total weight, whatever its share of the windows.
  * ``--aggregate {trimmed,median}`` / ``--trim-frac f`` / ``--flip-clients F`` (need ``--clients-per-gpu``): robust
    aggregation.  ``trimmed`` drops the ``floor(f * M)`` smallest and largest of a cohort's M deltas per parameter and
    averages the rest (``f`` in (0, 0.5), no default), ``median`` is the coordinate-wise median
    (``train.cohort.robust_delta``); the result takes the server step, a server optimizer or ``--server-scope global``
    like every other delta.  A cohort of at most 64; rejected with ``--client-dp-clip``.  ``--flip-clients F`` mirrors the
    training labels of every GPU's virtual clients 0..F-1 (``data.dataset.flip_client_labels``; the hold-out is
    untouched).  One ``robust`` event in ``--jsonl`` records the aggregate, f, k and F; no CSV and no checkpoint changes.
    Every rank trims within its own cohort: on W ranks the all-reduce(AVG) yields the mean of W robust estimates, not
    one estimate over all W * M clients.
"""
from __future__ import annotations

import os
import random
import time
from dataclasses import asdict
from glob import glob
from typing import Dict, List, Optional

import numpy as np
import torch

from ..config import FedAvgConfig
from ..data.dataset import load_shards_to_gpu
from ..data.shards import assign_shards_evenly
from ..models import build_model
from ..parallel.env import DistContext, barrier
from ..parallel.fedavg import Communicator, broadcast_model, weighted_fedavg_, model_flat
from ..parallel.overlap import CommRecord, FedAvgComm, FedAvgRound
from ..utils import profiling, usable_cpus
from ..utils.ckpt import (ckpt_path, save_checkpoint, load_checkpoint, latest_checkpoint, rank_state_path,
                          save_rank_state, load_trainer_local_state)
from ..utils.csvio import (RoundStats, append_results, ROUND_COLUMNS, EVAL_COLUMNS, PRIVACY_COLUMNS,
                           COHORT_COLUMNS, CLIENT_PRIVACY_COLUMNS)
from ..utils.philox import mix64
from .server_opt import ADAPTIVE as ADAPTIVE_SERVER_OPTS, check_server_opt, check_server_scope
from ..utils.privacy import epsilon as dp_epsilon
from ..utils.log import RankLogger
from .local import TorchLocalTrainer


def set_basic_seeds(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


def _sync(dev: torch.device):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def load_client_data(cfg: FedAvgConfig, ctx: DistContext):
    """This client's windows on its device: shards (round-robin) or on-device synthetic data."""
    dev = ctx.device
    if cfg.synthetic_windows > 0 or not cfg.data_root:
        n = cfg.synthetic_windows if cfg.synthetic_windows > 0 else cfg.max_windows
        n = min(n, cfg.max_windows) if cfg.max_windows else n
        g = torch.Generator(device=dev)
        g.manual_seed(1337 + ctx.rank)
        x = torch.randn((n, cfg.win_len), generator=g, device=dev)
        if cfg.labels == "parity":
            y = (x.mean(1) > 0).long()
        else:
            y = torch.zeros(n, dtype=torch.long, device=dev)
        return x, y
    paths = sorted(glob(os.path.join(cfg.data_root, "ecg_*.bin")))
    if not paths:
        raise RuntimeError(f"No ecg_*.bin files found in {cfg.data_root}")
    mine = assign_shards_evenly(paths, ctx.world_size, ctx.rank)
    return load_shards_to_gpu(mine, dev, max_windows=cfg.max_windows, labels=cfg.labels)


def split_holdout(cfg: FedAvgConfig, x, y, rank: int = 0):
    """(x_train, y_train, x_eval, y_eval): the last ``eval_windows`` windows are held out of training (views, no
    copy); 0 evaluates on the training windows themselves."""
    h = int(cfg.eval_windows)
    if h < 0 or cfg.eval_every < 0:
        raise ValueError("--eval-every and --eval-windows must be >= 0")
    if h == 0:
        return x, y, x, y
    if x.shape[0] - h < cfg.batch_size:
        raise RuntimeError(f"client {rank}: holding out --eval-windows {h} of {x.shape[0]} windows leaves "
                           f"{max(0, x.shape[0] - h)} training windows < batch {cfg.batch_size}")
    n = x.shape[0] - h
    return x[:n], y[:n], x[n:], y[n:]


def evaluate_client(trainer, model, backend: str, x_eval, y_eval, ctx: DistContext) -> torch.Tensor:
    """This client's evaluation record summed over all clients: a float64 vector {loss_sum, count, correct,
    conf...} on the host (one all-reduce(SUM); the integer counts are exact below 2^53)."""
    if backend == "fused":
        res = trainer.evaluate(x_eval, y_eval)
    else:
        from ..ops.tiny_eval import evaluate_torch
        res = evaluate_torch(model, x_eval, y_eval)
    vec = res.to_vector()
    if ctx.distributed:
        import torch.distributed as dist
        if ctx.backend != "nccl":
            vec = vec.cpu()
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
    return vec.cpu()


def eval_row(cname: str, world: int, r: int, vec: torch.Tensor, nc: int, eval_ms: float, backend: str,
             precision: str) -> Dict:
    from ..ops.tiny_eval import EvalResult, confusion_str
    res = EvalResult.from_vector(vec, nc)
    return {"config": cname, "world_size": world, "round_idx": r, "windows": res.count, "loss": res.loss,
            "accuracy": res.accuracy, "confusion": confusion_str(res.confusion), "eval_ms": eval_ms,
            "backend": backend, "precision": precision}


def _amp(cfg: FedAvgConfig):
    return {"bf16": torch.bfloat16, "fp16": torch.float16, "none": None}[cfg.amp_dtype]


def check_dp_config(cfg: FedAvgConfig, config_name: str, backend: str) -> None:
    """DP-SGD exists for TinyECG on the fused and torch backends, in fp32 or bf16, with local rounds."""
    if cfg.dp_clip < 0 or cfg.dp_noise < 0:
        raise ValueError("--dp-clip and --dp-noise must be >= 0")
    if cfg.dp_noise > 0 and cfg.dp_clip == 0:
        raise ValueError("--dp-noise needs --dp-clip > 0: the noise is scaled by the clip norm")
    if cfg.dp_clip == 0:
        return
    if not 0.0 < cfg.dp_delta < 1.0:
        raise ValueError("--dp-delta must be in (0, 1)")
    if backend == "hip" or cfg.model != "tiny_ecg":
        raise ValueError("DP-SGD (--dp-clip) is implemented for TinyECG on the fused and torch backends, not for "
                         "the ResNet1D engine (--kernel-backend hip)")
    if config_name == "G1" and cfg.amp_dtype == "fp16":
        raise ValueError("DP-SGD (--dp-clip) does not support fp16 AMP: its GradScaler would rescale the clipped "
                         "gradients; use --amp-dtype bf16 or none")
    if cfg.sync == "ddp":
        raise ValueError("DP-SGD (--dp-clip) does not support --sync ddp: " + (
            "the fused backend's per-step gradient all-reduce bypasses the round that clips and adds noise"
            if backend == "fused" else "per-sample gradients bypass DistributedDataParallel's gradient hooks"))


def check_prox_config(cfg: FedAvgConfig, config_name: str, backend: str) -> None:
    """FedProx exists for TinyECG on the fused backend and for any model on the torch backend, with local rounds that
    start from the averaged model; a client partition other than the contiguous one needs client sampling."""
    from ..data.dataset import PARTITIONS
    if not cfg.prox_mu >= 0:
        raise ValueError("--prox-mu must be >= 0")
    if cfg.client_partition not in PARTITIONS or (cfg.client_partition == "dirichlet" and not cfg.client_alpha > 0):
        raise ValueError(f"--client-partition must be one of {list(PARTITIONS)}, dirichlet together with its "
                         f"concentration --client-alpha a > 0 (there is no default); got {cfg.client_partition!r} with "
                         f"--client-alpha {cfg.client_alpha:g}")
    if cfg.client_shards < 1:
        raise ValueError("--client-shards must be >= 1")
    if (cfg.client_partition != "contiguous" or cfg.client_shards != 2) and cfg.clients_per_gpu <= 1:
        raise ValueError("--client-partition / --client-shards need client sampling (--clients-per-gpu K > 1): they "
                         "deal a GPU's windows to its virtual clients")
    if cfg.prox_mu == 0:
        return
    if backend == "hip":
        raise ValueError("FedProx (--prox-mu) is implemented for TinyECG on the fused backend and for the torch backend, "
                         "not for the ResNet1D engine (--kernel-backend hip)")
    if cfg.sync == "ddp":
        raise ValueError("FedProx (--prox-mu) does not support --sync ddp: its per-step gradient all-reduce bypasses "
                         "the round, and with it the round's starting weights that the proximal term pulls towards")
    if cfg.dp_clip > 0:
        raise ValueError("FedProx (--prox-mu) does not support DP-SGD (--dp-clip): the proximal gradient is not part "
                         "of the clipped per-sample gradients, and the DP reduce has no proximal term")
    if config_name == "G1" and cfg.amp_dtype == "fp16":
        raise ValueError("FedProx (--prox-mu) does not support fp16 AMP: its GradScaler would rescale the proximal "
                         "gradient; use --amp-dtype bf16 or none")
    if cfg.overlap == "delayed":
        raise ValueError("FedProx (--prox-mu) does not support --overlap delayed: a round there starts before the "
                         "averaged model exists, so its starting weights are not the anchor FedProx defines")


def hetero_on(cfg: FedAvgConfig) -> bool:
    """Unequal virtual clients: a Dirichlet partition, per-client local steps or a weighted aggregate."""
    return cfg.client_partition == "dirichlet" or cfg.local_epochs != 0 or cfg.aggregate != "mean"


def check_hetero_config(cfg: FedAvgConfig) -> None:
    """``--client-alpha`` / ``--local-epochs`` / ``--aggregate`` act on a cohort round's virtual clients: they need client
    sampling, and none of them goes with client-level DP."""
    from .cohort import AGGREGATES
    if cfg.aggregate not in AGGREGATES:
        raise ValueError(f"--aggregate must be one of {list(AGGREGATES)}, got {cfg.aggregate!r}")
    if cfg.local_epochs < 0:
        raise ValueError("--local-epochs must be >= 0")
    if cfg.client_alpha < 0:
        raise ValueError("--client-alpha must be > 0")
    if cfg.client_alpha > 0 and cfg.client_partition != "dirichlet":
        raise ValueError("--client-alpha is the concentration of --client-partition dirichlet: it needs that partition")
    if not hetero_on(cfg):
        return
    if cfg.clients_per_gpu <= 1:
        raise ValueError("--client-partition dirichlet / --local-epochs / --aggregate need client sampling "
                         "(--clients-per-gpu K > 1): they size, time and weight a GPU's virtual clients")
    if cfg.client_dp_clip > 0:
        if cfg.aggregate != "mean":
            raise ValueError(f"--aggregate {cfg.aggregate} does not support --client-dp-clip: the sensitivity of a "
                             "weighted, clipped mean is not C / M, and no accountant here covers it")
        if cfg.local_epochs != 0:
            raise ValueError("--local-epochs does not support --client-dp-clip: the accountant assumes clients that "
                             "differ in their data only, and the clip norm would bind short and long clients unevenly")
        raise ValueError("--client-partition dirichlet does not support --client-dp-clip: the accountant's sample rate "
                         "M / K assumes exchangeable clients, and clients of unequal sizes are not")
    if cfg.aggregate == "nova" and cfg.prox_mu > 0:
        raise ValueError("--aggregate nova does not support --prox-mu: its normaliser is derived for heavy-ball "
                         "momentum SGD, not for proximal steps")


def cohort_size(cfg: FedAvgConfig) -> int:
    """Clients trained per GPU and round: 1 without client sampling, else ``--cohort`` (default: all K)."""
    if cfg.clients_per_gpu <= 1:
        return 1
    return cfg.cohort if cfg.cohort else cfg.clients_per_gpu


def split_aggregate(cfg: FedAvgConfig):
    """``--aggregate`` names either the clients' weights (mean, weighted, nova: the trainers' ``aggregate``) or a robust
    estimate (trimmed, median: their ``robust``), which takes no weights.  Returns (the configuration as the checks and
    events of the weights see it - a robust estimate counts as "mean" there -, the trainers' ``robust``)."""
    from dataclasses import replace
    if cfg.aggregate in ("trimmed", "median"):
        return replace(cfg, aggregate="mean"), cfg.aggregate
    return cfg, "none"


def robust_on(cfg: FedAvgConfig) -> bool:
    """A robust aggregate or poisoned clients."""
    return cfg.aggregate in ("trimmed", "median") or cfg.trim_frac != 0 or cfg.flip_clients != 0


def check_robust_config(cfg: FedAvgConfig) -> int:
    """``--aggregate trimmed | median``, ``--trim-frac`` and ``--flip-clients`` act on a cohort round's virtual clients:
    they need client sampling.  Returns k, the clients dropped at each end (0: not a robust close)."""
    from .cohort import AGGREGATES, ROBUST_AGGREGATES, ROBUST_MAX_COHORT, trim_count
    if cfg.aggregate not in AGGREGATES + ROBUST_AGGREGATES:
        raise ValueError(f"--aggregate must be one of {list(AGGREGATES + ROBUST_AGGREGATES)}, got {cfg.aggregate!r}")
    if not robust_on(cfg):
        return 0
    if cfg.clients_per_gpu <= 1:
        raise ValueError("--aggregate trimmed / median, --trim-frac and --flip-clients need client sampling "
                         "(--clients-per-gpu K > 1): they act on a GPU's virtual clients")
    if cfg.flip_clients < 0 or cfg.flip_clients > cfg.clients_per_gpu:
        raise ValueError(f"--flip-clients must be in [0, --clients-per-gpu = {cfg.clients_per_gpu}], got "
                         f"{cfg.flip_clients}")
    if cfg.trim_frac != 0 and cfg.aggregate != "trimmed":
        raise ValueError(f"--trim-frac is the share --aggregate trimmed drops at each end: it needs that aggregate, not "
                         f"--aggregate {cfg.aggregate}")
    if cfg.aggregate not in ROBUST_AGGREGATES:
        return 0
    if cfg.client_dp_clip > 0:
        raise ValueError(f"--aggregate {cfg.aggregate} does not support --client-dp-clip: the sensitivity of a trimmed "
                         "mean is not C / M, and no accountant here covers it")
    M = cohort_size(cfg)
    if M > ROBUST_MAX_COHORT:
        raise ValueError(f"--aggregate {cfg.aggregate} needs a cohort of at most {ROBUST_MAX_COHORT} clients, got {M}: "
                         "the selection kernel holds one parameter's clients in the lanes of one wave")
    if cfg.aggregate == "trimmed":
        if cfg.trim_frac == 0:
            raise ValueError("--aggregate trimmed needs --trim-frac f, the share of the cohort dropped at each end: "
                             "there is no default")
        if not 0.0 < cfg.trim_frac < 0.5:
            raise ValueError(f"--trim-frac must be in (0, 0.5), got {cfg.trim_frac:g}")
    return trim_count(cfg.aggregate, M, cfg.trim_frac if cfg.aggregate == "trimmed" else None)


def check_cohort_config(cfg: FedAvgConfig, backend: str) -> None:
    """Client sampling (--clients-per-gpu K > 1) exists for TinyECG on the fused and torch backends, exact FedAvg."""
    K, M = cfg.clients_per_gpu, cfg.cohort
    if K < 1 or M < 0:
        raise ValueError("--clients-per-gpu must be >= 1 and --cohort >= 0")
    if M > K:
        raise ValueError(f"--cohort {M} exceeds --clients-per-gpu {K}: a cohort is drawn without replacement")
    if K == 1:
        return
    if backend == "hip" or cfg.model != "tiny_ecg":
        raise ValueError("client sampling (--clients-per-gpu) is implemented for TinyECG, not for ResNet1D models")
    if cfg.dp_clip > 0 and cfg.dp_noise == 0:
        raise ValueError("client sampling (--clients-per-gpu) takes DP-SGD (--dp-clip) only together with --dp-noise > 0: "
                         "clipping alone gives a record no guarantee, and the per-client epsilon this driver reports "
                         "for a cohort is undefined without noise")
    if cfg.sync == "ddp":
        raise ValueError("client sampling (--clients-per-gpu) does not support --sync ddp: virtual clients are "
                         "averaged per round, not per step")
    if cfg.drop_prob > 0:
        raise ValueError("client sampling (--clients-per-gpu) replaces --drop-prob: draw a smaller --cohort instead")
    if cfg.overlap == "delayed":
        raise ValueError("client sampling (--clients-per-gpu) does not support --overlap delayed: every cohort "
                         "starts from the averaged weights of the round before")


def check_client_dp_config(cfg: FedAvgConfig) -> None:
    """Client-level DP and the server step size act on a cohort round: they need client sampling (and with it
    everything ``check_cohort_config`` asks for)."""
    if cfg.client_dp_clip < 0 or cfg.client_dp_noise < 0:
        raise ValueError("--client-dp-clip and --client-dp-noise must be >= 0")
    if cfg.client_dp_noise > 0 and cfg.client_dp_clip == 0:
        raise ValueError("--client-dp-noise needs --client-dp-clip > 0: the noise is scaled by the clip norm")
    if not cfg.server_lr > 0:
        raise ValueError("--server-lr must be > 0")
    if cfg.client_dp_clip == 0 and cfg.server_lr == 1.0:
        return
    if cfg.clients_per_gpu <= 1:
        raise ValueError("--client-dp-clip / --client-dp-noise / --server-lr need client sampling (--clients-per-gpu "
                         "K > 1): they clip, noise and scale the mean of a cohort's client deltas")
    if cfg.client_dp_clip > 0 and not 0.0 < cfg.client_dp_delta < 1.0:
        raise ValueError("--client-dp-delta must be in (0, 1)")


def check_server_opt_config(cfg: FedAvgConfig, ctx: DistContext) -> None:
    """A server optimizer acts on a cohort round's averaged client delta: it needs client sampling (and with it
    everything ``check_cohort_config`` asks for).  Under ``--sync fedavg`` on W > 1 ranks only sgdm is exact: its rule
    is linear in Delta, so the all-reduce(AVG) of the ranks' ``g + eta * m_rank`` is the global FedAvgM step with
    ``m = AVG(m_rank)``; the adaptive rules are nonlinear in Delta and have to follow an all-reduce of the deltas, which
    is what ``--server-scope global`` does (for every rule, the plain step included; it needs client sampling too)."""
    check_server_opt(cfg.server_opt, cfg.server_beta1, cfg.server_beta2, cfg.server_tau)
    check_server_scope(cfg.server_scope)
    if cfg.server_scope == "global" and cfg.clients_per_gpu <= 1:
        raise ValueError("--server-scope global needs client sampling (--clients-per-gpu K > 1): it all-reduces the "
                         "mean of a cohort's client deltas and steps on the result")
    if cfg.server_opt == "none":
        return
    if cfg.clients_per_gpu <= 1:
        raise ValueError("--server-opt / --server-beta1 / --server-beta2 / --server-tau need client sampling "
                         "(--clients-per-gpu K > 1): the server optimizer steps on the mean of a cohort's client deltas")
    if (cfg.server_scope == "rank" and cfg.server_opt in ADAPTIVE_SERVER_OPTS and cfg.sync == "fedavg"
            and ctx.distributed and ctx.world_size > 1):
        raise ValueError(f"--server-opt {cfg.server_opt} does not support --sync fedavg on more than one rank: its step "
                         "m / (sqrt(v) + tau) is nonlinear in the averaged delta, so it must follow the all-reduce of "
                         "the ranks' deltas, and under --server-scope rank the driver all-reduces the weights after each "
                         "rank's own step; use --server-scope global, which all-reduces the deltas and takes one "
                         "replicated step on every rank, or --server-opt sgdm, whose rule is linear, one rank, or "
                         "--sync none")


def client_dp_world(cfg: FedAvgConfig, ctx: DistContext) -> int:
    """The number of ranks whose weights the driver averages after a round: every rank adds sigma / sqrt(that) of the
    client-level noise.  Only ``--sync fedavg`` on more than one rank averages; an independent client (``--sync none``, a
    single process) keeps its own weights and must add the whole of the noise itself."""
    return ctx.world_size if (cfg.sync == "fedavg" and ctx.distributed) else 1


def make_trainer(cfg: FedAvgConfig, config_name: str, model, x, y, ctx: DistContext, backend: str):
    seed = cfg.seed + 7919 * ctx.rank
    check_dp_config(cfg, config_name, backend)
    check_cohort_config(cfg, backend)
    check_client_dp_config(cfg)
    check_server_opt_config(cfg, ctx)
    check_prox_config(cfg, config_name, backend)
    check_robust_config(cfg)
    wcfg, robust = split_aggregate(cfg)
    check_hetero_config(wcfg)
    if cfg.clients_per_gpu > 1:
        kw = dict(robust=robust, trim_frac=cfg.trim_frac if robust == "trimmed" else None,
                  flip_clients=cfg.flip_clients,
                  dirichlet_alpha=cfg.client_alpha, local_epochs=cfg.local_epochs, aggregate=wcfg.aggregate,
                  prox_mu=cfg.prox_mu, partition=cfg.client_partition, shards_per_client=cfg.client_shards,
                  clients=cfg.clients_per_gpu, cohort=cohort_size(cfg), lr=cfg.lr, momentum=cfg.momentum, seed=seed,
                  client_dp_clip=cfg.client_dp_clip, client_dp_noise=cfg.client_dp_noise, client_dp_seed=mix64(seed),
                  server_lr=cfg.server_lr, world_size=client_dp_world(cfg, ctx), server_opt=cfg.server_opt,
                  server_beta1=cfg.server_beta1, server_beta2=cfg.server_beta2, server_tau=cfg.server_tau,
                  server_scope=cfg.server_scope,
                  dp_clip=cfg.dp_clip, dp_noise=cfg.dp_noise, dp_seed=mix64(seed))  # (stream words 2 + c: apart from
        # the client-level close's stream 1 under the same key)
        if backend == "fused":
            from ..ops.fused_cohort import FusedCohortTrainer
            prec = "bf16" if (config_name == "G1" and cfg.amp_dtype == "bf16") else "fp32"
            return FusedCohortTrainer(model, x, y, cfg.batch_size, cfg.local_steps, precision=prec, **kw)
        from .cohort import TorchCohortTrainer
        if config_name == "G1" and cfg.amp_dtype == "fp16":
            raise ValueError("client sampling (--clients-per-gpu) on the torch backend runs fp32 or bf16 AMP, not fp16")
        return TorchCohortTrainer(model, x, y, cfg.batch_size, cfg.local_steps,
                                  amp_dtype=None if config_name == "G0" else _amp(cfg), **kw)
    dp = dict(dp_clip=cfg.dp_clip, dp_noise=cfg.dp_noise, dp_seed=mix64(seed))
    if backend == "fused":
        from ..ops.fused_tiny import FusedTinyTrainer
        prec = "bf16" if (config_name == "G1" and cfg.amp_dtype == "bf16") else "fp32"
        return FusedTinyTrainer(model, x, y, cfg.batch_size, cfg.local_steps, lr=cfg.lr, momentum=cfg.momentum,
                                seed=seed, precision=prec, prox_mu=cfg.prox_mu, **dp)
    if backend == "hip":  # ResNet1D on the native step engine
        from .resnet_trainer import ResNetEngineTrainer
        return ResNetEngineTrainer(model, x, y, cfg.batch_size, cfg.local_steps, lr=cfg.lr, momentum=cfg.momentum,
                                   seed=seed, ctx=ctx, sync=cfg.sync, bucket_mb=cfg.bucket_mb)
    amp = None if config_name == "G0" else _amp(cfg)
    net = model
    if cfg.sync == "ddp" and ctx.distributed:
        from torch.nn.parallel import DistributedDataParallel as DDP
        net = DDP(model, device_ids=[dev_index(ctx)] if ctx.device.type == "cuda" else None, bucket_cap_mb=cfg.bucket_mb)
    return TorchLocalTrainer(net, x, y, cfg.batch_size, lr=cfg.lr, momentum=cfg.momentum, amp_dtype=amp, seed=seed,
                             prox_mu=cfg.prox_mu, **dp)


def dev_index(ctx):
    return ctx.device.index if ctx.device.index is not None else 0


def pick_backend(cfg: FedAvgConfig, config_name: str, ctx: DistContext) -> str:
    if cfg.kernel_backend == "torch" or ctx.device.type != "cuda":
        return "torch"
    if cfg.model.startswith("resnet"):
        if cfg.kernel_backend == "fused":
            raise ValueError("the fused HIP step implements TinyECG only; use --kernel-backend hip for ResNet1D")
        # the MFMA conv kernels compute in bf16: G1 with bf16 AMP only; G0 keeps fp32 semantics on MIOpen
        return "hip" if (config_name == "G1" and cfg.amp_dtype == "bf16") else "torch"
    # fused HIP step: TinyECG in fp32 (G0, or G1 with --amp-dtype none) or bf16 AMP (G1); fp16 AMP keeps the
    # reference's GradScaler path on eager PyTorch
    fused_ok = cfg.model == "tiny_ecg" and (config_name == "G0" or cfg.amp_dtype in ("bf16", "none"))
    if cfg.kernel_backend == "fused":
        if not fused_ok:
            raise ValueError("the fused HIP step implements TinyECG in fp32 or bf16 (not --amp-dtype fp16)")
        return "fused"
    return "fused" if fused_ok else "torch"


def _ddp_fused_round(trainer, ctx: DistContext, n: int):
    """Synchronous data parallel on the fused kernels: grads -> RCCL all-reduce(AVG) -> flat SGD per step."""
    from ..ops import _lib
    from ..ops.fused_tiny import tiny_step_grads
    from ..ops.sgd import FlatSGD
    from ..parallel.fedavg import allreduce_mean_
    if not hasattr(trainer, "_ddp_opt"):
        trainer._ddp_grad = torch.zeros_like(trainer.params)
        trainer._ddp_opt = FlatSGD(trainer.params, trainer._ddp_grad, lr=trainer.lr, momentum=trainer.momentum)
    table = trainer.take_staged(n)  # batches already drawn by trainer.prepare_round(n)
    lib = _lib.kernels()
    for s in range(n):
        tiny_step_grads(trainer.params, trainer.x, trainer.y32, table[s], trainer.B, trainer.nc, trainer.slab,
                        precision=trainer.precision, prefrag=trainer.prefrag, wprep=trainer.wprep)
        st = lib.ecg_slab_reduce_sgd(trainer.slab.data_ptr(), trainer.B, trainer.stride, trainer.P, None, None,
                                     trainer._ddp_grad.data_ptr(), trainer.loss_acc.data_ptr(), 0.0, 0.0, 0.0, 0, 0,
                                     None, _lib.stream_ptr(trainer.device))
        _lib.check(st, "ecg_slab_reduce_sgd")
        allreduce_mean_(trainer._ddp_grad, ctx)
        trainer._ddp_opt.step()


def _resume(cfg: FedAvgConfig, cname: str, ctx: DistContext, comm: Communicator, model, trainer, log) -> int:
    """Rank 0 resolves and loads the latest checkpoint and tells every rank the round to start from; each rank
    restores its own client state (momentum, sampler, RNG) when its directory has it (utils/ckpt.py)."""
    path = latest_checkpoint(cfg.ckpt_dir, cname) if ctx.rank == 0 else None
    rnd = -1
    if path:
        st = load_checkpoint(path)
        model.load_state_dict(st["model"])
        rnd = int(st["round"])
    rnd = int(comm.bcast(rnd, root=0))
    if rnd < 0:
        return 0
    own = rank_state_path(cfg.ckpt_dir, rnd, cname, ctx.rank)
    independent = cfg.sync not in ("fedavg", "ddp") or not ctx.distributed
    if os.path.exists(own):
        st = load_checkpoint(own)
        load_trainer_local_state(trainer, st)
        if st.get("client_weights") is not None:  # --sync none: every client continues from its OWN weights
            flat = model_flat(model)
            if st["client_weights"].shape != flat.shape:
                raise ValueError(f"client weights {tuple(st['client_weights'].shape)} != {tuple(flat.shape)}")
            with torch.no_grad():
                flat.copy_(st["client_weights"].to(flat.device))
        elif independent and ctx.rank != 0:
            raise RuntimeError(f"{own} holds no client weights: cannot resume an independent (--sync "
                               f"{cfg.sync}) client without them")
        log.info(f"[fedavg] rank {ctx.rank}: client state restored from {own}")
    elif independent and ctx.rank != 0:
        raise RuntimeError(f"--resume with --sync {cfg.sync}: {own} is missing; an independent client cannot be "
                           "restored from rank 0's model")
    else:
        log.info(f"[fedavg] rank {ctx.rank}: no {own}; momentum restarts at zero, sampler from its seed")
    if ctx.rank == 0:
        log.info(f"[fedavg] resumed {cname} from {path} at round {rnd + 1}")
    return rnd + 1


def run_fedavg(cfg: FedAvgConfig, ctx: DistContext) -> List[Dict]:
    log = RankLogger(ctx.rank, cfg.jsonl, cfg.quiet)
    if "{rank}" in (cfg.ckpt_dir or ""):  # node-local checkpoint directories (no shared filesystem)
        cfg.ckpt_dir = cfg.ckpt_dir.format(rank=ctx.rank)
    comm = Communicator(ctx)
    dev = ctx.device
    torch.set_num_threads(max(1, min(4, usable_cpus())))
    x, y = load_client_data(cfg, ctx)
    if x.shape[0] < cfg.batch_size:
        raise RuntimeError(f"client {ctx.rank} has {x.shape[0]} windows < batch {cfg.batch_size}")
    x, y, x_eval, y_eval = split_holdout(cfg, x, y, ctx.rank)
    log.info(f"[fedavg] world={ctx.world_size} backend={ctx.backend} device={dev} windows/client={x.shape[0]} "
             f"L={x.shape[1]} B={cfg.batch_size} rounds={cfg.rounds}x{cfg.local_steps} sync={cfg.sync} "
             f"overlap={cfg.overlap}")
    configs = ["G0", "G1"] if cfg.config == "both" else [cfg.config]
    for cname in configs:  # an unsupported DP-SGD combination stops the run before any configuration trains
        check_dp_config(cfg, cname, pick_backend(cfg, cname, ctx))
        check_cohort_config(cfg, pick_backend(cfg, cname, ctx))
        check_prox_config(cfg, cname, pick_backend(cfg, cname, ctx))
    check_client_dp_config(cfg)
    check_server_opt_config(cfg, ctx)
    robust_k = check_robust_config(cfg)
    check_hetero_config(split_aggregate(cfg)[0])
    M = cohort_size(cfg)  # clients trained per GPU and round (1: no client sampling)
    all_rows: List[Dict] = []
    fcomm = FedAvgComm(ctx)
    for cname in configs:
        set_basic_seeds(cfg.seed + ctx.rank)
        torch.manual_seed(cfg.seed)  # identical init on every client (the round-0 broadcast makes it exact)
        model = build_model(cfg.model, cfg.num_classes).to(dev)
        backend = pick_backend(cfg, cname, ctx)
        if hasattr(model, "flatten_parameters"):
            model.flatten_parameters()
        trainer = make_trainer(cfg, cname, model, x, y, ctx, backend)
        log.info(f"[fedavg] {cname}: kernel backend {backend}")
        if cfg.server_opt != "none":
            log.event("server_opt", config=cname, server_opt=cfg.server_opt, server_lr=cfg.server_lr,
                      beta1=cfg.server_beta1, beta2=cfg.server_beta2, tau=cfg.server_tau, scope=cfg.server_scope)
        if cfg.prox_mu > 0 or cfg.client_partition != "contiguous":
            log.event("prox", config=cname, mu=cfg.prox_mu, partition=cfg.client_partition,
                      shards_per_client=cfg.client_shards)
        if robust_on(cfg):
            log.event("robust", config=cname, aggregate=cfg.aggregate, trim_frac=cfg.trim_frac, k=robust_k,
                      flip_clients=cfg.flip_clients)
        start_round = _resume(cfg, cname, ctx, comm, model, trainer, log) if cfg.resume else 0
        if hasattr(trainer, "set_cohort_round"):  # the cohort sampler is a function of (seed, round): no other state
            trainer.set_cohort_round(start_round)
        fedavg = cfg.sync == "fedavg" and ctx.distributed
        weighted = fedavg and cfg.drop_prob > 0
        mode = cfg.overlap if (fedavg and not weighted) else "none"
        # ResNet engine: the tail step applies SGD per backward segment and all-reduces each segment at once
        seg_tail = mode == "tail" and hasattr(trainer, "tail_fedavg")
        # --server-scope global: a cohort round ends with the rank's delta; under FedAvg the delta is what is
        # all-reduced - not the weights: every rank takes the same step from the same g, m, v and averaged delta - and
        # the step follows the wait that completes the collective; without a collective it follows the round at once
        split = cfg.server_scope == "global" and cfg.clients_per_gpu > 1
        if split and fedavg:
            fround = FedAvgRound(trainer.server_delta, fcomm, mode, on_averaged=trainer.apply_server_step)
        else:
            fround = FedAvgRound(model_flat(model), fcomm, "none" if seg_tail else mode)
        if hasattr(trainer, "prepare"):  # capture + upload + warm the round graphs outside round 0's timing
            trainer.prepare([cfg.local_steps - 1 if seg_tail else cfg.local_steps])
        recs = []
        evals = []  # (round, summed record, this rank's eval_ms) per evaluated round
        privacy = []  # DP-SGD: this client's cumulative (round, steps, epsilon)
        cohorts = []  # client sampling: (round, this rank's drawn client ids)
        shapes = []  # unequal clients: (round, this rank's cohort sizes, steps, weights)
        hetero = hetero_on(split_aggregate(cfg)[0]) and cfg.clients_per_gpu > 1
        client_privacy = []  # client-level DP, rank 0: (round, median client norm, clipped share)
        sample_rate = cfg.batch_size / x.shape[0]
        # record-level DP-SGD in cohort rounds: the local steps each of this rank's K virtual clients has run so far.
        # The sampler is a pure function of (seed, round), so a resumed run recounts the rounds before it.
        cohort_dp = cfg.dp_clip > 0 and cfg.clients_per_gpu > 1
        client_steps = [0] * cfg.clients_per_gpu
        if cohort_dp:
            for r0 in range(start_round):
                ids0 = trainer.sampler.clients_of(r0)
                for k, sk in zip(ids0, trainer.sampler.steps_of(ids0, cfg.local_epochs)):
                    client_steps[k] += min(cfg.local_steps, sk)
        for r in range(start_round, cfg.rounds):
            t_round0 = time.perf_counter()
            rec = CommRecord()
            # ---- broadcast the global model (round 0 / resume / every round for reference parity) ----------
            # (--overlap tail / delayed skip the per-round re-broadcast: it would drain the in-flight all-reduce
            # and serialise the overlap away, and the RCCL AVG already leaves identical weights on every client)
            if ctx.distributed and cfg.sync in ("fedavg", "ddp") and (
                    r == start_round or (fedavg and cfg.bcast_every_round and mode == "none")):
                fround.finalize()  # nothing is in flight here except at a resume boundary
                with profiling.range("bcast"):
                    fcomm.blocking(lambda: broadcast_model(comm, model), rec)
            # ---- local steps (the previous round's tail all-reduce overlaps this round's batch preparation) --
            n = cfg.local_steps - 1 if seg_tail else cfg.local_steps
            m_l0 = fcomm.mark()
            stalls0 = len(fround._rec.stalls) if fround._rec is not None else 0
            prev_rec = fround._rec

            def prep(n=n):
                trainer.prepare_round(n)
                if cfg.inject_prep_delay_ms > 0:  # latency injection (weight-independent host work)
                    time.sleep(cfg.inject_prep_delay_ms / 1e3)

            with profiling.range("local_round"):
                fround.begin_round(prep=prep)
                if cfg.sync == "ddp" and backend == "fused" and ctx.distributed:
                    _ddp_fused_round(trainer, ctx, n)
                else:
                    trainer.launch_round(n)
                    if split and not fedavg:
                        trainer.apply_server_step()
                if seg_tail:  # the round's last step, its segment all-reduces overlapping its own backward
                    trainer.tail_fedavg(fcomm, rec)
            m_l1 = fcomm.mark()
            if cfg.clients_per_gpu > 1:
                cohorts.append((r, list(trainer.round_clients)))
                if hetero:
                    shapes.append((r,) + tuple(list(v) for v in trainer.last_round_shape()))
            if cohort_dp:
                # a record of virtual client k is touched only in the rounds that draw k, at sample rate B / n_k: the
                # round's figure is the largest epsilon over this rank's clients (no amplification by client sampling)
                for k, sk in zip(trainer.round_clients, trainer.last_round_shape()[1]):
                    client_steps[k] += sk
                privacy.append(max(
                    ((r, sk, cfg.batch_size / nk, dp_epsilon(cfg.dp_noise, cfg.batch_size / nk, sk, cfg.dp_delta))
                     for sk, nk in zip(client_steps, map(int, trainer.sampler.sizes_of(range(cfg.clients_per_gpu)))) if sk > 0),
                    key=lambda t: t[3]))
            elif cfg.dp_clip > 0:
                privacy.append((r, trainer.dp_steps, sample_rate,
                                dp_epsilon(cfg.dp_noise, sample_rate, trainer.dp_steps, cfg.dp_delta)))
            # the stall on the previous round's collective happened inside [m_l0, m_l1]: not local work
            inner = prev_rec.stalls[stalls0:] if prev_rec is not None else []
            inner = inner + (rec.stalls if seg_tail else [])
            # ---- FedAvg ----------------------------------------------------------------------------------
            if fedavg:
                with profiling.range("fedavg"):
                    if weighted:
                        rng = random.Random(cfg.seed * 1000003 + r * 8191 + ctx.rank)
                        w = 0.0 if rng.random() < cfg.drop_prob else float(cfg.batch_size * cfg.local_steps)
                        fcomm.blocking(lambda: weighted_fedavg_(model_flat(model), w, ctx), rec)
                    elif not seg_tail:
                        fround.end_round(rec)
            due = bool(cfg.ckpt_every) and (r + 1) % cfg.ckpt_every == 0
            eval_due = cfg.eval_every > 0 and (r + 1) % cfg.eval_every == 0
            if (due or eval_due) and mode != "delayed":
                fround.finalize()  # checkpoints hold averaged weights (drains an in-flight tail all-reduce)
            avg_loss = trainer.avg_loss()
            if due:
                own = model_flat(model) if cfg.sync not in ("fedavg", "ddp") else None  # independent clients
                if ctx.rank == 0:
                    mom = getattr(trainer, "mom", None)
                    with fround.averaged_in_place():  # delayed: avg_r saved, the stale correction stays pending
                        save_checkpoint(ckpt_path(cfg.ckpt_dir, r, cname), r, model, mom, cname, asdict(cfg))
                save_rank_state(cfg.ckpt_dir, r, cname, ctx.rank, trainer, client_weights=own)
            # windows the round trained on: B * sum_k S_k with unequal local work
            windows = cfg.batch_size * (sum(shapes[-1][2]) if hetero else M * cfg.local_steps)
            recs.append((r, rec, m_l0, m_l1, inner, avg_loss, (time.perf_counter() - t_round0) * 1e3, windows))
            if cfg.client_dp_clip > 0 and ctx.rank == 0:  # (avg_loss synchronised: the round's norms are there)
                norms, clipped = trainer.last_clip_stats()
                client_privacy.append((r, float(np.median(norms)), clipped))
            if eval_due:  # after the round's wall clock stopped; the stream is idle (avg_loss synchronised)
                _sync(dev)
                t_e0 = time.perf_counter()
                with profiling.range("evaluate"), fround.averaged_in_place():  # the weights a checkpoint would hold
                    vec = evaluate_client(trainer, model, backend, x_eval, y_eval, ctx)
                    _sync(dev)
                evals.append((r, vec, (time.perf_counter() - t_e0) * 1e3))
        fround.finalize()
        _sync(dev)
        rows = []
        for r, rec, m_l0, m_l1, inner, avg_loss, wall_ms, windows in recs:
            local_ms = m_l0.ms_to(m_l1) - sum(a.ms_to(b) for a, b in inner)
            row = RoundStats(config=cname, world_size=ctx.world_size, rank=ctx.rank, round_idx=r,
                             batch_size=cfg.batch_size, local_steps=cfg.local_steps, local_train_ms=local_ms,
                             comm_ms=rec.comm_ms(), samples_per_s=windows / (local_ms / 1e3),
                             avg_loss=avg_loss, comm_exposed_ms=rec.exposed_ms(), round_wall_ms=wall_ms,
                             backend=backend, overlap=(cfg.overlap if not weighted else "none")
                             if cfg.sync == "fedavg" else cfg.sync)
            rows.append(asdict(row))
            log.event("round", **asdict(row))
        if hasattr(trainer, "close"):
            trainer.close()
        if evals:
            prec = getattr(trainer, "precision", "fp32")
            all_ms = comm.gather([ms for _, _, ms in evals], root=0)
            if ctx.rank == 0:
                erows = [eval_row(cname, ctx.world_size, r, vec, cfg.num_classes, max(ms[i] for ms in all_ms),
                                  backend, prec) for i, (r, vec, _) in enumerate(evals)]
                if cfg.eval_csv:
                    append_results(erows, cfg.eval_csv, EVAL_COLUMNS)
                for e in erows:
                    log.event("eval", **e)
                    log.info(f"[eval] {cname} round {e['round_idx']}: {e['windows']} windows loss {e['loss']:.4f} "
                             f"accuracy {e['accuracy']:.4f} confusion {e['confusion']} ({e['eval_ms']:.2f} ms)")
        if privacy:
            prows = [{"config": cname, "world_size": ctx.world_size, "rank": ctx.rank, "round_idx": r, "steps": steps,
                      "sample_rate": q, "noise_multiplier": cfg.dp_noise, "clip_norm": cfg.dp_clip,
                      "delta": cfg.dp_delta, "epsilon": eps} for r, steps, q, eps in privacy]
            for row in prows:
                log.event("privacy", **row)
            all_prows = comm.gather(prows, root=0)
            if ctx.rank == 0:
                # one row per round: the client with the largest epsilon (clients differ when their shards do)
                worst = [max(per_round, key=lambda d: d["epsilon"]) for per_round in zip(*all_prows)]
                if cfg.privacy_csv:
                    append_results(worst, cfg.privacy_csv, PRIVACY_COLUMNS)
                last = worst[-1]
                log.info(f"[privacy] {cname}: after round {last['round_idx']} ({last['steps']} steps, q="
                         f"{last['sample_rate']:.4g}, sigma={cfg.dp_noise:g}, C={cfg.dp_clip:g}) epsilon <= "
                         f"{last['epsilon']:.4g} at delta={cfg.dp_delta:g} (Poisson-sampling bound; the training "
                         "loss is not private)" + (
                             "; record-level, the most exposed virtual client's own steps at q = B / n_k: "
                             "amplification by client sampling is ignored, which is conservative" if cohort_dp else ""))
        if cohorts and ctx.rank == 0:
            crows = [{"config": cname, "world_size": ctx.world_size, "round_idx": r,
                      "clients_per_gpu": cfg.clients_per_gpu, "cohort": M, "batch_size": cfg.batch_size,
                      "windows_per_round_per_gpu": M * cfg.batch_size * cfg.local_steps,
                      "clients_rank0": " ".join(str(c) for c in ids)} for r, ids in cohorts]
            if cfg.cohort_csv:
                append_results(crows, cfg.cohort_csv, COHORT_COLUMNS)
            for row in crows:
                log.event("cohort", **row)
        if shapes and ctx.rank == 0:
            for r, sizes, steps, weights in shapes:
                log.event("cohort_shape", config=cname, round_idx=r, partition=cfg.client_partition,
                          client_alpha=cfg.client_alpha, local_epochs=cfg.local_epochs, aggregate=cfg.aggregate,
                          sizes_rank0=sizes, steps_rank0=steps, weights_rank0=weights)
        if client_privacy:
            cprows = [{"config": cname, "world_size": ctx.world_size, "round_idx": r,
                       "sample_rate": M / cfg.clients_per_gpu, "noise_multiplier": cfg.client_dp_noise,
                       "clip_norm": cfg.client_dp_clip, "delta": cfg.client_dp_delta,
                       "epsilon": dp_epsilon(cfg.client_dp_noise, M / cfg.clients_per_gpu, r + 1, cfg.client_dp_delta),
                       "median_client_norm": med, "clipped_share_rank0": clipped}
                      for r, med, clipped in client_privacy]
            if cfg.client_privacy_csv:
                append_results(cprows, cfg.client_privacy_csv, CLIENT_PRIVACY_COLUMNS)
            for row in cprows:
                log.event("client_privacy", **row)
            last = cprows[-1]
            log.info(f"[client-privacy] {cname}: after round {last['round_idx']} (q = M/K = {last['sample_rate']:.4g}, "
                     f"sigma={cfg.client_dp_noise:g}, C={cfg.client_dp_clip:g}, server lr {cfg.server_lr:g}) client-level "
                     f"epsilon <= {last['epsilon']:.4g} at delta={cfg.client_dp_delta:g} (Poisson-subsampling bound "
                     "applied to fixed-size sampling without replacement: an approximation; avg_loss and the evaluation "
                     "metrics are not private)")
        gathered = comm.gather(rows, root=0)
        if ctx.rank == 0:
            flat_rows = [row for rl in gathered for row in rl]
            all_rows.extend(flat_rows)
            if cfg.results_csv:
                append_results(flat_rows, cfg.results_csv, ROUND_COLUMNS)
            summarize(flat_rows, cname, ctx.world_size, log, cohort=M)
        barrier(ctx)
    return all_rows


def summarize(rows: List[Dict], cname: str, world: int, log: RankLogger, cohort: int = 1) -> Dict[str, float]:
    """``cohort``: clients trained per GPU and round - a row's windows are cohort * batch_size * local_steps, or the
    ``B * sum_k S_k`` its ``samples_per_s`` counts when the clients' local steps differ."""
    if not rows:
        return {}
    rounds = sorted({r["round_idx"] for r in rows})
    per_rank = float(np.mean([r["samples_per_s"] for r in rows]))
    node = 0.0
    for ri in rounds:
        rr = [r for r in rows if r["round_idx"] == ri]
        wall = max(r["round_wall_ms"] for r in rr) / 1e3
        # (a row's windows: cohort * batch_size * local_steps, fewer with --local-epochs - samples_per_s counts them)
        node += sum(round(r["samples_per_s"] * r["local_train_ms"] / 1e3) for r in rr) / wall
    node /= len(rounds)
    comm = float(np.mean([r["comm_ms"] for r in rows]))
    local = float(np.mean([r["local_train_ms"] for r in rows]))
    log.info(f"=== {cname} world={world}: per-rank samples/s (ref metric, excl. comm) {per_rank:,.0f} | "
             f"node samples/s (incl. comm) {node:,.0f} | local_ms {local:.3f} comm_ms {comm:.3f} | "
             f"final loss {rows[-1]['avg_loss']:.4f}")
    return {"per_rank_sps": per_rank, "node_sps": node, "comm_ms": comm, "local_ms": local}
