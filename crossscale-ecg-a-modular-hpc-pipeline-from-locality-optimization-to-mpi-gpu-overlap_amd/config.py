"""Workload configuration: one dataclass per workload, populated from argparse with the reference's flag
names and defaults, plus the MI355X flags.  ``--config file.yaml`` overrides defaults
(yaml.safe_load only)."""
from __future__ import annotations

import argparse
from dataclasses import dataclass, field, fields
from typing import List, Optional


@dataclass
class FedAvgConfig:
    # ---- reference flags (TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py:140-147) ----
    data_root: Optional[str] = None
    batch_size: int = 256
    rounds: int = 10
    local_steps: int = 50
    max_windows: int = 30000
    config: str = "both"  # G0 | G1 | both
    # ---- MI355X additions ----
    kernel_backend: str = "auto"  # auto | fused | hip | torch  (hip = MFMA conv kernels for ResNet1D)
    amp_dtype: str = "bf16"  # bf16 | fp16 | none  (dtype of the G1 configuration)
    overlap: str = "none"  # none | tail (exact, ResNet engine) | delayed (stale-by-one)
    sync: str = "fedavg"  # fedavg | none | ddp
    bcast_every_round: bool = True  # the reference broadcasts every round; RCCL AVG makes it redundant
    synthetic_windows: int = 0  # >0: skip shards, generate N(0,1) windows on device
    labels: str = "zeros"  # zeros (reference) | parity (learnable)
    win_len: int = 500
    lr: float = 1e-2
    momentum: float = 0.9
    seed: int = 1234
    drop_prob: float = 0.0  # FL client dropout injection (weighted FedAvg, zero-weight skip)
    # latency injection: host sleep inside each round's weight-independent batch preparation (the work that
    # --overlap tail places under the in-flight all-reduce); lets the overlap tests prove exposure < comm
    inject_prep_delay_ms: float = 0.0
    bucket_mb: float = 4.0  # ResNet1D tail / DDP gradient-bucket size (~1-4 MB per collective)
    ckpt_every: int = 0
    ckpt_dir: str = "checkpoints"
    resume: bool = False
    # evaluation (off by default): after every eval_every-th round each client evaluates the weights a checkpoint
    # of that round would hold on its last eval_windows windows, which are held out of training (0: on its
    # training windows); rank 0 appends the summed record to eval_csv
    eval_every: int = 0
    eval_windows: int = 0
    eval_csv: str = "results/fedavg_eval.csv"
    # DP-SGD (off by default; TinyECG on the fused or torch backend): per-sample l2 clip norm C, noise multiplier
    # sigma (noise std = sigma * C on the summed clipped gradients) and the delta of the reported epsilon; with
    # dp_clip > 0 rank 0 appends every client's cumulative epsilon per round to privacy_csv
    dp_clip: float = 0.0
    dp_noise: float = 0.0
    dp_delta: float = 1e-5
    privacy_csv: str = "results/fedavg_privacy.csv"
    # client sampling (off by default; TinyECG on the fused or torch backend): every GPU holds clients_per_gpu virtual
    # clients (contiguous partitions of its training windows); each round a cohort of them (0: all) is drawn, trains
    # from the global weights with batches of batch_size, and their mean is this GPU's contribution to FedAvg; rank 0
    # appends the cohort's shape per round to cohort_csv
    clients_per_gpu: int = 1
    cohort: int = 0
    cohort_csv: str = "results/fedavg_cohort.csv"
    # client-level DP on a cohort round (off by default; needs clients_per_gpu > 1): every client's round delta is
    # clipped to l2 norm client_dp_clip, the clipped deltas are averaged, Gaussian noise with multiplier client_dp_noise
    # is added and the result is applied with the server step size server_lr (usable without a clip); with a clip rank 0
    # appends the cumulative client-level epsilon at client_dp_delta per round to client_privacy_csv
    client_dp_clip: float = 0.0
    client_dp_noise: float = 0.0
    client_dp_delta: float = 1e-5
    server_lr: float = 1.0
    client_privacy_csv: str = "results/fedavg_client_privacy.csv"
    # server optimizer on a cohort round's averaged (clipped, noised) client delta (none | sgdm | adagrad | adam | yogi;
    # needs clients_per_gpu > 1; train/server_opt.py states the rules): momentum / first-moment and second-moment
    # decay, and the adaptivity floor tau of adagrad, adam and yogi; server_lr is its step size
    server_opt: str = "none"
    server_beta1: float = 0.9
    server_beta2: float = 0.99
    server_tau: float = 1e-3
    # where the server step of a cohort round is taken (rank | global; global needs clients_per_gpu > 1): "rank" inside
    # every rank's round on that rank's delta, the driver then averaging the stepped weights; "global" after an
    # all-reduce of the ranks' deltas, one replicated step on every rank (what adagrad, adam and yogi need under
    # sync fedavg on more than one rank)
    server_scope: str = "rank"
    # FedProx (off by default; TinyECG on the fused backend with or without client sampling, any model on the torch
    # backend): every local step's gradient gains prox_mu * (w - the weights the round started from)
    prox_mu: float = 0.0
    # how a GPU's training windows are dealt to its virtual clients (needs clients_per_gpu > 1): contiguous slices, or
    # "shards" - client_shards runs of the label-sorted windows per client (label-skewed, non-IID clients)
    # "dirichlet" - the label-Dirichlet split with concentration client_alpha (> 0, no default): clients of unequal
    # sizes and label mixes
    client_partition: str = "contiguous"
    client_shards: int = 2
    client_alpha: float = 0.0
    # unequal local work and the aggregate of a cohort round (need clients_per_gpu > 1): local_epochs E > 0 - a virtual
    # client of n_k windows runs min(local_steps, max(1, E * (n_k // batch_size))) local steps (0: local_steps each);
    # aggregate mean | weighted (n_k / n over the cohort) | nova (FedNova's normalised averaging)
    local_epochs: int = 0
    aggregate: str = "mean"
    # robust aggregates (need clients_per_gpu > 1): aggregate trimmed - the coordinate-wise mean of a cohort's deltas
    # without the floor(trim_frac * M) smallest and largest (trim_frac in (0, 0.5), no default: 0 is "not given") - or
    # median; flip_clients F > 0 mirrors the training labels of virtual clients 0..F-1 (poisoned clients)
    trim_frac: float = 0.0
    flip_clients: int = 0
    results_csv: str = "results/fedavg_results.csv"
    jsonl: Optional[str] = None
    model: str = "tiny_ecg"
    num_classes: int = 2
    quiet: bool = False


@dataclass
class PseudoFLConfig:
    # ---- reference flags (Module_3/part3_mpi_gpu_train.py:424-430) ----
    batch_size: int = 256
    steps: int = 200
    max_windows: int = 20000
    data_root: Optional[str] = None
    # ---- MI355X additions ----
    kernel_backend: str = "auto"
    amp_dtype: str = "bf16"
    loader: str = "gpu"  # gpu (GPU-resident shards, reference active path) | stream (pinned + copy-stream H2D)
    synthetic_windows: int = 0
    win_len: int = 500
    seed: int = 1234
    results_csv: str = "results/part3_mpi_cuda_results.csv"
    quiet: bool = False


def add_dataclass_args(ap: argparse.ArgumentParser, cls, skip: List[str] = ()) -> None:
    for f in fields(cls):
        if f.name in skip:
            continue
        flag = "--" + f.name.replace("_", "-")
        default = f.default
        if f.type in ("bool", bool):
            ap.add_argument(flag, action=argparse.BooleanOptionalAction, default=default)
        else:
            typ = {"int": int, "float": float, "str": str}.get(str(f.type).replace("Optional[", "").rstrip("]"), str)
            ap.add_argument(flag, type=typ, default=default)


def from_args(cls, ns: argparse.Namespace):
    kw = {f.name: getattr(ns, f.name) for f in fields(cls) if hasattr(ns, f.name)}
    cfg = cls(**kw)
    path = getattr(ns, "config_file", None)
    if path:
        import yaml
        with open(path) as fh:
            over = yaml.safe_load(fh) or {}
        for k, v in over.items():
            if hasattr(cfg, k):
                setattr(cfg, k, v)
    return cfg
