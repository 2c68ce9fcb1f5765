#!/usr/bin/env python3
"""FedAvg ECG training entry point (API/CLI-compatible with the reference
Module_3/TRUE_FL_M3/part3_fedavg_overlap_mpi_gpu.py).

Launch one process per MI355X (RCCL over xGMI):
    torchrun --standalone --nproc-per-node 8 part3_fedavg_overlap_mpi_gpu.py --data-root data/shards \
        --batch-size 256 --rounds 5 --local-steps 50 --config both --max-windows 20000
``mpiexec -n 8`` / ``srun`` also work (launcher env shim).  On a CPU box the same command runs with gloo.
New flags: --kernel-backend {auto,fused,torch} --amp-dtype {bf16,fp16,none} --overlap {none,tail,delayed}
--sync {fedavg,none,ddp} --no-bcast-every-round --ckpt-every N --resume --drop-prob p
--synthetic-windows N --labels {zeros,parity} --config-file cfg.yaml
--eval-every R --eval-windows H --eval-csv path (per-round loss / accuracy / confusion of the averaged model on
each client's held-out last H windows)
--dp-clip C --dp-noise sigma --dp-delta delta --privacy-csv path (DP-SGD local steps: per-sample clip + Gaussian
noise; cumulative epsilon per round, Poisson-subsampling bound; the reported training loss is not private)
--clients-per-gpu K --cohort M --cohort-csv path (client sampling: K virtual clients per GPU, M of them drawn per
round and trained side by side from the global weights; TinyECG on the fused or torch backend)
--client-dp-clip C --client-dp-noise sigma --client-dp-delta delta --server-lr eta --client-privacy-csv path (client-level
DP on a cohort round, needs --clients-per-gpu: each client's round delta clipped to l2 norm C, Gaussian noise on the
mean, server step size eta; cumulative client-level epsilon per round at sample rate M / K, the Poisson-subsampling
bound as an approximation; avg_loss and the evaluation metrics are not private)
--server-opt {none,sgdm,adagrad,adam,yogi} --server-beta1 b1 --server-beta2 b2 --server-tau tau (server optimizer on a
cohort round's averaged client delta with step size --server-lr, needs --clients-per-gpu: FedAvgM, FedAdagrad, FedAdam,
FedYogi; state kept in the per-rank checkpoint; the three adaptive ones under --sync fedavg on more than one rank only
with --server-scope global)
--server-scope {rank,global} (global, needs --clients-per-gpu: the ranks' cohort deltas are all-reduced in place of
their weights and every rank takes one replicated server step on the average - a global server optimizer)
--prox-mu mu (FedProx: every local step's gradient gains mu * (w - the weights the round started from); TinyECG on the
fused backend, with or without --clients-per-gpu, any model on the torch backend; not with --dp-clip, --sync ddp, fp16
AMP or --overlap delayed)
--client-partition {contiguous,shards} --client-shards s (needs --clients-per-gpu: "shards" deals every virtual client s
runs of the GPU's label-sorted training windows - label-skewed, non-IID clients - instead of a contiguous slice)
--client-partition dirichlet --client-alpha a --local-epochs E --aggregate {mean,weighted,nova} (need --clients-per-gpu:
virtual clients of unequal sizes by the label-Dirichlet split, min(local steps, E passes over its own windows) local
steps per client, and the cohort's deltas averaged with n_k / n or with FedNova's normalised weights; not with
--client-dp-clip, nova not with --prox-mu)
--aggregate {trimmed,median} --trim-frac f --flip-clients F (need --clients-per-gpu: robust aggregation - per parameter
the floor(f * M) smallest and largest of the cohort's M <= 64 deltas are dropped and the rest averaged, f in (0, 0.5)
without a default, or the coordinate-wise median; F > 0 mirrors the training labels of virtual clients 0..F-1, the
poisoned clients to be robust against; not with --client-dp-clip)
"""
from __future__ import annotations

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import crossscale_ecg  # noqa: E402,F401
from crossscale_ecg.config import FedAvgConfig, add_dataclass_args, from_args  # noqa: E402
from crossscale_ecg.parallel.env import init_distributed, shutdown_distributed, setup_device  # noqa: E402,F401
from crossscale_ecg.parallel.fedavg import broadcast_model, fedavg_allreduce, Communicator  # noqa: E402,F401
from crossscale_ecg.train.steps import train_step_G0, train_step_G1  # noqa: E402,F401
from crossscale_ecg.train.fedavg import run_fedavg, set_basic_seeds  # noqa: E402,F401
from crossscale_ecg.utils.csvio import append_results, RoundStats  # noqa: E402,F401


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    add_dataclass_args(ap, FedAvgConfig)
    ap.add_argument("--config-file", dest="config_file", default=None, help="YAML overrides")
    return ap


def main(argv=None):
    ns = build_parser().parse_args(argv)
    cfg = from_args(FedAvgConfig, ns)
    if cfg.config not in ("G0", "G1", "both"):
        raise SystemExit("--config must be G0, G1 or both")
    ctx = init_distributed()
    try:
        return run_fedavg(cfg, ctx)
    finally:
        shutdown_distributed()


if __name__ == "__main__":
    main()
