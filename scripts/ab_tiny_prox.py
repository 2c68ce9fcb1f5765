#!/usr/bin/env python3
"""A/B: FedProx (``prox_mu`` = 0.1) against plain local SGD (``prox_mu`` = 0), in the cohort round and in the
single-client round.

One process, one resident synthetic shard, L = 500, bf16, S = 50 steps per round, every round one hipGraph replay:
  cohort   FusedCohortTrainer, M = 8 clients of B = 32 windows: (a) slab_reduce_cohort_sgd_kernel, (b)
           slab_reduce_cohort_prox_sgd_kernel anchored on the global weights (no further launch);
  single   FusedTinyTrainer, B = 256: (a) slab_reduce_sgd_kernel, (b) prox_snapshot_kernel once per round, then
           slab_reduce_prox_sgd_kernel.
Expectation, written before the first run: the prox kernels add one 4-byte load per updating thread, issued before the
slab reads and so under their latency, and a subtract and a multiply-add; the single-client round adds one 5.8 KB
snapshot launch per round.  So no measurable per-step difference is expected - every (b) arm's IQR overlaps its (a)
arm's - and at most a few microseconds per round for the single-client snapshot.
The arms are interleaved, each timed with hipEvents around its replay after warm-up (batch draws stay outside the timed
window); medians and IQRs of the microseconds per round are reported whether the expectation held or not.
Usage: python scripts/ab_tiny_prox.py [--reps 25] [--out profiles/r17/tiny_prox_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import crossscale_ecg  # noqa: E402,F401
from crossscale_ecg.models.tiny_ecg import TinyECG  # noqa: E402
from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer  # noqa: E402
from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer  # noqa: E402


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20480)
    ap.add_argument("--win-len", type=int, default=500)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--cohort", type=int, default=8)
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--single-batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--prox-mu", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "tiny_prox_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()
    M, B, S = a.cohort, a.batch_size, a.steps

    def cohort(mu):
        torch.manual_seed(0)
        return FusedCohortTrainer(TinyECG().to(dev), x, y, B, S, clients=a.clients, cohort=M, seed=0,
                                  precision=a.precision, prox_mu=mu)

    def single(mu):
        torch.manual_seed(0)
        return FusedTinyTrainer(TinyECG().to(dev), x, y, a.single_batch_size, S, seed=0, precision=a.precision,
                                prox_mu=mu)

    arms = {"cohort_a_mu0": cohort(0.0), "cohort_b_prox": cohort(a.prox_mu),
            "single_a_mu0": single(0.0), "single_b_prox": single(a.prox_mu)}
    for tr in arms.values():
        tr.prepare([S])
    times = {name: [] for name in arms}
    for rep in range(a.warmup + a.reps):
        for name, tr in arms.items():
            tr.prepare_round()  # the batch draws stay outside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.launch_round()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    lines = [
        f"# tiny FedProx A/B: prox_mu 0 vs {a.prox_mu:g}; cohort M={M} clients of B={B}, single client B={a.single_batch_size}; "
        f"L={a.win_len} {a.precision} S={S} steps per round (graph replays), {a.reps} interleaved repetitions after "
        f"{a.warmup} warm-up, hipEvent times around the replay of one arm",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}",
        "# expectation (written before the run): no measurable per-step difference - every prox arm's IQR overlaps its "
        "baseline's - and at most a few us per round for the single-client snapshot launch",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {arms[name].avg_loss():12.4f}")
    held = True
    for base, prox in (("cohort_a_mu0", "cohort_b_prox"), ("single_a_mu0", "single_b_prox")):
        (ma, a1, a3), (mb, b1, b3) = stats[base], stats[prox]
        overlap = not (a3 < b1 or b3 < a1)
        held &= overlap
        lines.append(f"{prox} - {base} = {mb - ma:+.1f} us per round ({(mb - ma) / S * 1e3:+.1f} ns per step, "
                     f"{(mb / ma - 1) * 100:+.2f} %); IQRs [{a1:.1f}, {a3:.1f}] vs [{b1:.1f}, {b3:.1f}] us: "
                     f"{'overlapping' if overlap else 'DISJOINT'}")
    lines.append("expectation (every prox arm's IQR overlaps its baseline's): " + ("held" if held else "did NOT hold"))
    for name in times:
        lines.append(f"raw_us {name:<13} " + " ".join(f"{t:.1f}" for t in times[name]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    for tr in arms.values():
        tr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
