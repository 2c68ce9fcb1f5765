#!/usr/bin/env python3
"""A/B/C: one cohort round of M virtual clients against the same clients run one after another.

One process, one resident synthetic shard, L = 500, bf16, S = 50 steps per round, every round one hipGraph replay:
  (a) cohort      one FusedCohortTrainer round of M = 8 clients of B = 32 windows (one step and one reduce launch per
                  step for all of them, plus the fan-out and the mean);
  (b) sequential  eight FusedTinyTrainer rounds of B = 32 replayed back to back - what the code without cohorts offers,
                  the baseline;
  (c) full        one FusedTinyTrainer round of B = 256: the same windows per launch as (a), prices the cohort overhead.
The arms are interleaved, each timed with hipEvents around its replays after warm-up (batch draws stay outside the
timed window); medians and IQRs of the microseconds per round are reported.  ``--only a`` runs the cohort arm alone
(for a kernel trace: rocprofv3 --kernel-trace --stats -- python scripts/ab_tiny_cohort.py --only a --reps 5).
Usage: python scripts/ab_tiny_cohort.py [--reps 25] [--out profiles/r11/tiny_cohort_ab.txt]
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
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="run one arm only: a, b or c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "tiny_cohort_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()
    M, B, S = a.cohort, a.batch_size, a.steps

    def model():
        torch.manual_seed(0)
        return TinyECG().to(dev)

    arms = {}
    if a.only in ("", "a"):
        arms["a_cohort"] = [FusedCohortTrainer(model(), x, y, B, S, clients=a.clients, cohort=M, seed=0,
                                               precision=a.precision)]
    if a.only in ("", "b"):
        arms["b_sequential"] = [FusedTinyTrainer(model(), x, y, B, S, seed=c, precision=a.precision) for c in range(M)]
    if a.only in ("", "c"):
        arms["c_full"] = [FusedTinyTrainer(model(), x, y, M * B, S, seed=0, precision=a.precision)]
    for trs in arms.values():
        for tr in trs:
            tr.prepare([S])
    times = {name: [] for name in arms}
    for rep in range(a.warmup + a.reps):
        for name, trs in arms.items():
            for tr in trs:
                tr.prepare_round()  # the batch draws stay outside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for tr in trs:
                tr.launch_round()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    lines = [
        f"# tiny_cohort A/B/C: M={M} clients of B={B}, L={a.win_len} {a.precision} S={S} steps per round (graph replays), "
        f"{a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around the replays of one arm",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  windows per round: {M * B * S} in every arm",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        loss = statistics.mean(tr.avg_loss() for tr in arms[name])
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {loss:12.4f}")
    if len(stats) == 3:
        (ma, a1, a3), (mb, b1, b3), (mc, _, _) = stats["a_cohort"], stats["b_sequential"], stats["c_full"]
        lines.append(f"sequential / cohort (b/a) = {mb / ma:.2f}x; IQRs [{a1:.1f}, {a3:.1f}] vs [{b1:.1f}, {b3:.1f}] us: "
                     f"{'disjoint' if a3 < b1 or b3 < a1 else 'OVERLAPPING'}; cohort {'faster' if ma < mb else 'NOT faster'}")
        lines.append(f"cohort / full-GPU single client (a/c) = {ma / mc:.2f}x ({(ma - mc) / S:+.3f} us per step: M x the "
                     "reduce blocks and per-client operands; the fan-out and the mean add two launches per round)")
    for name in times:
        lines.append(f"raw_us {name:<13} " + " ".join(f"{t:.1f}" for t in times[name]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    for trs in arms.values():
        for tr in trs:
            tr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
