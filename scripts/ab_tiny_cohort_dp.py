#!/usr/bin/env python3
"""A/B: a cohort round of plain local steps against the same round with record-level DP-SGD in every local step.

One process, one resident synthetic shard, L = 500, bf16, M = 8 clients of B = 32 windows, S = 50 steps per round,
every round one hipGraph replay of a FusedCohortTrainer:
  (a) off   DP-SGD off: fan-out, 50 x (step, cohort reduce), cohort_mean_kernel - the round as it was;
  (b) dp    --dp-clip / --dp-noise on: 50 x (step, dp_row_scale_cohort_kernel over the M * B rows,
            slab_reduce_cohort_dp_sgd_kernel) - one launch more per step - and the same close.
The arms are interleaved, each timed with hipEvents around its replay after warm-up (batch draws stay outside the timed
window); medians and IQRs of the microseconds per round are reported.  ``--only b`` runs the DP arm alone (for a kernel
trace: rocprofv3 --kernel-trace --stats -- python scripts/ab_tiny_cohort_dp.py --only b --reps 5).
Usage: python scripts/ab_tiny_cohort_dp.py [--reps 25] [--out profiles/r24/tiny_cohort_dp_ab.txt]
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
    ap.add_argument("--dp-clip", type=float, default=1.0)
    ap.add_argument("--dp-noise", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="run one arm only: a or b")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "tiny_cohort_dp_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()
    M, B, S = a.cohort, a.batch_size, a.steps

    def trainer(**kw):
        torch.manual_seed(0)
        return FusedCohortTrainer(TinyECG().to(dev), x, y, B, S, clients=a.clients, cohort=M, seed=0,
                                  precision=a.precision, **kw)

    arms = {}
    if a.only in ("", "a"):
        arms["a_off"] = trainer()
    if a.only in ("", "b"):
        arms["b_dp"] = trainer(dp_clip=a.dp_clip, dp_noise=a.dp_noise, dp_seed=1)
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
        f"# tiny_cohort record-level DP-SGD A/B: M={M} clients of B={B}, L={a.win_len} {a.precision} S={S} steps per round (graph "
        f"replays), {a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around the replay of one arm",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  DP-SGD arm: clip {a.dp_clip:g}, "
        f"noise multiplier {a.dp_noise:g}",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {arms[name].avg_loss():12.4f}")
    if len(stats) == 2:
        (ma, a1, a3), (mb, b1, b3) = stats["a_off"], stats["b_dp"]
        lines.append(f"dp - off (b - a) = {mb - ma:+.1f} us per round = {(mb - ma) / S:+.3f} us per step "
                     f"({(mb / ma - 1) * 100:+.2f} %); IQRs [{a1:.1f}, {a3:.1f}] "
                     f"vs [{b1:.1f}, {b3:.1f}] us: {'disjoint' if a3 < b1 or b3 < a1 else 'OVERLAPPING'}")
    if "b_dp" in arms:
        tr = arms["b_dp"]
        lines.append(f"dp arm, last step: {float((tr.dp_scale < 1).float().mean()):.2f} of the {tr.dp_scale.numel()} rows "
                     f"clipped; step word {int(tr.dp_step.item())}")
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
