#!/usr/bin/env python3
"""A/B: a cohort round with a server optimizer stepped inside the round graph (scope "rank") against the same round
split at the delta and stepped by a launch of its own (scope "global"), on one rank.

One process, one resident synthetic shard, L = 500, bf16, M = 8 clients of B = 32 windows, S = 50 steps per round, adam:
  (a) rank    one hipGraph replay: fan-out, 50 x (step, reduce), cohort_delta_scale_kernel + cohort_server_opt_kernel<adam>;
  (b) global  the graph replay ends with cohort_delta_scale_kernel + cohort_delta_kernel, then ecg_server_opt_step
              enqueues server_step_kernel<adam> behind it (what a driver does after its all-reduce of the deltas; here
              nothing is reduced, so both arms compute the same bits).
Arm (b) has one more launch boundary and sends the 5.8 KB delta through memory once more per round: a few microseconds
on a round of about 510 us are expected - written down before the run as 0 to 10 us.  The arms are interleaved, each
timed with hipEvents around its launches after warm-up (batch draws stay outside the timed window); medians and IQRs
of the microseconds per round are reported, and the two arms' weights are compared at the end.
Usage: python scripts/ab_tiny_cohort_global_server.py [--reps 25] [--out profiles/r16/tiny_cohort_global_server_ab.txt]
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

EXPECT_US = (0.0, 10.0)  # the extra cost of arm (b) expected from the code, per round


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
    ap.add_argument("--server-lr", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "tiny_cohort_global_server_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()
    M, B, S = a.cohort, a.batch_size, a.steps

    def trainer(**kw):
        torch.manual_seed(0)
        return FusedCohortTrainer(TinyECG().to(dev), x, y, B, S, clients=a.clients, cohort=M, seed=0,
                                  precision=a.precision, server_lr=a.server_lr, server_opt="adam", **kw)

    arms = {"a_rank": trainer(), "b_global": trainer(server_scope="global")}
    for tr in arms.values():
        tr.prepare([S])
    times = {name: [] for name in arms}
    for rep in range(a.warmup + a.reps):
        for name, tr in arms.items():
            tr.prepare_round()  # the batch draws stay outside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.launch_round()
            if tr.server_delta is not None:
                tr.apply_server_step()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    same = all(torch.equal(u, v) for u, v in zip(*((tr.params, tr.server_m, tr.server_v) for tr in arms.values())))
    lines = [
        f"# tiny_cohort global-server A/B: M={M} clients of B={B}, L={a.win_len} {a.precision} S={S} steps per round, adam, "
        f"{a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around one arm's launches (a: one graph "
        "replay; b: the graph replay plus the server step launch)",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  server lr {a.server_lr:g}, beta1 0.9, beta2 0.99, "
        "tau 1e-3, no client DP, one rank, no collective",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {arms[name].avg_loss():12.4f}")
    (ma, a1, a3), (mb, b1, b3) = stats["a_rank"], stats["b_global"]
    overlap = not (a3 < b1 or b3 < a1)
    lines.append(f"b_global - a_rank = {mb - ma:+.1f} us per round ({(mb / ma - 1) * 100:+.2f} %); IQRs [{a1:.1f}, {a3:.1f}] vs "
                 f"[{b1:.1f}, {b3:.1f}] us: {'overlapping' if overlap else 'DISJOINT'}")
    held = EXPECT_US[0] <= mb - ma <= EXPECT_US[1]
    lines.append(f"expectation (one more launch boundary and a 5.8 KB round trip: {EXPECT_US[0]:g} to {EXPECT_US[1]:g} us per "
                 f"round): {'held' if held else 'did NOT hold'}")
    lines.append(f"weights, m and v of the two arms after {a.warmup + a.reps} rounds: "
                 + ("bit-identical" if same else "DIFFERENT"))
    lines.append("multi-GPU RCCL runs (the all-reduce of the deltas between the two halves): not measured")
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
