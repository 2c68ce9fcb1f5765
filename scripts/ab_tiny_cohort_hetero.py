#!/usr/bin/env python3
"""A/B: a cohort round of equal clients and a plain mean against the same round with per-client step counts and a
weighted close.

One process, one resident synthetic shard, L = 500, bf16, M = 8 clients of B = 32 windows, S = 50 steps per round,
every round one hipGraph replay of a FusedCohortTrainer:
  (a) mean      the round of before: fan-out, 50 x (step, slab_reduce_cohort_sgd_kernel), cohort_mean_kernel (the
                machine code of these kernels is the parent commit's: profiles/r20/diff_device_asm.txt);
  (b) weighted  ``aggregate="weighted"`` on equal clients: every client active in every step, the reduce in its STEPS
                form (slab_reduce_cohort_steps_sgd_kernel, client_steps[c] = S), the close cohort_delta_wscale_kernel +
                cohort_dp_mean_kernel with weights 1 / 8;
  (c) dirichlet (information) ``partition="dirichlet"`` alpha 0.5, ``local_epochs=1``, weighted: clients frozen once
                their steps are done; the launches are those of (b).
Expected from the code, not measured: the STEPS reduce adds one scalar load of a pointer past the preloaded arguments
and one of client_steps[client] per block, which the FedProx item saw as a cost in the single-client reduce and not in
the cohort one; the close is two launches in place of one, as for every server step (the client-DP item measured that
at about 1 us per round).  So (b) - (a) is expected within the arms' IQRs, at most a few us per 50-step round.  (c)
skips the loads and stores of frozen clients' reduce blocks and is expected no slower than (b).  The arms are
interleaved, each timed with hipEvents around its replay after warm-up (batch draws stay outside the timed window);
medians and IQRs of the microseconds per round are reported, and the result is stated either way.
Usage: python scripts/ab_tiny_cohort_hetero.py [--reps 25] [--out profiles/r20/tiny_cohort_hetero_ab.txt]
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
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "tiny_cohort_hetero_ab.txt"))
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

    arms = {"a_mean": trainer(),
            "b_weighted": trainer(aggregate="weighted"),
            "c_dirichlet": trainer(aggregate="weighted", partition="dirichlet", dirichlet_alpha=0.5, local_epochs=1)}
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
        f"# tiny_cohort unequal-clients A/B: M={M} clients of B={B}, L={a.win_len} {a.precision} S={S} steps per round "
        f"(graph replays), {a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around the replay of "
        "one arm",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  c_dirichlet's last round: steps "
        f"{arms['c_dirichlet'].last_round_shape()[1]} of sizes {arms['c_dirichlet'].last_round_shape()[0]}",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {arms[name].avg_loss():12.4f}")
    ma, a1, a3 = stats["a_mean"]
    held = True
    for name in ("b_weighted", "c_dirichlet"):
        mb, b1, b3 = stats[name]
        overlap = not (a3 < b1 or b3 < a1)
        held &= overlap or name != "b_weighted"
        lines.append(f"{name} - a_mean = {mb - ma:+.1f} us per round ({(mb / ma - 1) * 100:+.2f} %); IQRs [{a1:.1f}, {a3:.1f}] "
                     f"vs [{b1:.1f}, {b3:.1f}] us: {'overlapping' if overlap else 'DISJOINT'}")
    lines.append("expectation (b_weighted - a_mean within the IQRs: the two IQRs overlap): "
                 + ("held" if held else "did NOT hold"))
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
