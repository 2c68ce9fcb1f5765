#!/usr/bin/env python3
"""A/B: a cohort round with the two-launch server-step close against the same round with a robust close.

One process, one resident synthetic shard, L = 500, bf16, M clients of B windows, S = 50 steps per round, every round
one hipGraph replay of a FusedCohortTrainer; two set-ups, M = 8 / B = 32 (eight parameters per wave in the selection)
and M = 64 / B = 4 (one parameter per wave):
  (a) server_lr   ``server_lr=0.9`` alone: cohort_delta_scale_kernel + cohort_dp_mean_kernel, the parent commit's close
                  (machine code unchanged: profiles/r21/diff_device_asm.txt);
  (b) trimmed     ``robust="trimmed"`` with k = 1 and the same server_lr: cohort_delta_scale_kernel,
                  cohort_robust_delta_kernel into the scratch buffer, server_step_kernel<256, 0>;
  (c) median      ``robust="median"``, k = (M - 1) // 2: the launches of (b).
Expected from the code, not measured: (b) and (c) add one launch boundary and one round trip of Delta (P floats, 5.8 KB)
through the scratch buffer, which the scope-"global" item saw as a few microseconds; the selection itself reads the
M * P client values once, like cohort_dp_mean_kernel, and its two M-iteration cross-lane loops run on 1458 * W lanes in
all - nothing against 50 steps.  So (b) - (a) and (c) - (a) are expected between 0 and 10 us per round, and (c) - (b)
within the IQRs (k is a scalar, the loops do not depend on it).  At M = 64 the selection has one parameter per wave and
64-iteration loops; the same expectation is stated for it, with less confidence.  The arms are interleaved, each timed
with hipEvents around its replay after warm-up (batch draws stay outside the timed window); medians and IQRs of the
microseconds per round are reported, and the result is stated either way.
Usage: python scripts/ab_tiny_cohort_robust.py [--reps 25] [--out profiles/r21/tiny_cohort_robust_ab.txt]
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

EXPECT_LO, EXPECT_HI = 0.0, 10.0  # us per round on top of (a), written down before the run


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[0], q[2]


def run_setup(a, dev, M, B, lines):
    S = a.steps
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()

    def trainer(**kw):
        torch.manual_seed(0)
        return FusedCohortTrainer(TinyECG().to(dev), x, y, B, S, clients=max(a.clients, M), cohort=M, seed=0,
                                  precision=a.precision, server_lr=0.9, **kw)

    arms = {"a_server_lr": trainer(), "b_trimmed": trainer(robust="trimmed", trim_frac=1.5 / M),
            "c_median": trainer(robust="median")}
    assert arms["b_trimmed"].trim == 1 and arms["c_median"].trim == (M - 1) // 2
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
    lines += [
        f"# tiny_cohort robust-close A/B: M={M} clients of B={B}, L={a.win_len} {a.precision} S={S} steps per round (graph "
        f"replays), {a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around the replay of one arm",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  k: trimmed 1, median {(M - 1) // 2}",
        "arm            median_us_per_round   q1_us      q3_us      iqr_us    min_us     max_us   us_per_step   final_loss",
    ]
    stats = {}
    for name, t in times.items():
        m, q1, q3 = quartiles(t)
        stats[name] = (m, q1, q3)
        lines.append(f"{name:<14} {m:19.1f} {q1:10.1f} {q3:10.1f} {q3 - q1:9.1f} {min(t):9.1f} {max(t):10.1f} "
                     f"{m / S:13.3f} {arms[name].avg_loss():12.4f}")
    ma, a1, a3 = stats["a_server_lr"]
    held = True
    for name in ("b_trimmed", "c_median"):
        mb, b1, b3 = stats[name]
        ok = EXPECT_LO <= mb - ma <= EXPECT_HI or not (a3 < b1 or b3 < a1)
        held &= ok
        lines.append(f"M={M} {name} - a_server_lr = {mb - ma:+.1f} us per round ({(mb / ma - 1) * 100:+.2f} %); IQRs "
                     f"[{a1:.1f}, {a3:.1f}] vs [{b1:.1f}, {b3:.1f}] us")
    lines.append(f"M={M} expectation ({EXPECT_LO:g} to {EXPECT_HI:g} us per round on top of (a), or overlapping IQRs): "
                 + ("held" if held else "did NOT hold"))
    for name in times:
        lines.append(f"raw_us M={M} {name:<13} " + " ".join(f"{t:.1f}" for t in times[name]))
    for tr in arms.values():
        tr.close()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20480)
    ap.add_argument("--win-len", type=int, default=500)
    ap.add_argument("--clients", type=int, default=64)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "tiny_cohort_robust_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    lines = []
    for M, B in ((8, 32), (64, 4)):
        run_setup(a, dev, M, B, lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
