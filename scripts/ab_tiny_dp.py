#!/usr/bin/env python3
"""A/B: a FusedTinyTrainer round with and without DP-SGD (per-sample clip + Gaussian noise on the reduce side).

One process, one resident synthetic shard; two trainers on copies of the same model, B = 256, L = 500, bf16, K = 50
steps per round (one hipGraph replay each).  DP adds one launch per step (the clip-factor pass, a second read of the
~1.5 MB slab) and the clipped, noised twin of the reduce.  (a) plain and (b) DP rounds are interleaved, each timed
with hipEvents after warm-up; medians and IQRs of the microseconds per step are reported.
Usage: python scripts/ab_tiny_dp.py [--reps 40] [--out profiles/r8/tiny_dp_ab.txt]
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
from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer  # noqa: E402


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[2] - q[0]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=20000)
    ap.add_argument("--win-len", type=int, default=500)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--dp-clip", type=float, default=1.0)
    ap.add_argument("--dp-noise", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "tiny_dp_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((a.windows, a.win_len), generator=g, device=dev)
    y = (x.mean(1) > 0).long()
    trainers = {}
    for name, kw in (("a_plain", {}), ("b_dp", dict(dp_clip=a.dp_clip, dp_noise=a.dp_noise))):
        torch.manual_seed(0)
        tr = FusedTinyTrainer(TinyECG().to(dev), x, y, a.batch_size, a.steps, seed=0, precision=a.precision, **kw)
        tr.prepare([a.steps])
        trainers[name] = tr
    times = {name: [] for name in trainers}
    for rep in range(a.warmup + a.reps):
        for name, tr in trainers.items():
            tr.prepare_round()  # the batch draw stays outside the timed window
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.launch_round()
            e1.record()
            e1.synchronize()
            if rep >= a.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.steps)
    dp = trainers["b_dp"]
    clipped = int((dp.dp_scale < 1).sum())
    (ma, ia), (mb, ib) = quartiles(times["a_plain"]), quartiles(times["b_dp"])
    lines = [
        f"# tiny_dp A/B: B={a.batch_size} L={a.win_len} {a.precision} K={a.steps} steps per round (one graph replay), "
        f"{a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times around the replay",
        f"# GPU {torch.cuda.get_device_name(0)}  torch {torch.__version__}  dp_clip={a.dp_clip:g} dp_noise={a.dp_noise:g} "
        f"(last step: {clipped}/{a.batch_size} rows clipped; {dp.dp_steps} DP steps, device counter {int(dp.dp_step.item())})",
        "variant    median_us_per_step   iqr_us   min_us   max_us   final_loss",
    ]
    for name, m, i in (("a_plain", ma, ia), ("b_dp", mb, ib)):
        t = times[name]
        lines.append(f"{name:<10} {m:18.3f} {i:8.3f} {min(t):8.3f} {max(t):8.3f} {trainers[name].avg_loss():12.4f}")
    lines.append(f"DP - plain median = {mb - ma:+.3f} us/step ({(mb / ma - 1) * 100:+.1f} %); expected from the code: one "
                 "launch boundary (~1.5 us) plus a second read of the slab")
    for name in trainers:
        lines.append(f"raw_us {name:<8} " + " ".join(f"{t:.3f}" for t in times[name]))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    for tr in trainers.values():
        tr.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
