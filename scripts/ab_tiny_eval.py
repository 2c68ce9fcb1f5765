#!/usr/bin/env python3
"""A/B: the fused TinyECG evaluation kernel vs what the training step's forward kernel offers for the same result.

One process, one resident synthetic shard of 262,144 windows x 500 fp32 (512 MiB: larger than the Infinity Cache,
so every repetition streams the shard from HBM).
  (a) fused:    ops.tiny_eval.tiny_evaluate (one persistent launch + finalize; no pred / logits written)
  (b) baseline: tiny_forward(flat, x, None, N) -> F.cross_entropy(reduction="sum"), argmax, bincount confusion
(a) and (b) are interleaved, each repetition timed with hipEvents after warm-up; medians and IQRs are reported with
windows/s, the effective GB/s of the window stream and its share of the HBM peak.
Usage: python scripts/ab_tiny_eval.py [--reps 25] [--out profiles/r7/tiny_eval_ab.txt]
"""
from __future__ import annotations

import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import crossscale_ecg  # noqa: E402,F401
from crossscale_ecg.models.tiny_ecg import TinyECG  # noqa: E402
from crossscale_ecg.ops.fused_tiny import tiny_forward  # noqa: E402
from crossscale_ecg.ops.tiny_eval import TinyEvaluator, tiny_evaluate  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak


def gpu_serial() -> str:
    try:
        txt = subprocess.run(["rocm-smi", "--showserial"], capture_output=True, text=True, timeout=30).stdout
        m = re.search(r"Serial Number:\s*(\S+)", txt)
        if m:
            return m.group(1)
    except Exception:
        pass
    return "unknown"


def quartiles(v):
    q = statistics.quantiles(v, n=4)
    return statistics.median(v), q[2] - q[0]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=262144)
    ap.add_argument("--win-len", type=int, default=500)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "tiny_eval_ab.txt"))
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    N, L, nc = a.windows, a.win_len, a.classes
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, L), generator=g, device=dev)
    x.mul_(0.25 + 2.75 * torch.rand((N, 1), generator=g, device=dev))
    y = torch.randint(0, nc, (N,), generator=g, device=dev)
    y32 = y.to(torch.int32)
    torch.manual_seed(0)
    model = TinyECG(nc).to(dev)
    with torch.no_grad():
        model.head.weight.mul_(8)
    flat = model.flatten_parameters()
    ev = TinyEvaluator(dev, nc)

    def fused():
        return tiny_evaluate(flat, x, y32, None, nc, evaluator=ev)

    def baseline():
        logits = tiny_forward(flat, x, None, N, nc)
        loss = F.cross_entropy(logits, y, reduction="sum")
        pred = logits.argmax(1)
        conf = torch.bincount(y * nc + pred, minlength=nc * nc)
        return loss, (pred == y).sum(), conf

    for _ in range(a.warmup):
        ra, rb = fused(), baseline()
    torch.cuda.synchronize()
    same = (ra.correct == int(rb[1]), torch.equal(ra.confusion.reshape(-1), rb[2].cpu()),
            abs(ra.loss_sum - float(rb[0])) / abs(float(rb[0])))
    ta, tb = [], []
    for _ in range(a.reps):
        for fn, acc in ((fused, ta), (baseline, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            acc.append(e0.elapsed_time(e1))
    (ma, ia), (mb, ib) = quartiles(ta), quartiles(tb)
    gb = N * L * 4 / 1e9
    lines = [
        f"# tiny_eval A/B: {N} windows x {L} fp32 ({N * L * 4 / 2**20:.0f} MiB resident), {nc} classes, "
        f"{a.reps} interleaved repetitions after {a.warmup} warm-up, hipEvent times",
        f"# GPU {torch.cuda.get_device_name(0)} serial {gpu_serial()}  torch {torch.__version__}",
        f"# same result: correct equal {same[0]}, confusion equal {same[1]}, loss_sum rel diff {same[2]:.2e} "
        f"(accuracy {ra.accuracy:.4f})",
        "variant      median_ms   iqr_ms   windows_per_s   eff_GB_per_s   share_of_HBM_peak",
    ]
    for name, m, i in (("a_fused", ma, ia), ("b_baseline", mb, ib)):
        lines.append(f"{name:<12} {m:9.4f} {i:8.4f} {N / (m / 1e3):15,.0f} {gb / (m / 1e3):14.1f} "
                     f"{gb / (m / 1e3) / HBM_PEAK_GBS:18.3f}")
    lines.append(f"fused / baseline median = {ma / mb:.3f} ({(1 - ma / mb) * 100:.1f} % lower; pass bar: > 10 % lower)"
                 f" -> {'PASS' if ma < 0.9 * mb else 'FAIL'}")
    lines.append("raw_ms a_fused    " + " ".join(f"{t:.4f}" for t in ta))
    lines.append("raw_ms b_baseline " + " ".join(f"{t:.4f}" for t in tb))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0


if __name__ == "__main__":
    sys.exit(main())
