#!/usr/bin/env python3
"""Record (or recompute) the bitwise fixtures of tests/test_tiny_step_valu_gpu.py on one MI355X.

    python scripts/record_tiny_step_r19.py [--tree CHECKOUT] [--out tests/golden/tiny_step_r19]

For every case of ``CASES`` - window length, classes, forced wave count, kind of windows - two ``FusedTinyTrainer``
rounds of 3 steps on the packed dataset read in place (``prepack="direct"``: the MODE 4 step kernel) from seeded
weights, windows and batches, and the per-sample gradient rows of ``ecg_tiny_step_grads`` at the initial weights.  A
case is one ``<name>.npy``: a 1-D uint32 array, the fp32 bits of

    [weights, momentum, summed loss] after round 1, the same after round 2, the gradient rows [B, P + 1]

``--tree``: import the package (and its built kernels) from another checkout, e.g. the commit the fixtures must come
from; the cases and the order of the numbers are this file's either way.  The committed fixtures were recorded with the
build of commit 702e5cb ("Cohort close: one Delta body, one dispatcher, a file of its own"), the parent of the change
that cut the step kernel's vector instructions.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiny_step_r19")
B, N, STEPS, ROUNDS = 3, 12, 3, 2

# (L, nc, waves, kind).  L = 8: the shortest window the kernel takes; 33: a partial last tile across one pair boundary;
# 100: several pairs and an odd tail.  "zeros": windows with a long run of exact zeros and a negative stretch, on
# weights whose conv1 bias is zero and whose conv2 bias is zero on every other channel - exact zero pre-activations of
# both convolutions, and relu' masks of both values next to each other.
CASES = [(L, nc, waves, "randn") for L in (8, 33, 100) for nc in (2, 5) for waves in (8, 16)]
CASES.append((100, 2, 16, "zeros"))


def case_name(L, nc, waves, kind):
    return f"L{L}_nc{nc}_w{waves}_{kind}"


def case_inputs(L, nc, kind):
    """Windows [N, L], labels [N] and the batches [ROUNDS, STEPS, B] of a case (CPU tensors, seeded)."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(1900 + 10 * L + nc + (7 if kind == "zeros" else 0))
    x = torch.randn(N, L, generator=g)
    if kind == "zeros":
        x[:, 15:60] = 0.0
        x[:, 60:] = -x[:, 60:].abs()
        x[::3, 58:62] = -0.0
    y = torch.randint(0, nc, (N,), generator=g)
    idx = torch.stack([torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(STEPS)])
                       for _ in range(ROUNDS)]).to(torch.int32)
    idx[0, 1, 1] = idx[0, 1, 0]  # the same window twice in one batch
    return x, y, idx


def compute_case(L, nc, waves, kind):
    """The case's numbers as one uint32 array (module docstring), computed by the package that is importable now."""
    import torch
    import crossscale_ecg  # noqa: F401
    from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer, labels_int32, tiny_step_grads
    dev = torch.device("cuda:0")
    x, y, idx = case_inputs(L, nc, kind)
    lib = _lib.kernels()
    prev = lib.ecg_tiny_force_waves(waves)
    try:
        torch.manual_seed(19)
        model = TinyECG(num_classes=nc)
        if kind == "zeros":
            with torch.no_grad():
                model.net[0].bias.zero_()
                model.net[2].bias[::2] = 0.0
        model = model.to(dev)
        model.flatten_parameters()
        P = num_params(nc)
        xd, yd = x.to(dev), y.to(dev)
        grads = tiny_step_grads(model.flat.clone(), xd, labels_int32(yd, nc), idx[0, 0].to(dev), B, nc)
        torch.cuda.synchronize()
        parts = []
        tr = FusedTinyTrainer(model, xd, yd, B, STEPS, seed=19, prepack="direct")
        assert tr.prepack == "direct", tr.prepack_fallback
        for r in range(ROUNDS):
            tr.prepare_round(STEPS)
            tr.idx_stage[:STEPS].copy_(idx[r].to(dev))  # the staged table is what the round reads
            tr.launch_round(STEPS)
            torch.cuda.synchronize()
            parts += [tr.params[:P].cpu(), tr.mom[:P].cpu(), tr.loss_acc.cpu()]
        tr.close()
        parts.append(grads[:, :P + 1].cpu().reshape(-1))
    finally:
        lib.ecg_tiny_force_waves(prev)
    return np.concatenate([p.contiguous().numpy().view(np.uint32) for p in parts])


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=ROOT, help="checkout whose package and kernels compute the numbers")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(a.tree))
    os.makedirs(a.out, exist_ok=True)
    for case in CASES:
        arr = compute_case(*case)
        f32 = arr.view(np.float32)
        assert np.isfinite(f32).all(), case
        np.save(os.path.join(a.out, case_name(*case) + ".npy"), arr)
        print(f"{case_name(*case)}: {arr.size} words")
    return 0


if __name__ == "__main__":
    sys.exit(main())
