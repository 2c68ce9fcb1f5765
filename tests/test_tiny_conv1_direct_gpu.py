"""The bf16 fused TinyECG kernels build their conv1 operand from bounded loads of the window row in global memory
(no LDS copy of the window).  Window lengths at which the row bounds and the 16-step tiles / 32-step pairs meet:
L = 8 (every window touches both row ends), 29 / 32 / 33 around the end of the first pair, 63 / 100 around later
ones, 300 (8 waves with a second pair per wave: the in-loop loads).  Rows are addressed directly (idx=None) and
through a shuffled idx into a dataset whose unselected rows hold huge values, so a read outside a row shows.

Inputs.  The gradients are compared with fp32 autograd under the bound of tests/test_fused_tiny_gpu.py (per-tensor
relative error < 3e-2), but at B = 3 instead of that file's B = 64.  A 3-sample gradient is a short, cancelling sum,
and for most random draws bf16 arithmetic as such is further than that from fp32: PyTorch's own CPU bf16 autocast of
the same model misses the bound for the majority of (weights, windows) seeds at L >= 29 (median deviation 2-4 %,
conv1 weight gradient worst; a ReLU whose pre-activation changes sign under bf16 rounding moves a whole term of the
sum).  At such a point the fp32 reference says nothing about a bf16 kernel, so ``_inputs`` draws seeds in order and
takes the first at which the reference is a usable yardstick: PyTorch's bf16 autocast (CPU, no code under test)
within HALF the bound of fp32 autograd for every tensor.  The other half is left to the kernel's own choices
(summation order, bf16 storage of dh1).  Bound, reference and cases are unchanged.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from test_fused_tiny_gpu import TOL, _ref_grads

pytestmark = pytest.mark.gpu

B = 3
LEAK = 1e6  # value of the rows no sample selects
CASES = [(L, nc, form) for L in (8, 29, 32, 33, 63, 100, 300) for nc in (2, 5) for form in ("direct", "idx")]
cases = pytest.mark.parametrize("L,nc,form", CASES)


def _cpu_grads(model, x, y, amp):
    model.zero_grad()
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=amp):
        out = model(x.unsqueeze(1))
    F.cross_entropy(out.float(), y).backward()
    return [p.grad.clone() for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _inputs(L, nc):
    """(model on the CPU, windows [B, L], labels [B]) of the first seed at which bf16 autocast is within half the
    bound of fp32 autograd (module docstring).  Decided with PyTorch alone."""
    for seed in range(64):
        g = torch.Generator(device="cpu").manual_seed(seed + L)
        torch.manual_seed(seed)
        model = TinyECG(num_classes=nc)
        x = torch.randn(B, L, generator=g)
        y = torch.randint(0, nc, (B,), generator=g)
        ref, amp = _cpu_grads(model, x, y, False), _cpu_grads(model, x, y, True)
        dev = max(((a - b).norm() / (a.norm() + 1e-6)).item() for a, b in zip(ref, amp))
        if dev < 0.5 * 3e-2:
            print(f"L={L} nc={nc}: seed {seed}, bf16 autocast vs fp32 autograd {dev:.4g}")
            model.zero_grad(set_to_none=True)
            return model, x, y
    raise AssertionError(f"L={L} nc={nc}: no seed below 64 where bf16 autocast is within 1.5e-2 of fp32 autograd")


def _case(L, nc, form):
    dev = torch.device("cuda:0")
    model0, x3, y3 = _inputs(L, nc)
    model = TinyECG(num_classes=nc)
    model.load_state_dict(model0.state_dict())
    model = model.to(dev)
    if form == "direct":
        return dev, x3.to(dev), y3.to(dev), model, None, torch.arange(B, dtype=torch.int32, device=dev)
    rows = torch.tensor([6, 0, 3], dtype=torch.int32)  # first and last row of the dataset selected
    x = torch.full((7, L), LEAK)
    y = torch.zeros(7, dtype=y3.dtype)
    x[rows.long()] = x3
    y[rows.long()] = y3
    return dev, x.to(dev), y.to(dev), model, rows.to(dev), rows.to(dev)


@functools.lru_cache(maxsize=None)
def _computed(L, nc, form):
    """Once per case: the fp32 autograd reference and the gradient rows of every kernel variant
    (waves 0 = automatic, 8, 16) x (prepared fragments, LDS-built operands)."""
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads, labels_int32
    dev, x, y, model, idx, sel = _case(L, nc, form)
    gref, lref = _ref_grads(model, x, y, sel)
    flat = model.flatten_parameters()
    y32 = labels_int32(y, nc)
    P = num_params(nc)  # columns [0, P]: gradient row + loss (the slab's padding columns are never written)
    lib = _lib.kernels()
    prev = lib.ecg_tiny_force_waves(0)
    rows = {}
    try:
        for waves in (0, 8, 16):
            lib.ecg_tiny_force_waves(waves)
            for pf in (True, False):
                rows[waves, pf] = tiny_step_grads(flat, x, y32, idx, B, nc, prefrag=pf)[:, :P + 1].clone()
        torch.cuda.synchronize()
    finally:
        lib.ecg_tiny_force_waves(prev)
    return model, gref, lref, rows


def _tensor_errs(model, a, b):
    off = 0
    for name, p in model.named_parameters():
        n = p.numel()
        yield name, (a[off:off + n] - b[off:off + n]).norm().item() / (b[off:off + n].norm().item() + 1e-6)
        off += n


@cases
def test_prefrag_rows_equal_lds_built_rows(L, nc, form):
    model, gref, lref, rows = _computed(L, nc, form)
    for waves in (0, 8, 16):
        a, b = rows[waves, True], rows[waves, False]
        assert torch.equal(a, b), (waves, (a - b).abs().max().item())


@cases
def test_rows_match_autograd(L, nc, form):
    from crossscale_ecg.ops.fused_tiny import reduce_slab
    model, gref, lref, rows = _computed(L, nc, form)
    for pf in (True, False):
        grad, loss = reduce_slab(rows[0, pf], nc)
        lerr = abs(loss.item() / B - lref.item())
        print(f"prefrag={pf}: loss err {lerr:.3g}")
        assert lerr < 1e-2 * max(1.0, abs(lref.item()))
        errs = list(_tensor_errs(model, grad, gref))
        print(f"prefrag={pf}:", ", ".join(f"{n} {e:.4g}" for n, e in errs))
        for name, rel in errs:
            assert rel < 3e-2, f"prefrag={pf}: {name}: rel err {rel:.4g}"


@cases
def test_8_and_16_waves_agree(L, nc, form):
    from crossscale_ecg.ops.fused_tiny import reduce_slab
    model, gref, lref, rows = _computed(L, nc, form)
    g8, g16 = reduce_slab(rows[8, True], nc)[0], reduce_slab(rows[16, True], nc)[0]
    errs = list(_tensor_errs(model, g8, g16))
    print("8 vs 16 waves:", ", ".join(f"{n} {e:.4g}" for n, e in errs))
    for name, rel in errs:
        assert rel < 3e-2, f"{name}: {rel:.4g}"


@pytest.mark.parametrize("form", ["direct", "idx"])
def test_forward_L33(form):
    from crossscale_ecg.ops.fused_tiny import tiny_forward
    dev, x, y, model, idx, sel = _case(33, 2, form)
    flat = model.flatten_parameters()
    fa = tiny_forward(flat, x, idx, B, 2, prefrag=True)
    fb = tiny_forward(flat, x, idx, B, 2, prefrag=False)
    ref = model(x[sel.long()].unsqueeze(1))
    torch.cuda.synchronize()
    assert torch.equal(fa, fb)
    err = (fa - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-3
    print(f"forward L=33 {form}: max err {err:.3g} (scale {scale:.3g})")
    assert err / scale < TOL["bf16"], f"max err {err} (scale {scale})"
