"""The TinyECG kernels against the operand-exact float64 reference (models/tiny_ecg_ref.py): a float64 model of the
forward and the per-sample backward that rounds to bf16 exactly where the bf16 kernels round, so what separates a
correct kernel from it is fp32 summation order and the rare value that order puts on the other side of a bf16 rounding
boundary - not the several percent that separate bf16 arithmetic from fp32 autograd.

Asserted, per sample row and per tensor of the row (the loss column included): ``|kernel - ref|_2 / |ref|_2 < bound``;
for logits ``max |kernel - ref| / max |ref| < bound``; for summed losses the relative difference.

Bounds (tests/tiny_operand_cases.py; measured on the CPU by tests/test_tiny_ref_cpu.py over exactly the cases below,
with no kernel involved, and asserted there):

    bf16 kernels: reference in float32 against reference in float64   floor 5.67e-07   REF_BOUND     = 5.7e-06
    fp32 kernels: float32 autograd against float64 autograd           floor 2.23e-07   REF_BOUND_F32 = 2.3e-06

Both are 10 x the floor and far below the condition ``REF_BOUND <= 1e-3`` (a third of the smallest seam defect
measured at L = 500, 2.9e-3; the defects injected by tests/test_tiny_ref_cpu.py move a row by 7e-4 .. 1.8e-2).  No
seed had to be replaced: seed 0 of every case is below ``SEED_FLOOR_MAX``, and none shows a rounding flip.

Cases (every shape is one another GPU test launches already), B = 4:
  * gradient rows of ``tiny_step_grads``: L in {8, 29, 32, 33, 63, 100, 300, 500} x nc in {2, 5}, waves forced to
    0 (automatic) / 8 / 16, prepared fragments and LDS-built operands, rows addressed directly and through an ``idx``
    into a dataset whose other rows hold 1e6; the recorder's "zeros" inputs at L = 100;
  * the production kernels - packed rows read in place (MODE 4), the copying gather and the converting gather feeding
    the packed-row kernel - through ``FusedTinyTrainer`` rounds of 3 steps with ``lr = 0``: the slab after the round
    holds the last step's rows at the unchanged weights (steps s > 0 are the PK kernels);
  * a cohort round of three clients with distinct weights (``fanout = 0``, NaN padding floats);
  * logits of ``tiny_forward`` (both operand builds) and of ``tiny_evaluate``, and its ``loss_sum``;
  * the fp32 kernels against the reference without rounding.

Worst errors observed on an MI355X (every test prints its own), all 103 cases inside the bound:

    tiny_step_grads rows, bf16 (204 variants)      1.7e-07  (loss column; worst gradient tensor below that)
    trainer rounds, last step's rows (48)          1.57e-07
    cohort round, three clients                    1.59e-07
    logits of tiny_forward / tiny_evaluate         < 3.6e-07
    tiny_evaluate loss_sum                         5.69e-07  (n = 1: one fp32 loss of 0.098 against float64)
    fp32 kernels' rows (24 variants)               2.17e-07  (conv2 weight gradient)

Every figure is a few fp32 ulps: in no case does a kernel value sit on the other side of a bf16 rounding boundary from
the reference's (one flipped h1 or dh1 element would show as 1e-5 or more in its tensor).
"""
import functools

import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.models.tiny_ecg_ref import logit_error, row_errors

import tiny_operand_cases as tc
from tiny_operand_cases import B, REF_BOUND, REF_BOUND_F32

pytestmark = pytest.mark.gpu

LEAK = 1e6            # value of the dataset rows no sample selects
ROWS = (6, 0, 3, 5)   # dataset rows of samples 0 .. 3: first and last row of the dataset selected
WAVES = (0, 8, 16)


def _dev():
    return torch.device("cuda:0")


def _dev_flat(flat):
    """The flat weights on the GPU, padded to 64 floats (the buffer of ``flatten_parameters``)."""
    out = torch.zeros((flat.numel() + 63) // 64 * 64, dtype=torch.float32, device=_dev())
    out[:flat.numel()] = flat
    return out


def _scattered(x, y):
    """(x7 [7, L], y7 [7]) with samples 0 .. 3 in rows ROWS and LEAK everywhere else."""
    x7 = torch.full((7, x.shape[1]), LEAK)
    y7 = torch.zeros(7, dtype=torch.long)
    x7[list(ROWS)] = x
    y7[list(ROWS)] = y
    return x7, y7


class _forced_waves:
    def __init__(self, waves):
        self.waves = waves

    def __enter__(self):
        from crossscale_ecg.ops import _lib
        self.lib = _lib.kernels()
        self.prev = self.lib.ecg_tiny_force_waves(self.waves)

    def __exit__(self, *exc):
        self.lib.ecg_tiny_force_waves(self.prev)


def _check_rows(what, got, ref_rows, nc, bound):
    errs = row_errors(got, ref_rows, nc)
    name, e = tc.worst(errs)
    print(f"{what}: worst {e:.3g} ({name}) of bound {bound:.3g}")
    assert torch.isfinite(got).all(), what
    for name, e in errs.items():
        assert e < bound, f"{what}: {name}: {e:.4g} >= {bound:.3g}   all: " + ", ".join(
            f"{n} {v:.3g}" for n, v in errs.items())
    return e


# ------------------------------------------------------------------------------------------------ tiny_step_grads
@functools.lru_cache(maxsize=None)
def _step_rows(L, nc, kind, form, precision="bf16"):
    """{(waves, prefrag): rows [B, P + 1]} of ``tiny_step_grads``, once per case."""
    from crossscale_ecg.ops.fused_tiny import labels_int32, tiny_step_grads
    c = tc.grad_case(L, nc, kind) if precision == "bf16" else tc.f32_case(L, nc)
    dev, P = _dev(), num_params(nc)
    flat = _dev_flat(c["flat"])
    if form == "direct":
        x, y, idx = c["x"].to(dev), c["y"].to(dev), None
    else:
        x7, y7 = _scattered(c["x"], c["y"])
        x, y, idx = x7.to(dev), y7.to(dev), torch.tensor(ROWS, dtype=torch.int32, device=dev)
    y32 = labels_int32(y, nc)
    out = {}
    for waves in WAVES:
        with _forced_waves(waves):
            for pf in ((True, False) if precision == "bf16" else (False,)):
                out[waves, pf] = tiny_step_grads(flat, x, y32, idx, B, nc, precision=precision,
                                                 prefrag=pf)[:, :P + 1].clone()
            torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("form", ["direct", "idx"])
@pytest.mark.parametrize("L,nc,kind", tc.GRAD_CASES)
def test_step_grads_rows(L, nc, kind, form):
    c = tc.grad_case(L, nc, kind)
    rows = _step_rows(L, nc, kind, form)
    assert len(rows) == 6
    for (waves, pf), got in rows.items():
        _check_rows(f"L={L} nc={nc} {kind} {form} waves={waves} prefrag={pf}", got, c["ref"].rows, nc, REF_BOUND)


@pytest.mark.parametrize("L,nc", tc.F32_CASES)
def test_fp32_step_grads_rows(L, nc):
    c = tc.f32_case(L, nc)
    for (waves, _), got in _step_rows(L, nc, "randn", "direct", "fp32").items():
        _check_rows(f"fp32 L={L} nc={nc} waves={waves}", got, c["ref"].rows, nc, REF_BOUND_F32)


# ------------------------------------------------------------------------------------- production kernels (trainer)
# batches of the round: every step takes the four samples, in another order (dataset rows; the rest hold LEAK)
TABLE = ((6, 0, 3, 5), (0, 5, 6, 3), (3, 6, 5, 0))


@pytest.mark.parametrize("waves", [8, 16])
@pytest.mark.parametrize("prepack", ["direct", "gather", "none"])
@pytest.mark.parametrize("L,nc", tc.TRAINER_CASES)
def test_trainer_last_step_rows(L, nc, prepack, waves):
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    c = tc.grad_case(L, nc)
    dev, P = _dev(), num_params(nc)
    x7, y7 = _scattered(c["x"], c["y"])
    model = TinyECG(num_classes=nc)
    torch.nn.utils.vector_to_parameters(c["flat"].clone(), model.parameters())
    model = model.to(dev)
    table = torch.tensor(TABLE, dtype=torch.int32, device=dev)
    with _forced_waves(waves):
        tr = FusedTinyTrainer(model, x7.to(dev), y7.to(dev), B, len(TABLE), lr=0.0, seed=0, prepack=prepack)
        try:
            assert tr.prepack == prepack, tr.prepack_fallback
            assert (tr.xpk is not None) == (prepack != "none") and (tr.xbg is not None) == (prepack != "direct")
            tr.prepare_round(len(TABLE))
            tr.idx_stage[:len(TABLE)].copy_(table)  # the staged table is what the round reads
            tr.launch_round(len(TABLE))
            torch.cuda.synchronize()
            got, params, loss = tr.slab[:, :P + 1].cpu(), tr.params[:P].cpu(), tr.loss_acc.item()
        finally:
            tr.close()
    assert torch.equal(params, c["flat"]), "lr = 0 must leave the weights as they were"
    order = [ROWS.index(r) for r in TABLE[-1]]  # the samples of the last step's rows
    _check_rows(f"trainer L={L} nc={nc} prepack={prepack} waves={waves}", got, c["ref"].rows[order], nc, REF_BOUND)
    want = len(TABLE) * c["ref"].loss.sum().item()
    print(f"summed loss {loss!r} reference {want!r}")
    assert abs(loss - want) < REF_BOUND * abs(want)


# ------------------------------------------------------------------------------------------------------- cohort
def test_cohort_round_rows():
    from cohort_harness import Cohort
    cc, case = tc.cohort_case(), tc.COHORT_CASE
    nc, M = case["nc"], case["M"]
    dev, P = _dev(), num_params(nc)
    co = Cohort(cc["x"].to(dev), cc["y"].to(torch.int32).to(dev), nc, M, B, 1, "bf16", cc["table"].to(dev), fanout=0,
                w=cc["w"].to(dev), m=torch.zeros(M, P, device=dev), pad=float("nan")).run()
    slab = co.slab[:, :P + 1].cpu()
    for c in range(M):
        _check_rows(f"cohort client {c}", slab[c * B:(c + 1) * B], cc["refs"][c].rows, nc, REF_BOUND)


# ------------------------------------------------------------------------------------------------------- logits
@pytest.mark.parametrize("L,nc", tc.LOGIT_CASES)
def test_logits_and_loss_sum(L, nc):
    from crossscale_ecg.ops.fused_tiny import tiny_forward
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    c = tc.logit_case(L, nc)
    dev = _dev()
    flat, x, y32 = _dev_flat(c["flat"]), c["x"].to(dev), c["y"].to(torch.int32).to(dev)
    worst = 0.0
    for n in tc.LOGIT_N:
        ref = c["ref"].logits[:n]
        res = tiny_evaluate(flat, x[:n], y32[:n], None, nc, return_logits=True)
        torch.cuda.synchronize()
        got = {"forward PF": tiny_forward(flat, x[:n], None, n, nc, prefrag=True),
               "forward LDS-built": tiny_forward(flat, x[:n], None, n, nc, prefrag=False),
               "evaluate": res.logits}
        torch.cuda.synchronize()
        for what, lg in got.items():
            e = logit_error(lg, ref)
            worst = max(worst, e)
            assert torch.isfinite(lg).all()
            assert e < REF_BOUND, f"L={L} nc={nc} n={n} {what}: {e:.4g} >= {REF_BOUND:.3g}"
        want = c["ref"].loss[:n].sum().item()
        e = abs(res.loss_sum - want) / abs(want)
        print(f"L={L} nc={nc} n={n}: loss_sum {res.loss_sum!r} reference {want!r}: {e:.3g}")
        worst = max(worst, e)
        assert res.count == n
        assert e < REF_BOUND, f"L={L} nc={nc} n={n} loss_sum: {e:.4g} >= {REF_BOUND:.3g}"
    print(f"L={L} nc={nc}: worst {worst:.3g} of bound {REF_BOUND:.3g}")
