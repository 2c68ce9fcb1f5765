"""The fused TinyECG evaluation kernel (ops.tiny_eval.tiny_evaluate / FusedTinyTrainer.evaluate) against an fp32
PyTorch reference and against the metrics of its own logits.

Inputs: windows with a random amplitude and offset per window and a head scaled by 8, so that the reference predicts
at least two classes (plain randn windows with the default init give near-identical logits for every window, which
would leave the confusion matrix untested).  Every case asserts that condition on its reference."""
import functools

import pytest
import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, state_dict_to_flat

pytestmark = pytest.mark.gpu

TOL = 2e-2  # the project's bf16 bound (tests/test_fused_tiny_gpu.py TOL["bf16"])
N_FULL = 2048
CASES = [(2, 500, 0), (2, 333, 2), (5, 500, 0), (16, 96, 3), (2, 64, 2)]


@functools.lru_cache(maxsize=None)
def _case(nc, L, seed, N=N_FULL):
    """(x, y int32, flat weights) on the GPU and the fp32 reference logits (computed once on the CPU, shared)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    amp = 0.25 + 2.75 * torch.rand(N, generator=g)
    off = 2 * torch.rand(N, generator=g) - 1
    x = torch.randn(N, L, generator=g) * amp[:, None] + off[:, None]
    y = torch.randint(0, nc, (N,), generator=g)
    torch.manual_seed(seed)
    model = TinyECG(nc)
    with torch.no_grad():
        model.head.weight.mul_(8)
        ref = model(x.unsqueeze(1))
    assert ref.argmax(1).unique().numel() >= 2, "the reference predicts a single class: inputs test nothing"
    dev = torch.device("cuda:0")
    flat = state_dict_to_flat(model.state_dict(), nc).to(dev)
    return x.to(dev), y.to(torch.int32).to(dev), flat, ref.to(dev)


def _rel_err(out, ref):
    return ((out - ref).abs().max() / (ref.abs().max() + 1e-3)).item()


def _check_own_metrics(res, y32, nc, n, ref=None):
    """The reduced metrics are exactly the metrics of the kernel's own logits (no tolerance around the argmax)."""
    torch.cuda.synchronize()
    logits, pred, y = res.logits, res.pred, y32.long()
    assert torch.equal(pred.long(), logits.argmax(1))
    assert res.count == n
    assert res.correct == int((pred.long() == y).sum())
    conf = torch.bincount(y * nc + pred.long(), minlength=nc * nc).reshape(nc, nc).cpu()
    assert torch.equal(res.confusion, conf)
    own = F.cross_entropy(logits.double(), y, reduction="sum").item()
    print(f"loss_sum {res.loss_sum!r} own-logits float64 {own!r}")
    assert abs(res.loss_sum - own) <= 1e-5 * abs(own)
    if ref is not None:
        err = _rel_err(logits, ref)
        lref = F.cross_entropy(ref, y).item()
        print(f"logits rel err {err:.3e}  mean loss {res.loss:.6f} ref {lref:.6f}")
        assert err < TOL
        assert abs(res.loss - lref) < 1e-2 * max(1.0, abs(lref))


@pytest.mark.parametrize("nc,L,seed", CASES)
def test_logits_and_metrics(nc, L, seed):
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, ref = _case(nc, L, seed)
    res = tiny_evaluate(flat, x, y, None, nc, return_pred=True, return_logits=True)
    _check_own_metrics(res, y, nc, N_FULL, ref)


@pytest.mark.parametrize("nc,L,seed", [(2, 500, 0), (5, 500, 0), (2, 333, 2)])
def test_same_metrics_without_optional_outputs(nc, L, seed):
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, _ = _case(nc, L, seed)
    full = tiny_evaluate(flat, x, y, None, nc, return_pred=True, return_logits=True)
    a = torch.cat([full.loss_sum_t.view(torch.int64), full.counts_t]).clone()
    for kw in ({}, {"return_pred": True}, {"return_logits": True}):
        r = tiny_evaluate(flat, x, y, None, nc, **kw)
        assert (r.pred is not None) == bool(kw.get("return_pred")) and (r.logits is not None) == bool(
            kw.get("return_logits"))
        assert torch.equal(torch.cat([r.loss_sum_t.view(torch.int64), r.counts_t]), a), kw


@pytest.mark.parametrize("L,seed", [(500, 0), (333, 2)])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_small_and_ragged_n(n, L, seed):
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, ref = _case(2, L, seed)
    res = tiny_evaluate(flat, x[:n], y[:n], None, 2, return_pred=True, return_logits=True)
    torch.cuda.synchronize()
    assert _rel_err(res.logits, ref[:n]) < TOL
    _check_own_metrics(res, y[:n], 2, n)


@pytest.mark.parametrize("L,seed", [(500, 0), (333, 2)])
def test_grid_caps_and_repeat(L, seed):
    """N = 300 on 1 and 2 workgroups (every wave walks several windows) and on the automatic grid (more waves than
    windows: some get none): counts and predictions are bit-identical, loss_sum differs at most in its fp64
    summation order; the same call repeated is bitwise identical."""
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, ref = _case(2, L, seed)
    n = 300
    runs = []
    for cap in (1, 2, 0, 0):
        r = tiny_evaluate(flat, x[:n], y[:n], None, 2, return_pred=True, return_logits=True, max_workgroups=cap)
        _check_own_metrics(r, y[:n], 2, n)
        runs.append((r.loss_sum_t.clone(), r.counts_t.clone(), r.pred, r.logits))
    assert _rel_err(runs[0][3], ref[:n]) < TOL
    for ls, counts, pred, logits in runs[1:]:
        assert torch.equal(counts, runs[0][1]) and torch.equal(pred, runs[0][2]) and torch.equal(logits, runs[0][3])
        assert abs(ls.item() - runs[0][0].item()) <= 1e-9 * abs(runs[0][0].item())
    assert torch.equal(runs[2][0].view(torch.int64), runs[3][0].view(torch.int64))  # repeated call: bitwise


def test_addressing_idx_with_repeats():
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, _ = _case(2, 500, 0)
    full = tiny_evaluate(flat, x, y, None, 2, return_pred=True, return_logits=True)
    g = torch.Generator(device="cpu").manual_seed(5)
    idx = torch.cat([torch.randperm(N_FULL, generator=g)[:400], torch.randint(0, N_FULL, (113,), generator=g)])
    idx = idx.to(torch.int32).to(x.device)
    res = tiny_evaluate(flat, x, y, idx, 2, return_pred=True, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(res.logits, full.logits[idx.long()])
    assert torch.equal(res.pred, full.pred[idx.long()])
    assert res.count == idx.numel()
    assert res.correct == int((full.pred[idx.long()] == y[idx.long()]).sum())


def test_addressing_unaligned_rows_and_row_stride():
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    # rows of an L = 333 shard start at odd multiples of 4 bytes
    x, y, flat, _ = _case(2, 333, 2)
    full = tiny_evaluate(flat, x, y, None, 2, return_pred=True, return_logits=True)
    assert x[1:].data_ptr() % 16 != 0
    res = tiny_evaluate(flat, x[1:], y[1:], None, 2, return_pred=True, return_logits=True)
    _check_own_metrics(res, y[1:], 2, N_FULL - 1)
    assert torch.equal(res.logits, full.logits[1:])
    # a [N, 512] shard viewed as [:, :500]: row stride != L (16-byte rows), plus a row slice of it
    x, y, flat, _ = _case(2, 500, 0)
    full = tiny_evaluate(flat, x, y, None, 2, return_pred=True, return_logits=True)
    wide = torch.full((N_FULL, 512), 1e30, device=x.device)
    wide[:, :500] = x
    view = wide[:, :500]
    assert view.stride(0) == 512
    res = tiny_evaluate(flat, view, y, None, 2, return_pred=True, return_logits=True)
    _check_own_metrics(res, y, 2, N_FULL)
    assert torch.equal(res.logits, full.logits)
    res = tiny_evaluate(flat, view[3:], y[3:], None, 2, return_pred=True, return_logits=True)
    torch.cuda.synchronize()
    assert torch.equal(res.logits, full.logits[3:])


@pytest.mark.parametrize("L,seed", [(500, 0), (333, 2)])
def test_canary_tail_stays_unread(L, seed):
    """Nothing past the last row is read: a shard followed by huge values evaluates exactly like a copy without."""
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, _ = _case(2, L, seed)
    n = 130
    buf = torch.full((n * L + 64,), 3e38, device=x.device)
    buf[:n * L] = x[:n].reshape(-1)
    tail = buf[:n * L].view(n, L)
    a = tiny_evaluate(flat, tail, y[:n], None, 2, return_pred=True, return_logits=True)
    av = (a.loss_sum_t.clone(), a.counts_t.clone())
    b = tiny_evaluate(flat, x[:n].clone(), y[:n], None, 2, return_pred=True, return_logits=True)
    torch.cuda.synchronize()
    assert torch.isfinite(a.logits).all()
    assert torch.equal(a.logits, b.logits) and torch.equal(a.pred, b.pred)
    assert torch.equal(av[1], b.counts_t) and torch.equal(av[0].view(torch.int64), b.loss_sum_t.view(torch.int64))


def test_inference_without_labels():
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, _ = _case(5, 500, 0)
    full = tiny_evaluate(flat, x, y, None, 5, return_pred=True, return_logits=True)
    res = tiny_evaluate(flat, x, None, None, 5)
    torch.cuda.synchronize()
    assert torch.equal(res.logits, full.logits) and torch.equal(res.pred, full.pred)
    assert res.count == 0 and res.correct == 0 and res.loss_sum == 0.0 and int(res.confusion.sum()) == 0


def test_bad_arguments_fail_before_launch():
    from crossscale_ecg.ops._lib import NativeError
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    x, y, flat, _ = _case(2, 500, 0)
    dev = x.device
    bad = (NativeError, ValueError)
    with pytest.raises(bad):
        tiny_evaluate(torch.zeros(4096, device=dev), x, y, None, 17)
    with pytest.raises(bad):
        tiny_evaluate(flat, torch.zeros(8, 4, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
    with pytest.raises(bad):
        tiny_evaluate(flat, torch.zeros(8, 2000, device=dev), torch.zeros(8, dtype=torch.int32, device=dev))
    with pytest.raises(bad):
        tiny_evaluate(flat, x, y.cpu())
    with pytest.raises(bad):
        tiny_evaluate(flat, x, y.long())
    torch.cuda.synchronize()


def test_trainer_evaluate():
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer, tiny_forward
    from crossscale_ecg.ops.tiny_eval import tiny_evaluate
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(11)
    x = torch.randn(4096, 500, generator=g).to(dev)
    y = (x.mean(1) > 0).long()

    def make():
        torch.manual_seed(3)
        return FusedTinyTrainer(TinyECG(2).to(dev), x, y, batch_size=128, steps_per_round=4, seed=5)

    tr, twin = make(), make()
    tr.run_round()
    twin.run_round()
    res = tr.evaluate()
    first = (res.loss_sum_t.clone(), res.counts_t.clone())
    direct = tiny_evaluate(tr.params, x, tr.y32, None, 2, return_pred=True, return_logits=True)
    _check_own_metrics(direct, tr.y32, 2, 4096)
    assert torch.equal(first[1], direct.counts_t)
    assert torch.equal(first[0].view(torch.int64), direct.loss_sum_t.view(torch.int64))
    # the same forward as the training step's kernel, inside the bound both hold against fp32
    for prec in ("bf16", "fp32"):
        other = tiny_forward(tr.params, x, None, 4096, 2, precision=prec)
        assert _rel_err(direct.logits, other) < TOL, prec
    # training state untouched: bitwise equal to a twin that never evaluated
    torch.cuda.synchronize()
    for name in ("params", "mom", "loss_acc", "idx_table", "idx_stage"):
        assert torch.equal(getattr(tr, name), getattr(twin, name)), name
    assert tr._staged == twin._staged and tr.steps_done == twin.steps_done
    # another round: evaluate() sees the new weights, and the twin still tracks
    tr.run_round()
    twin.run_round()
    res2 = tr.evaluate()
    direct2 = tiny_evaluate(tr.params, x, tr.y32, None, 2)
    torch.cuda.synchronize()
    assert torch.equal(res2.counts_t, direct2.counts_t)
    assert torch.equal(res2.loss_sum_t.view(torch.int64), direct2.loss_sum_t.view(torch.int64))
    assert not torch.equal(res2.loss_sum_t.view(torch.int64), first[0].view(torch.int64))
    for name in ("params", "mom", "loss_acc"):
        assert torch.equal(getattr(tr, name), getattr(twin, name)), name
    # held-out windows with int64 labels
    held = tr.evaluate(x[:1000], y[:1000])
    assert held.count == 1000 and int(held.confusion.sum()) == 1000
    tr.close()
    twin.close()
