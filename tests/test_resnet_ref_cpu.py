"""The teacher-forced per-block references (models/resnet1d_ref.py) equal PyTorch autograd of a training-mode
BasicBlock1D in float64 - the oracle the GPU engine test (test_resnet_engine_gpu.py) is pinned against."""
import pytest
import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.resnet1d import BasicBlock1D
from crossscale_ecg.models.resnet1d_ref import block_backward_reference, block_forward_reference


def _block_vs_autograd(cin, cout, stride, B, L):
    torch.manual_seed(0)
    blk = BasicBlock1D(cin, cout, stride).double().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.2, 0.2)
    h = F.relu(torch.randn(B, cin, L, dtype=torch.float64)).requires_grad_(True)
    # module forward with the intermediates exposed
    z1 = blk.conv1(h)
    a1 = F.relu(blk.bn1(z1))
    z2 = blk.conv2(a1)
    zd = blk.downsample[0](h) if blk.downsample is not None else None
    idt = blk.downsample[1](zd) if zd is not None else h
    pre = blk.bn2(z2) + idt
    out = F.relu(pre)
    up = torch.randn_like(out)
    for t in (z1, a1, z2, pre):
        t.retain_grad()
    out.backward(up)
    eps = blk.bn1.eps
    bn = {"bn1": (blk.bn1.weight.detach(), blk.bn1.bias.detach()), "bn2": (blk.bn2.weight.detach(), blk.bn2.bias.detach())}
    Wd = None
    if blk.downsample is not None:
        bn["ds"] = (blk.downsample[1].weight.detach(), blk.downsample[1].bias.detach())
        Wd = blk.downsample[0].weight.detach()
    d = lambda t: None if t is None else t.detach()  # noqa: E731
    fw = block_forward_reference(d(h), d(z1), d(a1), d(z2), d(zd), blk.conv1.weight.detach(),
                                 blk.conv2.weight.detach(), Wd, bn, stride, eps)
    for k, want in (("z1", z1), ("a1", a1), ("z2", z2), ("zd", zd), ("out", out)):
        if want is not None:
            assert torch.allclose(fw[k], want, atol=1e-10), k
    G = pre.grad.detach()
    g, din = block_backward_reference(G, d(h), d(z1), d(a1), d(z2), d(zd), blk.conv1.weight.detach(),
                                      blk.conv2.weight.detach(), Wd, bn, stride, eps, mask_in=False)
    for name, p in blk.named_parameters():
        assert torch.allclose(g[name], p.grad, atol=1e-9, rtol=1e-7), name
    assert torch.allclose(din, h.grad, atol=1e-9)


@pytest.mark.parametrize("cin,cout,stride", [(16, 16, 1), (16, 32, 2)])
def test_block_reference_matches_autograd(cin, cout, stride):
    _block_vs_autograd(cin, cout, stride, 4, 37)


# Block shapes the GPU engine test reaches off the benchmark window length (test_resnet_engine_gpu.py, OFF_SHAPES)
@pytest.mark.parametrize("cin,cout,stride,B,L", [
    (16, 32, 2, 3, 21),   # stride 2 from an odd length: 21 -> 11
    (16, 32, 2, 3, 84),   # stride 2 from an even length: the last input row is reached by one tap only (84 -> 42)
    (32, 32, 1, 5, 1),    # Lin = 1: both outer taps fall into the padding on every row
    (16, 32, 2, 5, 1),    # stride 2 on one input row (1 -> 1), downsample included
    (16, 32, 2, 3, 4),    # a downsample block with 6 output rows under its BatchNorms
    (16, 16, 1, 3, 2),    # 6 rows, identity residual
    (16, 32, 2, 7, 3),    # 3 -> 2
])
def test_block_reference_matches_autograd_off_shapes(cin, cout, stride, B, L):
    _block_vs_autograd(cin, cout, stride, B, L)


@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("Lf", [1, 2])
@pytest.mark.parametrize("ncls", [5, 16])
def test_head_autograd_matches_closed_form(ncls, Lf, B):
    """The engine test's head oracle - autograd of cross_entropy(linear(mean_t h)) - against the closed form the head
    kernel implements: g = (softmax - onehot) / B, dW = g^T feat, db = sum_b g, dh[b, :, t] = W^T g[b] / Lf."""
    torch.manual_seed(ncls + Lf)
    C = 24
    h = F.relu(torch.randn(B, C, Lf, dtype=torch.float64)).requires_grad_(True)
    W = torch.randn(ncls, C, dtype=torch.float64, requires_grad=True)
    b = torch.randn(ncls, dtype=torch.float64, requires_grad=True)
    y = torch.randint(0, ncls, (B,))
    loss = F.cross_entropy(F.linear(h.mean(dim=2), W, b), y)
    loss.backward()
    feat = h.detach().sum(dim=2) / Lf
    logits = feat @ W.detach().T + b.detach()
    lse = torch.logsumexp(logits, dim=1)
    assert torch.allclose(loss.detach(), (lse - logits[torch.arange(B), y]).sum() / B, atol=1e-12)
    g = (torch.exp(logits - lse[:, None]) - F.one_hot(y, ncls)) / B
    assert torch.allclose(W.grad, g.T @ feat, atol=1e-12)
    assert torch.allclose(b.grad, g.sum(0), atol=1e-12)
    assert torch.allclose(h.grad, ((g @ W.detach()) / Lf)[:, :, None].expand(B, C, Lf), atol=1e-12)


@pytest.mark.parametrize("B,L", [(5, 250), (3, 333), (7, 37), (5, 16)])
def test_stem_reference_matches_module_autograd(B, L):
    """The engine test's stem oracle (F.conv1d, bn_apply, relu, max_pool1d, conv1d_weight) against autograd of the
    Conv1d / BatchNorm1d / MaxPool1d modules, and its pool backward against the definition the stem kernels implement
    (the whole gradient of a window goes to its first maximum), at odd stem output lengths Lz (125, 167, 19: the last
    pool window holds two rows) and odd L."""
    from crossscale_ecg.models.resnet1d_ref import bn_apply, bn_backward
    torch.manual_seed(L)
    conv = torch.nn.Conv1d(1, 8, 7, 2, 3, bias=False).double()
    bn = torch.nn.BatchNorm1d(8).double().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    x = torch.randn(B, 1, L, dtype=torch.float64)
    z = conv(x)
    z.retain_grad()
    out = F.max_pool1d(F.relu(bn(z)), 3, 2, 1)
    Lz, Lp = z.shape[2], out.shape[2]
    assert Lz == (L - 1) // 2 + 1 and Lp == (Lz - 1) // 2 + 1
    up = torch.randn_like(out)
    out.backward(up)
    eps = bn.eps
    gam, bet = bn.weight.detach(), bn.bias.detach()
    z0 = F.conv1d(x, conv.weight.detach(), None, 2, 3)
    assert torch.allclose(z0, z.detach(), atol=1e-12)
    a = F.relu(bn_apply(z0, gam, bet, eps))
    assert torch.allclose(F.max_pool1d(a, 3, 2, 1), out.detach(), atol=1e-10)
    # pool + ReLU backward by definition: window o = rows 2o-1 .. 2o+1 inside [0, Lz), first maximum takes the gradient
    da = torch.zeros_like(a)
    for o in range(Lp):
        rows = [j for j in (2 * o - 1, 2 * o, 2 * o + 1) if 0 <= j < Lz]
        win = a[:, :, rows]
        mx = win.max(dim=2, keepdim=True).values
        first = ((win == mx).cumsum(dim=2) == 0).sum(dim=2)  # rows before the first maximum (argmax leaves ties open)
        for k, j in enumerate(rows):
            da[:, :, j] += up[:, :, o] * (first == k)
    da = da * (a > 0)
    dz, dgam, dbet = bn_backward(da, z0, gam, eps)
    assert torch.allclose(dgam, bn.weight.grad, atol=1e-9, rtol=1e-7)
    assert torch.allclose(dbet, bn.bias.grad, atol=1e-9, rtol=1e-7)
    assert torch.allclose(dz, z.grad, atol=1e-9)
    dW = torch.nn.grad.conv1d_weight(x, conv.weight.shape, dz, 2, 3)
    assert torch.allclose(dW, conv.weight.grad, atol=1e-9, rtol=1e-7)
