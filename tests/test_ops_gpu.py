"""HIP op numerics vs plain PyTorch fp32 references (Module-2 conv1d, flat SGD, gather/normalize)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("B", [64, 128, 256, 512])
@pytest.mark.parametrize("K", [3, 5, 7, 4, 32])
def test_conv1d_valid_fp32(B, K):
    from crossscale_ecg.ops.conv1d import conv1d_valid
    x = torch.randn(B, 500, device=DEV)
    w = torch.randn(K, device=DEV)
    y = conv1d_valid(x, w, backend="hip")
    ref = F.conv1d(x.unsqueeze(1).double(), w.double().view(1, 1, K))[:, 0].float()
    torch.cuda.synchronize()
    assert y.shape == (B, 500 - K + 1)
    assert torch.allclose(y, ref, atol=1e-5, rtol=1e-5), (y - ref).abs().max().item()


def test_conv1d_valid_bf16_and_3d_and_odd_alignment():
    from crossscale_ecg.ops.conv1d import conv1d_valid
    x = torch.randn(100, 1, 333, device=DEV)
    w = torch.randn(7, device=DEV)
    y = conv1d_valid(x, w, backend="hip")
    assert y.shape == (100, 1, 327)
    ref = F.conv1d(x, w.view(1, 1, 7))
    assert torch.allclose(y, ref, atol=1e-5, rtol=1e-5)
    xb = x[:, 0].bfloat16()
    yb = conv1d_valid(xb, w, backend="hip")
    refb = F.conv1d(xb.float().unsqueeze(1), w.view(1, 1, 7))[:, 0]
    assert (yb.float() - refb).abs().max().item() < 2e-2 * refb.abs().max().item()


@pytest.mark.parametrize("B,L,K", [(64, 500, 3), (256, 500, 7), (33, 333, 5), (8, 500, 32), (17, 101, 12)])
def test_conv1d_valid_backward_matches_autograd(B, L, K):
    """HIP dgrad + deterministic wgrad vs torch autograd of F.conv1d in fp64."""
    from crossscale_ecg.ops.conv1d import conv1d_valid_fn
    x = torch.randn(B, L, device=DEV, requires_grad=True)
    w = torch.randn(K, device=DEV, requires_grad=True)
    dy = torch.randn(B, L - K + 1, device=DEV)
    y = conv1d_valid_fn(x, w)
    y.backward(dy)
    xd, wd = x.detach().double().requires_grad_(), w.detach().double().requires_grad_()
    yr = F.conv1d(xd.unsqueeze(1), wd.view(1, 1, K))[:, 0]
    yr.backward(dy.double())
    assert torch.allclose(y.double(), yr, atol=1e-4, rtol=1e-5)
    assert torch.allclose(x.grad.double(), xd.grad, atol=1e-4, rtol=1e-5), (x.grad.double() - xd.grad).abs().max()
    assert torch.allclose(w.grad.double(), wd.grad, rtol=1e-4, atol=1e-3), (w.grad.double() - wd.grad).abs().max()
    # deterministic: the same inputs give the same bits
    from crossscale_ecg.ops.conv1d import conv1d_valid_backward
    a = conv1d_valid_backward(x.detach(), w.detach(), dy)
    b = conv1d_valid_backward(x.detach(), w.detach(), dy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_conv1d_valid_backward_bf16_and_blocking():
    from crossscale_ecg.ops.conv1d import conv1d_valid, conv1d_valid_backward
    x = torch.randn(128, 500, device=DEV).bfloat16()
    w = torch.randn(7, device=DEV)
    dy = torch.randn(128, 494, device=DEV).bfloat16()
    dx, dw = conv1d_valid_backward(x, w, dy)
    xd = x.double().requires_grad_()
    wd = w.double().requires_grad_()
    F.conv1d(xd.unsqueeze(1), wd.view(1, 1, 7))[:, 0].backward(dy.double())
    assert (dx.double() - xd.grad).abs().max().item() < 2e-2 * xd.grad.abs().max().item()
    assert (dw.double() - wd.grad).abs().max().item() < 1e-3 * wd.grad.abs().max().item()
    xf = torch.randn(256, 500, device=DEV)
    out = torch.empty(256, 494, device=DEV)
    y = conv1d_valid(xf, w, backend="hip", out=out, blocking=True)
    assert torch.allclose(y, F.conv1d(xf.unsqueeze(1), w.view(1, 1, 7))[:, 0], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize("momentum,dampening,wd,nesterov", [(0.9, 0.0, 0.0, False), (0.0, 0.0, 1e-4, False),
                                                             (0.9, 0.1, 1e-3, False), (0.9, 0.0, 0.0, True)])
def test_flat_sgd_matches_torch(momentum, dampening, wd, nesterov):
    from crossscale_ecg.ops.sgd import FlatSGD
    n = 1459
    p0 = torch.randn(n + 5, device=DEV)[:n].clone()
    p = torch.zeros(1472, device=DEV)
    p[:n] = p0
    g = torch.zeros_like(p)
    opt = FlatSGD(p, g, lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    q = torch.nn.Parameter(p0.clone())
    ref = torch.optim.SGD([q], lr=0.05, momentum=momentum, dampening=dampening, weight_decay=wd, nesterov=nesterov)
    for _ in range(4):
        gg = torch.randn(n, device=DEV)
        g[:n] = gg
        opt.step()
        q.grad = gg.clone()
        ref.step()
    torch.cuda.synchronize()
    assert torch.allclose(p[:n], q.detach(), rtol=1e-5, atol=1e-6)


def test_flat_sgd_found_inf_skips():
    from crossscale_ecg.ops.sgd import FlatSGD
    p = torch.ones(64, device=DEV)
    g = torch.ones(64, device=DEV)
    g[3] = float("inf")
    fi = torch.zeros(1, dtype=torch.int32, device=DEV)
    FlatSGD(p, g, lr=0.1, momentum=0.9).step(inv_scale=0.5, found_inf=fi)
    torch.cuda.synchronize()
    assert fi.item() == 1 and torch.all(p == 1)


@pytest.mark.parametrize("normalize", [False, True])
def test_gather_rows(normalize):
    from crossscale_ecg.ops.gather import gather_rows
    x = torch.randn(1000, 500, device=DEV) * 3 + 1
    idx = torch.randperm(1000, device=DEV)[:256].int()
    out = gather_rows(x, idx, normalize=normalize)
    ref = x[idx.long()].double()
    if normalize:
        ref = (ref - ref.mean(1, keepdim=True)) / (ref.std(1, unbiased=False, keepdim=True) + 1e-8)
    torch.cuda.synchronize()
    assert torch.allclose(out.double(), ref, atol=1e-5, rtol=1e-5)
    outb = gather_rows(x, idx, normalize=normalize, dtype=torch.bfloat16)
    assert torch.allclose(outb.double(), ref, atol=3e-2 * max(1, ref.abs().max().item()), rtol=1e-2)


def test_native_upload_and_prefetch(tmp_path):
    from crossscale_ecg.data.shards import write_shards
    from crossscale_ecg.ops import native_io
    data = np.random.default_rng(0).normal(size=(1000, 500)).astype(np.float32)
    paths = write_shards(data, str(tmp_path), shard_size=300)
    x = native_io.upload_shards(paths, DEV, 900, 500, chunk_rows=128)
    assert torch.equal(x.cpu(), torch.from_numpy(data[:900]))
    pf = native_io.NativePrefetcher(paths, batch_size=128, num_slots=3, normalize=False, pinned=True)
    pf.start()
    dst = torch.empty(128, 500, device=DEV)
    got = []
    while True:
        r = pf.next_batch_cpu()
        if r is None:
            break
        slot, view, _ms = r
        n = view.shape[0]
        pf.h2d(slot, n, dst)
        got.append(dst[:n].clone())
    pf.close()
    allx = torch.cat(got).cpu()
    assert torch.equal(allx, torch.from_numpy(data))


@pytest.mark.parametrize("B,K", [(64, 3), (256, 7), (512, 5), (300, 15), (33, 4)])
def test_conv1d_flag_call_matches_torch(B, K):
    """Blocking single call with the host-mapped completion word (Module-2 time_once path): output equal to
    F.conv1d after the call returns, over repeated calls (epoch logic) and interleaved with other stream work;
    K=4 (no compile-time variant) takes the launch + hipStreamSynchronize path."""
    import torch.nn.functional as F
    from crossscale_ecg.ops import _lib
    lib = _lib.kernels()
    raw = torch._C._cuda_getCurrentRawStream
    torch.manual_seed(B + K)
    for rep in range(3):
        x = torch.randn(B, 500, device="cuda")
        w = torch.randn(K, device="cuda")
        y = torch.full((B, 500 - K + 1), float("nan"), device="cuda")
        junk = torch.randn(1024, 1024, device="cuda") @ torch.randn(1024, 1024, device="cuda")  # work ahead of it
        st = lib.conv1d_batch_hip_flag(x.data_ptr(), w.data_ptr(), y.data_ptr(), B, 500, K, raw(0))
        assert st == 0
        ref = F.conv1d(x.unsqueeze(1), w.view(1, 1, K))[:, 0]
        torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-4)
        del junk


# n = 1, 3: only the scalar tail loop; 1459: float4 body + a 3-element tail; 2_097_155: the capped grid (2048 blocks x
# 256 threads x 4 floats = 2_097_152 elements in one sweep) plus a 3-element tail
@pytest.mark.parametrize("inv_scale", [1.0, 0.5])
@pytest.mark.parametrize("momentum,wd,nesterov", [(0.9, 1e-3, False), (0.9, 0.0, True)])
@pytest.mark.parametrize("n", [1, 3, 1459, 2_097_155])
def test_flat_sgd_tail_elements(n, momentum, wd, nesterov, inv_scale):
    """Three steps of sgd_flat_kernel on buffers whose length is no multiple of 4 (the scalar tail loop) against
    torch.optim.SGD in float64; with inv_scale = 0.5 and a finite gradient the update uses g * inv_scale and found_inf
    stays 0."""
    from crossscale_ecg.ops.sgd import FlatSGD
    gen = torch.Generator(device=DEV).manual_seed(n)
    p = torch.randn(n, device=DEV, generator=gen)
    g = torch.zeros_like(p)
    fi = torch.zeros(1, dtype=torch.int32, device=DEV) if inv_scale != 1.0 else None
    opt = FlatSGD(p, g, lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    q = torch.nn.Parameter(p.double().clone())
    ref = torch.optim.SGD([q], lr=0.05, momentum=momentum, weight_decay=wd, nesterov=nesterov)
    for _ in range(3):
        g.copy_(torch.randn(n, device=DEV, generator=gen))
        opt.step(inv_scale=inv_scale, found_inf=fi)
        q.grad = g.double() * inv_scale
        ref.step()
    torch.cuda.synchronize()
    assert fi is None or fi.item() == 0
    assert torch.allclose(p.double(), q.detach(), rtol=1e-5, atol=1e-6), (p.double() - q.detach()).abs().max().item()
    assert torch.allclose(opt.buf.double(), ref.state[q]["momentum_buffer"], rtol=1e-5, atol=1e-6)


def _gather_ref(rows, normalize):
    ref = rows.double()
    if normalize:
        ref = (ref - ref.mean(1, keepdim=True)) / (ref.std(1, unbiased=False, keepdim=True) + 1e-8)
    return ref


def _gather_check(x, idx, B, normalize):
    """gather_rows (fp32 and bf16 outputs) against float64 at test_gather_rows's tolerances."""
    from crossscale_ecg.ops.gather import gather_rows
    rows = x[idx.long()] if idx is not None else x[:B]
    ref = _gather_ref(rows, normalize)
    out = gather_rows(x, idx, batch=B, normalize=normalize)
    outb = gather_rows(x, idx, batch=B, normalize=normalize, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert out.shape == (B, x.shape[1]) and torch.isfinite(out).all()
    assert torch.allclose(out.double(), ref, atol=1e-5, rtol=1e-5), (out.double() - ref).abs().max().item()
    assert torch.allclose(outb.double(), ref, atol=3e-2 * max(1, ref.abs().max().item()), rtol=1e-2)
    return out, outb


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("L", [1, 63, 333, 502])
def test_gather_rows_short_and_odd_rows(L, B, normalize):
    """Rows shorter than a wave (L = 1, 63), odd (333) and with L % 4 != 0 (502: no 16-byte path); fewer rows than the
    four waves of a block, and one row past them."""
    torch.manual_seed(L + B)
    x = torch.randn(37, L, device=DEV) * 3 + 1
    idx = torch.randperm(37, device=DEV)[:B].int()
    _gather_check(x, idx, B, normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("L,lo", [(500, 4), (500, 1), (333, 3)])
def test_gather_rows_strided_and_misaligned_source(L, lo, normalize):
    """The source is a column slice of a wider tensor whose other columns hold 1e30 (ldx > L: a read past the row's
    L values shows at once); lo = 4 keeps the slice 16-byte aligned on every fourth row only, lo = 1 (x[:, 1:]) starts
    it 4 bytes past a 16-byte boundary with L % 4 == 0, where only the alignment test keeps the kernel off its
    16-byte loads.  With and without an index (idx=None gathers rows 0 .. B-1)."""
    torch.manual_seed(L + lo)
    wide = torch.full((40, lo + L + (0 if lo == 1 else 7)), 1e30, device=DEV)
    wide[:, lo:lo + L] = torch.randn(40, L, device=DEV) * 3 + 1
    x = wide[:, lo:lo + L]
    assert x.stride(0) > L or lo == 1
    idx = torch.randperm(40, device=DEV)[:9].int()
    _gather_check(x, idx, 9, normalize)
    _gather_check(x, None, 6, normalize)
    _gather_check(x, None, 40, normalize)  # batch omitted == every row
    from crossscale_ecg.ops.gather import gather_rows
    assert torch.equal(gather_rows(x, None, normalize=normalize), gather_rows(x, None, batch=40, normalize=normalize))


@pytest.mark.parametrize("L", [63, 333, 500, 502])
@pytest.mark.parametrize("c", [1.7, 0.1, -0.37, 3.0])
def test_gather_rows_constant_row_normalizes_to_zero(L, c):
    """A constant window (a flat-line lead) has variance 0: its z-score is exactly 0, finite, in fp32 and bf16 - also
    for values whose fp32 sum over L samples is not exact (1.7, 0.1, -0.37), next to ordinary rows that stay within
    the float64 tolerance."""
    torch.manual_seed(L)
    x = torch.randn(8, L, device=DEV) * 3 + 1
    x[2] = c
    idx = torch.tensor([5, 2, 0], dtype=torch.int32, device=DEV)
    out, outb = _gather_check(x, idx, 3, True)
    assert torch.all(out[1] == 0) and torch.all(outb[1] == 0)
