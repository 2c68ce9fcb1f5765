"""Argument order of the step and reduce kernels (their first 14 argument dwords are preloaded into SGPRs, so the
kernels' parameter lists are ordered for that and the launchers pass them in that order).  A launcher that put a value
in the wrong slot would still run, so every argument is made to matter here: a shuffled ``idx``, a shard pitch
different from the window length, labels that differ from sample to sample, weight decay with and without nesterov,
a slab pitch larger than P + 1 and a loss accumulator.  A 3-step round - enqueued and as a captured graph, so the
packed-row kernel, both reduce kernels' gather blocks and the SGD epilogue all run - must equal, bit for bit, the same
three steps issued one at a time through ``ecg_tiny_step_grads`` + ``ecg_slab_reduce_sgd`` (the unpacked, LDS-building
kernel, no gather) at the same forced wave count.  No tolerance except in the forward case."""
import ctypes as C

import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

pytestmark = pytest.mark.gpu

B, N, STEPS = 5, 16, 3
LR, MOMENTUM, WD = 1e-2, 0.9, 1e-2
WAVES = {8: 8, 36: 16, 500: 16}  # forced wave count per window length (both kernels of each family are covered)


def _case(L, nc, seed):
    """Dataset with pitch L + 4, labels cycling through the classes, a shuffled [STEPS][B] index table, weights and a
    non-zero momentum."""
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    xbuf = torch.randn(N, L + 4, generator=g).to(dev)
    y = (torch.arange(N) % nc).to(torch.int32).to(dev)
    idx = torch.stack([torch.randperm(N, generator=g)[:B] for _ in range(STEPS)]).to(torch.int32).to(dev)
    assert not torch.equal(idx[0].cpu(), torch.arange(B, dtype=torch.int32)) and y[idx[0].long()].unique().numel() > 1
    torch.manual_seed(seed)
    params = TinyECG(num_classes=nc).to(dev).flatten_parameters().detach().clone()
    mom = (0.01 * torch.randn(params.numel(), generator=g)).to(dev)
    return dev, xbuf, y, idx, params, mom


class _State:
    def __init__(self, dev, params, mom, nc):
        self.P = num_params(nc)
        self.stride = (self.P + 1 + 63) // 64 * 64 + 64  # larger than P + 1 and than the trainer's own pitch
        self.params, self.mom = params.clone(), mom.clone()
        self.slab = torch.zeros(B, self.stride, device=dev)
        self.loss = torch.zeros(1, device=dev)
        self.dp_scale = torch.zeros(B, device=dev)
        self.dp_step = torch.zeros(1, dtype=torch.int64, device=dev)

    def result(self):
        torch.cuda.synchronize()
        return self.params.clone(), self.mom.clone(), self.loss.clone()


def _round(mode, L, nc, nesterov, case, dp=None):
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import new_wprep
    lib = _lib.kernels()
    dev, xbuf, y, idx, params, mom = case
    st = _State(dev, params, mom, nc)
    wprep = new_wprep(dev)
    xg = torch.zeros(lib.ecg_tiny_gather_floats(L, B), device=dev)
    yg = torch.zeros(2 * B, dtype=torch.int32, device=dev)
    xbg = torch.zeros(lib.ecg_tiny_gather_halfs(L, B), dtype=torch.bfloat16, device=dev)
    clip, sigma, seed = dp or (0.0, 0.0, 0)
    r = _lib.TinyRound(X=xbuf.data_ptr(), ldx=xbuf.stride(0), idx=idx.data_ptr(), Y=y.data_ptr(),
                       params=st.params.data_ptr(), mom=st.mom.data_ptr(), slab=st.slab.data_ptr(),
                       loss_acc=st.loss.data_ptr(), wprep=wprep.data_ptr(), xg=xg.data_ptr(), yg=yg.data_ptr(), L=L,
                       nc=nc, slab_stride=st.stride, B=B, steps=STEPS, lr=LR, momentum=MOMENTUM, wd=WD,
                       nesterov=int(nesterov), prec=0, dp_clip=clip, dp_sigma=sigma, dp_seed=seed,
                       dp_scale=st.dp_scale.data_ptr(), dp_step=st.dp_step.data_ptr(), xbg=xbg.data_ptr())
    stream = _lib.stream_ptr(dev)
    if mode == "enqueue":
        _lib.check(lib.ecg_tiny_round_enqueue(C.byref(r), stream), "ecg_tiny_round_enqueue")
        return st.result()
    h = C.c_void_p()
    torch.cuda.synchronize()
    _lib.check(lib.ecg_tiny_round_capture(C.byref(h), C.byref(r)), "ecg_tiny_round_capture")
    try:
        _lib.check(lib.ecg_round_graph_launch(h, stream), "ecg_round_graph_launch")
        return st.result()
    finally:
        lib.ecg_round_graph_destroy(h)


def _one_at_a_time(L, nc, nesterov, case, dp=None):
    from crossscale_ecg.ops import _lib
    lib = _lib.kernels()
    dev, xbuf, y, idx, params, mom = case
    st = _State(dev, params, mom, nc)
    stream = _lib.stream_ptr(dev)
    for s in range(STEPS):
        _lib.check(lib.ecg_tiny_step_grads(xbuf.data_ptr(), L, xbuf.stride(0), idx[s].data_ptr(), y.data_ptr(),
                                           st.params.data_ptr(), nc, st.slab.data_ptr(), st.stride, B, 1.0 / B, 0, None,
                                           stream), "ecg_tiny_step_grads")
        if dp is None:
            _lib.check(lib.ecg_slab_reduce_sgd(st.slab.data_ptr(), B, st.stride, st.P, st.params.data_ptr(),
                                               st.mom.data_ptr(), None, st.loss.data_ptr(), LR, MOMENTUM, WD,
                                               int(nesterov), 1, None, stream), "ecg_slab_reduce_sgd")
        else:
            clip, sigma, seed = dp
            _lib.check(lib.ecg_slab_reduce_dp_sgd(st.slab.data_ptr(), B, st.stride, st.P, st.params.data_ptr(),
                                                  st.mom.data_ptr(), None, st.loss.data_ptr(), LR, MOMENTUM, WD,
                                                  int(nesterov), 1, None, clip, sigma, seed, st.dp_scale.data_ptr(),
                                                  st.dp_step.data_ptr(), stream), "ecg_slab_reduce_dp_sgd")
    return st.result()


def _compare(L, nc, nesterov, dp=None):
    from crossscale_ecg.ops import _lib
    lib = _lib.kernels()
    case = _case(L, nc, seed=1000 * L + 10 * nc + int(nesterov))
    prev = lib.ecg_tiny_force_waves(WAVES[L])
    try:
        ref = _one_at_a_time(L, nc, nesterov, case, dp)
        outs = {mode: _round(mode, L, nc, nesterov, case, dp) for mode in ("enqueue", "graph")}
    finally:
        lib.ecg_tiny_force_waves(prev)
    assert all(torch.isfinite(t).all() for t in ref) and not torch.equal(ref[0], case[4]) and ref[2].item() > 0
    for mode, out in outs.items():
        assert torch.equal(out[0], ref[0]), f"{mode}: weights differ by {(out[0] - ref[0]).abs().max().item()}"
        assert torch.equal(out[1], ref[1]), f"{mode}: momentum differs by {(out[1] - ref[1]).abs().max().item()}"
        assert torch.equal(out[2], ref[2]), f"{mode}: loss {out[2].item()} != {ref[2].item()}"


@pytest.mark.parametrize("nesterov", [False, True])
@pytest.mark.parametrize("nc", [2, 5])
@pytest.mark.parametrize("L", [8, 36, 500])
def test_round_equals_steps_issued_one_at_a_time(L, nc, nesterov):
    _compare(L, nc, nesterov)


def test_dp_round_equals_steps_issued_one_at_a_time():
    _compare(36, 5, True, dp=(1.0, 0.5, 0x1234_5678_9ABC))


def test_forward_with_pitched_rows_matches_torch():
    """MODE 1 shares the reordered parameter list: logits of shuffled, pitched rows against the torch model, at the
    tolerance of tests/test_fused_tiny_gpu.py::test_forward_matches_torch (bf16: 2e-2 of the largest logit)."""
    from crossscale_ecg.ops.fused_tiny import tiny_forward
    L, nc = 36, 5
    dev, xbuf, y, idx, params, _ = _case(L, nc, seed=7)
    model = TinyECG(num_classes=nc).to(dev)
    flat = model.flatten_parameters()
    flat.data.copy_(params)
    x = xbuf[:, :L]
    assert x.stride(0) == L + 4
    ref = model(x[idx[0].long()].unsqueeze(1))
    for prefrag in (True, False):
        out = tiny_forward(flat, x, idx[0].contiguous(), B, nc, precision="bf16", prefrag=prefrag)
        torch.cuda.synchronize()
        err = (out - ref).abs().max().item()
        scale = ref.abs().max().item() + 1e-3
        assert err / scale < 2e-2, f"prefrag={prefrag}: max err {err} (scale {scale})"
