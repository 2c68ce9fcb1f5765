"""DP-SGD on the fused TinyECG kernels: clip factors, the clipped and noised reduce, the Philox noise, DP rounds
(graph == enqueue, counter, prepare, fused fp32 == torch backend), argument checks, and the DP-off default.

Shapes: B = 37 runs only the reduce's tail row loop, B = 273 one unrolled 256-row chunk plus a tail; nc = 2 / 5 give
P + 1 = 1459 / 1510 columns, both ragged against the 32 columns of a reduce block and the 256 columns of a
clip-factor pass; L = 64 (16-byte gather rows) and L = 61 (scalar gather rows, rounds only)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.utils import philox

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SHAPES = [(37, 2), (273, 5), (37, 5), (273, 2)]


def _setup(B, L=64, N=1024, nc=2, seed=0):
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, L, generator=g).to(dev)
    y = torch.randint(0, nc, (N,), generator=g).to(dev)
    torch.manual_seed(seed)
    model = TinyECG(num_classes=nc).to(dev)
    idx = torch.randperm(N, generator=g)[:B].to(torch.int32).to(dev)
    return dev, x, y, model, idx


def _counter(dev, t=0):
    return torch.full((1,), t, dtype=torch.int64, device=dev)


@functools.lru_cache(maxsize=None)
def _case(B, nc):
    """One step's slab (read-only, shared by the tests below), its float64 row norms, the clip norm between the two
    middle norms (the nearest gap of at least 1e-3 relative) and the float64 clip factors."""
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads, labels_int32
    dev, x, y, model, idx = _setup(B, nc=nc)
    slab = tiny_step_grads(model.flatten_parameters(), x, labels_int32(y, nc), idx, B, nc)
    torch.cuda.synchronize()
    P = num_params(nc)
    n64 = B * slab[:, :P].double().norm(dim=1)
    s = n64.sort().values
    mid = B // 2
    order = sorted(range(1, B), key=lambda k: abs(k - mid))  # pairs (k - 1, k), outward from the middle
    k = next(k for k in order if (s[k] - s[k - 1]) / s[k] >= 1e-3)
    gap = float((s[k] - s[k - 1]) / s[k])
    clip = float((s[k - 1] * s[k]).sqrt())
    c64 = torch.clamp(clip / n64, max=1.0)
    return dict(dev=dev, slab=slab, P=P, n64=n64, clip=clip, gap=gap, c64=c64, k=k)


@pytest.mark.parametrize("B,nc", SHAPES)
def test_row_scales_match_float64(B, nc):
    from crossscale_ecg.ops.fused_tiny import dp_reduce_slab
    cs = _case(B, nc)
    assert cs["gap"] >= 1e-3, cs["gap"]
    step = _counter(cs["dev"], 41)
    _, _, scale = dp_reduce_slab(cs["slab"], cs["clip"], 0.0, SEED, step, nc)
    torch.cuda.synchronize()
    rel = ((scale.double() - cs["c64"]).abs() / cs["c64"]).max().item()
    clipped = int((scale < 1).sum())
    print(f"row scales B={B} nc={nc}: worst relative error {rel:.3e}, {clipped}/{B} rows clipped, gap {cs['gap']:.2e}")
    assert rel <= 1e-4  # worst-case fp32 accumulation over 1,458 squares: 1458 * 2^-24 = 8.7e-5
    assert torch.equal(scale < 1, cs["c64"] < 1) and clipped == B - cs["k"]  # the rows above the chosen gap
    assert step.item() == 42  # one step, one advance
    # a sample with a zero gradient is not scaled (n_b == 0 -> 1), whatever the clip norm
    z = cs["slab"].clone()
    z[3, :cs["P"]] = 0
    _, _, scale0 = dp_reduce_slab(z, 0.5 * float(cs["n64"].min()), 0.0, SEED, step, nc)
    assert scale0[3].item() == 1.0 and int((scale0 < 1).sum()) == B - 1


@pytest.mark.parametrize("B,nc", SHAPES)
def test_clipped_sum_matches_float64_and_loss_is_untouched(B, nc):
    from crossscale_ecg.ops.fused_tiny import dp_reduce_slab, reduce_slab
    cs = _case(B, nc)
    P = cs["P"]
    grad, loss, _ = dp_reduce_slab(cs["slab"], cs["clip"], 0.0, SEED, _counter(cs["dev"]), nc)
    _, loss_plain = reduce_slab(cs["slab"], nc)
    torch.cuda.synchronize()
    terms = cs["c64"][:, None] * cs["slab"][:, :P].double()
    err = (grad.double() - terms.sum(0)).abs()
    bound = 1e-4 * terms.abs().sum(0)
    print(f"clipped sum B={B} nc={nc}: worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()
    assert torch.equal(loss, loss_plain) and loss.item() > 0


def _reduce_sgd(cs, nc, dp, nesterov, wd):
    """One reduce + SGD (momentum 0.9, lr 0.05) on fresh copies of the same weights, momentum and image."""
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import new_wprep
    dev, slab, P = cs["dev"], cs["slab"], cs["P"]
    g = torch.Generator(device="cpu").manual_seed(9)
    params = torch.randn(P, generator=g).to(dev)
    mom = torch.randn(P, generator=g).to(dev)
    grad = torch.zeros(P, device=dev)
    loss = torch.zeros(1, device=dev)
    wprep = new_wprep(dev)
    lib = _lib.kernels()
    head = (slab.data_ptr(), slab.shape[0], slab.stride(0), P, params.data_ptr(), mom.data_ptr(), grad.data_ptr(),
            loss.data_ptr(), 0.05, 0.9, wd, nesterov, 1, wprep.data_ptr())
    if dp:
        scale = torch.zeros(slab.shape[0], device=dev)
        st = lib.ecg_slab_reduce_dp_sgd(*head, 1e30, 0.0, SEED, scale.data_ptr(), _counter(dev).data_ptr(),
                                        _lib.stream_ptr(dev))
        assert st == 0 and bool((scale == 1).all())
    else:
        assert lib.ecg_slab_reduce_sgd(*head, _lib.stream_ptr(dev)) == 0
    torch.cuda.synchronize()
    return grad, params, mom, wprep, loss


@pytest.mark.parametrize("B,nc,nesterov,wd", [(37, 2, 0, 0.0), (273, 5, 1, 1e-3)])
def test_no_clip_no_noise_is_bitwise_the_plain_reduce(B, nc, nesterov, wd):
    cs = _case(B, nc)
    plain = _reduce_sgd(cs, nc, False, nesterov, wd)
    dp = _reduce_sgd(cs, nc, True, nesterov, wd)
    for name, a, b in zip(("grad", "params", "momentum", "wprep", "loss"), plain, dp):
        assert torch.equal(a, b), name
    assert plain[3].any()  # the image was written


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
def test_noise_matches_numpy_philox(seed):
    from crossscale_ecg.ops.fused_tiny import dp_noise
    dev = torch.device("cuda:0")
    for t in (0, 1, 2 ** 32 + 5):
        for P in (1458, 1509):
            z = dp_noise(P, seed, t, dev).double().cpu().numpy()
            ref = philox.normal(seed, t, P)
            err = np.abs(z - ref).max()
            print(f"noise seed={seed:#x} t={t} P={P}: max |z - ref| = {err:.3e}")
            assert err <= 1e-5 and np.abs(z).max() <= 5.77


@pytest.mark.parametrize("B,nc", [(37, 2), (273, 5)])
def test_noised_gradient_adds_scaled_z_of_the_current_counter(B, nc):
    from crossscale_ecg.ops.fused_tiny import dp_reduce_slab
    cs = _case(B, nc)
    sigma, clip, t = 1.3, cs["clip"], 7
    g0, _, _ = dp_reduce_slab(cs["slab"], clip, 0.0, SEED, _counter(cs["dev"], t), nc)
    step = _counter(cs["dev"], t)
    g1, loss1, _ = dp_reduce_slab(cs["slab"], clip, sigma, SEED, step, nc)
    torch.cuda.synchronize()
    nscale = sigma * clip / B
    want = nscale * torch.from_numpy(philox.normal(SEED, t, cs["P"])).to(cs["dev"])
    _, e = torch.frexp(g1.abs())  # |g1| = m * 2^e with m in [0.5, 1): one ulp is 2^(e - 24)
    ulp = torch.ldexp(torch.ones_like(g1), e - 24).double()
    err = (g1.double() - g0.double() - want).abs()
    print(f"noised update B={B} nc={nc}: worst error / (1e-5 nscale + ulp) {(err / (1e-5 * nscale + ulp)).max().item():.3e}")
    assert (err <= 1e-5 * nscale + ulp).all()
    assert step.item() == t + 1
    other = nscale * torch.from_numpy(philox.normal(SEED, t + 1, cs["P"])).to(cs["dev"])
    assert (g1.double() - g0.double() - other).abs().max() > 0.1 * nscale  # not the next step's draw


# ------------------------------------------------------------------------------------------------ rounds
def _median_norm(model, x, y, nc, B, precision):
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads, labels_int32
    idx = torch.arange(B, dtype=torch.int32, device=x.device)
    slab = tiny_step_grads(model.flatten_parameters(), x, labels_int32(y, nc), idx, B, nc, precision=precision)
    return float((B * slab[:, :num_params(nc)].double().norm(dim=1)).median())


def _trainer(B, L, nc, precision, graph, steps=3, sigma=1.1, **kw):
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    dev, x, y, model, _ = _setup(B, L=L, nc=nc)
    clip = _median_norm(model, x, y, nc, B, precision)
    tr = FusedTinyTrainer(model, x, y, B, steps, seed=21, precision=precision, use_graph=graph, dp_clip=clip,
                          dp_noise=sigma, dp_seed=SEED, **kw)
    return tr


def _state(tr):
    torch.cuda.synchronize()
    return tr.params.clone(), tr.mom.clone(), tr.avg_loss(), int(tr.dp_step.item()), tr.dp_scale.clone()


@pytest.mark.parametrize("B,L,nc,precision", [(273, 64, 5, "bf16"), (37, 61, 2, "bf16"), (37, 64, 2, "fp32")])
def test_dp_round_graph_equals_enqueue_bitwise(B, L, nc, precision):
    """Two 3-step rounds (the LDS-built first step, both gather buffers, the rewritten image; the second round
    continues the counter): graph replay == enqueued launches, bit for bit."""
    outs = []
    for graph in (True, False):
        tr = _trainer(B, L, nc, precision, graph)
        assert tr.dp and tr.prefrag == (precision == "bf16") and tr.gather == (precision == "bf16")
        tr.run_round(reset_loss=False)
        tr.run_round(reset_loss=False)
        outs.append(_state(tr))
        assert tr.dp_steps == 6 and outs[-1][3] == 6 and tr.steps_done == 6
        assert 0 < int((outs[-1][4] < 1).sum()) < B  # the last step clipped some rows and kept others
        tr.close()
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and torch.equal(a[4], b[4])


def test_second_round_continues_the_counter():
    """Round 2 draws steps 3..5 of the noise stream: resetting the counter to 0 before it gives other weights, and
    setting it to the value it already has changes nothing."""
    outs = []
    for reset_to in (None, 3, 0):
        tr = _trainer(37, 64, 2, "bf16", True)
        tr.run_round()
        if reset_to is not None:
            tr.set_dp_steps(reset_to)
        tr.run_round()
        outs.append(_state(tr))
        tr.close()
    assert torch.equal(outs[0][0], outs[1][0]) and outs[0][3] == outs[1][3] == 6
    assert not torch.equal(outs[0][0], outs[2][0]) and outs[2][3] == 3


def test_prepared_trainer_equals_unprepared_twin_bitwise():
    outs = []
    for prepared in (False, True):
        tr = _trainer(37, 64, 2, "bf16", True)
        if prepared:
            tr.prepare([3])
            torch.cuda.synchronize()
            assert tr.dp_step.item() == 0 and tr.dp_steps == 0  # the warm-up replays were rolled back
        tr.run_round(reset_loss=False)
        tr.run_round(reset_loss=False)
        outs.append(_state(tr))
        tr.close()
    a, b = outs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] == 6


class _ReplaySampler:
    """Feeds a recorded index table to ``TorchLocalTrainer.step``, one row per step."""

    def __init__(self, table):
        self.table, self.i = table, 0

    def fill(self, out):
        out.copy_(self.table[self.i:self.i + out.shape[0]])
        self.i += out.shape[0]
        return out


@pytest.mark.parametrize("B,L", [(37, 64), (273, 61)])
def test_fused_fp32_dp_round_matches_torch_backend(B, L):
    """A fused fp32 DP round == ``TorchLocalTrainer`` DP steps on the same batches with the same seed and counter
    (per-sample gradients from torch.func, noise from utils/philox.py).  Tolerance: the fused-fp32-vs-torch SGD
    trajectory bound of tests/test_fused_tiny_gpu.py (relative l2 error of the weights < 1e-5)."""
    from crossscale_ecg.train.local import TorchLocalTrainer
    tr = _trainer(B, L, 2, "fp32", True)
    ref = TinyECG().to(tr.device)
    ref.load_state_dict(tr.model.state_dict())
    tr.run_round()
    torch.cuda.synchronize()
    tt = TorchLocalTrainer(ref, tr.x, tr.y32.long(), B, lr=tr.lr, momentum=tr.momentum, amp_dtype=None, seed=21,
                           dp_clip=tr.dp_clip, dp_noise=tr.dp_noise, dp_seed=SEED)
    tt.sampler = _ReplaySampler(tr.idx_table.clone())
    tt.run_steps(3)
    got = tr.params[:num_params(2)]
    want = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
    rel = (got - want).norm().item() / want.norm().item()
    print(f"fused fp32 DP round vs torch backend B={B} L={L}: relative l2 error {rel:.3e}")
    assert rel < 1e-5, rel
    assert tt.dp_steps == tr.dp_steps == 3
    assert abs(tt.avg_loss() - tr.avg_loss()) < 1e-4
    tr.close()


# ------------------------------------------------------------------------------------------------ arguments
def test_check_round_rejects_bad_dp_arguments_and_launches_nothing():
    from crossscale_ecg.ops import _lib
    tr = _trainer(37, 64, 2, "bf16", False)
    tr.stage(3)
    torch.cuda.synchronize()
    lib = _lib.kernels()
    before = (tr.params.clone(), tr.mom.clone(), tr.slab.clone(), tr.dp_scale.clone())
    good = {k: getattr(tr._round, k) for k in ("dp_clip", "dp_sigma", "dp_scale", "dp_step")}
    bad = [dict(dp_clip=-1.0), dict(dp_sigma=-0.5), dict(dp_clip=0.0, dp_sigma=1.0), dict(dp_scale=None),
           dict(dp_step=None)]
    for change in bad:
        for k, v in {**good, **change}.items():
            setattr(tr._round, k, v)
        assert lib.ecg_tiny_round_enqueue(tr._round_of(3, tr.idx_stage), _lib.stream_ptr(tr.device)) == 1, change
        handle = C.c_void_p()
        assert lib.ecg_tiny_round_capture(C.byref(handle), tr._round_of(3, tr.idx_stage)) == 1, change
        assert not handle.value
    torch.cuda.synchronize()
    assert tr.dp_step.item() == 0
    # bit for bit: the slab is ``torch.empty`` and nothing has written it yet, so it may hold NaN patterns left by
    # whatever owned the memory before, which compare unequal to themselves as floats
    for a, b in zip(before, (tr.params, tr.mom, tr.slab, tr.dp_scale)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the stand-alone pair checks the same
    step = _counter(tr.device)
    args = (tr.slab.data_ptr(), tr.B, tr.stride, tr.P, None, None, tr.mom.data_ptr(), None, 0.0, 0.0, 0.0, 0, 0, None)
    for clip, sigma, scale, stp in ((0.0, 0.0, tr.dp_scale, step), (-1.0, 0.0, tr.dp_scale, step),
                                    (1.0, -1.0, tr.dp_scale, step), (1.0, 1.0, None, step),
                                    (1.0, 1.0, tr.dp_scale, None)):
        st = lib.ecg_slab_reduce_dp_sgd(*args, clip, sigma, SEED, _lib.ptr(scale), _lib.ptr(stp),
                                        _lib.stream_ptr(tr.device))
        assert st == 1, (clip, sigma)
    torch.cuda.synchronize()
    assert step.item() == 0 and torch.equal(before[1], tr.mom)
    # the restored description runs
    for k, v in good.items():
        setattr(tr._round, k, v)
    tr.launch_round(3)
    torch.cuda.synchronize()
    assert tr.dp_step.item() == 3 and not torch.equal(before[0], tr.params)
    tr.close()
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    dev, x, y, model, _ = _setup(16)
    for kw in (dict(dp_clip=-1.0), dict(dp_noise=-1.0), dict(dp_noise=1.0)):
        with pytest.raises(ValueError):
            FusedTinyTrainer(model, x, y, 16, 2, **kw)


def test_default_trainer_is_dp_off_and_ends_on_todays_bits():
    """A trainer built with the defaults has no DP state, describes a round with dp_clip == 0, and its captured
    round == ``tiny_step_grads`` + ``ecg_slab_reduce_sgd`` stepped by hand, bit for bit."""
    from crossscale_ecg.ops import _lib
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer, tiny_step_grads, new_wprep
    B, nc, steps = 37, 2, 3
    dev, x, y, model, _ = _setup(B, nc=nc)
    tr = FusedTinyTrainer(model, x, y, B, steps, seed=21)
    assert not tr.dp and tr.dp_step is None and tr.dp_scale is None and tr.dp_steps == 0
    assert tr._round.dp_clip == 0.0 and tr._round.dp_sigma == 0.0 and not tr._round.dp_scale and not tr._round.dp_step
    params, mom = tr.params.clone(), tr.mom.clone()
    tr.run_round()
    torch.cuda.synchronize()
    assert tr.dp_steps == 0 and tr.steps_done == steps
    slab = torch.empty_like(tr.slab)
    loss = torch.zeros(1, device=dev)
    wprep = new_wprep(dev)
    lib = _lib.kernels()
    for s in range(steps):
        tiny_step_grads(params, tr.x, tr.y32, tr.idx_table[s], B, nc, slab, wprep=wprep)
        st = lib.ecg_slab_reduce_sgd(slab.data_ptr(), B, tr.stride, tr.P, params.data_ptr(), mom.data_ptr(), None,
                                     loss.data_ptr(), tr.lr, tr.momentum, 0.0, 0, 1, None, _lib.stream_ptr(dev))
        assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(params, tr.params) and torch.equal(mom, tr.mom) and torch.equal(loss, tr.loss_acc)
    tr.close()
