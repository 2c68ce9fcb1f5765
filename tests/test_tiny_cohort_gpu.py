"""Cohorts of virtual clients on the fused TinyECG kernels: one cohort round (one step launch and one reduce launch per
step for M clients) against M single-client rounds of the existing entry point, bitwise; graph replay against
enqueue; the fan-out and the mean; the trainer; the eager reference; argument checks.

Shapes (unless a test says otherwise): M = 3 clients of B = 5 windows, S = 3 steps (the LDS-built step 0, then both
ping-pong buffers), L in {500, 100, 99} (16 waves; 8 waves with the 16-byte gather; 8 waves with the element gather),
nc in {2, 5}, N = 64 windows with distinct content, momentum 0.9."""
import ctypes as C

import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

import cohort_harness
from cohort_harness import LR, MU, N, WD, _data, _lib, _table

pytestmark = pytest.mark.gpu

CANARY = 1234.5


def Cohort(x, y32, nc, M, B, S, precision, table, w=None, m=None, glob=None, fanout=0, momentum=MU):
    """The harness's round without a fan-out by default and with the clients' buffers, padding included, on CANARY."""
    return cohort_harness.Cohort(x, y32, nc, M, B, S, precision, table, glob, fanout=fanout, w=w, m=m,
                                 momentum=momentum, pad=CANARY)


def _weights(nc, M, seed=1):
    """(global [P], per-client weights [M, P], per-client momenta [M, P]): distinct per client."""
    torch.manual_seed(seed)
    flat = torch.cat([p.detach().reshape(-1) for p in TinyECG(num_classes=nc).parameters()]).cuda()
    g = torch.Generator().manual_seed(seed + 100)
    P = flat.numel()
    w = flat[None, :] + 0.05 * torch.randn(M, P, generator=g).cuda()
    m = 0.01 * torch.randn(M, P, generator=g).cuda()
    return flat, w, m


def _single_round(x, y32, nc, B, S, precision, table_c, w, m, momentum=MU):
    """One client's round through the existing ecg_tiny_round_enqueue: (params [P], mom [P], image, loss [1])."""
    from crossscale_ecg.ops.fused_tiny import prec_id, slab_stride
    L_ = _lib()
    lib = L_.kernels()
    dev, L = x.device, x.shape[1]
    P = num_params(nc)
    f32 = dict(dtype=torch.float32, device=dev)
    params, mom = torch.zeros((P + 63) // 64 * 64, **f32), torch.zeros((P + 63) // 64 * 64, **f32)
    params[:P], mom[:P] = w, m
    slab = torch.zeros((B, slab_stride(nc)), **f32)
    loss = torch.zeros(1, **f32)
    table_c = table_c.contiguous()
    wprep = xg = yg = xbg = None
    if precision == "bf16":
        wprep = torch.zeros(lib.ecg_tiny_wprep_bytes(), dtype=torch.uint8, device=dev)
        xg = torch.zeros(lib.ecg_tiny_gather_floats(L, B), **f32)
        yg = torch.zeros(2 * B, dtype=torch.int32, device=dev)
        xbg = torch.zeros(lib.ecg_tiny_gather_halfs(L, B), dtype=torch.bfloat16, device=dev)
    p = L_.ptr
    r = L_.TinyRound(X=x.data_ptr(), ldx=x.stride(0), idx=table_c.data_ptr(), Y=y32.data_ptr(), params=params.data_ptr(),
                     mom=mom.data_ptr(), slab=slab.data_ptr(), loss_acc=loss.data_ptr(), wprep=p(wprep), xg=p(xg),
                     yg=p(yg), L=L, nc=nc, slab_stride=slab.shape[1], B=B, steps=S, lr=LR, momentum=momentum, wd=WD,
                     nesterov=0, prec=prec_id(precision), dp_clip=0.0, dp_sigma=0.0, dp_seed=0, dp_scale=None,
                     dp_step=None, xbg=p(xbg))
    L_.check(lib.ecg_tiny_round_enqueue(C.byref(r), L_.stream_ptr(dev)), "ecg_tiny_round_enqueue")
    torch.cuda.synchronize()
    return params[:P], mom[:P], wprep, loss


def _assert_cohort_equals_single_rounds(L, nc, precision, M, B, S):
    dev, x, y32 = _data(L, nc)
    _, w, m = _weights(nc, M)
    table = _table(S, M * B)
    co = Cohort(x, y32, nc, M, B, S, precision, table, w, m, fanout=0).run()
    P = co.P
    for c in range(M):
        pc, mc, img, loss = _single_round(x, y32, nc, B, S, precision, table[:, c * B:(c + 1) * B], w[c], m[c])
        assert torch.equal(co.cparams[c, :P], pc), (c, "params")
        assert torch.equal(co.cmom[c, :P], mc), (c, "momentum")
        assert torch.equal(co.loss[c:c + 1], loss) and float(loss) > 0, (c, "loss")
        if precision == "bf16":
            assert torch.equal(co.image(c), img), (c, "image")
        assert not torch.equal(pc, w[c])
    # distinct starts stay distinct: no client trained on another client's weights
    assert not torch.equal(co.cparams[0, :P], co.cparams[1, :P])
    return co


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("nc", [2, 5])
@pytest.mark.parametrize("L", [500, 100, 99])
def test_cohort_round_equals_single_client_rounds_bitwise(L, nc, precision):
    """fanout = 0 from distinct per-client weights and momenta: a step-0 kernel that read client 0's weights for
    every client would pass after a fan-out, and fails here."""
    co = _assert_cohort_equals_single_rounds(L, nc, precision, M=3, B=5, S=3)
    # the mean of what the clients ended on, in ascending order
    P = co.P
    want = ((co.cparams[0, :P] + co.cparams[1, :P]) + co.cparams[2, :P]) * torch.tensor(1.0 / 3, dtype=torch.float32)
    assert torch.equal(co.glob, want)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replayed_twice_equals_two_enqueued_rounds_bitwise(precision):
    L_ = _lib()
    lib = L_.kernels()
    dev, x, y32 = _data(100, 2)
    glob, _, _ = _weights(2, 3)
    t0, t1 = _table(3, 15, seed=5), _table(3, 15, seed=6)
    a = Cohort(x, y32, 2, 3, 5, 3, precision, t0.clone(), glob=glob, fanout=1)
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(a.round)), "ecg_tiny_cohort_round_capture")
    try:
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        a.table.copy_(t1)  # refilled in place between the replays
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    b = Cohort(x, y32, 2, 3, 5, 3, precision, t0.clone(), glob=glob, fanout=1).run()
    after_one = b.glob.clone()
    b.table.copy_(t1)
    b.run()
    assert not torch.equal(after_one, b.glob) and not torch.equal(after_one, glob)
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u, v)


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_fanout_mean_and_padding(precision):
    dev, x, y32 = _data(99, 5)
    nc, M, B, S = 5, 3, 5, 3
    glob, _, _ = _weights(nc, M)
    table = _table(S, M * B)
    a = Cohort(x, y32, nc, M, B, S, precision, table, glob=glob, fanout=1).run()
    P = a.P
    # the fan-out == an explicit copy of the global weights and zero momenta, then the same round without it
    b = Cohort(x, y32, nc, M, B, S, precision, table, glob=glob, fanout=0)
    for c in range(M):
        b.cparams[c, :P] = glob
        b.cmom[c, :P] = 0.0
    b.run()
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u, v)
    # ... and the mean == the fp32 loop in ascending client order
    s = a.cparams[0, :P].clone()
    for c in range(1, M):
        s = s + a.cparams[c, :P]
    assert torch.equal(a.glob, s * torch.tensor(1.0 / M, dtype=torch.float32)) and not torch.equal(a.glob, glob)
    # the pstride - P padding floats of weights and momenta are untouched by every kernel of the round
    assert a.ps > P
    assert bool((a.cparams[:, P:] == CANARY).all()) and bool((a.cmom[:, P:] == CANARY).all())
    # momenta are zero after the fan-out: one step at lr = 0 leaves mom = momentum * mom_0 + d, and from the canary
    # momenta the fan-out found it gives what explicit zeros give
    z = Cohort(x, y32, nc, M, B, 1, precision, table, glob=glob, fanout=1, momentum=MU)
    z.round.lr = 0.0
    z.run()
    assert torch.equal(z.cparams[:, :P], glob[None, :].expand(M, P))  # lr = 0: the fanned-out weights themselves
    zz = Cohort(x, y32, nc, M, B, 1, precision, table, glob=glob, fanout=0, momentum=MU)
    zz.round.lr = 0.0
    zz.cparams[:, :P] = glob
    zz.cmom[:, :P] = 0.0
    zz.run()
    assert torch.equal(z.cmom[:, :P], zz.cmom[:, :P])  # as from explicit zeros, not from the canary


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_cohort_of_one_equals_a_fused_tiny_trainer_round(precision):
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    dev, x, y32 = _data(100, 2)
    torch.manual_seed(3)
    model = TinyECG().to(dev)
    tr = FusedTinyTrainer(model, x, y32.long(), 5, 3, lr=LR, momentum=MU, weight_decay=WD, seed=11,
                          precision=precision, use_graph=False)
    P = tr.P
    start = tr.params[:P].clone()
    tr.run_round()
    torch.cuda.synchronize()
    co = Cohort(x, y32, 2, 1, 5, 3, precision, tr.idx_table.clone(), glob=start, fanout=1).run()
    assert torch.equal(co.glob, tr.params[:P]) and torch.equal(co.cparams[0, :P], co.glob)
    assert torch.equal(co.cmom[0, :P], tr.mom[:P]) and torch.equal(co.loss, tr.loss_acc)
    if precision == "bf16":
        assert torch.equal(co.image(0), tr.wprep)
    tr.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_more_than_one_wave_of_workgroups(precision):
    """M = 9 clients of B = 32 windows: 288 workgroups on 256 CUs."""
    _assert_cohort_equals_single_rounds(500, 2, precision, M=9, B=32, S=2)


# 5 ---------------------------------------------------------------------------------------------------------------
def _trainer(x, y32, precision, seed=7, use_graph=True, clients=4, cohort=3, model_seed=3):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    torch.manual_seed(model_seed)
    model = TinyECG().to(x.device)
    return FusedCohortTrainer(model, x, y32.long(), 5, 3, clients=clients, cohort=cohort, lr=LR, momentum=MU,
                              weight_decay=WD, seed=seed, use_graph=use_graph, precision=precision)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_trainer_round_prepare_evaluate_and_seeds(precision):
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, precision)
    P = tr.P
    start = tr.params.clone()
    tr.prepare([3])  # warms both graphs, rolls back
    assert torch.equal(tr.params, start) and tr.cohort_round == 0 and tr.steps_done == 0
    tr.run_round()
    torch.cuda.synchronize()
    assert tr.cohort_round == 1 and tr.round_clients == tr.sampler.clients_of(0) and len(set(tr.round_clients)) == 3
    # ... equals the native round it describes
    co = Cohort(x, y32, 2, 3, 5, 3, precision, tr.idx_table.clone(), glob=start[:P], fanout=1).run()
    assert torch.equal(co.glob, tr.params[:P]) and not torch.equal(co.glob, start[:P])
    assert torch.equal(co.loss, tr.loss_acc)
    assert abs(tr.avg_loss() - float(co.loss.sum()) / (3 * 5 * 3)) < 1e-6 and tr.avg_loss() > 0
    # evaluate() leaves the training state bitwise untouched
    state = [tr.params, tr.cparams, tr.cmom, tr.loss_acc, tr.idx_table, tr.idx_stage] + \
        ([tr.wprep] if tr.wprep is not None else [])
    snap = [t.clone() for t in state]
    res = tr.evaluate()
    torch.cuda.synchronize()
    assert res.count == N and res.loss > 0
    assert all(torch.equal(u, v) for u, v in zip(state, snap)) and tr.cohort_round == 1
    # same seed: identical weights after 2 rounds (graph vs enqueue too); another seed: other cohorts
    tr.run_round()
    twin = _trainer(x, y32, precision, use_graph=False)
    twin.run_round()
    twin.run_round()
    torch.cuda.synchronize()
    assert torch.equal(tr.params, twin.params) and tr.round_clients == twin.round_clients
    other = _trainer(x, y32, precision, seed=8, clients=12)
    same = _trainer(x, y32, precision, seed=7, clients=12)
    assert any(other.sampler.clients_of(r) != same.sampler.clients_of(r) for r in range(8))
    for t in (tr, twin, other, same):
        t.close()
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    with pytest.raises(ValueError, match="DP-SGD"):
        FusedCohortTrainer(TinyECG().to(dev), x, y32.long(), 5, 3, clients=4, dp_clip=1.0)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_fp32_trainer_round_against_the_torch_cohort_reference():
    """One fp32 FusedCohortTrainer round vs one TorchCohortTrainer round on the same tables: relative l2 difference
    of the global weights below 1e-5, the bound of tests/test_fused_tiny_gpu.py's fp32 fused-vs-torch round
    (test_train_step_and_graph_match_torch_sgd)."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    dev, x, y32 = _data(500, 2)
    tr = _trainer(x, y32, "fp32")
    torch.manual_seed(3)
    ref_model = TinyECG().to(dev)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), 5, 3, clients=4, cohort=3, lr=LR, momentum=MU, weight_decay=WD,
                             amp_dtype=None, seed=7)
    P = tr.P
    assert torch.equal(tr.params[:P], torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()]))
    tr.run_round()
    ref.run_round(3)
    torch.cuda.synchronize()
    assert torch.equal(tr.idx_table, ref.table) and tr.round_clients == ref.round_clients
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    print(f"fp32 cohort round, fused vs torch: relative l2 difference {rel:.3e}")
    assert rel < 1e-5, rel
    assert abs(tr.avg_loss() - ref.avg_loss()) < 1e-4
    tr.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_argument_checks(precision):
    dev, x, y32 = _data(100, 2)
    glob, _, _ = _weights(2, 3)
    table = _table(3, 15)

    def fresh():
        return Cohort(x, y32, 2, 3, 5, 3, precision, table, glob=glob, fanout=1)

    lib = _lib().kernels()
    bad = 1  # kBadArg
    assert C.sizeof(_lib().TinyCohortRound) == lib.ecg_tiny_cohort_round_sizeof()
    ps, ws = lib.ecg_tiny_cohort_param_stride(2), lib.ecg_tiny_cohort_wprep_stride()
    assert ps >= num_params(2) and ps % 64 == 0 and ws >= lib.ecg_tiny_wprep_bytes() and ws % 16 == 0
    for field, value in [("M", 0), ("M", -1), ("steps", 0), ("X", None), ("Y", None), ("idx", None), ("params", None),
                         ("slab", None), ("global_params", None), ("mom", None), ("prec", 2)]:
        c = fresh()
        setattr(c.round, field, value)
        assert c.enqueue() == bad, field
    c = fresh()  # ... a momentum buffer is only needed with momentum
    c.round.mom, c.round.momentum = None, 0.0
    assert c.enqueue() == 0
    if precision == "bf16":  # a bf16 round without (all of) its gather buffers
        for field in ("wprep", "xg", "yg", "xbg"):
            c = fresh()
            setattr(c.round, field, None)
            assert c.enqueue() == bad, field
    else:  # fp32 rounds use none of them
        donor = Cohort(x, y32, 2, 3, 5, 3, "bf16", table, glob=glob, fanout=1)
        for field in ("wprep", "xg", "yg", "xbg"):
            c = fresh()
            setattr(c.round, field, getattr(donor, field).data_ptr())
            assert c.enqueue() == bad, field
    g = C.c_void_p()
    c = fresh()
    c.round.M = 0
    assert lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == bad and not g.value
    assert lib.ecg_tiny_cohort_round_capture(None, C.byref(fresh().round)) == bad
    torch.cuda.synchronize()
