"""FedProx in the fused TinyECG and cohort rounds: the prox reduce kernels against the definition
``d = gsum + wd * p + mu * (p - a)``, against the kernels of before (mu = 0, bitwise), the cohort form against M
single-client reduces, whole rounds (hand-stepped, graph replay against enqueue, the torch references) and the
argument checks.

Shapes: slabs of G in {1, 32, 256, 259} rows (the 256-row chunk of the reduce and its tail), nc in {2, 5} (P = 1458 at
nc = 2: a ragged last column block); rounds of S = 3 steps, B = 8 windows of L in {100, 99} out of N = 64."""
import ctypes as C

import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

import cohort_harness
from cohort_harness import N, _global as _flat, _lib as _L, _table

pytestmark = pytest.mark.gpu

LR, MOM, WD, MU = cohort_harness.LR, cohort_harness.MU, cohort_harness.WD, 0.1  # MU: the FedProx coefficient
GS = [1, 32, 256, 259]
OPTS = [(0.0, 0, 0.0), (MOM, 0, WD), (MOM, 1, WD)]  # (momentum, nesterov, weight decay)
BAD = 1  # kBadArg


def _stride(nc):
    from crossscale_ecg.ops.fused_tiny import slab_stride
    return slab_stride(nc)


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(shape, generator=g)).cuda()


def _reduce_inputs(G, nc, seed=0):
    """(slab [G, stride], params [P], mom [P], anchor [P]), random."""
    P = num_params(nc)
    return (_rand((G, _stride(nc)), seed), _rand(P, seed + 1, 0.3), _rand(P, seed + 2, 0.05), _rand(P, seed + 3, 0.3))


def _wprep(dev, M=1):
    L_ = _L()
    lib = L_.kernels()
    return torch.zeros(M * lib.ecg_tiny_cohort_wprep_stride() if M > 1 else lib.ecg_tiny_wprep_bytes(),
                       dtype=torch.uint8, device=dev)


def _prox_reduce(slab, P, params, mom, grad_out, loss, momentum, wd, nesterov, wprep, anchor, mu, lr=LR, apply=1):
    L_ = _L()
    return L_.kernels().ecg_slab_reduce_prox_sgd(
        slab.data_ptr(), slab.shape[0], slab.stride(0), P, L_.ptr(params), L_.ptr(mom), L_.ptr(grad_out), L_.ptr(loss),
        lr, momentum, wd, nesterov, apply, L_.ptr(wprep), L_.ptr(anchor), mu, L_.stream_ptr(slab.device))


def _cohort_prox_reduce(slab, G, M, P, cparams, cmom, loss, momentum, wd, nesterov, wprep, anchor, mu, lr=LR):
    L_ = _L()
    return L_.kernels().ecg_slab_reduce_cohort_prox_sgd(
        slab.data_ptr(), G, M, slab.stride(0), P, L_.ptr(cparams), L_.ptr(cmom), L_.ptr(loss), lr, momentum, wd,
        nesterov, L_.ptr(wprep), L_.ptr(anchor), mu, L_.stream_ptr(slab.device))


# 1 --------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("momentum,nesterov,wd", OPTS)
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nc", [2, 5])
def test_standalone_prox_reduce_against_the_definition_in_float64(nc, G, momentum, nesterov, wd):
    """The kernel's own fp32 column sums (``grad_out``) through the epilogue in float64.  Per element the error of
    ``params`` is within 8 * 2^-24 * (|p| + lr (1 + momentum) (|gsum| + wd |p| + mu (|p| + |a|) + momentum |m0|)) - at
    most eight roundings of intermediates bounded by that sum - and that of ``mom`` within 8 * 2^-24 of the inner sum.
    Worst measured fraction of the bound: 0.46 (params), 0.33 (mom)."""
    slab, p0, m0, a = _reduce_inputs(G, nc, seed=10 * G + nc)
    P = num_params(nc)
    params, mom = p0.clone(), m0.clone()
    gsum, loss = torch.zeros(P, device=slab.device), torch.zeros(1, device=slab.device)
    assert _prox_reduce(slab, P, params, mom, gsum, loss, momentum, wd, nesterov, None, a, MU) == 0
    torch.cuda.synchronize()
    # grad_out is the slab's column sum, the loss word column P's
    want_sum = slab.double().sum(0)
    assert torch.allclose(gsum.double(), want_sum[:P], rtol=0, atol=1e-5 * max(1.0, G ** 0.5))
    assert abs(float(loss) - float(want_sum[P])) < 1e-5 * max(1.0, G ** 0.5) * 4
    g64, p64, m64, a64 = gsum.double(), p0.double(), m0.double(), a.double()
    d = g64 + wd * p64 + MU * (p64 - a64)
    inner = g64.abs() + wd * p64.abs() + MU * (p64.abs() + a64.abs()) + momentum * m64.abs()
    if momentum != 0.0:
        bm = momentum * m64 + d
        d = d + momentum * bm if nesterov else bm
        err_m = (mom.double() - bm).abs()
        frac_m = float((err_m / (8 * 2.0 ** -24 * inner)).max())
        print(f"nc={nc} G={G} momentum={momentum} nesterov={nesterov}: mom worst fraction of the bound {frac_m:.3f}")
        assert frac_m <= 1.0
    else:
        assert torch.equal(mom, m0)  # not touched without momentum
    want = p64 - LR * d
    bound = 8 * 2.0 ** -24 * (p64.abs() + LR * (1 + momentum) * inner)
    frac = float(((params.double() - want).abs() / bound).max())
    print(f"nc={nc} G={G} momentum={momentum} nesterov={nesterov}: params worst fraction of the bound {frac:.3f}")
    assert frac <= 1.0
    # the proximal term is there: the same call with mu = 0 ends elsewhere
    plain = p0.clone()
    assert _prox_reduce(slab, P, plain, m0.clone(), None, None, momentum, wd, nesterov, None, a, 0.0) == 0
    torch.cuda.synchronize()
    assert not torch.equal(plain, params)


# 2 --------------------------------------------------------------------------------------------- mu = 0, bitwise
@pytest.mark.parametrize("momentum,nesterov,wd", OPTS[1:])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nc", [2, 5])
def test_mu_zero_through_the_prox_kernel_is_the_plain_reduce_bitwise(nc, G, momentum, nesterov, wd):
    L_ = _L()
    slab, p0, m0, a = _reduce_inputs(G, nc, seed=7 * G + nc)
    dev, P = slab.device, num_params(nc)
    out = []
    for prox in (False, True):
        params, mom, loss, img = p0.clone(), m0.clone(), torch.zeros(1, device=dev), _wprep(dev)
        if prox:
            st = _prox_reduce(slab, P, params, mom, None, loss, momentum, wd, nesterov, img, a, 0.0)
        else:
            st = L_.kernels().ecg_slab_reduce_sgd(slab.data_ptr(), G, slab.stride(0), P, params.data_ptr(),
                                                  mom.data_ptr(), None, loss.data_ptr(), LR, momentum, wd, nesterov, 1,
                                                  img.data_ptr(), L_.stream_ptr(dev))
        assert st == 0
        out.append((params, mom, img, loss))
    torch.cuda.synchronize()
    for u, v, what in zip(out[0], out[1], ("params", "mom", "image", "loss")):
        assert torch.equal(u, v), what
    assert not torch.equal(out[0][0], p0) and bool(out[0][2].any())


def Cohort(*args, prox_mu=0.0, with_prox_field=True, **kw):
    """The harness's round with ``prox_mu`` named, unless ``with_prox_field`` is False."""
    return cohort_harness.Cohort(*args, prox_mu=prox_mu if with_prox_field else None, **kw)


def _data(L, nc, seed=0):
    return cohort_harness._data(L, nc, seed)[1:]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("nc", [2, 5])
def test_mu_zero_through_the_cohort_prox_kernel_is_the_cohort_reduce_bitwise(nc, G, precision):
    """A one-step cohort round (prox_mu = 0: slab_reduce_cohort_sgd_kernel) leaves its gradient rows in the slab; the
    stand-alone cohort prox reduce with mu = 0 and a random anchor on those rows, from the same weights and momenta,
    ends on the round's weights, momenta, images and loss words."""
    M = 2
    x, y32 = _data(100, nc)
    flat = _flat(nc)
    P = flat.numel()
    w = flat[None, :] + _rand((M, P), 3, 0.05)
    m = _rand((M, P), 4, 0.01)
    co = Cohort(x, y32, nc, M, G, 1, precision, _table(1, M * G), flat, fanout=0, w=w, m=m).run()
    cparams, cmom = torch.zeros_like(co.cparams), torch.zeros_like(co.cmom)
    cparams[:, :P], cmom[:, :P] = w, m
    loss = torch.zeros(M, device=x.device)
    img = _wprep(x.device, 2) if precision == "bf16" else None
    assert _cohort_prox_reduce(co.slab, G, M, P, cparams, cmom, loss, MOM, WD, 0, img, _rand(P, 5), 0.0) == 0
    torch.cuda.synchronize()
    assert torch.equal(cparams, co.cparams) and torch.equal(cmom, co.cmom) and torch.equal(loss, co.loss)
    assert not torch.equal(cparams[:, :P], w)
    if precision == "bf16":
        assert torch.equal(img, co.wprep) and bool(img.any())


# 3 --------------------------------------------------------------------------------------------- cohort = M singles
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("nc", [2, 5])
def test_cohort_prox_reduce_equals_single_client_prox_reduces_bitwise(nc, M):
    G = 37
    L_ = _L()
    lib = L_.kernels()
    P, ps, ws = num_params(nc), lib.ecg_tiny_cohort_param_stride(nc), lib.ecg_tiny_cohort_wprep_stride()
    assert ps > P
    slab = _rand((M * G, _stride(nc)), 20 + nc)
    dev = slab.device
    w, m, a = _rand((M, P), 21, 0.3), _rand((M, P), 22, 0.05), _rand(P, 23, 0.3)
    cparams = torch.full((M, ps), float("nan"), device=dev)  # NaN in the padding: neither read nor written
    cmom = torch.full((M, ps), float("nan"), device=dev)
    cparams[:, :P], cmom[:, :P] = w, m
    loss, img = torch.zeros(M, device=dev), torch.zeros(M * ws, dtype=torch.uint8, device=dev)
    assert _cohort_prox_reduce(slab, G, M, P, cparams, cmom, loss, MOM, WD, 1, img, a, MU) == 0
    torch.cuda.synchronize()
    assert bool(cparams[:, P:].isnan().all()) and bool(cmom[:, P:].isnan().all())
    assert not bool(cparams[:, :P].isnan().any()) and not bool(cmom[:, :P].isnan().any())
    for c in range(M):
        pc, mc, lc, ic = w[c].clone(), m[c].clone(), torch.zeros(1, device=dev), _wprep(dev)
        assert _prox_reduce(slab[c * G:(c + 1) * G], P, pc, mc, None, lc, MOM, WD, 1, ic, a, MU) == 0
        torch.cuda.synchronize()
        assert torch.equal(cparams[c, :P], pc) and torch.equal(cmom[c, :P], mc), c
        assert torch.equal(loss[c:c + 1], lc) and torch.equal(img[c * ws:c * ws + ic.numel()], ic), c
    if M > 1:  # one anchor, distinct clients
        assert not torch.equal(cparams[0, :P], cparams[1, :P])


# 4 --------------------------------------------------------------------------------------------- rounds
def _tiny_trainer(L, precision, prox_mu, use_graph, seed=11, model_seed=3, nc=2, **kw):
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    x, y32 = _data(L, nc)
    torch.manual_seed(model_seed)
    model = TinyECG(num_classes=nc).cuda()
    return FusedTinyTrainer(model, x, y32.long(), 8, 3, lr=LR, momentum=MOM, weight_decay=WD, seed=seed,
                            precision=precision, use_graph=use_graph, prox_mu=prox_mu, **kw)


def _tiny_state(tr):
    return [t.clone() for t in (tr.params, tr.mom, tr.loss_acc) + ((tr.wprep,) if tr.wprep is not None else ())]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("L", [100, 99])
def test_trainer_round_ends_on_the_hand_stepped_bits(L, precision):
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads, new_wprep
    tr = _tiny_trainer(L, precision, MU, use_graph=False)
    assert tr._round.prox_mu == pytest.approx(MU) and tr._round.prox_snapshot == 1
    assert tr._round.prox_anchor == tr.prox_anchor.data_ptr() != tr.params.data_ptr()
    params, mom = tr.params.clone(), tr.mom.clone()
    anchor = params.clone()  # the snapshot the test takes
    tr.run_round()
    torch.cuda.synchronize()
    assert torch.equal(tr.prox_anchor, anchor)  # the round's first launch anchored it
    dev = tr.device
    slab, loss = torch.empty_like(tr.slab), torch.zeros(1, device=dev)
    wprep = new_wprep(dev) if precision == "bf16" else None
    for s in range(3):
        tiny_step_grads(params, tr.x, tr.y32, tr.idx_table[s], 8, 2, slab, precision=precision, wprep=wprep)
        assert _prox_reduce(slab, tr.P, params, mom, None, loss, MOM, WD, 0, None, anchor, MU) == 0
    torch.cuda.synchronize()
    assert torch.equal(params, tr.params) and torch.equal(mom, tr.mom) and torch.equal(loss, tr.loss_acc)
    # ... and not on the bits of the round without the proximal term
    plain = _tiny_trainer(L, precision, 0.0, use_graph=False)
    plain.run_round()
    torch.cuda.synchronize()
    assert torch.equal(plain.idx_table, tr.idx_table) and not torch.equal(plain.params, tr.params)
    tr.close()
    plain.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("L", [100, 99])
def test_trainer_graph_replayed_twice_equals_two_enqueued_rounds_bitwise(L, precision):
    """The second round is anchored on the first round's result: the snapshot is a node of the graph."""
    a = _tiny_trainer(L, precision, MU, use_graph=True)
    b = _tiny_trainer(L, precision, MU, use_graph=False)
    start = a.params.clone()
    a.prepare([3])  # warm-up replays write the anchor; every round derives it anew
    assert torch.equal(a.params, start)
    mids = []
    for t in (a, b):
        t.run_round()
        torch.cuda.synchronize()
        mids.append(t.params.clone())
        assert torch.equal(t.prox_anchor, start)
        t.run_round(reset_loss=False)
        torch.cuda.synchronize()
        assert torch.equal(t.prox_anchor, mids[-1]) and not torch.equal(mids[-1], start)
    assert len(a._graphs) == 2 and not b._graphs
    for u, v in zip(_tiny_state(a), _tiny_state(b)):
        assert torch.equal(u, v)
    a.close()
    b.close()


def _server_fields(P, dev, opt):
    f32 = dict(dtype=torch.float32, device=dev)
    kw = {}
    if opt:
        kw = dict(cdp_scale=torch.ones(3, **f32), cdp_norm=torch.zeros(3, **f32),
                  cdp_round=torch.zeros(1, dtype=torch.int64, device=dev), server_lr=0.05, server_opt=3, server_beta1=0.9,
                  server_beta2=0.99, server_tau=1e-3, server_m=torch.zeros(P, **f32), server_v=torch.full((P,), 1e-6, **f32))
    return kw


@pytest.mark.parametrize("close", ["mean", "adam"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("L", [100, 99])
def test_cohort_graph_replayed_twice_equals_two_enqueued_rounds_bitwise(L, precision, close):
    L_ = _L()
    lib = L_.kernels()
    x, y32 = _data(L, 2)
    glob = _flat(2)
    P, M, B, S = glob.numel(), 3, 8, 3
    t0, t1 = _table(S, M * B, seed=5), _table(S, M * B, seed=6)
    a = Cohort(x, y32, 2, M, B, S, precision, t0.clone(), glob, prox_mu=MU, **_server_fields(P, x.device, close == "adam"))
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(a.round)), "ecg_tiny_cohort_round_capture")
    try:
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(x.device)), "ecg_round_graph_launch")
        a.table.copy_(t1)
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(x.device)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    b = Cohort(x, y32, 2, M, B, S, precision, t0.clone(), glob, prox_mu=MU, **_server_fields(P, x.device, close == "adam"))
    b.run()
    after_one = b.glob.clone()
    b.table.copy_(t1)
    b.run()
    assert not torch.equal(after_one, b.glob) and not torch.equal(after_one, glob)
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u, v)
    # the proximal term acted: the same two rounds without it end elsewhere
    c = Cohort(x, y32, 2, M, B, S, precision, t0.clone(), glob, prox_mu=0.0, **_server_fields(P, x.device, close == "adam"))
    c.run()
    assert not torch.equal(c.glob, after_one)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_cohort_global_params_hold_the_starting_weights_until_the_close(precision):
    """The anchor of a cohort round is ``global_params`` itself.  A one-step round equals M single-client prox reduces
    of its gradient rows anchored on a COPY of the starting weights; under the split close (``server_delta``) a
    three-step round ends with ``global_params`` still on the starting weights, and its clients on the bits of the
    same round under the mean close."""
    x, y32 = _data(100, 2)
    glob = _flat(2)
    dev, P, M, B = x.device, glob.numel(), 3, 8
    f32 = dict(dtype=torch.float32, device=dev)
    delta = torch.zeros(P, **f32)
    co = Cohort(x, y32, 2, M, B, 1, precision, _table(1, M * B), glob, prox_mu=MU, cdp_scale=torch.ones(M, **f32),
                cdp_norm=torch.zeros(M, **f32), cdp_round=torch.zeros(1, dtype=torch.int64, device=dev),
                server_delta=delta).run()
    assert torch.equal(co.glob, glob) and bool(delta.any())
    # one step from the fanned-out weights with zero momenta, anchored on a copy
    anchor = glob.clone()
    for c in range(M):
        pc, mc = glob.clone(), torch.zeros(P, **f32)
        assert _prox_reduce(co.slab[c * B:(c + 1) * B], P, pc, mc, None, None, MOM, WD, 0, None, anchor, MU) == 0
        torch.cuda.synchronize()
        assert torch.equal(pc, co.cparams[c, :P]) and torch.equal(mc, co.cmom[c, :P]), c
    # three steps (from step 1 on the proximal term is non-zero) under the split close and under the mean
    co3 = Cohort(x, y32, 2, M, B, 3, precision, _table(3, M * B), glob, prox_mu=MU, cdp_scale=torch.ones(M, **f32),
                 cdp_norm=torch.zeros(M, **f32), cdp_round=torch.zeros(1, dtype=torch.int64, device=dev),
                 server_delta=torch.zeros(P, **f32)).run()
    co2 = Cohort(x, y32, 2, M, B, 3, precision, _table(3, M * B), glob, prox_mu=MU).run()
    assert torch.equal(co3.glob, glob) and not torch.equal(co2.glob, glob)
    assert torch.equal(co3.cparams, co2.cparams) and torch.equal(co3.cmom, co2.cmom)
    off = Cohort(x, y32, 2, M, B, 3, precision, _table(3, M * B), glob, prox_mu=0.0).run()
    assert not torch.equal(off.cparams, co2.cparams)
    s = co2.cparams[0, :P].clone()
    for c in range(1, M):
        s = s + co2.cparams[c, :P]
    assert torch.equal(co2.glob, s * torch.tensor(1.0 / M, dtype=torch.float32))


# 5 --------------------------------------------------------------------------------------------- prox_mu = 0
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_prox_mu_zero_is_the_round_of_before_bitwise(precision):
    """A ``TinyRound`` / ``TinyCohortRound`` built without the new fields (zero-filled) and trainers with prox_mu = 0
    against ones that name the fields."""
    from crossscale_ecg.ops.fused_tiny import prec_id
    L_ = _L()
    lib = L_.kernels()
    tr = _tiny_trainer(100, precision, 0.0, use_graph=False)
    assert tr.prox_anchor is None and tr._round.prox_mu == 0.0 and not tr._round.prox_anchor
    assert tr._round.prox_snapshot == 0
    p0, m0 = tr.params.clone(), tr.mom.clone()
    tr.run_round()
    torch.cuda.synchronize()
    # the same round described without the new fields, on buffers of its own
    params, mom, slab, loss = p0.clone(), m0.clone(), torch.empty_like(tr.slab), torch.zeros(1, device=tr.device)
    bufs = {k: (None if getattr(tr, k) is None else torch.zeros_like(getattr(tr, k))) for k in ("wprep", "xg", "yg", "xbg")}
    p = L_.ptr
    r = L_.TinyRound(X=tr.x.data_ptr(), ldx=tr.x.stride(0), idx=tr.idx_table.data_ptr(), Y=tr.y32.data_ptr(),
                     params=params.data_ptr(), mom=mom.data_ptr(), slab=slab.data_ptr(), loss_acc=loss.data_ptr(),
                     wprep=p(bufs["wprep"]), xg=p(bufs["xg"]), yg=p(bufs["yg"]), L=100, nc=2, slab_stride=tr.stride, B=8,
                     steps=3, lr=LR, momentum=MOM, wd=WD, nesterov=0, prec=prec_id(precision), xbg=p(bufs["xbg"]),
                     xpk=p(tr.xpk), prepack=L_.PREPACK[tr.prepack])
    L_.check(lib.ecg_tiny_round_enqueue(C.byref(r), L_.stream_ptr(tr.device)), "ecg_tiny_round_enqueue")
    # ... and with a garbage anchor and snapshot flag that prox_mu == 0 must leave unread
    params2, mom2, loss2 = p0.clone(), m0.clone(), torch.zeros(1, device=tr.device)
    junk = torch.full_like(p0, float("nan"))
    r.params, r.mom, r.loss_acc = params2.data_ptr(), mom2.data_ptr(), loss2.data_ptr()
    r.prox_mu, r.prox_anchor, r.prox_snapshot = 0.0, junk.data_ptr(), 1
    if bufs["wprep"] is not None:
        bufs["wprep"].zero_()
    L_.check(lib.ecg_tiny_round_enqueue(C.byref(r), L_.stream_ptr(tr.device)), "ecg_tiny_round_enqueue")
    torch.cuda.synchronize()
    for got_p, got_m, got_l in ((params, mom, loss), (params2, mom2, loss2)):
        assert torch.equal(got_p, tr.params) and torch.equal(got_m, tr.mom) and torch.equal(got_l, tr.loss_acc)
    assert bool(junk.isnan().all())  # no snapshot was taken
    tr.close()
    # cohort
    x, y32 = _data(100, 2)
    glob = _flat(2)
    table = _table(3, 24)
    a = Cohort(x, y32, 2, 3, 8, 3, precision, table, glob, with_prox_field=False).run()
    b = Cohort(x, y32, 2, 3, 8, 3, precision, table, glob, prox_mu=0.0).run()
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u, v)
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    trs = []
    for kw in ({}, dict(prox_mu=0.0, partition="contiguous")):
        torch.manual_seed(3)
        t = FusedCohortTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, clients=4, cohort=3, lr=LR, momentum=MOM,
                               weight_decay=WD, seed=7, precision=precision, **kw)
        t.run_round()
        trs.append(t)
    torch.cuda.synchronize()
    assert trs[0]._round.prox_mu == 0.0 and torch.equal(trs[0].params, trs[1].params)
    assert torch.equal(trs[0].idx_table, trs[1].idx_table)
    for t in trs:
        t.close()


# 6 --------------------------------------------------------------------------------------------- torch references
class _ReplaySampler:
    """Feeds a recorded index table to ``TorchLocalTrainer.step``, one row per step."""

    def __init__(self, table):
        self.table, self.i = table, 0

    def fill(self, out):
        out.copy_(self.table[self.i:self.i + out.shape[0]])
        self.i += out.shape[0]
        return out


def _rel(got, model):
    want = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    return (got - want).norm().item() / want.norm().item()


def test_fp32_fused_rounds_against_the_torch_local_trainer():
    """Two fp32 FedProx rounds, fused vs ``TorchLocalTrainer`` on the same batches: relative l2 difference of the
    weights below 1e-5, the bound the cohort and server-optimizer tests use for this comparison."""
    from crossscale_ecg.train.local import TorchLocalTrainer
    tr = _tiny_trainer(100, "fp32", MU, use_graph=True)
    ref = TinyECG().cuda()
    ref.load_state_dict(tr.model.state_dict())
    tt = TorchLocalTrainer(ref, tr.x, tr.y32.long(), 8, lr=LR, momentum=MOM, weight_decay=WD, amp_dtype=None, seed=11,
                           prox_mu=MU)
    for _ in range(2):
        tr.run_round()
        torch.cuda.synchronize()
        tt.sampler = _ReplaySampler(tr.idx_table.clone())
        tt.run_steps(3)
    rel = _rel(tr.params[:tr.P], ref)
    print(f"fp32 FedProx, 2 rounds, fused vs TorchLocalTrainer: relative l2 difference {rel:.3e}")
    assert rel < 1e-5, rel
    tr.close()


@pytest.mark.parametrize("server_opt", ["none", "adam"])
def test_fp32_fused_cohort_rounds_against_the_torch_cohort_trainer(server_opt):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y32 = _data(100, 2)
    kw = dict(clients=4, cohort=3, lr=LR, momentum=MOM, weight_decay=WD, seed=7, prox_mu=MU, partition="shards",
              server_opt=server_opt, server_lr=1.0 if server_opt == "none" else 0.05)
    torch.manual_seed(3)
    tr = FusedCohortTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, precision="fp32", **kw)
    torch.manual_seed(3)
    ref_model = TinyECG().cuda()
    ref = TorchCohortTrainer(ref_model, x, y32.long(), 8, 3, amp_dtype=None, **kw)
    start = tr.params.clone()
    for _ in range(2):
        tr.run_round()
        ref.run_round(3)
        torch.cuda.synchronize()
        assert torch.equal(tr.idx_table, ref.table) and tr.round_clients == ref.round_clients
    rel = _rel(tr.params[:tr.P], ref_model)
    print(f"fp32 FedProx cohort ({server_opt}), 2 rounds, fused vs TorchCohortTrainer: relative l2 difference {rel:.3e}")
    assert rel < 1e-5, rel
    assert not torch.equal(tr.params, start)
    # every drawn row belongs to its client's shards
    order = tr.sampler.order
    for j, k in enumerate(tr.round_clients):
        assert bool(torch.isin(tr.idx_table[:, j * 8:(j + 1) * 8].long(), order[k]).all())
    tr.close()


# 7 --------------------------------------------------------------------------------------------- rejections
def test_rejections():
    L_ = _L()
    lib = L_.kernels()
    assert C.sizeof(L_.TinyRound) == lib.ecg_tiny_round_sizeof()
    assert C.sizeof(L_.TinyCohortRound) == lib.ecg_tiny_cohort_round_sizeof()
    tr = _tiny_trainer(100, "bf16", MU, use_graph=False)
    tr.stage(3)
    torch.cuda.synchronize()
    before = _tiny_state(tr) + [tr.prox_anchor.clone()]
    dev = tr.device
    good = dict(prox_mu=tr._round.prox_mu, prox_anchor=tr._round.prox_anchor, dp_clip=0.0, dp_scale=None, dp_step=None)
    scale, step = torch.zeros(8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    bad = [dict(prox_mu=-0.1), dict(prox_anchor=None), dict(prox_anchor=tr.params.data_ptr()),
           dict(dp_clip=1.0, dp_scale=scale.data_ptr(), dp_step=step.data_ptr())]
    for change in bad:
        for k, v in {**good, **change}.items():
            setattr(tr._round, k, v)
        assert lib.ecg_tiny_round_enqueue(tr._round_of(3, tr.idx_stage), L_.stream_ptr(dev)) == BAD, change
        h = C.c_void_p()
        assert lib.ecg_tiny_round_capture(C.byref(h), tr._round_of(3, tr.idx_stage)) == BAD and not h.value, change
    for k, v in good.items():
        setattr(tr._round, k, v)
    torch.cuda.synchronize()
    for u, v in zip(before, _tiny_state(tr) + [tr.prox_anchor]):
        assert torch.equal(u, v)  # nothing was launched
    tr.launch_round(3)  # the restored description runs
    torch.cuda.synchronize()
    assert not torch.equal(before[0], tr.params)
    tr.close()
    # the cohort round
    x, y32 = _data(100, 2)
    glob = _flat(2)
    c = Cohort(x, y32, 2, 3, 8, 3, "fp32", _table(3, 24), glob, prox_mu=-0.1)
    assert c.enqueue() == BAD
    h = C.c_void_p()
    assert lib.ecg_tiny_cohort_round_capture(C.byref(h), C.byref(c.round)) == BAD and not h.value
    torch.cuda.synchronize()
    assert torch.equal(c.glob, glob)
    # the stand-alone entry points
    slab, p0, m0, a = _reduce_inputs(32, 2)
    P = p0.numel()
    params, mom = p0.clone(), m0.clone()
    assert _prox_reduce(slab, P, params, mom, None, None, MOM, WD, 0, None, None, MU) == BAD
    assert _prox_reduce(slab, P, params, mom, None, None, MOM, WD, 0, None, None, 0.0) == BAD
    assert _prox_reduce(slab, P, params, mom, None, None, MOM, WD, 0, None, a, -1.0) == BAD
    ps = lib.ecg_tiny_cohort_param_stride(2)
    cparams, cmom = torch.zeros(ps, device=slab.device), torch.zeros(ps, device=slab.device)
    assert _cohort_prox_reduce(slab, 32, 1, P, cparams, cmom, None, MOM, WD, 0, None, None, MU) == BAD
    assert _cohort_prox_reduce(slab, 32, 1, P, cparams, cmom, None, MOM, WD, 0, None, a, -1.0) == BAD
    assert _cohort_prox_reduce(slab, 32, 0, P, cparams, cmom, None, MOM, WD, 0, None, a, MU) == BAD
    torch.cuda.synchronize()
    assert torch.equal(params, p0) and torch.equal(mom, m0) and not bool(cparams.any())
    # the trainers
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    from crossscale_ecg.ops.fused_tiny import FusedTinyTrainer
    with pytest.raises(ValueError, match="prox_mu"):
        FusedTinyTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, prox_mu=-1.0)
    with pytest.raises(ValueError, match="DP-SGD"):
        FusedTinyTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, prox_mu=0.1, dp_clip=1.0)
    with pytest.raises(ValueError, match="prox_mu"):
        FusedCohortTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, clients=4, prox_mu=-1.0)
    with pytest.raises(ValueError, match="partition"):
        FusedCohortTrainer(TinyECG().cuda(), x, y32.long(), 8, 3, clients=4, partition="dirichlet")
