"""The split close of a cohort round on the GPU (``server_scope="global"``): cohort_delta_scale_kernel +
cohort_delta_kernel leave the averaged, clipped, noised delta in a buffer, the caller averages the ranks' buffers, and
server_step_kernel takes the server step.  Checked here: the two halves back to back against the fused closes bitwise,
``ecg_server_opt_step`` against ``train/server_opt.py: server_opt_step`` in float64, ``FusedCohortTrainer`` scope
"global" against scope "rank" bitwise (graph replay, enqueue, ``prepare``), two emulated ranks, the round without
``server_delta`` against a round that never named the field, the argument checks, and the driver on two gloo ranks that
share the one GPU.

Shapes: the stand-alone closes with nc in {2, 5} and M in {1, 3, 9}; rounds with B = 4, S = 2, L = 100, N = 64 windows, 4
clients of which 3 are drawn."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

from cohort_harness import DELTA_CANARY, LR, MU, N, WD, Cohort, _clients, _data, _global, _lib, _table

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SEED = 0xC0FFEE1234567
R0 = (1 << 32) + 3  # a round counter that uses both counter words
OPTS = {"none": 0, "sgdm": 1, "adagrad": 2, "adam": 3, "yogi": 4}
B1, B2, TAU = 0.9, 0.99, 1e-3
CANARY = DELTA_CANARY
BAD = 1  # kBadArg


def _f(x):
    return float(np.float32(x))


def _step(g, delta, n, opt, eta, m, v, b1=B1, b2=B2, tau=TAU):
    L_ = _lib()
    return L_.kernels().ecg_server_opt_step(L_.ptr(g), L_.ptr(delta), n, opt, eta, b1, b2, tau, L_.ptr(m), L_.ptr(v),
                                            L_.stream_ptr(torch.device("cuda:0")))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp", [True, False])
@pytest.mark.parametrize("M", [1, 3, 9])
@pytest.mark.parametrize("nc", [2, 5])
def test_split_close_equals_the_fused_close_bitwise(nc, M, dp):
    """ecg_cohort_delta_close + ecg_server_opt_step against ecg_cohort_dp_close (the plain step, eta in {1, 0.7}) and
    ecg_cohort_server_close (the four optimizers): two consecutive closes each (the second reads the first one's
    weights, m and v), clip and noise on or both off, NaN in the clients' padding floats.  Weights, m, v, clip factors,
    norms and round word are equal bit for bit; the delta close leaves ``global`` as found and writes P floats."""
    L_ = _lib()
    lib = L_.kernels()
    clip, sigma = (0.3, 1.5) if dp else (0.0, 0.0)
    P = num_params(nc)
    g0, params = _clients(nc, M, 0.3)
    stream = L_.stream_ptr(g0.device)
    f32 = dict(dtype=torch.float32, device="cuda")
    for opt, eta in (("none", 1.0), ("none", 0.7), ("sgdm", 0.7), ("adagrad", 0.05), ("adam", 0.05), ("yogi", 0.05)):
        oid = OPTS[opt]
        ga, gb = g0.clone(), g0.clone()
        ma = mb = va = vb = None
        if oid:
            ma, mb = torch.zeros(P, **f32), torch.zeros(P, **f32)
        if oid >= 2:
            va, vb = torch.full((P,), TAU, **f32) ** 2, torch.full((P,), TAU, **f32) ** 2
        wa, wb = (torch.tensor([R0], dtype=torch.int64, device="cuda") for _ in range(2))
        sa, na, sb, nb = (torch.full((M,), -1.0, **f32) for _ in range(4))
        delta = torch.full((P + 8,), CANARY, **f32)
        for call in range(2):
            if oid == 0:
                st = lib.ecg_cohort_dp_close(params.data_ptr(), ga.data_ptr(), nc, M, clip, sigma, eta, SEED,
                                             wa.data_ptr(), sa.data_ptr(), na.data_ptr(), stream)
            else:
                st = lib.ecg_cohort_server_close(params.data_ptr(), ga.data_ptr(), nc, M, clip, sigma, eta, SEED,
                                                 wa.data_ptr(), sa.data_ptr(), na.data_ptr(), oid, B1, B2, TAU,
                                                 ma.data_ptr(), L_.ptr(va), stream)
            assert st == 0
            before = gb.clone()
            st = lib.ecg_cohort_delta_close(params.data_ptr(), gb.data_ptr(), nc, M, clip, sigma, SEED, wb.data_ptr(),
                                            sb.data_ptr(), nb.data_ptr(), delta.data_ptr(), stream)
            torch.cuda.synchronize()
            assert st == 0 and torch.equal(gb, before)  # global is only read
            assert bool((delta[P:] == CANARY).all()) and bool(torch.isfinite(delta[:P]).all())
            assert _step(gb, delta, P, oid, eta, mb, vb) == 0
            torch.cuda.synchronize()
            assert torch.equal(ga, gb), (opt, eta, call)
            if call == 0:  # (one client, no noise, eta = 1: the first close lands on the client and the second delta is 0)
                assert float(delta[:P].abs().max()) > 1e-5 and not torch.equal(gb, before)
            for u, v in ((ma, mb), (va, vb)):
                assert (u is None and v is None) or torch.equal(u, v), (opt, call)
            assert torch.equal(sa, sb) and torch.equal(na, nb) and int(wa.item()) == int(wb.item()) == R0 + call + 1
            assert bool((delta[P:] == CANARY).all())
        if oid:
            assert float(mb.abs().max()) > 0
    assert bool(torch.isnan(params[:, P:]).all())


# 2 ---------------------------------------------------------------------------------------------------------------
def _bounds(opt, g, d, m, v, wm, wv, eta, b1, b2, tau):
    """(bound on g_new, on m_new, on v_new): tests/test_tiny_cohort_server_opt_gpu.py's element-wise first-order fp32
    bounds of the fused close (its ``_step64``; the derivation is in that file's first test) with e_D = 0 - here Delta
    is an input, not a computed value.  The plain step g + eta Delta takes sgdm's bound on g with m = Delta exact."""
    eta, b1, b2, tau = _f(eta), _f(b1), _f(b2), _f(tau)
    if opt == "none":
        return 2 * EPS32 * (np.abs(g) + np.abs(eta * d)), None, None
    if opt == "sgdm":
        e_m = 2 * EPS32 * (np.abs(b1 * m) + np.abs(d))
        return eta * e_m + 2 * EPS32 * (np.abs(g) + np.abs(eta * wm)), e_m, None
    e_m = 3 * EPS32 * (np.abs(b1 * m) + np.abs((1 - b1) * d))
    d2 = d * d
    if opt == "adagrad":
        e_v = 2 * EPS32 * (v + d2)
    elif opt == "adam":
        e_v = 3.5 * EPS32 * (v + d2)
    else:
        tie = np.abs(v - d2) <= EPS32 * (v + d2)  # the fp32 sign may be the other one (or 0) there
        e_v = 3.5 * EPS32 * (v + d2) + np.where(tie, 2 * (1 - b2) * d2, 0.0)
    den = np.sqrt(wv) + tau
    st = eta * wm / den
    e_den = e_v / np.sqrt(np.maximum(wv, 1e-300)) + 1.5 * EPS32 * den
    e_st = eta * e_m / den + np.abs(st) * (e_den / den + 2 * EPS32)
    return e_st + EPS32 * (np.abs(g) + np.abs(st)), e_m, e_v


@pytest.mark.parametrize("n", [1, 255, 257, 1458])
def test_server_opt_step_odd_sizes_against_float64(n):
    """Every rule on n floats (one element, one short of a block, one past it, TinyECG's P) with nonzero m and a v on
    both sides of Delta^2 (4 Delta^2 | Delta^2 / 4: both of yogi's signs, no near-ties), against ``server_opt_step``
    evaluated in float64 within the fused close's element-wise bound; a canary behind every written buffer."""
    from crossscale_ecg.train.server_opt import server_opt_step
    rng = np.random.default_rng(n)
    worst = {}
    for opt, oid in OPTS.items():
        eta = 0.7 if oid < 2 else 0.05
        g = torch.from_numpy(rng.standard_normal(n + 8)).float().cuda()
        d = torch.from_numpy(rng.standard_normal(n + 8) * 0.02).float().cuda()
        m = torch.from_numpy(rng.standard_normal(n + 8) * 0.01).float().cuda()
        d2 = (d * d).double().cpu().numpy()
        v = torch.from_numpy(np.where(np.arange(n + 8) % 2 == 0, 4.0 * d2, d2 / 4.0)).float().cuda()
        for t in (g, m, v):
            t[n:] = CANARY
        g0, m0, v0 = g.clone(), m.clone(), v.clone()
        G, D, Mo, V = (t[:n].double().cpu() for t in (g0, d, m0, v0))
        if oid == 0:
            wg, wm, wv = G + _f(eta) * D, None, None
        else:
            wg, wm, wv = server_opt_step(opt, G, D, Mo, V, eta, B1, B2, TAU, dtype=torch.float64)
            assert wg.dtype == torch.float64
        np_ = lambda t: None if t is None else t.numpy()  # noqa: E731
        bg, bm, bv = _bounds(opt, G.numpy(), D.numpy(), Mo.numpy(), V.numpy(), np_(wm), np_(wv), eta, B1, B2, TAU)
        assert _step(g, d, n, oid, eta, m if oid else None, v if oid >= 2 else None) == 0
        torch.cuda.synchronize()
        for t in (g, m, v):
            assert bool((t[n:] == CANARY).all()), opt
        assert torch.equal(m, m0) if oid == 0 else not torch.equal(m, m0)
        assert torch.equal(v, v0) if oid < 2 else not torch.equal(v, v0)  # sgdm and the plain step do not touch v
        for name, got, want, bound in (("g", g, wg, bg), ("m", m, wm, bm), ("v", v, wv if oid >= 2 else None, bv)):
            if want is None or bound is None:
                continue
            err = np.abs(got[:n].double().cpu().numpy() - want.numpy())
            ratio = float((err / bound).max())
            worst[opt] = max(worst.get(opt, 0.0), ratio)
            assert np.all(err <= bound), (opt, name, ratio)
        assert float((wg - G).abs().max()) > 1e-5
    print(f"n={n}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------ whole rounds
M_, B_, S_ = 3, 4, 2
DP = dict(cdp_clip=0.004, cdp_sigma=1.2, server_lr=0.8, cdp_seed=SEED, round=R0)


def _so(opt, **kw):
    return dict(dict(server_opt=OPTS[opt], server_beta1=B1, server_beta2=B2, server_tau=TAU), **kw)


def _trainer(x, y32, precision, use_graph=True, seed=7, **kw):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    torch.manual_seed(3)
    model = TinyECG().to(x.device)
    return FusedCohortTrainer(model, x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                              seed=seed, use_graph=use_graph, precision=precision, **kw)


def _tkw(opt):
    eta = {"none": 0.7, "sgdm": 0.8}.get(opt, 0.01)  # an adaptive step is eta * O(1) per parameter
    return dict(client_dp_clip=0.004, client_dp_noise=1.2, server_lr=eta, server_opt=opt)


def _tstate(tr):
    return [t.clone() for t in (tr.params, tr.server_m, tr.server_v, tr.cdp_round, tr.cdp_scale, tr.cdp_norm)
            if t is not None]


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["none", "sgdm", "adam"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_trainer_scope_global_equals_scope_rank_on_one_rank(precision, opt):
    """Two rounds: scope "rank" (one graph replay per round) against scope "global" replaying its graph and against
    scope "global" enqueueing its kernels - weights, m, v, round word, factors and norms bit for bit; ``prepare`` on the
    scope-"global" trainer, after a round, leaves that state as found."""
    dev, x, y32 = _data(100, 2)
    rank = _trainer(x, y32, precision, **_tkw(opt))
    glob = _trainer(x, y32, precision, server_scope="global", **_tkw(opt))
    eager = _trainer(x, y32, precision, use_graph=False, server_scope="global", **_tkw(opt))
    assert rank.server_delta is None and rank._round.server_delta is None
    r = glob._round
    assert r.server_delta == glob.server_delta.data_ptr() and r.server_opt == 0 and r.server_m is None
    assert glob.server_delta.shape == (glob.P,) and glob.client_dp and (glob.server_m is None) == (opt == "none")
    start = rank.params.clone()
    for rnd in range(2):
        for tr in (rank, glob, eager):
            tr.run_round()
        torch.cuda.synchronize()
        for tr in (glob, eager):
            for u, v in zip(_tstate(rank), _tstate(tr)):
                assert torch.equal(u, v), (rnd, tr.use_graph)
            assert tr.round_clients == rank.round_clients
        assert torch.equal(glob.server_delta, eager.server_delta) and float(glob.server_delta.abs().max()) > 0
        if rnd == 0:
            found = _tstate(glob)
            glob.prepare([S_])  # captures the second table's graph, replays both, rolls back
            for u, v in zip(found, _tstate(glob)):
                assert torch.equal(u, v)
            assert glob.cohort_round == 1 and len(glob._graphs) == 2
    assert not torch.equal(rank.params, start) and int(glob.cdp_round.item()) == 2
    # launch_round alone leaves the weights, m and v where they were and the delta in server_delta
    found = _tstate(glob)[:3 if opt == "adam" else 2 if opt == "sgdm" else 1]
    glob.prepare_round()
    glob.launch_round()
    torch.cuda.synchronize()
    for u, v in zip(found, _tstate(glob)):
        assert torch.equal(u, v)
    with pytest.raises(RuntimeError, match="server_scope"):
        rank.apply_server_step()
    for tr in (rank, glob, eager):
        tr.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_two_emulated_ranks_take_one_global_adam_step(precision):
    """Two trainers with world_size = 2 (each adds sigma / sqrt(2) of the noise), different seeds and windows, the same
    starting weights.  Per round each "rank" launches its round, both ``server_delta`` buffers are set to
    (d0 + d1) * 0.5, and each takes ``apply_server_step``.  After 3 rounds of adam with clipping and noise the weights,
    m and v are bit-identical on both; in fp32 they are within 1e-5 relative l2 (the project's fp32 bound) of the same
    procedure on two ``TorchCohortTrainer``s."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    kw = dict(world_size=2, server_scope="global", **_tkw("adam"))
    data = [_data(100, 2, seed=k) for k in range(2)]
    ranks = [_trainer(x, y32, precision, seed=7 + 100 * k, **kw) for k, (_, x, y32) in enumerate(data)]
    refs = []
    if precision == "fp32":
        for k, (dev, x, y32) in enumerate(data):
            torch.manual_seed(3)
            refs.append(TorchCohortTrainer(TinyECG().to(dev), x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR,
                                           momentum=MU, weight_decay=WD, amp_dtype=None, seed=7 + 100 * k, **kw))
    assert abs(ranks[0]._round.cdp_sigma - 1.2 / 2 ** 0.5) < 1e-6
    start = ranks[0].params.clone()
    assert torch.equal(ranks[1].params, start)
    for rnd in range(3):
        for group in (ranks, refs):
            for tr in group:
                tr.prepare_round(S_)
                tr.launch_round(S_)
            if not group:
                continue
            torch.cuda.synchronize()
            assert not torch.equal(group[0].server_delta, group[1].server_delta)
            avg = (group[0].server_delta + group[1].server_delta) * 0.5
            for tr in group:
                tr.server_delta.copy_(avg)
                tr.apply_server_step()
        torch.cuda.synchronize()
        assert torch.equal(ranks[0].params, ranks[1].params), rnd
        assert torch.equal(ranks[0].server_m, ranks[1].server_m) and torch.equal(ranks[0].server_v, ranks[1].server_v)
    assert ranks[0].round_clients != ranks[1].round_clients or not torch.equal(data[0][1], data[1][1])
    P = ranks[0].P
    moved = (ranks[0].params[:P] - start[:P]).norm().item() / start[:P].norm().item()
    assert moved > 1e-3
    if refs:
        want = torch.cat([p.detach().reshape(-1) for p in refs[0].model.parameters()])
        assert torch.equal(want, torch.cat([p.detach().reshape(-1) for p in refs[1].model.parameters()]))
        rel = (ranks[0].params[:P] - want).norm().item() / want.norm().item()
        rel_m = (ranks[0].server_m - refs[0].server_m).norm().item() / refs[0].server_m.norm().item()
        print(f"two emulated ranks, adam, 3 rounds, fused vs torch: relative l2 {rel:.3e} (update {moved:.3e}; m {rel_m:.3e})")
        assert rel < 1e-5, rel
    for tr in ranks:
        tr.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_null_server_delta_is_the_round_without_the_field(precision):
    """All three closes (mean, DP, server optimizer): a struct whose ``server_delta`` was set and put back to null
    against one that never named it, bitwise; and with the buffer set the round ends with the starting weights, the
    delta of the fused close and nothing behind P written, whatever the server_opt fields hold."""
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    table = _table(S_, M_ * B_)
    scratch = torch.zeros(num_params(2), device=dev)
    for dp, so in ((None, None), (DP, None), (DP, _so("adam"))):
        a = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, dp, so).run()
        b = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, dp, so)
        b.round.server_delta = scratch.data_ptr()
        b.round.server_delta = None
        b.run()
        assert not torch.equal(a.glob, glob)
        for u, v in zip(a.state(), b.state()):
            assert torch.equal(u, v)
    assert float(scratch.abs().max()) == 0.0
    fused = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, DP).run()
    for so in (None, _so("adam"), dict(server_opt=9, server_beta1=7.0, server_beta2=-1.0, server_tau=-1.0)):
        c = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, DP, None, split=True)
        for k, val in (so or {}).items():
            setattr(c.round, k, val)  # (m and v stay null: with server_delta set none of them is read)
        c.run()
        assert torch.equal(c.glob, glob) and bool((c.delta[c.P:] == CANARY).all())
        assert torch.equal(c.scale, fused.scale) and torch.equal(c.norm, fused.norm) and int(c.word.item()) == R0 + 1
        assert torch.equal(c.cparams, fused.cparams) and torch.equal(c.loss, fused.loss)
        assert _step(c.glob, c.delta, c.P, 0, DP["server_lr"], None, None) == 0
        torch.cuda.synchronize()
        assert torch.equal(c.glob, fused.glob)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_rejections():
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    table = _table(S_, M_ * B_)
    lib = _lib().kernels()
    assert C.sizeof(_lib().TinyCohortRound) == lib.ecg_tiny_cohort_round_sizeof()
    assert Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, DP, None, split=True).enqueue() == 0
    for field in ("cdp_scale", "cdp_norm", "cdp_round"):  # the split close needs the DP close's buffers
        c = Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, DP, None, split=True)
        setattr(c.round, field, None)
        assert c.enqueue() == BAD, field
        g = C.c_void_p()
        assert lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == BAD and not g.value
    c = Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, None, None, split=True)  # no DP buffers at all
    assert c.enqueue() == BAD
    c = Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, DP, None, split=True)
    c.round.cdp_sigma, c.round.cdp_clip = 1.0, 0.0  # noise without a clip norm stays rejected
    assert c.enqueue() == BAD
    # ecg_cohort_delta_close
    P = num_params(2)
    gp, params = _clients(2, 3, 0.3)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    sc, nm, d = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda"), torch.zeros(P, device="cuda")
    ok = [params.data_ptr(), gp.data_ptr(), 2, 3, 0.3, 1.0, 1, w.data_ptr(), sc.data_ptr(), nm.data_ptr(), d.data_ptr(),
          None]
    for i, val in ((0, None), (1, None), (7, None), (8, None), (9, None), (10, None), (2, 0), (2, 99), (3, 0), (3, 65536),
                   (4, -1.0), (5, -1.0)):
        args = list(ok)
        args[i] = val
        assert lib.ecg_cohort_delta_close(*args) == BAD, i
    args = list(ok)
    args[4] = 0.0  # noise without a clip norm
    assert lib.ecg_cohort_delta_close(*args) == BAD
    # ecg_server_opt_step
    g, m, v = torch.ones(P, device="cuda"), torch.zeros(P, device="cuda"), torch.ones(P, device="cuda")
    ok = [g.data_ptr(), d.data_ptr(), P, 3, 0.1, B1, B2, TAU, m.data_ptr(), v.data_ptr(), None]
    for i, val in ((0, None), (1, None), (2, 0), (2, -5), (3, -1), (3, 5), (4, -0.1), (5, 1.0), (5, -0.1), (6, 1.0),
                   (6, -0.5), (7, 0.0), (7, -1.0), (8, None), (9, None)):
        args = list(ok)
        args[i] = val
        assert lib.ecg_server_opt_step(*args) == BAD, i
    for opt in (2, 4):  # adagrad and yogi need v and tau too; sgdm needs m only; the plain step neither
        args = list(ok)
        args[3], args[9] = opt, None
        assert lib.ecg_server_opt_step(*args) == BAD
    args = list(ok)
    args[3], args[8] = 1, None
    assert lib.ecg_server_opt_step(*args) == BAD
    torch.cuda.synchronize()
    assert int(w.item()) == 0 and bool((g == 1).all()) and float(m.abs().max()) == 0.0  # nothing was launched
    d.fill_(0.5)
    args = list(ok)
    args[3], args[7], args[9] = 1, 0.0, None  # sgdm: no tau, no v
    assert lib.ecg_server_opt_step(*args) == 0
    args = [g.data_ptr(), d.data_ptr(), P, 0, 0.0, 7.0, -1.0, -1.0, None, None, None]  # plain: eta 0 means 1
    assert lib.ecg_server_opt_step(*args) == 0
    torch.cuda.synchronize()
    assert bool((m == 0.5).all()) and bool((g == 1.0 + _f(0.1) * 0.5 + 0.5).all())
    with pytest.raises(ValueError, match="unknown server scope"):
        _trainer(x, y32, "fp32", server_scope="node")


# 7 ---------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _driver_worker(rank, world, port, overlap, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", ECG_DIST_BACKEND="gloo")
    import crossscale_ecg  # noqa: F401
    from crossscale_ecg.config import FedAvgConfig
    from crossscale_ecg.parallel.env import init_distributed, shutdown_distributed
    from crossscale_ecg.train import fedavg as drv
    ctx = init_distributed()
    kept = []
    real = drv.make_trainer

    def spy(*a):
        kept.append(real(*a))
        return kept[-1]

    drv.make_trainer = spy
    tmp = os.path.join(out_dir, f"{overlap}_{rank}")
    cfg = FedAvgConfig(batch_size=4, rounds=3, local_steps=2, config="G1", amp_dtype="bf16", kernel_backend="fused",
                       synthetic_windows=128, max_windows=128, labels="parity", win_len=100, quiet=True,
                       clients_per_gpu=4, cohort=3, server_opt="adam", server_lr=0.01, server_scope="global",
                       client_dp_clip=0.05, client_dp_noise=0.5, overlap=overlap,
                       results_csv=os.path.join(tmp, "rounds.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                       client_privacy_csv=os.path.join(tmp, "cp.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    try:
        rows = drv.run_fedavg(cfg, ctx)
        tr = kept[0]
        assert type(tr).__name__ == "FusedCohortTrainer" and tr.server_scope == "global" and ctx.backend == "gloo"
        assert rank != 0 or (len(rows) == 6 and all(r["backend"] == "fused" for r in rows))
        torch.cuda.synchronize()
        torch.save({"w": tr.params.cpu(), "m": tr.server_m.cpu(), "v": tr.server_v.cpu(),
                    "sigma": float(tr._round.cdp_sigma)}, os.path.join(out_dir, f"{overlap}_{rank}.pt"))
    finally:
        shutdown_distributed()


def test_driver_two_gloo_ranks_share_the_gpu(tmp_path):
    """The driver on the fused backend with --server-opt adam --server-scope global on two gloo ranks that share the
    GPU: both ranks end on identical weights, m and v, and --overlap tail ends on the bits of --overlap none."""
    runs = [mp.start_processes(_driver_worker, args=(2, _free_port(), overlap, str(tmp_path)), nprocs=2, join=False,
                               start_method="spawn") for overlap in ("none", "tail")]
    for ctx in runs:
        while not ctx.join():
            pass
    out = {(o, r): torch.load(tmp_path / f"{o}_{r}.pt", weights_only=True) for o in ("none", "tail") for r in (0, 1)}
    torch.manual_seed(1234)
    for o in ("none", "tail"):
        for k in ("w", "m", "v"):
            assert torch.equal(out[o, 0][k], out[o, 1][k]), (o, k)
        assert abs(out[o, 0]["sigma"] - 0.5 / 2 ** 0.5) < 1e-6
    for k in ("w", "m", "v"):
        assert torch.equal(out["none", 0][k], out["tail", 0][k]), k
    assert float(out["none", 0]["m"].abs().max()) > 0
