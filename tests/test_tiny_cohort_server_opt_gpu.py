"""Server optimizers on the close of a cohort round on the GPU (cohort_delta_scale_kernel + cohort_server_opt_kernel):
the stand-alone close against the definition in float64 numpy, sgdm without momentum against the DP close bitwise, whole
rounds (graph replay against enqueue, prepare, resume), the trainer against ``TorchCohortTrainer``, the server_opt == 0
path against a round built without the new fields, and the argument checks.

The definition: Delta = (sum_c s_c d_c, ascending c) * fp32(1 / M) + nu * z as in the client-DP close
(tests/test_tiny_cohort_client_dp_gpu.py), then with the server state m, v (fp32, no bias correction)
  sgdm     m = b1 m + Delta,            g += eta m
  adagrad  m = b1 m + (1 - b1) Delta,   v = v + Delta^2
  adam     m as adagrad,                v = b2 v + (1 - b2) Delta^2
  yogi     m as adagrad,                v = v - (1 - b2) Delta^2 sign(v - Delta^2), sign(0) = 0
  adagrad, adam, yogi:                  g += eta m / (sqrt(v) + tau)

Shapes: the stand-alone close with nc in {2, 5} and M in {1, 3, 5}; rounds with B = 4, S = 2, L = 100, N = 64 windows."""
import ctypes as C

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.utils import philox

from cohort_harness import LR, MU, N, WD, Cohort, _clients, _data, _global, _lib, _table

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SEED = 0xC0FFEE1234567
R0 = (1 << 32) + 3  # a round counter that uses both counter words
OPTS = {"sgdm": 1, "adagrad": 2, "adam": 3, "yogi": 4}
B1, B2, TAU = 0.9, 0.99, 1e-3


def _f(x):
    return float(np.float32(x))


def _server_close(params, glob, m, v, word, nc, M, clip, sigma, eta, seed, opt, b1=B1, b2=B2, tau=TAU):
    """ecg_cohort_server_close in place on glob, m, v, word: (status, scale, norm)."""
    L_ = _lib()
    scale = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    norm = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    st = L_.kernels().ecg_cohort_server_close(params.data_ptr(), glob.data_ptr(), nc, M, clip, sigma, eta, seed,
                                              word.data_ptr(), scale.data_ptr(), norm.data_ptr(), OPTS[opt], b1, b2, tau,
                                              m.data_ptr(), L_.ptr(v), L_.stream_ptr(glob.device))
    torch.cuda.synchronize()
    return st, scale, norm


def _delta64(params, glob, P, M, clip, nu, seed, r):
    """(Delta, its error bound) of the definition in float64 on the fp32 inputs.  The bound is the client-DP test's
    bound on Delta - (M + 8) roundings of fp32 on the mean of |d_c| and on nu |z|, plus 4e-6 nu for the device-vs-numpy
    Box-Muller difference - plus the clip factors' own error (that test's bound on them: (P / 64 + 8) roundings,
    relative) on the clipped clients' share of the mean."""
    g = glob.double().cpu().numpy()
    d = params[:, :P].double().cpu().numpy() - g[None, :]
    n = np.linalg.norm(d, axis=1)
    s = np.array([1.0 if (v == 0 or clip == 0) else min(1.0, clip / v) for v in n])
    z = philox.normal(seed, r, P, stream=1) if nu != 0 else np.zeros(P)
    delta = (s[:, None] * d).sum(0) / M + nu * z
    clipped = (np.where(s < 1.0, s, 0.0)[:, None] * np.abs(d)).sum(0) / M
    e = (M + 8) * EPS32 * (np.abs(d).mean(0) + nu * np.abs(z)) + 4e-6 * nu + (P / 64 + 8) * EPS32 * clipped
    return delta, e


def _step64(opt, g, d, e_d, m, v, eta, b1, b2, tau):
    """(g_new, m_new, v_new, bound on g_new, on m_new, on v_new): the definition in float64 and its first-order fp32
    error bounds (the derivation is in test_server_close_against_the_definition_in_float64's docstring)."""
    eta, b1, b2, tau = _f(eta), _f(b1), _f(b2), _f(tau)
    if opt == "sgdm":
        m1 = b1 * m + d
        e_m = e_d + 2 * EPS32 * (np.abs(b1 * m) + np.abs(d))
        g1 = g + eta * m1
        return g1, m1, None, eta * e_m + 2 * EPS32 * (np.abs(g) + np.abs(eta * m1)), e_m, None
    m1 = b1 * m + (1 - b1) * d
    e_m = (1 - b1) * e_d + 3 * EPS32 * (np.abs(b1 * m) + np.abs((1 - b1) * d))
    d2 = d * d
    e_d2 = 2 * np.abs(d) * e_d + e_d * e_d
    if opt == "adagrad":
        v1 = v + d2
        e_v = e_d2 + 2 * EPS32 * (v + d2)
    elif opt == "adam":
        v1 = b2 * v + (1 - b2) * d2
        e_v = (1 - b2) * e_d2 + 3.5 * EPS32 * (v + d2)
    else:
        v1 = v - (1 - b2) * d2 * np.sign(v - d2)
        tie = np.abs(v - d2) <= e_d2 + EPS32 * (v + d2)  # the fp32 sign may be the other one (or 0) there
        e_v = (1 - b2) * e_d2 + 3.5 * EPS32 * (v + d2) + np.where(tie, 2 * (1 - b2) * d2, 0.0)
    den = np.sqrt(v1) + tau
    st = eta * m1 / den
    e_den = e_v / np.sqrt(np.maximum(v1, 1e-300)) + 1.5 * EPS32 * den
    e_st = eta * e_m / den + np.abs(st) * (e_den / den + 2 * EPS32)
    return g + st, m1, v1, e_st + EPS32 * (np.abs(g) + np.abs(st)), e_m, e_v


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dp", [True, False])
@pytest.mark.parametrize("M", [1, 3, 5])
@pytest.mark.parametrize("nc", [2, 5])
def test_server_close_against_the_definition_in_float64(nc, M, dp):
    """Every optimizer, two consecutive calls (the second reads the first one's m, v and weights), with clip and noise
    on and with both off; each call is compared with the float64 definition evaluated on the fp32 state going in.

    The element-wise bound, to first order, u = 2^-24 per correctly rounded fp32 operation and EPS32 = 2u.  This file is
    compiled with -fno-honor-nans -fno-signed-zeros and without fast-math: fp32 division and sqrtf are correctly rounded
    (0.5 ulp each), and contraction to fused multiply-adds only removes roundings.
      e_D  the bound on Delta (``_delta64``: the client-DP test's (M + 8) 2^-23 (mean |d_c| + nu |z|) + 4e-6 nu, plus
           the clip factors' error on the clipped share).
      sgdm m = b1 m + D: 2 operations, e_m = e_D + 2 EPS32 (|b1 m| + |D|) (1 EPS32 counted, 1 added);
           g + eta m: 2 operations, e_g = eta e_m + 2 EPS32 (|g| + |eta m|).
      m    = b1 m + (1 - b1) D: 4 operations, e_m = (1 - b1) e_D + 3 EPS32 (|b1 m| + |(1 - b1) D|).
      D^2  e_D2 = 2 |D| e_D + e_D^2.
      v    adagrad, 2 operations: e_v = e_D2 + 2 EPS32 (v + D^2); adam and yogi, at most 5: e_v = (1 - b2) e_D2 + 3.5
           EPS32 (v + D^2); yogi where |v - D^2| is within its own error: the sign is undetermined, + 2 (1 - b2) D^2.
      den  = sqrt(v) + tau: e_den = e_v / sqrt(v) (twice the first-order term e_v / (2 sqrt(v))) + 1.5 EPS32 den.
      step = eta m / den: e_s = eta e_m / den + |step| (e_den / den + 2 EPS32);  g + step: e_g = e_s + EPS32 (|g| + |step|).
    Measured worst error / bound: see profiles/r14/tiny_cohort_server_opt.txt."""
    clip, sigma, eta = (0.3, 1.5, 0.05) if dp else (0.0, 0.0, 0.05)
    P = num_params(nc)
    g0, params = _clients(nc, M, 0.3)
    before = params.clone()
    nu = sigma * clip / M
    worst = {}
    for opt in OPTS:
        g = g0.clone()
        m = torch.zeros(P, dtype=torch.float32, device="cuda")
        d0, _ = _delta64(params, g, P, M, clip, nu, SEED, R0)
        v = None
        if opt == "yogi":  # both signs of v - Delta^2 with no near-ties: v = 4 Delta^2 | Delta^2 / 4
            v = torch.from_numpy(np.where(np.arange(P) % 2 == 0, 4.0 * d0 * d0, d0 * d0 / 4.0)).float().cuda()
        elif opt != "sgdm":
            v = torch.full((P,), TAU, dtype=torch.float32, device="cuda") ** 2
        word = torch.tensor([R0], dtype=torch.int64, device="cuda")
        for call in range(2):
            g64, m64 = g.double().cpu().numpy(), m.double().cpu().numpy()
            v64 = None if v is None else v.double().cpu().numpy()
            d, e_d = _delta64(params, g, P, M, clip, nu, SEED, R0 + call)
            if opt == "yogi" and call == 0:
                sg = np.sign(v64 - d * d)
                assert (sg > 0).sum() > P // 3 and (sg < 0).sum() > P // 3
            wg, wm, wv, bg, bm, bv = _step64(opt, g64, d, e_d, m64, v64, eta, B1, B2, TAU)
            st, scale, norm = _server_close(params, g, m, v, word, nc, M, clip, sigma, eta, SEED, opt)
            assert st == 0 and int(word.item()) == R0 + call + 1  # the round counter advanced by one
            assert bool((scale <= 1.0).all()) and bool((scale > 0.0).all()) and bool((norm >= 0.0).all())
            if not dp:
                assert bool((scale == 1.0).all())
            for name, got, want, bound in (("g", g, wg, bg), ("m", m, wm, bm), ("v", v, wv, bv)):
                if got is None:
                    continue
                assert bool(torch.isfinite(got).all()), (opt, name)  # the NaN padding was not read
                err = np.abs(got.double().cpu().numpy() - want)
                ratio = float((err / bound).max())
                worst[opt] = max(worst.get(opt, 0.0), ratio)
                assert np.all(err <= bound), (opt, call, name, ratio)
            assert np.abs(wg - g64).max() > 1e-5 and (call == 0 or np.abs(m64).max() > 0)  # moved; nonzero m was read
    assert torch.equal(params[:, :P], before[:, :P]) and bool(torch.isnan(params[:, P:]).all())  # read only
    print(f"nc={nc} M={M} dp={dp}: worst error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1.5, 0.0])
@pytest.mark.parametrize("eta", [1.0, 0.7])
def test_sgdm_without_momentum_is_the_dp_close_bitwise(eta, sigma):
    L_ = _lib()
    nc, M, clip = 2, 5, 0.3
    P = num_params(nc)
    g, params = _clients(nc, M, clip)
    want = g.clone()
    sc0, nm0 = torch.zeros(M, device="cuda"), torch.zeros(M, device="cuda")
    w0 = torch.tensor([R0], dtype=torch.int64, device="cuda")
    L_.check(L_.kernels().ecg_cohort_dp_close(params.data_ptr(), want.data_ptr(), nc, M, clip, sigma, eta, SEED,
                                              w0.data_ptr(), sc0.data_ptr(), nm0.data_ptr(), L_.stream_ptr(g.device)),
             "ecg_cohort_dp_close")
    got, m = g.clone(), torch.zeros(P, dtype=torch.float32, device="cuda")
    w1 = torch.tensor([R0], dtype=torch.int64, device="cuda")
    st, sc1, nm1 = _server_close(params, got, m, None, w1, nc, M, clip, sigma, eta, SEED, "sgdm", b1=0.0)  # v == nullptr
    assert st == 0 and torch.equal(got, want) and not torch.equal(got, g)
    assert torch.equal(sc1, sc0) and torch.equal(nm1, nm0) and int(w1.item()) == int(w0.item()) == R0 + 1
    # m is Delta, and g_new = fl(g + eta m): one rounding (eta == 1: g_new - g is m up to it; else the product's too
    # where the compiler does not fuse it into the sum)
    err = (got.double() - g.double() - _f(eta) * m.double()).abs()
    slack = 0.0 if eta == 1.0 else 2.0 ** -24 * _f(eta) * m.double().abs()
    assert bool((err <= 2.0 ** -24 * got.double().abs() + slack).all()) and float(m.abs().max()) > 1e-4


# ------------------------------------------------------------------------------------------------------ whole rounds
M_, B_, S_ = 3, 4, 2
DP = dict(cdp_clip=0.004, cdp_sigma=1.2, server_lr=0.8, cdp_seed=SEED, round=R0)


def _so(opt, **kw):
    return dict(dict(server_opt=OPTS[opt], server_beta1=B1, server_beta2=B2, server_tau=TAU), **kw)


def _dp(opt):
    return dict(DP, server_lr=0.8 if opt == "sgdm" else 0.01)  # an adaptive step is eta * O(1) per parameter


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgdm", "adam"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replayed_twice_equals_two_enqueued_rounds_bitwise(precision, opt):
    L_ = _lib()
    lib = L_.kernels()
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    t0, t1 = _table(S_, M_ * B_, seed=5), _table(S_, M_ * B_, seed=6)
    a = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, _dp(opt), _so(opt))
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(a.round)), "ecg_tiny_cohort_round_capture")
    try:
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        a.table.copy_(t1)  # refilled in place between the replays
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    b = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, _dp(opt), _so(opt)).run()
    after_one, m_one = b.glob.clone(), b.m.clone()
    assert int(b.word.item()) == R0 + 1 and float(m_one.abs().max()) > 0
    if opt == "adam":
        assert not torch.equal(b.v, torch.full_like(b.v, TAU) ** 2)
    b.table.copy_(t1)
    b.run()
    assert not torch.equal(after_one, b.glob) and not torch.equal(after_one, glob) and not torch.equal(b.m, m_one)
    for u, v in zip(a.state(), b.state()):  # weights, client buffers, clip factors, round word, m, v
        assert torch.equal(u, v)
    assert int(a.word.item()) == R0 + 2
    # the second round read the first round's m: the same two rounds with m zeroed in between end elsewhere
    c = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, _dp(opt), _so(opt)).run()
    assert torch.equal(c.glob, after_one) and torch.equal(c.m, m_one)
    c.m.zero_()
    c.table.copy_(t1)
    c.run()
    assert not torch.equal(c.glob, a.glob) and not torch.equal(c.m, a.m) and torch.equal(c.scale, a.scale)


# ------------------------------------------------------------------------------------------------------ the trainer
def _trainer(x, y32, precision, use_graph=True, **kw):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    torch.manual_seed(3)
    model = TinyECG().to(x.device)
    return FusedCohortTrainer(model, x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                              seed=7, use_graph=use_graph, precision=precision, **kw)


def _tdp(opt):
    return dict(client_dp_clip=0.004, client_dp_noise=1.2, server_lr=0.8 if opt == "sgdm" else 0.01, server_opt=opt)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgdm", "yogi"])
def test_prepare_leaves_the_state_as_found(opt):
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, "bf16", **_tdp(opt))
    assert torch.equal(tr.server_m, torch.zeros_like(tr.server_m)) and tr.server_m.numel() == tr.P
    assert (tr.server_v is None) == (opt == "sgdm")
    tr.set_cohort_round(5)
    tr.run_round()  # (captures one graph) m and v now hold a round's update
    torch.cuda.synchronize()
    found = [t.clone() for t in (tr.params, tr.server_m, tr.cdp_round) + (() if tr.server_v is None else (tr.server_v,))]
    assert float(tr.server_m.abs().max()) > 0 and int(tr.cdp_round.item()) == 6
    tr.prepare([S_])  # warms both graphs (two replays), rolls back
    now = [tr.params, tr.server_m, tr.cdp_round] + ([] if tr.server_v is None else [tr.server_v])
    for u, v in zip(found, now):
        assert torch.equal(u, v)
    assert tr.cohort_round == 6
    tr.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgdm", "adam"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_resumed_trainer_reproduces_the_next_round_bitwise(precision, opt):
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, precision, **_tdp(opt))
    tr.prepare([S_])
    tr.run_round()
    torch.cuda.synchronize()
    weights, st = tr.params.clone(), tr.server_state()
    assert set(st) == ({"server_m"} if opt == "sgdm" else {"server_m", "server_v"}) and st["server_m"].device.type == "cpu"
    tr.run_round()
    torch.cuda.synchronize()

    def resumed(restore):
        re = _trainer(x, y32, precision, use_graph=False, **_tdp(opt))
        re.params.copy_(weights)
        if restore:
            re.load_server_state(st)
        re.set_cohort_round(1)
        re.run_round()
        torch.cuda.synchronize()
        out = (re.params.clone(), re.server_m.clone(), re.round_clients)
        re.close()
        return out

    p, m, clients = resumed(True)
    assert torch.equal(p, tr.params) and torch.equal(m, tr.server_m) and clients == tr.round_clients
    assert not torch.equal(resumed(False)[0], tr.params)  # a restarted optimizer takes another step
    tr.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", list(OPTS))
def test_fp32_trainer_against_the_torch_cohort_reference(opt):
    """Two fp32 rounds with client DP and a server optimizer, FusedCohortTrainer vs TorchCohortTrainer: relative l2
    difference of the global weights below 1e-5 (the project's fp32 bound) on an update of at least 1e-3."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, "fp32", world_size=2, **_tdp(opt))
    torch.manual_seed(3)
    ref_model = TinyECG().to(dev)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                             amp_dtype=None, seed=7, world_size=2, **_tdp(opt))
    P = tr.P
    start = tr.params[:P].clone()
    for _ in range(2):
        tr.run_round()
        ref.run_round(S_)
    torch.cuda.synchronize()
    assert tr.round_clients == ref.round_clients
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    moved = (want - start).norm().item() / want.norm().item()
    rel_m = (tr.server_m - ref.server_m).norm().item() / ref.server_m.norm().item()
    print(f"fp32 cohort rounds, {opt}, fused vs torch: relative l2 difference {rel:.3e} (update {moved:.3e}; m {rel_m:.3e})")
    assert rel < 1e-5, rel
    assert moved > 1e-3
    tr.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_server_opt_zero_is_the_round_without_the_new_fields(precision):
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    table = _table(S_, M_ * B_)
    # the mean close: a trainer with everything off leaves the new fields zero ...
    tr = _trainer(x, y32, precision)
    r = tr._round
    assert (r.server_opt, r.server_beta1, r.server_beta2, r.server_tau, r.server_m, r.server_v) == (0, 0.0, 0.0, 0.0, None, None)
    assert tr.server_m is None and tr.server_v is None and tr.server_state() == {} and not tr.client_dp
    tr.close()
    # ... and server_opt == 0 reads none of the other five, for the mean close and for the DP close
    off = dict(server_opt=0, server_beta1=7.0, server_beta2=-1.0, server_tau=-1.0)
    for dp in (None, DP):
        a = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, dp).run()  # the new fields not named
        b = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, dp)
        for k, val in off.items():
            setattr(b.round, k, val)
        b.run()
        assert not torch.equal(a.glob, glob)
        for u, v in zip(a.state(), b.state()):
            assert torch.equal(u, v)
    # sgdm without momentum is that DP close bit for bit in a whole round too
    a = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, DP).run()
    b = Cohort(x, y32, 2, M_, B_, S_, precision, table, glob, DP, _so("sgdm", server_beta1=0.0)).run()
    assert torch.equal(a.glob, b.glob) and torch.equal(a.scale, b.scale) and int(b.word.item()) == R0 + 1


def test_check_cohort_round_rejections():
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    table = _table(S_, M_ * B_)
    NODP = dict(DP, cdp_clip=0.0, cdp_sigma=0.0, server_lr=1.0)

    def fresh(opt="adam", dp=DP, **kw):
        return Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, dp, _so(opt, **kw))

    bad = 1  # kBadArg
    assert C.sizeof(_lib().TinyCohortRound) == _lib().kernels().ecg_tiny_cohort_round_sizeof()
    for opt in OPTS:
        assert fresh(opt).enqueue() == 0
    assert fresh("adam", NODP).enqueue() == 0  # an optimizer alone turns the two-launch close on
    for so in (dict(server_opt=5), dict(server_opt=-1), dict(server_beta1=1.0), dict(server_beta1=-0.1),
               dict(server_beta2=1.0), dict(server_beta2=-0.1), dict(server_tau=0.0), dict(server_tau=-1.0)):
        c = fresh()
        for k, val in so.items():
            setattr(c.round, k, val)
        assert c.enqueue() == bad, so
    for opt in ("adagrad", "yogi"):
        c = fresh(opt)
        c.round.server_tau = 0.0
        assert c.enqueue() == bad, opt
    c = fresh("sgdm")
    c.round.server_tau = 0.0  # sgdm has no tau, and takes no v
    assert c.round.server_v is None and c.enqueue() == 0
    for opt in OPTS:
        c = fresh(opt)
        c.round.server_m = None
        assert c.enqueue() == bad, opt
    for opt in ("adagrad", "adam", "yogi"):
        c = fresh(opt)
        c.round.server_v = None
        assert c.enqueue() == bad, opt
    for field in ("cdp_scale", "cdp_norm", "cdp_round"):  # the optimizer alone needs the DP close's buffers
        c = fresh("sgdm", NODP)
        setattr(c.round, field, None)
        assert c.enqueue() == bad, field
    g = C.c_void_p()
    c = fresh(server_beta1=1.0)
    assert _lib().kernels().ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == bad and not g.value
    # the stand-alone close checks its arguments the same way
    lib = _lib().kernels()
    gp, params = _clients(2, 3, 0.3)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    sc, nm = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    m, v = torch.zeros(num_params(2), device="cuda"), torch.ones(num_params(2), device="cuda")
    ok = [params.data_ptr(), gp.data_ptr(), 2, 3, 0.3, 1.0, 1.0, 1, w.data_ptr(), sc.data_ptr(), nm.data_ptr(), 3, B1, B2,
          TAU, m.data_ptr(), v.data_ptr(), None]
    for i, val in ((0, None), (1, None), (8, None), (9, None), (10, None), (2, 0), (3, 0), (3, 65536), (4, -1.0),
                   (5, -1.0), (6, -1.0), (11, 0), (11, 5), (12, 1.0), (13, -0.5), (14, 0.0), (15, None), (16, None)):
        args = list(ok)
        args[i] = val
        assert lib.ecg_cohort_server_close(*args) == bad, i
    args = list(ok)
    args[4] = 0.0  # noise without a clip norm
    assert lib.ecg_cohort_server_close(*args) == bad
    torch.cuda.synchronize()
    assert int(w.item()) == 0 and float(m.abs().max()) == 0.0  # nothing was launched
