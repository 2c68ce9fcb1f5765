"""Client-level DP close of a cohort round on the GPU (cohort_delta_scale_kernel + cohort_dp_mean_kernel): the stand-alone
close against the definition in float64 numpy, its noise against utils/philox.py, whole rounds (graph replay against
enqueue, the round word, prepare / resume), the trainer against ``TorchCohortTrainer``, the flags-off path against a
round built without the new fields, and the argument checks.

The definition: d_c = p_c - g, n_c = |d_c|_2, s_c = min(1, C / n_c) (n_c == 0 -> 1),
g_new = g + eta * ((sum_c s_c d_c, ascending c) * fp32(1 / M) + nu * z), nu = sigma * C / M for one rank,
z = philox.normal(seed, round, P, stream=1).

Shapes: the stand-alone close with nc in {2, 5} and M in {1, 3, 5, 9} (4 clients per block: one block, a partial block,
several blocks); rounds with L in {100, 99}, B = 4, S = 2, N = 64 windows."""
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


def _close(params, glob, nc, M, clip, sigma, eta, seed, r):
    """ecg_cohort_dp_close on copies: (new global, scale, norm, round word afterwards)."""
    L_ = _lib()
    out = glob.clone()
    scale = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    norm = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    word = torch.tensor([r], dtype=torch.int64, device="cuda")
    L_.check(L_.kernels().ecg_cohort_dp_close(params.data_ptr(), out.data_ptr(), nc, M, clip, sigma, eta, seed,
                                              word.data_ptr(), scale.data_ptr(), norm.data_ptr(),
                                              L_.stream_ptr(glob.device)), "ecg_cohort_dp_close")
    torch.cuda.synchronize()
    return out, scale, norm, int(word.item())


def _definition(params, glob, P, M, clip, nu, eta, seed, r):
    """(g_new, norms, factors, z, mean_c |d_c|) of the definition in float64 on the fp32 inputs."""
    g = glob.double().cpu().numpy()
    d = params[:, :P].double().cpu().numpy() - g[None, :]
    n = np.linalg.norm(d, axis=1)
    s = np.array([1.0 if v == 0 else min(1.0, clip / v) for v in n])
    z = philox.normal(seed, r, P, stream=1) if nu != 0 else np.zeros(P)
    return g + eta * ((s[:, None] * d).sum(0) / M + nu * z), n, s, z, np.abs(d).mean(0)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 5, 9])
@pytest.mark.parametrize("nc", [2, 5])
def test_close_against_the_definition_in_float64(nc, M):
    clip, sigma, eta = 0.3, 1.5, 0.7
    P = num_params(nc)
    g, params = _clients(nc, M, clip)
    before = params.clone()
    got, scale, norm, word = _close(params, g, nc, M, clip, sigma, eta, SEED, R0)
    nu = sigma * clip / M
    want, n, s, z, dmean = _definition(params, g, P, M, clip, nu, eta, SEED, R0)
    assert word == R0 + 1  # the round counter advanced by one
    assert torch.equal(params[:, :P], before[:, :P]) and bool(torch.isnan(params[:, P:]).all())  # read only
    # factors: 1 for the zero and the small deltas, < 1 for the large ones; both kinds occur from M = 2 on
    sc = scale.cpu().numpy()
    assert np.all(sc[s == 1.0] == 1.0) and np.all(sc[s < 1.0] < 1.0) and bool((sc < 1.0).any())
    assert bool((sc == 1.0).any()) == (M >= 2)
    assert np.all(np.abs(sc - s) <= (P / 64 + 8) * EPS32 * s)
    # norms: P squares summed per lane in column order, then six butterfly steps
    nm = norm.cpu().numpy()
    rel = np.abs(nm - n) / np.where(n > 0, n, 1.0)
    print(f"nc={nc} M={M}: worst relative norm error {rel.max():.3e} (bound {(P / 64 + 8) * EPS32:.3e})")
    assert np.all(rel <= (P / 64 + 8) * EPS32) and np.all(nm[n == 0] == 0.0)
    # the new global weights: the fp32 operation count, plus the device-vs-numpy Box-Muller difference on nu * z
    bound = (M + 8) * EPS32 * (np.abs(g.double().cpu().numpy()) + eta * (dmean + nu * np.abs(z))) + 4e-6 * eta * nu
    err = np.abs(got.double().cpu().numpy() - want)
    print(f"nc={nc} M={M}: worst error / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound), float((err / bound).max())
    assert not torch.equal(got, g)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [1e30, 0.0])  # a huge clip norm; clip == 0: no clipping
@pytest.mark.parametrize("M", [3, 9])
def test_no_noise_no_clipping_is_the_plain_mean(M, clip):
    nc = 2
    P = num_params(nc)
    g, params = _clients(nc, M, 0.3)
    got, scale, norm, _ = _close(params, g, nc, M, clip, 0.0, 1.0, SEED, R0)
    assert bool((scale == 1.0).all()) and float(norm.max()) > 1.0
    mean = params[:, :P].double().cpu().numpy().mean(0)
    _, _, _, _, dmean = _definition(params, g, P, M, 1e30, 0.0, 1.0, SEED, R0)
    bound = (M + 8) * EPS32 * (np.abs(g.double().cpu().numpy()) + dmean)
    assert np.all(np.abs(got.double().cpu().numpy() - mean) <= bound)
    # server_lr == 0 means 1 (an all-zero struct field)
    again, _, _, _ = _close(params, g, nc, M, clip, 0.0, 0.0, SEED, R0)
    assert torch.equal(again, got)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_noise_kernel_matches_the_numpy_twin_on_its_own_stream():
    L_ = _lib()
    lib = L_.kernels()
    P = num_params(5)
    z1 = torch.zeros(P, dtype=torch.float32, device="cuda")
    z0 = torch.zeros(P, dtype=torch.float32, device="cuda")
    L_.check(lib.ecg_cohort_dp_noise(z1.data_ptr(), P, SEED, R0, L_.stream_ptr(z1.device)), "ecg_cohort_dp_noise")
    L_.check(lib.ecg_dp_noise(z0.data_ptr(), P, SEED, R0, L_.stream_ptr(z0.device)), "ecg_dp_noise")
    torch.cuda.synchronize()
    want = philox.normal(SEED, R0, P, stream=1)
    err = np.abs(z1.double().cpu().numpy() - want).max()
    print(f"cohort DP noise, device vs numpy: worst absolute difference {err:.3e}")
    assert err <= 4e-6, err
    assert np.abs(z0.double().cpu().numpy() - philox.normal(SEED, R0, P)).max() <= 4e-6  # the DP-SGD stream as before
    assert not bool((z0 == z1).any())  # the same (seed, t) on the two streams: other values
    assert lib.ecg_cohort_dp_noise(None, P, SEED, R0, None) == 1 and lib.ecg_cohort_dp_noise(z1.data_ptr(), 0, 1, 1, None) == 1


# ------------------------------------------------------------------------------------------------------ whole rounds
M_, B_, S_ = 3, 4, 2
DP = dict(cdp_clip=0.004, cdp_sigma=1.2, server_lr=0.8, cdp_seed=SEED, round=R0)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_graph_replayed_twice_equals_two_enqueued_rounds_bitwise(precision):
    L_ = _lib()
    lib = L_.kernels()
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    t0, t1 = _table(S_, M_ * B_, seed=5), _table(S_, M_ * B_, seed=6)
    a = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, DP)
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(a.round)), "ecg_tiny_cohort_round_capture")
    try:
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        a.table.copy_(t1)  # refilled in place between the replays
        L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(dev)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    b = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, DP).run()
    after_one, scale_one = b.glob.clone(), b.scale.clone()
    assert int(b.word.item()) == R0 + 1
    b.table.copy_(t1)
    b.run()
    assert not torch.equal(after_one, b.glob) and not torch.equal(after_one, glob)
    for u, v in zip(a.state(), b.state()):
        assert torch.equal(u, v)
    assert int(a.word.item()) == R0 + 2  # the word advanced once per replay
    # the second replay drew round R0 + 1's noise, not R0's again: the same two rounds with the word put back to R0
    # before the second one end eta * nu * (z(R0 + 1) - z(R0)) away from the replays, and differ in nothing else
    c = Cohort(x, y32, 2, M_, B_, S_, precision, t0.clone(), glob, DP).run()
    assert torch.equal(c.glob, after_one) and torch.equal(c.scale, scale_one) and bool((c.scale < 1.0).any())
    c.word.fill_(R0)
    c.table.copy_(t1)
    c.run()
    assert torch.equal(c.scale, a.scale) and int(c.word.item()) == R0 + 1
    nu = DP["cdp_sigma"] * DP["cdp_clip"] / M_
    dz = philox.normal(SEED, R0 + 1, a.P, stream=1) - philox.normal(SEED, R0, a.P, stream=1)
    diff = (a.glob.double() - c.glob.double()).cpu().numpy()
    assert np.abs(diff).max() > 1e-4 and np.abs(diff - DP["server_lr"] * nu * dz).max() < 1e-6


# 5 ---------------------------------------------------------------------------------------------------------------
def _trainer(x, y32, precision, use_graph=True, **kw):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    torch.manual_seed(3)
    model = TinyECG().to(x.device)
    return FusedCohortTrainer(model, x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                              seed=7, use_graph=use_graph, precision=precision, **kw)


TDP = dict(client_dp_clip=0.004, client_dp_noise=1.2, server_lr=0.8)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_prepare_set_cohort_round_and_resume(precision):
    dev, x, y32 = _data(99, 2)
    tr = _trainer(x, y32, precision, **TDP)
    assert int(tr.cdp_round.item()) == 0
    tr.set_cohort_round(5)
    assert int(tr.cdp_round.item()) == 5 and tr.cohort_round == 5
    start = tr.params.clone()
    tr.prepare([S_])  # warms both graphs (two replays), rolls back
    assert torch.equal(tr.params, start) and int(tr.cdp_round.item()) == 5 and tr.cohort_round == 5
    tr.set_cohort_round(0)
    after = []
    for _ in range(3):
        tr.run_round()
        torch.cuda.synchronize()
        after.append(tr.params.clone())
    assert int(tr.cdp_round.item()) == 3 and tr.cohort_round == 3
    norms, clipped = tr.last_clip_stats()
    assert len(norms) == M_ and all(n > 0 for n in norms) and 0.0 < clipped <= 1.0
    # a trainer resumed at round 2 from the weights after round 1 reproduces round 2
    re = _trainer(x, y32, precision, use_graph=False, **TDP)
    re.params.copy_(after[1])
    re.set_cohort_round(2)
    re.run_round()
    torch.cuda.synchronize()
    assert torch.equal(re.params, after[2]) and re.round_clients == tr.round_clients
    assert not torch.equal(after[2], after[1])
    tr.close()
    re.close()


# 6 ---------------------------------------------------------------------------------------------------------------
def test_fp32_trainer_against_the_torch_cohort_reference_with_client_dp():
    """Two fp32 rounds with client DP, FusedCohortTrainer vs TorchCohortTrainer: relative l2 difference of the global
    weights below 1e-5, the bound of tests/test_tiny_cohort_gpu.py's fp32 reference test.  Measured: 1.4e-8."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, "fp32", world_size=2, **TDP)
    torch.manual_seed(3)
    ref_model = TinyECG().to(dev)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), B_, S_, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                             amp_dtype=None, seed=7, world_size=2, **TDP)
    P = tr.P
    start = tr.params[:P].clone()
    for _ in range(2):
        tr.run_round()
        ref.run_round(S_)
    torch.cuda.synchronize()
    assert tr.round_clients == ref.round_clients and tr.cdp_seed == ref.cdp_seed
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    moved = (want - start).norm().item() / want.norm().item()
    print(f"fp32 cohort rounds with client DP, fused vs torch: relative l2 difference {rel:.3e} (update {moved:.3e})")
    assert rel < 1e-5, rel
    assert moved > 1e-3
    n_f, c_f = tr.last_clip_stats()
    n_t, c_t = ref.last_clip_stats()
    assert np.allclose(n_f, n_t, rtol=1e-4) and c_f == c_t and c_f > 0
    tr.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_flags_off_is_the_round_without_the_new_fields(precision):
    dev, x, y32 = _data(100, 2)
    tr = _trainer(x, y32, precision, client_dp_clip=0.0, client_dp_noise=0.0, server_lr=1.0)
    assert not tr.client_dp and tr.cdp_round is None
    r = tr._round
    assert (r.cdp_clip, r.cdp_sigma, r.server_lr, r.cdp_seed, r.cdp_scale, r.cdp_norm, r.cdp_round) == \
        (0.0, 0.0, 0.0, 0, None, None, None)
    P = tr.P
    start = tr.params.clone()
    tr.run_round()
    torch.cuda.synchronize()
    co = Cohort(x, y32, 2, M_, B_, S_, precision, tr.idx_table.clone(), start[:P]).run()  # dp=None: fields not named
    assert torch.equal(co.glob, tr.params[:P]) and not torch.equal(co.glob, start[:P])
    assert torch.equal(co.loss, tr.loss_acc)
    # ... which is the mean of the clients in ascending order (cohort_mean_kernel's result)
    s = co.cparams[0, :P].clone()
    for c in range(1, M_):
        s = s + co.cparams[c, :P]
    assert torch.equal(co.glob, s * torch.tensor(1.0 / M_, dtype=torch.float32))
    assert tr.last_clip_stats() == ([], 0.0)
    tr.close()


# 8 ---------------------------------------------------------------------------------------------------------------
def test_check_cohort_round_rejections():
    dev, x, y32 = _data(100, 2)
    glob = _global(2)
    table = _table(S_, M_ * B_)

    def fresh(**kw):
        return Cohort(x, y32, 2, M_, B_, S_, "fp32", table, glob, dict(DP, **kw))

    bad = 1  # kBadArg
    assert C.sizeof(_lib().TinyCohortRound) == _lib().kernels().ecg_tiny_cohort_round_sizeof()
    assert fresh().enqueue() == 0
    for kw in (dict(cdp_clip=-1.0), dict(cdp_sigma=-0.5), dict(server_lr=-1.0), dict(cdp_clip=0.0, cdp_sigma=1.0)):
        assert fresh(**kw).enqueue() == bad, kw
    for field in ("cdp_scale", "cdp_norm", "cdp_round"):
        c = fresh()
        setattr(c.round, field, None)
        assert c.enqueue() == bad, field
        c = fresh(cdp_clip=0.0, cdp_sigma=0.0, server_lr=0.5)  # the server step alone needs the buffers too
        setattr(c.round, field, None)
        assert c.enqueue() == bad, field
        c = fresh(cdp_clip=0.0, cdp_sigma=0.0, server_lr=1.0)  # nothing on: the pointers are not needed
        setattr(c.round, field, None)
        assert c.enqueue() == 0, field
    g = C.c_void_p()
    c = fresh(cdp_clip=-1.0)
    assert _lib().kernels().ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == bad and not g.value
    # the stand-alone close checks its arguments the same way
    lib = _lib().kernels()
    gp, params = _clients(2, 3, 0.3)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    sc, nm = torch.zeros(3, device="cuda"), torch.zeros(3, device="cuda")
    ok = [params.data_ptr(), gp.data_ptr(), 2, 3, 0.3, 1.0, 1.0, 1, w.data_ptr(), sc.data_ptr(), nm.data_ptr(), None]
    for i, v in ((0, None), (1, None), (8, None), (9, None), (10, None), (2, 0), (3, 0), (3, 65536), (4, -1.0), (5, -1.0), (6, -1.0)):
        args = list(ok)
        args[i] = v
        assert lib.ecg_cohort_dp_close(*args) == bad, i
    args = list(ok)
    args[4] = 0.0  # noise without a clip norm
    assert lib.ecg_cohort_dp_close(*args) == bad
    torch.cuda.synchronize()
    assert int(w.item()) == 0  # nothing was launched
