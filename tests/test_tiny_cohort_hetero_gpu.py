"""Unequal virtual clients in the fused cohort round on the GPU: the STEPS form of the cohort reduce
(``EcgTinyCohortRound.client_steps``: a client that has run its local steps is frozen) and the weighted close
(``client_weight``: cohort_delta_wscale_kernel in front of the second kernel of every close).  Checked here: all
clients active and no weights against the round without the fields bitwise; a truncated client against an existing-path
round of its own step count bitwise; a captured graph replayed on rewritten device arrays; uniform power-of-two weights
against the unweighted closes bitwise; ``ecg_cohort_weighted_close`` against the definition in float64;
``FusedCohortTrainer`` on a Dirichlet partition against ``TorchCohortTrainer``; the argument checks.

Shapes: rounds with L in {33, 100}, nc in {2, 5}, B = 4, S = 5, M = 3 (steps (5, 2, 1) and (1, 5, 3)) or M = 4 (the
power-of-two weights), N = 64 windows; the stand-alone close with nc in {2, 5} and M in {1, 3, 9}."""
import ctypes as C

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

from cohort_harness import DELTA_CANARY, LR, MU, WD, Cohort, _clients, _data, _global, _lib, _table
from test_tiny_cohort_server_opt_gpu import _f, _step64  # the fused close's element-wise bound, as derived there

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
SEED = 0xC0FFEE1234567
R0 = (1 << 32) + 3
B_, S_ = 4, 5
B1, B2, TAU = 0.9, 0.99, 1e-3
OPTS = {"none": 0, "sgdm": 1, "adagrad": 2, "adam": 3, "yogi": 4}
NODP = dict(cdp_clip=0.0, cdp_sigma=0.0, server_lr=1.0, cdp_seed=SEED, round=R0)  # the close's buffers, nothing on
BAD = 1  # kBadArg
SHAPES = [(33, 5), (100, 2)]
NAMES = ("glob", "cparams", "cmom", "loss", "wprep", "scale", "norm", "word", "m", "v", "delta")


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _f32(vals):
    return torch.tensor(vals, dtype=torch.float32, device="cuda")


def _assert_same(a, b, names=NAMES):
    for n in names:
        u, v = getattr(a, n), getattr(b, n)
        assert (u is None) == (v is None), n
        if u is not None:
            assert torch.equal(u, v), n


def _graph_run(c, launches=1, between=None):
    L_ = _lib()
    lib = L_.kernels()
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)), "ecg_tiny_cohort_round_capture")
    try:
        for i in range(launches):
            if i and between:
                between()
            L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(c.glob.device)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    return c


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("L,nc", SHAPES)
def test_all_clients_active_and_no_weights_is_the_existing_round_bitwise(L, nc, precision):
    dev, x, y32 = _data(L, nc)
    glob, table, M = _global(nc), _table(S_, 3 * B_), 3
    for prox in (None, 0.05):
        a = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox).run()
        assert not torch.equal(a.glob, glob)
        # a round described without the fields, one that names them as null, one with every client active
        b = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox, client_steps=None, client_weight=None).run()
        c = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox, client_steps=_i32([S_] * M)).run()
        d = _graph_run(Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox, client_steps=_i32([S_, S_ + 3, S_])))
        for other in (b, c, d):
            _assert_same(a, other)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prox", [None, 0.05])
@pytest.mark.parametrize("steps", [(5, 2, 1), (1, 5, 3)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("L,nc", SHAPES)
def test_a_truncated_client_equals_a_round_of_its_own_step_count_bitwise(L, nc, precision, steps, prox):
    """Client c of a round with steps (s_0, .., s_{M-1}) ends on the weights, momentum, loss word (and bf16 image) of
    client c of an existing-path round of s_c steps on the same table and starting weights: no tolerance."""
    dev, x, y32 = _data(L, nc)
    glob, table, M = _global(nc), _table(S_, 3 * B_, seed=4), 3
    a = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox, client_steps=_i32(steps)).run()
    P = a.P
    for s in sorted(set(steps)):
        ref = Cohort(x, y32, nc, M, B_, s, precision, table, glob, prox_mu=prox).run()
        for c in (c for c in range(M) if steps[c] == s):
            assert torch.equal(a.cparams[c], ref.cparams[c]), (s, c)
            assert torch.equal(a.cmom[c], ref.cmom[c]) and float(ref.cmom[c, :P].abs().max()) > 0, (s, c)
            assert torch.equal(a.loss[c], ref.loss[c]) and float(ref.loss[c]) > 0, (s, c)
            if precision == "bf16":
                assert torch.equal(a.image(c), ref.image(c)), (s, c)
        if s < S_:  # the cut acts: the full round leaves these clients elsewhere
            full = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, prox_mu=prox).run()
            for c in (c for c in range(M) if steps[c] == s):
                assert not torch.equal(a.cparams[c], full.cparams[c])
    # the close is the mean of the clients as they ended
    want = a.cparams[0, :P].clone()
    for c in range(1, M):
        want += a.cparams[c, :P]
    assert torch.equal(a.glob, want * torch.tensor(1.0 / M, dtype=torch.float32, device=dev))


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_one_graph_replayed_on_rewritten_arrays_equals_enqueues_with_the_new_arrays(precision):
    dev, x, y32 = _data(100, 2)
    glob, table, M = _global(2), _table(S_, 3 * B_, seed=5), 3
    s0, s1 = (5, 2, 1), (1, 5, 3)
    w0, w1 = (0.5, 0.3, 0.2), (0.1, 0.25, 0.65)

    def fresh():
        return Cohort(x, y32, 2, M, B_, S_, precision, table, glob, NODP, client_steps=_i32(s0), client_weight=_f32(w0))

    a = fresh()
    st, w = a.keep

    def rewrite():  # on the device, between the replays: kernel arguments are baked into the graph, these are not
        st.copy_(_i32(s1))
        w.copy_(_f32(w1))

    _graph_run(a, 2, rewrite)
    b = fresh().run()
    one = b.glob.clone()
    b.keep[0].copy_(_i32(s1))
    b.keep[1].copy_(_f32(w1))
    b.run()
    _assert_same(a, b)
    assert int(a.word.item()) == R0 + 2 and torch.equal(a.scale, _f32(w1))
    # the arrays act: the same two rounds on the first arrays end elsewhere
    c = fresh().run()
    assert torch.equal(c.glob, one)
    c.run()
    assert not torch.equal(c.glob, a.glob) and not torch.equal(one, a.glob)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("close", ["dp_mean", "sgdm", "adam", "split"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_uniform_power_of_two_weights_are_the_unweighted_close_bitwise(precision, close):
    """client_weight = 0.25 for M = 4 against today's close with clip = 0: sum_c fma(0.25, d_c, .) is 0.25 times
    sum_c fma(1, d_c, .) exactly - scaling by a power of two commutes with every rounding, away from underflow (deltas
    of 1e-3 .. 1e-1 here) - and fma(s, 0.25, 0) = fma(0.25 s, 1, 0)."""
    dev, x, y32 = _data(100, 2)
    glob, M = _global(2), 4
    table = _table(S_, M * B_, seed=6)
    dp = dict(NODP, server_lr={"dp_mean": 0.8, "sgdm": 0.8, "adam": 0.01, "split": 1.0}[close])
    so = None
    if close in ("sgdm", "adam"):
        so = dict(server_opt=OPTS[close], server_beta1=B1, server_beta2=B2, server_tau=TAU)
    kw = dict(dp=dp, so=so, split=close == "split")
    a = Cohort(x, y32, 2, M, B_, S_, precision, table, glob, **kw).run()
    b = Cohort(x, y32, 2, M, B_, S_, precision, table, glob, client_weight=_f32([0.25] * M), **kw).run()
    c = _graph_run(Cohort(x, y32, 2, M, B_, S_, precision, table, glob, client_weight=_f32([0.25] * M), **kw))
    assert torch.equal(a.scale, torch.ones_like(a.scale)) and torch.equal(b.scale, _f32([0.25] * M))
    names = tuple(n for n in NAMES if n != "scale")
    _assert_same(a, b, names)
    _assert_same(a, c, names)
    if close == "split":
        assert torch.equal(a.glob, glob) and float(a.delta[: a.P].abs().max()) > 1e-4
        assert torch.equal(b.delta[a.P:], torch.full_like(b.delta[a.P:], DELTA_CANARY))
    else:
        assert not torch.equal(a.glob, glob)
    assert float(a.norm.min()) > 1e-3  # far from underflow


# 5 ---------------------------------------------------------------------------------------------------------------
def _weighted_close(params, glob, nc, M, weight, eta, word, opt, m=None, v=None, delta=None):
    L_ = _lib()
    scale = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    norm = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    st = L_.kernels().ecg_cohort_weighted_close(params.data_ptr(), glob.data_ptr(), nc, M, L_.ptr(weight), eta,
                                                word.data_ptr(), scale.data_ptr(), norm.data_ptr(), opt, B1, B2, TAU,
                                                L_.ptr(m), L_.ptr(v), L_.ptr(delta), L_.stream_ptr(glob.device))
    torch.cuda.synchronize()
    return st, scale, norm


WORST = {}


@pytest.mark.parametrize("M", [1, 3, 9])
@pytest.mark.parametrize("nc", [2, 5])
def test_weighted_close_against_the_definition_in_float64(nc, M):
    """Delta = sum_c w_c (p_c - g) in float64 on the fp32 inputs, then the plain step, every server optimizer and the
    split close.  The bound on Delta is the one tests/test_tiny_cohort_server_opt_gpu.py derives for the fused close
    with w_c s_c in place of s_c / M and nothing clipped or drawn (s_c = 1): (M + 8) 2^-23 sum_c w_c |d_c| element-wise
    (d_c = p_c - g is one rounding, each of the M fused multiply-adds one more on a partial sum below sum_c w_c |d_c|).
    From Delta on, ``_step64`` of that file for the optimizers; the plain step g + eta Delta is one fused
    multiply-add: eta e_D + 2^-24 (|g| + |eta Delta|); the split close stores Delta itself: e_D.
    Measured worst error / bound (MI355X): 0.096 (Delta), 0.964 (the plain step, M = 1: its bound is the half ulp
    of one fused multiply-add), 0.314 (the optimizers' weights)."""
    P = num_params(nc)
    g0, params = _clients(nc, M, 0.3)  # |d_c| = 1.2, 0.15, 0; NaN in the clients' padding floats
    gen = torch.Generator().manual_seed(100 * nc + M)
    weight = (torch.rand(M, generator=gen) * 1.5 + 0.05).cuda()
    w64 = weight.double().cpu().numpy()
    before = params.clone()
    g64 = g0.double().cpu().numpy()
    d = params[:, :P].double().cpu().numpy() - g64[None, :]
    delta = (w64[:, None] * d).sum(0)
    e_d = (M + 8) * EPS32 * (w64[:, None] * np.abs(d)).sum(0)
    assert np.isfinite(delta).all() and np.abs(delta).max() > 1e-3
    # the split close
    word = torch.tensor([R0], dtype=torch.int64, device="cuda")
    out = torch.full((P + 8,), DELTA_CANARY, dtype=torch.float32, device="cuda")
    g = g0.clone()
    st, scale, norm = _weighted_close(params, g, nc, M, weight, 0.0, word, 0, delta=out)
    assert st == 0 and torch.equal(g, g0) and int(word.item()) == R0 + 1
    assert torch.equal(scale, weight)  # s_c = 1: the weights as the second kernel reads them
    assert np.allclose(norm.double().cpu().numpy(), np.linalg.norm(d, axis=1), rtol=(P / 64 + 8) * EPS32, atol=0)
    assert torch.equal(out[P:], torch.full_like(out[P:], DELTA_CANARY))
    got = out[:P].double().cpu().numpy()
    assert np.isfinite(got).all()
    frac = float((np.abs(got - delta) / e_d.clip(1e-300)).max())
    WORST["delta"] = max(WORST.get("delta", 0.0), frac)
    print(f"weighted close nc {nc} M {M} split: worst error / bound {frac:.3f}")
    assert frac <= 1.0
    # the plain step and the four optimizers
    for opt, oid in OPTS.items():
        eta = 0.05 if oid >= 2 else 0.8
        g = g0.clone()
        m = torch.full((P,), 0.01, dtype=torch.float32, device="cuda") if oid else None
        v = torch.full((P,), 0.02, dtype=torch.float32, device="cuda") ** 2 if oid >= 2 else None
        m64 = None if m is None else m.double().cpu().numpy()
        v64 = None if v is None else v.double().cpu().numpy()
        st, scale, _ = _weighted_close(params, g, nc, M, weight, eta, word, oid, m, v)
        assert st == 0 and torch.equal(scale, weight)
        if oid == 0:
            want = g64 + _f(eta) * delta
            e_g = _f(eta) * e_d + 0.5 * EPS32 * (np.abs(g64) + np.abs(_f(eta) * delta))
        else:
            want, wm, wv, e_g, e_m, e_v = _step64(opt, g64, delta, e_d, m64, v64, eta, B1, B2, TAU)
            assert (np.abs(m.double().cpu().numpy() - wm) <= e_m).all(), opt
            if wv is not None:
                assert (np.abs(v.double().cpu().numpy() - wv) <= e_v).all(), opt
        got = g.double().cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got - g64).max() > 1e-4, opt
        frac = float((np.abs(got - want) / e_g).max())
        WORST["step"] = max(WORST.get("step", 0.0), frac)
        print(f"weighted close nc {nc} M {M} {opt}: worst error / bound {frac:.3f}")
        assert frac <= 1.0, opt
    assert torch.equal(params[:, :P], before[:, :P]) and int(word.item()) == R0 + 1 + len(OPTS)
    print(f"weighted close: worst error / bound so far {WORST}")


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["none", "adam"])
@pytest.mark.parametrize("aggregate", ["weighted", "nova"])
def test_fp32_trainer_on_a_dirichlet_partition_against_the_torch_cohort_reference(aggregate, opt):
    """Two fp32 rounds, Dirichlet partition (alpha 0.5), one local epoch, FusedCohortTrainer (graph replays) vs
    TorchCohortTrainer: relative l2 difference of the global weights below 1e-5, the siblings' bound.
    Measured (MI355X): see the README's item on unequal clients."""
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    dev, x, y32 = _data(100, 2)
    kw = dict(clients=4, cohort=3, lr=LR, momentum=MU, weight_decay=WD, seed=7, partition="dirichlet",
              dirichlet_alpha=0.5, local_epochs=1, aggregate=aggregate, server_opt=opt,
              server_lr=0.01 if opt == "adam" else 1.0)
    torch.manual_seed(3)
    tr = FusedCohortTrainer(TinyECG().to(dev), x, y32.long(), B_, S_, precision="fp32", **kw)
    torch.manual_seed(3)
    ref_model = TinyECG().to(dev)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), B_, S_, amp_dtype=None, **kw)
    P = tr.P
    start = tr.params[:P].clone()
    tr.prepare([S_])
    assert torch.equal(tr.params[:P], start)
    unequal = 0
    for _ in range(2):
        tr.run_round()
        ref.run_round(S_)
        assert tr.round_clients == ref.round_clients and tr.last_round_shape() == ref.last_round_shape()
        sizes, steps, weights = tr.last_round_shape()
        unequal += len(set(steps)) > 1 and len(set(sizes)) > 1
        st, w = tr._pairs[tr.idx_table.data_ptr()]
        assert st.tolist() == steps and w.tolist() == weights  # what the round's kernels read
    torch.cuda.synchronize()
    assert unequal == 2, "rounds with equal clients: the case checks nothing"
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    moved = (want - start).norm().item() / want.norm().item()
    loss, ref_loss = tr.avg_loss(), ref.avg_loss()
    print(f"fp32 cohort rounds, dirichlet, {aggregate}, {opt}, fused vs torch: relative l2 difference {rel:.3e} "
          f"(update {moved:.3e}; avg loss {loss:.6f} vs {ref_loss:.6f})")
    assert rel < 1e-5, rel
    assert moved > 1e-3
    assert abs(loss - ref_loss) < 1e-5 * ref_loss  # both divide by B * sum_c S_c
    tr.close()


# 7 ---------------------------------------------------------------------------------------------------------------
def test_rejections():
    dev, x, y32 = _data(100, 2)
    glob, M = _global(2), 3
    table = _table(S_, M * B_)
    lib = _lib().kernels()
    assert C.sizeof(_lib().TinyCohortRound) == lib.ecg_tiny_cohort_round_sizeof()

    def fresh(dp=NODP, **kw):
        return Cohort(x, y32, 2, M, B_, S_, "fp32", table, glob, dp, client_weight=_f32([0.2, 0.3, 0.5]), **kw)

    assert fresh().enqueue() == 0
    assert fresh(split=True).enqueue() == 0
    for field in ("cdp_scale", "cdp_norm", "cdp_round"):  # the weights need the close's buffers
        c = fresh()
        setattr(c.round, field, None)
        assert c.enqueue() == BAD, field
    c = Cohort(x, y32, 2, M, B_, S_, "fp32", table, glob, client_weight=_f32([0.2, 0.3, 0.5]))  # none of them
    assert c.enqueue() == BAD
    assert fresh(dict(NODP, cdp_clip=0.5)).enqueue() == BAD  # weights with a clip norm
    assert fresh(dict(NODP, cdp_clip=0.5, cdp_sigma=1.0)).enqueue() == BAD
    g = C.c_void_p()
    c = fresh(dict(NODP, cdp_clip=0.5))
    assert lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == BAD and not g.value
    torch.cuda.synchronize()
    assert torch.equal(c.glob, glob) and int(c.word.item()) == R0  # nothing was launched
    # the stand-alone entries
    gp, params = _clients(2, 3, 0.3)
    w = torch.zeros(1, dtype=torch.int64, device="cuda")
    wt = _f32([0.2, 0.3, 0.5])
    st, _, _ = _weighted_close(params, gp.clone(), 2, 3, None, 1.0, w, 0)
    assert st == BAD
    m = torch.zeros(num_params(2), device="cuda")
    assert _weighted_close(params, gp.clone(), 2, 3, wt, 1.0, w, 3, m, None)[0] == BAD  # adam without v
    assert _weighted_close(params, gp.clone(), 2, 3, wt, 1.0, w, 5, m, m.clone())[0] == BAD
    assert _weighted_close(params, gp.clone(), 2, 0, wt, 1.0, w, 0)[0] == BAD
    assert int(w.item()) == 0
    a = Cohort(x, y32, 2, M, B_, S_, "fp32", table, glob)
    ok = [a.slab.data_ptr(), B_, M, a.slab.shape[1], a.P, a.cparams.data_ptr(), a.cmom.data_ptr(), a.loss.data_ptr(),
          LR, MU, WD, 0, None, None, 0.0, _i32([1, 1, 1]).data_ptr(), 0, None]
    for i, val in ((0, None), (2, 0), (2, 65536), (15, None), (16, -1), (5, None), (6, None)):
        args = list(ok)
        args[i] = val
        assert lib.ecg_slab_reduce_cohort_steps_sgd(*args) == BAD, i
    args = list(ok)
    args[14] = 0.1  # a proximal term without its anchor
    assert lib.ecg_slab_reduce_cohort_steps_sgd(*args) == BAD
    torch.cuda.synchronize()
    assert float(a.cparams.abs().max()) == 0.0 and float(a.loss.abs().max()) == 0.0


def test_steps_reduce_entry_freezes_exactly_the_finished_clients():
    """``ecg_slab_reduce_cohort_steps_sgd`` on a slab of known rows: clients with client_steps[c] > step take the
    update of ``ecg_slab_reduce_cohort_prox_sgd`` bitwise, the others keep weights, momentum and loss word."""
    L_ = _lib()
    lib = L_.kernels()
    nc, M = 5, 3
    P, ps = num_params(nc), lib.ecg_tiny_cohort_param_stride(nc)
    from crossscale_ecg.ops.fused_tiny import slab_stride
    stride = slab_stride(nc)
    gen = torch.Generator().manual_seed(9)
    slab = torch.randn(M * B_, stride, generator=gen).cuda()
    p0 = torch.randn(M, ps, generator=gen).cuda()
    m0 = torch.randn(M, ps, generator=gen).cuda()
    anchor = torch.randn(P, generator=gen).cuda()
    for mu in (0.0, 0.3):
        ref_p, ref_m, ref_l = p0.clone(), m0.clone(), torch.zeros(M, device="cuda")
        L_.check(lib.ecg_slab_reduce_cohort_prox_sgd(slab.data_ptr(), B_, M, stride, P, ref_p.data_ptr(), ref_m.data_ptr(),
                                                     ref_l.data_ptr(), LR, MU, WD, 0, None, anchor.data_ptr(), mu,
                                                     L_.stream_ptr(slab.device)), "ecg_slab_reduce_cohort_prox_sgd")
        for step, steps in ((0, (1, 1, 1)), (1, (2, 1, 5)), (4, (4, 5, 1)), (2, (1, 2, 2))):
            p, m, l = p0.clone(), m0.clone(), torch.zeros(M, device="cuda")
            L_.check(lib.ecg_slab_reduce_cohort_steps_sgd(slab.data_ptr(), B_, M, stride, P, p.data_ptr(), m.data_ptr(),
                                                          l.data_ptr(), LR, MU, WD, 0, None, anchor.data_ptr(), mu,
                                                          _i32(steps).data_ptr(), step, L_.stream_ptr(slab.device)),
                     "ecg_slab_reduce_cohort_steps_sgd")
            torch.cuda.synchronize()
            for c in range(M):
                live = steps[c] > step
                assert torch.equal(p[c], ref_p[c] if live else p0[c]), (mu, step, c)
                assert torch.equal(m[c], ref_m[c] if live else m0[c]), (mu, step, c)
                assert float(l[c]) == (float(ref_l[c]) if live else 0.0), (mu, step, c)
        assert not torch.equal(ref_p[:, :P], p0[:, :P])
