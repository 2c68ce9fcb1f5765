"""Robust aggregation in the close of a fused cohort round on the GPU: ``cohort_robust_delta_kernel`` (the coordinate-wise
trimmed mean of the clients' deltas; the median at k = (M - 1) // 2), ``ecg_cohort_robust_close`` and the
``robust_trim`` / ``robust_scratch`` fields of ``EcgTinyCohortRound``.  Checked here: the stand-alone close against a
numpy float32 emulation of the definition (``train/cohort.py``'s ``robust_delta``) bitwise; the non-split close against
the split close plus ``ecg_server_opt_step`` bitwise; NaN and infinite clients; the float64 bound; the argument checks;
rounds (enqueue against graph replays, against the stand-alone close on a mean round's client weights, fields zero
against a round without them, with ``client_steps``); ``FusedCohortTrainer`` against ``TorchCohortTrainer``, resume,
flipped labels.

Shapes: L = 100, B = 4, S = 3, nc in {2, 5}, N = 64 windows; the stand-alone close with (M, k) from (3, 1) to (64, 31)."""
import ctypes as C

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params

from cohort_harness import DELTA_CANARY, LR, MU, WD, Cohort, _data, _global, _lib, _table

pytestmark = pytest.mark.gpu

F32 = np.float32
R0 = (1 << 32) + 3
L_, B_, S_ = 100, 4, 3
B1, B2, TAU = 0.9, 0.99, 1e-3
OPTS = {"none": 0, "sgdm": 1, "adam": 3, "yogi": 4}
NODP = dict(cdp_clip=0.0, cdp_sigma=0.0, server_lr=1.0, cdp_seed=7, round=R0)  # the close's buffers, nothing on
BAD = 1  # kBadArg
MK = [(3, 1), (4, 1), (5, 2), (8, 1), (8, 3), (9, 4), (33, 5), (64, 1), (64, 31)]
NAMES = ("glob", "cparams", "cmom", "loss", "wprep", "scale", "norm", "word", "m", "v")


# ------------------------------------------------------------------------------------------------ the definition
def emulate(params, g, k):
    """The issue's definition on numpy float32: ``params`` [M, P], ``g`` [P] -> Delta [P] (float32)."""
    M = params.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        x = (params.astype(F32) - g.astype(F32)[None, :]).astype(F32)
        b = x.view(np.uint32).astype(np.int64)
        key = np.where((b >> 31) != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)
        key[np.isnan(x)] = 0xFFFFFFFF
        c = np.arange(M)[:, None]
        rank = np.zeros_like(key)
        for j in range(M):
            rank += ((key[j] < key) | ((key[j] == key) & (j < c))).astype(np.int64)
        assert (np.sort(rank, axis=0) == c).all()  # a permutation per parameter
        kept = (rank >= k) & (rank < M - k)
        s = np.full(x.shape[1], -0.0, dtype=F32)  # -0 + x is x bit for bit
        for j in range(M):
            s = np.where(kept[j], (s + x[j]).astype(F32), s)
        return (s * (F32(1.0) / F32(M - 2 * k))).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def make_clients(nc, M, seed=0):
    """(g [P], params [M, pstride]) on the device: random deltas of about 0.05 with exact ties across clients at every
    third parameter, +0 / -0 deltas at every seventh, and NaN in every client's pstride - P padding floats."""
    P, ps = num_params(nc), _lib().kernels().ecg_tiny_cohort_param_stride(nc)
    g = _global(nc).cpu().numpy().copy()
    rng = np.random.default_rng(1000 * nc + 10 * M + seed)
    d = (rng.standard_normal((M, P)) * 0.05).astype(F32)
    i = np.arange(P)
    tie = i % 3 == 0
    d[1::2, tie] = d[0:2 * (M // 2):2, tie]  # clients 2a and 2a + 1 agree (p_c equal, so x_c equal exactly)
    if M >= 4:
        d[3, i % 6 == 0] = d[0, i % 6 == 0]  # three equal values
    p = (g[None, :] + d).astype(F32)
    zero = i % 7 == 1
    g[zero] = 0.0
    p[:, zero] = (rng.standard_normal((M, int(zero.sum()))) * 0.05).astype(F32)
    p[0::2, i % 14 == 1] = -0.0  # x = -0 - (+0) = -0 on the even clients, +0 on the odd ones
    p[1::2, i % 14 == 1] = 0.0
    p[0, i % 14 == 8], p[M - 1, i % 14 == 8] = 0.0, -0.0  # one pair among random values
    params = torch.full((M, ps), float("nan"), dtype=torch.float32, device="cuda")
    params[:, :P] = torch.from_numpy(p).cuda()
    return torch.from_numpy(g).cuda(), params


def robust_close(params, glob, nc, M, k, eta, word, opt=0, m=None, v=None, delta=None, scratch=None):
    lib = _lib()
    scale = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    norm = torch.full((M,), -1.0, dtype=torch.float32, device="cuda")
    st = lib.kernels().ecg_cohort_robust_close(params.data_ptr(), glob.data_ptr(), nc, M, k, eta, lib.ptr(word),
                                               scale.data_ptr(), norm.data_ptr(), opt, B1, B2, TAU, lib.ptr(m),
                                               lib.ptr(v), lib.ptr(delta), lib.ptr(scratch), lib.stream_ptr(glob.device))
    torch.cuda.synchronize()
    return st, scale, norm


def split_delta(params, g, nc, M, k, word=None):
    """The split robust close: (status, Delta [P] as numpy, the output buffer with its canary, scale, norm)."""
    P = num_params(nc)
    word = torch.tensor([R0], dtype=torch.int64, device="cuda") if word is None else word
    out = torch.full((P + 8,), DELTA_CANARY, dtype=torch.float32, device="cuda")
    st, scale, norm = robust_close(params, g, nc, M, k, 0.0, word, delta=out)
    return st, out[:P].cpu().numpy(), out, scale, norm


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k", MK)
@pytest.mark.parametrize("nc", [2, 5])
def test_split_close_equals_the_definition_bitwise(nc, M, k):
    P = num_params(nc)
    g, params = make_clients(nc, M)
    g0, before = g.clone(), params.clone()
    word = torch.tensor([R0], dtype=torch.int64, device="cuda")
    st, got, out, scale, norm = split_delta(params, g, nc, M, k, word)
    assert st == 0 and torch.equal(g, g0) and int(word.item()) == R0 + 1
    assert torch.equal(params[:, :P], before[:, :P])
    assert torch.equal(out[P:], torch.full_like(out[P:], DELTA_CANARY))  # delta[i] for i < P and nothing else
    assert torch.equal(scale, torch.ones_like(scale))  # no clip: every factor is 1; the norms are still reported
    pn, gn = params[:, :P].cpu().numpy(), g.cpu().numpy()
    d64 = pn.astype(np.float64) - gn.astype(np.float64)[None, :]
    assert np.allclose(norm.double().cpu().numpy(), np.linalg.norm(d64, axis=1), rtol=(P / 64 + 8) * 2.0 ** -23, atol=0)
    want = emulate(pn, gn, k)
    assert np.isfinite(got).all()  # the padding's NaN was not read
    assert (bits(got) == bits(want)).all(), int((bits(got) != bits(want)).sum())
    # the inputs do what they are there for: a trim that acts, zeros of both signs among the results (the median of
    # an odd cohort is the last of its -0 values where the even clients hold -0 and the odd ones +0)
    assert np.abs(got - d64.mean(0)).max() > 1e-4
    assert (bits(got) == 0).any()
    if M % 2 == 1 and k == (M - 1) // 2:
        assert (bits(got) == 0x80000000).any()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", list(OPTS))
@pytest.mark.parametrize("nc,M,k", [(2, 8, 2), (5, 5, 2)])
def test_non_split_close_equals_split_close_then_server_step_bitwise(nc, M, k, opt):
    lib = _lib()
    P, oid = num_params(nc), OPTS[opt]
    eta = 0.05 if oid >= 2 else 0.8
    g0, params = make_clients(nc, M, seed=1)

    def state():
        m = torch.full((P,), 0.01, dtype=torch.float32, device="cuda") if oid else None
        v = torch.full((P,), 0.02, dtype=torch.float32, device="cuda") ** 2 if oid >= 2 else None
        return g0.clone(), m, v

    g, m, v = state()
    word = torch.tensor([R0], dtype=torch.int64, device="cuda")
    scratch = torch.full((P + 8,), DELTA_CANARY, dtype=torch.float32, device="cuda")
    st, _, _ = robust_close(params, g, nc, M, k, eta, word, oid, m, v, scratch=scratch)
    assert st == 0 and int(word.item()) == R0 + 1 and not torch.equal(g, g0)
    assert torch.equal(scratch[P:], torch.full_like(scratch[P:], DELTA_CANARY))
    g2, m2, v2 = state()
    st, _, out, _, _ = split_delta(params, g2, nc, M, k)
    assert st == 0 and torch.equal(out[:P], scratch[:P])
    lib.check(lib.kernels().ecg_server_opt_step(g2.data_ptr(), out.data_ptr(), P, oid, eta, B1, B2, TAU, lib.ptr(m2),
                                                lib.ptr(v2), lib.stream_ptr(g2.device)), "ecg_server_opt_step")
    torch.cuda.synchronize()
    assert torch.equal(g, g2)
    for a, b in ((m, m2), (v, v2)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    if oid:
        assert not torch.equal(m, torch.full_like(m, 0.01))


# 3 ---------------------------------------------------------------------------------------------------------------
def test_bad_clients_are_trimmed_away_up_to_k_and_propagate_beyond():
    nc, M, k = 5, 8, 1
    P = num_params(nc)
    g, params = make_clients(nc, M, seed=2)
    clean = params.clone()
    # one client all NaN; one at +inf and one at -inf
    for poison in ({3: float("nan")}, {1: float("inf"), 6: float("-inf")}):
        params.copy_(clean)
        for c, val in poison.items():
            params[c, :P] = val
        st, got, _, _, _ = split_delta(params, g, nc, M, k)
        want = emulate(params[:, :P].cpu().numpy(), g.cpu().numpy(), k)
        assert st == 0 and np.isfinite(got).all() and np.isfinite(want).all()
        assert (bits(got) == bits(want)).all()
    # two NaN clients, one of them only at every other parameter: NaN exactly where two values are NaN
    params.copy_(clean)
    params[3, :P] = float("nan")
    params[5, 0:P:2] = float("nan")
    st, got, _, _, _ = split_delta(params, g, nc, M, k)
    want = emulate(params[:, :P].cpu().numpy(), g.cpu().numpy(), k)
    assert st == 0 and np.array_equal(got, want, equal_nan=True)
    where = np.zeros(P, dtype=bool)
    where[0:P:2] = True
    assert (np.isnan(got) == where).all() and (np.isnan(want) == where).all()
    fin = ~where
    assert (bits(got[fin]) == bits(want[fin])).all()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,k", MK)
def test_split_close_within_the_float64_bound(M, k):
    """|Delta - robust_delta_f64| <= (n + 1) 2^-24 sum over the kept |x_c| per element: one rounding per subtraction,
    n - 1 adds and one product, each at most 2^-24 of a quantity below that sum.  Asserted as the worst fraction of the
    bound.  Measured (MI355X): see the README's item on robust aggregation."""
    from crossscale_ecg.train.cohort import robust_delta_f64
    nc = 5
    P, n = num_params(nc), M - 2 * k
    g, params = make_clients(nc, M, seed=3)
    st, got, _, _, _ = split_delta(params, g, nc, M, k)
    assert st == 0
    stack, g64 = params[:, :P].cpu(), g.cpu()
    want = robust_delta_f64(stack, g64, k).numpy()
    x = np.sort(stack.double().numpy() - g64.double().numpy()[None, :], axis=0)[k:M - k]
    bound = (n + 1) * 2.0 ** -24 * np.abs(x).sum(0)
    err = np.abs(got.astype(np.float64) - want)
    frac = float((err / np.maximum(bound, 1e-300)).max())
    print(f"robust close M {M} k {k}: worst error / bound {frac:.3f}")
    assert (err[bound == 0] == 0).all() and frac <= 1.0


# 5 ---------------------------------------------------------------------------------------------------------------
def test_native_checks():
    dev, x, y32 = _data(L_, 2)
    glob, M, P = _global(2), 3, num_params(2)
    table = _table(S_, M * B_)
    lib = _lib().kernels()
    assert C.sizeof(_lib().TinyCohortRound) == lib.ecg_tiny_cohort_round_sizeof()

    def fresh(dp=NODP, trim=1, scratch=True, **kw):
        sc = torch.zeros(P, device="cuda") if scratch else None
        return Cohort(x, y32, 2, M, B_, S_, "fp32", table, glob, dp, robust_trim=trim, robust_scratch=sc, **kw)

    assert fresh().enqueue() == 0
    assert fresh(split=True, scratch=False).enqueue() == 0  # the split close needs no scratch
    assert fresh(scratch=False).enqueue() == BAD  # a null scratch without delta
    assert fresh(trim=-1).enqueue() == BAD
    assert fresh(trim=2).enqueue() == BAD  # 2 k >= M
    assert fresh(dict(NODP, cdp_clip=0.5)).enqueue() == BAD
    assert fresh(dict(NODP, cdp_clip=0.5, cdp_sigma=1.0)).enqueue() == BAD
    assert fresh(client_weight=torch.tensor([0.2, 0.3, 0.5], device="cuda")).enqueue() == BAD
    for field in ("cdp_scale", "cdp_norm", "cdp_round"):  # the existing null checks of the close's buffers
        c = fresh()
        setattr(c.round, field, None)
        assert c.enqueue() == BAD, field
    g = C.c_void_p()
    c = fresh(trim=2)
    assert lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)) == BAD and not g.value
    torch.cuda.synchronize()
    assert torch.equal(c.glob, glob) and int(c.word.item()) == R0  # nothing was launched
    # the stand-alone entry
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    ps = lib.ecg_tiny_cohort_param_stride(2)
    big = torch.zeros((65, ps), device="cuda")
    sc = torch.zeros(P, device="cuda")
    m = torch.zeros(P, device="cuda")
    for M_, k_, kw in ((3, 0, {}), (3, -1, {}), (3, 2, {}), (4, 2, {}), (65, 1, {}), (3, 1, dict(scratch=None)),
                       (3, 1, dict(opt=3, m=m)), (3, 1, dict(opt=5, m=m, v=m.clone())), (0, 1, {})):
        kw = dict(dict(scratch=sc), **kw)
        assert robust_close(big, glob.clone(), 2, M_, k_, 1.0, word, **kw)[0] == BAD, (M_, k_)
    assert robust_close(big, glob.clone(), 2, 3, 1, 1.0, None, scratch=sc)[0] == BAD  # no round word
    assert int(word.item()) == 0
    for M_, k_ in ((3, 1), (4, 1), (64, 1), (64, 31)):  # the valid neighbours
        assert robust_close(big, glob.clone(), 2, M_, k_, 1.0, word, scratch=sc)[0] == 0, (M_, k_)
    assert robust_close(big, glob.clone(), 2, 3, 1, 1.0, word, delta=sc, scratch=None)[0] == 0
    assert int(word.item()) == 5


# 6 ---------------------------------------------------------------------------------------------------------------
def _assert_same(a, b, names=NAMES):
    for n in names:
        u, v = getattr(a, n), getattr(b, n)
        assert (u is None) == (v is None), n
        if u is not None:
            assert torch.equal(u, v), n


def _graph_run(c, launches=1):
    lib_ = _lib()
    lib = lib_.kernels()
    g = C.c_void_p()
    lib_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)), "ecg_tiny_cohort_round_capture")
    try:
        for _ in range(launches):
            lib_.check(lib.ecg_round_graph_launch(g, lib_.stream_ptr(c.glob.device)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    return c


def _close_on(clients, glob, nc, M, k):
    """``ecg_cohort_robust_close`` (the plain step, eta = 1) on a round's client weights and its starting weights."""
    g = glob.clone()
    word = torch.zeros(1, dtype=torch.int64, device="cuda")
    st, _, _ = robust_close(clients, g, nc, M, k, 1.0, word, scratch=torch.zeros(num_params(nc), device="cuda"))
    assert st == 0
    return g


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("nc,M,k", [(2, 3, 1), (5, 8, 2)])
def test_rounds_enqueue_graph_and_the_stand_alone_close_agree_bitwise(nc, M, k, precision):
    dev, x, y32 = _data(L_, nc)
    glob, table, P = _global(nc), _table(S_, M * B_, seed=4), num_params(nc)

    def fresh():
        return Cohort(x, y32, nc, M, B_, S_, precision, table, glob, NODP, robust_trim=k,
                      robust_scratch=torch.zeros(P, device="cuda"))

    a = fresh().run()
    one = a.glob.clone()
    # a mean-close round from the same start leaves the same client weights; the robust close on them is the round's
    mean = Cohort(x, y32, nc, M, B_, S_, precision, table, glob).run()
    assert torch.equal(mean.cparams, a.cparams)
    assert torch.equal(_close_on(mean.cparams, glob, nc, M, k), one)
    assert not torch.equal(one, mean.glob) and not torch.equal(one, glob)  # the trim acts
    a.run()  # the second round starts from the first one's result
    assert not torch.equal(a.glob, one) and int(a.word.item()) == R0 + 2
    b = _graph_run(fresh(), 2)
    _assert_same(a, b)
    assert torch.equal(a.keep[0], b.keep[0])  # the scratch holds the last Delta


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_fields_zero_is_the_round_without_them_and_client_steps_compose(precision):
    nc, M = 2, 3
    dev, x, y32 = _data(L_, nc)
    glob, table, P = _global(nc), _table(S_, M * B_, seed=5), num_params(nc)
    for dp in (None, dict(NODP, server_lr=0.8)):
        a = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, dp).run()
        b = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, dp, robust_trim=0, robust_scratch=None).run()
        c = _graph_run(Cohort(x, y32, nc, M, B_, S_, precision, table, glob, dp, robust_trim=0, robust_scratch=None))
        _assert_same(a, b)
        _assert_same(a, c)
        assert not torch.equal(a.glob, glob)
    steps = torch.tensor([S_, 1, S_], dtype=torch.int32, device="cuda")
    r = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, NODP, client_steps=steps, robust_trim=1,
               robust_scratch=torch.zeros(P, device="cuda")).run()
    mean = Cohort(x, y32, nc, M, B_, S_, precision, table, glob, client_steps=steps.clone()).run()
    full = Cohort(x, y32, nc, M, B_, S_, precision, table, glob).run()
    assert torch.equal(mean.cparams, r.cparams) and not torch.equal(full.cparams[1], r.cparams[1])
    assert torch.equal(_close_on(mean.cparams, glob, nc, M, 1), r.glob) and not torch.equal(r.glob, glob)


# 7 ---------------------------------------------------------------------------------------------------------------
CASES = {"trimmed": dict(robust="trimmed", trim_frac=0.25, cohort=4),
         "median": dict(robust="median", cohort=5),
         "median-adam": dict(robust="median", cohort=4, server_opt="adam", server_lr=0.01),
         "trimmed-global": dict(robust="trimmed", trim_frac=0.34, cohort=3, server_scope="global")}


def _pair(case, **more):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    dev, x, y32 = _data(L_, 2)
    kw = dict(clients=6, lr=LR, momentum=MU, weight_decay=WD, seed=7, **CASES[case])
    kw.update(more)
    torch.manual_seed(3)
    tr = FusedCohortTrainer(TinyECG().to(dev), x, y32.long(), B_, S_, precision="fp32", **kw)
    torch.manual_seed(3)
    ref_model = TinyECG().to(dev)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), B_, S_, amp_dtype=None, **kw)
    return tr, ref, ref_model, y32


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_trainer_against_the_torch_cohort_reference(case):
    """Two fp32 rounds, FusedCohortTrainer (graph replays) vs TorchCohortTrainer: relative l2 difference of the global
    weights at most 1e-5, the siblings' bound (a trimmed mean is continuous in its inputs).
    Measured (MI355X): see the README's item on robust aggregation."""
    tr, ref, ref_model, _ = _pair(case)
    P = tr.P
    assert tr.trim == ref.trim == 1 + (case == "median") and not tr.hetero and tr._round.client_steps is None
    assert tr._round.robust_trim == tr.trim and tr._round.client_weight is None
    start = tr.params[:P].clone()
    tr.prepare([S_])
    assert torch.equal(tr.params[:P], start)
    for _ in range(2):
        tr.run_round()
        ref.run_round(S_)
        assert tr.round_clients == ref.round_clients
    torch.cuda.synchronize()
    norms, clipped = tr.last_clip_stats()
    assert len(norms) == tr.M and min(norms) > 0 and clipped == 0.0
    assert np.allclose(norms, ref.last_clip_stats()[0], rtol=1e-4)
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    moved = (want - start).norm().item() / want.norm().item()
    print(f"fp32 cohort rounds, {case}, fused vs torch: relative l2 difference {rel:.3e} (update {moved:.3e}; "
          f"avg loss {tr.avg_loss():.6f} vs {ref.avg_loss():.6f})")
    assert rel <= 1e-5, rel
    assert moved > 1e-4
    tr.close()


def test_resume_continues_bitwise_and_flipped_labels_agree():
    whole, _, _, y32 = _pair("median-adam", flip_clients=2)
    P = whole.P
    whole.prepare([S_])
    whole.run_round()
    whole.run_round()
    torch.cuda.synchronize()
    first, ref, _, _ = _pair("median-adam", flip_clients=2)
    first.prepare([S_])
    first.run_round()
    torch.cuda.synchronize()
    ckpt = (first.params[:P].clone(), first.server_state(), first.cohort_round)
    rest, _, _, _ = _pair("median-adam", flip_clients=2)
    rest.params[:P].copy_(ckpt[0])
    rest.load_server_state(ckpt[1])
    rest.set_cohort_round(ckpt[2])
    rest.prepare([S_])
    rest.run_round()
    torch.cuda.synchronize()
    assert rest.cohort_round == 2 and torch.equal(rest.params[:P], whole.params[:P])
    for key, t in whole.server_state().items():
        assert torch.equal(rest.server_state()[key], t), key
    # both trainers train on the same labels: clients 0 and 1 (rows [0, 2 n)) mirrored, the rest as given
    n = y32.shape[0] // 6
    assert torch.equal(whole.y32, ref.y.to(torch.int32))
    assert torch.equal(whole.y32[: 2 * n], 1 - y32[: 2 * n]) and torch.equal(whole.y32[2 * n:], y32[2 * n:])
    plain, _, _, _ = _pair("median-adam")
    assert torch.equal(plain.y32, y32)
    for t in (whole, first, rest, plain):
        t.close()
