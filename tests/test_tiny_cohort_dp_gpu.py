"""Record-level DP-SGD inside the fused cohort round on the GPU: the cohort clip factors (un-scaling B, not M * B), the
clipped per-client sums and loss words, the bitwise equalities with the plain cohort reduce, the single-client DP
reduce and the round without the fields, the per-client Philox streams (2 + c), DP rounds (graph == enqueue, the step
word with a frozen client, prepare), the fused fp32 trainer against ``TorchCohortTrainer``, and the argument checks.

Shapes: B = 37 runs only the reduce's tail row loop, B = 273 one unrolled 256-row chunk plus a tail; nc = 2 / 5 give
P + 1 = 1459 / 1510 columns, both ragged against the 32 columns of a reduce block and the 256 columns of a clip-factor
pass; M = 3 clients (M = 1: the single-client equality); L = 64 (16-byte gather rows) and L = 61 (scalar gather rows);
rounds of S <= 3 steps."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import crossscale_ecg  # noqa: F401
from crossscale_ecg.models.tiny_ecg import TinyECG, num_params
from crossscale_ecg.utils import philox

from cohort_harness import LR, MU, WD, Cohort, _data, _global, _lib, _table

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SHAPES = [(37, 2), (273, 5)]
M_ = 3
BAD = 1  # kBadArg
BIG = 1e30  # a clip norm no row reaches: every factor is 1


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


def _word(t=0):
    return torch.full((1,), t, dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(B, nc, M=M_):
    """One cohort step's slab (read-only, shared): client c's B rows are per-sample gradients at weights of its own,
    pre-scaled by 1 / B.  The clip norm as tests/test_tiny_dp_gpu.py::_case chooses it - the middle of a relative gap of
    at least 1e-3 between two neighbouring float64 row norms, searched outward from the median - per client, then the
    first candidate that leaves every client both clipped and unclipped rows and stays 2e-4 (twice the device's
    relative error bound) away from every norm of the cohort."""
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B + nc)
    x = torch.randn(1024, 64, generator=g).to(dev)
    y32 = torch.randint(0, nc, (1024,), generator=g).to(torch.int32).to(dev)
    P = num_params(nc)
    slabs = []
    for c in range(M):
        torch.manual_seed(10 + c)
        w = torch.cat([p.detach().reshape(-1) for p in TinyECG(num_classes=nc).parameters()]).to(dev)
        idx = torch.randperm(1024, generator=g)[:B].to(torch.int32).to(dev)
        slabs.append(tiny_step_grads(w, x, y32, idx, B, nc))
    slab = torch.cat(slabs).contiguous()
    torch.cuda.synchronize()
    n64 = (B * slab[:, :P].double().norm(dim=1)).view(M, B)
    cands = []
    for c in range(M):
        s = n64[c].sort().values
        for k in sorted(range(1, B), key=lambda k: abs(k - B // 2)):
            if (s[k] - s[k - 1]) / s[k] >= 1e-3:
                cands.append(float((s[k - 1] * s[k]).sqrt()))
    ok = [cl for cl in cands
          if all(0 < int((n64[c] > cl).sum()) < B for c in range(M)) and float((n64 / cl - 1).abs().min()) >= 2e-4]
    assert ok, "no clip norm with clipped and unclipped rows in every client"
    clip = ok[0]
    c64 = torch.clamp(clip / n64, max=1.0).view(-1)
    return dict(dev=dev, slab=slab, P=P, n64=n64.view(-1), clip=clip, c64=c64, B=B, M=M, nc=nc)


def _reduce(cs, *, dp=None, steps=None, step=0, lr=1.0, momentum=0.0, wd=0.0, nesterov=0, rand=False, image=False,
            M=None, word=0):
    """One cohort reduce + SGD on the case's slab, on fresh buffers (zeros, or ``rand`` weights and momenta).
    ``dp`` (clip, sigma): ecg_slab_reduce_cohort_dp_sgd; None: the plain STEPS kernel (with ``steps`` None every client
    active, which leaves the plain cohort kernel's bits)."""
    L_ = _lib()
    lib = L_.kernels()
    M = cs["M"] if M is None else M
    B, P, nc, dev, slab = cs["B"], cs["P"], cs["nc"], cs["dev"], cs["slab"]
    ps, ws = lib.ecg_tiny_cohort_param_stride(nc), lib.ecg_tiny_cohort_wprep_stride()
    params, mom = torch.zeros(M, ps, device=dev), torch.zeros(M, ps, device=dev)
    if rand:
        g = torch.Generator().manual_seed(9)
        params[:, :P] = torch.randn(M, P, generator=g).to(dev)
        mom[:, :P] = torch.randn(M, P, generator=g).to(dev)
    loss = torch.zeros(M, device=dev)
    wprep = torch.zeros(M * ws, dtype=torch.uint8, device=dev) if image else None
    scale = torch.full((M * B + 8,), -7.5, device=dev)  # 8 canaries behind the factors
    w = _word(word)
    head = (slab.data_ptr(), B, M, slab.stride(0), P, params.data_ptr(), mom.data_ptr(), loss.data_ptr(), lr, momentum,
            wd, nesterov, L_.ptr(wprep), None, 0.0)
    if dp is not None:
        cst = None if steps is None else _i32(steps)
        st = lib.ecg_slab_reduce_cohort_dp_sgd(*head, L_.ptr(cst), step, dp[0], dp[1], SEED, scale.data_ptr(),
                                               w.data_ptr(), L_.stream_ptr(dev))
    else:
        cst = _i32([1 << 20] * M if steps is None else steps)
        st = lib.ecg_slab_reduce_cohort_steps_sgd(*head, cst.data_ptr(), step, L_.stream_ptr(dev))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(scale[M * B:], torch.full((8,), -7.5, device=dev))
    return dict(params=params, mom=mom, loss=loss, wprep=wprep, scale=scale[:M * B], word=int(w.item()))


def _same(a, b, names=("params", "mom", "loss", "wprep")):
    for n in names:
        assert (a[n] is None) == (b[n] is None), n
        if a[n] is not None:
            assert torch.equal(a[n], b[n]), n


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nc", SHAPES)
def test_clip_factors_of_three_clients_match_float64_with_unscaling_B(B, nc):
    cs = _case(B, nc)
    n64, c64, clip = cs["n64"], cs["c64"], cs["clip"]
    for c in range(M_):  # the condition the clip norm was chosen for, on the float64 reference
        assert 0 < int((c64[c * B:(c + 1) * B] < 1).sum()) < B, c
    flip = (n64 < clip) & (M_ * n64 > clip * (1 + 1e-3))  # unclipped, but clipped had the row count M * B un-scaled
    assert int(flip.sum()) >= 1
    out = _reduce(cs, dp=(clip, 0.0), word=41)
    scale = out["scale"]
    rel = ((scale.double() - c64).abs() / c64).max().item()
    print(f"cohort clip factors B={B} nc={nc}: worst relative error {rel:.3e}, {int((scale < 1).sum())}/{M_ * B} rows "
          f"clipped, {int(flip.sum())} rows the un-scaling M * B would have flipped")
    assert rel <= 1e-4  # worst-case fp32 accumulation over 1,458 squares: 1458 * 2^-24 = 8.7e-5
    assert torch.equal(scale < 1, c64 < 1)
    assert bool((scale[flip] == 1).all())
    assert out["word"] == 42  # one cohort step, one advance
    z = cs["slab"].clone()  # a sample with a zero gradient is not scaled, whatever the clip norm
    z[B + 3, :cs["P"]] = 0
    out0 = _reduce(dict(cs, slab=z), dp=(0.5 * float(n64.min()), 0.0))
    assert out0["scale"][B + 3].item() == 1.0 and int((out0["scale"] < 1).sum()) == M_ * B - 1


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nc", SHAPES)
def test_clipped_sums_per_client_match_float64_and_loss_words_are_untouched(B, nc):
    """lr = 1 on zero weights without momentum or weight decay: client c ends on minus its clipped sum."""
    cs = _case(B, nc)
    P = cs["P"]
    out = _reduce(cs, dp=(cs["clip"], 0.0))
    plain = _reduce(cs)
    terms = (cs["c64"][:, None] * cs["slab"][:, :P].double()).view(M_, B, P)
    err = (-out["params"][:, :P].double() - terms.sum(1)).abs()
    bound = 1e-4 * terms.abs().sum(1)
    print(f"cohort clipped sums B={B} nc={nc}: worst error / bound {(err / bound.clamp_min(1e-300)).max().item():.3e}")
    assert (err <= bound).all()
    assert torch.equal(out["loss"], plain["loss"]) and float(out["loss"].min()) > 0  # the unclipped column sums
    col = cs["slab"][:, P].double().view(M_, B).sum(1)
    assert ((out["loss"].double() - col).abs() <= 1e-4 * col).all()
    assert not torch.equal(out["params"], plain["params"])  # the clip acts


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [None, (3, 1, 2)])
@pytest.mark.parametrize("B,nc,nesterov,wd", [(37, 2, 0, 0.0), (273, 5, 1, 1e-3)])
def test_no_clip_no_noise_is_bitwise_the_plain_cohort_reduce(B, nc, nesterov, wd, steps):
    cs = _case(B, nc)
    kw = dict(steps=steps, step=1, lr=0.05, momentum=0.9, wd=wd, nesterov=nesterov, rand=True, image=True)
    plain, dp = _reduce(cs, **kw), _reduce(cs, dp=(BIG, 0.0), **kw)
    _same(plain, dp)
    assert bool((dp["scale"] == 1).all()) and plain["wprep"].any() and dp["word"] == 1
    if steps:  # client 1 is frozen at step 1: not written
        untouched = _reduce(cs, dp=(BIG, 0.0), **dict(kw, lr=0.0, momentum=0.0, wd=0.0))
        assert float(dp["loss"][1]) == 0 and torch.equal(dp["params"][1], untouched["params"][1])
        assert float(dp["loss"][0]) > 0


@pytest.mark.parametrize("precision,L,nc,B,S", [("bf16", 64, 5, 273, 2), ("fp32", 61, 2, 37, 3), ("bf16", 61, 2, 37, 3)])
def test_rounds_without_clip_and_noise_and_without_the_fields_are_the_existing_round_bitwise(precision, L, nc, B, S):
    dev, x, y32 = _data(L, nc)
    glob, table = _global(nc), _table(S, M_ * B)
    names = ("glob", "cparams", "cmom", "loss", "wprep")

    def dpf(clip):
        return dict(dp_clip=clip, dp_sigma=0.0, dp_seed=SEED, dp_scale=torch.zeros(M_ * B, device=dev), dp_step=_word(5))

    for st in (None, (S, 1, 2)):
        cst = {} if st is None else dict(client_steps=_i32(st))
        a = Cohort(x, y32, nc, M_, B, S, precision, table, glob, **cst).run()
        b = Cohort(x, y32, nc, M_, B, S, precision, table, glob, **cst, **dpf(BIG)).run()
        for n in names:
            u, v = getattr(a, n), getattr(b, n)
            assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), (n, st)
        assert int(b.keep[-1].item()) == 5 + S and not torch.equal(a.glob, glob)
    # every new field named as zero / null: the round of before
    c = Cohort(x, y32, nc, M_, B, S, precision, table, glob, dp_clip=0.0, dp_sigma=0.0, dp_seed=0, dp_scale=None,
               dp_step=None).run()
    a = Cohort(x, y32, nc, M_, B, S, precision, table, glob).run()
    for n in names:
        u, v = getattr(a, n), getattr(c, n)
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), n


@pytest.mark.parametrize("B,nc", SHAPES)
def test_a_cohort_of_one_without_noise_is_bitwise_the_single_client_dp_reduce(B, nc):
    from crossscale_ecg.ops.fused_tiny import new_wprep
    L_ = _lib()
    lib = L_.kernels()
    cs = _case(B, nc)
    P, dev, slab = cs["P"], cs["dev"], cs["slab"]
    co = _reduce(cs, dp=(cs["clip"], 0.0), lr=0.05, momentum=0.9, wd=1e-3, rand=True, image=True, M=1)
    g = torch.Generator().manual_seed(9)
    params, mom = torch.randn(1, P, generator=g).to(dev)[0].contiguous(), torch.randn(1, P, generator=g).to(dev)[0].contiguous()
    loss, wprep, scale, w = torch.zeros(1, device=dev), new_wprep(dev), torch.zeros(B, device=dev), _word()
    st = lib.ecg_slab_reduce_dp_sgd(slab.data_ptr(), B, slab.stride(0), P, params.data_ptr(), mom.data_ptr(), None,
                                    loss.data_ptr(), 0.05, 0.9, 1e-3, 0, 1, wprep.data_ptr(), cs["clip"], 0.0, SEED,
                                    scale.data_ptr(), w.data_ptr(), L_.stream_ptr(dev))
    assert st == 0
    torch.cuda.synchronize()
    assert torch.equal(co["params"][0, :P], params) and torch.equal(co["mom"][0, :P], mom)
    assert torch.equal(co["loss"], loss) and torch.equal(co["scale"], scale) and 0 < int((scale < 1).sum()) < B
    assert torch.equal(co["wprep"][:wprep.numel()], wprep) and wprep.any()


# 4 ---------------------------------------------------------------------------------------------------------------
def _noise(P, seed, t, stream):
    L_ = _lib()
    z = torch.empty(P, device="cuda")
    assert L_.kernels().ecg_dp_noise_stream(z.data_ptr(), P, seed, t, stream, L_.stream_ptr(z.device)) == 0
    torch.cuda.synchronize()
    return z


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
def test_noise_of_client_streams_matches_numpy_philox(seed):
    from crossscale_ecg.ops.fused_tiny import dp_noise
    for c in (0, 1, 65534):
        for t in (0, 2 ** 32 + 5):
            for P in (1458, 1509):
                z = _noise(P, seed, t, 2 + c).double().cpu().numpy()
                err = np.abs(z - philox.normal(seed, t, P, stream=2 + c)).max()
                print(f"noise seed={seed:#x} t={t} P={P} stream={2 + c}: max |z - ref| = {err:.3e}")
                assert err <= 1e-5 and np.abs(z).max() <= 5.77
    # stream 0 is the single client's draw, bit for bit, and the client-level close's stream 1 is another vector
    z0 = _noise(1458, seed, 7, 0)
    assert torch.equal(z0, dp_noise(1458, seed, 7, z0.device))
    assert not torch.equal(z0, _noise(1458, seed, 7, 1)) and not torch.equal(z0, _noise(1458, seed, 7, 2))


@pytest.mark.parametrize("B,nc", SHAPES)
def test_noised_reduce_adds_each_clients_scaled_z_of_the_current_word(B, nc):
    cs = _case(B, nc)
    P, dev = cs["P"], cs["dev"]
    sigma, clip, t = 1.3, cs["clip"], 7
    g0 = -_reduce(cs, dp=(clip, 0.0), word=t)["params"][:, :P]
    out = _reduce(cs, dp=(clip, sigma), word=t)
    g1 = -out["params"][:, :P]
    nscale = sigma * clip / B
    _, e = torch.frexp(g1.abs())  # |g1| = m * 2^e with m in [0.5, 1): one ulp is 2^(e - 24)
    ulp = torch.ldexp(torch.ones_like(g1), e - 24).double()
    diff = g1.double() - g0.double()
    for c in range(M_):
        want = nscale * torch.from_numpy(philox.normal(SEED, t, P, stream=2 + c)).to(dev)
        err = (diff[c] - want).abs()
        print(f"noised cohort update B={B} nc={nc} client {c}: worst error / (1e-5 nscale + ulp) "
              f"{(err / (1e-5 * nscale + ulp[c])).max().item():.3e}")
        assert (err <= 1e-5 * nscale + ulp[c]).all()
        other = nscale * torch.from_numpy(philox.normal(SEED, t + 1, P, stream=2 + c)).to(dev)
        assert (diff[c] - other).abs().max() > 0.1 * nscale  # not the next step's draw
    assert out["word"] == t + 1
    for a in range(M_):  # independent draws: the clients' noise vectors differ pairwise, far beyond rounding
        for b in range(a + 1, M_):
            assert (diff[a] - diff[b]).abs().max() > 0.1 * nscale
    # a frozen client draws nothing and is not written, and the word still advances
    fr = _reduce(cs, dp=(clip, sigma), steps=(2, 1, 2), step=1, word=t)
    assert fr["word"] == t + 1 and not fr["params"][1].any() and torch.equal(fr["params"][0], out["params"][0])


# 5 ---------------------------------------------------------------------------------------------------------------
def _median_norm(glob, x, y32, table, B, nc, precision):
    from crossscale_ecg.ops.fused_tiny import tiny_step_grads
    slab = tiny_step_grads(glob, x, y32, table[0, :B].contiguous(), B, nc, precision=precision)
    return float((B * slab[:, :num_params(nc)].double().norm(dim=1)).median())


def _dp_cohort(x, y32, nc, B, S, precision, table, glob, clip, sigma=1.1, word=3, **kw):
    dev = x.device
    return Cohort(x, y32, nc, M_, B, S, precision, table, glob, dp_clip=clip, dp_sigma=sigma, dp_seed=SEED,
                  dp_scale=torch.zeros(M_ * B, device=dev), dp_step=_word(word), **kw)


def _graph_run(c, launches=1):
    L_ = _lib()
    lib = L_.kernels()
    g = C.c_void_p()
    L_.check(lib.ecg_tiny_cohort_round_capture(C.byref(g), C.byref(c.round)), "ecg_tiny_cohort_round_capture")
    try:
        for _ in range(launches):
            L_.check(lib.ecg_round_graph_launch(g, L_.stream_ptr(c.glob.device)), "ecg_round_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.ecg_round_graph_destroy(g)
    return c


ROUND_NAMES = ("glob", "cparams", "cmom", "loss", "wprep")


def _assert_rounds_equal(a, b):
    for n in ROUND_NAMES:
        u, v = getattr(a, n), getattr(b, n)
        assert (u is None) == (v is None) and (u is None or torch.equal(u, v)), n
    for u, v in zip(a.keep, b.keep):  # client_steps, the clip factors of the last step, the step word
        assert torch.equal(u, v)


@pytest.mark.parametrize("precision,L,nc,B", [("bf16", 64, 5, 273), ("bf16", 61, 2, 37), ("fp32", 61, 2, 37)])
def test_dp_round_graph_equals_enqueue_and_a_second_replay_continues_the_word(precision, L, nc, B):
    S = 3
    dev, x, y32 = _data(L, nc)
    glob, table = _global(nc), _table(S, M_ * B)
    clip = _median_norm(glob, x, y32, table, B, nc, precision)

    def fresh():
        return _dp_cohort(x, y32, nc, B, S, precision, table, glob, clip)

    e1, g1 = fresh().run(), _graph_run(fresh())
    _assert_rounds_equal(e1, g1)
    scale, word = g1.keep
    assert int(word.item()) == 3 + S and 0 < int((scale < 1).sum()) < M_ * B
    e2, g2 = fresh().run().run(), _graph_run(fresh(), 2)
    _assert_rounds_equal(e2, g2)
    assert int(g2.keep[1].item()) == 3 + 2 * S and not torch.equal(g1.glob, g2.glob)
    # the noise acts, and it is the word's: the same round from another word ends elsewhere
    other = _dp_cohort(x, y32, nc, B, S, precision, table, glob, clip, word=4).run()
    quiet = _dp_cohort(x, y32, nc, B, S, precision, table, glob, clip, sigma=0.0).run()
    assert not torch.equal(other.glob, e1.glob) and not torch.equal(quiet.glob, e1.glob)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_frozen_client_leaves_the_word_advancing_and_ends_on_its_own_step_count(precision):
    L, nc, B, S = 61, 2, 37, 3
    dev, x, y32 = _data(L, nc)
    glob, table = _global(nc), _table(S, M_ * B, seed=4)
    clip = _median_norm(glob, x, y32, table, B, nc, precision)
    steps = (3, 1, 2)
    a = _graph_run(_dp_cohort(x, y32, nc, B, S, precision, table, glob, clip, client_steps=_i32(steps)))
    assert int(a.keep[1].item()) == 3 + S  # (keep: dp_scale, dp_step, client_steps)
    for s in (1, 2):
        ref = _dp_cohort(x, y32, nc, B, s, precision, table, glob, clip).run()
        c = steps.index(s)
        assert torch.equal(a.cparams[c], ref.cparams[c]) and torch.equal(a.cmom[c], ref.cmom[c])
        assert torch.equal(a.loss[c], ref.loss[c]) and float(ref.loss[c]) > 0
        if precision == "bf16":
            assert torch.equal(a.image(c), ref.image(c))
    full = _dp_cohort(x, y32, nc, B, S, precision, table, glob, clip).run()
    assert torch.equal(a.cparams[0], full.cparams[0]) and not torch.equal(a.cparams[1], full.cparams[1])


def _trainer(x, y32, precision, B, clip, use_graph=True, **kw):
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    torch.manual_seed(3)
    model = TinyECG(num_classes=2).to(x.device)
    return FusedCohortTrainer(model, x, y32.long(), B, 3, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                              seed=7, use_graph=use_graph, precision=precision, dp_clip=clip, dp_noise=1.1,
                              dp_seed=SEED, **kw)


def _tdata(L, N=256):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, L, generator=g).cuda()
    return x, torch.randint(0, 2, (N,), generator=g).to(torch.int32).cuda()


def _tclip(x, y32, B, precision):
    torch.manual_seed(3)
    w = torch.cat([p.detach().reshape(-1) for p in TinyECG(num_classes=2).parameters()]).cuda()
    idx = torch.arange(M_ * B, dtype=torch.int32, device="cuda").view(1, -1)
    return _median_norm(w, x, y32, idx, B, 2, precision)


def test_prepared_trainer_equals_unprepared_twin_bitwise():
    x, y32 = _tdata(64)
    clip = _tclip(x, y32, 37, "bf16")
    outs = []
    for prepared in (False, True):
        tr = _trainer(x, y32, "bf16", 37, clip)
        assert tr.dp and tr._round.dp_clip > 0
        if prepared:
            tr.prepare([3])
            torch.cuda.synchronize()
            assert tr.dp_step.item() == 0 and tr.dp_steps == 0  # the warm-up replays were rolled back
        tr.run_round(reset_loss=False)
        tr.run_round(reset_loss=False)
        torch.cuda.synchronize()
        outs.append((tr.params.clone(), tr.avg_loss(), int(tr.dp_step.item()), tr.dp_steps, tr.dp_scale.clone()))
        tr.close()
    a, b = outs
    assert torch.equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] == a[3] == b[3] == 6
    assert 0 < int((a[4] < 1).sum()) < a[4].numel()
    # set_dp_steps moves the word: the second round from step 0 again ends elsewhere
    tr = _trainer(x, y32, "bf16", 37, clip)
    tr.run_round(reset_loss=False)
    tr.set_dp_steps(0)
    tr.run_round(reset_loss=False)
    torch.cuda.synchronize()
    assert tr.dp_step.item() == 3 and not torch.equal(tr.params, a[0])
    tr.close()


# 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("server_opt", ["none", "sgdm"])
def test_fused_fp32_cohort_dp_rounds_match_the_torch_cohort_trainer(server_opt):
    """Two fused fp32 rounds of M = 3 clients with clip and noise == ``TorchCohortTrainer`` (per-sample gradients from
    torch.func, noise from utils/philox.py at stream 2 + j) on the same tables.  Tolerance: the fused-fp32-vs-torch SGD
    trajectory bound of tests/test_fused_tiny_gpu.py (relative l2 error of the weights < 1e-5)."""
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    B = 37
    x, y32 = _tdata(61)
    clip = _tclip(x, y32, B, "fp32")
    kw = dict(server_opt=server_opt, server_lr=0.8) if server_opt != "none" else {}
    tr = _trainer(x, y32, "fp32", B, clip, **kw)
    torch.manual_seed(3)
    ref_model = TinyECG(num_classes=2).to(x.device)
    ref = TorchCohortTrainer(ref_model, x, y32.long(), B, 3, clients=4, cohort=M_, lr=LR, momentum=MU, weight_decay=WD,
                             amp_dtype=None, seed=7, dp_clip=clip, dp_noise=1.1, dp_seed=SEED, **kw)
    P = tr.P
    for _ in range(2):
        tr.run_round(reset_loss=False)
        ref.run_round(3, reset_loss=False)
        torch.cuda.synchronize()
        assert torch.equal(tr.idx_table, ref.table) and tr.round_clients == ref.round_clients
    want = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters()])
    rel = (tr.params[:P] - want).norm().item() / want.norm().item()
    print(f"fp32 cohort DP rounds ({server_opt}), fused vs torch: relative l2 difference {rel:.3e}, "
          f"avg loss {tr.avg_loss():.6f} vs {ref.avg_loss():.6f}")
    assert rel < 1e-5, rel
    assert abs(tr.avg_loss() - ref.avg_loss()) < 1e-4
    assert tr.dp_steps == ref.dp_steps == 6 and tr.dp_step.item() == 6
    assert 0 < int((tr.dp_scale < 1).sum()) < tr.dp_scale.numel()  # the last step clipped some rows and kept others
    tr.close()


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_check_cohort_round_rejects_bad_dp_arguments_and_touches_nothing(precision):
    L_ = _lib()
    lib = L_.kernels()
    L, nc, B, S = 64, 2, 37, 2
    dev, x, y32 = _data(L, nc)
    glob, table = _global(nc), _table(S, M_ * B)

    def fresh(prox_mu=None, **change):
        scale = torch.full((M_ * B + 8,), -7.5, device=dev)  # factors and 8 canaries
        f = dict(dp_clip=0.5, dp_sigma=1.0, dp_seed=SEED, dp_scale=scale, dp_step=_word(9))
        f.update(change)
        return Cohort(x, y32, nc, M_, B, S, precision, table, glob, prox_mu=prox_mu, **f)

    bad = [dict(dp_clip=-1.0), dict(dp_sigma=-0.5), dict(dp_clip=0.0, dp_sigma=1.0), dict(dp_scale=None),
           dict(dp_step=None), dict(prox_mu=0.05)]
    for change in bad:
        c = fresh(**change)
        before = c.state() + [c.slab.clone()]
        assert c.enqueue() == BAD, change
        handle = C.c_void_p()
        assert lib.ecg_tiny_cohort_round_capture(C.byref(handle), C.byref(c.round)) == BAD, change
        assert not handle.value
        torch.cuda.synchronize()
        for u, v in zip(before, c.state() + [c.slab]):
            assert torch.equal(u, v), change
    good = fresh().run()  # the description the changes were made to runs
    scale, word = good.keep
    assert int(word.item()) == 9 + S and torch.equal(scale[M_ * B:], torch.full((8,), -7.5, device=dev))
    assert bool((scale[:M_ * B] <= 1).all()) and not torch.equal(good.glob, glob)
    # the stand-alone pair checks the same, and has no proximal form
    cs = _case(37, 2)
    ps = lib.ecg_tiny_cohort_param_stride(2)
    params, sc, w = torch.zeros(M_, ps, device=dev), torch.full((M_ * 37,), -7.5, device=dev), _word()
    head = (cs["slab"].data_ptr(), 37, M_, cs["slab"].stride(0), cs["P"], params.data_ptr(), None, None, 1.0, 0.0, 0.0, 0,
            None)
    for anchor, mu, clip, sigma, s_, w_ in ((None, 0.0, 0.0, 0.0, sc, w), (None, 0.0, -1.0, 0.0, sc, w),
                                            (None, 0.0, 1.0, -1.0, sc, w), (None, 0.0, 1.0, 1.0, None, w),
                                            (None, 0.0, 1.0, 1.0, sc, None), (glob, 0.05, 1.0, 1.0, sc, w)):
        st = lib.ecg_slab_reduce_cohort_dp_sgd(*head, L_.ptr(anchor), mu, None, 0, clip, sigma, SEED, L_.ptr(s_),
                                               L_.ptr(w_), L_.stream_ptr(dev))
        assert st == BAD, (mu, clip, sigma)
    torch.cuda.synchronize()
    assert w.item() == 0 and not params.any() and bool((sc == -7.5).all())
    from crossscale_ecg.ops.fused_cohort import FusedCohortTrainer
    xt, yt = _tdata(64)
    for kw, match in ((dict(dp_clip=-1.0), ">= 0"), (dict(dp_noise=1.0), "needs a clip norm"),
                      (dict(dp_clip=1.0, dp_seed=SEED, prox_mu=0.1), "FedProx"),
                      (dict(dp_clip=1.0, dp_noise=1.0), "needs dp_seed")):
        with pytest.raises(ValueError, match=match):
            FusedCohortTrainer(TinyECG().to(dev), xt, yt.long(), 8, 2, clients=4, **kw)
