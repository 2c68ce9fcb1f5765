"""Server optimizers on cohort rounds (FedAvgM, FedAdagrad, FedAdam, FedYogi), on the CPU: ``server_opt_step`` against
the definition in float64 numpy, ``TorchCohortTrainer(server_opt=...)``, two gloo ranks with sgdm against global
FedAvgM, the checkpoint round trip of the optimizer state, and the driver's rejections.

The definition (train/server_opt.py), Delta the averaged client delta of a round, no bias correction:
  sgdm     m = b1 m + Delta,            g += eta m
  adagrad  m = b1 m + (1 - b1) Delta,   v = v + Delta^2
  adam     m as adagrad,                v = b2 v + (1 - b2) Delta^2
  yogi     m as adagrad,                v = v - (1 - b2) Delta^2 sign(v - Delta^2)
  adagrad, adam, yogi:                  g += eta m / (sqrt(v) + tau)"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv

P = 1458  # TinyECG, 2 classes
EPS32 = 2.0 ** -23
OPTS = ("sgdm", "adagrad", "adam", "yogi")


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _f(x):
    return float(np.float32(x))


def definition64(opt, g, d, m, v, eta, b1, b2, tau):
    """(g_new, m_new, v_new) of the definition in float64 numpy; the constants are the fp32 values."""
    eta, b1, b2, tau = _f(eta), _f(b1), _f(b2), _f(tau)
    if opt == "sgdm":
        m = b1 * m + d
        return g + eta * m, m, v
    m = b1 * m + (1.0 - b1) * d
    d2 = d * d
    if opt == "adagrad":
        v = v + d2
    elif opt == "adam":
        v = b2 * v + (1.0 - b2) * d2
    else:
        v = v - (1.0 - b2) * d2 * np.sign(v - d2)
    return g + eta * m / (np.sqrt(v) + tau), m, v


# ------------------------------------------------------------------------------------------------ 1: the step rule
@pytest.mark.parametrize("opt", OPTS)
def test_server_opt_step_against_the_definition_in_float64(opt):
    """Three consecutive steps; every step is compared with the float64 definition evaluated on the fp32 state going
    in.  Bounds, with u = 2^-24 per correctly rounded fp32 operation (torch on the CPU: no fused multiply-add; EPS32 =
    2u): m takes 4 operations (1 - b1, two products, a sum): |dm| <= 2 EPS32 (|b1 m| + |(1 - b1) Delta|); v takes at
    most 5 (Delta^2, 1 - b2, two products, a sum): |dv| <= 2.5 EPS32 (|v| + Delta^2); the step s = eta m / (sqrt(v) +
    tau) takes 4 more (product, sqrt, sum, quotient) and inherits dm / m and, through the square root, dv / (2 v):
    |ds| <= |s| (2 EPS32 + dv / (2 v)) + eta dm / (sqrt(v) + tau); the sum g + s adds u |g_new|.  Every bound below is
    taken with one more EPS32 than counted."""
    from crossscale_ecg.train.server_opt import server_opt_step
    eta, b1, b2, tau = 0.3, 0.9, 0.99, 1e-3
    rng = np.random.default_rng(7)
    g = torch.from_numpy(rng.standard_normal(P)).float()
    m = torch.zeros(P)
    v = None
    worst = 0.0
    for step in range(3):
        d = torch.from_numpy(rng.standard_normal(P) * 0.02).float()
        if opt == "yogi" and step == 0:  # both signs of v - Delta^2, no near-ties: v = 4 Delta^2 | Delta^2 / 4
            d2 = (d * d).double().numpy()
            v = torch.from_numpy(np.where(np.arange(P) % 2 == 0, 4.0 * d2, d2 / 4.0)).float()
        elif opt != "sgdm" and step == 0:
            v = torch.full((P,), tau * tau)
        g64, d64, m64 = g.double().numpy(), d.double().numpy(), m.double().numpy()
        v64 = None if v is None else v.double().numpy()
        if opt == "yogi":
            s = np.sign(v64 - d64 * d64)
            margin = np.abs(v64 - d64 * d64) / np.maximum(v64, d64 * d64)
            assert margin.min() > 1e-4, margin.min()  # no near-tie: the fp32 sign is the float64 sign
            assert (s > 0).any() and (s < 0).any()
        wg, wm, wv = definition64(opt, g64, d64, m64, v64, eta, b1, b2, tau)
        g2, m2, v2 = server_opt_step(opt, g, d, m, v, eta, b1, b2, tau)
        assert g2.dtype == m2.dtype == torch.float32 and g2 is not g and m2 is not m  # inputs are not written
        e = _f(eta)
        if opt == "sgdm":
            bm = 2 * EPS32 * (np.abs(_f(b1) * m64) + np.abs(d64))
            bg = e * bm + 2 * EPS32 * (np.abs(g64) + np.abs(e * wm))
            assert v2 is None
        else:
            bm = 3 * EPS32 * (np.abs(_f(b1) * m64) + np.abs((1 - _f(b1)) * d64))
            bv = 3.5 * EPS32 * (np.abs(v64) + d64 * d64)
            den = np.sqrt(wv) + _f(tau)
            st = e * wm / den
            bg = np.abs(st) * (3 * EPS32 + bv / (2 * wv)) + e * bm / den + EPS32 * (np.abs(g64) + np.abs(st))
            ev = np.abs(v2.double().numpy() - wv)
            assert np.all(ev <= bv), float((ev / bv).max())
            worst = max(worst, float((ev / bv).max()))
        em, eg = np.abs(m2.double().numpy() - wm), np.abs(g2.double().numpy() - wg)
        assert np.all(em <= bm), float((em / np.maximum(bm, 1e-300)).max())
        assert np.all(eg <= bg), float((eg / bg).max())
        worst = max(worst, float((eg / bg).max()))
        assert np.abs(wg - g64).max() > 1e-4  # the step moved the weights
        g, m, v = g2, m2, v2
    print(f"{opt}: worst error / bound over three steps {worst:.3f}")


def test_names_ids_and_checks():
    from crossscale_ecg.train import server_opt as so
    assert so.SERVER_OPTS == ("none", "sgdm", "adagrad", "adam", "yogi")
    assert [so.SERVER_OPT_IDS[n] for n in so.SERVER_OPTS] == [0, 1, 2, 3, 4]  # EcgTinyCohortRound's server_opt
    assert (so.BETA1, so.BETA2, so.TAU) == (0.9, 0.99, 1e-3)
    assert so.check_server_opt("adam") == 3 and so.check_server_opt("none", 5.0, -1.0, 0.0) == 0  # off: nothing read
    with pytest.raises(ValueError, match="unknown server optimizer"):
        so.check_server_opt("lamb")
    for kw in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=-0.5)):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            so.check_server_opt("sgdm", **kw)
    with pytest.raises(ValueError, match="server_tau"):
        so.check_server_opt("yogi", tau=0.0)
    so.check_server_opt("sgdm", tau=0.0)  # sgdm has no tau
    m, v = so.server_opt_init("adam", 5, 1e-3, "cpu")
    assert torch.equal(m, torch.zeros(5)) and torch.equal(v, torch.full((5,), 1e-3) ** 2)
    assert so.server_opt_init("sgdm", 5, 1e-3, "cpu")[1] is None and so.server_opt_init("none", 5, 1e-3, "cpu") == (None, None)


# ------------------------------------------------------------------------------------------------ 2: the trainer
B, S, K, M, L, N = 5, 3, 4, 3, 64, 48


def _data():
    g = torch.Generator().manual_seed(3)
    return torch.randn(N, L, generator=g), torch.randint(0, 2, (N,), generator=g)


def _trainer(**kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    return TorchCohortTrainer(TinyECG(), x, y, B, S, clients=K, cohort=M, lr=1e-2, momentum=0.9, amp_dtype=None, seed=5,
                              **kw)


DP = dict(client_dp_clip=0.05, client_dp_noise=1.0)


@pytest.mark.parametrize("dp", [{}, DP])
def test_sgdm_without_momentum_is_the_server_lr_close_bitwise(dp):
    plain, sgdm = _trainer(server_lr=0.5, **dp), _trainer(server_lr=0.5, server_opt="sgdm", server_beta1=0.0, **dp)
    assert plain.server_m is None and sgdm.client_dp and torch.equal(sgdm.server_m, torch.zeros(P))
    g0 = _flat(plain.model).clone()
    for _ in range(2):
        plain.run_round(S)
        sgdm.run_round(S)
        assert torch.equal(_flat(plain.model), _flat(sgdm.model))
    assert not torch.equal(_flat(plain.model), g0) and sgdm.server_v is None and sgdm.server_m.abs().max() > 0


def test_sgdm_momentum_adds_eta_b1_m1_in_the_second_round():
    eta, b1 = 0.5, 0.9
    mom = _trainer(server_lr=eta, server_opt="sgdm", server_beta1=b1)
    none = _trainer(server_lr=eta, server_opt="sgdm", server_beta1=0.0)
    mom.run_round(S)
    none.run_round(S)
    g1 = _flat(mom.model).clone()
    assert torch.equal(g1, _flat(none.model))  # m_0 = 0: the first round has no momentum to add
    m1 = mom.server_m.clone()
    assert torch.equal(m1, none.server_m) and m1.abs().max() > 1e-4
    mom.run_round(S)
    none.run_round(S)
    diff = (_flat(mom.model).double() - _flat(none.model).double()).numpy()
    want = _f(eta) * _f(b1) * m1.double().numpy()
    # both runs round b1 m + Delta, eta m and g + eta m once each: 4 EPS32 of the largest term, as test_server_lr_half_...
    bound = 4 * EPS32 * (g1.abs().max().item() + float(np.abs(mom.server_m.numpy()).max()))
    assert np.abs(want).max() > 1e-4 and np.abs(diff - want).max() <= bound, np.abs(diff - want).max() / bound


def test_trainer_argument_checks_and_state():
    with pytest.raises(ValueError, match="unknown server optimizer"):
        _trainer(server_opt="nadam")
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        _trainer(server_opt="adam", server_beta2=1.0)
    with pytest.raises(ValueError, match="server_tau"):
        _trainer(server_opt="adagrad", server_tau=-1.0)
    tr = _trainer(server_opt="yogi", server_tau=0.01)
    assert set(tr.server_state()) == {"server_m", "server_v"} and torch.equal(tr.server_v, torch.full((P,), 0.01) ** 2)
    assert set(_trainer(server_opt="sgdm").server_state()) == {"server_m"} and _trainer().server_state() == {}
    with pytest.raises(ValueError, match="server_m shape"):
        tr.load_server_state({"server_m": torch.zeros(3)})


# ------------------------------------------------------------------------------------------------ 4: the checkpoint
@pytest.mark.parametrize("opt", ["sgdm", "adam"])
def test_checkpoint_round_trip_continues_the_optimizer(opt, tmp_path):
    from crossscale_ecg.utils import ckpt
    kw = dict(server_opt=opt, server_lr=0.05 if opt == "adam" else 0.5, **DP)
    run = _trainer(**kw)
    run.run_round(S)
    path = ckpt.save_rank_state(str(tmp_path), 0, "G0", 0, run)
    weights, run_m1 = _flat(run.model).clone(), run.server_m.clone()
    run.run_round(S)
    want = _flat(run.model)
    st = torch.load(path, map_location="cpu", weights_only=True)
    assert st["cohort_round"] == 1 and torch.equal(st["server_m"], run_m1) and run_m1.abs().max() > 0
    assert ("server_v" in st) == (opt == "adam")

    def resumed(restore):
        tr = _trainer(**kw)
        torch.nn.utils.vector_to_parameters(weights.clone(), tr.model.parameters())
        if restore:
            ckpt.load_trainer_local_state(tr, st)
        else:
            tr.set_cohort_round(1)
        tr.run_round(S)
        return _flat(tr.model)

    assert torch.equal(resumed(True), want)
    assert not torch.equal(resumed(False), want)  # a restarted optimizer takes another step
    assert "server_m" not in ckpt.trainer_local_state(_trainer())  # no optimizer: nothing added to the file


# ------------------------------------------------------------------------------------------------ 5: the driver
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=4, cohort=2, server_opt="sgdm", server_lr=0.7,
                results_csv=os.path.join(tmp, "rounds.csv"), eval_csv=os.path.join(tmp, "eval.csv"),
                privacy_csv=os.path.join(tmp, "privacy.csv"), cohort_csv=os.path.join(tmp, "cohort.csv"),
                client_privacy_csv=os.path.join(tmp, "client_privacy.csv"), ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


class Ctx2(penv.DistContext):  # a rank of 2 initialised ranks, without a process group
    distributed = True


def test_flags_parse_and_are_checked(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (cfg.server_opt, cfg.server_beta1, cfg.server_beta2, cfg.server_tau) == ("none", 0.9, 0.99, 1e-3)
    drv.check_server_opt_config(cfg, _ctx1())  # off: nothing to check
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--server-opt", "yogi", "--server-beta1", "0.8", "--server-beta2",
         "0.95", "--server-tau", "0.01", "--server-lr", "0.1"]))
    assert (cfg.server_opt, cfg.server_beta1, cfg.server_beta2, cfg.server_tau, cfg.server_lr) == ("yogi", 0.8, 0.95, 0.01, 0.1)
    drv.check_server_opt_config(cfg, _ctx1())
    t = str(tmp_path)
    for opt in ("sgdm", "adagrad", "adam", "yogi"):  # rejected without client sampling
        with pytest.raises(ValueError, match="--clients-per-gpu"):
            drv.check_server_opt_config(_cfg(t, clients_per_gpu=1, cohort=0, server_opt=opt), _ctx1())
    with pytest.raises(ValueError, match="--clients-per-gpu"):
        drv.run_fedavg(_cfg(t, clients_per_gpu=1, cohort=0, server_lr=1.0), _ctx1())
    with pytest.raises(ValueError, match="unknown server optimizer"):
        drv.check_server_opt_config(_cfg(t, server_opt="lamb"), _ctx1())
    for kw in (dict(server_beta1=1.0), dict(server_beta2=-0.1), dict(server_opt="adam", server_beta2=1.5)):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    with pytest.raises(ValueError, match="server_tau"):
        drv.run_fedavg(_cfg(t, server_opt="adagrad", server_tau=0.0), _ctx1())
    # the adaptive rules under --sync fedavg on two ranks: rejected, with the reason; sgdm, --sync none and one rank pass
    ctx2 = Ctx2(0, 2, 0, "gloo", torch.device("cpu"))
    for opt in ("adagrad", "adam", "yogi"):
        with pytest.raises(ValueError, match="nonlinear in the averaged delta"):
            drv.check_server_opt_config(_cfg(t, server_opt=opt), ctx2)
        drv.check_server_opt_config(_cfg(t, server_opt=opt, sync="none"), ctx2)
        drv.check_server_opt_config(_cfg(t, server_opt=opt), _ctx1())
    drv.check_server_opt_config(_cfg(t, server_opt="sgdm"), ctx2)
    x, y = torch.randn(256, 64), torch.zeros(256, dtype=torch.long)
    with pytest.raises(ValueError, match="nonlinear"):
        drv.make_trainer(_cfg(t, server_opt="adam"), "G0", TinyECG(), x, y, ctx2, "torch")
    tr = drv.make_trainer(_cfg(t, server_opt="adam", sync="none", server_tau=0.01), "G0", TinyECG(), x, y, ctx2, "torch")
    assert (tr.server_opt, tr.server_beta1, tr.server_beta2, tr.server_tau, tr.server_lr) == ("adam", 0.9, 0.99, 0.01, 0.7)
    # every combination client sampling rejects stays rejected with a server optimizer on
    for kw, match in ((dict(dp_clip=1.0), "--dp-clip"), (dict(sync="ddp"), "--sync ddp"),
                      (dict(drop_prob=0.1), "--drop-prob"), (dict(overlap="delayed"), "--overlap delayed"),
                      (dict(model="resnet1d"), "ResNet1D")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv"))


def test_driver_world1_resume_continues_the_optimizer(tmp_path):
    """Three rounds in one run against two rounds, a checkpoint, and --resume for the third: the same weights bitwise,
    and the optimizer is logged once per configuration."""
    import json
    from crossscale_ecg.train import fedavg as drv

    def run(tmp, **kw):
        kept = []
        real = drv.make_trainer
        drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
        try:
            drv.run_fedavg(_cfg(tmp, server_opt="adam", server_lr=0.05, **kw), _ctx1())
        finally:
            drv.make_trainer = real
        return kept[0]

    whole = run(str(tmp_path / "a"), jsonl=str(tmp_path / "a.jsonl"))
    events = [json.loads(line) for line in open(tmp_path / "a.jsonl")]
    so = [e for e in events if e["event"] == "server_opt"]
    assert len(so) == 1 and (so[0]["server_opt"], so[0]["beta1"], so[0]["beta2"], so[0]["tau"], so[0]["server_lr"]) == \
        ("adam", 0.9, 0.99, 1e-3, 0.05)
    t = str(tmp_path / "b")
    run(t, rounds=2, ckpt_every=1)
    part = run(t, rounds=3, ckpt_every=1, resume=True)
    assert part.cohort_round == 3 and torch.equal(_flat(part.model), _flat(whole.model))
    assert torch.equal(part.server_m, whole.server_m) and torch.equal(part.server_v, whole.server_v)


# ------------------------------------------------------------------------------------------------ 3: gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    penv._CTX = None
    torch.set_num_threads(1)
    try:
        from crossscale_ecg.train import fedavg as drv
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        kept = []
        real = drv.make_trainer

        def spy(*a):
            kept.append(real(*a))
            return kept[-1]

        drv.make_trainer = spy
        drv.run_fedavg(_cfg(tmp), ctx)
        tr = kept[0]
        q.put((rank, "ok", (_flat(tr.model).tolist(), tr.server_m.tolist())))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def _global_fedavgm(tmp, world, rounds):
    """Global FedAvgM in one process, in float64: per round every rank's plain cohort mean from the global weights (the
    driver's trainers, data and seeds, no server optimizer), Delta = mean over ranks of (mean_k - g), m = b1 m + Delta,
    g += eta m.  Returns (g, m)."""
    from crossscale_ecg.models import build_model
    from crossscale_ecg.train import fedavg as drv
    cfg = _cfg(tmp, server_opt="none", server_lr=1.0)
    eta, b1 = _f(0.7), _f(0.9)
    trainers = []
    for k in range(world):
        ctx = Ctx2(k, world, k, "gloo", torch.device("cpu"))
        x, y = drv.load_client_data(cfg, ctx)
        torch.manual_seed(cfg.seed)
        model = build_model(cfg.model, cfg.num_classes)
        trainers.append(drv.make_trainer(cfg, "G0", model, x, y, ctx, "torch"))
    g = _flat(trainers[0].model).double()
    m = torch.zeros_like(g)
    for _ in range(rounds):
        delta = torch.zeros_like(g)
        for tr in trainers:
            torch.nn.utils.vector_to_parameters(g.float(), tr.model.parameters())
            tr.run_round(cfg.local_steps)
            delta += (_flat(tr.model).double() - g.float().double()) / world
        m = b1 * m + delta
        g = g + eta * m
    return g, m


def test_gloo_world2_sgdm_is_global_fedavgm(tmp_path):
    """Each rank keeps its own m_rank; the all-reduce(AVG) of g + eta m_rank is g + eta AVG(m_rank), and AVG(m_rank)
    obeys m = b1 m + AVG(Delta_rank): global FedAvgM.  Relative l2 bound 1e-5, the project's fp32 bound."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    want_g, want_m = _global_fedavgm(str(tmp_path / "emu"), world, 3)  # (while the ranks run)
    out = {}
    for _ in range(world):
        rank, status, res = q.get(timeout=240)
        assert status == "ok", res
        out[rank] = res
    for p in ps:
        p.join(timeout=60)
    assert out[0][0] == out[1][0] and len(out[0][0]) == P  # FedAvg leaves the same global weights on both ranks
    assert out[0][1] != out[1][1]  # ... from different per-rank momenta
    got = torch.tensor(out[0][0], dtype=torch.float64)
    m_avg = (torch.tensor(out[0][1], dtype=torch.float64) + torch.tensor(out[1][1], dtype=torch.float64)) / 2
    rel = ((got - want_g).norm() / want_g.norm()).item()
    rel_m = ((m_avg - want_m).norm() / want_m.norm()).item()
    torch.manual_seed(1234)
    moved = ((want_g - _flat(TinyECG()).double()).norm() / want_g.norm()).item()
    print(f"gloo world 2, sgdm vs global FedAvgM after 3 rounds: weights rel l2 {rel:.3e}, AVG(m_rank) rel l2 {rel_m:.3e} "
          f"(update {moved:.3e})")
    assert rel < 1e-5 and moved > 1e-3
    # m is a sum of differences p - g of fp32 weights: its error is relative to |g|, (cohort + 8) roundings per round
    # (the bound of the DP close's tests), not to |m|
    assert (m_avg - want_m).norm().item() <= 3 * (2 + 8) * EPS32 * want_g.norm().item()
