"""Global server optimizers on cohort rounds (``--server-scope global``), on the CPU: ``TorchCohortTrainer`` scope
"global" against scope "rank", ``FedAvgRound(on_averaged=...)``, the flags, and the driver - two gloo ranks against a
one-process emulation and against global FedAdam / FedYogi / FedAvgM in float64, ``--overlap tail`` against ``none``
with the order of wait, step and launch, ``--resume`` at world 1, and the noise share under client-level DP.

Under scope "global" a cohort round ends with the rank's averaged client delta; the driver all-reduces(AVG) the ranks'
deltas in place of their weights and every rank takes the same server step (train/server_opt.py) on the average."""
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
CLOSES = (("none", 0.7), ("sgdm", 0.7), ("adagrad", 0.05), ("adam", 0.05), ("yogi", 0.05))


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _f(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ 1: the trainer
B, S, K, M, L, N = 5, 3, 4, 3, 64, 48
DP = dict(client_dp_clip=0.05, client_dp_noise=1.0)


def _trainer(**kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(N, L, generator=g), torch.randint(0, 2, (N,), generator=g)
    torch.manual_seed(0)
    return TorchCohortTrainer(TinyECG(), x, y, B, S, clients=K, cohort=M, lr=1e-2, momentum=0.9, amp_dtype=None, seed=5,
                              **kw)


@pytest.mark.parametrize("dp", [{}, DP])
@pytest.mark.parametrize("opt,eta", CLOSES)
def test_torch_trainer_scope_global_equals_scope_rank_bitwise(opt, eta, dp):
    rank = _trainer(server_opt=opt, server_lr=eta, **dp)
    glob = _trainer(server_opt=opt, server_lr=eta, server_scope="global", **dp)
    assert rank.server_delta is None and glob.server_delta.shape == (P,) and glob.client_dp
    g0 = _flat(rank.model).clone()
    for rnd in range(2):
        rank.run_round(S)
        held = _flat(glob.model).clone()
        buf = glob.server_delta
        glob.prepare_round(S)
        glob.launch_round(S)  # ends with the delta; the model, m and v are as they were
        assert torch.equal(_flat(glob.model), held) and glob.server_delta is buf and float(buf.abs().max()) > 0
        assert not torch.equal(_flat(glob.model), _flat(rank.model))
        glob.apply_server_step()
        assert torch.equal(_flat(glob.model), _flat(rank.model)), rnd
        for u, v in ((rank.server_m, glob.server_m), (rank.server_v, glob.server_v)):
            assert (u is None and v is None) or torch.equal(u, v)
        assert glob.round_clients == rank.round_clients and glob.last_clip_stats() == rank.last_clip_stats()
    assert not torch.equal(_flat(rank.model), g0)
    both = _trainer(server_opt=opt, server_lr=eta, server_scope="global", **dp)
    both.run_round(S)
    both.run_round(S)  # run_round takes both halves
    assert torch.equal(_flat(both.model), _flat(rank.model))
    with pytest.raises(RuntimeError, match="server_scope"):
        rank.apply_server_step()
    with pytest.raises(ValueError, match="unknown server scope"):
        _trainer(server_scope="node")


# ------------------------------------------------------------------------------------------------ 2: on_averaged
def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


def test_fedavg_round_on_averaged_runs_once_per_collective():
    from crossscale_ecg.parallel.overlap import CommRecord, FedAvgComm, FedAvgRound
    comm, flat, calls = FedAvgComm(_ctx1()), torch.zeros(4), []
    fr = FedAvgRound(flat, comm, "none", on_averaged=lambda: calls.append("avg"))
    fr.end_round(CommRecord())
    assert calls == ["avg"]
    fr.begin_round(prep=lambda: calls.append("prep"))
    fr.finalize()
    assert calls == ["avg", "prep"]  # nothing was in flight
    calls.clear()
    fr = FedAvgRound(flat, comm, "tail", on_averaged=lambda: calls.append("avg"))
    fr.end_round(CommRecord())
    assert calls == [] and fr.in_flight
    fr.begin_round(prep=lambda: calls.append("prep"))
    assert calls == ["prep", "avg"] and not fr.in_flight  # after prep, right after the wait
    fr.begin_round(prep=lambda: calls.append("prep"))
    assert calls == ["prep", "avg", "prep"]
    fr.end_round(CommRecord())
    fr.finalize()
    fr.finalize()
    assert calls == ["prep", "avg", "prep", "avg"]
    for mode in ("none", "tail"):  # None: nothing changes
        fr = FedAvgRound(flat, comm, mode)
        fr.end_round(CommRecord())
        fr.begin_round()
        fr.finalize()
    with pytest.raises(ValueError, match="delayed"):
        FedAvgRound(flat, comm, "delayed", on_averaged=lambda: None)


# ------------------------------------------------------------------------------------------------ 3: the flags
def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=4, cohort=2, server_opt="adam", server_lr=0.05,
                server_scope="global", results_csv=os.path.join(tmp, "rounds.csv"),
                eval_csv=os.path.join(tmp, "eval.csv"), privacy_csv=os.path.join(tmp, "privacy.csv"),
                cohort_csv=os.path.join(tmp, "cohort.csv"), client_privacy_csv=os.path.join(tmp, "client_privacy.csv"),
                ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


class Ctx2(penv.DistContext):  # a rank of 2 initialised ranks, without a process group
    distributed = True


def test_flags_parse_and_are_checked(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    from crossscale_ecg.train.cohort import client_dp_nu
    assert from_args(FedAvgConfig, entry.build_parser().parse_args([])).server_scope == "rank"
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--server-opt", "yogi", "--server-scope", "global"]))
    assert (cfg.server_opt, cfg.server_scope) == ("yogi", "global")
    t = str(tmp_path)
    ctx2 = Ctx2(0, 2, 0, "gloo", torch.device("cpu"))
    for opt in ("adagrad", "adam", "yogi"):
        with pytest.raises(ValueError, match="nonlinear in the averaged delta"):  # the default still rejects
            drv.check_server_opt_config(_cfg(t, server_opt=opt, server_scope="rank"), ctx2)
        drv.check_server_opt_config(_cfg(t, server_opt=opt), ctx2)  # --server-scope global passes
        drv.check_server_opt_config(_cfg(t, server_opt=opt), _ctx1())
        drv.check_server_opt_config(_cfg(t, server_opt=opt, sync="none"), ctx2)
    for opt in ("none", "sgdm"):
        drv.check_server_opt_config(_cfg(t, server_opt=opt), ctx2)
    for opt in ("none", "adam"):  # global without client sampling
        with pytest.raises(ValueError, match="--server-scope global needs client sampling .--clients-per-gpu"):
            drv.check_server_opt_config(_cfg(t, server_opt=opt, clients_per_gpu=1, cohort=0), _ctx1())
    with pytest.raises(ValueError, match="--clients-per-gpu"):
        drv.run_fedavg(_cfg(t, server_opt="none", server_lr=1.0, clients_per_gpu=1, cohort=0), _ctx1())
    with pytest.raises(ValueError, match="unknown server scope"):
        drv.check_server_opt_config(_cfg(t, server_scope="node"), _ctx1())
    drv.check_server_opt_config(_cfg(t, server_opt="none", server_scope="rank", clients_per_gpu=1, cohort=0), _ctx1())
    x, y = torch.randn(256, 64), torch.zeros(256, dtype=torch.long)
    with pytest.raises(ValueError, match="nonlinear"):
        drv.make_trainer(_cfg(t, server_scope="rank"), "G0", TinyECG(), x, y, ctx2, "torch")
    tr = drv.make_trainer(_cfg(t), "G0", TinyECG(), x, y, ctx2, "torch")
    assert (tr.server_opt, tr.server_scope, tr.server_lr) == ("adam", "global", 0.05) and tr.server_delta is not None
    # client-level DP at world 2 under scope global: every rank still adds sigma / sqrt(2) of the noise - the average
    # of 2 deltas with that share each has the noise the accountant assumes
    cfg = _cfg(t, client_dp_clip=0.05, client_dp_noise=1.0)
    assert drv.client_dp_world(cfg, ctx2) == 2 and drv.client_dp_world(cfg, _ctx1()) == 1
    tr = drv.make_trainer(cfg, "G0", TinyECG(), x, y, ctx2, "torch")
    assert tr.cdp_nu == client_dp_nu(1.0, 0.05, 2, 2) == _f(1.0 / 2 ** 0.5 * 0.05 / 2)
    # every combination client sampling rejects stays rejected under scope global
    for kw, match in ((dict(dp_clip=1.0), "--dp-clip"), (dict(sync="ddp"), "--sync ddp"),
                      (dict(drop_prob=0.1), "--drop-prob"), (dict(overlap="delayed"), "--overlap delayed"),
                      (dict(model="resnet1d"), "ResNet1D")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv"))


# ------------------------------------------------------------------------------------------------ 4: resume
def _run_world1(tmp, **kw):
    from crossscale_ecg.train import fedavg as drv
    kept = []
    real = drv.make_trainer
    drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
    try:
        drv.run_fedavg(_cfg(tmp, **kw), _ctx1())
    finally:
        drv.make_trainer = real
    return kept[0]


def test_driver_world1_resume_and_scope_rank_bitwise(tmp_path):
    """Three rounds in one run against one round, a checkpoint, and --resume for the other two: the same weights, m
    and v bitwise; without a collective the step follows the round at once, so the run also ends on the bits of scope
    "rank"; the server_opt event carries the scope."""
    import json
    whole = _run_world1(str(tmp_path / "a"), jsonl=str(tmp_path / "a.jsonl"))
    so = [e for e in map(json.loads, open(tmp_path / "a.jsonl")) if e["event"] == "server_opt"]
    assert len(so) == 1 and (so[0]["server_opt"], so[0]["scope"]) == ("adam", "global")
    t = str(tmp_path / "b")
    first = _run_world1(t, rounds=1, ckpt_every=1)
    assert first.cohort_round == 1
    part = _run_world1(t, rounds=3, ckpt_every=1, resume=True)
    rank = _run_world1(str(tmp_path / "c"), server_scope="rank")
    start = _flat(TinyECG())
    for other in (part, rank):
        assert other.cohort_round == 3 and torch.equal(_flat(other.model), _flat(whole.model))
        assert torch.equal(other.server_m, whole.server_m) and torch.equal(other.server_v, whole.server_v)
    assert float(whole.server_m.abs().max()) > 0 and _flat(whole.model).shape == start.shape


# ------------------------------------------------------------------------------------------------ 5: gloo world 2
RUNS = {  # name -> configuration overrides of one driver run on two gloo ranks
    "adam": dict(server_opt="adam"),
    "yogi": dict(server_opt="yogi"),
    "adam_tail": dict(server_opt="adam", overlap="tail", bcast_every_round=False),
    "sgdm": dict(server_opt="sgdm", server_lr=0.7),
    "sgdm_rank": dict(server_opt="sgdm", server_lr=0.7, server_scope="rank"),
}


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
    try:
        from crossscale_ecg.parallel import overlap
        from crossscale_ecg.train import fedavg as drv
        drv.usable_cpus = lambda: 1  # the driver sizes torch's thread pool by it: one thread, one summation order
        torch.set_num_threads(1)
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        events, kept = [], []
        real_make, real_wait = drv.make_trainer, overlap.FedAvgComm.wait

        def spy(*a):
            tr = real_make(*a)
            for name, tag in (("prepare_round", "prep"), ("launch_round", "launch"), ("apply_server_step", "step")):
                fn = getattr(tr, name, None)
                if fn is not None:
                    setattr(tr, name, lambda *b, _fn=fn, _tag=tag, **k: events.append(_tag) or _fn(*b, **k))
            kept.append(tr)
            return tr

        def wait(self, pendings, rec):
            if any(not p.waited for p in pendings):
                events.append("wait")
            return real_wait(self, pendings, rec)

        drv.make_trainer, overlap.FedAvgComm.wait = spy, wait
        out = {}
        for name, kw in RUNS.items():
            del events[:], kept[:]
            drv.run_fedavg(_cfg(os.path.join(tmp, name), **kw), ctx)
            tr = kept[0]
            out[name] = (_flat(tr.model).tolist(), tr.server_m.tolist(),
                         None if tr.server_v is None else tr.server_v.tolist(), list(events))
        q.put((rank, "ok", out))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def _rank_trainers(tmp, world, **kw):
    """The driver's trainers of all ranks in this process (its data, seeds and initial weights, no process group)."""
    from crossscale_ecg.models import build_model
    from crossscale_ecg.train import fedavg as drv
    cfg = _cfg(tmp, **kw)
    trainers = []
    for k in range(world):
        ctx = Ctx2(k, world, k, "gloo", torch.device("cpu"))
        x, y = drv.load_client_data(cfg, ctx)
        torch.manual_seed(cfg.seed)
        model = build_model(cfg.model, cfg.num_classes)
        trainers.append(drv.make_trainer(cfg, "G0", model, x, y, ctx, "torch"))
    return cfg, trainers


def _emulate_fp32(tmp, world, rounds, **kw):
    """The driver's procedure in one process, in fp32: per round every rank's ``launch_round``, the deltas averaged as
    (d0 + d1) / 2 into every rank's ``server_delta``, every rank's ``apply_server_step``.  (weights, m, v) of rank 0."""
    cfg, trainers = _rank_trainers(tmp, world, **kw)
    for _ in range(rounds):
        for tr in trainers:
            tr.prepare_round(cfg.local_steps)
            tr.launch_round(cfg.local_steps)
        avg = (trainers[0].server_delta + trainers[1].server_delta) / 2
        for tr in trainers:
            tr.server_delta.copy_(avg)
            tr.apply_server_step()
    for tr in trainers[1:]:
        assert torch.equal(_flat(tr.model), _flat(trainers[0].model))
    return _flat(trainers[0].model), trainers[0].server_m, trainers[0].server_v


def _global_fedopt64(tmp, world, rounds, opt, eta, tau=1e-3):
    """Global FedAvgM / FedAdam / FedYogi in one process, in float64: per round every rank's plain cohort mean from the
    global weights (the driver's trainers, data and seeds; no server step of their own), Delta = mean over ranks of
    (mean_k - g), then the rule of train/server_opt.py written out with the fp32 constants.  Returns (g, m, v)."""
    cfg, trainers = _rank_trainers(tmp, world, server_opt="none", server_lr=1.0, server_scope="rank")
    eta, b1, b2, tau = _f(eta), _f(0.9), _f(0.99), _f(tau)
    g = _flat(trainers[0].model).double()
    m = torch.zeros_like(g)
    v = torch.full_like(g, tau * tau)
    for _ in range(rounds):
        d = torch.zeros_like(g)
        for tr in trainers:
            torch.nn.utils.vector_to_parameters(g.float(), tr.model.parameters())
            tr.run_round(cfg.local_steps)
            d += (_flat(tr.model).double() - g.float().double()) / world
        if opt == "sgdm":
            m = b1 * m + d
            g = g + eta * m
            continue
        m = b1 * m + (1.0 - b1) * d
        if opt == "adam":
            v = b2 * v + (1.0 - b2) * d * d
        else:  # yogi
            v = v - (1.0 - b2) * d * d * torch.sign(v - d * d)
        g = g + eta * m / (torch.sqrt(v) + tau)
    return g, m, v


@pytest.fixture(scope="module")
def gloo_runs(tmp_path_factory):
    """Every driver run of ``RUNS`` on two gloo ranks, once: {name: {rank: (weights, m, v, events)}}."""
    tmp = str(tmp_path_factory.mktemp("gloo"))
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, tmp, q)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    for _ in range(world):
        rank, status, res = q.get(timeout=300)
        assert status == "ok", res
        got[rank] = res
    for p in ps:
        p.join(timeout=60)
    return {name: {r: got[r][name] for r in range(world)} for name in RUNS}


def _t(lst):
    return torch.tensor(lst, dtype=torch.float32)


@pytest.mark.parametrize("opt", ["adam", "yogi"])
def test_gloo_world2_adaptive_rules_are_global(opt, gloo_runs, tmp_path):
    """Both ranks hold identical weights, m and v; they are the bits of the one-process fp32 emulation; and that
    emulation is within 1e-5 relative l2 (the project's fp32 bound) of global FedAdam / FedYogi in float64.  tau is the
    default 1e-3: the float64 comparison measures 1.9e-7 for both rules there, so it was not raised to 0.01."""
    run = gloo_runs[opt]
    for i in range(3):
        assert run[0][i] == run[1][i] and len(run[0][i]) == P, i
    prev = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        w, m, v = _emulate_fp32(str(tmp_path / "emu"), 2, 3, **RUNS[opt])
        g64, m64, v64 = _global_fedopt64(str(tmp_path / "ref"), 2, 3, opt, 0.05)
    finally:
        torch.set_num_threads(prev)
    assert torch.equal(_t(run[0][0]), w) and torch.equal(_t(run[0][1]), m) and torch.equal(_t(run[0][2]), v)
    rel = ((w.double() - g64).norm() / g64.norm()).item()
    rel_m = ((m.double() - m64).norm() / m64.norm()).item()
    rel_v = ((v.double() - v64).norm() / v64.norm()).item()
    torch.manual_seed(1234)
    moved = ((g64 - _flat(TinyECG()).double()).norm() / g64.norm()).item()
    print(f"gloo world 2, {opt}, scope global vs float64 global rule after 3 rounds: weights rel l2 {rel:.3e}, m {rel_m:.3e}, "
          f"v {rel_v:.3e} (update {moved:.3e})")
    assert rel < 1e-5 and moved > 1e-3


def test_gloo_world2_sgdm_global_m_is_the_average_of_the_rank_momenta(gloo_runs, tmp_path):
    """Scope global: one m, identical on both ranks.  Scope rank: every rank its own m_rank, and AVG(m_rank) obeys the
    same recurrence on AVG(Delta_rank).  The two agree within 3 (M + 8) 2^-23 |g| (M = 2 clients per cohort; the bound of
    the scope-rank sgdm test: m is a sum of differences of fp32 weights, (M + 8) roundings per round, 3 rounds)."""
    glob, rank = gloo_runs["sgdm"], gloo_runs["sgdm_rank"]
    assert glob[0][1] == glob[1][1] and glob[0][0] == glob[1][0] and glob[0][2] is None
    assert rank[0][1] != rank[1][1] and rank[0][0] == rank[1][0]
    m_avg = (_t(rank[0][1]).double() + _t(rank[1][1]).double()) / 2
    m = _t(glob[0][1]).double()
    g = _t(glob[0][0]).double()
    err = (m - m_avg).norm().item()
    bound = 3 * (2 + 8) * EPS32 * g.norm().item()
    g64, m64, _ = _global_fedopt64(str(tmp_path / "ref"), 2, 3, "sgdm", 0.7)
    rel = ((g - g64).norm() / g64.norm()).item()
    print(f"gloo world 2, sgdm: |m_global - AVG(m_rank)| {err:.3e} (bound {bound:.3e}); weights vs float64 FedAvgM {rel:.3e}")
    assert err <= bound and m.norm().item() > 100 * bound
    assert rel < 1e-5
    assert ((g - _t(rank[0][0]).double()).norm() / g.norm()).item() < 1e-5  # the two scopes are the same algorithm


def test_gloo_world2_overlap_tail_ends_on_the_bits_of_none(gloo_runs):
    none, tail = gloo_runs["adam"], gloo_runs["adam_tail"]
    for r in (0, 1):
        for i in range(3):
            assert tail[r][i] == none[0][i], (r, i)
        # none: the wait and the step close every round.  tail: the collective stays in flight under the next round's
        # batch preparation; the step follows the wait and precedes the launch; the last one is drained by finalize()
        assert none[r][3] == ["prep", "launch", "wait", "step"] * 3
        assert tail[r][3] == ["prep", "launch"] + ["prep", "wait", "step", "launch"] * 2 + ["wait", "step"]
