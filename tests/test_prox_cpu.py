"""FedProx and label-skewed clients on the CPU: ``TorchLocalTrainer`` / ``TorchCohortTrainer`` with ``prox_mu`` against
a float64 loop of the definition (the gradient that enters SGD is ``g + wd * p + mu * (p - a)``, ``a`` the weights the
round started from), ``shard_partition``, ``CohortSampler(order=...)``, and the driver's flags on the torch backend: one
process and two gloo ranks, ``--resume``, the ``prox`` event, the CSV schemas and every rejected combination."""
import copy
import csv
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F

import crossscale_ecg  # noqa: F401
from crossscale_ecg.config import FedAvgConfig
from crossscale_ecg.models.tiny_ecg import TinyECG
from crossscale_ecg.parallel import env as penv

# lr and mu are large on purpose: the proximal term is zero in a round's first step (p == a) and enters the second
# step's weights as lr * mu * (p_1 - a) ~ lr^2 * mu * |d|, which these values keep far above the comparison's bound
LR, MOM, WD, MU = 0.1, 0.9, 1e-2, 2.0
B, S, L, N = 8, 2, 64, 96
# fp32 trainer against the float64 loop, relative l2 of the weights: every weight is rounded once per step (2^-24 each,
# two steps) and the update lr * (1 + momentum) * d carries the fp32 gradient's error, a few 1e-6 of |d| <~ |p|: below
# 2 * 6e-8 + 0.2 * 1e-5 < 3e-6
TOL = 3e-6


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _data(seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, L, generator=g)
    return x, (x.mean(1) > 0).long()


def _sgd64(model, x, y, batches, mu, mom=MOM):
    """``len(batches)`` SGD steps from zero momentum on a float64 copy of ``model``, anchored on its weights: the
    definition written out.  Returns the flat weights."""
    m64 = copy.deepcopy(model).double()
    if getattr(m64, "_flat", None) is not None:
        m64._flat = None
    ps = list(m64.parameters())
    a = [p.detach().clone() for p in ps]
    bufs = [torch.zeros_like(p) for p in ps]
    m64.train()
    for sel in batches:
        loss = F.cross_entropy(m64(x[sel].double().unsqueeze(1)), y[sel])
        grads = torch.autograd.grad(loss, ps)
        with torch.no_grad():
            for p, g, buf, a_ in zip(ps, grads, bufs, a):
                d = g + WD * p + mu * (p - a_)
                buf.mul_(mom).add_(d)
                p.sub_(LR * buf)
    return _flat(m64)


def _rel(got, want):
    return ((got.double() - want).norm() / want.norm()).item()


class _Replay:
    def __init__(self, table):
        self.table, self.i = table, 0

    def fill(self, out):
        out.copy_(self.table[self.i:self.i + out.shape[0]])
        self.i += out.shape[0]
        return out


# ------------------------------------------------------------------------------------------------ 1: the trainers
def _local(mu, **kw):
    from crossscale_ecg.train.local import TorchLocalTrainer
    x, y = _data()
    torch.manual_seed(0)
    model = TinyECG()
    return model, TorchLocalTrainer(model, x, y, B, lr=LR, momentum=MOM, weight_decay=WD, amp_dtype=None, seed=5,
                                    prox_mu=mu, **kw)


def test_torch_local_trainer_against_the_float64_definition():
    x, y = _data()
    table = torch.randint(0, N, (2 * S, B), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    model, tr = _local(MU)
    start = copy.deepcopy(model)
    tr.sampler = _Replay(table)
    tr.run_steps(S)
    want = _sgd64(start, x, y, [table[s].long() for s in range(S)], MU)
    plain = _sgd64(start, x, y, [table[s].long() for s in range(S)], 0.0)
    rel, effect = _rel(_flat(model), want), _rel(plain, want)
    print(f"TorchLocalTrainer prox vs float64: rel l2 {rel:.3e} (the proximal term moves the weights by {effect:.3e})")
    assert rel < TOL and effect > 100 * TOL


def test_torch_local_trainer_second_round_against_float64_without_momentum():
    """A second round anchors on the weights it starts from, not on the first round's: with momentum 0 (a local
    trainer's momentum carries over between rounds) it is a fresh run from the first round's weights."""
    from crossscale_ecg.train.local import TorchLocalTrainer
    x, y = _data()
    table = torch.randint(0, N, (2 * S, B), generator=torch.Generator().manual_seed(9)).to(torch.int32)
    torch.manual_seed(0)
    model = TinyECG()
    tr = TorchLocalTrainer(model, x, y, B, lr=LR, momentum=0.0, weight_decay=WD, amp_dtype=None, seed=5, prox_mu=MU)
    tr.sampler = _Replay(table)
    tr.run_steps(S)
    mid = copy.deepcopy(model)
    tr.run_round(S)
    want = _sgd64(mid, x, y, [table[s].long() for s in range(S, 2 * S)], MU, mom=0.0)
    rel = _rel(_flat(model), want)
    print(f"TorchLocalTrainer prox, second round vs float64: rel l2 {rel:.3e}")
    assert rel < TOL


def test_prox_mu_zero_is_todays_result_bitwise():
    outs = []
    for kw in ({}, dict(prox_mu=0.0)):
        from crossscale_ecg.train.local import TorchLocalTrainer
        x, y = _data()
        torch.manual_seed(0)
        model = TinyECG()
        tr = TorchLocalTrainer(model, x, y, B, lr=LR, momentum=MOM, weight_decay=WD, amp_dtype=None, seed=5, **kw)
        tr.run_steps(S)
        tr.run_round(S)
        outs.append(_flat(model).clone())
    assert torch.equal(outs[0], outs[1])
    couts = []
    for kw in ({}, dict(prox_mu=0.0, partition="contiguous", shards_per_client=2)):
        model, tr = _cohort(None, **kw)
        tr.run_round(S)
        tr.run_round(S)
        couts.append((_flat(model).clone(), tr.table.clone()))
    assert torch.equal(couts[0][0], couts[1][0]) and torch.equal(couts[0][1], couts[1][1])


def _cohort(mu, **kw):
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    x, y = _data()
    torch.manual_seed(0)
    model = TinyECG()
    if mu is not None:
        kw["prox_mu"] = mu
    return model, TorchCohortTrainer(model, x, y, B, S, clients=4, cohort=3, lr=LR, momentum=MOM, weight_decay=WD,
                                     amp_dtype=None, seed=5, **kw)


@pytest.mark.parametrize("partition", ["contiguous", "shards"])
def test_torch_cohort_trainer_against_the_float64_definition(partition):
    x, y = _data()
    model, tr = _cohort(MU, partition=partition)
    for rnd in range(2):  # the second round anchors on the first round's mean
        start = copy.deepcopy(model)
        tr.run_round(S)
        ends, plains = [], []
        for j in range(3):
            batches = [tr.table[s, j * B:(j + 1) * B].long() for s in range(S)]
            ends.append(_sgd64(start, x, y, batches, MU))
            plains.append(_sgd64(start, x, y, batches, 0.0))
        want, plain = sum(ends) / 3, sum(plains) / 3
        rel, effect = _rel(_flat(model), want), _rel(plain, want)
        print(f"TorchCohortTrainer prox ({partition}) round {rnd} vs float64: rel l2 {rel:.3e} (effect {effect:.3e})")
        assert rel < TOL and effect > 100 * TOL


def test_trainers_reject_what_fedprox_does_not_support():
    from crossscale_ecg.train.cohort import TorchCohortTrainer
    from crossscale_ecg.train.local import TorchLocalTrainer
    x, y = _data()
    for cls, extra in ((TorchLocalTrainer, ()), (TorchCohortTrainer, (S, 4))):
        with pytest.raises(ValueError, match="prox_mu must be >= 0"):
            cls(TinyECG(), x, y, B, *extra, prox_mu=-0.1)
        with pytest.raises(ValueError, match="fp16 AMP"):
            cls(TinyECG(), x, y, B, *extra, prox_mu=0.1, amp_dtype=torch.float16)
        cls(TinyECG(), x, y, B, *extra, prox_mu=0.0, amp_dtype=torch.float16)  # off: nothing to reject
    with pytest.raises(ValueError, match="DP-SGD"):
        TorchLocalTrainer(TinyECG(), x, y, B, prox_mu=0.1, dp_clip=1.0)
    with pytest.raises(ValueError, match="partition must be one of"):
        TorchCohortTrainer(TinyECG(), x, y, B, S, 4, partition="dirichlet")

    class FakeDDP(torch.nn.parallel.DistributedDataParallel):  # a DDP-wrapped model, without a process group
        def __init__(self, module):
            torch.nn.Module.__init__(self)
            self.module = module

    with pytest.raises(ValueError, match="DistributedDataParallel"):
        TorchLocalTrainer(FakeDDP(TinyECG()), x, y, B, prox_mu=0.1)


# ------------------------------------------------------------------------------------------------ 2: shard_partition
@pytest.mark.parametrize("n_rows,K,s,nc", [(1003, 10, 2, 2), (96, 4, 2, 2), (500, 7, 3, 5), (64, 4, 1, 2)])
def test_shard_partition(n_rows, K, s, nc):
    from crossscale_ecg.data.dataset import shard_partition
    y = torch.randint(0, nc, (n_rows,), generator=torch.Generator().manual_seed(n_rows))
    order = shard_partition(y, K, s, seed=5)
    n = s * (n_rows // (K * s))
    assert order.dtype == torch.int64 and tuple(order.shape) == (K, n)  # every client has exactly n rows
    assert order.unique().numel() == K * n and int(order.min()) >= 0 and int(order.max()) < n_rows  # no row twice
    # each client's rows come from at most s runs of the stable label-sorted order
    pos = torch.empty(n_rows, dtype=torch.int64)
    pos[torch.argsort(y, stable=True)] = torch.arange(n_rows)
    for k in range(K):
        p = pos[order[k]].sort().values
        assert int((p[1:] - p[:-1] != 1).sum()) + 1 <= s, k
    assert int(pos[order].max()) < K * n  # the remainder at the end of the sorted order is unused
    # label skew: a shard is a run of the sorted labels, so at most nc - 1 of the K * s shards hold two labels
    shards = y[order].view(K * s, n // s)
    assert int((shards.min(1).values != shards.max(1).values).sum()) <= nc - 1
    # a pure function of its arguments; another seed deals the shards differently
    assert torch.equal(order, shard_partition(y.clone(), K, s, seed=5))
    if K * s > 2:
        assert any(not torch.equal(order, shard_partition(y, K, s, seed=sd)) for sd in (6, 7, 8))
    with pytest.raises(RuntimeError, match="fewer than"):
        shard_partition(y[:K * s - 1], K, s, seed=5)
    with pytest.raises(ValueError):
        shard_partition(y, 0, s, seed=5)


# ------------------------------------------------------------------------------------------------ 3: CohortSampler
def _table_of_today(n_windows, batch, steps, clients, cohort, seed, r):
    """The table ``CohortSampler.fill`` wrote before it took ``order`` (its lines, kept here as the reference)."""
    from crossscale_ecg.utils.philox import mix64
    n = n_windows // clients
    passes = (steps * batch + n - 1) // n
    round_seed = mix64(seed) ^ int(r)
    g = torch.Generator()
    g.manual_seed(round_seed)
    ids = torch.randperm(clients, generator=g)[:cohort].tolist()
    g = torch.Generator(device="cpu")
    g.manual_seed(mix64(round_seed))
    keys = torch.randint(0, 1 << 62, (cohort, passes, n), generator=g, dtype=torch.int64)
    rows = keys.argsort(dim=2).reshape(cohort, passes * n)[:, : steps * batch]
    rows = rows + (torch.tensor(ids, dtype=torch.int64) * n)[:, None]
    return ids, rows.view(cohort, steps, batch).permute(1, 0, 2).reshape(steps, cohort * batch).to(torch.int32)


def test_cohort_sampler_order():
    from crossscale_ecg.data.dataset import CohortSampler, shard_partition
    K, M, steps = 6, 4, 5  # n = 16 rows per client, 40 drawn per round: more than one pass over a partition
    for sampler in (CohortSampler(N, B, steps, K, M, "cpu", seed=7), CohortSampler(N, B, steps, K, M, "cpu", seed=7, order=None)):
        for r in (0, 1, 5):
            table = torch.zeros((steps, M * B), dtype=torch.int32)
            ids = sampler.fill(r, table)
            want_ids, want = _table_of_today(N, B, steps, K, M, 7, r)
            assert ids == want_ids and torch.equal(table, want)
    y = torch.randint(0, 2, (N,), generator=torch.Generator().manual_seed(1))
    order = shard_partition(y, K, 2, seed=7)
    sampler = CohortSampler(N, B, steps, K, M, "cpu", seed=7, order=order)
    assert sampler.n == order.shape[1] == 16
    seen = set()
    for r in range(4):
        table = torch.zeros((steps, M * B), dtype=torch.int32)
        ids = sampler.fill(r, table)
        assert ids == sampler.clients_of(r) == CohortSampler(N, B, steps, K, M, "cpu", seed=7).clients_of(r)
        for j, k in enumerate(ids):
            rows = table[:, j * B:(j + 1) * B].reshape(-1).long()
            assert bool(torch.isin(rows, order[k]).all()), (r, k)  # every row of client k lies in order[k]
            assert rows[:16].unique().numel() == 16  # a pass over the partition takes every row once
            seen.update(rows.tolist())
        again = torch.zeros_like(table)
        assert sampler.fill(r, again) == ids and torch.equal(again, table)  # stateless
    assert len(seen) > 16 * M  # different clients over the rounds
    with pytest.raises(ValueError, match="order must be int64"):
        CohortSampler(N, B, steps, K, M, "cpu", seed=7, order=order[:3])
    with pytest.raises(ValueError, match="outside"):
        CohortSampler(N, B, steps, K, M, "cpu", seed=7, order=order + N)
    with pytest.raises(RuntimeError, match="per client < batch"):
        CohortSampler(N, B, steps, K, M, "cpu", seed=7, order=order[:, :B - 1])


# ------------------------------------------------------------------------------------------------ 4: the driver
ROUND_COLUMNS_TODAY = ["config", "world_size", "rank", "round_idx", "batch_size", "local_steps", "local_train_ms", "comm_ms",
                       "samples_per_s", "avg_loss", "comm_exposed_ms", "round_wall_ms", "backend", "overlap"]
COHORT_COLUMNS_TODAY = ["config", "world_size", "round_idx", "clients_per_gpu", "cohort", "batch_size",
                        "windows_per_round_per_gpu", "clients_rank0"]


def _cfg(tmp, **kw):
    base = dict(batch_size=8, rounds=3, local_steps=2, config="G0", kernel_backend="torch", synthetic_windows=256,
                labels="parity", win_len=64, quiet=True, clients_per_gpu=4, cohort=2, prox_mu=0.1,
                client_partition="shards", results_csv=os.path.join(tmp, "rounds.csv"),
                eval_csv=os.path.join(tmp, "eval.csv"), privacy_csv=os.path.join(tmp, "privacy.csv"),
                cohort_csv=os.path.join(tmp, "cohort.csv"), client_privacy_csv=os.path.join(tmp, "client_privacy.csv"),
                ckpt_dir=os.path.join(tmp, "ckpt"))
    base.update(kw)
    return FedAvgConfig(**base)


def _ctx1():
    return penv.DistContext(0, 1, 0, "none", torch.device("cpu"))


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


def _header(path):
    with open(path) as f:
        return next(csv.reader(f))


def test_driver_world1_resume_event_and_csv_schemas(tmp_path):
    from crossscale_ecg.utils.csvio import COHORT_COLUMNS, ROUND_COLUMNS
    a = str(tmp_path / "a")
    whole = _run_world1(a, jsonl=str(tmp_path / "a.jsonl"))
    assert (whole.prox_mu, whole.partition, whole.shards_per_client) == (0.1, "shards", 2)
    assert whole.sampler.order is not None and whole.cohort_round == 3
    ev = [e for e in map(json.loads, open(tmp_path / "a.jsonl")) if e["event"] == "prox"]
    assert len(ev) == 1 and (ev[0]["mu"], ev[0]["partition"], ev[0]["shards_per_client"]) == (0.1, "shards", 2)
    assert ROUND_COLUMNS == ROUND_COLUMNS_TODAY == _header(os.path.join(a, "rounds.csv"))
    assert COHORT_COLUMNS == COHORT_COLUMNS_TODAY == _header(os.path.join(a, "cohort.csv"))
    b = str(tmp_path / "b")
    first = _run_world1(b, rounds=1, ckpt_every=1)
    assert first.cohort_round == 1
    part = _run_world1(b, rounds=3, ckpt_every=1, resume=True)
    assert part.cohort_round == 3 and torch.equal(_flat(part.model), _flat(whole.model))
    assert torch.equal(part.sampler.order, whole.sampler.order)
    # the flags act: without the proximal term, and on contiguous clients, the run ends elsewhere
    off = _run_world1(str(tmp_path / "c"), prox_mu=0.0, jsonl=str(tmp_path / "c.jsonl"))
    iid = _run_world1(str(tmp_path / "d"), client_partition="contiguous")
    assert not torch.equal(_flat(off.model), _flat(whole.model)) and not torch.equal(_flat(iid.model), _flat(whole.model))
    assert [e["mu"] for e in map(json.loads, open(tmp_path / "c.jsonl")) if e["event"] == "prox"] == [0.0]
    # no event when both are off; a single client per GPU takes --prox-mu too
    plain = _run_world1(str(tmp_path / "e"), prox_mu=0.0, client_partition="contiguous", jsonl=str(tmp_path / "e.jsonl"))
    assert plain.prox_mu == 0.0 and not [e for e in map(json.loads, open(tmp_path / "e.jsonl")) if e["event"] == "prox"]
    one = _run_world1(str(tmp_path / "f"), clients_per_gpu=1, cohort=0, client_partition="contiguous")
    assert one.prox_mu == 0.1 and one._anchor is not None


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
        from crossscale_ecg.train import fedavg as drv
        drv.usable_cpus = lambda: 1
        torch.set_num_threads(1)
        ctx = penv.init_distributed(backend="gloo", prefer_gpu=False)
        kept = []
        real = drv.make_trainer
        drv.make_trainer = lambda *a: kept.append(real(*a)) or kept[-1]
        drv.run_fedavg(_cfg(os.path.join(tmp, "w2")), ctx)
        tr = kept[0]
        q.put((rank, "ok", (_flat(tr.model).tolist(), tr.sampler.order.tolist(), tr.prox_mu)))
    except Exception:  # pragma: no cover - reported to the parent
        import traceback
        q.put((rank, "err", traceback.format_exc()))
    finally:
        penv.shutdown_distributed()


def test_driver_gloo_world2_weights_identical_on_both_ranks(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    for p in ps:
        p.start()
    got = {}
    for _ in range(world):
        rank, status, res = q.get(timeout=300)
        assert status == "ok", res
        got[rank] = res
    for p in ps:
        p.join(timeout=60)
    assert got[0][0] == got[1][0] and len(got[0][0]) == 1458
    assert got[0][1] != got[1][1]  # every rank deals its own windows by its own seed
    assert got[0][2] == got[1][2] == 0.1
    torch.manual_seed(1234)
    assert got[0][0] != _flat(TinyECG()).tolist()


class Ctx2(penv.DistContext):  # a rank of 2 initialised ranks, without a process group
    distributed = True


def test_flags_parse_and_every_rejected_combination_raises_with_its_reason(tmp_path):
    import part3_fedavg_overlap_mpi_gpu as entry
    from crossscale_ecg.config import from_args
    from crossscale_ecg.train import fedavg as drv
    d = from_args(FedAvgConfig, entry.build_parser().parse_args([]))
    assert (d.prox_mu, d.client_partition, d.client_shards) == (0.0, "contiguous", 2)
    cfg = from_args(FedAvgConfig, entry.build_parser().parse_args(
        ["--clients-per-gpu", "64", "--cohort", "8", "--prox-mu", "0.01", "--client-partition", "shards",
         "--client-shards", "3"]))
    assert (cfg.prox_mu, cfg.client_partition, cfg.client_shards) == (0.01, "shards", 3)
    t = str(tmp_path)
    plain = dict(clients_per_gpu=1, cohort=0, client_partition="contiguous")
    for kw, backend, cname, match in (
            (dict(prox_mu=-0.1), "torch", "G0", "--prox-mu must be >= 0"),
            (dict(model="resnet1d34", **plain), "hip", "G1", "not for the ResNet1D engine"),
            (dict(sync="ddp", **plain), "torch", "G0", "does not support --sync ddp"),
            (dict(sync="ddp", **plain), "fused", "G1", "does not support --sync ddp"),
            (dict(dp_clip=1.0, **plain), "fused", "G1", "does not support DP-SGD"),
            (dict(amp_dtype="fp16", **plain), "torch", "G1", "does not support fp16 AMP"),
            (dict(overlap="delayed", **plain), "fused", "G1", "does not support --overlap delayed"),
            (dict(client_partition="dirichlet"), "torch", "G0", "--client-partition must be one of"),
            (dict(client_shards=0), "torch", "G0", "--client-shards must be >= 1"),
            (dict(clients_per_gpu=1, cohort=0), "torch", "G0", "need client sampling"),
            (dict(clients_per_gpu=1, cohort=0, client_partition="contiguous", client_shards=3), "torch", "G0",
             "need client sampling")):
        with pytest.raises(ValueError, match=match):
            drv.check_prox_config(_cfg(t, **kw), cname, backend)
    # accepted: TinyECG fused with and without client sampling, any model on the torch backend, fp16 in the fp32 config
    for kw, backend, cname in ((dict(), "fused", "G1"), (plain, "fused", "G0"), (dict(model="resnet1d34", **plain), "torch", "G1"),
                               (dict(amp_dtype="fp16", **plain), "torch", "G0"), (dict(prox_mu=0.0, sync="ddp", **plain), "torch", "G0"),
                               (dict(server_opt="adam", server_scope="global", client_dp_clip=0.1), "fused", "G1")):
        drv.check_prox_config(_cfg(t, **kw), cname, backend)
    # the driver stops before any configuration trains
    for kw, match in ((dict(prox_mu=-1.0), "--prox-mu"), (dict(dp_clip=1.0, **plain), "--dp-clip"),
                      (dict(sync="ddp", **plain), "--sync ddp"), (dict(overlap="delayed", **plain), "--overlap delayed"),
                      (dict(config="G1", amp_dtype="fp16", **plain), "fp16 AMP"),
                      (dict(clients_per_gpu=1, cohort=0), "--clients-per-gpu")):
        with pytest.raises(ValueError, match=match):
            drv.run_fedavg(_cfg(t, **kw), _ctx1())
    assert not os.path.exists(os.path.join(t, "rounds.csv"))
    x, y = torch.randn(256, 64), torch.zeros(256, dtype=torch.long)
    x[:128] += 1.0
    y[:128] = 1
    tr = drv.make_trainer(_cfg(t), "G0", TinyECG(), x, y, Ctx2(1, 2, 1, "gloo", torch.device("cpu")), "torch")
    assert (tr.prox_mu, tr.partition) == (0.1, "shards") and tuple(tr.sampler.order.shape) == (4, 64)
